// Fused paired training-input augmentation: crop + the eight symmetries of the square (two flips and a transpose) +
// stain jitter in optical-density space + to_tensor + Normalize, for source, target and class mask in one pass over the
// bytes.  DESIGN.md section 3.20.
//
//   s2s_paired_augment     uint8 source / target (HWC RGB) and an optional uint8 mask -> fp32 NCHW network inputs, the mask
//                          as fp32 / uint8 / int64, optionally the augmented uint8 images
//   s2s_stain_augment_u8   the stain map alone on uint8 [B][H][W][3]; uint8 HWC or fp32 NCHW out
//
// Geometry.  params int32 [B][4 | 5] = (top, left, hflip, vflip[, transpose]) on the device.  With
//   f[a][b] = img[n][top + (vflip ? S-1-a : a)][left + (hflip ? S-1-b : b)]       out[y][x] = transpose ? f[x][y] : f[y][x]
//
// Pixel map.  12 fp32 numbers per sample and image kind: A[3][3] row-major, then b[3].  od(u) is the 256-entry table of
// stain_quant.hip (from the host).  od'_c = ((od_r A[0][c] + od_g A[1][c]) + od_b A[2][c]) + b[c], every operation rounded
// on its own; u'_c = clamp(rint(255 * exp2(od'_c * -log2(10))), 0, 255): the expression of stain_norm.hip's apply pass
// with a bias.  A pixel with min(R, G, B) >= white keeps its bytes (glass is not tinted).  Without a map the bytes pass.
//
// One thread owns four consecutive output pixels of one row, of source, target and mask together: twelve source bytes
// come as three dwords where they are 4-byte aligned (bytes otherwise: `left`, the pitch and the base are arbitrary), a
// horizontal flip reverses the quad in registers, each fp32 plane gets one 16-byte store where the row allows it.  A
// workgroup owns one 32 x 32 output tile of one sample, so the sample's transpose bit is uniform in it: a plain sample
// goes from registers to memory; a transposed one reads the mirrored tile of f row by row as well, exchanges the mapped
// bytes through an LDS tile (two words per pixel: source RGB + mask, target RGB) and writes rows again.  No lane walks a
// column of global memory, no workgroup waits for another.
//
// Nothing here allocates, synchronises or reads back to the host.
#include "common.h"

namespace {

constexpr int AG_T = 32;                     // edge of a workgroup's output tile: 32 rows x 8 quads = 256 threads
constexpr int AG_STAIN_BLOCKS = 16384;       // grid.x cap of the stain-only pass
constexpr int AG_MAX_S = 32768;

struct AgParams {
  const unsigned char *src, *tgt, *mask;
  long src_pitch, src_img, tgt_pitch, tgt_img, mask_pitch, mask_img;   // bytes
  const int* params;
  const float *src_map, *tgt_map;
  float *out_src, *out_tgt;
  void* out_mask;
  unsigned char *u8_src, *u8_tgt;
  int cols, S, tiles_x, white, mask_kind;    // white: 256 = off; mask_kind: 0 none, 1 fp32, 2 uint8, 3 int64
  float od[256];
};

struct AgStainParams {
  const unsigned char* img;
  long pitch, img_stride;
  const float* maps;
  void* out;
  long out_pitch, out_img;
  int H, W, white;
  float od[256];
};

// ((a0 * c0) + (a1 * c1)) + (a2 * c2), every operation rounded on its own (sn_dot3 of stain_norm.hip)
__device__ __forceinline__ float ag_dot3(float a0, float a1, float a2, float c0, float c1, float c2) {
#pragma clang fp contract(off)
  const float p0 = a0 * c0, p1 = a1 * c1, p2 = a2 * c2;
  const float s = p0 + p1;
  return s + p2;
}

// the level of channel c under the map m = A[3][3], b[3]
__device__ __forceinline__ float ag_level(float odr, float odg, float odb, const float* m, int c) {
#pragma clang fp contract(off)
  const float d = ag_dot3(odr, odg, odb, m[c], m[3 + c], m[6 + c]);
  const float od = d + m[9 + c];
  const float e = od * -3.321928094887362f;    // 10^(-od) = 2^(-od * log2(10))
  const float v = 255.0f * exp2f(e);
  return fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

// what to_tensor + Normalize(0.5, 0.5) make of the byte: (u / 255 - 0.5) / 0.5, each operation rounded on its own
__device__ __forceinline__ float ag_network(unsigned u) {
#pragma clang fp contract(off)
  const float a = (float)u / 255.0f;
  const float b = a - 0.5f;
  return b / 0.5f;
}

// The pixel map both entry points share: the first px pixels of v (3 j + c) in place.
__device__ __forceinline__ void ag_map_quad(const float* lut, const float* m, int white, int px, unsigned* v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < px) {
      const unsigned r = v[3 * j], g = v[3 * j + 1], b = v[3 * j + 2];
      if ((int)min(r, min(g, b)) < white) {
        const float odr = lut[r], odg = lut[g], odb = lut[b];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * j + c] = (unsigned)ag_level(odr, odg, odb, m, c);
      }
    }
  }
}

// px (1..4) consecutive RGB pixels from byte address p on; slot j takes pixel (rev ? px-1-j : j)
__device__ __forceinline__ void ag_load_rgb(const unsigned char* p, int px, bool rev, unsigned* v) {
  if (px == 4 && ((uintptr_t)p & 3) == 0) {
    const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];   // r0 g0 b0 r1
    const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];   // g1 b1 r2 g2
    const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];   // b2 r3 g3 b3
    unsigned t[12];
    t[0] = w0 & 255; t[1] = (w0 >> 8) & 255; t[2] = (w0 >> 16) & 255;
    t[3] = w0 >> 24; t[4] = w1 & 255; t[5] = (w1 >> 8) & 255;
    t[6] = (w1 >> 16) & 255; t[7] = w1 >> 24; t[8] = w2 & 255;
    t[9] = (w2 >> 8) & 255; t[10] = (w2 >> 16) & 255; t[11] = w2 >> 24;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * j + c] = rev ? t[3 * (3 - j) + c] : t[3 * j + c];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const unsigned char* q = p + 3 * (rev ? px - 1 - j : j);
        v[3 * j] = q[0]; v[3 * j + 1] = q[1]; v[3 * j + 2] = q[2];
      }
    }
  }
}

__device__ __forceinline__ void ag_load_mask(const unsigned char* p, int px, bool rev, unsigned* v) {
  if (px == 4 && ((uintptr_t)p & 3) == 0) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
    const unsigned t[4] = {w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24};
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = rev ? t[3 - j] : t[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) v[j] = p[rev ? px - 1 - j : j];
    }
  }
}

// f[a][b0 .. b0 + px) of sample n, mapped: vs / vt 3 j + c, vm j
__device__ __forceinline__ void ag_fetch(const AgParams& P, int n, int a, int b0, int px, int top, int left, bool hflip,
                                         bool vflip, const float* lut, const float* ms, const float* mt, unsigned* vs,
                                         unsigned* vt, unsigned* vm) {
  const long row = top + (vflip ? P.S - 1 - a : a);
  const long col = left + (hflip ? P.S - b0 - px : b0);
  ag_load_rgb(P.src + (long)n * P.src_img + row * P.src_pitch + 3 * col, px, hflip, vs);
  ag_load_rgb(P.tgt + (long)n * P.tgt_img + row * P.tgt_pitch + 3 * col, px, hflip, vt);
  if (P.mask) ag_load_mask(P.mask + (long)n * P.mask_img + row * P.mask_pitch + col, px, hflip, vm);
  if (P.src_map) ag_map_quad(lut, ms, P.white, px, vs);
  if (P.tgt_map) ag_map_quad(lut, mt, P.white, px, vt);
}

// px pixels (3 j + c) to the three planes of one fp32 image from o on
__device__ __forceinline__ void ag_store_planes(float* o, long plane, int px, bool vec, const unsigned* v) {
  if (vec) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<f32x4*>(o + c * plane) =
          f32x4{ag_network(v[c]), ag_network(v[3 + c]), ag_network(v[6 + c]), ag_network(v[9 + c])};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane + j] = ag_network(v[3 * j + c]);
      }
    }
  }
}

// px RGB pixels as bytes from o on: three dword stores where the twelve bytes are aligned
__device__ __forceinline__ void ag_store_rgb(unsigned char* o, int px, const unsigned* v) {
  if (px == 4 && ((uintptr_t)o & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      reinterpret_cast<unsigned*>(o)[i] = v[4 * i] | (v[4 * i + 1] << 8) | (v[4 * i + 2] << 16) | (v[4 * i + 3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        o[3 * j] = (unsigned char)v[3 * j]; o[3 * j + 1] = (unsigned char)v[3 * j + 1];
        o[3 * j + 2] = (unsigned char)v[3 * j + 2];
      }
    }
  }
}

// out[y][xb .. xb + px) of sample n
__device__ __forceinline__ void ag_store(const AgParams& P, int n, int y, int xb, int px, const unsigned* vs,
                                         const unsigned* vt, const unsigned* vm) {
  const long plane = (long)P.S * P.S;
  const long at = (long)y * P.S + xb;
  float* os = P.out_src + (long)n * 3 * plane + at;
  float* ot = P.out_tgt + (long)n * 3 * plane + at;
  const bool quad = px == 4 && (plane & 3) == 0;
  ag_store_planes(os, plane, px, quad && ((uintptr_t)os & 15) == 0, vs);
  ag_store_planes(ot, plane, px, quad && ((uintptr_t)ot & 15) == 0, vt);
  if (P.mask_kind == 1) {
    float* om = reinterpret_cast<float*>(P.out_mask) + (long)n * plane + at;
    if (px == 4 && ((uintptr_t)om & 15) == 0) {
      *reinterpret_cast<f32x4*>(om) = f32x4{(float)vm[0], (float)vm[1], (float)vm[2], (float)vm[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) om[j] = (float)vm[j];
      }
    }
  } else if (P.mask_kind == 2) {
    unsigned char* om = reinterpret_cast<unsigned char*>(P.out_mask) + (long)n * plane + at;
    if (px == 4 && ((uintptr_t)om & 3) == 0) {
      *reinterpret_cast<unsigned*>(om) = vm[0] | (vm[1] << 8) | (vm[2] << 16) | (vm[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) om[j] = (unsigned char)vm[j];
      }
    }
  } else if (P.mask_kind == 3) {
    long long* om = reinterpret_cast<long long*>(P.out_mask) + (long)n * plane + at;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) om[j] = (long long)vm[j];
    }
  }
  if (P.u8_src) ag_store_rgb(P.u8_src + ((long)n * plane + at) * 3, px, vs);
  if (P.u8_tgt) ag_store_rgb(P.u8_tgt + ((long)n * plane + at) * 3, px, vt);
}

__global__ __launch_bounds__(256) void ag_paired_kernel(const AgParams P) {
  __shared__ float lut[256];
  __shared__ unsigned tile[2][AG_T][AG_T + 1];
  const int tid = threadIdx.x, n = blockIdx.y;
  if (P.src_map || P.tgt_map) {                // uniform in the grid
    lut[tid] = P.od[tid];                      // 256 lanes, 256 entries
    __syncthreads();
  }
  const int* pr = P.params + (long)n * P.cols;
  const int top = pr[0], left = pr[1];
  const bool hflip = pr[2] != 0, vflip = pr[3] != 0;
  const bool transposed = P.cols == 5 && pr[4] != 0;
  float ms[12], mt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    ms[i] = P.src_map ? P.src_map[(long)n * 12 + i] : 0.0f;
    mt[i] = P.tgt_map ? P.tgt_map[(long)n * 12 + i] : 0.0f;
  }
  const int ty = blockIdx.x / P.tiles_x, tx = blockIdx.x - ty * P.tiles_x;
  const int y0 = ty * AG_T, x0 = tx * AG_T;
  const int r = tid >> 3, q = tid & 7;
  const int y = y0 + r, xb = x0 + 4 * q;
  const int px = min(4, P.S - xb);
  unsigned vs[12], vt[12], vm[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) vs[i] = vt[i] = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) vm[j] = 0u;
  if (!transposed) {                           // uniform in the workgroup
    if (y < P.S && px > 0) {
      ag_fetch(P, n, y, xb, px, top, left, hflip, vflip, lut, ms, mt, vs, vt, vm);
      ag_store(P, n, y, xb, px, vs, vt, vm);
    }
    return;
  }
  // out[y0 + i][x0 + k] = f[x0 + k][y0 + i]: read rows x0.. of f at columns y0.., exchange, write rows y0.. of out
  const int a = x0 + r, b0 = y0 + 4 * q;
  const int pf = min(4, P.S - b0);
  if (a < P.S && pf > 0) ag_fetch(P, n, a, b0, pf, top, left, hflip, vflip, lut, ms, mt, vs, vt, vm);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    tile[0][r][4 * q + j] = vs[3 * j] | (vs[3 * j + 1] << 8) | (vs[3 * j + 2] << 16) | (vm[j] << 24);
    tile[1][r][4 * q + j] = vt[3 * j] | (vt[3 * j + 1] << 8) | (vt[3 * j + 2] << 16);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned w0 = tile[0][4 * q + j][r], w1 = tile[1][4 * q + j][r];
    vs[3 * j] = w0 & 255; vs[3 * j + 1] = (w0 >> 8) & 255; vs[3 * j + 2] = (w0 >> 16) & 255;
    vm[j] = w0 >> 24;
    vt[3 * j] = w1 & 255; vt[3 * j + 1] = (w1 >> 8) & 255; vt[3 * j + 2] = (w1 >> 16) & 255;
  }
  if (y < P.S && px > 0) ag_store(P, n, y, xb, px, vs, vt, vm);
}

// One thread per 4 consecutive pixels of one row; blockIdx.y is the sample, so its map is uniform in the workgroup.
template <bool F32>
__global__ __launch_bounds__(256) void ag_stain_kernel(const AgStainParams P) {
  __shared__ float lut[256];
  const int tid = threadIdx.x, n = blockIdx.y;
  lut[tid] = P.od[tid];
  __syncthreads();
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = P.maps[(long)n * 12 + i];
  const int nq = (P.W + 3) >> 2;
  const long total = (long)P.H * nq;
  const long plane = (long)P.H * P.W;
  const unsigned char* base = P.img + (long)n * P.img_stride;
  for (long i = (long)blockIdx.x * 256 + tid; i < total; i += (long)gridDim.x * 256) {
    const int y = (int)(i / nq), xq = (int)(i - (long)y * nq);
    const int x0 = 4 * xq, px = min(4, P.W - x0);
    unsigned v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = 0u;
    ag_load_rgb(base + (long)y * P.pitch + 3L * x0, px, false, v);
    ag_map_quad(lut, m, P.white, px, v);
    if (F32) {
      float* o = reinterpret_cast<float*>(P.out) + (long)n * 3 * plane + (long)y * P.W + x0;
      ag_store_planes(o, plane, px, px == 4 && (plane & 3) == 0 && ((uintptr_t)o & 15) == 0, v);
    } else {
      ag_store_rgb(reinterpret_cast<unsigned char*>(P.out) + (long)n * P.out_img + (long)y * P.out_pitch + 3L * x0, px,
                   v);
    }
  }
}

bool ag_bad_u8(long pitch, long img, int B, int H, long row_bytes) {
  return pitch < row_bytes || (B > 1 && img < pitch * (long)H);
}

}  // namespace

// src / tgt: uint8 [B][Hs][Ws][3] with a row pitch and an image stride in bytes; mask (optional): uint8 [B][Hs][Ws] with
// its own; params: DEVICE int32 [B][param_cols], param_cols 4 or 5; src_map / tgt_map (each optional): DEVICE fp32
// [B][12]; od_table: HOST fp32 [256] (needed with a map); white: -1 = off, else 0..255.  out_src / out_tgt: fp32
// [B][3][S][S]; out_mask per mask_kind (0 none, 1 fp32, 2 uint8, 3 int64) [B][1][S][S]; out_src_u8 / out_tgt_u8 (each
// optional): uint8 [B][S][S][3].  The crop windows are validated by the caller on the host; the kernel does not clamp.
extern "C" int s2s_paired_augment(const void* src_u8, long src_pitch, long src_img, const void* tgt_u8, long tgt_pitch,
                                  long tgt_img, const void* mask_u8, long mask_pitch, long mask_img, int B, int Hs,
                                  int Ws, int S, const int* params, int param_cols, const float* src_map,
                                  const float* tgt_map, const float* od_table, int white, float* out_src,
                                  float* out_tgt, void* out_mask, int mask_kind, void* out_src_u8, void* out_tgt_u8,
                                  void* stream) {
  if (!src_u8 || !tgt_u8 || !params || !out_src || !out_tgt) return S2S_ERR_NULL;
  if ((src_map || tgt_map) && !od_table) return S2S_ERR_NULL;
  if (mask_kind < 0 || mask_kind > 3) return S2S_ERR_DTYPE;
  if ((mask_kind != 0) != (mask_u8 != nullptr) || (mask_kind != 0) != (out_mask != nullptr)) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || S < 1 || S > AG_MAX_S || Hs < S || Ws < S || Hs > (1 << 30) || Ws > (1 << 30))
    return S2S_ERR_SHAPE;
  if (param_cols != 4 && param_cols != 5) return S2S_ERR_SHAPE;
  if (white < -1 || white > 255) return S2S_ERR_SHAPE;
  if (ag_bad_u8(src_pitch, src_img, B, Hs, 3L * Ws) || ag_bad_u8(tgt_pitch, tgt_img, B, Hs, 3L * Ws))
    return S2S_ERR_SHAPE;
  if (mask_u8 && ag_bad_u8(mask_pitch, mask_img, B, Hs, Ws)) return S2S_ERR_SHAPE;
  AgParams P;
  P.src = (const unsigned char*)src_u8; P.tgt = (const unsigned char*)tgt_u8; P.mask = (const unsigned char*)mask_u8;
  P.src_pitch = src_pitch; P.src_img = src_img;
  P.tgt_pitch = tgt_pitch; P.tgt_img = tgt_img;
  P.mask_pitch = mask_pitch; P.mask_img = mask_img;
  P.params = params; P.cols = param_cols;
  P.src_map = src_map; P.tgt_map = tgt_map;
  P.out_src = out_src; P.out_tgt = out_tgt; P.out_mask = out_mask; P.mask_kind = mask_kind;
  P.u8_src = (unsigned char*)out_src_u8; P.u8_tgt = (unsigned char*)out_tgt_u8;
  P.S = S; P.tiles_x = cdiv(S, AG_T);
  P.white = white < 0 ? 256 : white;
  for (int i = 0; i < 256; ++i) P.od[i] = od_table ? od_table[i] : 0.0f;
  hipLaunchKernelGGL(ag_paired_kernel, dim3((unsigned)(P.tiles_x * P.tiles_x), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, P);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// img: uint8 [B][H][W][3] with pitch / img_stride in bytes; maps: DEVICE fp32 [B][12]; od_table: HOST fp32 [256]; white as
// above.  out_f32 == 0: uint8 [B][H][W][3] with out_pitch / out_img in bytes; else fp32 [B][3][H][W] = (u' / 255 - 0.5) /
// 0.5 (out_pitch, out_img ignored).
extern "C" int s2s_stain_augment_u8(const void* img, long pitch, long img_stride, int B, int H, int W, const float* maps,
                                    const float* od_table, int white, void* out, long out_pitch, long out_img,
                                    int out_f32, void* stream) {
  if (!img || !maps || !od_table || !out) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30)) return S2S_ERR_SHAPE;
  if (white < -1 || white > 255) return S2S_ERR_SHAPE;
  if (ag_bad_u8(pitch, img_stride, B, H, 3L * W)) return S2S_ERR_SHAPE;
  if (!out_f32 && ag_bad_u8(out_pitch, out_img, B, H, 3L * W)) return S2S_ERR_SHAPE;
  AgStainParams P;
  P.img = (const unsigned char*)img; P.pitch = pitch; P.img_stride = img_stride;
  P.maps = maps; P.out = out; P.out_pitch = out_pitch; P.out_img = out_img;
  P.H = H; P.W = W;
  P.white = white < 0 ? 256 : white;
  for (int i = 0; i < 256; ++i) P.od[i] = od_table[i];
  long blocks = ((long)H * cdiv(W, 4) + 255) / 256;
  if (blocks > AG_STAIN_BLOCKS) blocks = AG_STAIN_BLOCKS;
  const dim3 grid((unsigned)blocks, (unsigned)B);
  if (out_f32) hipLaunchKernelGGL(ag_stain_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, P);
  else hipLaunchKernelGGL(ag_stain_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, P);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
