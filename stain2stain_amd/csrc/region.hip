// Tiled whole-region translation: everything between two sampler calls (stain2stain_amd/region.py).
//
// A region (uint8 RGB, any size) is cut into overlapping T x T tiles (region.plan_tiles), the tiles of one batch are
// gathered and normalised (s2s_region_gather), the sampler runs on them, and the outputs are added into an fp32
// accumulator with a feathered separable weight (s2s_region_blend); rows no later tile covers are divided out, converted
// and cleared (s2s_region_finalize).  The accumulator is a ring of band_rows image rows (row r at r % band_rows), so its
// size does not depend on the region's height.
//
// Determinism: every accumulator element has exactly one writer per blend launch, which adds the tiles covering it in
// plan order (acc = fmaf(w, v, acc), wsum += w).  No atomics; results are bit-reproducible.
// All three kernels are bandwidth-bound and tiny next to the sampler.
#include "common.h"

namespace {

// numpy.pad(mode="reflect") index folding, pads longer than the axis included; L == 1 maps everything to 0.
__device__ __forceinline__ int reflect_index(int i, int L) {
  if (L == 1) return 0;
  const int period = 2 * (L - 1);
  if (i < 0) i = -i;
  i %= period;
  return i < L ? i : period - i;
}

// to_tensor + Normalize(0.5, 0.5): the expression and order of paired_prepare_kernel (input_pipeline.hip)
__device__ __forceinline__ float normalise_u8(unsigned v) { return ((float)v / 255.0f - 0.5f) / 0.5f; }

// One thread per 4 consecutive tile pixels of one tile row: 12 input bytes (three dword loads when they are 4-byte
// aligned, the common case of a tightly packed image and a tile stride that is a multiple of 4), one 16-byte store per
// channel plane.  Rows outside [band_top, band_top + band_h) of the buffer are never read: such a pixel (an origin the
// caller did not stage) comes out as NaN.
__global__ void region_gather_kernel(const unsigned char* __restrict__ img, long pitch, int H, int W, int band_top,
                                     int band_h, const int* __restrict__ origins, float* __restrict__ out, int B,
                                     int T) {
  const int TQ = T >> 2;
  const long total = (long)B * T * TQ;
  const long plane = (long)T * T;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int xq = (int)(q % TQ);
    const long t = q / TQ;
    const int y = (int)(t % T);
    const int n = (int)(t / T);
    const int top = origins[2 * n], left = origins[2 * n + 1];
    const int by = reflect_index(top + y, H) - band_top;
    f32x4 c0, c1, c2;
    if (by < 0 || by >= band_h) {
      const float nan = __builtin_nanf("");
      c0 = f32x4{nan, nan, nan, nan}; c1 = c0; c2 = c0;
    } else {
      const unsigned char* row = img + (long)by * pitch;
      const int x0 = left + 4 * xq;
      const unsigned char* p = row + 3L * x0;
      if (x0 >= 0 && x0 + 3 < W && ((uintptr_t)p & 3) == 0) {
        const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];   // r0 g0 b0 r1
        const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];   // g1 b1 r2 g2
        const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];   // b2 r3 g3 b3
        c0 = f32x4{normalise_u8(w0 & 255), normalise_u8(w0 >> 24), normalise_u8((w1 >> 16) & 255),
                   normalise_u8((w2 >> 8) & 255)};
        c1 = f32x4{normalise_u8((w0 >> 8) & 255), normalise_u8(w1 & 255), normalise_u8(w1 >> 24),
                   normalise_u8((w2 >> 16) & 255)};
        c2 = f32x4{normalise_u8((w0 >> 16) & 255), normalise_u8((w1 >> 8) & 255), normalise_u8(w2 & 255),
                   normalise_u8(w2 >> 24)};
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned char* s = row + 3L * reflect_index(x0 + k, W);
          c0[k] = normalise_u8(s[0]);
          c1[k] = normalise_u8(s[1]);
          c2[k] = normalise_u8(s[2]);
        }
      }
    }
    float* o = out + (long)n * 3 * plane + (long)y * T + 4 * xq;
    *reinterpret_cast<f32x4*>(o) = c0;
    *reinterpret_cast<f32x4*>(o + plane) = c1;
    *reinterpret_cast<f32x4*>(o + 2 * plane) = c2;
  }
}

// feathered window along one axis: 1 without overlap, else min(1, (i + 0.5) / overlap, (T - i - 0.5) / overlap)
__device__ __forceinline__ float axis_weight(int i, int T, int overlap) {
  if (overlap == 0) return 1.0f;
  const float ov = (float)overlap;
  const float a = ((float)i + 0.5f) / ov;
  const float b = ((float)(T - i) - 0.5f) / ov;
  return fminf(1.0f, fminf(a, b));
}

// C + 1 interleaved floats of one accumulator pixel; 16-byte accesses when the pixel is a whole number of them
template <int N>
__device__ __forceinline__ void load_px(const float* p, float* v) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p + k);
      v[k] = a[0]; v[k + 1] = a[1]; v[k + 2] = a[2]; v[k + 3] = a[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = p[k];
  }
}
template <int N>
__device__ __forceinline__ void store_px(float* p, const float* v) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 4) *reinterpret_cast<f32x4*>(p + k) = f32x4{v[k], v[k + 1], v[k + 2], v[k + 3]};
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = v[k];
  }
}

// One thread per image pixel of rows [r0, r0 + rows): the single writer of that pixel's accumulator.  The tile loop is
// uniform across the workgroup (origins are read by every lane alike), the coverage test per lane.  Channel c < ca of
// tile k comes from a[k][c], the others from b[k][c - ca]: the sampler's image and probabilities without a concatenation.
template <int C>
__global__ void region_blend_kernel(const float* __restrict__ a, int ca, const float* __restrict__ b,
                                    const int* __restrict__ origins, int n, int T, int overlap,
                                    float* __restrict__ acc, int band_rows, int W, int r0, int wblocks) {
  const int r = r0 + (int)(blockIdx.x / wblocks);
  const int x = (int)(blockIdx.x % wblocks) * blockDim.x + threadIdx.x;
  if (x >= W) return;
  const int cb = C - ca;
  const long plane = (long)T * T;
  float* p = acc + ((long)(r % band_rows) * W + x) * (C + 1);
  float v[C + 1];
  load_px<C + 1>(p, v);
  bool hit = false;
  for (int k = 0; k < n; ++k) {
    const int i = r - origins[2 * k], j = x - origins[2 * k + 1];
    if ((unsigned)i >= (unsigned)T || (unsigned)j >= (unsigned)T) continue;
    const float w = axis_weight(i, T, overlap) * axis_weight(j, T, overlap);
    const long off = (long)i * T + j;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float s = c < ca ? a[((long)k * ca + c) * plane + off] : b[((long)k * cb + (c - ca)) * plane + off];
      v[c] = fmaf(w, s, v[c]);
    }
    v[C] += w;
    hit = true;
  }
  if (hit) store_px<C + 1>(p, v);
}

// One thread per pixel of rows [r0, r0 + rows): out = acc / wsum (IEEE division), optionally as fp32 [rows][W][C];
// channels 0..2 as uint8 with the reference's save conversion, trunc(clamp((out * 0.5 + 0.5) * 255, 0, 255)), each
// operation rounded in fp32 (no contraction into an fma); then the ring row is cleared for reuse.
template <int C>
__global__ void region_finalize_kernel(float* __restrict__ acc, int band_rows, int W, int r0, int rows,
                                       unsigned char* __restrict__ out_u8, long pitch_u8, float* __restrict__ out_f,
                                       long pitch_f, int out_top) {
#pragma clang fp contract(off)
  const long total = (long)rows * W;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int x = (int)(q % W);
    const int r = r0 + (int)(q / W);
    float* p = acc + ((long)(r % band_rows) * W + x) * (C + 1);
    float v[C + 1];
    load_px<C + 1>(p, v);
    float o[C];
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = v[c] / v[C];
    if (out_f) {
      float* d = out_f + (long)(r - out_top) * pitch_f + (long)x * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = o[c];
    }
    if (out_u8) {
      unsigned char* d = out_u8 + (long)(r - out_top) * pitch_u8 + 3L * x;
#pragma unroll
      for (int c = 0; c < 3 && c < C; ++c) {
        const float y = o[c] * 0.5f;
        const float z = (y + 0.5f) * 255.0f;
        d[c] = (unsigned char)(int)fminf(fmaxf(z, 0.0f), 255.0f);
      }
    }
    float zero[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) zero[c] = 0.0f;
    store_px<C + 1>(p, zero);
  }
}

// ---- tissue-aware regions: background tiles are measured, skipped and passed through --------

// One workgroup of 256 lanes per tile; counts[k] = tissue pixels of the tile's intersection with the image (reflected
// padding is not counted).  Lanes walk the in-image rows as the gather does: one lane per 4 consecutive pixels, three
// dword loads when the 12 bytes are aligned and the quad is whole, bytes otherwise.  Integer count per lane, xor-shuffle
// over the wave, four partials through LDS, one plain store: every counts[k] is written.  A tile whose in-image rows are
// not all inside the band gets -1 and reads nothing.
__global__ void __launch_bounds__(256)
region_tissue_count_kernel(const unsigned char* __restrict__ img, long pitch, int H, int W, int band_top, int band_h,
                           const int* __restrict__ origins, int T, int white, int black, int* __restrict__ counts) {
  __shared__ int part[4];
  const int k = blockIdx.x;
  const int top = origins[2 * k], left = origins[2 * k + 1];
  const int hh = min(T, H - top), ww = min(T, W - left);
  if (top < band_top || top + hh > band_top + band_h || top < 0 || left < 0 || hh <= 0 || ww <= 0) {   // block-uniform
    if (threadIdx.x == 0) counts[k] = -1;
    return;
  }
  const int nq = (ww + 3) >> 2;
  const int total = hh * nq;
  int cnt = 0;
  for (int q = threadIdx.x; q < total; q += 256) {
    const int y = q / nq, xq = q - y * nq;
    const unsigned char* p = img + (long)(top - band_top + y) * pitch + 3L * (left + 4 * xq);
    const int px = min(4, ww - 4 * xq);
    if (px == 4 && ((uintptr_t)p & 3) == 0) {
      const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];   // r0 g0 b0 r1
      const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];   // g1 b1 r2 g2
      const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];   // b2 r3 g3 b3
      cnt += is_tissue(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, white, black);
      cnt += is_tissue(w0 >> 24, w1 & 255, (w1 >> 8) & 255, white, black);
      cnt += is_tissue((w1 >> 16) & 255, w1 >> 24, w2 & 255, white, black);
      cnt += is_tissue((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24, white, black);
    } else {
      for (int j = 0; j < px; ++j) cnt += is_tissue(p[3 * j], p[3 * j + 1], p[3 * j + 2], white, black);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[k] = part[0] + part[1] + part[2] + part[3];
}

// One thread per image pixel of rows [r0, r0 + rows), the single writer of that pixel's skip weight: ws += wy(i) * wx(j)
// for every skipped tile covering it, in the given order, with the blend's axis_weight.  Reads no image bytes.
__global__ void region_skip_weight_kernel(const int* __restrict__ origins, int n, int T, int overlap,
                                          float* __restrict__ ws, int band_rows, int W, int r0, int wblocks) {
  const int r = r0 + (int)(blockIdx.x / wblocks);
  const int x = (int)(blockIdx.x % wblocks) * blockDim.x + threadIdx.x;
  if (x >= W) return;
  float* p = ws + (long)(r % band_rows) * W + x;
  float v = *p;
  bool hit = false;
  for (int k = 0; k < n; ++k) {
    const int i = r - origins[2 * k], j = x - origins[2 * k + 1];
    if ((unsigned)i >= (unsigned)T || (unsigned)j >= (unsigned)T) continue;
    v += axis_weight(i, T, overlap) * axis_weight(j, T, overlap);
    hit = true;
  }
  if (hit) *p = v;
}

// region_finalize_kernel for a region with skipped tiles.  wk = acc[C] is the weight of the kept tiles, s = ws the
// weight of the skipped ones, whose image is the normalised source and whose probabilities are 0.  A pixel no kept tile
// covers is the source itself: its bytes are copied, never converted (the fp32 normalise -> save round trip loses 1 on
// 63 of the 256 byte values).  Elsewhere x = fmaf(s, normalise_u8(src), acc) / (wk + s); with s == 0 that is acc / wk,
// bit-equal to region_finalize_kernel.  Both ring rows are cleared.
template <int C>
__global__ void region_finalize_mixed_kernel(float* __restrict__ acc, float* __restrict__ ws, int band_rows, int W,
                                             int r0, int rows, const unsigned char* __restrict__ src, long src_pitch,
                                             int src_top, unsigned char* __restrict__ out_u8, long pitch_u8,
                                             float* __restrict__ out_f, long pitch_f, int out_top) {
#pragma clang fp contract(off)
  const long total = (long)rows * W;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int x = (int)(q % W);
    const int r = r0 + (int)(q / W);
    const long ring = (long)(r % band_rows) * W + x;
    float* p = acc + ring * (C + 1);
    float v[C + 1];
    load_px<C + 1>(p, v);
    const float s = ws[ring];
    const unsigned char* u = src + (long)(r - src_top) * src_pitch + 3L * x;
    const unsigned char b[3] = {u[0], u[1], u[2]};
    const bool copy = v[C] == 0.0f;
    float o[C];
    if (copy) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = c < 3 ? normalise_u8(b[c]) : 0.0f;
    } else {
      const float den = v[C] + s;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = (c < 3 ? fmaf(s, normalise_u8(b[c]), v[c]) : v[c]) / den;
    }
    if (out_f) {
      float* d = out_f + (long)(r - out_top) * pitch_f + (long)x * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = o[c];
    }
    if (out_u8) {
      unsigned char* d = out_u8 + (long)(r - out_top) * pitch_u8 + 3L * x;
#pragma unroll
      for (int c = 0; c < 3 && c < C; ++c) {
        const float y = o[c] * 0.5f;
        const float z = (y + 0.5f) * 255.0f;
        d[c] = copy ? b[c] : (unsigned char)(int)fminf(fmaxf(z, 0.0f), 255.0f);
      }
    }
    float zero[C + 1];
#pragma unroll
    for (int c = 0; c <= C; ++c) zero[c] = 0.0f;
    store_px<C + 1>(p, zero);
    ws[ring] = 0.0f;
  }
}

inline int grid_for(long total) {
  long g = (total + 255) / 256;
  if (g > 16384) g = 16384;
  return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int s2s_region_gather(const void* img_u8, long pitch, int H, int W, int band_top, int band_h,
                                 const int* origins, float* out, int B, int T, void* stream) {
  if (!img_u8 || !origins || !out) return S2S_ERR_NULL;
  if (H <= 0 || W <= 0 || B <= 0 || T <= 0 || (T & 3) || band_h <= 0 || band_top < 0 || band_top + band_h > H ||
      pitch < 3L * W)
    return S2S_ERR_SHAPE;
  if ((uintptr_t)out & 15) return S2S_ERR_ALIGN;
  const long total = (long)B * T * (T / 4);
  hipLaunchKernelGGL(region_gather_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)img_u8, pitch, H, W, band_top, band_h, origins, out, B, T);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

#define S2S_REGION_SWITCH(C, CALL) \
  switch (C) {                     \
    case 1: CALL(1); break;        \
    case 2: CALL(2); break;        \
    case 3: CALL(3); break;        \
    case 4: CALL(4); break;        \
    case 5: CALL(5); break;        \
    case 6: CALL(6); break;        \
    case 7: CALL(7); break;        \
    case 8: CALL(8); break;        \
    default: return S2S_ERR_SHAPE; \
  }

extern "C" int s2s_region_blend(const float* tiles, int c0, const float* tiles1, int c1, const int* origins, int n,
                                int T, int overlap, float* acc, int band_rows, int H, int W, int r0, int r1,
                                void* stream) {
  if (!tiles || !origins || !acc || (c1 > 0 && !tiles1)) return S2S_ERR_NULL;
  const int C = c0 + c1;
  if (c0 < 1 || c1 < 0 || C > 8 || n <= 0 || T <= 0 || overlap < 0 || overlap >= T || H <= 0 || W <= 0 ||
      band_rows <= 0 || r0 < 0 || r1 > H || r1 <= r0 || r1 - r0 > band_rows)
    return S2S_ERR_SHAPE;
  if ((C + 1) % 4 == 0 && ((uintptr_t)acc & 15)) return S2S_ERR_ALIGN;
  const int wblocks = cdiv(W, 256);
  const long blocks = (long)wblocks * (r1 - r0);
  if (blocks >= (1L << 31)) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
#define S2S_BLEND(CC)                                                                                              \
  hipLaunchKernelGGL(region_blend_kernel<CC>, dim3((unsigned)blocks), dim3(256), 0, s, tiles, c0, tiles1, origins, \
                     n, T, overlap, acc, band_rows, W, r0, wblocks)
  S2S_REGION_SWITCH(C, S2S_BLEND)
#undef S2S_BLEND
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_region_finalize(float* acc, int band_rows, int W, int C, int r0, int r1, void* out_u8,
                                   long pitch_u8, float* out_f, long pitch_f, int out_top, void* stream) {
  if (!acc || (!out_u8 && !out_f)) return S2S_ERR_NULL;
  if (C < 1 || C > 8 || W <= 0 || band_rows <= 0 || r0 < 0 || r1 <= r0 || r1 - r0 > band_rows || out_top < 0 ||
      out_top > r0 || (out_u8 && (C < 3 || pitch_u8 < 3L * W)) || (out_f && pitch_f < (long)C * W))
    return S2S_ERR_SHAPE;
  if ((C + 1) % 4 == 0 && ((uintptr_t)acc & 15)) return S2S_ERR_ALIGN;
  const long total = (long)(r1 - r0) * W;
  hipStream_t s = (hipStream_t)stream;
#define S2S_FINALIZE(CC)                                                                                            \
  hipLaunchKernelGGL(region_finalize_kernel<CC>, dim3(grid_for(total)), dim3(256), 0, s, acc, band_rows, W, r0,     \
                     r1 - r0, (unsigned char*)out_u8, pitch_u8, out_f, pitch_f, out_top)
  S2S_REGION_SWITCH(C, S2S_FINALIZE)
#undef S2S_FINALIZE
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_region_tissue_count(const void* img_u8, long pitch, int H, int W, int band_top, int band_h,
                                       const int* origins, int n, int T, int white, int black, int* counts,
                                       void* stream) {
  if (!img_u8 || !origins || !counts) return S2S_ERR_NULL;
  if (H <= 0 || W <= 0 || n <= 0 || T <= 0 || band_h <= 0 || band_top < 0 || band_top + band_h > H ||
      pitch < 3L * W || white < 1 || white > 256 || black < 0 || black > 255)
    return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(region_tissue_count_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)img_u8, pitch, H, W, band_top, band_h, origins, T, white, black, counts);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_region_skip_weight(const int* origins, int n, int T, int overlap, float* ws, int band_rows, int H,
                                      int W, int r0, int r1, void* stream) {
  if (!origins || !ws) return S2S_ERR_NULL;
  if (n <= 0 || T <= 0 || overlap < 0 || overlap >= T || H <= 0 || W <= 0 || band_rows <= 0 || r0 < 0 || r1 > H ||
      r1 <= r0 || r1 - r0 > band_rows)
    return S2S_ERR_SHAPE;
  const int wblocks = cdiv(W, 256);
  const long blocks = (long)wblocks * (r1 - r0);
  if (blocks >= (1L << 31)) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(region_skip_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, origins, n,
                     T, overlap, ws, band_rows, W, r0, wblocks);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_region_finalize_mixed(float* acc, float* ws, int band_rows, int W, int C, int r0, int r1,
                                         const void* src_u8, long src_pitch, int src_top, void* out_u8, long pitch_u8,
                                         float* out_f, long pitch_f, int out_top, void* stream) {
  if (!acc || !ws || !src_u8 || (!out_u8 && !out_f)) return S2S_ERR_NULL;
  if (C < 3 || C > 8 || W <= 0 || band_rows <= 0 || r0 < 0 || r1 <= r0 || r1 - r0 > band_rows || out_top < 0 ||
      out_top > r0 || src_top < 0 || src_top > r0 || src_pitch < 3L * W || (out_u8 && pitch_u8 < 3L * W) ||
      (out_f && pitch_f < (long)C * W))
    return S2S_ERR_SHAPE;
  if ((C + 1) % 4 == 0 && ((uintptr_t)acc & 15)) return S2S_ERR_ALIGN;
  const long total = (long)(r1 - r0) * W;
  hipStream_t s = (hipStream_t)stream;
#define S2S_FINALIZE_MIXED(CC)                                                                                      \
  hipLaunchKernelGGL(region_finalize_mixed_kernel<CC>, dim3(grid_for(total)), dim3(256), 0, s, acc, ws, band_rows,  \
                     W, r0, r1 - r0, (const unsigned char*)src_u8, src_pitch, src_top, (unsigned char*)out_u8,      \
                     pitch_u8, out_f, pitch_f, out_top)
  S2S_REGION_SWITCH(C, S2S_FINALIZE_MIXED)
#undef S2S_FINALIZE_MIXED
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
