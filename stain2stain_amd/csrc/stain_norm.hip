// Macenko stain normalisation (Macenko et al., ISBI 2009): three fit passes over the bytes of an H&E image and one apply
// pass.  DESIGN.md section 3.18.
//
//   s2s_stain_moments_u8        pass A: n, sum q_c, sum q_c q_d (c <= d) of the kept pixels, int64 partials per chunk
//   s2s_stain_moments_finalize  partials -> the ten int64 moments
//   s2s_stain_angle_hist_u8     pass B: the histogram of the kept pixels' diamond angle in the plane of the two leading
//                               eigenvectors
//   s2s_stain_conc_hist_u8      pass C: the histograms of the two stain concentrations of the kept pixels
//   s2s_stain_normalize_u8      apply: every pixel re-expressed in the reference basis; uint8 HWC or fp32 NCHW out
//
// Definition.  od(u) is the 256-entry fp32 table of stain_quant.hip; q(u) = rint(od(u) * 2^12) as int32 comes from the
// host as well.  A pixel is KEPT iff black <= max(R, G, B) <= u_beta.  Everything that is counted is an integer: the
// moments are sums of integer products, the histograms count pixels.  The bin of a pixel comes from fp32 arithmetic in
// which every product, sum and quotient is rounded on its own (plain operators under fp contract(off), as sq_conc of
// stain_quant.hip), so a numpy float32 restatement lands in the same bin.  Integer sums do not depend on their order:
// the results are bit-equal run to run and independent of the banding.
//
// The uint8 buffers hold image rows [band_top, band_top + band_h) of B images of H x W pixels, any row pitch, any base
// alignment.  One thread consumes whole pixels, four at a time: three dword loads where the twelve bytes are 4-byte
// aligned, bytes otherwise.
//
// Pass A follows sq_reduce_kernel: a workgroup reduces one chunk of SN_CH rows x SN_CW columns and stores ten int64
// partials at a slot that depends on the chunk's place in the whole image alone; no atomics.  Passes B and C keep a
// uint32 histogram per workgroup in LDS (LDS integer atomics), walk the band with a grid-stride loop and flush their
// non-empty bins once, with 64-bit integer atomics, into a histogram that the call's own first launch zeroes (`reset`).
//
// Nothing here allocates, synchronises or reads back to the host.
#include "common.h"

namespace {

constexpr int SN_CH = 16, SN_CW = 1024;      // rows x columns of one workgroup's chunk in pass A
constexpr int SN_K = 10;                     // int64 partials per chunk
constexpr int SN_NB = 4096;                  // histogram bins (stain_norm.NB)
constexpr float SN_CONC_BINS = 1024.0f;      // NB / CONC_MAX, CONC_MAX = 4 (log10 OD)
constexpr int SN_HIST_BLOCKS = 1024;         // workgroups of the persistent histogram grid: 4 per CU
constexpr int SN_APPLY_BLOCKS = 16384;

struct SnParams {
  const void* img;
  long pitch, img_stride;     // bytes
  int B, W;
  int rows;                   // rows the buffer holds (the band)
  int row0;                   // pass A: image row of the buffer's first row (a multiple of SN_CH)
  int ncy, ncx;               // pass A: chunks of the whole image
  int u_beta, black;
  float coef[17];             // B: plane[2 ch + k]; C: m[3 ch + k]; apply: m[9], scale[2], ref[3 k + ch]
  float od[256];
};

struct SnMomentParams {
  SnParams p;
  int q[256];
};

// px (1..4) consecutive pixels of one row from byte address p on: v[3 j + c]
__device__ __forceinline__ void sn_load_quad(const unsigned char* p, int px, unsigned* v) {
  if (px == 4 && ((uintptr_t)p & 3) == 0) {
    const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];   // r0 g0 b0 r1
    const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];   // g1 b1 r2 g2
    const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];   // b2 r3 g3 b3
    v[0] = w0 & 255; v[1] = (w0 >> 8) & 255; v[2] = (w0 >> 16) & 255;
    v[3] = w0 >> 24; v[4] = w1 & 255; v[5] = (w1 >> 8) & 255;
    v[6] = (w1 >> 16) & 255; v[7] = w1 >> 24; v[8] = w2 & 255;
    v[9] = (w2 >> 8) & 255; v[10] = (w2 >> 16) & 255; v[11] = w2 >> 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) { v[3 * j] = p[3 * j]; v[3 * j + 1] = p[3 * j + 1]; v[3 * j + 2] = p[3 * j + 2]; }
    }
  }
}

__device__ __forceinline__ bool sn_kept(unsigned r, unsigned g, unsigned b, int u_beta, int black) {
  const int mx = (int)max(r, max(g, b));
  return mx <= u_beta && mx >= black;
}

// ((a0 * c0) + (a1 * c1)) + (a2 * c2), every operation rounded on its own
__device__ __forceinline__ float sn_dot3(float a0, float a1, float a2, float c0, float c1, float c2) {
#pragma clang fp contract(off)
  const float p0 = a0 * c0, p1 = a1 * c1, p2 = a2 * c2;
  const float s = p0 + p1;
  return s + p2;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- pass A ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_moments_kernel(const SnMomentParams mp, long long* __restrict__ part) {
  __shared__ int lut[256];
  __shared__ long long red[4][SN_K];
  const SnParams& p = mp.p;
  const int tid = threadIdx.x;
  lut[tid] = mp.q[tid];                        // 256 lanes, 256 entries
  __syncthreads();
  const int cx = blockIdx.x, cyb = blockIdx.y, n = blockIdx.z;
  const int top = cyb * SN_CH, left = cx * SN_CW;               // in the band
  const int hh = max(min(SN_CH, p.rows - top), 0), ww = max(min(SN_CW, p.W - left), 0);
  const int nq = (ww + 3) >> 2;
  const int total = hh * nq;
  const unsigned char* base = reinterpret_cast<const unsigned char*>(p.img) + (long)n * p.img_stride;
  long long acc[SN_K] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < total; i += 256) {
    const int y = i / nq, xq = i - y * nq;
    const int x0 = left + 4 * xq, px = min(4, ww - 4 * xq);
    unsigned v[12];
    sn_load_quad(base + (long)(top + y) * p.pitch + 3L * x0, px, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px && sn_kept(v[3 * j], v[3 * j + 1], v[3 * j + 2], p.u_beta, p.black)) {
        const long long qr = lut[v[3 * j]], qg = lut[v[3 * j + 1]], qb = lut[v[3 * j + 2]];
        acc[0] += 1;
        acc[1] += qr; acc[2] += qg; acc[3] += qb;
        acc[4] += qr * qr; acc[5] += qr * qg; acc[6] += qr * qb;
        acc[7] += qg * qg; acc[8] += qg * qb; acc[9] += qb * qb;
      }
    }
  }
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < SN_K; ++k) {
    const long long s = wave_sum_ll(acc[k]);
    if (lane == 0) red[wv][k] = s;
  }
  __syncthreads();
  if (tid < SN_K) {
    const long cy = (long)(p.row0 / SN_CH) + cyb;
    const long slot = (((long)n * p.ncy + cy) * p.ncx + cx) * SN_K + tid;
    part[slot] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
}

// one workgroup: thread t adds slots t, t + 256, ..., then a tree (integer sums: any order gives the same bits)
__global__ __launch_bounds__(256) void sn_moments_finalize_kernel(const long long* __restrict__ part, long nslots,
                                                                  long long* __restrict__ out) {
  __shared__ long long r[SN_K][256];
  const int tid = threadIdx.x;
  long long s[SN_K] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long i = tid; i < nslots; i += 256) {
#pragma unroll
    for (int k = 0; k < SN_K; ++k) s[k] += part[i * SN_K + k];
  }
#pragma unroll
  for (int k = 0; k < SN_K; ++k) r[k][tid] = s[k];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < SN_K; ++k) r[k][tid] += r[k][tid + h];
    }
    __syncthreads();
  }
  if (tid < SN_K) out[tid] = r[tid][0];
}

// ---- passes B and C -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_zero_kernel(unsigned long long* __restrict__ hist, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hist[i] = 0ull;
}

__device__ __forceinline__ int sn_clamp_bin(float f) {      // f is finite: floor, then clamp as a float, then convert
  return (int)fminf(fmaxf(floorf(f), 0.0f), (float)(SN_NB - 1));
}

// bin of the diamond angle s = y / (|x| + |y|) in [-1, 1]; -1: the pixel lies in the plane's origin
__device__ __forceinline__ int sn_angle_bin(const SnParams& p, float odr, float odg, float odb) {
#pragma clang fp contract(off)
  const float x = sn_dot3(odr, odg, odb, p.coef[0], p.coef[2], p.coef[4]);
  const float y = sn_dot3(odr, odg, odb, p.coef[1], p.coef[3], p.coef[5]);
  const float d = fabsf(x) + fabsf(y);
  if (d == 0.0f) return -1;
  const float s = y / d;
  const float t = s + 1.0f;
  return sn_clamp_bin(t * (float)(SN_NB / 2));
}

__device__ __forceinline__ int sn_conc_bin(const SnParams& p, float odr, float odg, float odb, int k) {
#pragma clang fp contract(off)
  const float c = sn_dot3(odr, odg, odb, p.coef[k], p.coef[3 + k], p.coef[6 + k]);
  return sn_clamp_bin(c * SN_CONC_BINS);
}

// CONC: two histograms (stain 0, stain 1), else the angle histogram.  A workgroup counts at most
// ceil(quads / gridDim.x) * 4 * 256 < 2^32 pixels (the entry points bound the quads of a launch).
template <bool CONC>
__global__ __launch_bounds__(256) void sn_hist_kernel(const SnParams p, unsigned long long* __restrict__ hist) {
  constexpr int NH = CONC ? 2 * SN_NB : SN_NB;
  __shared__ float lut[256];
  __shared__ unsigned h[NH];
  const int tid = threadIdx.x;
  lut[tid] = p.od[tid];
  for (int i = tid; i < NH; i += 256) h[i] = 0u;
  __syncthreads();
  const int nq = (p.W + 3) >> 2;
  const long total = (long)p.B * p.rows * nq;
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const int xq = (int)(q % nq);
    const long t = q / nq;
    const int y = (int)(t % p.rows), n = (int)(t / p.rows);
    const int x0 = 4 * xq, px = min(4, p.W - x0);
    unsigned v[12];
    sn_load_quad(reinterpret_cast<const unsigned char*>(p.img) + (long)n * p.img_stride + (long)y * p.pitch + 3L * x0,
                 px, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px && sn_kept(v[3 * j], v[3 * j + 1], v[3 * j + 2], p.u_beta, p.black)) {
        const float odr = lut[v[3 * j]], odg = lut[v[3 * j + 1]], odb = lut[v[3 * j + 2]];
        if (CONC) {
          atomicAdd(&h[sn_conc_bin(p, odr, odg, odb, 0)], 1u);
          atomicAdd(&h[SN_NB + sn_conc_bin(p, odr, odg, odb, 1)], 1u);
        } else {
          const int b = sn_angle_bin(p, odr, odg, odb);
          if (b >= 0) atomicAdd(&h[b], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NH; i += 256) {
    const unsigned c = h[i];
    if (c) atomicAdd(&hist[i], (unsigned long long)c);
  }
}

// ---- apply ----------------------------------------------------------------------------------------------------------
// the normalised byte of one channel: od' = (c0' * ref_0ch) + (c1' * ref_1ch), u' = clamp(rint(255 * 10^(-od')), 0, 255)
__device__ __forceinline__ float sn_level(float c0, float c1, float r0, float r1) {
#pragma clang fp contract(off)
  const float a = c0 * r0, b = c1 * r1;
  const float od = a + b;
  const float e = od * -3.321928094887362f;    // 10^(-od) = 2^(-od * log2(10))
  const float v = 255.0f * exp2f(e);
  return fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}

// what to_tensor + Normalize(0.5, 0.5) make of the byte: (u / 255 - 0.5) / 0.5, each operation rounded on its own
__device__ __forceinline__ float sn_network(float u) {
#pragma clang fp contract(off)
  const float a = u / 255.0f;
  const float b = a - 0.5f;
  return b / 0.5f;
}

// One thread per 4 consecutive pixels of one row.  uint8 out: three dword stores where the twelve bytes are aligned;
// fp32 out: one 16-byte store per channel plane where the row allows it.
template <bool F32>
__global__ __launch_bounds__(256) void sn_apply_kernel(const SnParams p, void* __restrict__ out, long out_pitch,
                                                       long out_img) {
  __shared__ float lut[256];
  const int tid = threadIdx.x;
  lut[tid] = p.od[tid];
  __syncthreads();
  const int nq = (p.W + 3) >> 2;
  const long total = (long)p.B * p.rows * nq;
  const long plane = (long)p.rows * p.W;
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const int xq = (int)(q % nq);
    const long t = q / nq;
    const int y = (int)(t % p.rows), n = (int)(t / p.rows);
    const int x0 = 4 * xq, px = min(4, p.W - x0);
    unsigned v[12];
    sn_load_quad(reinterpret_cast<const unsigned char*>(p.img) + (long)n * p.img_stride + (long)y * p.pitch + 3L * x0,
                 px, v);
    float u[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
#pragma clang fp contract(off)
        const float odr = lut[v[3 * j]], odg = lut[v[3 * j + 1]], odb = lut[v[3 * j + 2]];
        float c0 = sn_dot3(odr, odg, odb, p.coef[0], p.coef[3], p.coef[6]);
        float c1 = sn_dot3(odr, odg, odb, p.coef[1], p.coef[4], p.coef[7]);
        c0 = c0 * p.coef[9];
        c1 = c1 * p.coef[10];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) u[3 * j + ch] = sn_level(c0, c1, p.coef[11 + ch], p.coef[14 + ch]);
      }
    }
    if (F32) {
      float* o = reinterpret_cast<float*>(out) + (long)n * 3 * plane + (long)y * p.W + x0;
      if (px == 4 && ((uintptr_t)o & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          *reinterpret_cast<f32x4*>(o + ch * plane) =
              f32x4{sn_network(u[ch]), sn_network(u[3 + ch]), sn_network(u[6 + ch]), sn_network(u[9 + ch])};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < px) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch * plane + j] = sn_network(u[3 * j + ch]);
          }
        }
      }
    } else {
      unsigned char* o = reinterpret_cast<unsigned char*>(out) + (long)n * out_img + (long)y * out_pitch + 3L * x0;
      if (px == 4 && ((uintptr_t)o & 3) == 0) {
        unsigned w[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
          w[i] = (unsigned)u[4 * i] | ((unsigned)u[4 * i + 1] << 8) | ((unsigned)u[4 * i + 2] << 16) |
                 ((unsigned)u[4 * i + 3] << 24);
        reinterpret_cast<unsigned*>(o)[0] = w[0];
        reinterpret_cast<unsigned*>(o)[1] = w[1];
        reinterpret_cast<unsigned*>(o)[2] = w[2];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < px) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[3 * j + ch] = (unsigned char)u[3 * j + ch];
          }
        }
      }
    }
  }
}

// the checks every pass shares; fills what they share of the parameters
int sn_fill(SnParams& p, const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
            const float* od_table, const float* coef, int ncoef, int u_beta, int black) {
  if (!img || !od_table || !coef) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30)) return S2S_ERR_SHAPE;
  if (band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (pitch < 3L * W || (B > 1 && img_stride < pitch * (long)band_h)) return S2S_ERR_SHAPE;
  if (u_beta < 0 || u_beta > 255 || black < 0 || black > 255) return S2S_ERR_SHAPE;
  p.img = img;
  p.pitch = pitch;
  p.img_stride = img_stride;
  p.B = B;
  p.W = W;
  p.rows = band_h;
  p.row0 = band_top;
  p.ncy = cdiv(H, SN_CH);
  p.ncx = cdiv(W, SN_CW);
  p.u_beta = u_beta;
  p.black = black;
  for (int i = 0; i < 17; ++i) p.coef[i] = i < ncoef ? coef[i] : 0.0f;
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  return S2S_OK;
}

// workgroups of a grid-stride pass over `quads` four-pixel groups; 0: too many for the uint32 LDS counters
unsigned sn_blocks(long quads, int cap) {
  long blocks = (quads + 255) / 256;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const long per_thread = (quads + blocks * 256 - 1) / (blocks * 256);
  return per_thread * 1024 >= (1L << 32) ? 0u : (unsigned)blocks;
}

template <bool CONC>
int sn_hist(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H, int W,
            const float* od_table, const float* coef, int ncoef, int u_beta, int black, int reset, long* hist,
            void* stream) {
  if (!hist) return S2S_ERR_NULL;
  SnParams p;
  const int rc = sn_fill(p, img, pitch, img_stride, B, band_top, band_h, H, W, od_table, coef, ncoef, u_beta, black);
  if (rc != S2S_OK) return rc;
  const unsigned blocks = sn_blocks((long)B * band_h * cdiv(W, 4), SN_HIST_BLOCKS);
  if (!blocks) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(unsigned long long), "int64 counts");
  constexpr int NH = CONC ? 2 * SN_NB : SN_NB;
  hipStream_t s = (hipStream_t)stream;
  if (reset) {
    hipLaunchKernelGGL(sn_zero_kernel, dim3(NH / 256), dim3(256), 0, s, (unsigned long long*)hist, NH);
    S2S_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(sn_hist_kernel<CONC>, dim3(blocks), dim3(256), 0, s, p, (unsigned long long*)hist);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

extern "C" long s2s_stain_moments_slots(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30)) return S2S_ERR_SHAPE;
  return (long)B * cdiv(H, SN_CH) * cdiv(W, SN_CW);
}

extern "C" int s2s_stain_moments_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h,
                                    int H, int W, const int* q_table, int u_beta, int black, long* part,
                                    void* stream) {
  if (!q_table || !part) return S2S_ERR_NULL;
  SnMomentParams mp;
  const float none[1] = {0.0f};
  float od[256];
  for (int i = 0; i < 256; ++i) od[i] = 0.0f;
  const int rc = sn_fill(mp.p, img, pitch, img_stride, B, band_top, band_h, H, W, od, none, 0, u_beta, black);
  if (rc != S2S_OK) return rc;
  // a band is whole chunk rows: it starts on one, and ends on one or with the image
  if (band_top % SN_CH != 0 || (band_h % SN_CH != 0 && band_top + band_h != H)) return S2S_ERR_SHAPE;
  const int ng = cdiv(band_h, SN_CH);
  if (ng > 65535) return S2S_ERR_SHAPE;
  for (int i = 0; i < 256; ++i) mp.q[i] = q_table[i];
  static_assert(sizeof(long) == sizeof(long long), "int64 partials");
  hipLaunchKernelGGL(sn_moments_kernel, dim3((unsigned)mp.p.ncx, (unsigned)ng, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, mp, (long long*)part);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_moments_finalize(const long* part, long nslots, long* out, void* stream) {
  if (!part || !out) return S2S_ERR_NULL;
  if (nslots < 1 || nslots > (1L << 40)) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(sn_moments_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long long*)part,
                     nslots, (long long*)out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_angle_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h,
                                       int H, int W, const float* od_table, const float* plane, int u_beta, int black,
                                       int reset, long* hist, void* stream) {
  return sn_hist<false>(img, pitch, img_stride, B, band_top, band_h, H, W, od_table, plane, 6, u_beta, black, reset,
                        hist, stream);
}

extern "C" int s2s_stain_conc_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h,
                                      int H, int W, const float* od_table, const float* unmix, int u_beta, int black,
                                      int reset, long* hist, void* stream) {
  return sn_hist<true>(img, pitch, img_stride, B, band_top, band_h, H, W, od_table, unmix, 9, u_beta, black, reset,
                       hist, stream);
}

extern "C" int s2s_stain_normalize_u8(const void* img, long pitch, long img_stride, int B, int H, int W,
                                      const float* od_table, const float* coef, void* out, long out_pitch,
                                      long out_img, int out_f32, void* stream) {
  if (!out) return S2S_ERR_NULL;
  SnParams p;
  const int rc = sn_fill(p, img, pitch, img_stride, B, 0, H, H, W, od_table, coef, 17, 255, 0);
  if (rc != S2S_OK) return rc;
  if (!out_f32 && (out_pitch < 3L * W || (B > 1 && out_img < out_pitch * (long)H))) return S2S_ERR_SHAPE;
  const unsigned blocks = sn_blocks((long)B * H * cdiv(W, 4), SN_APPLY_BLOCKS);
  if (!blocks) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (out_f32) hipLaunchKernelGGL(sn_apply_kernel<true>, dim3(blocks), dim3(256), 0, s, p, out, 0L, 0L);
  else hipLaunchKernelGGL(sn_apply_kernel<false>, dim3(blocks), dim3(256), 0, s, p, out, out_pitch, out_img);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
