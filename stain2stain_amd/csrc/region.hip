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
