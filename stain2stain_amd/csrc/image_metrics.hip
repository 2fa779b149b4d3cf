// Image-quality metrics of generated tiles and whole regions against their targets: per-sample MSE, MAE, PSNR and
// SSIM (Wang et al. 2004: separable Gaussian window, biased local moments, valid positions only), one fused pass.
//
//   s2s_image_quality_f32       fp32 NCHW pairs in the network's normalised range, C in 1..4
//                                 quantize = 0: v = clamp(x * 0.5 + 0.5, 0, 1), L = 1
//                                 quantize = 1: v = trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)), L = 255 (the save
//                                               conversion of region.hip: the numbers one measures from the saved PNGs)
//   s2s_image_quality_u8        uint8 HWC RGB pairs with a row pitch per image, L = 255; the buffers may hold a band of
//                               rows of a taller image (region_quality streams a host region through such bands)
//   s2s_image_quality_finalize  partials -> out[4][B] = psnr, ssim, mae, mse
//
// A workgroup owns IQ_TH x IQ_TW valid SSIM positions of one sample.  Per channel it stages the block plus the
// window's halo of both images in LDS, runs the horizontal and then the vertical Gaussian over the five moments
// (a, b, a^2, b^2, ab) -- no blurred map goes to memory -- and forms SSIM per position.  The squared and absolute
// differences are taken while staging, from the pixels the block OWNS: the centres of its valid positions, and for the
// blocks on the rim of the image also the border rows / columns that are no valid position, so every pixel is counted
// exactly once.  Sums are fp64; a block writes three partials (no atomics), the finalize pass adds a sample's partials
// in a fixed order: bit-equal run to run, and a sample's result does not depend on its batch mates.  The partials of a
// region are indexed by the block's position in the WHOLE image, so the result does not depend on the banding either.
//
// Second moments are taken of centred data: E[x^2] - mu^2 in fp32 loses |mu|^2 * 2^-24, which on a flat bright area is
// most of the variance.  Variances and the covariance are shift invariant, so a block subtracts, per channel and image,
// the value of the pixel in the middle of its staged tile (any constant would do; L/2 only buys a factor of 4 on
// bright areas, the local value leaves |mu| at the size of the local contrast) and gives it back to the means.
//
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int IQ_TW = 32, IQ_TH = 32;        // valid positions per block (image_metrics.BLOCK_ROWS is IQ_TH)
constexpr int IQ_MAXWIN = 11;
constexpr int IQ_SH = IQ_TH + IQ_MAXWIN - 1, IQ_SW = IQ_TW + IQ_MAXWIN - 1;
constexpr int IQ_STRIP = 4;                  // output rows per thread of the vertical pass (256 threads = 32 x 8 strips)

enum { IQ_F32_UNIT = 0, IQ_F32_QUANT = 1, IQ_U8 = 2 };

struct IqParams {
  const void* a;
  const void* b;
  long pitch_a, pitch_b;      // row pitch: bytes (uint8) or elements (fp32)
  long img_a, img_b;          // sample stride, same unit
  long chan;                  // fp32: elements per channel plane
  int C, H, W;                // H, W of the whole image
  int band_top;               // image row of the buffers' first row
  int by0, nby_total, nbx;    // first block row of this launch; block rows / columns of the whole image
  int win;
  float c1, c2;
  float g[IQ_MAXWIN];
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int LOADER>
__device__ __forceinline__ float iq_load(const void* base, long off, int x, int c) {
  if (LOADER == IQ_U8) return (float)reinterpret_cast<const unsigned char*>(base)[off + 3 * (long)x + c];
  const float v = reinterpret_cast<const float*>(base)[off + x];
  const float u = __fadd_rn(__fmul_rn(v, 0.5f), 0.5f);
  if (LOADER == IQ_F32_UNIT) return fminf(fmaxf(u, 0.0f), 1.0f);
  return (float)(int)fminf(fmaxf(__fmul_rn(u, 255.0f), 0.0f), 255.0f);
}

// identical a and b give exactly 1: every product and sum below is rounded on its own (no contraction), so the
// numerator and the denominator are then the same numbers
__device__ __forceinline__ float iq_ssim(float ma, float mb, float saa, float sbb, float sab, float pa, float pb,
                                         float c1, float c2) {
  const float va = __fmaf_rn(-ma, ma, saa), vb = __fmaf_rn(-mb, mb, sbb), cov = __fmaf_rn(-ma, mb, sab);
  const float ua = __fadd_rn(ma, pa), ub = __fadd_rn(mb, pb);
  const float n1 = __fadd_rn(__fmul_rn(__fmul_rn(2.0f, ua), ub), c1);
  const float d1 = __fadd_rn(__fadd_rn(__fmul_rn(ua, ua), __fmul_rn(ub, ub)), c1);
  const float n2 = __fadd_rn(__fmul_rn(2.0f, cov), c2);
  const float d2 = __fadd_rn(__fadd_rn(va, vb), c2);
  return __fmul_rn(n1, n2) / __fmul_rn(d1, d2);
}

// WINT: the window size at compile time (the default 11: both passes fully unrolled), 0: p.win at run time
template <int LOADER, int WINT>
__global__ __launch_bounds__(256) void iq_block_kernel(const IqParams p, double* __restrict__ part) {
  __shared__ float sa[IQ_SH][IQ_SW + 1], sb[IQ_SH][IQ_SW + 1];
  __shared__ float hm[5][IQ_SH][IQ_TW];
  __shared__ double red[4][3];
  const int tid = threadIdx.x;
  const int win = WINT ? WINT : p.win;
  const int halo = win - 1, r = win >> 1;
  const int bx = blockIdx.x, by = p.by0 + blockIdx.y, n = blockIdx.z;
  const int Hv = p.H - halo, Wv = p.W - halo;
  const int y0 = by * IQ_TH, x0 = bx * IQ_TW;                 // first valid position = first staged pixel
  const int vh = min(IQ_TH, Hv - y0), vw = min(IQ_TW, Wv - x0);
  const int sh = vh + halo, sw = vw + halo;                   // staged pixels: rows y0 .. y0 + sh - 1 < H
  // owned pixels, in tile coordinates
  const int oy0 = by == 0 ? 0 : r, oy1 = (y0 + vh == Hv) ? sh : vh + r;
  const int ox0 = bx == 0 ? 0 : r, ox1 = (x0 + vw == Wv) ? sw : vw + r;
  const long row0 = (long)(y0 - p.band_top);
  double s_ssim = 0.0, s_sq = 0.0, s_abs = 0.0;
  for (int c = 0; c < p.C; ++c) {
    const long ca = (long)n * p.img_a + (LOADER == IQ_U8 ? 0 : (long)c * p.chan) + row0 * p.pitch_a;
    const long cb = (long)n * p.img_b + (LOADER == IQ_U8 ? 0 : (long)c * p.chan) + row0 * p.pitch_b;
    // the pivots: the middle pixel of the staged tile (one address for the whole block)
    const float pa = iq_load<LOADER>(p.a, ca + (long)(sh >> 1) * p.pitch_a, x0 + (sw >> 1), c);
    const float pb = iq_load<LOADER>(p.b, cb + (long)(sh >> 1) * p.pitch_b, x0 + (sw >> 1), c);
    for (int i = tid; i < sh * sw; i += 256) {
      const int ty = i / sw, tx = i - ty * sw;
      const float a = iq_load<LOADER>(p.a, ca + (long)ty * p.pitch_a, x0 + tx, c);
      const float b = iq_load<LOADER>(p.b, cb + (long)ty * p.pitch_b, x0 + tx, c);
      if (ty >= oy0 && ty < oy1 && tx >= ox0 && tx < ox1) {
        const double d = (double)__fsub_rn(a, b);
        s_sq += d * d;
        s_abs += fabs(d);
      }
      sa[ty][tx] = a - pa;
      sb[ty][tx] = b - pb;
    }
    __syncthreads();
    // horizontal pass: hm[m][row][col], every staged row, the block's vw columns
    for (int i = tid; i < sh * IQ_TW; i += 256) {
      const int ty = i / IQ_TW, tx = i % IQ_TW;
      if (tx < vw) {
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < (WINT ? WINT : IQ_MAXWIN); ++k) {
          if (WINT || k < win) {
            const float g = p.g[k], a = sa[ty][tx + k], b = sb[ty][tx + k];
            const float ga = g * a, gb = g * b;
            m0 += ga;
            m1 += gb;
            m2 = fmaf(ga, a, m2);
            m3 = fmaf(gb, b, m3);
            m4 = fmaf(ga, b, m4);
          }
        }
        hm[0][ty][tx] = m0;
        hm[1][ty][tx] = m1;
        hm[2][ty][tx] = m2;
        hm[3][ty][tx] = m3;
        hm[4][ty][tx] = m4;
      }
    }
    __syncthreads();
    // vertical pass: a thread owns IQ_STRIP consecutive rows of one column and walks the rows they share once.  Rows
    // at or beyond sh hold stale data; they only reach outputs at or beyond vh, which are dropped.
    {
      const int col = tid % IQ_TW, q0 = (tid / IQ_TW) * IQ_STRIP;
      if (col < vw && q0 < vh) {
        float acc[IQ_STRIP][5];
#pragma unroll
        for (int q = 0; q < IQ_STRIP; ++q)
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[q][m] = 0.f;
        if (WINT) {
#pragma unroll
          for (int rr = 0; rr < IQ_STRIP + (WINT ? WINT : 1) - 1; ++rr) {
            float v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = hm[m][q0 + rr][col];
#pragma unroll
            for (int q = 0; q < IQ_STRIP; ++q) {
              const int k = rr - q;
              if (k >= 0 && k < (WINT ? WINT : 1)) {
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[q][m] = fmaf(p.g[k], v[m], acc[q][m]);
              }
            }
          }
        } else {
#pragma unroll
          for (int q = 0; q < IQ_STRIP; ++q)
            for (int k = 0; k < win; ++k) {
              const float g = p.g[k];
#pragma unroll
              for (int m = 0; m < 5; ++m) acc[q][m] = fmaf(g, hm[m][q0 + q + k][col], acc[q][m]);
            }
        }
#pragma unroll
        for (int q = 0; q < IQ_STRIP; ++q)
          if (q0 + q < vh)
            s_ssim += (double)iq_ssim(acc[q][0], acc[q][1], acc[q][2], acc[q][3], acc[q][4], pa, pb, p.c1, p.c2);
      }
    }
    // the next channel's staging overwrites sa / sb, last read before the barrier above; its horizontal pass
    // overwrites hm behind the barrier that follows the staging, which every thread reaches after this vertical pass
  }
  const int lane = tid & 63, wv = tid >> 6;
  const double r0 = wave_sum_d(s_ssim), r1 = wave_sum_d(s_sq), r2 = wave_sum_d(s_abs);
  if (lane == 0) { red[wv][0] = r0; red[wv][1] = r1; red[wv][2] = r2; }
  __syncthreads();
  if (tid < 3) {
    const long blk = ((long)n * p.nby_total + by) * p.nbx + bx;
    part[blk * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  }
}

// one workgroup per sample: thread t adds partials t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void iq_finalize_kernel(const double* __restrict__ part, long nblk, double n_px,
                                                          double n_valid, double range, int B,
                                                          float* __restrict__ out) {
  __shared__ double red[3][256];
  const int n = blockIdx.x, tid = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  const double* pp = part + (long)n * nblk * 3;
  for (long i = tid; i < nblk; i += 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += pp[i * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double mse = red[1][0] / n_px, mae = red[2][0] / n_px;
    out[n] = mse == 0.0 ? INFINITY : (float)(10.0 * log10(range * range / mse));
    out[B + n] = (float)(red[0][0] / n_valid);
    out[2 * B + n] = (float)mae;
    out[3 * B + n] = (float)mse;
  }
}

int iq_fill(IqParams& p, int H, int W, int win, const float* taps, float k1, float k2, float range) {
  if (!taps) return S2S_ERR_NULL;
  if (win < 1 || win > IQ_MAXWIN || !(win & 1) || H < win || W < win) return S2S_ERR_SHAPE;
  p.H = H;
  p.W = W;
  p.win = win;
  p.nby_total = cdiv(H - win + 1, IQ_TH);
  p.nbx = cdiv(W - win + 1, IQ_TW);
  p.c1 = (k1 * range) * (k1 * range);
  p.c2 = (k2 * range) * (k2 * range);
  for (int k = 0; k < IQ_MAXWIN; ++k) p.g[k] = k < win ? taps[k] : 0.f;
  return S2S_OK;
}

template <int LOADER>
void iq_launch(const IqParams& p, int nby, int B, double* part, hipStream_t s) {
  const dim3 grid(p.nbx, nby, B);
  if (p.win == IQ_MAXWIN) hipLaunchKernelGGL((iq_block_kernel<LOADER, IQ_MAXWIN>), grid, dim3(256), 0, s, p, part);
  else hipLaunchKernelGGL((iq_block_kernel<LOADER, 0>), grid, dim3(256), 0, s, p, part);
}

}  // namespace

extern "C" int s2s_image_quality_blocks(int H, int W, int win) {
  if (win < 1 || win > IQ_MAXWIN || !(win & 1) || H < win || W < win) return S2S_ERR_SHAPE;
  const long n = (long)cdiv(H - win + 1, IQ_TH) * cdiv(W - win + 1, IQ_TW);
  return n > (1L << 30) ? S2S_ERR_SHAPE : (int)n;
}

extern "C" int s2s_image_quality_f32(const float* a, const float* b, int B, int C, int H, int W, int quantize, int win,
                                     const float* taps, float k1, float k2, double* part, void* stream) {
  if (!a || !b || !part) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || C < 1 || C > 4) return S2S_ERR_SHAPE;
  IqParams p;
  const int rc = iq_fill(p, H, W, win, taps, k1, k2, quantize ? 255.0f : 1.0f);
  if (rc != S2S_OK) return rc;
  if (p.nby_total > 65535) return S2S_ERR_SHAPE;
  p.a = a;
  p.b = b;
  p.pitch_a = p.pitch_b = W;
  p.chan = (long)H * W;
  p.img_a = p.img_b = (long)C * H * W;
  p.C = C;
  p.band_top = 0;
  p.by0 = 0;
  if (quantize) iq_launch<IQ_F32_QUANT>(p, p.nby_total, B, part, (hipStream_t)stream);
  else iq_launch<IQ_F32_UNIT>(p, p.nby_total, B, part, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_image_quality_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b,
                                    int B, int band_top, int band_h, int H, int W, int by0, int nby, int win,
                                    const float* taps, float k1, float k2, double* part, void* stream) {
  if (!a || !b || !part) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  IqParams p;
  const int rc = iq_fill(p, H, W, win, taps, k1, k2, 255.0f);
  if (rc != S2S_OK) return rc;
  if (pitch_a < 3L * W || pitch_b < 3L * W || by0 < 0 || nby < 1 || nby > 65535 || by0 + nby > p.nby_total)
    return S2S_ERR_SHAPE;
  if (B > 1 && (img_a < pitch_a * (long)band_h || img_b < pitch_b * (long)band_h)) return S2S_ERR_SHAPE;
  // the buffers must hold every row these block rows stage
  const long first = (long)by0 * IQ_TH;
  long last = (long)(by0 + nby) * IQ_TH + win - 1;
  if (last > H) last = H;
  if (band_top < 0 || band_h < 1 || band_top > first || (long)band_top + band_h < last) return S2S_ERR_SHAPE;
  p.a = a;
  p.b = b;
  p.pitch_a = pitch_a;
  p.pitch_b = pitch_b;
  p.img_a = img_a;
  p.img_b = img_b;
  p.chan = 0;
  p.C = 3;
  p.band_top = band_top;
  p.by0 = by0;
  iq_launch<IQ_U8>(p, nby, B, part, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_image_quality_finalize(const double* part, int B, int C, int H, int W, int win, float range,
                                          float* out, void* stream) {
  if (!part || !out) return S2S_ERR_NULL;
  const int nblk = s2s_image_quality_blocks(H, W, win);
  if (nblk < 0 || B < 1 || B > 65535 || C < 1 || C > 4) return S2S_ERR_SHAPE;
  const double n_px = (double)C * H * W, n_valid = (double)C * (H - win + 1) * (W - win + 1);
  hipLaunchKernelGGL(iq_finalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, part, (long)nblk, n_px, n_valid,
                     (double)range, B, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
