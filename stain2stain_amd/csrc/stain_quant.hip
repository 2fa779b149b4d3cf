// Stain quantification: colour deconvolution (Ruifrok & Johnston 2001) and the positive-area burden, per sample, per
// map cell of a whole region, and paired (generated against real).  DESIGN.md section 3.17.
//
//   s2s_stain_quant_u8        uint8 HWC RGB images of any row pitch; a second image makes it the paired form, which reads
//                             both once; the buffers may hold a band of rows of a taller image (region_stain_map streams a
//                             host region through such bands)
//   s2s_stain_quant_f32       fp32 NCHW (C = 3) in the network's range, through the save conversion of region.hip:
//                             u = trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255)): what one measures from the saved PNG
//   s2s_stain_quant_finalize  partials -> int64 counts, fp64 sums, fp32 burdens / mean ODs (single) or burdens, their
//                             absolute difference, Dice and IoU of the positive masks (paired)
//   s2s_stain_separate        uint8 or fp32 in, fp32 [B][3][H][W] concentrations out
//   s2s_stain_mask_u8 / _f32  the positive mask of one stain as bytes: bit 0 = positive, bit 1 = tissue; the tissue count
//                             per sample on the side (what objects.hip labels)
//
// Definition.  od(u) = -log10(max(u, 1) / 255) comes from a 256-entry fp32 table the host computes in double (no device
// log); the table lives in LDS.  c_k = ((od_r * m_rk) + (od_g * m_gk)) + (od_b * m_bk), every product and sum rounded on
// its own, m the fp32 inverse of the stain basis (nine kernel arguments).  A pixel is tissue by the rule of
// s2s_region_tissue_count (is_tissue, common.h) and positive for stain k iff it is tissue and c_k > thr_k.  A numpy
// float32 restatement is bit-equal, so every count is an exact integer.
//
// An OWNER is one sample, or one cell_h x cell_w cell of one sample (the heat map; ragged edge cells count their own
// pixels only).  A cell is cut into fixed chunks of SQ_CH rows x SQ_CW columns; a workgroup reduces one chunk, so it
// never spans two owners.  One thread consumes all three bytes of a pixel (four pixels: three dword loads where the
// twelve bytes are 4-byte aligned, bytes otherwise).  Per owner: the tissue count, the positive count per stain and the
// fp64 sum of max(c_k, 0) over tissue per stain; the paired form: both tissue counts and, for one chosen stain, the
// pixels positive in both, in the prediction only and in the target only.  Partials go through a wave butterfly, then a
// fixed order across the four waves, and are stored per chunk at a place that depends on the chunk's position in the
// WHOLE image alone: no atomics, bit-equal run to run, independent of batch mates and of the banding.
//
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int SQ_CH = 16, SQ_CW = 1024;      // rows x columns of one workgroup's chunk (stain_quant.CHUNK_ROWS is SQ_CH)
constexpr int SQ_K1 = 7, SQ_K2 = 5;          // 8-byte partial slots per chunk: single / paired

enum { SQ_U8 = 0, SQ_F32 = 1 };

struct SqParams {
  const void* a;
  const void* b;              // paired form only
  long pitch_a, img_a;        // row pitch and sample stride: bytes (uint8) or elements (fp32)
  long pitch_b, img_b;
  long chan;                  // fp32: elements per channel plane
  int H, W;                   // the whole image
  int band_top;               // image row of the buffers' first row
  int cell_h, cell_w, Gy, Gx; // the owners' grid
  int ncy, ncx;               // chunks per cell
  int g0;                     // first chunk row (gy * ncy + cy) of this launch
  int white, black, stain;
  float m[9];                 // m[3 * channel + stain]
  float thr[3];
  float od[256];
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the save conversion of region_finalize_kernel / image_quality(quantize=True)
__device__ __forceinline__ unsigned sq_quantise(float x) {
#pragma clang fp contract(off)
  const float h = x * 0.5f;
  const float u = (h + 0.5f) * 255.0f;
  return (unsigned)(int)fminf(fmaxf(u, 0.0f), 255.0f);
}

// px (1..4) consecutive pixels of one row from column x0 on: v[3 j + c]
template <int LOADER>
__device__ __forceinline__ void sq_load_quad(const void* base, long row_off, long chan, int x0, int px, unsigned* v) {
  if (LOADER == SQ_U8) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + row_off + 3L * x0;
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
  } else {
    const float* p = reinterpret_cast<const float*>(base) + row_off + x0;
    if (px == 4 && ((uintptr_t)p & 15) == 0 && (chan & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p + c * chan);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[3 * j + c] = sq_quantise(q[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = sq_quantise(p[c * chan + j]);
        }
      }
    }
  }
}

// hipcc contracts a * b + c into an fma by default, through __fmul_rn / __fadd_rn too (their operators sit in a header,
// out of a pragma's reach): plain operators under the pragma, as in region_finalize_kernel, keep every product and sum
// rounded on its own
__device__ __forceinline__ float sq_conc(const SqParams& p, float odr, float odg, float odb, int k) {
#pragma clang fp contract(off)
  const float pr = odr * p.m[k], pg = odg * p.m[3 + k], pb = odb * p.m[6 + k];
  const float s = pr + pg;
  return s + pb;
}

// THE rule: positive for stain k iff tissue and c_k > thr_k (every kernel here decides through this one statement)
__device__ __forceinline__ int sq_positive(const SqParams& p, int t, float c, int k) { return (t && c > p.thr[k]) ? 1 : 0; }

__device__ __forceinline__ void sq_table_to_lds(const SqParams& p, float* lut) {
  lut[threadIdx.x] = p.od[threadIdx.x];        // 256 lanes, 256 entries
  __syncthreads();
}

// offset of row y of sample n: uint8 rows are relative to the band, fp32 images are whole
template <int LOADER>
__device__ __forceinline__ long sq_row(long img, long pitch, int n, int y, int band_top) {
  return (long)n * img + (long)(y - (LOADER == SQ_U8 ? band_top : 0)) * pitch;
}

template <int LOADER, bool PAIRED>
__global__ __launch_bounds__(256) void sq_reduce_kernel(const SqParams p, double* __restrict__ part) {
  __shared__ float lut[256];
  __shared__ double redd[4][3];
  __shared__ int redi[4][5];
  const int tid = threadIdx.x;
  sq_table_to_lds(p, lut);
  const int gx = blockIdx.x / p.ncx, cx = blockIdx.x - gx * p.ncx;
  const int g = p.g0 + blockIdx.y, gy = g / p.ncy, cy = g - gy * p.ncy;
  const int n = blockIdx.z;
  const long top = (long)gy * p.cell_h + (long)cy * SQ_CH, left = (long)gx * p.cell_w + (long)cx * SQ_CW;
  const long bottom = min(min(top + SQ_CH, ((long)gy + 1) * p.cell_h), (long)p.H);
  const long right = min(min(left + SQ_CW, ((long)gx + 1) * p.cell_w), (long)p.W);
  const int hh = (int)max(bottom - top, 0L), ww = (int)max(right - left, 0L);   // an empty chunk writes zeros
  const int nq = (ww + 3) >> 2;
  const int total = hh * nq;
  int ci[5] = {0, 0, 0, 0, 0};
  double cd[3] = {0.0, 0.0, 0.0};
  for (int q = tid; q < total; q += 256) {
    const int y = q / nq, xq = q - y * nq;
    const int x0 = (int)left + 4 * xq, px = min(4, ww - 4 * xq);
    unsigned va[12], vb[12];
    sq_load_quad<LOADER>(p.a, sq_row<LOADER>(p.img_a, p.pitch_a, n, (int)top + y, p.band_top), p.chan, x0, px, va);
    if (PAIRED)
      sq_load_quad<LOADER>(p.b, sq_row<LOADER>(p.img_b, p.pitch_b, n, (int)top + y, p.band_top), p.chan, x0, px, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const unsigned r = va[3 * j], gg = va[3 * j + 1], b = va[3 * j + 2];
        const int t = is_tissue(r, gg, b, p.white, p.black);
        const float odr = lut[r], odg = lut[gg], odb = lut[b];
        if (!PAIRED) {
          ci[0] += t;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float c = sq_conc(p, odr, odg, odb, k);
            ci[1 + k] += sq_positive(p, t, c, k);
            cd[k] += t ? (double)fmaxf(c, 0.0f) : 0.0;
          }
        } else {
          const unsigned r2 = vb[3 * j], g2 = vb[3 * j + 1], b2 = vb[3 * j + 2];
          const int t2 = is_tissue(r2, g2, b2, p.white, p.black);
          const int k = p.stain;
          const float ca = sq_conc(p, odr, odg, odb, k), cb = sq_conc(p, lut[r2], lut[g2], lut[b2], k);
          const int pa = sq_positive(p, t, ca, k), pb = sq_positive(p, t2, cb, k);
          ci[0] += t;
          ci[1] += t2;
          ci[2] += pa & pb;
          ci[3] += pa & (pb ^ 1);
          ci[4] += pb & (pa ^ 1);
        }
      }
    }
  }
  constexpr int NI = PAIRED ? 5 : 4;
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < NI; ++k) {
    const int s = wave_sum_i(ci[k]);
    if (lane == 0) redi[wv][k] = s;
  }
  if (!PAIRED) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double s = wave_sum_d(cd[k]);
      if (lane == 0) redd[wv][k] = s;
    }
  }
  __syncthreads();
  constexpr int K = PAIRED ? SQ_K2 : SQ_K1;
  if (tid < K) {
    const long owner = ((long)n * p.Gy + gy) * p.Gx + gx;
    const long slot = ((owner * p.ncy + cy) * p.ncx + cx) * K + tid;
    if (tid < NI) {
      const long long s = (long long)redi[0][tid] + redi[1][tid] + redi[2][tid] + redi[3][tid];
      part[slot] = __longlong_as_double(s);
    } else {
      const int k = tid - NI;
      part[slot] = ((redd[0][k] + redd[1][k]) + redd[2][k]) + redd[3][k];
    }
  }
}

// one workgroup per owner: thread t adds partials t, t + 256, ... in order, then a fixed tree
template <bool PAIRED>
__global__ __launch_bounds__(256) void sq_finalize_kernel(const double* __restrict__ part, int nchunk,
                                                          long long* __restrict__ counts, double* __restrict__ sums,
                                                          float* __restrict__ out) {
  constexpr int NI = PAIRED ? 5 : 4, ND = PAIRED ? 0 : 3, K = NI + ND;
  __shared__ long long ri[5][256];
  __shared__ double rd[3][256];
  const int o = blockIdx.x, tid = threadIdx.x;
  long long si[5] = {0, 0, 0, 0, 0};
  double sd[3] = {0.0, 0.0, 0.0};
  const double* pp = part + (long)o * nchunk * K;
  for (int i = tid; i < nchunk; i += 256) {
#pragma unroll
    for (int k = 0; k < NI; ++k) si[k] += __double_as_longlong(pp[(long)i * K + k]);
#pragma unroll
    for (int k = 0; k < ND; ++k) sd[k] += pp[(long)i * K + NI + k];
  }
#pragma unroll
  for (int k = 0; k < NI; ++k) ri[k][tid] = si[k];
#pragma unroll
  for (int k = 0; k < ND; ++k) rd[k][tid] = sd[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < NI; ++k) ri[k][tid] += ri[k][tid + s];
#pragma unroll
      for (int k = 0; k < ND; ++k) rd[k][tid] += rd[k][tid + s];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  if (!PAIRED) {
    const double den = (double)max(ri[0][0], 1LL);
    counts[(long)o * 4] = ri[0][0];
    for (int k = 0; k < 3; ++k) {
      counts[(long)o * 4 + 1 + k] = ri[1 + k][0];
      sums[(long)o * 3 + k] = rd[k][0];
      out[(long)o * 6 + k] = (float)((double)ri[1 + k][0] / den);
      out[(long)o * 6 + 3 + k] = (float)(rd[k][0] / den);
    }
  } else {
    const long long ta = ri[0][0], tb = ri[1][0], both = ri[2][0], oa = ri[3][0], ob = ri[4][0];
    for (int k = 0; k < 5; ++k) counts[(long)o * 5 + k] = ri[k][0];
    const double ba = (double)(both + oa) / (double)max(ta, 1LL), bb = (double)(both + ob) / (double)max(tb, 1LL);
    const long long uni = both + oa + ob;
    out[(long)o * 5] = (float)ba;
    out[(long)o * 5 + 1] = (float)bb;
    out[(long)o * 5 + 2] = (float)fabs(ba - bb);
    out[(long)o * 5 + 3] = uni == 0 ? 1.0f : (float)(2.0 * (double)both / (double)(2 * both + oa + ob));
    out[(long)o * 5 + 4] = uni == 0 ? 1.0f : (float)((double)both / (double)uni);
  }
}

// One thread per 4 consecutive pixels of one row; a 16-byte store per stain plane where the row allows it.
template <int LOADER>
__global__ __launch_bounds__(256) void sq_separate_kernel(const SqParams p, int B, float* __restrict__ out) {
  __shared__ float lut[256];
  sq_table_to_lds(p, lut);
  const int nq = (p.W + 3) >> 2;
  const long plane = (long)p.H * p.W;
  const long total = (long)B * p.H * nq;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int xq = (int)(q % nq);
    const long t = q / nq;
    const int y = (int)(t % p.H), n = (int)(t / p.H);
    const int x0 = 4 * xq, px = min(4, p.W - x0);
    unsigned v[12];
    sq_load_quad<LOADER>(p.a, sq_row<LOADER>(p.img_a, p.pitch_a, n, y, 0), p.chan, x0, px, v);
    float c[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const float odr = lut[v[3 * j]], odg = lut[v[3 * j + 1]], odb = lut[v[3 * j + 2]];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k][j] = sq_conc(p, odr, odg, odb, k);
      }
    }
    float* o = out + (long)n * 3 * plane + (long)y * p.W + x0;
    if (px == 4 && ((uintptr_t)o & 15) == 0 && (plane & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) *reinterpret_cast<f32x4*>(o + k * plane) = f32x4{c[k][0], c[k][1], c[k][2], c[k][3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) {
#pragma unroll
          for (int k = 0; k < 3; ++k) o[k * plane + j] = c[k][j];
        }
      }
    }
  }
}

// One thread per 4 consecutive pixels of one row: mask byte = positive | tissue << 1 for stain p.stain; tissue[n] += the
// tissue pixels (an integer atomic per workgroup; the caller zeroes it, and the bands of a region add up in it).
template <int LOADER>
__global__ __launch_bounds__(256) void sq_mask_kernel(const SqParams p, int band_h, unsigned char* __restrict__ mask,
                                                      long mpitch, long mimg, unsigned long long* tissue) {
  __shared__ float lut[256];
  __shared__ int red[4];
  sq_table_to_lds(p, lut);
  const int n = blockIdx.y, nq = (p.W + 3) >> 2, k = p.stain;
  const long total = (long)band_h * nq;
  int nt = 0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int xq = (int)(q % nq), y = p.band_top + (int)(q / nq);
    const int x0 = 4 * xq, px = min(4, p.W - x0);
    unsigned v[12];
    sq_load_quad<LOADER>(p.a, sq_row<LOADER>(p.img_a, p.pitch_a, n, y, p.band_top), p.chan, x0, px, v);
    unsigned bytes = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const int t = is_tissue(v[3 * j], v[3 * j + 1], v[3 * j + 2], p.white, p.black);
        const float c = sq_conc(p, lut[v[3 * j]], lut[v[3 * j + 1]], lut[v[3 * j + 2]], k);
        bytes |= (unsigned)(sq_positive(p, t, c, k) | (t << 1)) << (8 * j);
        nt += t;
      }
    }
    unsigned char* o = mask + (long)n * mimg + (long)y * mpitch + x0;
    if (px == 4 && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<unsigned*>(o) = bytes;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) o[j] = (unsigned char)(bytes >> (8 * j));
      }
    }
  }
  nt = wave_sum_i(nt);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = nt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(tissue + n, (unsigned long long)s);
  }
}

template <int LOADER>
void sq_mask_launch(const SqParams& p, int B, int band_h, void* mask, long mpitch, long mimg, long* tissue, hipStream_t s) {
  long blocks = ((long)band_h * cdiv(p.W, 4) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(sq_mask_kernel<LOADER>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, p, band_h,
                     (unsigned char*)mask, mpitch, mimg, (unsigned long long*)tissue);
}

int sq_fill(SqParams& p, int H, int W, int cell_h, int cell_w, const float* od_table, const float* unmix, int white,
            int black, int stain) {
  if (!od_table || !unmix) return S2S_ERR_NULL;
  if (H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || cell_h < 1 || cell_w < 1 || cell_h > (1 << 30) ||
      cell_w > (1 << 30) || white < 1 || white > 256 || black < 0 || black > 255 || stain < 0 || stain > 2)
    return S2S_ERR_SHAPE;
  p.H = H;
  p.W = W;
  p.cell_h = cell_h;
  p.cell_w = cell_w;
  p.Gy = cdiv(H, cell_h);
  p.Gx = cdiv(W, cell_w);
  p.ncy = cdiv(cell_h, SQ_CH);
  p.ncx = cdiv(cell_w, SQ_CW);
  if ((long)p.Gy * p.ncy > (1L << 30) || (long)p.Gx * p.ncx > (1L << 30)) return S2S_ERR_SHAPE;
  p.white = white;
  p.black = black;
  p.stain = stain;
  for (int i = 0; i < 9; ++i) p.m[i] = unmix[i];
  for (int i = 0; i < 3; ++i) p.thr[i] = unmix[9 + i];
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  p.b = nullptr;
  p.pitch_b = p.img_b = 0;
  p.chan = 0;
  p.band_top = 0;
  p.g0 = 0;
  return S2S_OK;
}

template <int LOADER>
void sq_launch(const SqParams& p, int ng, int B, double* part, hipStream_t s) {
  const dim3 grid((unsigned)(p.Gx * p.ncx), (unsigned)ng, (unsigned)B);
  if (p.b) hipLaunchKernelGGL((sq_reduce_kernel<LOADER, true>), grid, dim3(256), 0, s, p, part);
  else hipLaunchKernelGGL((sq_reduce_kernel<LOADER, false>), grid, dim3(256), 0, s, p, part);
}

}  // namespace

extern "C" int s2s_stain_quant_chunks(int cell_h, int cell_w) {
  if (cell_h < 1 || cell_w < 1 || cell_h > (1 << 30) || cell_w > (1 << 30)) return S2S_ERR_SHAPE;
  const long n = (long)cdiv(cell_h, SQ_CH) * cdiv(cell_w, SQ_CW);
  return n > (1L << 30) ? S2S_ERR_SHAPE : (int)n;
}

extern "C" int s2s_stain_quant_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b,
                                  int paired, int B, int band_top, int band_h, int H, int W, int cell_h, int cell_w,
                                  int g0, int ng, const float* od_table, const float* unmix, int white, int black,
                                  int stain, double* part, void* stream) {
  if (!a || !part || (paired && !b)) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  SqParams p;
  const int rc = sq_fill(p, H, W, cell_h, cell_w, od_table, unmix, white, black, stain);
  if (rc != S2S_OK) return rc;
  if (pitch_a < 3L * W || (paired && pitch_b < 3L * W) || g0 < 0 || ng < 1 || ng > 65535 ||
      (long)g0 + ng > (long)p.Gy * p.ncy)
    return S2S_ERR_SHAPE;
  if (band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && (img_a < pitch_a * (long)band_h || (paired && img_b < pitch_b * (long)band_h))) return S2S_ERR_SHAPE;
  // the buffers must hold every row these chunk rows read
  const int gl = g0 + ng - 1;
  const long first = (long)(g0 / p.ncy) * cell_h + (long)(g0 % p.ncy) * SQ_CH;
  long last = (long)(gl / p.ncy) * cell_h + (long)(gl % p.ncy) * SQ_CH + SQ_CH;
  if (last > ((long)(gl / p.ncy) + 1) * cell_h) last = ((long)(gl / p.ncy) + 1) * cell_h;
  if (last > H) last = H;
  if (band_top > first || (long)band_top + band_h < last) return S2S_ERR_SHAPE;
  p.a = a;
  p.pitch_a = pitch_a;
  p.img_a = img_a;
  if (paired) {
    p.b = b;
    p.pitch_b = pitch_b;
    p.img_b = img_b;
  }
  p.band_top = band_top;
  p.g0 = g0;
  sq_launch<SQ_U8>(p, ng, B, part, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_quant_f32(const float* a, const float* b, int paired, int B, int H, int W,
                                   const float* od_table, const float* unmix, int white, int black, int stain,
                                   double* part, void* stream) {
  if (!a || !part || (paired && !b)) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  SqParams p;
  const int rc = sq_fill(p, H, W, H, W, od_table, unmix, white, black, stain);
  if (rc != S2S_OK) return rc;
  if (p.ncy > 65535) return S2S_ERR_SHAPE;
  p.a = a;
  p.pitch_a = p.pitch_b = W;
  p.chan = (long)H * W;
  p.img_a = p.img_b = 3L * H * W;
  if (paired) p.b = b;
  sq_launch<SQ_F32>(p, p.ncy, B, part, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_quant_finalize(const double* part, long owners, int nchunk, int paired, long* counts,
                                        double* sums, float* out, void* stream) {
  if (!part || !counts || !out || (!paired && !sums)) return S2S_ERR_NULL;
  if (owners < 1 || owners > 0x7fffffffL || nchunk < 1 || nchunk > (1 << 30)) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  hipStream_t s = (hipStream_t)stream;
  if (paired)
    hipLaunchKernelGGL(sq_finalize_kernel<true>, dim3((unsigned)owners), dim3(256), 0, s, part, nchunk,
                       (long long*)counts, sums, out);
  else
    hipLaunchKernelGGL(sq_finalize_kernel<false>, dim3((unsigned)owners), dim3(256), 0, s, part, nchunk,
                       (long long*)counts, sums, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_separate(const void* img, int is_f32, long pitch, long img_stride, int B, int H, int W,
                                  const float* od_table, const float* unmix, float* out, void* stream) {
  if (!img || !out) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  SqParams p;
  const int rc = sq_fill(p, H, W, H, W, od_table, unmix, 256, 0, 0);
  if (rc != S2S_OK) return rc;
  const long row = is_f32 ? (long)W : 3L * W;
  if (pitch < row || (B > 1 && img_stride < (is_f32 ? 3L : 1L) * pitch * H)) return S2S_ERR_SHAPE;
  p.a = img;
  p.pitch_a = pitch;
  p.img_a = img_stride;
  p.chan = is_f32 ? pitch * H : 0;
  long blocks = ((long)B * H * cdiv(W, 4) + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (is_f32) hipLaunchKernelGGL(sq_separate_kernel<SQ_F32>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, B, out);
  else hipLaunchKernelGGL(sq_separate_kernel<SQ_U8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, B, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_mask_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H,
                                 int W, const float* od_table, const float* unmix, int white, int black, int stain,
                                 void* mask, long mask_pitch, long mask_stride, long* tissue, void* stream) {
  if (!img || !mask || !tissue) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  SqParams p;
  const int rc = sq_fill(p, H, W, H, W, od_table, unmix, white, black, stain);
  if (rc != S2S_OK) return rc;
  if (pitch < 3L * W || mask_pitch < W || band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && (img_stride < pitch * (long)band_h || mask_stride < mask_pitch * (long)H)) return S2S_ERR_SHAPE;
  p.a = img;
  p.pitch_a = pitch;
  p.img_a = img_stride;
  p.band_top = band_top;
  sq_mask_launch<SQ_U8>(p, B, band_h, mask, mask_pitch, mask_stride, tissue, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_mask_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix,
                                  int white, int black, int stain, void* mask, long mask_pitch, long mask_stride,
                                  long* tissue, void* stream) {
  if (!img || !mask || !tissue) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  SqParams p;
  const int rc = sq_fill(p, H, W, H, W, od_table, unmix, white, black, stain);
  if (rc != S2S_OK) return rc;
  if (mask_pitch < W || (B > 1 && mask_stride < mask_pitch * (long)H)) return S2S_ERR_SHAPE;
  p.a = img;
  p.pitch_a = W;
  p.chan = (long)H * W;
  p.img_a = 3L * H * W;
  sq_mask_launch<SQ_F32>(p, B, H, mask, mask_pitch, mask_stride, tissue, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
