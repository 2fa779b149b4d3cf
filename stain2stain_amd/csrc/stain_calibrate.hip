// Stain threshold calibration: exact integer histograms of the stain concentrations per owner, and the threshold rules
// (Otsu, triangle, quantiles; for pairs the burden-matching and the best-Dice threshold) evaluated on the device.
// DESIGN.md section 3.33.
//
//   s2s_stain_hist_u8 / _f32        hist long [owners][3][4096] += tissue pixels by bin(c_k), tissue long [owners] += them
//   s2s_stain_pair_hist_u8 / _f32   hist long [owners][4][4096] for one stain of a prediction a and a target b: a's tissue
//                                   by bin_a, b's tissue by bin_b, tissue in both by min(bin_a, bin_b), and (jt > 0) tissue
//                                   in both with bin_b >= jt by bin_a; tissue long [owners][2]
//   s2s_stain_thresholds            per histogram row: the suffix sums positive[j], Otsu, triangle and quantile bins
//   s2s_stain_pair_thresholds       per owner: the four suffix sums, the two Dice curves, the two matching rules
//
// Concentration and tissue are those of stain_quant.hip (the same table, the same three products and two sums under
// fp contract(off), the same save conversion for fp32 input).  bin(c) = clamp(ceil(c * 1024) - 1, 0, 4095) in fp32, so
// bin(c) >= j <=> c > j / 1024 for j in 1..4095: a suffix sum of the histogram IS the positive count at that threshold.
//
// An OWNER is one sample, or the whole batch (pool).  A workgroup never spans two owners: grid = (workgroups per owner,
// owners).  It keeps uint32 histograms in LDS, updates them with LDS integer atomics and flushes its non-empty bins with
// 64-bit integer atomics: integer sums, so the result is bit-equal run to run and for every split into bands or calls.
//
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int SC_NB = 4096;                  // histogram bins (stain_calibrate.NB)
constexpr float SC_BINS_PER_OD = 1024.0f;    // bin j starts right above j / 1024
constexpr int SC_CUS = 256, SC_LDS_PER_CU = 160 * 1024;       // the grid is sized to one resident round of workgroups
constexpr int SC_QUADS = 8;                  // quads a lane should at least have before another workgroup is worth its flush
constexpr long SC_MAX_PIXELS = 1L << 40;     // pixels of one owner in one launch
constexpr int SC_MAX_Q = 8;                  // quantiles of one s2s_stain_thresholds call
constexpr int SC_LUT_BYTES = 256 * 4, SC_HIST_BYTES = SC_NB * 4;

enum { SC_U8 = 0, SC_F32 = 1 };

struct ScParams {
  const void* a;
  const void* b;              // paired form only
  long pitch_a, img_a;        // row pitch and sample stride: bytes (uint8) or elements (fp32)
  long pitch_b, img_b;
  long chan;                  // fp32: elements per channel plane
  int rows, W;                // rows the buffers hold per sample (the band), columns
  int spo;                    // samples per owner: 1, or B when pooled
  int white, black;
  int ns, sel[3];             // single: the selected stains; paired: sel[0] is the stain
  int jt;                     // paired: the target's bin threshold, 0 = none
  float m[9];                 // m[3 * channel + stain]
  float od[256];
};

// the save conversion of region_finalize_kernel / image_quality(quantize=True)
__device__ __forceinline__ unsigned sc_quantise(float x) {
#pragma clang fp contract(off)
  const float h = x * 0.5f;
  const float u = (h + 0.5f) * 255.0f;
  return (unsigned)(int)fminf(fmaxf(u, 0.0f), 255.0f);
}

// px (1..4) consecutive pixels of one row from column x0 on: v[3 j + c] (the loads of sn_load_quad / sq_load_quad)
template <int LOADER>
__device__ __forceinline__ void sc_load_quad(const void* base, long row_off, long chan, int x0, int px, unsigned* v) {
  if (LOADER == SC_U8) {
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
        for (int j = 0; j < 4; ++j) v[3 * j + c] = sc_quantise(q[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = sc_quantise(p[c * chan + j]);
        }
      }
    }
  }
}

// ((od_r m_r) + (od_g m_g)) + (od_b m_b): plain operators under the pragma keep every product and sum rounded on its
// own (see sq_conc)
__device__ __forceinline__ float sc_conc(float odr, float odg, float odb, float mr, float mg, float mb) {
#pragma clang fp contract(off)
  const float pr = odr * mr, pg = odg * mg, pb = odb * mb;
  const float s = pr + pg;
  return s + pb;
}

// THE bin rule.  c is finite; c * 1024 is exact; ceil, minus one and the clamp act on a float, then one conversion
// (as sn_clamp_bin does with floor)
__device__ __forceinline__ int sc_bin(float c) {
#pragma clang fp contract(off)
  const float s = c * SC_BINS_PER_OD;
  const float t = ceilf(s) - 1.0f;
  return (int)fminf(fmaxf(t, 0.0f), (float)(SC_NB - 1));
}

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// quad q of an owner -> (sample, row, first column, pixels)
struct ScQuad {
  int n, y, x0, px;
};
__device__ __forceinline__ ScQuad sc_quad(const ScParams& p, int owner, long q, int nq, long per) {
  long s = 0, r = q;
  if (p.spo > 1) {                             // uniform: only a pooled batch pays for the 64-bit division
    s = q / per;
    r = q - s * per;
  }
  int y, xq;
  if (per <= 0x7fffffffL) {                    // uniform
    y = (int)((unsigned)r / (unsigned)nq);
    xq = (int)((unsigned)r - (unsigned)y * (unsigned)nq);
  } else {
    y = (int)(r / nq);
    xq = (int)(r - (long)y * nq);
  }
  return ScQuad{owner * p.spo + (int)s, y, 4 * xq, min(4, p.W - 4 * xq)};
}

// h[bin] += 1 for the lanes with act.  Where every such lane of the wave has the same bin (a flat image, a saturated
// channel) one lane adds their number: 64 atomics on one LDS address would be served one after the other.  Any other
// wave takes the plain atomic; its equal bins are few (Measured).
__device__ __forceinline__ void sc_lds_add(unsigned* h, int bin, bool act) {
  if (act) {
    const int b0 = __builtin_amdgcn_readfirstlane(bin);
    const unsigned long long lanes = __ballot(1), same = __ballot(bin == b0);
    if (same == lanes) {
      if ((int)__lane_id() == __ffsll((long long)lanes) - 1) atomicAdd(&h[b0], (unsigned)__popcll(lanes));
    } else {
      atomicAdd(&h[bin], 1u);
    }
  }
}

__global__ __launch_bounds__(256) void sc_zero_kernel(unsigned long long* __restrict__ hist, long n,
                                                      unsigned long long* __restrict__ tissue, int nt) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) hist[i] = 0ull;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < nt; i += 256) tissue[i] = 0ull;
  }
}

// adds the workgroup's tissue counts (cols per lane) to tissue[owner * cols + c]: wave butterfly, then the four waves
template <int COLS>
__device__ __forceinline__ void sc_flush_tissue(const int* nt, int* red, int owner, unsigned long long* tissue) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < COLS; ++c) {
    const int s = sc_wave_sum(nt[c]);
    if ((tid & 63) == 0) red[(tid >> 6) * COLS + c] = s;
  }
  __syncthreads();
  if (tid < COLS) {
    const long long s = (long long)red[tid] + red[COLS + tid] + red[2 * COLS + tid] + red[3 * COLS + tid];
    if (s) atomicAdd(tissue + (long)owner * COLS + tid, (unsigned long long)s);
  }
}

// LDS: the 256-entry table, then p.ns histograms of 4096 uint32.  A workgroup counts at most
// ceil(quads of its owner / gridDim.x) * 4 * 256 < 2^32 pixels (sc_blocks).
template <int LOADER>
__global__ __launch_bounds__(256) void sc_hist_kernel(const ScParams p, unsigned long long* __restrict__ hist,
                                                      unsigned long long* __restrict__ tissue) {
  extern __shared__ unsigned sc_lds[];
  __shared__ int red[4];
  float* lut = reinterpret_cast<float*>(sc_lds);
  unsigned* h = sc_lds + 256;
  const int tid = threadIdx.x, owner = blockIdx.y, nh = p.ns * SC_NB;
  lut[tid] = p.od[tid];                        // 256 lanes, 256 entries
  for (int i = tid; i < nh; i += 256) h[i] = 0u;
  __syncthreads();
  float mr[3], mg[3], mb[3];                   // the selected stains' columns of m (slots past p.ns are not used)
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    mr[s] = p.m[p.sel[s]];
    mg[s] = p.m[3 + p.sel[s]];
    mb[s] = p.m[6 + p.sel[s]];
  }
  const int nq = (p.W + 3) >> 2;
  const long per = (long)p.rows * nq, total = per * p.spo;
  int nt = 0;
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const ScQuad d = sc_quad(p, owner, q, nq, per);
    unsigned v[12] = {};                       // (the pixels a short quad does not load are not counted)
    sc_load_quad<LOADER>(p.a, (long)d.n * p.img_a + (long)d.y * p.pitch_a, p.chan, d.x0, d.px, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool t = j < d.px && is_tissue(v[3 * j], v[3 * j + 1], v[3 * j + 2], p.white, p.black);
      const float odr = lut[v[3 * j]], odg = lut[v[3 * j + 1]], odb = lut[v[3 * j + 2]];
      nt += t ? 1 : 0;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        if (s < p.ns) sc_lds_add(h + s * SC_NB, sc_bin(sc_conc(odr, odg, odb, mr[s], mg[s], mb[s])), t);
      }
    }
  }
  sc_flush_tissue<1>(&nt, red, owner, tissue);           // (its barrier also ends the LDS updates)
  for (int i = tid; i < nh; i += 256) {
    const unsigned c = h[i];
    const int k = (i >> 12) == 0 ? p.sel[0] : (i >> 12) == 1 ? p.sel[1] : p.sel[2];
    if (c) atomicAdd(&hist[((long)owner * 3 + k) * SC_NB + (i & (SC_NB - 1))], (unsigned long long)c);
  }
}

// LDS: the table, then four histograms (the fourth stays empty without jt)
template <int LOADER>
__global__ __launch_bounds__(256) void sc_pair_hist_kernel(const ScParams p, unsigned long long* __restrict__ hist,
                                                           unsigned long long* __restrict__ tissue) {
  extern __shared__ unsigned sc_lds[];
  __shared__ int red[8];
  float* lut = reinterpret_cast<float*>(sc_lds);
  unsigned* h = sc_lds + 256;
  const int tid = threadIdx.x, owner = blockIdx.y;
  const float mr = p.m[p.sel[0]], mg = p.m[3 + p.sel[0]], mb = p.m[6 + p.sel[0]];
  lut[tid] = p.od[tid];
  for (int i = tid; i < 4 * SC_NB; i += 256) h[i] = 0u;
  __syncthreads();
  const int nq = (p.W + 3) >> 2;
  const long per = (long)p.rows * nq, total = per * p.spo;
  int nt[2] = {0, 0};
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const ScQuad d = sc_quad(p, owner, q, nq, per);
    unsigned va[12] = {}, vb[12] = {};         // (the pixels a short quad does not load are not counted)
    sc_load_quad<LOADER>(p.a, (long)d.n * p.img_a + (long)d.y * p.pitch_a, p.chan, d.x0, d.px, va);
    sc_load_quad<LOADER>(p.b, (long)d.n * p.img_b + (long)d.y * p.pitch_b, p.chan, d.x0, d.px, vb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = j < d.px;
      const bool ta = in && is_tissue(va[3 * j], va[3 * j + 1], va[3 * j + 2], p.white, p.black);
      const bool tb = in && is_tissue(vb[3 * j], vb[3 * j + 1], vb[3 * j + 2], p.white, p.black);
      const int ba = sc_bin(sc_conc(lut[va[3 * j]], lut[va[3 * j + 1]], lut[va[3 * j + 2]], mr, mg, mb));
      const int bb = sc_bin(sc_conc(lut[vb[3 * j]], lut[vb[3 * j + 1]], lut[vb[3 * j + 2]], mr, mg, mb));
      nt[0] += ta ? 1 : 0;
      nt[1] += tb ? 1 : 0;
      sc_lds_add(h, ba, ta);
      sc_lds_add(h + SC_NB, bb, tb);
      sc_lds_add(h + 2 * SC_NB, min(ba, bb), ta && tb);
      sc_lds_add(h + 3 * SC_NB, ba, ta && tb && p.jt > 0 && bb >= p.jt);
    }
  }
  sc_flush_tissue<2>(nt, red, owner, tissue);
  for (int i = tid; i < 4 * SC_NB; i += 256) {
    const unsigned c = h[i];
    if (c) atomicAdd(&hist[(long)owner * 4 * SC_NB + i], (unsigned long long)c);
  }
}

// ---- the threshold rules --------------------------------------------------------------------------------------------
// Lane t of the one workgroup holds bins 16 t .. 16 t + 15.

// v[i] -> the suffix sum over every bin >= 16 t + i of the workgroup's 4096 values; tot: 256 words of LDS
__device__ __forceinline__ void sc_suffix(long long* v, long long* tot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 14; i >= 0; --i) v[i] += v[i + 1];
  __syncthreads();                             // the previous use of tot is over
  tot[tid] = v[0];
  __syncthreads();
  long long above = 0;
  for (int u = tid + 1; u < 256; ++u) above += tot[u];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] += above;
}

// |x y - z w| for x, y, z, w < 2^63 as (hi, lo)
__device__ __forceinline__ void sc_absdiff_products(unsigned long long x, unsigned long long y, unsigned long long z,
                                                    unsigned long long w, unsigned long long& hi,
                                                    unsigned long long& lo) {
  const unsigned long long l1 = x * y, h1 = __umul64hi(x, y), l2 = z * w, h2 = __umul64hi(z, w);
  const bool ge = h1 > h2 || (h1 == h2 && l1 >= l2);
  const unsigned long long al = ge ? l1 : l2, ah = ge ? h1 : h2, bl = ge ? l2 : l1, bh = ge ? h2 : h1;
  lo = al - bl;
  hi = ah - bh - (al < bl ? 1ull : 0ull);
}

// (hi, lo) -> double, rounded once to nearest even.  Above 2^64 the leading 64 bits are taken with every lower bit
// ORed into their last one (a sticky bit, eleven places below the rounding position), the hardware rounds that integer,
// and the power of two is exact.
__device__ __forceinline__ double sc_u128_to_double(unsigned long long hi, unsigned long long lo) {
  if (hi == 0) return (double)lo;
  const int s = __clzll((long long)hi);
  unsigned long long top = hi, rest = lo;
  if (s) {
    top = (hi << s) | (lo >> (64 - s));
    rest = lo << s;
  }
  top |= rest ? 1ull : 0ull;
  return ldexp((double)top, 64 - s);
}

// arg-max over the workgroup in the strict order (larger value, then smaller index); every lane gets the winner
template <typename T>
__device__ __forceinline__ void sc_argmax(T& val, int& idx, T* sv, int* si) {
  const int tid = threadIdx.x;
  __syncthreads();
  sv[tid] = val;
  si[tid] = idx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const T ov = sv[tid + s];
      const int oi = si[tid + s];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) {
        sv[tid] = ov;
        si[tid] = oi;
      }
    }
    __syncthreads();
  }
  val = sv[0];
  idx = si[0];
}

struct ScQuantiles {
  double q[SC_MAX_Q];
};

// one workgroup per histogram row
__global__ __launch_bounds__(256) void sc_thresholds_kernel(const long long* __restrict__ hist, int coarse, int nquant,
                                                            const ScQuantiles qs, long long* __restrict__ positive,
                                                            int* __restrict__ bins, int* __restrict__ valid,
                                                            double* __restrict__ thr) {
  __shared__ long long fine[SC_NB];
  __shared__ long long grp[SC_NB / 2];
  __shared__ long long tot[256];
  __shared__ double svd[256];
  __shared__ int si[256];
  long long* svl = tot;                        // the integer arg-max runs after the last suffix sum
  const int tid = threadIdx.x, nout = 2 + nquant;
  const long row = blockIdx.x;
  const long long* hr = hist + row * SC_NB;
  long long pos[16], s1[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long c = hr[16 * tid + i];
    fine[16 * tid + i] = c;
    pos[i] = c;
    s1[i] = (long long)(16 * tid + i) * c;
  }
  sc_suffix(pos, tot);
  sc_suffix(s1, tot);
#pragma unroll
  for (int i = 0; i < 16; ++i) positive[row * SC_NB + 16 * tid + i] = pos[i];
  __syncthreads();
  if (tid == 0) {
    tot[0] = pos[0];
    tot[1] = s1[0];
  }
  __syncthreads();
  const long long N = tot[0], S = tot[1];

  // Otsu: sigma(j) = a^2 / (P (N - P)), a = double(N S1[j] - P S)
  double bv = 0.0;
  int bi = SC_NB;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = 16 * tid + i;
    const long long P = pos[i];
    if (j >= 1 && P != 0 && P != N) {
#pragma clang fp contract(off)
      unsigned long long hi, lo;
      sc_absdiff_products((unsigned long long)N, (unsigned long long)s1[i], (unsigned long long)P, (unsigned long long)S,
                          hi, lo);
      const double a = sc_u128_to_double(hi, lo);
      const double num = a * a;
      const double den = (double)P * (double)(N - P);
      const double sg = num / den;
      if (sg > bv) {                           // ascending j: the first maximum stays
        bv = sg;
        bi = j;
      }
    }
  }
  sc_argmax<double>(bv, bi, svd, si);
  const int otsu_ok = bv > 0.0 ? 1 : 0, otsu_bin = otsu_ok ? bi : 0;

  // triangle on the histogram coarsened by `coarse`
  const int G = SC_NB / coarse;
  const long long* g = fine;
  if (coarse > 1) {
    for (int i = tid; i < G; i += 256) {
      long long s = 0;
      for (int u = 0; u < coarse; ++u) s += fine[i * coarse + u];
      grp[i] = s;
    }
    g = grp;
  }
  __syncthreads();
  long long pv = -1;
  int pi = SC_NB, ev = -1, ei = 0;
  for (int i = tid; i < G; i += 256) {
    const long long c = g[i];
    if (c > pv) {
      pv = c;
      pi = i;
    }
    if (c > 0) ev = i;                         // ascending i: the largest non-empty index stays
  }
  sc_argmax<long long>(pv, pi, svl, si);
  sc_argmax<int>(ev, ei, reinterpret_cast<int*>(svd), si);
  const int pk = pi, e = ev;
  int tri_ok = 0, tri_bin = 0;
  if (e > pk + 1) {                            // uniform over the workgroup
    const long long gp = g[pk], ge = g[e], w = e - pk;
    long long tv = INT64_MIN;
    int ti = SC_NB;
    for (int i = pk + 1 + tid; i < e; i += 256) {
      const long long T = gp * w + (ge - gp) * (long long)(i - pk) - g[i] * w;
      if (T > tv) {
        tv = T;
        ti = i;
      }
    }
    sc_argmax<long long>(tv, ti, svl, si);
    tri_ok = 1;
    tri_bin = coarse * ti;
  }

  // quantiles: the smallest j >= 1 with positive[j] <= floor(q N); positive falls with j
  int qbin[SC_MAX_Q], qok[SC_MAX_Q];
#pragma unroll
  for (int u = 0; u < SC_MAX_Q; ++u) {
    qbin[u] = SC_NB - 1;
    qok[u] = 0;
    if (u < nquant) {                          // uniform
      const long long K = (long long)floor(qs.q[u] * (double)N);
      int first = -SC_NB, none = 0;            // max of -j = min of j
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        const int j = 16 * tid + i;
        if (j >= 1 && pos[i] <= K) first = -j;
      }
      sc_argmax<int>(first, none, reinterpret_cast<int*>(svd), si);
      if (N > 0 && first > -SC_NB) {
        qbin[u] = -first;
        qok[u] = 1;
      }
    }
  }
  if (tid == 0) {
    int* ob = bins + row * nout;
    int* ov = valid + row * nout;
    double* ot = thr + row * nout;
    ob[0] = otsu_bin;
    ov[0] = otsu_ok;
    ob[1] = tri_bin;
    ov[1] = tri_ok;
#pragma unroll
    for (int u = 0; u < SC_MAX_Q; ++u) {
      if (u < nquant) {
        ob[2 + u] = qbin[u];
        ov[2 + u] = qok[u];
      }
    }
    for (int u = 0; u < nout; ++u) ot[u] = (double)ob[u] / 1024.0;
  }
}

// Dice as a fraction n / d; d == 0 counts as 1 / 1
struct ScFrac {
  long long n, d;
};
__device__ __forceinline__ bool sc_frac_gt(const ScFrac& x, const ScFrac& y) {      // x > y, exactly (operands < 2^42)
  return (unsigned __int128)x.n * (unsigned __int128)y.d > (unsigned __int128)y.n * (unsigned __int128)x.d;
}
__device__ __forceinline__ bool sc_frac_eq(const ScFrac& x, const ScFrac& y) {
  return (unsigned __int128)x.n * (unsigned __int128)y.d == (unsigned __int128)y.n * (unsigned __int128)x.d;
}
__device__ __forceinline__ double sc_dice(long long both, long long den) {
  return den == 0 ? 1.0 : (double)(2 * both) / (double)den;
}

// one workgroup per owner
__global__ __launch_bounds__(256) void sc_pair_thresholds_kernel(const long long* __restrict__ hist, int jt,
                                                                 long long* __restrict__ counts,
                                                                 double* __restrict__ dice, int* __restrict__ bins,
                                                                 int* __restrict__ valid, double* __restrict__ vals) {
  __shared__ long long tot[256];
  __shared__ long long sn[256], sd[256];
  __shared__ int si[256];
  __shared__ long long keep[3];                // N_a, N_b, positive_b[jt]
  const int tid = threadIdx.x;
  const long o = blockIdx.x;
  const long long* hr = hist + o * 4 * SC_NB;
  long long pa[16], pb[16], bc[16], bd[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    pa[i] = hr[16 * tid + i];
    pb[i] = hr[SC_NB + 16 * tid + i];
    bc[i] = hr[2 * SC_NB + 16 * tid + i];
    bd[i] = hr[3 * SC_NB + 16 * tid + i];
  }
  sc_suffix(pa, tot);
  sc_suffix(pb, tot);
  sc_suffix(bc, tot);
  sc_suffix(bd, tot);
  if (tid == 0) {
    keep[0] = pa[0];
    keep[1] = pb[0];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (16 * tid + i == jt) keep[2] = pb[i];   // jt = 0: the whole of b's tissue, never used
  }
  __syncthreads();
  const long long Na = keep[0], Nb = keep[1], pbt = keep[2];
  long long* oc = counts + o * 4 * SC_NB;
  double* od = dice + o * 2 * SC_NB;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = 16 * tid + i;
    oc[j] = pa[i];
    oc[SC_NB + j] = pb[i];
    oc[2 * SC_NB + j] = bc[i];
    oc[3 * SC_NB + j] = bd[i];
    od[j] = sc_dice(bc[i], pa[i] + pb[i]);
    od[SC_NB + j] = jt > 0 ? sc_dice(bd[i], pa[i] + pbt) : 0.0;
  }
  if (jt <= 0) {                               // uniform: no target threshold, no matching rule
    if (tid == 0) {
      bins[o * 2] = bins[o * 2 + 1] = 0;
      valid[o * 2] = valid[o * 2 + 1] = 0;
      for (int u = 0; u < 8; ++u) vals[o * 8 + u] = 0.0;
    }
    return;
  }
  // match_burden: the smallest j >= 1 of minimal |positive_a[j] N_b - positive_b[jt] N_a|, as (hi, lo)
  unsigned long long mh = ~0ull, ml = ~0ull;
  int mj = SC_NB;
  ScFrac best{-1, 1};                          // below every Dice
  int bj = SC_NB;
  long long pa_m = 0, pa_b = 0, bd_m = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = 16 * tid + i;
    if (j >= 1) {
      unsigned long long hi, lo;
      sc_absdiff_products((unsigned long long)pa[i], (unsigned long long)Nb, (unsigned long long)pbt,
                          (unsigned long long)Na, hi, lo);
      if (hi < mh || (hi == mh && lo < ml)) {
        mh = hi;
        ml = lo;
        mj = j;
        pa_m = pa[i];
        bd_m = bd[i];
      }
      const long long den = pa[i] + pbt;
      const ScFrac f = den == 0 ? ScFrac{1, 1} : ScFrac{2 * bd[i], den};
      if (best.n < 0 || sc_frac_gt(f, best)) {
        best = f;
        bj = j;
        pa_b = pa[i];
      }
    }
  }
  // the two reductions, by hand: the keys are wider than one word
  __syncthreads();
  sn[tid] = (long long)mh;
  sd[tid] = (long long)ml;
  si[tid] = mj;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const unsigned long long oh = (unsigned long long)sn[tid + s], ol = (unsigned long long)sd[tid + s];
      const unsigned long long th = (unsigned long long)sn[tid], tl = (unsigned long long)sd[tid];
      const int oi = si[tid + s];
      if (oh < th || (oh == th && (ol < tl || (ol == tl && oi < si[tid])))) {
        sn[tid] = (long long)oh;
        sd[tid] = (long long)ol;
        si[tid] = oi;
      }
    }
    __syncthreads();
  }
  const int match_bin = si[0];
  __syncthreads();
  sn[tid] = best.n;
  sd[tid] = best.d;
  si[tid] = bj;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const ScFrac of{sn[tid + s], sd[tid + s]}, tf{sn[tid], sd[tid]};
      const int oi = si[tid + s];
      const bool take = tf.n < 0 ? of.n >= 0 : (of.n >= 0 && (sc_frac_gt(of, tf) || (sc_frac_eq(of, tf) && oi < si[tid])));
      if (take) {
        sn[tid] = of.n;
        sd[tid] = of.d;
        si[tid] = oi;
      }
    }
    __syncthreads();
  }
  const int dice_bin = si[0];
  // the lanes that own the chosen bins write what belongs to them
  const int ok = (Na > 0 && Nb > 0) ? 1 : 0;
  const double bt = (double)pbt / (double)max(Nb, 1LL);
  if (mj == match_bin) {                       // one lane: bins are owned by one lane each
    const double bp = (double)pa_m / (double)max(Na, 1LL);
    bins[o * 2] = match_bin;
    valid[o * 2] = ok;
    vals[o * 8] = (double)match_bin / 1024.0;
    vals[o * 8 + 4] = bt;
    vals[o * 8 + 5] = bp;
    vals[o * 8 + 6] = fabs(bp - bt);
    vals[o * 8 + 7] = sc_dice(bd_m, pa_m + pbt);
  }
  if (bj == dice_bin) {
    bins[o * 2 + 1] = dice_bin;
    valid[o * 2 + 1] = ok;
    vals[o * 8 + 1] = (double)dice_bin / 1024.0;
    vals[o * 8 + 2] = best.d == 0 ? 1.0 : (double)best.n / (double)best.d;
    vals[o * 8 + 3] = (double)pa_b / (double)max(Na, 1LL);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int sc_fill(ScParams& p, int B, int rows, int H, int W, const float* od_table, const float* unmix, int white, int black,
            int pool) {
  if (!od_table || !unmix) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || white < 1 || white > 256 || black < 0 ||
      black > 255)
    return S2S_ERR_SHAPE;
  if ((long)H * W > SC_MAX_PIXELS / (pool ? B : 1)) return S2S_ERR_SHAPE;     // an owner holds at most 2^40 pixels
  p.rows = rows;
  p.W = W;
  p.spo = pool ? B : 1;
  p.white = white;
  p.black = black;
  p.ns = 0;
  p.sel[0] = p.sel[1] = p.sel[2] = 0;
  p.jt = 0;
  for (int i = 0; i < 9; ++i) p.m[i] = unmix[i];
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  p.b = nullptr;
  p.pitch_b = p.img_b = 0;
  p.chan = 0;
  return S2S_OK;
}

// workgroups per owner, all owners together at most what is resident at once with `lds` bytes each (a second round
// would run at a fraction of the machine); 0: a uint32 LDS bin could wrap
unsigned sc_blocks(long quads, int owners, int lds) {
  int resident = SC_LDS_PER_CU / lds;
  if (resident > 8) resident = 8;              // 8 workgroups of four waves fill a CU's wave slots
  long cap = (long)SC_CUS * resident / owners;
  if (cap < 1) cap = 1;
  long blocks = (quads + 256L * SC_QUADS - 1) / (256L * SC_QUADS);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const long per_thread = (quads + blocks * 256 - 1) / (blocks * 256);
  return per_thread * 1024 >= (1L << 32) ? 0u : (unsigned)blocks;
}

template <int LOADER>
int sc_launch(const ScParams& p, int B, int pool, bool paired, int reset, long* hist, long* tissue, hipStream_t s) {
  const int owners = pool ? 1 : B;
  const int lds = SC_LUT_BYTES + (paired ? 4 : p.ns) * SC_HIST_BYTES;      // paired: 65 KiB, above the 64 KiB a kernel gets unasked
  const unsigned blocks = sc_blocks((long)p.spo * p.rows * cdiv(p.W, 4), owners, lds);
  if (!blocks) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(unsigned long long), "int64 counts");
  unsigned long long* h = (unsigned long long*)hist;
  unsigned long long* t = (unsigned long long*)tissue;
  const int nh = paired ? 4 : 3, nt = paired ? 2 : 1;
  if (reset) {
    const long n = (long)owners * nh * SC_NB;
    const long zb = (n + 255) / 256;
    hipLaunchKernelGGL(sc_zero_kernel, dim3((unsigned)(zb > 1024 ? 1024 : zb)), dim3(256), 0, s, h, n, t, owners * nt);
    S2S_LAUNCH_CHECK();
  }
  const dim3 grid(blocks, (unsigned)owners);
  if (paired) {
    static unsigned long long attr_devs = 0;                   // hipFuncSetAttribute is per device
    if (int rc = s2s_allow_dyn_lds(reinterpret_cast<const void*>(sc_pair_hist_kernel<LOADER>), lds, &attr_devs)) return rc;
    hipLaunchKernelGGL(sc_pair_hist_kernel<LOADER>, grid, dim3(256), lds, s, p, h, t);
  } else {
    hipLaunchKernelGGL(sc_hist_kernel<LOADER>, grid, dim3(256), lds, s, p, h, t);
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

int sc_select(ScParams& p, int stain_mask) {
  if (stain_mask < 1 || stain_mask > 7) return S2S_ERR_SHAPE;
  for (int k = 0; k < 3; ++k) {
    if (stain_mask >> k & 1) p.sel[p.ns++] = k;
  }
  return S2S_OK;
}

int sc_u8_layout(long pitch, long img, int B, int band_top, int band_h, int H, int W) {
  if (pitch < 3L * W || band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && img < pitch * (long)band_h) return S2S_ERR_SHAPE;
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_stain_hist_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H,
                                 int W, const float* od_table, const float* unmix, int white, int black, int stain_mask,
                                 int pool, int reset, long* hist, long* tissue, void* stream) {
  if (!img || !hist || !tissue) return S2S_ERR_NULL;
  ScParams p;
  int rc = sc_fill(p, B, band_h, H, W, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = sc_u8_layout(pitch, img_stride, B, band_top, band_h, H, W);
  if (rc == S2S_OK) rc = sc_select(p, stain_mask);
  if (rc != S2S_OK) return rc;
  p.a = img;
  p.pitch_a = pitch;
  p.img_a = img_stride;
  return sc_launch<SC_U8>(p, B, pool, false, reset, hist, tissue, (hipStream_t)stream);
}

extern "C" int s2s_stain_hist_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix,
                                  int white, int black, int stain_mask, int pool, int reset, long* hist, long* tissue,
                                  void* stream) {
  if (!img || !hist || !tissue) return S2S_ERR_NULL;
  ScParams p;
  int rc = sc_fill(p, B, H, H, W, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = sc_select(p, stain_mask);
  if (rc != S2S_OK) return rc;
  p.a = img;
  p.pitch_a = W;
  p.chan = (long)H * W;
  p.img_a = 3L * H * W;
  return sc_launch<SC_F32>(p, B, pool, false, reset, hist, tissue, (hipStream_t)stream);
}

extern "C" int s2s_stain_pair_hist_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b,
                                      int B, int band_top, int band_h, int H, int W, const float* od_table,
                                      const float* unmix, int white, int black, int stain, int jt, int pool, int reset,
                                      long* hist, long* tissue, void* stream) {
  if (!a || !b || !hist || !tissue) return S2S_ERR_NULL;
  ScParams p;
  int rc = sc_fill(p, B, band_h, H, W, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = sc_u8_layout(pitch_a, img_a, B, band_top, band_h, H, W);
  if (rc == S2S_OK) rc = sc_u8_layout(pitch_b, img_b, B, band_top, band_h, H, W);
  if (rc != S2S_OK) return rc;
  if (stain < 0 || stain > 2 || jt < 0 || jt >= SC_NB) return S2S_ERR_SHAPE;
  p.a = a;
  p.pitch_a = pitch_a;
  p.img_a = img_a;
  p.b = b;
  p.pitch_b = pitch_b;
  p.img_b = img_b;
  p.ns = 1;
  p.sel[0] = stain;
  p.jt = jt;
  return sc_launch<SC_U8>(p, B, pool, true, reset, hist, tissue, (hipStream_t)stream);
}

extern "C" int s2s_stain_pair_hist_f32(const float* a, const float* b, int B, int H, int W, const float* od_table,
                                       const float* unmix, int white, int black, int stain, int jt, int pool, int reset,
                                       long* hist, long* tissue, void* stream) {
  if (!a || !b || !hist || !tissue) return S2S_ERR_NULL;
  ScParams p;
  const int rc = sc_fill(p, B, H, H, W, od_table, unmix, white, black, pool);
  if (rc != S2S_OK) return rc;
  if (stain < 0 || stain > 2 || jt < 0 || jt >= SC_NB) return S2S_ERR_SHAPE;
  p.a = a;
  p.b = b;
  p.pitch_a = p.pitch_b = W;
  p.chan = (long)H * W;
  p.img_a = p.img_b = 3L * H * W;
  p.ns = 1;
  p.sel[0] = stain;
  p.jt = jt;
  return sc_launch<SC_F32>(p, B, pool, true, reset, hist, tissue, (hipStream_t)stream);
}

extern "C" int s2s_stain_thresholds(const long* hist, long rows, int coarse, const double* quantiles, int nquant,
                                    long* positive, int* bins, int* valid, double* thr, void* stream) {
  if (!hist || !positive || !bins || !valid || !thr || (nquant > 0 && !quantiles)) return S2S_ERR_NULL;
  if (rows < 1 || rows > 0x7fffffffL || nquant < 0 || nquant > SC_MAX_Q) return S2S_ERR_SHAPE;
  if (coarse < 1 || coarse > SC_NB || (coarse & (coarse - 1)) != 0) return S2S_ERR_SHAPE;
  ScQuantiles qs;
  for (int i = 0; i < SC_MAX_Q; ++i) {
    qs.q[i] = i < nquant ? quantiles[i] : 0.0;
    if (!(qs.q[i] >= 0.0 && qs.q[i] <= 1.0)) return S2S_ERR_SHAPE;
  }
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  hipLaunchKernelGGL(sc_thresholds_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)hist, coarse, nquant, qs, (long long*)positive, bins, valid, thr);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_stain_pair_thresholds(const long* hist, long owners, int jt, long* counts, double* dice, int* bins,
                                         int* valid, double* vals, void* stream) {
  if (!hist || !counts || !dice || !bins || !valid || !vals) return S2S_ERR_NULL;
  if (owners < 1 || owners > 0x7fffffffL || jt < 0 || jt >= SC_NB) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(sc_pair_thresholds_kernel, dim3((unsigned)owners), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)hist, jt, (long long*)counts, dice, bins, valid, vals);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
