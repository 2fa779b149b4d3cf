// Stain object morphometry: per-object shape, thickness and stain intensity from a label image, all on the GPU.
// DESIGN.md section 3.26.
//
//   s2s_objfeat_shape          labels int32 [B][H][W] (0 = background, objects 1..count as s2s_objects_label numbers them)
//                              -> per sample the largest label, per object numbered <= max_objects: area, bounding box,
//                              the five raw moments, crack length, boundary pixels, border flag and, given the squared
//                              distance map of s2s_morph_edt, the largest squared distance inside the object
//   s2s_objfeat_intensity_u8   labels + uint8 HWC RGB rows (a band of a taller image, any row pitch) -> per object the
//   s2s_objfeat_intensity_f32  sum, the sum of squares and the maximum of the quantised stain concentration q; the fp32
//                              form reads [B][3][H][W] through the save conversion of stain_quant.hip
//   s2s_objfeat_finalize       the integer table -> fp64 centroid, axes, eccentricity, orientation, compactness,
//                              concentration mean / deviation / maximum and inscribed radius
//
// The hot path is a reduction keyed by label.  One global atomic per pixel and quantity would serialise on a large
// object, so the sums are built in three steps:
//   wave       a wave covers 64 consecutive pixels of ONE row (shape) or 4 x 64 of one row (intensity).  It peels off its
//              distinct labels by ballot; for the shape pass the count, first and last column, sum of columns and sum of
//              squared columns of a label's pixels follow from the ballot mask alone (popcounts against constant masks),
//              the neighbour tallies from three more ballots per row.  Only the maximum of d2 and the q sums need a
//              butterfly (the intensity pass folds a lane's four pixels first: one butterfly per distinct label).
//   workgroup  an open-addressed LDS table of OF_SLOTS labels (linear probing, OF_PROBES tries); lanes 0..13 of the wave
//              each add or max ONE quantity into the label's slot, so a (row, label) pair costs two LDS instructions
//   device     after a barrier every occupied slot is flushed with one 64-bit integer atomic (or one 32-bit maximum) per
//              quantity; a label that found no slot goes to global memory directly.  All global atomics are agent scope:
//              the XCDs' L2s are private.
// The shape pass's workgroup owns a 64 x 64 tile; each wave walks 16 consecutive rows and keeps the row above, the row
// itself and the row below in registers, so a label is loaded 18 / 16 times, plus one load per row by each of the two
// edge lanes for the columns left and right of the tile.  Left and right neighbours inside the tile are lane shuffles.
//
// Everything accumulated is an integer and every maximum is of non-negative integers, so the atomics give the same bits
// in any order; there is no float atomic.  The caller zeroes count and the tables; the bounding box's first row and
// column are kept as 32768 - value while they accumulate (a maximum over zero-initialised memory) and turned back by a
// second, tiny launch.  Nothing here allocates, synchronises, reads the environment or reads back to the host.
#include <limits.h>

#include "common.h"

namespace {

constexpr int OF_TW = 64, OF_TH = 64;        // the shape pass's tile (object_features.TILE)
constexpr int OF_ROWS = OF_TH / 4;           // consecutive rows per wave
constexpr int OF_IW = 256, OF_IH = 16;       // the intensity pass's tile: 4 pixels per lane, 4 rows per wave
constexpr int OF_SLOTS = 64;                 // labels per workgroup table (object_features.LDS_SLOTS)
constexpr int OF_PROBES = 8;
constexpr int OF_NQ = 14;                    // 8 sums + 6 maxima per label
constexpr int OF_MAX_SIDE = 32767;
constexpr int OF_COMPLEMENT = 32768;         // first row / column are accumulated as OF_COMPLEMENT - value
constexpr int OF_NF = 15;                    // fp64 values per object (object_features.N_DERIVED)
constexpr int OF_FAR = INT_MAX;

#define OF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct OfTable {
  int M;
  unsigned long long* area;      // [B][M]
  int* bbox;                     // [B][M][4]
  unsigned long long* moments;   // [B][M][5]  sum y, sum x, sum y^2, sum x^2, sum yx
  unsigned long long* edges;     // [B][M]
  unsigned long long* boundary;  // [B][M]
  int* border;                   // [B][M]
  int* max_d2;                   // [B][M] or null
};

// quantity q of a label: 0 area, 1..5 moments, 6 edges, 7 boundary (sums); 8 32768 - y0, 9 32768 - x0, 10 y1, 11 x1,
// 12 border, 13 max d2 (maxima)
__device__ __forceinline__ void of_commit(const OfTable& tb, long row, int q, unsigned long long v) {
  if (v == 0) return;
  if (q < 8) {
    unsigned long long* p = q == 0 ? tb.area + row : q <= 5 ? tb.moments + 5 * row + (q - 1)
                                                   : q == 6 ? tb.edges + row : tb.boundary + row;
    __hip_atomic_fetch_add(p, v, OF_RLX_AGENT);
  } else {
    if (q == 13 && !tb.max_d2) return;
    int* p = q <= 11 ? tb.bbox + 4 * row + (q - 8) : q == 12 ? tb.border + row : tb.max_d2 + row;
    __hip_atomic_fetch_max(p, (int)v, OF_RLX_AGENT);
  }
}

// the slot of label k in the workgroup's table, -1 when OF_PROBES tries found neither it nor a free place
__device__ __forceinline__ int of_slot(int* keys, int k) {
  const unsigned h = ((unsigned)k * 2654435761u) >> 26;
  for (int p = 0; p < OF_PROBES; ++p) {
    const int s = (int)((h + p) & (OF_SLOTS - 1));
    const int old = atomicCAS(keys + s, 0, k);
    if (old == 0 || old == k) return s;
  }
  return -1;
}

// the lanes of a wave whose squared lane number has bit B set
constexpr unsigned long long of_sq_mask(int b) {
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l)
    if (((l * l) >> b) & 1) m |= 1ull << l;
  return m;
}
template <int B>
__device__ __forceinline__ int of_sq_term(unsigned long long same) {
  constexpr unsigned long long m = of_sq_mask(B);
  return __popcll(same & m) << B;
}

__global__ __launch_bounds__(256) void of_shape_kernel(const int* __restrict__ labels, const int* __restrict__ d2, int H,
                                                       int W, const OfTable tb, int* count) {
  __shared__ unsigned long long s_acc[OF_SLOTS][8];
  __shared__ int s_max[OF_SLOTS][8];
  __shared__ int s_key[OF_SLOTS];
  __shared__ int s_top;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.z;
  for (int i = threadIdx.x; i < OF_SLOTS * 8; i += 256) {
    (&s_acc[0][0])[i] = 0;
    (&s_max[0][0])[i] = 0;
  }
  if (threadIdx.x < OF_SLOTS) s_key[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_top = 0;
  __syncthreads();
  const int x0 = blockIdx.x * OF_TW, x = x0 + lane;
  const int ya = blockIdx.y * OF_TH + wv * OF_ROWS, yb = min(ya + OF_ROWS, H);
  const int* lab = labels + (long)n * H * W;
  const int* dd = d2 ? d2 + (long)n * H * W : nullptr;
  auto load = [&](int y, int xx) -> int {                   // -1: outside the image
    return (y >= 0 && y < H && xx >= 0 && xx < W) ? lab[(long)y * W + xx] : -1;
  };
  int top = 0, last_k = 0, last_slot = -1;
  if (ya < H) {                                             // wave-uniform
    int up = load(ya - 1, x), cur = load(ya, x);
    for (int y = ya; y < yb; ++y) {
      const int down = load(y + 1, x);
      int side = -1;
      if (lane == 0) side = load(y, x0 - 1);
      else if (lane == 63) side = load(y, x0 + OF_TW);
      int left = __shfl_up(cur, 1, 64), right = __shfl_down(cur, 1, 64);
      if (lane == 0) left = side;
      if (lane == 63) right = side;
      const int e = (up != cur) + (down != cur) + (left != cur) + (right != cur);
      top = max(top, cur);
      const bool in = cur > 0 && cur <= tb.M;
      const int dv = (dd && in) ? dd[(long)y * W + x] : 0;
      const unsigned long long e0 = __ballot(e & 1), e1 = __ballot(e & 2), e2 = __ballot(e & 4), eb = __ballot(e != 0);
      unsigned long long todo = __ballot(in);
      while (todo) {                                        // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int lk = __shfl(cur, leader, 64);
        const unsigned long long same = __ballot(cur == lk);
        todo &= ~same;
        const int cnt = __popcll(same);
        const int first = __ffsll((long long)same) - 1, last = 63 - __clzll((long long)same);
        // sums of the set bits' positions and of their squares, from the mask alone
        const int pos = __popcll(same & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(same & 0xCCCCCCCCCCCCCCCCull) +
                        4 * __popcll(same & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(same & 0xFF00FF00FF00FF00ull) +
                        16 * __popcll(same & 0xFFFF0000FFFF0000ull) + 32 * __popcll(same & 0xFFFFFFFF00000000ull);
        const int pos2 = of_sq_term<0>(same) + of_sq_term<2>(same) + of_sq_term<3>(same) + of_sq_term<4>(same) +
                         of_sq_term<5>(same) + of_sq_term<6>(same) + of_sq_term<7>(same) + of_sq_term<8>(same) +
                         of_sq_term<9>(same) + of_sq_term<10>(same) + of_sq_term<11>(same);   // (bit 1 of a square is 0)
        int md = 0;
        if (dd) {
          md = cur == lk ? dv : 0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) md = max(md, __shfl_xor(md, o, 64));
        }
        const long long sx = (long long)x0 * cnt + pos;
        const long long sxx = (long long)x0 * x0 * cnt + 2LL * x0 * pos + pos2;
        const int xf = x0 + first, xl = x0 + last;
        const int edge = (y == 0 || y == H - 1 || xf == 0 || xl == W - 1) ? 1 : 0;
        unsigned long long v;
        switch (lane) {
          case 0: v = (unsigned long long)cnt; break;
          case 1: v = (unsigned long long)((long long)y * cnt); break;
          case 2: v = (unsigned long long)sx; break;
          case 3: v = (unsigned long long)((long long)y * y * cnt); break;
          case 4: v = (unsigned long long)sxx; break;
          case 5: v = (unsigned long long)((long long)y * sx); break;
          case 6: v = (unsigned long long)(__popcll(same & e0) + 2 * __popcll(same & e1) + 4 * __popcll(same & e2)); break;
          case 7: v = (unsigned long long)__popcll(same & eb); break;
          case 8: v = (unsigned long long)(OF_COMPLEMENT - y); break;
          case 9: v = (unsigned long long)(OF_COMPLEMENT - xf); break;
          case 10: v = (unsigned long long)(y + 1); break;
          case 11: v = (unsigned long long)(xl + 1); break;
          case 12: v = (unsigned long long)edge; break;
          case 13: v = (unsigned long long)md; break;
          default: v = 0; break;
        }
        if (lk != last_k) {                                 // (wave-uniform) a wave mostly meets the label it met last
          int s = -1;
          if (lane == 0) s = of_slot(s_key, lk);
          last_slot = __shfl(s, 0, 64);
          last_k = lk;
        }
        if (lane < OF_NQ && v != 0) {
          if (last_slot < 0) of_commit(tb, (long)n * tb.M + lk - 1, lane, v);
          else if (lane < 8) atomicAdd(&s_acc[last_slot][lane], v);
          else atomicMax(&s_max[last_slot][lane - 8], (int)v);
        }
      }
      up = cur;
      cur = down;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
  if (lane == 0 && top > 0) atomicMax(&s_top, top);
  __syncthreads();
  for (int i = threadIdx.x; i < OF_SLOTS * OF_NQ; i += 256) {
    const int slot = i / OF_NQ, q = i - slot * OF_NQ;
    const int k = s_key[slot];
    if (k == 0) continue;
    of_commit(tb, (long)n * tb.M + k - 1, q, q < 8 ? s_acc[slot][q] : (unsigned long long)s_max[slot][q - 8]);
  }
  if (threadIdx.x == 0 && s_top > 0) __hip_atomic_fetch_max(count + n, s_top, OF_RLX_AGENT);
}

// first row / column back from their complements; rows of labels that own no pixel stay zero
__global__ __launch_bounds__(256) void of_bbox_kernel(const int* __restrict__ count, const long long* __restrict__ area,
                                                      int M, long rows, int* __restrict__ bbox) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int n = (int)(r / M), j = (int)(r - (long)n * M);
  if (j >= count[n] || area[r] <= 0) return;
  bbox[4 * r] = OF_COMPLEMENT - bbox[4 * r];
  bbox[4 * r + 1] = OF_COMPLEMENT - bbox[4 * r + 1];
}

// ---- intensity ---------------------------------------------------------------------------------------------------------
enum { OF_U8 = 0, OF_F32 = 1 };

struct OfImage {
  const void* a;
  long pitch, img;            // row pitch and sample stride: bytes (uint8) or elements (fp32)
  long chan;                  // fp32: elements per channel plane
  int band_top, band_h;       // image rows [band_top, band_top + band_h) are in the buffer (uint8; fp32: the whole image)
  int H, W, M;
  float m[3];                 // the chosen stain's column of the unmixing matrix
  float od[256];
};

// the save conversion of stain_quant.hip (sq_quantise)
__device__ __forceinline__ unsigned of_quantise(float x) {
#pragma clang fp contract(off)
  const float h = x * 0.5f;
  const float u = (h + 0.5f) * 255.0f;
  return (unsigned)(int)fminf(fmaxf(u, 0.0f), 255.0f);
}

// px (1..4) consecutive pixels of one row from column x0 on: v[3 j + c]
template <int LOADER>
__device__ __forceinline__ void of_load_quad(const void* base, long row_off, long chan, int x0, int px, unsigned* v) {
  if (LOADER == OF_U8) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + row_off + 3L * x0;
    if (px == 4 && ((uintptr_t)p & 3) == 0) {
      const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];
      const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];
      const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];
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
        for (int j = 0; j < 4; ++j) v[3 * j + c] = of_quantise(q[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = of_quantise(p[c * chan + j]);
        }
      }
    }
  }
}

// q = min(rint(max(c, 0) * 1024), 4095), c the fp32 concentration of stain_quant.hip: every product and sum rounded on
// its own (plain operators under the pragma; see sq_conc)
__device__ __forceinline__ int of_q(const float* m, float odr, float odg, float odb) {
#pragma clang fp contract(off)
  const float pr = odr * m[0], pg = odg * m[1], pb = odb * m[2];
  const float s = pr + pg;
  const float c = s + pb;
  return min((int)rintf(fmaxf(c, 0.0f) * 1024.0f), 4095);
}

struct OfSums {
  int* key;                       // LDS [OF_SLOTS]
  unsigned long long* acc;        // LDS [OF_SLOTS][2]
  int* mx;                        // LDS [OF_SLOTS]
  unsigned long long* sum_q;      // global [B][M]
  unsigned long long* sum_q2;
  int* max_q;
};

// Every lane brings four pixels: labels l, values q, and in ``pend`` one bit per pixel whose label is tabulated.  A round
// takes the first pending label of the first pending lane; every lane folds its pixels of that label, a butterfly sums
// them over the wave, and lanes 0..2 add the three results into the label's slot.  Rounds = distinct labels of the wave.
__device__ __forceinline__ void of_accumulate(const OfSums& t, long row0, int lane, const int* l, const int* q,
                                              unsigned pend) {
  static_assert(4ull * 64 * 4095 * 4095 <= 0xFFFFFFFFull, "a wave's sum of q^2 fits 32 bits");
  unsigned long long todo = __ballot(pend != 0);
  while (todo) {                                            // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const int first = (pend & 1) ? l[0] : (pend & 2) ? l[1] : (pend & 4) ? l[2] : l[3];
    const int lk = __shfl(first, leader, 64);
    unsigned a = 0, b = 0;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (((pend >> j) & 1) && l[j] == lk) {
        a += (unsigned)q[j];
        b += (unsigned)(q[j] * q[j]);
        c = max(c, q[j]);
        pend &= ~(1u << j);
      }
    }
    todo = __ballot(pend != 0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
      c = max(c, __shfl_xor(c, o, 64));
    }
    int slot = -1;
    if (lane == 0) slot = of_slot(t.key, lk);
    slot = __shfl(slot, 0, 64);
    const long row = row0 + lk - 1;
    if (slot >= 0) {
      if (lane == 0) atomicAdd(t.acc + 2 * slot, (unsigned long long)a);
      else if (lane == 1) atomicAdd(t.acc + 2 * slot + 1, (unsigned long long)b);
      else if (lane == 2) atomicMax(t.mx + slot, c);
    } else {
      if (lane == 0 && a) __hip_atomic_fetch_add(t.sum_q + row, (unsigned long long)a, OF_RLX_AGENT);
      else if (lane == 1 && b) __hip_atomic_fetch_add(t.sum_q2 + row, (unsigned long long)b, OF_RLX_AGENT);
      else if (lane == 2 && c) __hip_atomic_fetch_max(t.max_q + row, c, OF_RLX_AGENT);
    }
  }
}

template <int LOADER>
__global__ __launch_bounds__(256) void of_intensity_kernel(const OfImage p, const int* __restrict__ labels,
                                                           unsigned long long* sum_q, unsigned long long* sum_q2,
                                                           int* max_q) {
  __shared__ float lut[256];
  __shared__ unsigned long long s_acc[OF_SLOTS][2];
  __shared__ int s_mx[OF_SLOTS];
  __shared__ int s_key[OF_SLOTS];
  lut[threadIdx.x] = p.od[threadIdx.x];                     // 256 lanes, 256 entries
  if (threadIdx.x < OF_SLOTS) {
    s_acc[threadIdx.x][0] = s_acc[threadIdx.x][1] = 0;
    s_mx[threadIdx.x] = 0;
    s_key[threadIdx.x] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.z;
  const int xq = blockIdx.x * OF_IW + 4 * lane;
  const int px = max(0, min(4, p.W - xq));
  const long row0 = (long)n * p.M;
  const OfSums t{s_key, &s_acc[0][0], s_mx, sum_q, sum_q2, max_q};
  const int* lab = labels + (long)n * p.H * p.W;
  for (int r = wv; r < OF_IH; r += 4) {
    const int y = p.band_top + blockIdx.y * OF_IH + r;
    if (y >= p.band_top + p.band_h) break;                  // wave-uniform
    int l[4] = {0, 0, 0, 0};
    if (px > 0) {
      const int* lp = lab + (long)y * p.W + xq;
      if (px == 4 && ((uintptr_t)lp & 15) == 0) {
        const int4 q4 = *reinterpret_cast<const int4*>(lp);
        l[0] = q4.x; l[1] = q4.y; l[2] = q4.z; l[3] = q4.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < px) l[j] = lp[j];
      }
    }
    unsigned pend = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (l[j] > 0 && l[j] <= p.M) pend |= 1u << j;
    if (!__ballot(pend != 0)) continue;                     // a wave of background reads no pixel
    int q[4] = {0, 0, 0, 0};
    if (pend) {
      unsigned v[12];
      const long off = (long)n * p.img + (long)(y - (LOADER == OF_U8 ? p.band_top : 0)) * p.pitch;
      of_load_quad<LOADER>(p.a, off, p.chan, xq, px, v);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((pend >> j) & 1) q[j] = of_q(p.m, lut[v[3 * j]], lut[v[3 * j + 1]], lut[v[3 * j + 2]]);
    }
    of_accumulate(t, row0, lane, l, q, pend);
  }
  __syncthreads();
  if (threadIdx.x < OF_SLOTS) {
    const int k = s_key[threadIdx.x];
    if (k) {
      const long row = row0 + k - 1;
      if (s_acc[threadIdx.x][0]) __hip_atomic_fetch_add(sum_q + row, s_acc[threadIdx.x][0], OF_RLX_AGENT);
      if (s_acc[threadIdx.x][1]) __hip_atomic_fetch_add(sum_q2 + row, s_acc[threadIdx.x][1], OF_RLX_AGENT);
      if (s_mx[threadIdx.x]) __hip_atomic_fetch_max(max_q + row, s_mx[threadIdx.x], OF_RLX_AGENT);
    }
  }
}

// ---- finalize ----------------------------------------------------------------------------------------------------------
struct U128 {
  unsigned long long hi, lo;
};
__device__ __forceinline__ U128 u128_mul(unsigned long long a, unsigned long long b) { return {__umul64hi(a, b), a * b}; }
__device__ __forceinline__ bool u128_less(const U128& a, const U128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ U128 u128_sub(const U128& a, const U128& b) {            // a >= b
  return {a.hi - b.hi - (a.lo < b.lo ? 1ull : 0ull), a.lo - b.lo};
}
// the nearest double, rounded once: the top 64 bits with everything below them folded into the last one (a sticky bit,
// eleven places under the rounding position), converted and scaled by a power of two
__device__ __forceinline__ double u128_double(const U128& a) {
  if (a.hi == 0) return (double)a.lo;
  const int lz = __clzll((long long)a.hi);
  unsigned long long t = a.hi, rest = a.lo;
  if (lz) {
    t = (a.hi << lz) | (a.lo >> (64 - lz));
    rest = a.lo << lz;
  }
  if (rest) t |= 1ull;
  return ldexp((double)t, 64 - lz);
}
// A s2 - s1 s1' as a double, exact until the one conversion; may be negative when s1 != s1'
__device__ __forceinline__ double of_numerator(unsigned long long A, unsigned long long s2, unsigned long long s1a,
                                               unsigned long long s1b) {
  const U128 p = u128_mul(A, s2), q = u128_mul(s1a, s1b);
  return u128_less(p, q) ? -u128_double(u128_sub(q, p)) : u128_double(u128_sub(p, q));
}

struct OfFinal {
  const int* count;
  const long long* area;
  const long long* moments;
  const long long* edges;
  const long long* sum_q;        // null: no intensity
  const long long* sum_q2;
  const int* max_q;
  const int* max_d2;             // null: no thickness
};

// One thread per object.  The order of operations is the one include/stain2stain_hip.h spells out; no contraction, so a
// float64 restatement that follows it differs by the device's sqrt and atan2 alone.
__global__ __launch_bounds__(256) void of_finalize_kernel(const OfFinal f, int M, long rows, double* __restrict__ out) {
#pragma clang fp contract(off)
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int n = (int)(r / M), j = (int)(r - (long)n * M);
  double* o = out + OF_NF * r;
  const long long A = j < f.count[n] ? f.area[r] : 0;
  if (A <= 0) {
#pragma unroll
    for (int i = 0; i < OF_NF; ++i) o[i] = 0.0;
    return;
  }
  const unsigned long long a = (unsigned long long)A;
  const unsigned long long sy = (unsigned long long)f.moments[5 * r], sx = (unsigned long long)f.moments[5 * r + 1];
  const unsigned long long syy = (unsigned long long)f.moments[5 * r + 2], sxx = (unsigned long long)f.moments[5 * r + 3];
  const unsigned long long syx = (unsigned long long)f.moments[5 * r + 4];
  const double Ad = (double)A, A2 = Ad * Ad;
  o[0] = (double)sy / Ad;
  o[1] = (double)sx / Ad;
  const double four_a = 4.0 * Ad;
  o[2] = sqrt(four_a / 3.141592653589793);
  const double myy = of_numerator(a, syy, sy, sy) / A2;
  const double mxx = of_numerator(a, sxx, sx, sx) / A2;
  const double myx = of_numerator(a, syx, sy, sx) / A2;
  o[3] = myy;
  o[4] = mxx;
  o[5] = myx;
  const double t = mxx + myy, d = mxx - myy;
  const double dd = d * d, cc = myx * myx;
  const double disc = dd + 4.0 * cc;
  const double root = sqrt(disc);
  const double l1 = fmax(0.5 * (t + root), 0.0), l2 = fmax(0.5 * (t - root), 0.0);
  o[6] = 4.0 * sqrt(l1);
  o[7] = 4.0 * sqrt(l2);
  double ecc = 0.0;
  if (l1 > 0.0) {
    const double ratio = l2 / l1;
    ecc = sqrt(fmax(1.0 - ratio, 0.0));
  }
  o[8] = ecc;
  const double twice = 2.0 * myx;
  o[9] = (twice == 0.0 && d == 0.0) ? 0.0 : 0.5 * atan2(twice, d);
  const double E = (double)f.edges[r];
  const double num = 12.566370614359172 * Ad;
  o[10] = num / (E * E);
  if (f.sum_q) {
    const unsigned long long sq = (unsigned long long)f.sum_q[r], sq2 = (unsigned long long)f.sum_q2[r];
    const double mean = (double)sq / Ad;
    o[11] = mean / 1024.0;
    const double var = of_numerator(a, sq2, sq, sq) / A2;
    o[12] = sqrt(fmax(var, 0.0)) / 1024.0;
    o[13] = (double)f.max_q[r] / 1024.0;
  } else {
    o[11] = o[12] = o[13] = 0.0;
  }
  if (f.max_d2) {
    const int m = f.max_d2[r];
    o[14] = m == OF_FAR ? (double)INFINITY : sqrt((double)m);
  } else {
    o[14] = 0.0;
  }
}

bool of_shape_ok(int B, int H, int W, int M) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= OF_MAX_SIDE && W <= OF_MAX_SIDE && M >= 1 &&
         (long)B * M <= 0x7fffffffL;
}

int of_image(OfImage& p, int B, int H, int W, int M, const float* od_table, const float* unmix, int stain) {
  if (!od_table || !unmix) return S2S_ERR_NULL;
  if (!of_shape_ok(B, H, W, M) || stain < 0 || stain > 2) return S2S_ERR_SHAPE;
  p.H = H;
  p.W = W;
  p.M = M;
  for (int c = 0; c < 3; ++c) p.m[c] = unmix[3 * c + stain];
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  p.chan = 0;
  p.band_top = 0;
  p.band_h = H;
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_objfeat_shape(const int* labels, const int* d2, int B, int H, int W, int max_objects, int* count,
                                 long* area, int* bbox, long* moments, long* edges, long* boundary, int* border,
                                 int* max_d2, void* stream) {
  if (!labels || !count || !area || !bbox || !moments || !edges || !boundary || !border || (d2 && !max_d2))
    return S2S_ERR_NULL;
  if (!of_shape_ok(B, H, W, max_objects)) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(long long), "int64 tables");
  hipStream_t s = (hipStream_t)stream;
  const OfTable tb{max_objects, (unsigned long long*)area, bbox, (unsigned long long*)moments,
                   (unsigned long long*)edges, (unsigned long long*)boundary, border, d2 ? max_d2 : nullptr};
  hipLaunchKernelGGL(of_shape_kernel, dim3((unsigned)cdiv(W, OF_TW), (unsigned)cdiv(H, OF_TH), (unsigned)B), dim3(256), 0,
                     s, labels, d2, H, W, tb, count);
  const long rows = (long)B * max_objects;
  hipLaunchKernelGGL(of_bbox_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, count,
                     (const long long*)area, max_objects, rows, bbox);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objfeat_intensity_u8(const int* labels, const void* img, long pitch, long img_stride, int B,
                                        int band_top, int band_h, int H, int W, int max_objects, const float* od_table,
                                        const float* unmix, int stain, long* sum_q, long* sum_q2, int* max_q,
                                        void* stream) {
  if (!labels || !img || !sum_q || !sum_q2 || !max_q) return S2S_ERR_NULL;
  OfImage p;
  const int rc = of_image(p, B, H, W, max_objects, od_table, unmix, stain);
  if (rc != S2S_OK) return rc;
  if (pitch < 3L * W || band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && img_stride < pitch * (long)band_h) return S2S_ERR_SHAPE;
  p.a = img;
  p.pitch = pitch;
  p.img = img_stride;
  p.band_top = band_top;
  p.band_h = band_h;
  hipLaunchKernelGGL(of_intensity_kernel<OF_U8>, dim3((unsigned)cdiv(W, OF_IW), (unsigned)cdiv(band_h, OF_IH), (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, p, labels, (unsigned long long*)sum_q,
                     (unsigned long long*)sum_q2, max_q);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objfeat_intensity_f32(const int* labels, const float* img, int B, int H, int W, int max_objects,
                                         const float* od_table, const float* unmix, int stain, long* sum_q, long* sum_q2,
                                         int* max_q, void* stream) {
  if (!labels || !img || !sum_q || !sum_q2 || !max_q) return S2S_ERR_NULL;
  OfImage p;
  const int rc = of_image(p, B, H, W, max_objects, od_table, unmix, stain);
  if (rc != S2S_OK) return rc;
  p.a = img;
  p.pitch = W;
  p.chan = (long)H * W;
  p.img = 3L * H * W;
  hipLaunchKernelGGL(of_intensity_kernel<OF_F32>, dim3((unsigned)cdiv(W, OF_IW), (unsigned)cdiv(H, OF_IH), (unsigned)B),
                     dim3(256), 0, (hipStream_t)stream, p, labels, (unsigned long long*)sum_q,
                     (unsigned long long*)sum_q2, max_q);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objfeat_finalize(const int* count, const long* area, const long* moments, const long* edges,
                                    const long* sum_q, const long* sum_q2, const int* max_q, const int* max_d2, int B,
                                    int max_objects, double* out, void* stream) {
  if (!count || !area || !moments || !edges || !out) return S2S_ERR_NULL;
  if (sum_q && (!sum_q2 || !max_q)) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || max_objects < 1 || (long)B * max_objects > 0x7fffffffL) return S2S_ERR_SHAPE;
  const long rows = (long)B * max_objects;
  const OfFinal f{count, (const long long*)area, (const long long*)moments, (const long long*)edges,
                  (const long long*)sum_q, sum_q ? (const long long*)sum_q2 : nullptr, sum_q ? max_q : nullptr, max_d2};
  hipLaunchKernelGGL(of_finalize_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f,
                     max_objects, rows, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
