// Bilinear x2 up-sampling with align_corners=True (+ the zero pad to the skip's size), NHWC.
//
// Replaces nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) followed by F.pad in
// the reference's Up block (src/models/components/task_decoders.py:34,42-47) and its backward.
// The forward writes straight into a channel slice of the decoder's concat buffer (explicit pixel
// stride), optionally adding the per-(sample, channel) time-conditioning bias to its input first
// (FlowMatchingDecoder.forward: x = bottleneck + t[:, :, None, None], task_decoders.py:119-125).
//
// Index arithmetic follows ATen's upsample_bilinear2d: scale = (in-1)/(out-1) in fp32,
// src = scale*dst, i0 = (int)src, i1 = i0 + (i0 < in-1), w1 = src - i0, w0 = 1 - w1.
#include "common.h"
#include <stdlib.h>

namespace {

struct Axis {
  int i0, i1;
  float w0, w1;
};

__device__ __forceinline__ Axis ac_axis(int dst, int n_in, float scale) {
  Axis a;
  const float src = scale * (float)dst;
  a.i0 = (int)src;
  if (a.i0 > n_in - 1) a.i0 = n_in - 1;
  a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
  a.w1 = src - (float)a.i0;
  a.w0 = 1.f - a.w1;
  return a;
}

// The forward kernels' axis: ac_axis with w1 = src - i0 taken as ONE fused multiply-subtract of scale * dst, which is what
// the compiler made of it in the row-sweep kernel; a rounded product followed by a subtract (what it makes of the same
// source inside another loop) differs in the last bit of the weight.  The indices are ac_axis's.
__device__ __forceinline__ Axis ac_axis_fwd(int dst, int n_in, float scale) {
  Axis a = ac_axis(dst, n_in, scale);
  a.w1 = __builtin_fmaf(scale, (float)dst, -(float)a.i0);
  a.w0 = 1.f - a.w1;
  return a;
}

// One forward output, in two steps that both forward kernels compile from this source: the horizontal mix of one source
// row (bias added per tap), then the vertical mix of two such rows.  A mix w0 * p + w1 * q rounds one product and
// fuses the other into the add, and which one is which changes the last bit.  Left to the compiler the choice fell by
// channel parity (it vectorised the row-sweep kernel two channels at a time and paired the products crosswise), and
// differently again in another kernel.  The step's results are pinned to those bits, so the choice is written out:
// channel k of a piece of 8 fuses w1 * q when k is even and w0 * p when k is odd.
__device__ __forceinline__ float up_mix2(float w0, float p, float w1, float q, int k) {
  return (k & 1) ? __builtin_fmaf(w0, p, w1 * q) : __builtin_fmaf(w1, q, w0 * p);
}
__device__ __forceinline__ float up_row_mix(const Axis& ax, float v0, float v1, float b, int k) {
  return up_mix2(ax.w0, v0 + b, ax.w1, v1 + b, k);
}
__device__ __forceinline__ float up_col_mix(const Axis& ay, float h0, float h1, int k) {
  return up_mix2(ay.w0, h0, ay.w1, h1, k);
}

// Thread layout (both directions): a workgroup owns one image row; lanes walk the channel pieces of a pixel first
// (PCB pieces of 8 channels, so a wave touches whole NHWC pixel rows) and the remaining 256/PCB thread slots walk
// the pixels of the row.  Row quantities (vertical tap and weights, row base pointers) are wave-uniform and there
// is no per-element div/mod; the earlier flat-index kernels spent ~300 VALU instructions per 16 B and ran at a
// third of the HBM rate.
__host__ __device__ __forceinline__ int rs_pcb(int C) {
  int p = 1;
  while (p < 32 && p * 8 < C) p <<= 1;
  return p;
}

template <typename T, bool BIAS>
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const T* __restrict__ x, int ldx,
                                                             const float* __restrict__ bias, T* __restrict__ y,
                                                             int ldy, int B, int Hin, int Win, int Hout, int Wout,
                                                             int padT, int padL, int C, int band) {
  const int cp = C >> 3;
  const int Hu = 2 * Hin, Wu = 2 * Win;
  const float sh = Hu > 1 ? (float)(Hin - 1) / (float)(Hu - 1) : 0.f;
  const float sw = Wu > 1 ? (float)(Win - 1) / (float)(Wu - 1) : 0.f;
  const int PCB = rs_pcb(C), WL = 256 / PCB;
  const int pc = threadIdx.x & (PCB - 1), slot = threadIdx.x / PCB;
  // A workgroup takes BANDS of `band` consecutive output rows (round 3): consecutive output rows read the same two
  // input rows, and workgroups are dealt to the eight XCDs round-robin, so with one row per workgroup every XCD's L2
  // fetched every input row (the counters had the launch at 1.6x its algorithmic bytes); a band keeps the shared rows
  // in one L2.
  const int nrows = B * Hout;
  for (int row0 = blockIdx.x * band; row0 < nrows; row0 += gridDim.x * band)
  for (int row = row0; row < row0 + band && row < nrows; ++row) {
    const int n = row / Hout, oy = row - n * Hout;
    const int uy = oy - padT;
    const bool row_in = uy >= 0 && uy < Hu;
    const Axis ay = ac_axis_fwd(row_in ? uy : 0, Hin, sh);
    const T* const r0 = x + ((long)n * Hin + ay.i0) * Win * ldx;
    const T* const r1 = x + ((long)n * Hin + ay.i1) * Win * ldx;
    T* const yr = y + (long)row * Wout * ldy;
    for (int pb = 0; pb < cp; pb += PCB) {
      const int c8 = (pb + pc) * 8;
      if (pb + pc >= cp) continue;
      float bv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) bv[k] = BIAS ? bias[(long)n * C + c8 + k] : 0.f;
      for (int ox = slot; ox < Wout; ox += WL) {
        const int ux = ox - padL;
        f32x8 o;
        if (!row_in || ux < 0 || ux >= Wu) {
#pragma unroll
          for (int k = 0; k < 8; ++k) o.v[k] = 0.f;
        } else {
          const Axis ax = ac_axis_fwd(ux, Win, sw);
          const int o0 = ax.i0 * ldx + c8, o1 = ax.i1 * ldx + c8;
          const f32x8 v00 = load8(r0 + o0), v01 = load8(r0 + o1), v10 = load8(r1 + o0), v11 = load8(r1 + o1);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const float b = bv[k];
            o.v[k] = up_col_mix(ay, up_row_mix(ax, v00.v[k], v01.v[k], b, k), up_row_mix(ax, v10.v[k], v11.v[k], b, k), k);
          }
        }
        store8(yr + ox * ldy + c8, o);
      }
    }
  }
}

// Gather form of the backward: input pixel (iy, ix) collects from every up-sampled pixel that read
// it.  With scale < 1 at most 3 destination rows map their i0 or i1 onto one source row; the
// candidates are bracketed from the inverse scale and tested exactly with the forward's own index
// arithmetic, so forward and backward can never disagree.
template <typename T>
__global__ void upsample2x_bwd_kernel(const T* __restrict__ dy, int lddy, T* __restrict__ dx, int lddx, int B,
                                      int Hin, int Win, int Hout, int Wout, int padT, int padL, int C) {
  const int cp = C >> 3;
  const int Hu = 2 * Hin, Wu = 2 * Win;
  const float sh = Hu > 1 ? (float)(Hin - 1) / (float)(Hu - 1) : 0.f;
  const float sw = Wu > 1 ? (float)(Win - 1) / (float)(Wu - 1) : 0.f;
  const int total = B * Hin * Win * cp;             // 32-bit element index (checked on the host)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t0 = i / cp, c8 = (i - t0 * cp) * 8;
    const int t1 = t0 / Win, ix = t0 - t1 * Win;
    const int n = t1 / Hin, iy = t1 - n * Hin;
    // candidate destination range: rows whose src coordinate lies in (iy-1, iy+1)
    int y_lo, y_hi, x_lo, x_hi;
    if (Hin == 1) { y_lo = 0; y_hi = Hu - 1; }
    else {
      y_lo = (int)floorf((float)(iy - 1) / sh) - 1; y_hi = (int)ceilf((float)(iy + 1) / sh) + 1;
      if (y_lo < 0) y_lo = 0;
      if (y_hi > Hu - 1) y_hi = Hu - 1;
    }
    if (Win == 1) { x_lo = 0; x_hi = Wu - 1; }
    else {
      x_lo = (int)floorf((float)(ix - 1) / sw) - 1; x_hi = (int)ceilf((float)(ix + 1) / sw) + 1;
      if (x_lo < 0) x_lo = 0;
      if (x_hi > Wu - 1) x_hi = Wu - 1;
    }
    // column candidates once per source pixel (they were re-derived for every contributing row): slot j = ux - x_lo,
    // weight 0 = does not read this source column / outside the padded output
    constexpr int NSLOT = 12;                         // the bracket holds at most 2/scale + 5 <= 11 candidates
    float wxs[NSLOT];
#pragma unroll
    for (int j = 0; j < NSLOT; ++j) {
      const int ux = x_lo + j;
      float wx = 0.f;
      if (ux <= x_hi) {
        const Axis ax = ac_axis(ux, Win, sw);
        if (ax.i0 == ix) wx += ax.w0;
        if (ax.i1 == ix) wx += ax.w1;
        const int ox = ux + padL;
        if (ox < 0 || ox >= Wout) wx = 0.f;
      }
      wxs[j] = wx;
    }
    f32x8 acc;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc.v[k] = 0.f;
    for (int uy = y_lo; uy <= y_hi; ++uy) {
      const Axis ay = ac_axis(uy, Hin, sh);
      float wy = 0.f;
      if (ay.i0 == iy) wy += ay.w0;
      if (ay.i1 == iy) wy += ay.w1;
      const int oy = uy + padT;
      if (wy == 0.f || oy < 0 || oy >= Hout) continue;
      const T* const rowp = dy + (((long)n * Hout + oy) * Wout + x_lo + padL) * lddy + c8;
#pragma unroll
      for (int j = 0; j < NSLOT; ++j) {
        if (wxs[j] == 0.f) continue;
        const f32x8 g = load8(rowp + (long)j * lddy);
        const float w = wy * wxs[j];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc.v[k] += w * g.v[k];
      }
    }
    store8(dx + (((long)n * Hin + iy) * Win + ix) * lddx + c8, acc);
  }
}

// The same gather with a FIXED 5 x 5 window of unconditional loads (maps wider than 3 source pixels per axis).  The
// rows that read source row iy are those whose i0 is iy - 1 or iy: consecutive, and at most five of them when
// 2 (2 Hin - 1) / (Hin - 1) < 5, i.e. Hin > 3.  The first one is found by walking the forward's own index arithmetic up
// from a conservative estimate (no loads), the five weights follow from it (zero where a row does not contribute or
// falls outside), and the 25 loads of a thread are independent of any weight test, so they are all in flight at once;
// the loop above issues each load behind a data-dependent branch and is latency-bound (2.3 TB/s).
__device__ __forceinline__ float ac_weight_of(int dst, int n_in, float scale, int src_index) {
  const Axis a = ac_axis(dst, n_in, scale);
  return (a.i0 == src_index ? a.w0 : 0.f) + (a.i1 == src_index ? a.w1 : 0.f);
}

template <typename T>
__global__ void upsample2x_bwd_win_kernel(const T* __restrict__ dy, int lddy, T* __restrict__ dx, int lddx, int B,
                                          int Hin, int Win, int Hout, int Wout, int padT, int padL, int C) {
  const int cp = C >> 3;
  const int Hu = 2 * Hin, Wu = 2 * Win;
  const float sh = (float)(Hin - 1) / (float)(Hu - 1), sw = (float)(Win - 1) / (float)(Wu - 1);
  const int total = B * Hin * Win * cp;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t0 = i / cp, c8 = (i - t0 * cp) * 8;
    const int t1 = t0 / Win, ix = t0 - t1 * Win;
    const int n = t1 / Hin, iy = t1 - n * Hin;
    int uy0 = (int)floorf((float)(iy - 1) / sh) - 1, ux0 = (int)floorf((float)(ix - 1) / sw) - 1;
    if (uy0 < 0) uy0 = 0;
    if (ux0 < 0) ux0 = 0;
    for (int t = 0; t < 8 && uy0 < Hu - 1 && ac_weight_of(uy0, Hin, sh, iy) == 0.f; ++t) ++uy0;
    for (int t = 0; t < 8 && ux0 < Wu - 1 && ac_weight_of(ux0, Win, sw, ix) == 0.f; ++t) ++ux0;
    float wy[5], wx[5];
    int oyc[5], oxc[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int uy = uy0 + j, ux = ux0 + j;
      const int oy = uy + padT, ox = ux + padL;
      wy[j] = (uy <= Hu - 1 && oy >= 0 && oy < Hout) ? ac_weight_of(uy, Hin, sh, iy) : 0.f;
      wx[j] = (ux <= Wu - 1 && ox >= 0 && ox < Wout) ? ac_weight_of(ux, Win, sw, ix) : 0.f;
      oyc[j] = oy < 0 ? 0 : (oy > Hout - 1 ? Hout - 1 : oy);
      oxc[j] = ox < 0 ? 0 : (ox > Wout - 1 ? Wout - 1 : ox);
    }
    f32x8 acc;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc.v[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const T* const rowp = dy + ((long)n * Hout + oyc[j]) * Wout * lddy + c8;
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const f32x8 g = load8(rowp + (long)oxc[m] * lddy);
        const float w = wy[j] * wx[m];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc.v[k] = fmaf(w, g.v[k], acc.v[k]);
      }
    }
    store8(dx + (((long)n * Hin + iy) * Win + ix) * lddx + c8, acc);
  }
}

// 8 channels as loaded (bf16: 4 registers, fp32: 8), widened to fp32 only where they are used; the widening is exact
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> { bf16x8 a; };
template <> struct Raw8<float> { f32x4 a, b; };
__device__ __forceinline__ Raw8<bf16_t> load_raw8(const bf16_t* p) {
  Raw8<bf16_t> r;
  r.a = *reinterpret_cast<const bf16x8*>(p);
  return r;
}
__device__ __forceinline__ Raw8<float> load_raw8(const float* p) {
  Raw8<float> r;
  r.a = *reinterpret_cast<const f32x4*>(p);
  r.b = *reinterpret_cast<const f32x4*>(p + 4);
  return r;
}
__device__ __forceinline__ f32x8 widen8(const Raw8<bf16_t>& r) {
  f32x8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o.v[i] = (float)r.a[i];
  return o;
}
__device__ __forceinline__ f32x8 widen8(const Raw8<float>& r) {
  f32x8 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) { o.v[i] = r.a[i]; o.v[4 + i] = r.b[i]; }
  return o;
}

// an empty statement that makes the compiler hold r's current value in registers here
__device__ __forceinline__ void pin8(f32x8& r) {
#pragma unroll
  for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(r.v[i]));
}

// The production backward for maps of 4 .. 4096 source pixels per axis: the same per-output chain as the window kernel
// above (acc = fmaf(wy * wx, g, acc), rows ascending, columns ascending within a row, weights from ac_weight_of), with
// the window placed in closed form and shared between neighbours.
//
// For n_in in 4..4096 every destination with a non-zero weight on source index i lies in [2i - 1, 2i + 2] (in exact
// arithmetic the source coordinate dst (n-1)/(2n-1) is an integer only at dst = 0 and 2n - 1, and is at least
// 1/(2n-1) away from one elsewhere, far more than the fp32 rounding of scale * dst; the two end points carry weight 0
// or fall on the clamped index; checked exhaustively on the CPU with the kernel's fp32 arithmetic, w1 taken both as a
// rounded subtract and as a fused multiply-subtract).  So a 4 x 4 window holds every term of the 5 x 5 one that is
// not multiplied by 0, and a term multiplied by 0 leaves acc unchanged for finite g: the results are the window
// kernel's bit for bit.  The windows of source pixels 2a and 2a + 1 overlap in two of their four rows / columns, so a
// thread produces a 2 x 2 block of source pixels of one channel piece from ONE 6 x 6 set of loads: 9 loads of 16 B per
// output instead of 25.
//
// Layout as in the forward: a workgroup owns one pair of source rows (and one group of PCB channel pieces); lanes walk
// the channel pieces of a pixel first, the remaining 256/PCB thread slots walk the pixel pairs of the row.  Row taps,
// row weights and row pointers are wave-uniform and there is no per-element div/mod.  Neighbouring row pairs share two
// of their six dy rows; workgroup ids are dealt so that the ids congruent mod 8 (which share an XCD's L2 under the
// round-robin dispatch) take a CONTIGUOUS run of row pairs -- a speed choice only, any placement gives the same result.
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 4 : 2) void upsample2x_bwd_quad_kernel(const T* __restrict__ dy, int lddy,
                                                                  T* __restrict__ dx, int lddx, int B, int Hin,
                                                                  int Win, int Hout, int Wout, int padT, int padL,
                                                                  int C, int nwork) {
  const int cp = C >> 3;
  const int Hu = 2 * Hin, Wu = 2 * Win;
  const float sh = (float)(Hin - 1) / (float)(Hu - 1), sw = (float)(Win - 1) / (float)(Wu - 1);
  const int PCB = rs_pcb(C), WL = 256 / PCB;
  const int pc = threadIdx.x & (PCB - 1), slot = threadIdx.x / PCB;
  const int HP = (Hin + 1) >> 1, WP = (Win + 1) >> 1;
  // bijective deal of the workgroup ids: class b % 8 takes a contiguous run
  const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, cls = blockIdx.x & 7;
  const int wgid = (cls < r ? cls * (q + 1) : r * (q + 1) + (cls - r) * q) + (blockIdx.x >> 3);
  const int chunk = wgid / nwork, work = wgid - chunk * nwork;       // channel group outermost
  // an odd map's last pair is moved back by one: it recomputes the pixel before it (same chain, same bits, written
  // twice), so every thread stores its four pixels unconditionally -- with conditional stores the compiler sank the
  // accumulation into the branches and kept all 36 loads alive (spills)
  const int n = work / HP, iy0 = min(2 * (work - n * HP), Hin - 2);
  const int piece = chunk * PCB + pc;
  if (piece >= cp) return;
  const int c8 = piece * 8;

  float wyA[4], wyB[4];                     // rows 2 iy0 - 1 + j: j = 0..3 feed iy0, j = 2..5 feed iy0 + 1
  const T* rowp[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int uy = 2 * iy0 - 1 + j;
    const bool in = uy >= 0 && uy <= Hu - 1;
    if (j < 4) wyA[j] = in ? ac_weight_of(uy, Hin, sh, iy0) : 0.f;
    if (j >= 2) wyB[j - 2] = in ? ac_weight_of(uy, Hin, sh, iy0 + 1) : 0.f;
    int oy = uy + padT;
    oy = oy < 0 ? 0 : (oy > Hout - 1 ? Hout - 1 : oy);
    rowp[j] = dy + ((long)n * Hout + oy) * Wout * lddy;      // wave-uniform; the lane's channel offset goes into off[]
  }
  T* const dr0 = dx + ((long)n * Hin + iy0) * Win * lddx + c8;
  T* const dr1 = dr0 + (long)Win * lddx;

#pragma unroll 1
  for (int px = slot; px < WP; px += WL) {
    const int ix0 = min(2 * px, Win - 2);
    float wxA[4], wxB[4];
    int off[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      const int ux = 2 * ix0 - 1 + m;
      const bool in = ux >= 0 && ux <= Wu - 1;
      if (m < 4) wxA[m] = in ? ac_weight_of(ux, Win, sw, ix0) : 0.f;
      if (m >= 2) wxB[m - 2] = in ? ac_weight_of(ux, Win, sw, ix0 + 1) : 0.f;
      int ox = ux + padL;
      ox = ox < 0 ? 0 : (ox > Wout - 1 ? Wout - 1 : ox);
      off[m] = ox * lddy + c8;
    }
    f32x8 a00, a01, a10, a11;
#pragma unroll
    for (int k = 0; k < 8; ++k) a00.v[k] = a01.v[k] = a10.v[k] = a11.v[k] = 0.f;
    // one row of raw loads at a time: nothing moves across a row's end, so the register need stays at one row of
    // loads beside the four accumulators whatever the scheduler would like to hoist (it spilled otherwise); the
    // other waves of the SIMD cover the latency
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      Raw8<T> cur[6];
#pragma unroll
      for (int m = 0; m < 6; ++m) cur[m] = load_raw8(rowp[j] + off[m]);
      f32x8 g[6];
#pragma unroll
      for (int m = 0; m < 6; ++m) g[m] = widen8(cur[m]);
      if (j < 4) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float w = wyA[j] * wxA[m];
#pragma unroll
          for (int k = 0; k < 8; ++k) a00.v[k] = fmaf(w, g[m].v[k], a00.v[k]);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float w = wyA[j] * wxB[m];
#pragma unroll
          for (int k = 0; k < 8; ++k) a01.v[k] = fmaf(w, g[m + 2].v[k], a01.v[k]);
        }
      }
      if (j >= 2) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float w = wyB[j - 2] * wxA[m];
#pragma unroll
          for (int k = 0; k < 8; ++k) a10.v[k] = fmaf(w, g[m].v[k], a10.v[k]);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float w = wyB[j - 2] * wxB[m];
#pragma unroll
          for (int k = 0; k < 8; ++k) a11.v[k] = fmaf(w, g[m + 2].v[k], a11.v[k]);
        }
      }
      // the accumulators are pinned at the end of the row: without it the compiler sinks the fmas of three of the four
      // pixels below the last row and keeps all 36 loads alive (spills)
      if (j < 4) { pin8(a00); pin8(a01); }
      if (j >= 2) { pin8(a10); pin8(a11); }
      __builtin_amdgcn_sched_barrier(0);
    }
    // An odd map's moved-back pair stores a row / column that the pair before it stores too, from another thread or
    // workgroup at the same time.  That is safe only because both write the same bits: the pixel is the second of one
    // pair and the first of the other, and both run the same chain on it (same rows, same ac_weight_of arguments,
    // same fmaf order).  Keep the two halves of the accumulation identical.
    store8(dr0 + ix0 * lddx, a00);
    store8(dr0 + (ix0 + 1) * lddx, a01);
    store8(dr1 + ix0 * lddx, a10);
    store8(dr1 + (ix0 + 1) * lddx, a11);
  }
}

// Almost always output row 2a mixes source rows (a - 1, a) and row 2a + 1 rows (a, a + 1).  The first and last output row
// of a map do not (their second tap is clamped or their first is row 0 itself), and whatever else ac_axis may round to
// would not either: the kernel tests every pair, which is wave-uniform.
__device__ __forceinline__ bool up_usual_pair(const Axis (&ay)[2], int a) {
  const bool u = ay[0].i0 == a - 1 && ay[0].i1 == a && ay[1].i0 == a && ay[1].i1 == a + 1;
  return __builtin_amdgcn_readfirstlane((int)u) != 0;
}

// The production forward for maps of 2 .. 4096 source pixels per axis: the same per-output expression as
// upsample2x_fwd_kernel above (up_row_mix, up_col_mix, weights from ac_axis), with the vertical reuse held in registers.
//
// For n_in in 1..4096 outputs 2a and 2a + 1 of an axis read only source indices in [a - 1, a + 1]: i0 is a - 1 or a and
// i1 <= a + 1 (checked exhaustively on the CPU with the kernel's fp32 arithmetic, tests/test_upsample_fwd_window_cpu.py).
// A thread owns source column sx of one channel piece, i.e. output columns 2 sx and 2 sx + 1, and walks down the source
// rows a = a0 .. a1 - 1 of its band.  For each source row it loads the four horizontal taps of its two output columns
// (two of them usually name the same pixel) and mixes them horizontally once: that mix does not depend on the output
// row.  The mixes of rows a - 1, a, a + 1 are what output rows 2a and 2a + 1 need, and two of the three carry over to
// a + 1: one source row of loads per two output rows, where the kernel above loads two per output row, and every source
// row is fetched once per band instead of once per output row.  The window is a matter of speed only: every pair is
// tested (up_usual_pair) and one that does not fit it loads the rows its taps name, in a loop of its own after the walk
// so that the walk's registers stay what the usual pair needs.
//
// A workgroup owns (sample, band of source rows, group of 256/PCB source columns, group of PCB channel pieces); lanes
// walk channel pieces first.  Row taps and weights are wave-uniform.  A band re-reads one source row above and one below
// it (its neighbours' rows); workgroup ids congruent mod 8 take a contiguous run of work items so those stay in one
// XCD's L2.  The zero pad around the up-sampled image belongs to the threads at its edge: the first and last source
// column take the pad columns, the first and last band take the pad rows.  Row bases are wave-uniform 64-bit pointers,
// what a lane adds is an unsigned 32-bit byte offset (the host checks that a row's bytes fit).
template <typename T>
struct UpTaps { Raw8<T> t[2][2]; };          // one source row as loaded: [output column 2 sx + e][tap i0, i1]
struct UpMix2 { f32x8 e[2]; };               // its horizontal mixes for output columns 2 sx and 2 sx + 1

// AFFINE: x is a convolution's raw output and the kernel up-samples relu(bn(x)) without that activation ever being
// stored: every tap value v becomes round_T(fmaxf(fmaf(v, scale[c], shift[c]), 0)) as it is widened, the expression and
// the rounding of bn_relu_apply_kernel, so the result is that of bn_relu_apply followed by this kernel, bit for bit.  The
// time bias is added after it, as to a stored activation; the zero pad is written as zeros and never sees the affine.
// A lane's sixteen constants stay in registers: the bf16 no-bias instance compiles to 120 VGPRs (110 without the affine), so
// it keeps 4 waves per SIMD without scratch; read from LDS per row instead they made the four launches 2 % slower.
template <typename T, bool BIAS, bool AFFINE>
__global__ __launch_bounds__(256, sizeof(T) == 2 && !BIAS ? 4 : 2) void upsample2x_fwd_win_kernel(
    const T* __restrict__ x, int ldx, const float* __restrict__ bias, const float* __restrict__ scale,
    const float* __restrict__ shift, T* __restrict__ y, int ldy, int B, int Hin, int Win, int Hout, int Wout, int padT,
    int padL, int C, int band, int nband, int ncol, int nwork) {
  constexpr unsigned ES = sizeof(T);
  const int cp = C >> 3;
  const int Hu = 2 * Hin, Wu = 2 * Win;
  const float sh = (float)(Hin - 1) / (float)(Hu - 1), sw = (float)(Win - 1) / (float)(Wu - 1);
  const int PCB = rs_pcb(C), WL = 256 / PCB;
  const int pc = threadIdx.x & (PCB - 1), slot = threadIdx.x / PCB;
  // bijective deal of the workgroup ids: class b % 8 takes a contiguous run
  const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, cls = blockIdx.x & 7;
  const int wgid = (cls < r ? cls * (q + 1) : r * (q + 1) + (cls - r) * q) + (blockIdx.x >> 3);
  const int chunk = wgid / nwork;                                     // channel group outermost
  int work = wgid - chunk * nwork;
  const int cg = work % ncol; work /= ncol;
  const int bi = work % nband, n = work / nband;
  const int a0 = bi * band, a1 = min(a0 + band, Hin);
  const int sx = cg * WL + slot, piece = chunk * PCB + pc;
  if (sx >= Win || piece >= cp) return;
  const int c8 = piece * 8;
  float kc0[8], kc1[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { kc0[k] = AFFINE ? scale[c8 + k] : 1.f; kc1[k] = AFFINE ? shift[c8 + k] : 0.f; }

  float bv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bv[k] = BIAS ? bias[(long)n * C + c8 + k] : 0.f;

  const Axis ax[2] = {ac_axis_fwd(2 * sx, Win, sw), ac_axis_fwd(2 * sx + 1, Win, sw)};
  const unsigned off[2][2] = {{(unsigned)(ax[0].i0 * ldx + c8) * ES, (unsigned)(ax[0].i1 * ldx + c8) * ES},
                              {(unsigned)(ax[1].i0 * ldx + c8) * ES, (unsigned)(ax[1].i1 * ldx + c8) * ES}};
  const int ox0 = padL + 2 * sx;
  const unsigned yo[2] = {(unsigned)(ox0 * ldy + c8) * ES, (unsigned)((ox0 + 1) * ldy + c8) * ES};
  const char* const xn = reinterpret_cast<const char*>(x + (long)n * Hin * Win * ldx);
  char* const yn = reinterpret_cast<char*>(y + (long)n * Hout * Wout * ldy);
  const long xrow = (long)Win * ldx * ES, yrow = (long)Wout * ldy * ES;

  auto load_row = [&](int iy) {
    const char* const rp = xn + min(max(iy, 0), Hin - 1) * xrow;
    UpTaps<T> w;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int t = 0; t < 2; ++t) w.t[e][t] = load_raw8(reinterpret_cast<const T*>(rp + off[e][t]));
    return w;
  };
  auto mix_row = [&](const UpTaps<T>& w) {
    UpMix2 m;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      f32x8 v0 = widen8(w.t[e][0]), v1 = widen8(w.t[e][1]);
      if (AFFINE) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          v0.v[k] = to_f32(from_f32<T>(fmaxf(fmaf(v0.v[k], kc0[k], kc1[k]), 0.f)));
          v1.v[k] = to_f32(from_f32<T>(fmaxf(fmaf(v1.v[k], kc0[k], kc1[k]), 0.f)));
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) m.e[e].v[k] = up_row_mix(ax[e], v0.v[k], v1.v[k], bv[k], k);
    }
    return m;
  };
  auto put_row = [&](char* yr, const Axis& ay, const UpMix2& top, const UpMix2& bot) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      f32x8 o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o.v[k] = up_col_mix(ay, top.e[f].v[k], bot.e[f].v[k], k);
      store8(reinterpret_cast<T*>(yr + yo[f]), o);
    }
  };

  UpMix2 m0 = mix_row(load_row(a0 - 1)), m1 = mix_row(load_row(a0)), m2 = mix_row(load_row(a0 + 1));
#pragma unroll 1
  for (int a = a0; a < a1; ++a) {
    // the next source row is on its way while this pair of output rows is mixed and stored (past the band's end it is
    // the clamped row again, which nobody uses)
    const UpTaps<T> nx = load_row(min(a + 2, a1));
    const Axis ay[2] = {ac_axis_fwd(2 * a, Hin, sh), ac_axis_fwd(2 * a + 1, Hin, sh)};
    if (up_usual_pair(ay, a)) {
      char* const yr = yn + (padT + 2 * a) * yrow;
      put_row(yr, ay[0], m0, m1);
      put_row(yr + yrow, ay[1], m1, m2);
    }
    m0 = m1;
    m1 = m2;
    m2 = mix_row(nx);
  }
  // the pairs left out above load the rows that their taps name
#pragma unroll 1
  for (int a = a0; a < a1; ++a) {
    const Axis ay[2] = {ac_axis_fwd(2 * a, Hin, sh), ac_axis_fwd(2 * a + 1, Hin, sh)};
    if (up_usual_pair(ay, a)) continue;
#pragma unroll 1
    for (int e = 0; e < 2; ++e) {
      const Axis ae = ac_axis_fwd(2 * a + e, Hin, sh);
      const UpMix2 top = mix_row(load_row(ae.i0)), bot = mix_row(load_row(ae.i1));
      put_row(yn + (padT + 2 * a + e) * yrow, ae, top, bot);
    }
  }

  // the zero pad: columns left of the first and right of the last source column for this band's rows, and all of this
  // thread's columns in the rows above the first and below the last band
  const int zl = sx == 0 ? 0 : ox0, zr = sx == Win - 1 ? Wout : ox0 + 2;      // this thread's output columns [zl, zr)
  const int ry0 = a0 == 0 ? 0 : padT + 2 * a0, ry1 = a1 == Hin ? Hout : padT + 2 * a1;      // and output rows
  f32x8 zero;
#pragma unroll
  for (int k = 0; k < 8; ++k) zero.v[k] = 0.f;
  for (int oy = ry0; oy < ry1; ++oy) {
    const bool pad_row = oy < padT || oy >= padT + Hu;
    char* const yr = yn + oy * yrow;
    for (int ox = zl; ox < zr; ++ox)
      if (pad_row || ox < ox0 || ox >= ox0 + 2) store8(reinterpret_cast<T*>(yr + (unsigned)(ox * ldy + c8) * ES), zero);
  }
}

// out[n][c] (+)= sum over the H*W pixels of x[n][.][.][c]   (gradient of the broadcast time bias)
template <typename T>
__global__ void pixel_sum_kernel(const T* __restrict__ x, int ldx, float* __restrict__ out, int HW, int C,
                                 int accumulate) {
  const int n = blockIdx.y;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rg = threadIdx.x >> 6;  // 4 pixel groups
  float s = 0.f;
  if (c < C) {
    // a thread's loads are issued ahead of its adds, sixteen at a time; the adds keep their order (p ascending)
    constexpr int U = 16;
    const T* const xp = x + (long)n * HW * ldx + c;
    int p = rg;
    for (; p + 4 * (U - 1) < HW; p += 4 * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = to_f32(xp[(long)(p + 4 * u) * ldx]);
#pragma unroll
      for (int u = 0; u < U; ++u) s += v[u];
    }
    for (; p < HW; p += 4) s += to_f32(xp[(long)p * ldx]);
  }
  __shared__ float red[4][64];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  if (rg == 0 && c < C) {
    s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    out[(long)n * C + c] = accumulate ? out[(long)n * C + c] + s : s;
  }
}

inline int ew_grid(long total) {
  long b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

namespace {

// Which forward kernel a launch takes (s2s_upsample2x_fwd_family hands it to tests): the register-window kernel where
// its window is proven (at most 4096 source pixels per axis), a map has at least two source pixels on both axes, a row's
// bytes fit a 32-bit offset and the work-item count fits 32 bits; else the row-sweep kernel, which is also the test
// reference.
enum UpFwdFamily { kUpFwdRows = 0, kUpFwdWindow = 1 };

// S2S_UP_BAND overrides either forward kernel's band (rows per work item); any value gives the same result
int up_band_env() {
  static const int band_env = [] { const char* e = getenv("S2S_UP_BAND"); return e ? atoi(e) : 0; }();
  return band_env;
}

// source rows per work item of the register-window kernel: 8 where that leaves at least 2048 workgroups (8 per CU, two
// rounds at 4 waves per SIMD), else 4 -- the fastest of 2 / 4 / 8 / 16 / 32 at each of the benchmark's four launches
int upsample2x_fwd_band(int B, int Hin, int Win, int C) {
  if (up_band_env() > 0) return up_band_env();
  const long per_band = (long)B * cdiv(Win, 256 / rs_pcb(C)) * cdiv(C / 8, 32);
  return per_band * cdiv(Hin, 8) >= 2048 ? 8 : 4;
}

int upsample2x_fwd_family(int ldx, int ldy, int B, int Hin, int Win, int Wout, int C, bool reference) {
  if (reference || Hin < 2 || Win < 2 || Hin > 4096 || Win > 4096) return kUpFwdRows;
  if ((long)Win * ldx >= (1L << 29) || (long)Wout * ldy >= (1L << 29)) return kUpFwdRows;   // 32-bit byte offsets in a row
  const long nwg = (long)B * cdiv(Hin, upsample2x_fwd_band(B, Hin, Win, C)) * cdiv(Win, 256 / rs_pcb(C)) *
                   cdiv(C / 8, 32);
  return nwg < (1L << 31) ? kUpFwdWindow : kUpFwdRows;
}

int upsample2x_fwd_check(int ldx, int ldy, int B, int Hin, int Win, int Hout, int Wout, int C) {
  if (B <= 0 || Hin <= 0 || Win <= 0 || C <= 0 || (C % 8) || (ldx % 8) || (ldy % 8)) return S2S_ERR_SHAPE;
  if (Hout < 2 * Hin || Wout < 2 * Win) return S2S_ERR_SHAPE;  // F.pad with a negative size (crop) is not supported
  if ((long)Win * ldx >= (1L << 31) || (long)Wout * ldy >= (1L << 31) || (long)B * Hout >= (1L << 31))
    return S2S_ERR_SHAPE;                                        // 32-bit offsets inside a row
  return S2S_OK;
}

// `reference`: the row-sweep kernel that the register-window kernel replaced (tests compare the two bit for bit)
// scale / shift (both or neither): the window kernel's affine form; the row-sweep kernel has none, so a launch that
// would take it is refused (the caller applies bn_relu_apply first)
int upsample2x_fwd_launch(int dtype, const void* x, int ldx, const float* bias_nc, void* y, int ldy, int B, int Hin,
                          int Win, int Hout, int Wout, int C, void* stream, bool reference,
                          const float* scale = nullptr, const float* shift = nullptr) {
  if (!x || !y) return S2S_ERR_NULL;
  if (int rc = upsample2x_fwd_check(ldx, ldy, B, Hin, Win, Hout, Wout, C)) return rc;
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  const int padT = (Hout - 2 * Hin) / 2, padL = (Wout - 2 * Win) / 2;
  hipStream_t s = (hipStream_t)stream;
  if (upsample2x_fwd_family(ldx, ldy, B, Hin, Win, Wout, C, reference) == kUpFwdWindow) {
    const int band = upsample2x_fwd_band(B, Hin, Win, C), nband = cdiv(Hin, band);
    const int ncol = cdiv(Win, 256 / rs_pcb(C)), nwork = B * nband * ncol;
    const dim3 wgrid((unsigned)((long)nwork * cdiv(C / 8, 32)));
#define S2S_UPW(TT, BB, AA)                                                                                         \
  hipLaunchKernelGGL((upsample2x_fwd_win_kernel<TT, BB, AA>), wgrid, dim3(256), 0, s, (const TT*)x, ldx, bias_nc, scale, \
                     shift, (TT*)y, ldy, B, Hin, Win, Hout, Wout, padT, padL, C, band, nband, ncol, nwork)
    if (scale) {
      if (dtype == S2S_BF16) { if (bias_nc) S2S_UPW(bf16_t, true, true); else S2S_UPW(bf16_t, false, true); }
      else { if (bias_nc) S2S_UPW(float, true, true); else S2S_UPW(float, false, true); }
    } else {
      if (dtype == S2S_BF16) { if (bias_nc) S2S_UPW(bf16_t, true, false); else S2S_UPW(bf16_t, false, false); }
      else { if (bias_nc) S2S_UPW(float, true, false); else S2S_UPW(float, false, false); }
    }
#undef S2S_UPW
    S2S_LAUNCH_CHECK();
    return S2S_OK;
  }
  if (scale) return S2S_ERR_SHAPE;
  const long rows = (long)B * Hout;
  // rows per workgroup: 4 while that still leaves >= 1024 workgroups (4 per CU), else 2, else 1 (S2S_UP_BAND overrides)
  const int band = up_band_env() > 0 ? up_band_env() : (rows >= 4096 ? 4 : rows >= 2048 ? 2 : 1);
  const long nwg = (rows + band - 1) / band;
  const dim3 grid((unsigned)(nwg < 65535 * 4 ? nwg : 65535 * 4));
#define S2S_UP(TT, BB)                                                                                          \
  hipLaunchKernelGGL((upsample2x_fwd_kernel<TT, BB>), grid, dim3(256), 0, s, (const TT*)x, ldx, bias_nc, (TT*)y, \
                     ldy, B, Hin, Win, Hout, Wout, padT, padL, C, band)
  if (dtype == S2S_BF16) { if (bias_nc) S2S_UP(bf16_t, true); else S2S_UP(bf16_t, false); }
  else { if (bias_nc) S2S_UP(float, true); else S2S_UP(float, false); }
#undef S2S_UP
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_upsample2x_bilinear_ac_fwd(int dtype, const void* x, int ldx, const float* bias_nc, void* y,
                                              int ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                                              void* stream) {
  return upsample2x_fwd_launch(dtype, x, ldx, bias_nc, y, ldy, B, Hin, Win, Hout, Wout, C, stream, false);
}

// The up-sampling of relu(bn(x)) from the convolution's raw output x, with that layer's folded scale / shift (rows 2 and
// 3 of bn_finalize): the result of s2s_bn_relu_apply followed by s2s_upsample2x_bilinear_ac_fwd, bit for bit, without the
// activation in between.  Shapes for which s2s_upsample2x_fwd_family answers 0 (the row-sweep kernel) are refused with
// S2S_ERR_SHAPE.
extern "C" int s2s_upsample2x_bn_relu_fwd(int dtype, const void* x, int ldx, const float* scale, const float* shift,
                                          const float* bias_nc, void* y, int ldy, int B, int Hin, int Win, int Hout,
                                          int Wout, int C, void* stream) {
  if (!scale || !shift) return S2S_ERR_NULL;
  return upsample2x_fwd_launch(dtype, x, ldx, bias_nc, y, ldy, B, Hin, Win, Hout, Wout, C, stream, false, scale, shift);
}

// test-facing: the kernel the production entry point replaced, on the same arguments
extern "C" int s2s_upsample2x_bilinear_ac_fwd_ref(int dtype, const void* x, int ldx, const float* bias_nc, void* y,
                                                  int ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                                                  void* stream) {
  return upsample2x_fwd_launch(dtype, x, ldx, bias_nc, y, ldy, B, Hin, Win, Hout, Wout, C, stream, true);
}

// test-facing, no launch: 0 = row-sweep kernel, 1 = register-window kernel, < 0 = the shape error the launch would
// return.  reference != 0: as s2s_upsample2x_bilinear_ac_fwd_ref chooses.
extern "C" int s2s_upsample2x_fwd_family(int ldx, int ldy, int B, int Hin, int Win, int Hout, int Wout, int C,
                                         int reference) {
  if (int rc = upsample2x_fwd_check(ldx, ldy, B, Hin, Win, Hout, Wout, C)) return rc;
  return upsample2x_fwd_family(ldx, ldy, B, Hin, Win, Wout, C, reference != 0);
}

namespace {

// Which backward kernel a launch takes (UpBwdFamily; s2s_upsample2x_bwd_family hands it to tests): the branching gather
// for maps of fewer than 4 source pixels on an axis, the 2 x 2 kernel where its window placement is proven (4..4096
// source pixels per axis) and its 32-bit offsets inside a row hold, else the per-pixel window kernel.
enum UpBwdFamily { kUpBwdGather = 0, kUpBwdWindow = 1, kUpBwdQuad = 2 };

int upsample2x_bwd_family(int lddy, int lddx, int B, int Hin, int Win, int Wout, int C, bool reference) {
  if (!(Hin > 3 && Win > 3)) return kUpBwdGather;
  const long nwork = (long)B * ((Hin + 1) / 2);
  const bool quad = !reference && Hin <= 4096 && Win <= 4096 && (long)Wout * lddy < (1L << 31) &&
                    (long)Win * lddx < (1L << 31) && nwork * cdiv(C / 8, 32) < (1L << 31);
  return quad ? kUpBwdQuad : kUpBwdWindow;
}

// `reference`: the per-pixel 5 x 5 window kernel that the 2 x 2 kernel replaced (tests compare the two bit for bit)
int upsample2x_bwd_launch(int dtype, const void* dy, int lddy, void* dx, int lddx, int B, int Hin, int Win, int Hout,
                          int Wout, int C, void* stream, bool reference) {
  if (!dy || !dx) return S2S_ERR_NULL;
  if (B <= 0 || Hin <= 0 || Win <= 0 || C <= 0 || (C % 8) || (lddy % 8) || (lddx % 8)) return S2S_ERR_SHAPE;
  if (Hout < 2 * Hin || Wout < 2 * Win) return S2S_ERR_SHAPE;
  const int padT = (Hout - 2 * Hin) / 2, padL = (Wout - 2 * Win) / 2;
  const long total = (long)B * Hin * Win * (C / 8);
  if (total >= (1L << 31) - (1L << 22)) return S2S_ERR_SHAPE;   // 32-bit element index in the kernel
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(ew_grid(total));
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  const int family = upsample2x_bwd_family(lddy, lddx, B, Hin, Win, Wout, C, reference);
  const bool win = family != kUpBwdGather;   // at most five contributing rows / columns per source pixel
  const int nchunk = cdiv(C / 8, 32);        // rs_pcb(C) channel pieces per workgroup; one group whenever C <= 256
  const long nwork = (long)B * ((Hin + 1) / 2);
  if (family == kUpBwdQuad) {
    const dim3 qgrid((unsigned)(nwork * nchunk));
    if (dtype == S2S_BF16)
      hipLaunchKernelGGL(upsample2x_bwd_quad_kernel<bf16_t>, qgrid, dim3(256), 0, s, (const bf16_t*)dy, lddy,
                         (bf16_t*)dx, lddx, B, Hin, Win, Hout, Wout, padT, padL, C, (int)nwork);
    else
      hipLaunchKernelGGL(upsample2x_bwd_quad_kernel<float>, qgrid, dim3(256), 0, s, (const float*)dy, lddy, (float*)dx,
                         lddx, B, Hin, Win, Hout, Wout, padT, padL, C, (int)nwork);
    S2S_LAUNCH_CHECK();
    return S2S_OK;
  }
#define S2S_UPB(KERN, TT)                                                                                           \
  hipLaunchKernelGGL(KERN<TT>, grid, dim3(256), 0, s, (const TT*)dy, lddy, (TT*)dx, lddx, B, Hin, Win, Hout, Wout,   \
                     padT, padL, C)
  if (dtype == S2S_BF16) { if (win) S2S_UPB(upsample2x_bwd_win_kernel, bf16_t); else S2S_UPB(upsample2x_bwd_kernel, bf16_t); }
  else { if (win) S2S_UPB(upsample2x_bwd_win_kernel, float); else S2S_UPB(upsample2x_bwd_kernel, float); }
#undef S2S_UPB
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_upsample2x_bilinear_ac_bwd(int dtype, const void* dy, int lddy, void* dx, int lddx, int B, int Hin,
                                              int Win, int Hout, int Wout, int C, void* stream) {
  return upsample2x_bwd_launch(dtype, dy, lddy, dx, lddx, B, Hin, Win, Hout, Wout, C, stream, false);
}

// test-facing: the kernel the production entry point replaced, on the same arguments
extern "C" int s2s_upsample2x_bilinear_ac_bwd_ref(int dtype, const void* dy, int lddy, void* dx, int lddx, int B,
                                                  int Hin, int Win, int Hout, int Wout, int C, void* stream) {
  return upsample2x_bwd_launch(dtype, dy, lddy, dx, lddx, B, Hin, Win, Hout, Wout, C, stream, true);
}

// test-facing, no launch: 0 = branching gather, 1 = per-pixel window kernel, 2 = 2 x 2 kernel, < 0 = the shape error the
// launch would return.  reference != 0: as s2s_upsample2x_bilinear_ac_bwd_ref chooses.
extern "C" int s2s_upsample2x_bwd_family(int lddy, int lddx, int B, int Hin, int Win, int Hout, int Wout, int C,
                                         int reference) {
  if (B <= 0 || Hin <= 0 || Win <= 0 || C <= 0 || (C % 8) || (lddy % 8) || (lddx % 8)) return S2S_ERR_SHAPE;
  if (Hout < 2 * Hin || Wout < 2 * Win) return S2S_ERR_SHAPE;
  if ((long)B * Hin * Win * (C / 8) >= (1L << 31) - (1L << 22)) return S2S_ERR_SHAPE;
  return upsample2x_bwd_family(lddy, lddx, B, Hin, Win, Wout, C, reference != 0);
}

extern "C" int s2s_pixel_sum(int dtype, const void* x, int ldx, float* out_nc, int B, int HW, int C, int accumulate,
                             void* stream) {
  if (!x || !out_nc) return S2S_ERR_NULL;
  if (B <= 0 || HW <= 0 || C <= 0) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(cdiv(C, 64), B);
  if (dtype == S2S_BF16)
    hipLaunchKernelGGL(pixel_sum_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)x, ldx, out_nc, HW, C, accumulate);
  else if (dtype == S2S_F32)
    hipLaunchKernelGGL(pixel_sum_kernel<float>, grid, dim3(256), 0, s, (const float*)x, ldx, out_nc, HW, C, accumulate);
  else return S2S_ERR_DTYPE;
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
