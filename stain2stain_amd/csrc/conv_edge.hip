// The two bandwidth-bound convolutions at the ends of the U-Net.
//
//   * stem: Conv3x3(pad 1) from the image tensor (NCHW fp32, Cin <= 6: RGB, or RGB + mask channel) to NHWC features -- the first conv of
//     SharedEncoder.inc (src/models/components/shared_encoder.py:15,67).  Forward: one K = 32 MFMA step on an
//     im2col patch built in LDS (kernel in conv3x3_mfma.hip, next to the shared epilogue); weight/bias gradient:
//     the MFMA kernel below.  The layer is bound by moving its 64-channel output / gradient.
//   * head: Conv1x1 from NHWC features to the NCHW fp32 velocity field -- FlowMatchingDecoder.outc
//     (src/models/components/task_decoders.py:100,132,169), Cout <= 8 (3 RGB, 1 mask, up to 8 classes).
// and their backward passes (weight / bias gradients; the stem needs no data gradient).
#include "common.h"

namespace {

constexpr int STEM_MAX_CIN = 8;

// ---------------------------------------------------------------------------------------------
// stem weight / bias gradient on MFMA:
//   D[co][k] = sum_p dY[p][co] * P[p][k],  k = ci*9 + tap (Cin*9 <= 31 columns used), P[p][Cin*9] = 1 (bias)
// One workgroup walks 16x16 pixel tiles.  dY is staged as [pixel][32 co] images and the im2col patch
// P as a [pixel][32 k] image (built in LDS from the fp32 halo), both read with ds_read_b64_tr_b16 exactly
// like conv3x3_wgrad_mfma.hip.  Wave w owns output channels 32*(w&1).. and the pixel half (w>>1) of
// every tile; partial slabs part[2*gridDim.x][Cout][32] are folded by stem_wgrad_reduce_kernel.
// T = float: three-way bf16 split of both operands, six MFMAs (see conv3x3_mfma.hip).
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ bf16x8 tr_frag8(const char* p) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * 64));
  bf16x4 l4 = __builtin_bit_cast(bf16x4, lo), h4 = __builtin_bit_cast(bf16x4, hi);
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = l4[i]; r[4 + i] = h4[i]; }
  return r;
}

template <int NIMG>
__device__ __forceinline__ void split_store(char* base, int img_stride, int off, const float* v8) {
  bf16x8 h, m, l;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    h[i] = (bf16_t)v8[i];
    const float r1 = v8[i] - (float)h[i];
    m[i] = (bf16_t)r1;
    l[i] = (bf16_t)(r1 - (float)m[i]);
  }
  *reinterpret_cast<bf16x8*>(base + off) = h;
  if (NIMG == 3) {
    *reinterpret_cast<bf16x8*>(base + img_stride + off) = m;
    *reinterpret_cast<bf16x8*>(base + 2 * img_stride + off) = l;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const T* __restrict__ dy, int lddy,
                                                         const float* __restrict__ x, float* __restrict__ part,
                                                         int B, int H, int W, int Cin, int Cout, int tilesY,
                                                         int tilesX) {
  constexpr int NIMG = sizeof(T) == 4 ? 3 : 1;
  constexpr int NPX = 256;
  constexpr int DY_IMG = 2 * NPX * 64;      // two 32-channel images of 64-B rows
  constexpr int P_IMG = NPX * 64;           // [pixel][32 k]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ldsDY = smem;                                  // [NIMG][2][256][64B]
  char* const ldsP = smem + NIMG * DY_IMG;                   // [NIMG][256][64B]
  float* const xl = reinterpret_cast<float*>(ldsP + NIMG * P_IMG);  // [Cin][18][18]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave & 1, whalf = wave >> 1;
  const int co0 = blockIdx.y * 64;
  const int c0 = blockIdx.z * 3;                             // channel group (27 of 32 k-columns, +1 for the bias)
  const int nc = (Cin - c0) < 3 ? (Cin - c0) : 3, K = nc * 9;
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
  const int frag_off = ((g >> 1) * 8 + q) * 64 + ((g & 1) * 16 + pq * 4) * 2;
  const int ntiles = B * tilesY * tilesX;
  f32x16 acc;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int bt = tile;
    const int tx = bt % tilesX; bt /= tilesX;
    const int ty = bt % tilesY;
    const int n = bt / tilesY;
    const int y0 = ty * 16, x0 = tx * 16;
    __syncthreads();   // previous tile fully consumed
    for (int i = tid; i < nc * 324; i += 256) {
      const int ci = i / 324, r = i - ci * 324, hy = r / 18, hx = r - hy * 18;
      const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
      xl[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? x[(((long)n * Cin + c0 + ci) * H + gy) * W + gx] : 0.f;
    }
    // dY tile: 256 px x 64 co = 2048 pieces of 8 channels
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = tid + it * 256;
      const int px = idx >> 3, pc = idx & 7;
      const int gy = y0 + (px >> 4), gx = x0 + (px & 15), co = co0 + pc * 8;
      float v8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v8[k] = 0.f;
      if (gy < H && gx < W && co < Cout) {
        const f32x8 v = load8(dy + (((long)n * H + gy) * W + gx) * lddy + co);
#pragma unroll
        for (int k = 0; k < 8; ++k) v8[k] = v.v[k];
      }
      split_store<NIMG>(ldsDY, DY_IMG, (pc >> 2) * (NPX * 64) + px * 64 + (pc & 3) * 16, v8);
    }
    __syncthreads();   // halo visible
    {                  // im2col row of pixel `tid`: k = ci*9+tap, column K = 1 (bias), rest 0
      const int py = tid >> 4, px = tid & 15;
      const bool inside = (y0 + py < H) && (x0 + px < W);
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        float v8[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int kk = c4 * 8 + k;
          float v = 0.f;
          if (kk < K) {
            const int ci = kk / 9, t = kk - ci * 9;
            v = xl[ci * 324 + (py + t / 3) * 18 + px + t % 3];
          } else if (kk == K && c0 == 0) {
            v = inside ? 1.f : 0.f;   // dY is zero outside anyway
          }
          v8[k] = v;
        }
        split_store<NIMG>(ldsP, P_IMG, tid * 64 + c4 * 16, v8);
      }
    }
    __syncthreads();
    const char* A0 = ldsDY + wco * (NPX * 64) + frag_off;
    const char* B0 = ldsP + frag_off;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int m0 = (whalf * 8 + ks) * 16;
      const bf16x8 ah = tr_frag8(A0 + m0 * 64);
      const bf16x8 bh = tr_frag8(B0 + m0 * 64);
      if constexpr (NIMG == 3) {
        const bf16x8 am = tr_frag8(A0 + DY_IMG + m0 * 64), al = tr_frag8(A0 + 2 * DY_IMG + m0 * 64);
        const bf16x8 bm = tr_frag8(B0 + P_IMG + m0 * 64), bl = tr_frag8(B0 + 2 * P_IMG + m0 * 64);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
      }
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    }
  }
  // D[co][k]: column = lane&31 = k, rows = co
  const int kcol = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int co = co0 + wco * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
    if (co < Cout)
      part[((((long)blockIdx.z * gridDim.x + blockIdx.x) * 2 + whalf) * Cout + co) * 32 + kcol] = acc[j];
  }
}

// ---------------------------------------------------------------------------------------------
// bf16: the same computation with its operands in flight while the MFMAs run.  Per tile the kernel above runs global
// loads -> ds_write -> barrier -> im2col build -> barrier -> 8 MFMA steps -> barrier, with nothing outstanding during the
// MFMAs; a workgroup walks 8 tiles of the 256^2 x 16 batch that way at 2.0 TB/s.  Here
//   * the two [pixel][32 co] images of dY arrive by LDS-DMA (global_load_lds_dwordx4, one 16-pixel row of an image per
//     wave instruction, as conv3x3_wgrad_dma_kernel stages its operands) into the OTHER of two buffers while the
//     current tile's MFMAs run; pixels past the image and channels past Cout fetch a zero page, so every wave issues the
//     same 8 DMAs per tile;
//   * the 27 fp32 taps of a thread's own pixel for the next tile are loaded (predicated) into registers at the same
//     time, straight from the image -- neighbouring threads' taps overlap, the loads hit in L1 / L2 -- so there is no
//     fp32 halo in LDS and no barrier between it and the im2col build;
//   * LDS is two dY buffers of 32 KB and ONE 16 KB patch: 80 KB, two workgroups per CU.  The single patch costs a
//     second barrier per tile (all MFMAs of tile i before the patch of tile i + 1 is written), with the DMAs still in
//     flight across it.
// The arithmetic is the kernel's above: the same tiles in the same order per (block, pixel half) slab, the same chain of
// eight MFMAs per tile (ks ascending) on the same bf16 values (dY as stored, the patch rounded from the same fp32 taps),
// the same partial layout: the results are equal bit for bit.
// ---------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(64))) char g_stem_zero_page[64];

// LDS-DMA from inline asm (see dma16_asm in conv3x3_wgrad_mfma.hip: the compiler's waitcnt pass does not see it, so
// completion is tracked by the explicit vmcnt(0) below; M0 carries the wave-uniform LDS destination and is restored)
__device__ __forceinline__ void stem_dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

constexpr int STEM_PIPE_LDS = 2 * (2 * 256 * 64) + 256 * 64;      // 81920

__global__ __launch_bounds__(256, 2) void stem_wgrad_pipe_kernel(const bf16_t* __restrict__ dy, int lddy,
                                                                 const float* __restrict__ x, float* __restrict__ part,
                                                                 int B, int H, int W, int Cin, int Cout, int tilesY,
                                                                 int tilesX) {
  constexpr int NPX = 256;
  constexpr int DY_IMG = 2 * NPX * 64;      // one buffer: two 32-channel images of 64-B rows
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const ldsP = smem + 2 * DY_IMG;                      // [256][64B]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wco = wave & 1, whalf = wave >> 1;
  const int co0 = blockIdx.y * 64;
  const int c0 = blockIdx.z * 3;
  const int nc = (Cin - c0) < 3 ? (Cin - c0) : 3, K = nc * 9;
  const int g = lane >> 4, q = (lane & 15) >> 2, pq = lane & 3;
  const int frag_off = ((g >> 1) * 8 + q) * 64 + ((g & 1) * 16 + pq * 4) * 2;
  const int ntiles = B * tilesY * tilesX;
  const int drow = lane >> 2, dslot = lane & 3;              // a DMA lane's pixel of the 16-pixel row, its 8-channel piece
  const int py = tid >> 4, px = tid & 15;                    // the pixel whose im2col row this thread builds
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

  // tile -> (sample, first row, first column)
  auto origin = [&](int tile, int& n, int& y0, int& x0) {
    int bt = tile;
    const int tx = bt % tilesX; bt /= tilesX;
    const int ty = bt % tilesY;
    n = bt / tilesY; y0 = ty * 16; x0 = tx * 16;
  };
  // DMA group grp = wave + 4 j: image grp / 16 (channels co0 + 32 (grp / 16) ..), tile row grp % 16
  auto dma_tile = [&](int tile, int buf) {
    int n, y0, x0;
    origin(tile, n, y0, x0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int grp = wave + 4 * j;
      const int gy = y0 + (grp & 15), gx = x0 + drow, co = co0 + (grp >> 4) * 32 + dslot * 8;
      const bool in = gy < H && gx < W && co < Cout;
      const bf16_t* const pix = dy + (((long)n * H + min(gy, H - 1)) * W + min(gx, W - 1)) * lddy + min(co, Cout - 8);
      const void* const src = in ? (const void*)pix : (const void*)g_stem_zero_page;
      stem_dma16(src, __builtin_amdgcn_readfirstlane(lds0 + buf * DY_IMG + grp * 1024));
    }
  };
  // the thread's 27 taps (k = ci * 9 + tap) as loaded, bit kk of `in` = tap kk is inside the image and the group's
  // channels (build_patch zeroes the others: a use of the loaded values here would wait for them in front of the MFMAs),
  // and its bias column
  auto load_taps = [&](int tile, float (&tp)[27], unsigned& in, float& one) {
    int n, y0, x0;
    origin(tile, n, y0, x0);
    one = (y0 + py < H && x0 + px < W) ? 1.f : 0.f;          // dY is zero outside anyway
    // every load is unconditional, from the address clamped into the image and the group's channels: a branch per tap
    // otherwise
    in = 0u;
#pragma unroll
    for (int kk = 0; kk < 27; ++kk) {
      const int ci = kk / 9, t = kk - ci * 9;
      const int gy = y0 + py + t / 3 - 1, gx = x0 + px + t % 3 - 1;
      in |= (unsigned)(kk < K && gy >= 0 && gy < H && gx >= 0 && gx < W) << kk;
      const int cc = c0 + min(ci, nc - 1), yy = min(max(gy, 0), H - 1), xx = min(max(gx, 0), W - 1);
      tp[kk] = x[(((long)n * Cin + cc) * H + yy) * W + xx];
    }
  };
  auto build_patch = [&](const float (&tp)[27], unsigned in, float one) {
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      float v8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int kk = c4 * 8 + k;
        float v = (kk < 27 && ((in >> (kk & 31)) & 1u)) ? tp[kk < 27 ? kk : 0] : 0.f;
        if (kk == K && c0 == 0) v = one;
        v8[k] = v;
      }
      split_store<1>(ldsP, 0, tid * 64 + c4 * 16, v8);
    }
  };

  f32x16 acc;
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  float tp[27], one;
  unsigned tin;
  int tile = blockIdx.x, buf = 0;
  if (tile < ntiles) {
    dma_tile(tile, 0);
    load_taps(tile, tp, tin, one);
    build_patch(tp, tin, one);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
    const bool more = tile + (int)gridDim.x < ntiles;        // block-uniform
    // Both land while the MFMAs below run.  The taps go first: the compiler cannot see the vmcnt(0) at the loop's end, so
    // it waits for the previous iteration's tap loads before it overwrites their registers -- a wait that is free as
    // long as no DMA has been issued yet, and one for the DMAs otherwise.
    if (more) {
      load_taps(tile + gridDim.x, tp, tin, one);
      dma_tile(tile + gridDim.x, buf ^ 1);
    }
    __builtin_amdgcn_sched_barrier(0);                       // nothing that waits for those loads moves up here
    const char* A0 = smem + buf * DY_IMG + wco * (NPX * 64) + frag_off;
    const char* B0 = ldsP + frag_off;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const int m0 = (whalf * 8 + ks) * 16;
      const bf16x8 ah = tr_frag8(A0 + m0 * 64);
      const bf16x8 bh = tr_frag8(B0 + m0 * 64);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      __syncthreads();   // every wave has read the patch of this tile
      build_patch(tp, tin, one);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the next tile's dY images have landed
      __syncthreads();
    }
  }
  const int kcol = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int co = co0 + wco * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
    if (co < Cout)
      part[((((long)blockIdx.z * gridDim.x + blockIdx.x) * 2 + whalf) * Cout + co) * 32 + kcol] = acc[j];
  }
}

// one workgroup per (output channel, channel group): 32 k-columns x 32 slab groups (1024 slabs: 32 loads a thread)
__global__ __launch_bounds__(1024) void stem_wgrad_reduce_kernel(const float* part, int nslab, int Cout, int Cin, float* dw, float* db,
                                         int accumulate) {
  __shared__ double red[32][33];
  const int c0 = blockIdx.y * 3;
  const int K = ((Cin - c0) < 3 ? (Cin - c0) : 3) * 9;
  const int co = blockIdx.x, k = threadIdx.x & 31, sg = threadIdx.x >> 5;
  part += (long)blockIdx.y * nslab * Cout * 32;
  double s = 0.0, s1 = 0.0;
  int b = sg;
  for (; b + 32 < nslab; b += 64) {
    s += (double)part[((long)b * Cout + co) * 32 + k];
    s1 += (double)part[((long)(b + 32) * Cout + co) * 32 + k];
  }
  for (; b < nslab; b += 32) s += (double)part[((long)b * Cout + co) * 32 + k];
  s += s1;
  red[sg][k] = s;
  __syncthreads();
  if (sg == 0) {
    for (int j = 1; j < 32; ++j) s += red[j][k];
    if (k < K) {
      float* dst = dw + co * Cin * 9 + c0 * 9 + k;
      *dst = accumulate ? *dst + (float)s : (float)s;
    } else if (k == K && c0 == 0 && db) {
      db[co] = accumulate ? db[co] + (float)s : (float)s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// head: 1x1 conv NHWC -> NCHW fp32
// ---------------------------------------------------------------------------------------------
constexpr int HEAD_MAX_COUT = 4;      // fused head+loss kernel (flow head, 3 channels)
constexpr int HEAD_WIDE_COUT = 8;     // plain head kernels (segmentation head: num_classes)

template <typename T, int MO>
__global__ void head_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                const float* __restrict__ bias, float* __restrict__ y, long npix, int HW, int C,
                                int Cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);  // [Cout][C]
  for (int i = threadIdx.x; i < Cout * C; i += blockDim.x) wl[i] = w[i];
  __syncthreads();
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    float acc[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) acc[o] = 0.f;
    for (int c8 = 0; c8 < C; c8 += 8) {
      const f32x8 v = load8(x + p * ldx + c8);
#pragma unroll
      for (int o = 0; o < MO; ++o)
        if (o < Cout)
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[o] = fmaf(v.v[k], wl[o * C + c8 + k], acc[o]);
    }
    const long n = p / HW, q = p - n * HW;
#pragma unroll
    for (int o = 0; o < MO; ++o)
      if (o < Cout) y[(n * Cout + o) * HW + q] = acc[o] + (bias ? bias[o] : 0.f);
  }
}

// dX[p][c] = sum_o dY[n][o][q] * W[o][c]
template <typename T, int MO>
__global__ void head_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                     int lddx, long npix, int HW, int C, int Cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);
  for (int i = threadIdx.x; i < Cout * C; i += blockDim.x) wl[i] = w[i];
  __syncthreads();
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long)gridDim.x * blockDim.x) {
    const long n = p / HW, q = p - n * HW;
    float g[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) g[o] = o < Cout ? dy[(n * Cout + o) * HW + q] : 0.f;
    for (int c8 = 0; c8 < C; c8 += 8) {
      f32x8 v;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float a = 0.f;
#pragma unroll
        for (int o = 0; o < MO; ++o)
          if (o < Cout) a = fmaf(g[o], wl[o * C + c8 + k], a);
        v.v[k] = a;
      }
      store8(dx + p * lddx + c8, v);
    }
  }
}

// dW[o][c] = sum_p dY[p][o]*X[p][c], db[o] = sum_p dY[p][o]; part[gridDim.x][Cout][C+1]
template <typename T, int MO>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ dy, const T* __restrict__ x,
                                                         int ldx, float* __restrict__ part, long npix, int HW, int C,
                                                         int Cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xl = reinterpret_cast<float*>(smem);            // [64 px][C+1]
  float* gl = xl + 64 * (C + 1);                         // [64 px][MO]
  const int nout = Cout * (C + 1);
  float acc[8];                                          // outputs tid, tid+256, ... (nout <= 2048)
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (long p0 = (long)blockIdx.x * 64; p0 < npix; p0 += (long)gridDim.x * 64) {
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * C; i += 256) {
      const int pp = i / C, c = i - pp * C;
      xl[pp * (C + 1) + c] = (p0 + pp < npix) ? to_f32(x[(p0 + pp) * ldx + c]) : 0.f;
    }
    for (int i = threadIdx.x; i < 64 * MO; i += 256) {
      const int pp = i / MO, o = i - pp * MO;
      float v = 0.f;
      if (o < Cout && p0 + pp < npix) {
        const long p = p0 + pp, n = p / HW, q = p - n * HW;
        v = dy[(n * Cout + o) * HW + q];
      }
      gl[i] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int id = threadIdx.x + i * 256;
      if (id < nout) {
        const int o = id / (C + 1), c = id - o * (C + 1);
        float a = acc[i];
        if (c < C) for (int pp = 0; pp < 64; ++pp) a = fmaf(gl[pp * MO + o], xl[pp * (C + 1) + c], a);
        else for (int pp = 0; pp < 64; ++pp) a += gl[pp * MO + o];
        acc[i] = a;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int id = threadIdx.x + i * 256;
    if (id < nout) part[(long)blockIdx.x * nout + id] = acc[i];
  }
}

// part[nblk][nout] -> dw/db; 8 outputs x 32 block groups per workgroup (the 195 outputs of the 64 -> 3 head give
// 25 workgroups; with 32 outputs each there were 7 and the 1024-row sum took 34 us)
__global__ __launch_bounds__(256) void head_wgrad_reduce_kernel(const float* part, int nblk, int Cout, int C, float* dw, float* db,
                                         int accumulate) {
  __shared__ double red[32][9];
  const int nout = Cout * (C + 1);
  const int ol = threadIdx.x & 7, sg = threadIdx.x >> 3;
  const int i = blockIdx.x * 8 + ol;
  double s = 0.0;
  if (i < nout) {
    double s1 = 0.0;
    int b = sg;
    for (; b + 32 < nblk; b += 64) { s += (double)part[(long)b * nout + i]; s1 += (double)part[(long)(b + 32) * nout + i]; }
    for (; b < nblk; b += 32) s += (double)part[(long)b * nout + i];
    s += s1;
  }
  red[sg][ol] = s;
  __syncthreads();
  if (sg == 0 && i < nout) {
    for (int j = 1; j < 32; ++j) s += red[j][ol];
    const int o = i / (C + 1), c = i - o * (C + 1);
    if (c == C && !db) return;
    float* dst = (c < C) ? dw + o * C + c : db + o;
    *dst = accumulate ? *dst + (float)s : (float)s;
  }
}

// ---------------------------------------------------------------------------------------------
// head + loss fused (training step): one pass over the last activation computes
//   v = W a + b,  loss += (v-u)^2,  dv = coef (v-u),  da = W^T dv,  dW += dv a^T,  db += dv
// i.e. FlowMatchingDecoder.outc (task_decoders.py:132) + mean((vt-ut)**2) (conditional_flow_matching.py:72)
// + their backward, reading the 64-channel activation once instead of three times.
// part[gridDim.x][Cout][C+1] (dW | db), lpart[gridDim.x] (double, sum of squares).
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head_loss_fused_kernel(const T* __restrict__ x, int ldx,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ u, float* __restrict__ v_out,
                                                              T* __restrict__ dx, int lddx, float coef,
                                                              float* __restrict__ part, double* __restrict__ lpart,
                                                              long npix, int HW, int C, int Cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);                 // [Cout][C]
  float* gl = wl + HEAD_MAX_COUT * C;                          // [256][HEAD_MAX_COUT] dv
  bf16_t* al = reinterpret_cast<bf16_t*>(gl + 256 * HEAD_MAX_COUT);   // [256][C+8] activation tile (bf16 is enough for dW)
  __shared__ double lred[256];
  const int AS = C + 8;
  for (int i = threadIdx.x; i < Cout * C; i += 256) wl[i] = w[i];
  const int nout = Cout * (C + 1);
  float acc[4];                                                // outputs tid, tid+256, ... (nout <= 1024)
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = 0.f;
  double lsum = 0.0;
  __syncthreads();
  for (long p0 = (long)blockIdx.x * 256; p0 < npix; p0 += (long)gridDim.x * 256) {
    const long p = p0 + threadIdx.x;
    const bool ok = p < npix;
    float g[HEAD_MAX_COUT];
#pragma unroll
    for (int o = 0; o < HEAD_MAX_COUT; ++o) g[o] = 0.f;
    if (ok) {
      float vv[HEAD_MAX_COUT];
#pragma unroll
      for (int o = 0; o < HEAD_MAX_COUT; ++o) vv[o] = 0.f;
      for (int c8 = 0; c8 < C; c8 += 8) {
        const f32x8 a = load8(x + p * ldx + c8);
        bf16x8 ab;
#pragma unroll
        for (int k = 0; k < 8; ++k) ab[k] = (bf16_t)a.v[k];
        *reinterpret_cast<bf16x8*>(al + threadIdx.x * AS + c8) = ab;
#pragma unroll
        for (int o = 0; o < HEAD_MAX_COUT; ++o)
          if (o < Cout)
#pragma unroll
            for (int k = 0; k < 8; ++k) vv[o] = fmaf(a.v[k], wl[o * C + c8 + k], vv[o]);
      }
      const long n = p / HW, q = p - n * HW;
#pragma unroll
      for (int o = 0; o < HEAD_MAX_COUT; ++o)
        if (o < Cout) {
          const float vo = vv[o] + (bias ? bias[o] : 0.f);
          const long idx = (n * Cout + o) * HW + q;
          if (v_out) v_out[idx] = vo;
          const float d = vo - u[idx];
          lsum += (double)(d * d);
          g[o] = coef * d;
        }
      for (int c8 = 0; c8 < C; c8 += 8) {
        f32x8 da;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float s = 0.f;
#pragma unroll
          for (int o = 0; o < HEAD_MAX_COUT; ++o)
            if (o < Cout) s = fmaf(g[o], wl[o * C + c8 + k], s);
          da.v[k] = s;
        }
        store8(dx + p * lddx + c8, da);
      }
    } else {
      for (int c8 = 0; c8 < C; c8 += 8) {
        bf16x8 z;
#pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = (bf16_t)0.f;
        *reinterpret_cast<bf16x8*>(al + threadIdx.x * AS + c8) = z;
      }
    }
#pragma unroll
    for (int o = 0; o < HEAD_MAX_COUT; ++o) gl[threadIdx.x * HEAD_MAX_COUT + o] = g[o];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = threadIdx.x + i * 256;
      if (id < nout) {
        const int o = id / (C + 1), c = id - o * (C + 1);
        float a = acc[i];
        if (c < C) for (int pp = 0; pp < 256; ++pp) a = fmaf(gl[pp * HEAD_MAX_COUT + o], (float)al[pp * AS + c], a);
        else for (int pp = 0; pp < 256; ++pp) a += gl[pp * HEAD_MAX_COUT + o];
        acc[i] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + i * 256;
    if (id < nout) part[(long)blockIdx.x * nout + id] = acc[i];
  }
  lred[threadIdx.x] = lsum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) lred[threadIdx.x] += lred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) lpart[blockIdx.x] = lred[0];
}

// Lane-per-piece form of the fused head (C = 8*PCB, PCB a power of two <= 64): the PCB lanes of a pixel each
// own 8 of its channels, so a wave reads and writes whole NHWC pixel rows (the one-thread-per-pixel form above
// issues 64 different cache lines per load instruction and needs an LDS transpose for dW).  v = W a is finished by
// a butterfly over the PCB lanes; dW and db accumulate in registers over the workgroup's pixels and are folded
// once at the end.  Same outputs and workspace as head_loss_fused_kernel.
template <typename T, int PCB>
__global__ __launch_bounds__(256) void head_loss_lanes_kernel(const T* __restrict__ x, int ldx,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ u, float* __restrict__ v_out,
                                                              T* __restrict__ dx, int lddx, float coef,
                                                              float* __restrict__ part, double* __restrict__ lpart,
                                                              long npix, int HW, int Cout) {
  constexpr int C = PCB * 8, PPB = 256 / PCB, MO = HEAD_MAX_COUT;      // (loops over 3 instead of 4 outputs: no faster)
  __shared__ float fold[256][MO * 8 + 1];
  __shared__ float dbf[PPB][MO];
  __shared__ double lred[256];
  const int tid = threadIdx.x, pc = tid & (PCB - 1), slot = tid / PCB;
  const int lane = tid & 63, grp0 = lane & ~(PCB - 1);
  float wr[MO][8], bo[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    bo[o] = (o < Cout && bias) ? bias[o] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) wr[o][k] = o < Cout ? w[o * C + pc * 8 + k] : 0.f;
  }
  float dwacc[MO][8], dbacc[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    dbacc[o] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) dwacc[o][k] = 0.f;
  }
  double lsum = 0.0;
  // the next pixel's piece is fetched before this one is processed (one load in flight per thread left the loop
  // latency-bound: 2.4 TB/s); pixel indices fit 32 bits (checked on the host), so n = p / HW is a 32-bit division
  const int np = (int)npix, stride = (int)gridDim.x * PPB;
  f32x8 a_next;
  {
    const int pf = (int)blockIdx.x * PPB + slot;
#pragma unroll
    for (int k = 0; k < 8; ++k) a_next.v[k] = 0.f;
    if (pf < np) a_next = load8(x + (long)pf * ldx + pc * 8);
  }
  for (int p0 = (int)blockIdx.x * PPB; p0 < np; p0 += stride) {
    const int p = p0 + slot;
    const bool ok = p < np;
    const f32x8 a = a_next;
    {
      const int pn = p + stride;
#pragma unroll
      for (int k = 0; k < 8; ++k) a_next.v[k] = 0.f;
      if (p0 + stride < np && pn < np) a_next = load8(x + (long)pn * ldx + pc * 8);
    }
    float vv[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t = fmaf(a.v[k], wr[o][k], t);
#pragma unroll
      for (int m = 1; m < PCB; m <<= 1) t += __shfl_xor(t, m, 64);
      vv[o] = t + bo[o];
    }
    const int n = p / HW, q = p - n * HW;
    float gm[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      gm[o] = 0.f;
      if (ok && o < Cout && (o & (PCB - 1)) == pc) {        // this lane owns output channel o of the pixel
        const long idx = ((long)n * Cout + o) * HW + q;
        if (v_out) v_out[idx] = vv[o];
        const float d = vv[o] - u[idx];
        lsum += (double)(d * d);
        gm[o] = coef * d;
      }
    }
    float g[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) g[o] = __shfl(gm[o], grp0 + (o & (PCB - 1)), 64);
    if (ok) {
      f32x8 da;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        float t = 0.f;
#pragma unroll
        for (int o = 0; o < MO; ++o) t = fmaf(g[o], wr[o][k], t);
        da.v[k] = t;
      }
      store8(dx + (long)p * lddx + pc * 8, da);
    }
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      if (pc == 0) dbacc[o] += g[o];
#pragma unroll
      for (int k = 0; k < 8; ++k) dwacc[o][k] = fmaf(g[o], a.v[k], dwacc[o][k]);
    }
  }
#pragma unroll
  for (int o = 0; o < MO; ++o) {
#pragma unroll
    for (int k = 0; k < 8; ++k) fold[tid][o * 8 + k] = dwacc[o][k];
    if (pc == 0) dbf[slot][o] = dbacc[o];
  }
  lred[tid] = lsum;
  __syncthreads();
  const int nout = Cout * (C + 1);
  for (int id = tid; id < nout; id += 256) {
    const int o = id / (C + 1), c = id - o * (C + 1);
    float t = 0.f;
    if (c < C) {
      const int cp = c >> 3, k = c & 7;
      for (int sl = 0; sl < PPB; ++sl) t += fold[sl * PCB + cp][o * 8 + k];
    } else {
      for (int sl = 0; sl < PPB; ++sl) t += dbf[sl][o];
    }
    part[(long)blockIdx.x * nout + id] = t;
  }
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) lred[tid] += lred[tid + o];
    __syncthreads();
  }
  if (tid == 0) lpart[blockIdx.x] = lred[0];
}

// The same lane-per-piece layout for the module path, where the loss lives outside (autograd drives the head alone):
// FWD = v = W a + b only; otherwise the backward from an incoming dY (NCHW fp32): da = W^T dy, dW += dy a^T, db += dy.
// (The one-thread-per-pixel kernels above read 64 different cache lines per load instruction: 122 / 100 / 348 us for the
// forward / data gradient / weight gradient of the 64 -> 3 head at 16 x 256 x 256, against ~35 us of HBM time each.)
template <typename T, int PCB, bool FWD>
__global__ __launch_bounds__(256) void head_lanes_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const float* __restrict__ dy,
                                                         float* __restrict__ v_out, T* __restrict__ dx, int lddx,
                                                         float* __restrict__ part, long npix, int HW, int Cout) {
  constexpr int C = PCB * 8, PPB = 256 / PCB, MO = HEAD_MAX_COUT;
  __shared__ float fold[FWD ? 1 : 256][MO * 8 + 1];
  __shared__ float dbf[PPB][MO];
  const int tid = threadIdx.x, pc = tid & (PCB - 1), slot = tid / PCB;
  const int lane = tid & 63, grp0 = lane & ~(PCB - 1);
  float wr[MO][8], bo[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    bo[o] = (o < Cout && bias) ? bias[o] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) wr[o][k] = o < Cout ? w[o * C + pc * 8 + k] : 0.f;
  }
  float dwacc[MO][8], dbacc[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    dbacc[o] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) dwacc[o][k] = 0.f;
  }
  const int np = (int)npix, stride = (int)gridDim.x * PPB;
  f32x8 a_next;
  {
    const int pf = (int)blockIdx.x * PPB + slot;
#pragma unroll
    for (int k = 0; k < 8; ++k) a_next.v[k] = 0.f;
    if (pf < np) a_next = load8(x + (long)pf * ldx + pc * 8);
  }
  for (int p0 = (int)blockIdx.x * PPB; p0 < np; p0 += stride) {
    const int p = p0 + slot;
    const bool ok = p < np;
    const f32x8 a = a_next;
    {
      const int pn = p + stride;
#pragma unroll
      for (int k = 0; k < 8; ++k) a_next.v[k] = 0.f;
      if (p0 + stride < np && pn < np) a_next = load8(x + (long)pn * ldx + pc * 8);
    }
    const int n = p / HW, q = p - n * HW;
    if (FWD) {
#pragma unroll
      for (int o = 0; o < MO; ++o) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t = fmaf(a.v[k], wr[o][k], t);
#pragma unroll
        for (int m = 1; m < PCB; m <<= 1) t += __shfl_xor(t, m, 64);
        if (ok && o < Cout && (o & (PCB - 1)) == pc) v_out[((long)n * Cout + o) * HW + q] = t + bo[o];
      }
    } else {
      float gm[MO], g[MO];
#pragma unroll
      for (int o = 0; o < MO; ++o) {
        gm[o] = 0.f;
        if (ok && o < Cout && (o & (PCB - 1)) == pc) gm[o] = dy[((long)n * Cout + o) * HW + q];
      }
#pragma unroll
      for (int o = 0; o < MO; ++o) g[o] = __shfl(gm[o], grp0 + (o & (PCB - 1)), 64);
      if (ok) {
        f32x8 da;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float t = 0.f;
#pragma unroll
          for (int o = 0; o < MO; ++o) t = fmaf(g[o], wr[o][k], t);
          da.v[k] = t;
        }
        store8(dx + (long)p * lddx + pc * 8, da);
      }
#pragma unroll
      for (int o = 0; o < MO; ++o) {
        if (pc == 0) dbacc[o] += g[o];
#pragma unroll
        for (int k = 0; k < 8; ++k) dwacc[o][k] = fmaf(g[o], a.v[k], dwacc[o][k]);
      }
    }
  }
  if (FWD) return;
#pragma unroll
  for (int o = 0; o < MO; ++o) {
#pragma unroll
    for (int k = 0; k < 8; ++k) fold[tid][o * 8 + k] = dwacc[o][k];
    if (pc == 0) dbf[slot][o] = dbacc[o];
  }
  __syncthreads();
  const int nout = Cout * (C + 1);
  for (int id = tid; id < nout; id += 256) {
    const int o = id / (C + 1), c = id - o * (C + 1);
    float t = 0.f;
    if (c < C) {
      const int cp = c >> 3, k = c & 7;
      for (int sl = 0; sl < PPB; ++sl) t += fold[sl * PCB + cp][o * 8 + k];
    } else {
      for (int sl = 0; sl < PPB; ++sl) t += dbf[sl][o];
    }
    part[(long)blockIdx.x * nout + id] = t;
  }
}

// Which kernels a head launch takes (s2s_head_family): the lane-per-piece form returns its PCB (C = 8 PCB, PCB a power of
// two <= 64, Cout <= 4), the one-thread-per-pixel kernels HEAD_FALLBACK + MO (MO = 4 or 8 outputs unrolled); a negative
// status is a launch the entry points refuse.  s2s_head_conv1x1_fwd / _bwd dispatch on this value and on nothing else.
constexpr int HEAD_FALLBACK = 100;
int head_family(int dtype, int B, int H, int W, int C, int Cout, int forward) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) || Cout <= 0 || Cout > HEAD_WIDE_COUT) return S2S_ERR_SHAPE;
  if (!forward && Cout * (C + 1) > 2048) return S2S_ERR_SHAPE;     // head_wgrad_kernel: 8 outputs a thread
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  const long npix = (long)B * H * W;
  const int pcb = C / 8;
  if (Cout <= HEAD_MAX_COUT && npix < (1L << 31) - (1L << 20) && pcb <= 64 && !(pcb & (pcb - 1))) return pcb;
  return HEAD_FALLBACK + (Cout <= 4 ? 4 : 8);
}

// Which kernel s2s_head_loss_fused launches (s2s_head_loss_family): the lane-per-piece kernel returns its PCB (C = 8 PCB,
// PCB a power of two <= 64; static shared memory, a loop over its Cout (C + 1) partial sums), every other C % 8 == 0 the
// one-thread-per-pixel kernel, HEAD_LOSS_PIXEL, whose limits are its own: a dynamic LDS tile of at most 60 KB (C <= 96)
// and four partial sums a thread.  A negative status is a launch the entry point refuses; it dispatches on this value.
constexpr int HEAD_LOSS_PIXEL = 100;
inline int head_loss_pixel_lds(int C) { return (HEAD_MAX_COUT * C + 256 * HEAD_MAX_COUT) * 4 + 256 * (C + 8) * 2; }
int head_loss_family(int dtype, int B, int H, int W, int C, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) || Cout <= 0 || Cout > HEAD_MAX_COUT) return S2S_ERR_SHAPE;
  if ((long)B * H * W >= (1L << 31) - (1L << 20)) return S2S_ERR_SHAPE;   // 32-bit pixel index (+ one grid stride) in the kernels
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  const int pcb = C / 8;
  if (pcb <= 64 && !(pcb & (pcb - 1))) return pcb;
  if (Cout * (C + 1) > 1024 || head_loss_pixel_lds(C) > 60 * 1024) return S2S_ERR_SHAPE;
  return HEAD_LOSS_PIXEL;
}

// launch head_lanes_kernel<T, PP, FWD> for the PP head_family chose
template <typename T, bool FWD>
void launch_head_lanes(int pp, const void* x, int ldx, const float* w, const float* bias, const float* dy, float* v, void* dx,
                       int lddx, float* part, int nb, long npix, int HW, int Cout, hipStream_t s) {
#define S2S_HLN(PP)                                                                                                  \
  hipLaunchKernelGGL((head_lanes_kernel<T, PP, FWD>), dim3(nb), dim3(256), 0, s, (const T*)x, ldx, w, bias, dy, v,   \
                     (T*)dx, lddx, part, npix, HW, Cout);                                                            \
  break;
  switch (pp) {
    case 1: S2S_HLN(1) case 2: S2S_HLN(2) case 4: S2S_HLN(4) case 8: S2S_HLN(8) case 16: S2S_HLN(16) case 32: S2S_HLN(32)
    case 64: S2S_HLN(64)
  }
#undef S2S_HLN
}

// ---------------------------------------------------------------------------------------------
// fused tail of the training step: last BatchNorm + ReLU -> head -> MSE loss -> head backward -> BatchNorm backward.
// The last activation has one reader (the head) and its gradient one reader (the BatchNorm backward), and the whole
// chain is local to a pixel, so neither tensor is stored: three passes that read the saved conv output (and write
// 12.6 + 134 MB) instead of four passes over three 64-channel tensors.
//   pass A (tail_fwd_loss_kernel): a = relu(scale raw + shift) rounded to T, v = W a + b, g = coef (v - u), partial
//     sums of the loss and of dW | db; writes only g (and v when asked), both NCHW fp32.
//   sums (norm_act.hip, bn_relu_bwd_reduce_tail_kernel): da = W^T g rounded to T, sum dz and sum dz xhat, dz = da (a > 0),
//     then bn_bwd_finalize.
//   pass B (tail_bwd_apply_kernel): recomputes da from g and writes d raw = gamma invstd (dz - c1 - xhat c2).
// Every value is rounded where the stored tensors of the unfused chain (bn_relu_apply -> head_loss_lanes_kernel ->
// bn_relu_bwd_*_flat_kernel) rounded it, with their expressions, and every sum is taken in that chain's order: pass A
// has head_loss_lanes_kernel's grid and pixel-to-lane map, the sums pass bn_relu_bwd_reduce_flat_kernel's (the two
// differ, which is why the BatchNorm sums are not taken in pass A).  The results are the chain's, bit for bit.
// Same lane-per-piece layout as head_loss_lanes_kernel (C = 8 PCB).
// ---------------------------------------------------------------------------------------------
// Sum over the PCB lanes that share a pixel, every lane getting the total: the butterfly of head_loss_lanes_kernel
// (t += t[lane ^ m], m = 1, 2, 4, ...) with DPP moves in place of LDS permutes for m <= 8.  After the two quad steps
// the four lanes of a quad agree, so the mirrored lane of the other quad (or half row) holds what lane ^ 4 (lane ^ 8)
// holds: the same additions, bit for bit.  Needs every lane of the wave active.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int PCB>
__device__ __forceinline__ float group_sum(float t) {
  if (PCB >= 2) t += dpp_f32<0xB1>(t);        // quad_perm [1,0,3,2]
  if (PCB >= 4) t += dpp_f32<0x4E>(t);        // quad_perm [2,3,0,1]
  if (PCB >= 8) t += dpp_f32<0x141>(t);       // row_half_mirror
  if (PCB >= 16) t += dpp_f32<0x140>(t);      // row_mirror
#pragma unroll
  for (int m = 16; m < PCB; m <<= 1) t += __shfl_xor(t, m, 64);
  return t;
}

// a pixel piece as loaded (bf16 stays packed while the load is in flight: 4 VGPRs a stage instead of 8)
__device__ __forceinline__ bf16x8 tail_ld(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ f32x8 tail_ld(const float* p) { return load8(p); }
__device__ __forceinline__ float tail_at(const bf16x8& v, int k) { return (float)v[k]; }
__device__ __forceinline__ float tail_at(const f32x8& v, int k) { return v.v[k]; }

template <typename T, int PCB, int MO>
__global__ __launch_bounds__(256) void tail_fwd_loss_kernel(const T* __restrict__ raw, int ldx,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            const float* __restrict__ u, float* __restrict__ v_out,
                                                            float* __restrict__ g_out, float coef,
                                                            float* __restrict__ part, double* __restrict__ lpart,
                                                            long npix, int HW, int Cout) {
  constexpr int C = PCB * 8, PPB = 256 / PCB;     // MO: outputs the loops cover (3 for the flow head: 16 fewer VGPRs)
  __shared__ float fold[256][MO * 8 + 1];
  __shared__ float dbf[PPB][MO];
  __shared__ double lred[256];
  const int tid = threadIdx.x, pc = tid & (PCB - 1), slot = tid / PCB;
  float wr[MO][8], bo[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    bo[o] = (o < Cout && bias) ? bias[o] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) wr[o][k] = o < Cout ? w[o * C + pc * 8 + k] : 0.f;
  }
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { sc[k] = scale[pc * 8 + k]; sh[k] = shift[pc * 8 + k]; }
  float dwacc[MO][8], dbacc[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) {
    dbacc[o] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) dwacc[o][k] = 0.f;
  }
  double lsum = 0.0;
  const int np = (int)npix, stride = (int)gridDim.x * PPB;     // 32-bit pixel indices (checked on the host)
  // Two pixels ahead: the piece and the targets of the next two iterations are in flight while this one is processed
  // (with one, 3 waves x 1 KB a SIMD left the pass latency-bound at 1.2 TB/s).  Every lane of a pixel reads its targets
  // (one address per pixel and output) and forms g itself: no owner-lane broadcast through LDS.
  struct Stage {
    decltype(tail_ld((const T*)nullptr)) r;
    float u[MO];
    long i;                                                       // offset of output 0 of the pixel in the NCHW tensors
  };
  auto fetch = [&](Stage& st, int pf) {       // past the end: the last pixel again (finite values; its g is forced to 0 below)
    pf = pf < np ? pf : np - 1;
    st.r = tail_ld(raw + (long)pf * ldx + pc * 8);
    const int n = pf / HW, q = pf - n * HW;
    st.i = (long)n * Cout * HW + q;
#pragma unroll
    for (int o = 0; o < MO; ++o) st.u[o] = u[st.i + (long)(o < Cout ? o : Cout - 1) * HW];   // (no branch around a load)
  };
  Stage sa, sb;
  fetch(sa, (int)blockIdx.x * PPB + slot);
  fetch(sb, (int)blockIdx.x * PPB + slot + stride);
  // one pixel: take the stage's values, refill it two pixels ahead (the two stages alternate, so no register of a load
  // in flight is copied), then the arithmetic
  auto step = [&](Stage& st, int p0) {
    const int p = p0 + slot;
    const bool ok = p < np;
    f32x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r.v[k] = tail_at(st.r, k);
    float cu[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) cu[o] = st.u[o];
    const long i0 = st.i;
    fetch(st, p + 2 * stride);
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)                                   // bn_relu_apply's expression, stored as T
      a[k] = to_f32(from_f32<T>(fmaxf(fmaf(r.v[k], sc[k], sh[k]), 0.f)));
    float vv[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) t = fmaf(a[k], wr[o][k], t);
      vv[o] = group_sum<PCB>(t) + bo[o];
    }
    float g[MO];                                                  // (a pixel past the end has g = 0: it adds nothing to any sum)
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      const float d = vv[o] - cu[o];
      g[o] = (ok && o < Cout) ? coef * d : 0.f;
      if (ok && o < Cout && (o & (PCB - 1)) == pc) {        // this lane writes output channel o of the pixel
        const long idx = i0 + (long)o * HW;
        if (v_out) v_out[idx] = vv[o];
        lsum += (double)(d * d);
        g_out[idx] = g[o];
      }
    }
#pragma unroll
    for (int o = 0; o < MO; ++o) {
      if (pc == 0) dbacc[o] += g[o];
#pragma unroll
      for (int k = 0; k < 8; ++k) dwacc[o][k] = fmaf(g[o], a[k], dwacc[o][k]);
    }
  };
  for (int p0 = (int)blockIdx.x * PPB; p0 < np; p0 += 2 * stride) {
    step(sa, p0);
    if (p0 + stride < np) step(sb, p0 + stride);                  // (workgroup-uniform)
  }
#pragma unroll
  for (int o = 0; o < MO; ++o) {
#pragma unroll
    for (int k = 0; k < 8; ++k) fold[tid][o * 8 + k] = dwacc[o][k];
    if (pc == 0) dbf[slot][o] = dbacc[o];
  }
  lred[tid] = lsum;
  __syncthreads();
  const int nout = Cout * (C + 1);
  for (int id = tid; id < nout; id += 256) {
    const int o = id / (C + 1), c = id - o * (C + 1);
    float t = 0.f;
    if (c < C) {
      const int cp = c >> 3, k = c & 7;
      for (int sl = 0; sl < PPB; ++sl) t += fold[sl * PCB + cp][o * 8 + k];
    } else {
      for (int sl = 0; sl < PPB; ++sl) t += dbf[sl][o];
    }
    part[(long)blockIdx.x * nout + id] = t;
  }
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) lred[tid] += lred[tid + o];
    __syncthreads();
  }
  if (tid == 0) lpart[blockIdx.x] = lred[0];
}

template <typename T, int PCB, int MO>
__global__ __launch_bounds__(256) void tail_bwd_apply_kernel(const T* __restrict__ raw, int ldx,
                                                             const float* __restrict__ g_nchw, const float* __restrict__ w,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ c1,
                                                             const float* __restrict__ c2, T* __restrict__ dx, int lddx,
                                                             long npix, int HW, int Cout) {
  constexpr int C = PCB * 8, PPB = 256 / PCB;     // MO: outputs the loops cover (3 for the flow head: 16 fewer VGPRs)
  const int tid = threadIdx.x, pc = tid & (PCB - 1), slot = tid / PCB;
  float wr[MO][8];
#pragma unroll
  for (int o = 0; o < MO; ++o)
#pragma unroll
    for (int k = 0; k < 8; ++k) wr[o][k] = o < Cout ? w[o * C + pc * 8 + k] : 0.f;
  float ga[8], k1[8], k2[8], mu[8], is[8], sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = pc * 8 + k;
    mu[k] = mean[c]; is[k] = invstd[c]; sc[k] = scale[c]; sh[k] = shift[c];
    ga[k] = gamma[c] * is[k]; k1[k] = c1[c]; k2[k] = c2[c];
  }
  // back to front, like the flat apply pass: pass A read the tensor front to back, so its tail is what the memory-side
  // cache still holds.  The next pixel's piece and gradient are fetched before this one is processed.
  const int np = (int)npix, stride = (int)gridDim.x * PPB;
  const int first = (int)blockIdx.x * PPB + slot;
  const int nit = first < np ? (np - first + stride - 1) / stride : 0;
  f32x8 r_next;
  float g_next[MO];
  auto fetch = [&](int p) {
    r_next = load8(raw + (long)p * ldx + pc * 8);
    const int n = p / HW, q = p - n * HW;
#pragma unroll
    for (int o = 0; o < MO; ++o) g_next[o] = o < Cout ? g_nchw[((long)n * Cout + o) * HW + q] : 0.f;
  };
  if (nit > 0) fetch(first + (nit - 1) * stride);
  for (int it = nit - 1; it >= 0; --it) {
    const int p = first + it * stride;
    const f32x8 r = r_next;
    float g[MO];
#pragma unroll
    for (int o = 0; o < MO; ++o) g[o] = g_next[o];
    if (it > 0) fetch(p - stride);
    f32x8 out;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = 0.f;
#pragma unroll
      for (int o = 0; o < MO; ++o) t = fmaf(g[o], wr[o][k], t);
      const float da = to_f32(from_f32<T>(t));
      const float dz = fmaf(r.v[k], sc[k], sh[k]) > 0.f ? da : 0.f;
      out.v[k] = ga[k] * (dz - k1[k] - ((r.v[k] - mu[k]) * is[k]) * k2[k]);
    }
    store8(dx + (long)p * lddx + pc * 8, out);
  }
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* part, int n, double inv_count, float* loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] * inv_count);
}

}  // namespace

// MFMA stem forward lives next to the shared epilogue in conv3x3_mfma.hip
int s2s_internal_stem_fwd(int dtype, const float* x_nchw, const float* w_oihw, const float* bias, void* y, int ldy,
                          float* stat_part, int B, int H, int W, int Cin, int Cout, hipStream_t s);

extern "C" int s2s_stem_stat_blocks(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return S2S_ERR_SHAPE;
  return B * cdiv(H, 16) * cdiv(W, 16);
}

extern "C" int s2s_stem_conv3x3_fwd(int dtype, const float* x_nchw, const float* w_oihw, const float* bias, void* y,
                                    int ldy, float* stat_part, int B, int H, int W, int Cin, int Cout, void* stream) {
  if (!x_nchw || !w_oihw || !y) return S2S_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin > 6 || Cout <= 0 || (Cout % 8) || (ldy % 8))
    return S2S_ERR_SHAPE;
  return s2s_internal_stem_fwd(dtype, x_nchw, w_oihw, bias, y, ldy, stat_part, B, H, W, Cin, Cout,
                               (hipStream_t)stream);
}

extern "C" int s2s_stem_wgrad_blocks(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return S2S_ERR_SHAPE;
  const int nt = B * cdiv(H, 16) * cdiv(W, 16);
  constexpr int cap = 512;   // 2 per CU: 98 us vs 126 us at 256
  return nt < cap ? nt : cap;
}

namespace {

// Which kernel a stem weight-gradient launch takes (s2s_stem_wgrad_family hands it to tests): bf16 the pipelined kernel,
// fp32 (three images per operand: 240 KB of LDS in that form) and `reference` the kernel it replaced
enum StemWgradFamily { kStemWgradReference = 0, kStemWgradPipelined = 1 };

int stem_wgrad_family(int dtype, bool reference) { return dtype == S2S_BF16 && !reference ? kStemWgradPipelined : kStemWgradReference; }

int stem_wgrad_check(int dtype, int B, int H, int W, int Cin, int Cout, int lddy) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin > 6 || Cout <= 0 || (Cout % 8) || (lddy % 8))
    return S2S_ERR_SHAPE;
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  return S2S_OK;
}

// part: float[ceil(Cin/3)][2*blocks][Cout][32]
int stem_wgrad_launch(int dtype, const void* dy, int lddy, const float* x_nchw, float* part, float* dw_oihw, float* dbias,
                      int accumulate, int B, int H, int W, int Cin, int Cout, void* stream, bool reference) {
  if (!dy || !x_nchw || !part || !dw_oihw) return S2S_ERR_NULL;
  if (int rc = stem_wgrad_check(dtype, B, H, W, Cin, Cout, lddy)) return rc;
  const int nb = s2s_stem_wgrad_blocks(B, H, W);
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(nb, cdiv(Cout, 64), cdiv(Cin, 3));
  if (stem_wgrad_family(dtype, reference) == kStemWgradPipelined) {
    if ((uintptr_t)dy & 15) return S2S_ERR_ALIGN;          // the DMA moves whole 16-byte pieces
    static unsigned long long attr_devs = 0;   // hipFuncSetAttribute is per device
    if (int rc = s2s_allow_dyn_lds(reinterpret_cast<const void*>(stem_wgrad_pipe_kernel), STEM_PIPE_LDS, &attr_devs)) return rc;
    hipLaunchKernelGGL(stem_wgrad_pipe_kernel, grid, dim3(256), STEM_PIPE_LDS, s, (const bf16_t*)dy, lddy, x_nchw, part, B,
                       H, W, Cin, Cout, cdiv(H, 16), cdiv(W, 16));
  } else if (dtype == S2S_BF16) {
    const int lds = 1 * (2 * 256 * 64 + 256 * 64) + 3 * 324 * 4;
    hipLaunchKernelGGL(stem_wgrad_kernel<bf16_t>, grid, dim3(256), lds, s, (const bf16_t*)dy, lddy, x_nchw, part, B,
                       H, W, Cin, Cout, cdiv(H, 16), cdiv(W, 16));
  } else {
    const int lds = 3 * (2 * 256 * 64 + 256 * 64) + 3 * 324 * 4;
    static unsigned long long attr_devs = 0;   // hipFuncSetAttribute is per device
    if (int rc = s2s_allow_dyn_lds(reinterpret_cast<const void*>(stem_wgrad_kernel<float>), lds, &attr_devs)) return rc;
    hipLaunchKernelGGL(stem_wgrad_kernel<float>, grid, dim3(256), lds, s, (const float*)dy, lddy, x_nchw, part, B, H,
                       W, Cin, Cout, cdiv(H, 16), cdiv(W, 16));
  }
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(Cout, cdiv(Cin, 3)), dim3(1024), 0, s, part, 2 * nb, Cout, Cin, dw_oihw, dbias,
                     accumulate);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_stem_conv3x3_wgrad(int dtype, const void* dy, int lddy, const float* x_nchw, float* part,
                                      float* dw_oihw, float* dbias, int accumulate, int B, int H, int W, int Cin,
                                      int Cout, void* stream) {
  return stem_wgrad_launch(dtype, dy, lddy, x_nchw, part, dw_oihw, dbias, accumulate, B, H, W, Cin, Cout, stream, false);
}

// test-facing: the kernel the bf16 production launch replaced, on the same arguments (fp32: the same launch)
extern "C" int s2s_stem_conv3x3_wgrad_ref(int dtype, const void* dy, int lddy, const float* x_nchw, float* part,
                                          float* dw_oihw, float* dbias, int accumulate, int B, int H, int W, int Cin,
                                          int Cout, void* stream) {
  return stem_wgrad_launch(dtype, dy, lddy, x_nchw, part, dw_oihw, dbias, accumulate, B, H, W, Cin, Cout, stream, true);
}

// test-facing, no launch: 0 = the reference kernel, 1 = the pipelined kernel, < 0 = the error the launch would return.
// reference != 0: as s2s_stem_conv3x3_wgrad_ref chooses.
extern "C" int s2s_stem_wgrad_family(int dtype, int lddy, int B, int H, int W, int Cin, int Cout, int reference) {
  if (int rc = stem_wgrad_check(dtype, B, H, W, Cin, Cout, lddy)) return rc;
  return stem_wgrad_family(dtype, reference != 0);
}

extern "C" int s2s_head_family(int dtype, int B, int H, int W, int C, int Cout, int forward) {
  return head_family(dtype, B, H, W, C, Cout, forward);
}

extern "C" int s2s_head_conv1x1_fwd(int dtype, const void* x, int ldx, const float* w, const float* bias,
                                    float* y_nchw, int B, int H, int W, int C, int Cout, void* stream) {
  if (!x || !w || !y_nchw) return S2S_ERR_NULL;
  if (ldx % 8) return S2S_ERR_SHAPE;
  const int fam = head_family(dtype, B, H, W, C, Cout, 1);
  if (fam < 0) return fam;
  const long npix = (long)B * H * W;
  long grid = (npix + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipStream_t s = (hipStream_t)stream;
  if (fam < HEAD_FALLBACK) {
    const int nbl = (int)(((npix + 255) / 256) < 2048 ? ((npix + 255) / 256) : 2048);
    if (dtype == S2S_BF16)
      launch_head_lanes<bf16_t, true>(fam, x, ldx, w, bias, nullptr, y_nchw, nullptr, 8, nullptr, nbl, npix, H * W, Cout, s);
    else
      launch_head_lanes<float, true>(fam, x, ldx, w, bias, nullptr, y_nchw, nullptr, 8, nullptr, nbl, npix, H * W, Cout, s);
    S2S_LAUNCH_CHECK();
    return S2S_OK;
  }
  const int mo = fam - HEAD_FALLBACK;
#define S2S_HEAD_FWD(TT, MO)                                                                                        \
  hipLaunchKernelGGL((head_fwd_kernel<TT, MO>), dim3((int)grid), dim3(256), Cout * C * 4, s, (const TT*)x, ldx, w, \
                     bias, y_nchw, npix, H * W, C, Cout)
  if (dtype == S2S_BF16) { if (mo == 4) S2S_HEAD_FWD(bf16_t, 4); else S2S_HEAD_FWD(bf16_t, 8); }
  else { if (mo == 4) S2S_HEAD_FWD(float, 4); else S2S_HEAD_FWD(float, 8); }
#undef S2S_HEAD_FWD
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_head_wgrad_blocks(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return S2S_ERR_SHAPE;
  const long nb = ((long)B * H * W + 63) / 64;
  return (int)(nb < 512 ? nb : 512);
}

// part: float[blocks][Cout][C+1]
extern "C" int s2s_head_conv1x1_bwd(int dtype, const float* dy_nchw, const void* x, int ldx, const float* w, void* dx,
                                    int lddx, float* part, float* dw, float* dbias, int accumulate, int B, int H, int W,
                                    int C, int Cout, void* stream) {
  if (!dy_nchw || !x || !w || !dx || !part || !dw) return S2S_ERR_NULL;
  if ((ldx % 8) || (lddx % 8)) return S2S_ERR_SHAPE;
  const int fam = head_family(dtype, B, H, W, C, Cout, 0);
  if (fam < 0) return fam;
  const long npix = (long)B * H * W;
  long grid = (npix + 255) / 256;
  if (grid > 4096) grid = 4096;
  const int nb = s2s_head_wgrad_blocks(B, H, W);
  hipStream_t s = (hipStream_t)stream;
  if (fam < HEAD_FALLBACK) {
    // one pass over the activation for both gradients (lane-per-piece form, partial dW | db rows per workgroup)
    if (dtype == S2S_BF16)
      launch_head_lanes<bf16_t, false>(fam, x, ldx, w, nullptr, dy_nchw, nullptr, dx, lddx, part, nb, npix, H * W, Cout, s);
    else
      launch_head_lanes<float, false>(fam, x, ldx, w, nullptr, dy_nchw, nullptr, dx, lddx, part, nb, npix, H * W, Cout, s);
  } else {
    const int mo = fam - HEAD_FALLBACK;
    const int lds = (64 * (C + 1) + 64 * mo) * 4;
#define S2S_HEAD_BWD(TT, MO)                                                                                       \
  hipLaunchKernelGGL((head_bwd_data_kernel<TT, MO>), dim3((int)grid), dim3(256), Cout * C * 4, s, dy_nchw, w,      \
                     (TT*)dx, lddx, npix, H * W, C, Cout);                                                         \
  hipLaunchKernelGGL((head_wgrad_kernel<TT, MO>), dim3(nb), dim3(256), lds, s, dy_nchw, (const TT*)x, ldx, part,   \
                     npix, H * W, C, Cout);
    if (dtype == S2S_BF16) { if (mo == 4) { S2S_HEAD_BWD(bf16_t, 4) } else { S2S_HEAD_BWD(bf16_t, 8) } }
    else { if (mo == 4) { S2S_HEAD_BWD(float, 4) } else { S2S_HEAD_BWD(float, 8) } }
#undef S2S_HEAD_BWD
  }
  hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3(cdiv(Cout * (C + 1), 8)), dim3(256), 0, s, part, nb, Cout, C,
                     dw, dbias, accumulate);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_head_loss_blocks(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return S2S_ERR_SHAPE;
  const long nb = ((long)B * H * W + 255) / 256;
  return (int)(nb < 1024 ? nb : 1024);
}

extern "C" int s2s_head_loss_family(int dtype, int B, int H, int W, int C, int Cout) {
  return head_loss_family(dtype, B, H, W, C, Cout);
}

// part: float[blocks][Cout][C+1]; lpart: double[blocks]; v_out (optional) NCHW fp32; dv scale = 2*grad_scale/count
extern "C" int s2s_head_loss_fused(int dtype, const void* x, int ldx, const float* w, const float* bias,
                                   const float* u_nchw, float* v_nchw, void* dx, int lddx, float grad_scale,
                                   float* part, double* lpart, float* dw, float* dbias, float* loss, int accumulate,
                                   int B, int H, int W, int C, int Cout, void* stream) {
  if (!x || !w || !u_nchw || !dx || !part || !lpart || !dw || !loss) return S2S_ERR_NULL;
  if ((ldx % 8) || (lddx % 8)) return S2S_ERR_SHAPE;
  const int fam = head_loss_family(dtype, B, H, W, C, Cout);
  if (fam < 0) return fam;
  const long npix = (long)B * H * W;
  const double count = (double)npix * Cout;
  const int nb = s2s_head_loss_blocks(B, H, W);
  hipStream_t s = (hipStream_t)stream;
  const float coef = (float)(2.0 * (double)grad_scale / count);
#define S2S_HL(TT, PP)                                                                                              \
  hipLaunchKernelGGL((head_loss_lanes_kernel<TT, PP>), dim3(nb), dim3(256), 0, s, (const TT*)x, ldx, w, bias, u_nchw, \
                     v_nchw, (TT*)dx, lddx, coef, part, lpart, npix, H * W, Cout);
#define S2S_HL_T(TT)                                                                                    \
  switch (fam) {                                                                                        \
    case 1: { S2S_HL(TT, 1) } break;  case 2: { S2S_HL(TT, 2) } break;  case 4: { S2S_HL(TT, 4) } break;    \
    case 8: { S2S_HL(TT, 8) } break;  case 16: { S2S_HL(TT, 16) } break; case 32: { S2S_HL(TT, 32) } break;  \
    case 64: { S2S_HL(TT, 64) } break; default: break;                                                  \
  }
  if (dtype == S2S_BF16) { S2S_HL_T(bf16_t) } else { S2S_HL_T(float) }
#undef S2S_HL_T
#undef S2S_HL
  if (fam == HEAD_LOSS_PIXEL) {
    const int lds = head_loss_pixel_lds(C);
    if (dtype == S2S_BF16)
      hipLaunchKernelGGL(head_loss_fused_kernel<bf16_t>, dim3(nb), dim3(256), lds, s, (const bf16_t*)x, ldx, w, bias,
                         u_nchw, v_nchw, (bf16_t*)dx, lddx, coef, part, lpart, npix, H * W, C, Cout);
    else
      hipLaunchKernelGGL(head_loss_fused_kernel<float>, dim3(nb), dim3(256), lds, s, (const float*)x, ldx, w, bias,
                         u_nchw, v_nchw, (float*)dx, lddx, coef, part, lpart, npix, H * W, C, Cout);
  }
  hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3(cdiv(Cout * (C + 1), 8)), dim3(256), 0, s, part, nb, Cout, C,
                     dw, dbias, accumulate);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, lpart, nb, 1.0 / count, loss);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// the BatchNorm backward sums of the tail (reduction pass from g + per-channel finalize) live in norm_act.hip
int s2s_internal_tail_bn_sums(int dtype, const void* raw, int ldx, const float* g_nchw, const float* w, const float* scale,
                              const float* shift, const float* mean, const float* invstd, float* work, float* dgamma,
                              float* dbeta, float* zero_out, int accumulate, int B, int H, int W, int C, int Cout,
                              hipStream_t s);
extern "C" int s2s_bn_bwd_blocks(int B, int H, int W, int C);

namespace {
// Which instantiation a fused-tail launch takes (s2s_tail_family): 256 MO + PCB, PCB = C / 8 lanes per pixel (a power of
// two <= 64) and MO = 3 or 4 outputs covered by the kernels' loops; a negative status is a launch the entry points
// refuse.  s2s_tail_fwd_loss and s2s_tail_bwd_apply dispatch on this value.
int tail_family(int dtype, int B, int H, int W, int C, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || C < 8 || (C % 8) || Cout <= 0 || Cout > HEAD_MAX_COUT) return S2S_ERR_SHAPE;
  const int pcb = C / 8;
  if (pcb > 64 || (pcb & (pcb - 1))) return S2S_ERR_SHAPE;
  if ((long)B * H * W >= (1L << 31) - (1L << 20)) return S2S_ERR_SHAPE;   // 32-bit pixel index (+ one grid stride) in the kernels
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  return 256 * (Cout <= 3 ? 3 : HEAD_MAX_COUT) + pcb;
}
}  // namespace

extern "C" int s2s_tail_family(int dtype, int B, int H, int W, int C, int Cout) {
  return tail_family(dtype, B, H, W, C, Cout);
}

// workgroups of passes A and B = rows of pass A's partial buffers
extern "C" int s2s_tail_blocks(int B, int H, int W) { return s2s_head_loss_blocks(B, H, W); }

// Pass A of the fused tail (see tail_fwd_loss_kernel) + the folds of its partial sums (head dW | db, the loss), then the
// BatchNorm backward's sums from g and their per-channel finalize (dgamma, dbeta, the two means pass B reads; conv_dbias,
// the gradient of a bias in front of a train-mode BatchNorm, is exactly zero as in s2s_bn_relu_bwd).
//   part: float[blocks][Cout][C+1]; lpart: double[blocks], blocks = s2s_tail_blocks;
//   bnwork: float[2*C*nb + 2*C] (sums | c1 | c2), nb = s2s_bn_bwd_blocks; g_nchw: [B][Cout][H][W] fp32 out; v_nchw: optional
extern "C" int s2s_tail_fwd_loss(int dtype, const void* raw, int ldx, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, const float* w, const float* bias,
                                 const float* u_nchw, float* v_nchw, float* g_nchw, float grad_scale, float* part,
                                 double* lpart, float* bnwork, float* dw, float* dbias, float* loss, float* dgamma,
                                 float* dbeta, float* conv_dbias, int accumulate, int B, int H, int W, int C, int Cout,
                                 void* stream) {
  if (!raw || !scale || !shift || !mean || !invstd || !w || !u_nchw || !g_nchw || !part || !lpart || !bnwork || !dw ||
      !loss || !dgamma || !dbeta)
    return S2S_ERR_NULL;
  if (ldx % 8) return S2S_ERR_SHAPE;
  const int fam = tail_family(dtype, B, H, W, C, Cout);
  if (fam < 0) return fam;
  const long npix = (long)B * H * W;
  const double count = (double)npix * Cout;
  const int nb = s2s_tail_blocks(B, H, W);
  hipStream_t s = (hipStream_t)stream;
  const float coef = (float)(2.0 * (double)grad_scale / count);
#define S2S_TA(TT, PP)                                                                                               \
  if (fam >> 8 == 3)                                                                                                 \
    hipLaunchKernelGGL((tail_fwd_loss_kernel<TT, PP, 3>), dim3(nb), dim3(256), 0, s, (const TT*)raw, ldx, scale,     \
                       shift, w, bias, u_nchw, v_nchw, g_nchw, coef, part, lpart, npix, H * W, Cout);                \
  else                                                                                                               \
  hipLaunchKernelGGL((tail_fwd_loss_kernel<TT, PP, HEAD_MAX_COUT>), dim3(nb), dim3(256), 0, s, (const TT*)raw, ldx, scale, shift,   \
                     w, bias, u_nchw, v_nchw, g_nchw, coef, part, lpart, npix, H * W, Cout);
#define S2S_TA_T(TT)                                                                                    \
  switch (fam & 255) {                                                                                  \
    case 1: { S2S_TA(TT, 1) } break;  case 2: { S2S_TA(TT, 2) } break;  case 4: { S2S_TA(TT, 4) } break;    \
    case 8: { S2S_TA(TT, 8) } break;  case 16: { S2S_TA(TT, 16) } break; case 32: { S2S_TA(TT, 32) } break;  \
    default: { S2S_TA(TT, 64) } break;                                                                  \
  }
  if (dtype == S2S_BF16) { S2S_TA_T(bf16_t) } else { S2S_TA_T(float) }
#undef S2S_TA_T
#undef S2S_TA
  hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3(cdiv(Cout * (C + 1), 8)), dim3(256), 0, s, part, nb, Cout, C,
                     dw, dbias, accumulate);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, lpart, nb, 1.0 / count, loss);
  if (int rc = s2s_internal_tail_bn_sums(dtype, raw, ldx, g_nchw, w, scale, shift, mean, invstd, bnwork, dgamma, dbeta,
                                         (conv_dbias && !accumulate) ? conv_dbias : nullptr, accumulate, B, H, W, C,
                                         Cout, s))
    return rc;
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// Pass B of the fused tail: d raw from the saved conv output, g and the means s2s_tail_fwd_loss left in bnwork.
extern "C" int s2s_tail_bwd_apply(int dtype, const void* raw, int ldx, const float* g_nchw, const float* w,
                                  const float* scale, const float* shift, const float* mean, const float* invstd,
                                  const float* gamma, const float* bnwork, void* dx, int lddx, int B, int H, int W,
                                  int C, int Cout, void* stream) {
  if (!raw || !g_nchw || !w || !scale || !shift || !mean || !invstd || !gamma || !bnwork || !dx) return S2S_ERR_NULL;
  if ((ldx % 8) || (lddx % 8) || lddx < C) return S2S_ERR_SHAPE;
  const int fam = tail_family(dtype, B, H, W, C, Cout);
  if (fam < 0) return fam;
  const long npix = (long)B * H * W;
  const int nb = s2s_tail_blocks(B, H, W);
  const float* const c1 = bnwork + (long)2 * C * s2s_bn_bwd_blocks(B, H, W, C);
  hipStream_t s = (hipStream_t)stream;
#define S2S_TB(TT, PP)                                                                                              \
  if (fam >> 8 == 3)                                                                                                \
    hipLaunchKernelGGL((tail_bwd_apply_kernel<TT, PP, 3>), dim3(nb), dim3(256), 0, s, (const TT*)raw, ldx, g_nchw,  \
                       w, scale, shift, mean, invstd, gamma, c1, c1 + C, (TT*)dx, lddx, npix, H * W, Cout);         \
  else                                                                                                              \
  hipLaunchKernelGGL((tail_bwd_apply_kernel<TT, PP, HEAD_MAX_COUT>), dim3(nb), dim3(256), 0, s, (const TT*)raw, ldx, g_nchw, w,    \
                     scale, shift, mean, invstd, gamma, c1, c1 + C, (TT*)dx, lddx, npix, H * W, Cout);
#define S2S_TB_T(TT)                                                                                    \
  switch (fam & 255) {                                                                                  \
    case 1: { S2S_TB(TT, 1) } break;  case 2: { S2S_TB(TT, 2) } break;  case 4: { S2S_TB(TT, 4) } break;    \
    case 8: { S2S_TB(TT, 8) } break;  case 16: { S2S_TB(TT, 16) } break; case 32: { S2S_TB(TT, 32) } break;  \
    default: { S2S_TB(TT, 64) } break;                                                                  \
  }
  if (dtype == S2S_BF16) { S2S_TB_T(bf16_t) } else { S2S_TB_T(float) }
#undef S2S_TB_T
#undef S2S_TB
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
