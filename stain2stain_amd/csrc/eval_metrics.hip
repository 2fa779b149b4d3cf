// Evaluation (validation / test) passes of the multitask model: the losses without their gradients plus the
// reference's thresholded segmentation metrics, and the flow head + MSE without v, dx or dW.
//
//   s2s_seg_eval_binary      DiceLoss + BCEWithLogits (as s2s_seg_loss) and the metric block of
//                            validation_step / test_step (conditional_flow_matching_multitask.py:326-343, 366-381):
//                              pred = sigmoid(z) > 0.5, I = sum pred*g, P = sum pred, G = sum g, U = sum (pred | g)
//                              dice_coef = (2 I + 1e-7) / (P + G + 1e-7), iou = (I + 1e-7) / (U + 1e-7)   (fp32)
//   s2s_seg_eval_multiclass  softmax Dice + CE (as s2s_seg_loss_multiclass) and test_step's per-class metrics
//                            (conditional_flow_matching_multitask_multiclassloss.py:437-470): pred = argmax_c z
//                            (first maximal index), per class I_c, P_c, G_c, U_c, mean Dice / IoU over c != ignore
//   s2s_head_mse_eval        FlowMatchingDecoder.outc (task_decoders.py:132) + mean((v-u)^2) of model_step
//
// Every kernel reads its operands once, writes per-workgroup partials (fp64 sums, 64-bit counts) and leaves the
// combination to a one-workgroup finalize pass that walks them in a fixed order: no atomics, bit-reproducible run to run.
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
//
// Knife edge: pred uses the loss kernel's p = 1/(1+exp(-z)) > 0.5, which is not the same predicate as z > 0 for
// 0 < z <~ 1e-7 (p rounds to exactly 0.5 there).  torch's sigmoid on another device may round differently in that band.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int EV_BLOCKS = 512;          // partial rows of the segmentation passes (as seg_loss.hip)
constexpr int HM_BLOCKS = 2048;         // partial rows of the head + MSE pass
constexpr int MC_MAX = 8;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// torch's CPU sum of a short contiguous fp32 vector (n <= 7; the n = 8 order is host-dependent and may differ from this
// by one ulp): the first four terms seed four accumulators, the rest go to the first, then ((a0 + a1) + a2) + a3
__device__ __forceinline__ float torch_cpu_sum(const float* v, int n) {
  if (n <= 4) {
    float s = v[0];
    for (int i = 1; i < n; ++i) s += v[i];
    return s;
  }
  float a0 = v[0];
  for (int i = 4; i < n; ++i) a0 += v[i];
  return ((a0 + v[1]) + v[2]) + v[3];
}

// dice_coef / iou exactly as torch evaluates the reference's expressions: integer counts x Python float -> fp32
__device__ __forceinline__ float dice_coef_f32(float i, float pg) { return (2.0f * i + 1e-7f) / (pg + 1e-7f); }
__device__ __forceinline__ float iou_f32(float i, float u) { return (i + 1e-7f) / (u + 1e-7f); }

// ---------------------------------------------------------------------------------------------
// binary: part row = 4 doubles (sum p*g, sum p, sum g, sum bce) | cpart row = 4 counts (I, P, G, U)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_eval_reduce_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                                              long n, double* __restrict__ part,
                                                              unsigned long long* __restrict__ cpart) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned int c[4] = {0u, 0u, 0u, 0u};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float zi = z[i], gi = g[i];
    const float p = 1.f / (1.f + expf(-zi));          // the loss kernel's sigmoid
    s[0] += (double)(p * gi);
    s[1] += (double)p;
    s[2] += (double)gi;
    s[3] += (double)(fmaxf(zi, 0.f) - zi * gi + log1pf(expf(-fabsf(zi))));
    const bool pr = p > 0.5f, gt = gi != 0.f;
    c[0] += (pr && gt) ? 1u : 0u;
    c[1] += pr ? 1u : 0u;
    c[2] += gt ? 1u : 0u;
    c[3] += (pr || gt) ? 1u : 0u;
  }
  __shared__ double sd[4][4];
  __shared__ unsigned long long sc[4][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = wave_sum_d(s[k]);
    const unsigned long long b = wave_sum_u((unsigned long long)c[k]);
    if (lane == 0) { sd[wv][k] = a; sc[wv][k] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    part[(long)blockIdx.x * 4 + k] = ((sd[0][k] + sd[1][k]) + sd[2][k]) + sd[3][k];
    cpart[(long)blockIdx.x * 4 + k] = sc[0][k] + sc[1][k] + sc[2][k] + sc[3][k];
  }
}

// out[0..5) = seg, dice loss, bce, dice_coef, iou; counts[0..4) = I, P, G, U
__global__ void seg_eval_finalize_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ cpart,
                                         int nblk, long n, float smooth, float dice_w, float* __restrict__ out,
                                         long* __restrict__ counts) {
  __shared__ double sums[4];
  __shared__ unsigned long long cnt[4];
  const int k = threadIdx.x;
  if (k < 4) {
    double a = 0.0;
    unsigned long long b = 0;
    for (int i = 0; i < nblk; ++i) { a += part[(long)i * 4 + k]; b += cpart[(long)i * 4 + k]; }
    sums[k] = a;
    cnt[k] = b;
  }
  __syncthreads();
  if (k == 0) {
    const double I = sums[0], P = sums[1], G = sums[2];
    const double dice = 1.0 - (2.0 * I + smooth) / (P + G + smooth);
    const double bce = sums[3] / (double)n;
    out[0] = (float)(dice_w * dice + (1.0 - dice_w) * bce);
    out[1] = (float)dice;
    out[2] = (float)bce;
    // reference: union = pred.sum() + mask.sum() is an int64 sum, the iou union a .float().sum()
    out[3] = dice_coef_f32((float)(long long)cnt[0], (float)(long long)(cnt[1] + cnt[2]));
    out[4] = iou_f32((float)(long long)cnt[0], (float)(long long)cnt[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) counts[j] = (long)cnt[j];
  }
}

// ---------------------------------------------------------------------------------------------
// multiclass: part row = 26 doubles in s2s_seg_loss_multiclass's layout ([0..C) I_c, [8..) P_c, [16..) G_c, [24] CE sum,
// [25] CE count); cpart row = 32 counts ([0..C) I_c, [8..) P_c, [16..) G_c, [24..) U_c of the argmax prediction)
// ---------------------------------------------------------------------------------------------
constexpr int MC_SUMS = 26, MC_CNTS = 32;

template <int C>
__global__ __launch_bounds__(256) void mc_eval_reduce_kernel(const float* __restrict__ z, const long* __restrict__ tgt,
                                                             long npix, long HW, int ignore_index,
                                                             double* __restrict__ part,
                                                             unsigned long long* __restrict__ cpart) {
  double s[3 * C + 2];
  unsigned int cn[4 * C];
#pragma unroll
  for (int k = 0; k < 3 * C + 2; ++k) s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 4 * C; ++k) cn[k] = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const long n = i / HW, q = i - n * HW;
    const long t = tgt[i];
    const long base = n * C * HW + q;
    float zc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) zc[c] = z[base + c * HW];
    // softmax as softmax_px of seg_loss.hip
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) m = fmaxf(m, zc[c]);
    float p[C], sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(zc[c] - m); sum += p[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    const float lse = m + logf(sum);
    const bool dice_valid = !(ignore_index >= 0 && t == ignore_index);
    if (dice_valid) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float oh = (t == c) ? 1.f : 0.f;
        s[c] += (double)(p[c] * oh);
        s[C + c] += (double)p[c];
        s[2 * C + c] += (double)oh;
      }
    }
    if (t != ignore_index && t >= 0 && t < C) {
      float zt = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) zt = (t == c) ? zc[c] : zt;
      s[3 * C] += (double)(lse - zt);
      s[3 * C + 1] += 1.0;
    }
    // torch.argmax: the first maximal index (ascending scan, strict >)
    int am = 0;
    float best = zc[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
      if (zc[c] > best) { best = zc[c]; am = c; }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const bool pr = am == c, gt = t == c;
      cn[c] += (pr && gt) ? 1u : 0u;
      cn[C + c] += pr ? 1u : 0u;
      cn[2 * C + c] += gt ? 1u : 0u;
      cn[3 * C + c] += (pr || gt) ? 1u : 0u;
    }
  }
  __shared__ double sd[4][3 * C + 2];
  __shared__ unsigned long long sc[4][4 * C];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3 * C + 2; ++k) {
    const double a = wave_sum_d(s[k]);
    if (lane == 0) sd[wv][k] = a;
  }
#pragma unroll
  for (int k = 0; k < 4 * C; ++k) {
    const unsigned long long b = wave_sum_u((unsigned long long)cn[k]);
    if (lane == 0) sc[wv][k] = b;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < 3 * C + 2) {
    const int slot = k < C ? k : k < 2 * C ? 8 + (k - C) : k < 3 * C ? 16 + (k - 2 * C) : 24 + (k - 3 * C);
    part[(long)blockIdx.x * MC_SUMS + slot] = ((sd[0][k] + sd[1][k]) + sd[2][k]) + sd[3][k];
  } else if (k >= 64 && k < 64 + 4 * C) {
    const int j = k - 64, slot = (j / C) * 8 + (j % C);
    cpart[(long)blockIdx.x * MC_CNTS + slot] = sc[0][j] + sc[1][j] + sc[2][j] + sc[3][j];
  }
}

// out[0..5) = seg, dice loss, ce, mean dice_coef, mean iou; counts[32] = I_c, P_c, G_c, U_c at [0|8|16|24 + c]
__global__ void mc_eval_finalize_kernel(const double* __restrict__ part, const unsigned long long* __restrict__ cpart,
                                        int nblk, int C, int ignore_index, float smooth, float dice_w,
                                        float* __restrict__ out, long* __restrict__ counts) {
  __shared__ double sums[MC_SUMS];
  __shared__ unsigned long long cnt[MC_CNTS];
  const int k = threadIdx.x;
  if (k < MC_SUMS) {
    double a = 0.0;
    if (k >= 24 || (k & 7) < C)
      for (int i = 0; i < nblk; ++i) a += part[(long)i * MC_SUMS + k];
    sums[k] = a;
  } else if (k >= 32 && k < 32 + MC_CNTS) {
    const int j = k - 32;
    unsigned long long b = 0;
    if ((j & 7) < C)
      for (int i = 0; i < nblk; ++i) b += cpart[(long)i * MC_CNTS + j];
    cnt[j] = b;
  }
  __syncthreads();
  if (k < MC_CNTS) counts[k] = (long)cnt[k];
  if (k == 0) {
    double md = 0.0;
    for (int c = 0; c < C; ++c) md += (2.0 * sums[c] + smooth) / (sums[8 + c] + sums[16 + c] + smooth);
    const double dice = 1.0 - md / C;
    const double ce = sums[24] / sums[25];          // 0/0 = nan when every pixel is ignored, like torch
    out[0] = (float)(dice_w * dice + (1.0 - dice_w) * ce);
    out[1] = (float)dice;
    out[2] = (float)ce;
    // reference: per class (pred_c & target_c).float().sum() etc., then torch.stack(list).mean() = the CPU fp32 sum of
    // the list divided by its length
    float vd[MC_MAX], vi[MC_MAX];
    int kept = 0;
    for (int c = 0; c < C; ++c) {
      if (c == ignore_index) continue;
      const float I = (float)(long long)cnt[c], P = (float)(long long)cnt[8 + c], G = (float)(long long)cnt[16 + c],
                  U = (float)(long long)cnt[24 + c];
      vd[kept] = dice_coef_f32(I, P + G);
      vi[kept] = iou_f32(I, U);
      ++kept;
    }
    out[3] = kept ? torch_cpu_sum(vd, kept) / (float)kept : 0.f;
    out[4] = kept ? torch_cpu_sum(vi, kept) / (float)kept : 0.f;
  }
}

template <int C>
void mc_eval_launch(const float* z, const long* t, float* out, long* counts, double* work, long npix, long HW,
                    int ignore, float smooth, float dw, hipStream_t s) {
  long nb = (npix + 255) / 256;
  if (nb > EV_BLOCKS) nb = EV_BLOCKS;
  unsigned long long* cpart = reinterpret_cast<unsigned long long*>(work + (long)EV_BLOCKS * MC_SUMS);
  hipLaunchKernelGGL(mc_eval_reduce_kernel<C>, dim3((int)nb), dim3(256), 0, s, z, t, npix, HW, ignore, work, cpart);
  hipLaunchKernelGGL(mc_eval_finalize_kernel, dim3(1), dim3(64), 0, s, work, cpart, (int)nb, C, ignore, smooth, dw, out,
                     counts);
}

// ---------------------------------------------------------------------------------------------
// head + MSE, forward only: v = W a + b never leaves the registers.  A pixel is served by GL lanes (GL a power of two,
// 8*GL <= C); lane j of the group reads the 8-channel chunks j, j+GL, ... of its pixel (one 16-byte load per chunk in
// bf16, two in fp32), the GL partial dot products meet in a DPP butterfly, and the lane that owns output o reads u there.
// Each thread keeps UN pixels' loads in flight.
// ---------------------------------------------------------------------------------------------
// sum over the GL lanes of a pixel group by DPP moves (no LDS round trip, unlike __shfl_xor's ds_bpermute):
// quad_perm [1,0,3,2] and [2,3,0,1] leave the quad's sum in each of its lanes, row_half_mirror (lane i <-> 7-i) adds the
// other quad of the 8-lane group
template <int GL>
__device__ __forceinline__ float group_sum(float v) {
  if (GL >= 2) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
  if (GL >= 4) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, true));
  if (GL >= 8) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true));
  return v;
}

__device__ __forceinline__ f32x8 ld8(const float* p) { return load8(p); }
__device__ __forceinline__ f32x8 ld8(const bf16_t* p) {
  const s16x8 v = *reinterpret_cast<const s16x8*>(p);
  f32x8 r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r.v[k] = __uint_as_float(((unsigned int)(unsigned short)v[k]) << 16);
  return r;
}

template <typename T, int GL, int MO, int UN>
__global__ __launch_bounds__(256) void head_mse_eval_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ u,
                                                            double* __restrict__ lpart, long npix, long HW, int C,
                                                            int Cout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wl = reinterpret_cast<float*>(smem);          // [MO][C], rows >= Cout zero
  __shared__ double red[4];
  for (int i = threadIdx.x; i < MO * C; i += 256) wl[i] = i < Cout * C ? w[i] : 0.f;
  __syncthreads();
  constexpr int PPB = 256 / GL;                         // pixels per workgroup and unroll slot
  const int pc = threadIdx.x & (GL - 1), slot = threadIdx.x / GL;
  float bo[MO];
#pragma unroll
  for (int o = 0; o < MO; ++o) bo[o] = (o < Cout && bias) ? bias[o] : 0.f;
  double acc = 0.0;
  const long stride = (long)gridDim.x * PPB * UN;
  for (long p0 = (long)blockIdx.x * PPB * UN; p0 < npix; p0 += stride) {
    // the owner lanes' u first, so that its latency hides under the activation loads
    float uv[UN][MO];
#pragma unroll
    for (int r = 0; r < UN; ++r) {
      const long p = p0 + (long)r * PPB + slot;
      const int pi = (int)p, hw = (int)HW;             // 32-bit: the launcher keeps npix + one grid stride < 2^31
      const int n = pi / hw, q = pi - n * hw;
#pragma unroll
      for (int o = 0; o < MO; ++o)
        uv[r][o] = (p < npix && o < Cout && (o & (GL - 1)) == pc) ? u[((long)n * Cout + o) * HW + q] : 0.f;
    }
    float vv[UN][MO];
#pragma unroll
    for (int r = 0; r < UN; ++r)
#pragma unroll
      for (int o = 0; o < MO; ++o) vv[r][o] = 0.f;
    for (int c8 = pc * 8; c8 < C; c8 += GL * 8) {
      f32x8 a[UN];
#pragma unroll
      for (int r = 0; r < UN; ++r) {
        const long p = p0 + (long)r * PPB + slot;
        if (p < npix) a[r] = ld8(x + p * ldx + c8);
        else {
#pragma unroll
          for (int k = 0; k < 8; ++k) a[r].v[k] = 0.f;
        }
      }
#pragma unroll
      for (int o = 0; o < MO; ++o) {
        float wr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wr[k] = wl[o * C + c8 + k];
#pragma unroll
        for (int r = 0; r < UN; ++r)
#pragma unroll
          for (int k = 0; k < 8; ++k) vv[r][o] = fmaf(a[r].v[k], wr[k], vv[r][o]);
      }
    }
#pragma unroll
    for (int r = 0; r < UN; ++r) {
      const long p = p0 + (long)r * PPB + slot;
#pragma unroll
      for (int o = 0; o < MO; ++o) {
        const float t = group_sum<GL>(vv[r][o]);
        if (p < npix && o < Cout && (o & (GL - 1)) == pc) {
          const float d = (t + bo[o]) - uv[r][o];
          acc += (double)(d * d);
        }
      }
    }
  }
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) lpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void head_mse_finalize_kernel(const double* __restrict__ lpart, int nblk,
                                                                double inv_count, float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += lpart[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] * inv_count);
}

constexpr int HM_UN = 4;

int head_mse_blocks(long npix, int gl) {
  const long per = (long)(256 / gl) * HM_UN;
  long nb = (npix + per - 1) / per;
  return (int)(nb < HM_BLOCKS ? nb : HM_BLOCKS);
}

int head_mse_lanes(int C) {
  int gl = 1;
  while (gl < 8 && gl * 16 <= C) gl <<= 1;              // largest power of two <= 8 with 8*gl <= C
  return gl;
}

// Which instantiation s2s_head_mse_eval launches (s2s_head_mse_family): 256 MO + GL, GL = lanes per pixel (1, 2, 4, 8) and
// MO = 3, 4 or 8 outputs unrolled; a negative status is a launch the entry point refuses.  It dispatches on this value.
int head_mse_family(int dtype, int B, int H, int W, int C, int Cout) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8) || Cout <= 0 || Cout > 8) return S2S_ERR_SHAPE;
  if (8 * C * 4 > 60 * 1024) return S2S_ERR_SHAPE;
  if (dtype != S2S_BF16 && dtype != S2S_F32) return S2S_ERR_DTYPE;
  if ((long)B * H * W >= (1L << 31) - (1L << 22)) return S2S_ERR_SHAPE;   // 32-bit pixel index (+ one grid stride) in the kernel
  return 256 * (Cout == 3 ? 3 : Cout <= 4 ? 4 : 8) + head_mse_lanes(C);
}

template <typename T, int MO>
void head_mse_launch(const void* x, int ldx, const float* w, const float* bias, const float* u, double* lpart, long npix,
                     long HW, int C, int Cout, int gl, int nb, hipStream_t s) {
  const int lds = MO * C * 4;
#define S2S_HM(G)                                                                                                 \
  hipLaunchKernelGGL((head_mse_eval_kernel<T, G, MO, HM_UN>), dim3(nb), dim3(256), lds, s, (const T*)x, ldx, w, bias, \
                     u, lpart, npix, HW, C, Cout)
  switch (gl) {
    case 1: S2S_HM(1); break;
    case 2: S2S_HM(2); break;
    case 4: S2S_HM(4); break;
    default: S2S_HM(8); break;
  }
#undef S2S_HM
}

}  // namespace

extern "C" int s2s_seg_eval_binary(const float* z, const float* g, float* out, long* counts, double* work, long n,
                                   float smooth, float dice_weight, void* stream) {
  if (!z || !g || !out || !counts || !work) return S2S_ERR_NULL;
  if (n <= 0 || n > (1L << 40)) return S2S_ERR_SHAPE;
  if (n / EV_BLOCKS / 256 >= (1L << 32) - 1) return S2S_ERR_SHAPE;   // per-thread 32-bit counts
  hipStream_t s = (hipStream_t)stream;
  long nb = (n + 255) / 256;
  if (nb > EV_BLOCKS) nb = EV_BLOCKS;
  unsigned long long* cpart = reinterpret_cast<unsigned long long*>(work + (long)EV_BLOCKS * 4);
  hipLaunchKernelGGL(seg_eval_reduce_kernel, dim3((int)nb), dim3(256), 0, s, z, g, n, work, cpart);
  hipLaunchKernelGGL(seg_eval_finalize_kernel, dim3(1), dim3(64), 0, s, work, cpart, (int)nb, n, smooth, dice_weight,
                     out, counts);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_seg_eval_multiclass(const float* z, const long* target, float* out, long* counts, double* work,
                                       long B, long HW, int C, int ignore_index, float smooth, float dice_weight,
                                       void* stream) {
  if (!z || !target || !out || !counts || !work) return S2S_ERR_NULL;
  if (B <= 0 || HW <= 0 || C < 2 || C > MC_MAX) return S2S_ERR_SHAPE;
  const long npix = B * HW;
  if (npix / EV_BLOCKS / 256 >= (1L << 32) - 1) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
#define S2S_MCE(CC) case CC: mc_eval_launch<CC>(z, target, out, counts, work, npix, HW, ignore_index, smooth, dice_weight, s); break;
  switch (C) { S2S_MCE(2) S2S_MCE(3) S2S_MCE(4) S2S_MCE(5) S2S_MCE(6) S2S_MCE(7) S2S_MCE(8) }
#undef S2S_MCE
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_head_mse_eval_blocks(int B, int H, int W, int C) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 8)) return S2S_ERR_SHAPE;
  return head_mse_blocks((long)B * H * W, head_mse_lanes(C));
}

extern "C" int s2s_head_mse_family(int dtype, int B, int H, int W, int C, int Cout) {
  return head_mse_family(dtype, B, H, W, C, Cout);
}

extern "C" int s2s_head_mse_eval(int dtype, const void* x, int ldx, const float* w, const float* bias,
                                 const float* u_nchw, float* loss, double* lpart, int B, int H, int W, int C, int Cout,
                                 void* stream) {
  if (!x || !w || !u_nchw || !loss || !lpart) return S2S_ERR_NULL;
  if (ldx < C || (ldx % 8)) return S2S_ERR_SHAPE;
  const int fam = head_mse_family(dtype, B, H, W, C, Cout);
  if (fam < 0) return fam;
  if (((uintptr_t)x) & 15) return S2S_ERR_ALIGN;
  const long npix = (long)B * H * W, HW = (long)H * W;
  const int gl = fam & 255, mo = fam >> 8;
  const int nb = head_mse_blocks(npix, gl);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == S2S_BF16) {
    if (mo == 3) head_mse_launch<bf16_t, 3>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
    else if (mo == 4) head_mse_launch<bf16_t, 4>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
    else head_mse_launch<bf16_t, 8>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
  } else {
    if (mo == 3) head_mse_launch<float, 3>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
    else if (mo == 4) head_mse_launch<float, 4>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
    else head_mse_launch<float, 8>(x, ldx, w, bias, u_nchw, lpart, npix, HW, C, Cout, gl, nb, s);
  }
  hipLaunchKernelGGL(head_mse_finalize_kernel, dim3(1), dim3(256), 0, s, lpart, nb, 1.0 / ((double)npix * Cout), loss);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
