// Per-sample adaptive Dormand-Prince 5(4) on the device.
//
//   s2s_dp_partials   partial sums per sample of the error-norm kernels (the workspace size)
//   s2s_dp_init       Hairer's initial step per sample, around the two extra network evaluations
//   s2s_dp_stage      out = y + sum_j (h_b a_ij) k_j and the node time float(t_b + c_i h_b), one pass
//   s2s_dp_error      the 4th/5th-order difference in registers, per-sample scaled square sums (fixed block order)
//   s2s_dp_control    per sample: norm, accept / reject, t, h, counters, flags; the status word of the batch
//   s2s_dp_commit     accepted samples: y <- y_new, k1 <- k7 (first same as last)
//
// Every sample b owns a row of DP_SLOTS doubles in `state`; a sample that has reached t = 1 is frozen (h = 0, its
// stage inputs are y, its state and counters no longer change).  The element arithmetic repeats the batch-wide
// sampler's s2s_axpy chain operation for operation (x = fma((float)(h a_ij), k_j, x) over ascending j, zero
// coefficients skipped; the error from 0 the same way), so a sample alone in a batch of one is stepped exactly as
// dopri5_integrate steps it.  The scalar double arithmetic is written with contraction off, as Python evaluates it.
// Nothing here allocates or synchronises: a whole attempted step can be captured.
//
// Fixed-step explicit Runge-Kutta schemes with at most four stages, same conventions:
//
//   s2s_rk_stage      out = x + sum_j c_j k_j (c_j = the host's float(h a_ij), zero terms left out) and the node time
//                     t_out[0..B) = table[counter * stages + stage], one pass
//   s2s_rk_combine    x += sum_j c_j k_j (c_j = float(h b_j)) in place, one pass; advances the step counter
#include "common.h"

namespace {

enum { S_T, S_H, S_ACC, S_REJ, S_REJECTED, S_DONE, S_ACCEPT, S_AUX, DP_SLOTS };   // S_AUX: d1 in init, then last norm
enum { ST_ACTIVE, ST_LIMIT, ST_ATTEMPTS, ST_WORDS = 4 };

// Dormand-Prince nodes, stage rows (row 6 = the 5th-order weights) and error weights, as samplers._DP_*.
// Row 0 is the initial-step probe y + h0 k1 of s2s_dp_init.
__device__ constexpr double kC[7] = {1.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__device__ constexpr double kA[7][6] = {
    {1.0},
    {1.0 / 5},
    {3.0 / 40, 9.0 / 40},
    {44.0 / 45, -56.0 / 15, 32.0 / 9},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656},
    {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
__device__ constexpr double kE[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525,
                                     1.0 / 40};

constexpr int kThreads = 256;
constexpr int kMaxPartials = 128;

inline int dp_partials(long n4) {
  long b = (n4 + 2 * kThreads - 1) / (2 * kThreads);
  return (int)(b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b));
}
inline int dp_grid_x(long n4) {
  long b = (n4 + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

__device__ __forceinline__ double node_time(double t, double c, double h) {
#pragma clang fp contract(off)
  return t + c * h;                                   // Python: t + _DP_C[i] * h, two roundings
}

// sqrt(mean) rounded to fp32, as s2s_ode_error_norm hands the batch-wide sampler its norm
__device__ __forceinline__ double rms_f32(double sum, long n) { return (double)(float)sqrt(sum * (1.0 / (double)n)); }

// block sum of one double per thread, result valid in thread 0
__device__ __forceinline__ double block_sum(double s) {
  __shared__ double red[kThreads];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// out = y + sum_{j<I} (float)(h a_Ij) k_j; grid (x, B).  I = 0: the probe y + (float)h0 k1.
template <int I>
__global__ __launch_bounds__(kThreads) void dp_stage_kernel(const f32x4* __restrict__ y, const f32x4* __restrict__ k0,
                                                            const f32x4* __restrict__ k1, const f32x4* __restrict__ k2,
                                                            const f32x4* __restrict__ k3, const f32x4* __restrict__ k4,
                                                            const f32x4* __restrict__ k5, const double* __restrict__ state,
                                                            f32x4* __restrict__ out, float* __restrict__ t_out, long n4) {
  constexpr int NJ = I == 0 ? 1 : I;
  const int b = blockIdx.y;
  const double* st = state + (long)b * DP_SLOTS;
  const double h = st[S_H];
  const bool frozen = st[S_DONE] != 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = (float)node_time(st[S_T], kC[I], h);
  float a[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) a[j] = (float)(h * kA[I][j]);
  const f32x4* ks[6] = {k0, k1, k2, k3, k4, k5};
  const long base = (long)b * n4;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    f32x4 x = y[base + i];
    if (!frozen) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (kA[I][j] != 0.0) x += a[j] * ks[j][base + i];       // s2s_axpy's expression: one fma per term
    }
    out[base + i] = x;
  }
}

// part[b * nblk + blockIdx.x] = sum over this block's share of sample b of (e / (atol + rtol max(|y0|, |y1|)))^2, e the
// error estimate sum_j (float)(h e_j) k_j; the same block count and order every run.  Frozen samples are skipped.
__global__ __launch_bounds__(kThreads) void dp_error_kernel(
    const f32x4* __restrict__ k0, const f32x4* __restrict__ k1, const f32x4* __restrict__ k2,
    const f32x4* __restrict__ k3, const f32x4* __restrict__ k4, const f32x4* __restrict__ k5,
    const f32x4* __restrict__ k6, const f32x4* __restrict__ y0, const f32x4* __restrict__ y1,
    const double* __restrict__ state, float atol, float rtol, long n4, double* __restrict__ part) {
  const int b = blockIdx.y;
  const double* st = state + (long)b * DP_SLOTS;
  if (st[S_DONE] != 0.0) return;
  const double h = st[S_H];
  float a[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) a[j] = (float)(h * kE[j]);
  const f32x4* ks[7] = {k0, k1, k2, k3, k4, k5, k6};
  const long base = (long)b * n4;
  double s = 0.0;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    f32x4 e = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 7; ++j)
      if (kE[j] != 0.0) e += a[j] * ks[j][base + i];
    const f32x4 p = y0[base + i], q = y1[base + i];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sc = atol + rtol * fmaxf(fabsf(p[c]), fabsf(q[c]));    // ode_err_partial_kernel's expression
      const float r = e[c] / sc;
      s += (double)r * (double)r;
    }
  }
  s = block_sum(s);
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = s;
}

// init, first half: part[0 .. B*nblk) <- sums of (y / sc)^2, part[B*nblk ..) <- sums of (k1 / sc)^2, sc from y alone;
// second half (d != nullptr): part[0 .. B*nblk) <- sums of ((fa - k1) / sc)^2
__global__ __launch_bounds__(kThreads) void dp_init_norm_kernel(const f32x4* __restrict__ y, const f32x4* __restrict__ k1,
                                                                const f32x4* __restrict__ fa, float atol, float rtol,
                                                                long n4, double* __restrict__ part) {
  const int b = blockIdx.y;
  const long base = (long)b * n4;
  double s0 = 0.0, s1 = 0.0;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    const f32x4 p = y[base + i], k = k1[base + i];
    f32x4 d = p;
    if (fa) {
      d = fa[base + i];
      d += -1.0f * k;                                 // axpy_(fa, k1, -1.0)
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float sc = atol + rtol * fmaxf(fabsf(p[c]), fabsf(p[c]));
      const float r0 = d[c] / sc;
      s0 += (double)r0 * (double)r0;
      if (!fa) {
        const float r1 = k[c] / sc;
        s1 += (double)r1 * (double)r1;
      }
    }
  }
  const long slot = (long)b * gridDim.x + blockIdx.x;
  s0 = block_sum(s0);
  if (threadIdx.x == 0) part[slot] = s0;
  if (!fa) {
    __syncthreads();
    s1 = block_sum(s1);
    if (threadIdx.x == 0) part[(long)gridDim.y * gridDim.x + slot] = s1;
  }
}

__device__ __forceinline__ double sum_row(const double* p, int nblk) {
  double s = 0.0;
  for (int j = 0; j < nblk; ++j) s += p[j];
  return s;
}

// init, after the first evaluation: h0 per sample (Hairer, Norsett, Wanner II.4), t = 0; d1 kept in S_AUX
__global__ __launch_bounds__(kThreads) void dp_init_h0_kernel(const double* __restrict__ part, int nblk, int B, long n,
                                                              double* __restrict__ state) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const double d0 = rms_f32(sum_row(part + (long)b * nblk, nblk), n);
    const double d1 = rms_f32(sum_row(part + ((long)B + b) * nblk, nblk), n);
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    double* st = state + (long)b * DP_SLOTS;
    for (int s = 0; s < DP_SLOTS; ++s) st[s] = 0.0;
    st[S_H] = h0;
    st[S_AUX] = d1;
  }
}

// init, after the probe evaluation: the first step h per sample; counters and flags cleared; the status word reset
__global__ __launch_bounds__(kThreads) void dp_init_h_kernel(const double* __restrict__ part, int nblk, int B, long n,
                                                             double* __restrict__ state, int* __restrict__ status) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < B; b += kThreads) {
    double* st = state + (long)b * DP_SLOTS;
    const double h0 = st[S_H], d1 = st[S_AUX];
    const double d2 = rms_f32(sum_row(part + (long)b * nblk, nblk), n) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / 5.0);
    st[S_H] = fmin(fmin(100 * h0, h1), 1.0 - 0.0);
    st[S_AUX] = 0.0;
  }
  if (threadIdx.x == 0) {
    status[ST_ACTIVE] = B;
    status[ST_LIMIT] = 0;
    status[ST_ATTEMPTS] = 0;
    status[3] = 0;
  }
}

__global__ __launch_bounds__(kThreads) void dp_control_kernel(const double* __restrict__ part, int nblk, int B, long n,
                                                              int max_steps, double* __restrict__ state,
                                                              int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ int cnt[kThreads];
  int active = 0;
  for (int b = threadIdx.x; b < B; b += kThreads) {
    double* st = state + (long)b * DP_SLOTS;
    if (st[S_DONE] != 0.0) {
      st[S_ACCEPT] = 0.0;
      continue;
    }
    const double en = rms_f32(sum_row(part + (long)b * nblk, nblk), n);
    double t = st[S_T], h = st[S_H];
    if (en < 1.0) {
      double factor = en == 0.0 ? 10.0 : fmin(10.0, 0.9 * pow(en, -0.2));
      if (st[S_REJECTED] != 0.0) factor = fmin(1.0, factor);
      t = t + h;
      h = h * factor;
      st[S_REJECTED] = 0.0;
      st[S_ACC] += 1.0;
      st[S_ACCEPT] = 1.0;
    } else {
      h = h * fmax(0.2, 0.9 * pow(en, -0.2));
      st[S_REJECTED] = 1.0;
      st[S_REJ] += 1.0;
      st[S_ACCEPT] = 0.0;
    }
    if (t >= 1.0) {                                   // frozen from now on
      st[S_DONE] = 1.0;
      h = 0.0;
    } else {
      h = fmin(h, 1.0 - t);                           // the loop head's h = min(h, t1 - t)
      ++active;
    }
    st[S_T] = t;
    st[S_H] = h;
    st[S_AUX] = en;
  }
  cnt[threadIdx.x] = active;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) cnt[threadIdx.x] += cnt[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int attempts = status[ST_ATTEMPTS] + 1;
    status[ST_ACTIVE] = cnt[0];
    status[ST_ATTEMPTS] = attempts;
    status[ST_LIMIT] = attempts >= max_steps ? 1 : 0;     // dopri5_integrate raises once max_steps attempts ran
  }
}

__global__ __launch_bounds__(kThreads) void dp_commit_kernel(f32x4* __restrict__ y, const f32x4* __restrict__ y_new,
                                                             f32x4* __restrict__ k1, const f32x4* __restrict__ k7,
                                                             const double* __restrict__ state, long n4) {
  const int b = blockIdx.y;
  if (state[(long)b * DP_SLOTS + S_ACCEPT] == 0.0) return;
  const long base = (long)b * n4;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    y[base + i] = y_new[base + i];
    k1[base + i] = k7[base + i];
  }
}

// ---- fixed-step explicit Runge-Kutta ------------------------------------------------------------------------------
// One term of the s2s_axpy chain, x = fma(c, k, x) per element, written as an fma so that no contraction setting can
// regroup the chain; the results are bit-equal to clone + s2s_axpy per coefficient.
__device__ __forceinline__ f32x4 rk_term(float c, f32x4 k, f32x4 acc) {
  const f32x4 c4 = {c, c, c, c};
  return __builtin_elementwise_fma(c4, k, acc);
}

// the node time of stage `stage` of step *counter; a step past the table's end reads nothing and yields NaN
__device__ __forceinline__ float rk_node_time(const float* __restrict__ table, const int* __restrict__ counter, int stages,
                                              int stage, int table_len) {
  const long idx = (long)counter[0] * stages + stage;
  return (idx >= 0 && idx < table_len) ? table[idx] : __builtin_nanf("");
}

// out = x + sum_{j<NK} c_j k_j, grid (x, B); block (0, b) writes t_out[b].  The counter is only read here.
template <int NK>
__global__ __launch_bounds__(kThreads) void rk_stage_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ k0,
                                                            const f32x4* __restrict__ k1, const f32x4* __restrict__ k2,
                                                            float c0, float c1, float c2, f32x4* __restrict__ out,
                                                            float* __restrict__ t_out, const float* __restrict__ table,
                                                            const int* __restrict__ counter, int stages, int stage,
                                                            int table_len, long n4) {
  const int b = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) t_out[b] = rk_node_time(table, counter, stages, stage, table_len);
  const long base = (long)b * n4;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    f32x4 acc = x[base + i];
    if (NK > 0) acc = rk_term(c0, k0[base + i], acc);
    if (NK > 1) acc = rk_term(c1, k1[base + i], acc);
    if (NK > 2) acc = rk_term(c2, k2[base + i], acc);
    out[base + i] = acc;
  }
}

// the node time alone (the first stage evaluates the network on x itself): t_out[0..B)
__global__ __launch_bounds__(kThreads) void rk_time_kernel(float* __restrict__ t_out, int B, const float* __restrict__ table,
                                                           const int* __restrict__ counter, int stages, int stage,
                                                           int table_len) {
  const float v = rk_node_time(table, counter, stages, stage, table_len);
  for (int b = threadIdx.x; b < B; b += kThreads) t_out[b] = v;
}

// x += sum_{j<NK} c_j k_j in place, grid (x, B); one thread of the launch advances the step counter, nobody reads it
template <int NK>
__global__ __launch_bounds__(kThreads) void rk_combine_kernel(f32x4* __restrict__ x, const f32x4* __restrict__ k0,
                                                              const f32x4* __restrict__ k1, const f32x4* __restrict__ k2,
                                                              const f32x4* __restrict__ k3, float c0, float c1, float c2,
                                                              float c3, int* __restrict__ counter, long n4) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counter[0] += 1;
  const long base = (long)blockIdx.y * n4;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long)gridDim.x * kThreads) {
    f32x4 acc = x[base + i];
    acc = rk_term(c0, k0[base + i], acc);
    if (NK > 1) acc = rk_term(c1, k1[base + i], acc);
    if (NK > 2) acc = rk_term(c2, k2[base + i], acc);
    if (NK > 3) acc = rk_term(c3, k3[base + i], acc);
    x[base + i] = acc;
  }
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

inline int check_bn(int B, long n) {
  if (B <= 0 || B > 65535 || n <= 0 || (n % 4)) return S2S_ERR_SHAPE;
  return S2S_OK;
}

template <int I>
void launch_stage(const float* y, const float* const* k, const double* state, float* out, float* t_out, int B, long n,
                  hipStream_t s) {
  const long n4 = n / 4;
  hipLaunchKernelGGL(dp_stage_kernel<I>, dim3(dp_grid_x(n4), B), dim3(kThreads), 0, s, (const f32x4*)y,
                     (const f32x4*)k[0], (const f32x4*)k[1], (const f32x4*)k[2], (const f32x4*)k[3], (const f32x4*)k[4],
                     (const f32x4*)k[5], state, (f32x4*)out, t_out, n4);
}

}  // namespace

extern "C" int s2s_dp_partials(long n) { return n > 0 ? dp_partials(n / 4) : 0; }

extern "C" int s2s_dp_init(int phase, const float* y, const float* k1, const float* fa, double* state, double* part,
                           float* out, float* t_out, int* status, float atol, float rtol, int B, long n, void* stream) {
  if (!y || !k1 || !state || !part || !status) return S2S_ERR_NULL;
  if (phase == 0 && (!out || !t_out)) return S2S_ERR_NULL;
  if (phase == 1 && !fa) return S2S_ERR_NULL;
  if ((phase != 0 && phase != 1) || check_bn(B, n)) return S2S_ERR_SHAPE;
  if (misaligned(y) || misaligned(k1) || misaligned(fa) || misaligned(out)) return S2S_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const long n4 = n / 4;
  const int nblk = dp_partials(n4);
  hipLaunchKernelGGL(dp_init_norm_kernel, dim3(nblk, B), dim3(kThreads), 0, s, (const f32x4*)y, (const f32x4*)k1,
                     phase == 1 ? (const f32x4*)fa : nullptr, atol, rtol, n4, part);
  if (phase == 0) {
    hipLaunchKernelGGL(dp_init_h0_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, nblk, B, n, state);
    const float* k[6] = {k1, k1, k1, k1, k1, k1};
    launch_stage<0>(y, k, state, out, t_out, B, n, s);
  } else {
    hipLaunchKernelGGL(dp_init_h_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, nblk, B, n, state, status);
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_dp_stage(int i, const float* y, const float* k1, const float* k2, const float* k3, const float* k4,
                            const float* k5, const float* k6, const double* state, float* out, float* t_out, int B,
                            long n, void* stream) {
  if (i < 1 || i > 6) return S2S_ERR_SHAPE;
  const float* k[6] = {k1, k2, k3, k4, k5, k6};
  if (!y || !state || !out || !t_out) return S2S_ERR_NULL;
  for (int j = 0; j < i; ++j)
    if (!k[j]) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  if (misaligned(y) || misaligned(out)) return S2S_ERR_ALIGN;
  for (int j = 0; j < i; ++j)
    if (misaligned(k[j])) return S2S_ERR_ALIGN;
  for (int j = i; j < 6; ++j) k[j] = k[0];            // rows shorter than 6 never read them
  hipStream_t s = (hipStream_t)stream;
  switch (i) {
    case 1: launch_stage<1>(y, k, state, out, t_out, B, n, s); break;
    case 2: launch_stage<2>(y, k, state, out, t_out, B, n, s); break;
    case 3: launch_stage<3>(y, k, state, out, t_out, B, n, s); break;
    case 4: launch_stage<4>(y, k, state, out, t_out, B, n, s); break;
    case 5: launch_stage<5>(y, k, state, out, t_out, B, n, s); break;
    default: launch_stage<6>(y, k, state, out, t_out, B, n, s); break;
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_dp_error(const float* k1, const float* k2, const float* k3, const float* k4, const float* k5,
                            const float* k6, const float* k7, const float* y, const float* y_new, const double* state,
                            double* part, float atol, float rtol, int B, long n, void* stream) {
  const float* k[7] = {k1, k2, k3, k4, k5, k6, k7};
  for (int j = 0; j < 7; ++j)
    if (j != 1 && !k[j]) return S2S_ERR_NULL;          // e_2 = 0: k2 is never read
  if (!y || !y_new || !state || !part) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  for (int j = 0; j < 7; ++j)
    if (misaligned(k[j])) return S2S_ERR_ALIGN;
  if (misaligned(y) || misaligned(y_new)) return S2S_ERR_ALIGN;
  const long n4 = n / 4;
  hipLaunchKernelGGL(dp_error_kernel, dim3(dp_partials(n4), B), dim3(kThreads), 0, (hipStream_t)stream,
                     (const f32x4*)k1, (const f32x4*)(k2 ? k2 : k1), (const f32x4*)k3, (const f32x4*)k4,
                     (const f32x4*)k5, (const f32x4*)k6, (const f32x4*)k7, (const f32x4*)y, (const f32x4*)y_new, state,
                     atol, rtol, n4, part);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_dp_control(double* state, const double* part, int* status, int max_steps, int B, long n,
                              void* stream) {
  if (!state || !part || !status) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(dp_control_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, part, dp_partials(n / 4), B, n,
                     max_steps, state, status);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_dp_commit(float* y, const float* y_new, float* k1, const float* k7, const double* state, int B,
                             long n, void* stream) {
  if (!y || !y_new || !k1 || !k7 || !state) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  if (misaligned(y) || misaligned(y_new) || misaligned(k1) || misaligned(k7)) return S2S_ERR_ALIGN;
  const long n4 = n / 4;
  hipLaunchKernelGGL(dp_commit_kernel, dim3(dp_grid_x(n4), B), dim3(kThreads), 0, (hipStream_t)stream, (f32x4*)y,
                     (const f32x4*)y_new, (f32x4*)k1, (const f32x4*)k7, state, n4);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// ---- fixed-step explicit Runge-Kutta ------------------------------------------------------------------------------
extern "C" int s2s_rk_stage(const float* x, const float* k1, const float* k2, const float* k3, float c1, float c2,
                            float c3, int nk, float* out, float* t_out, const float* table, const int* counter,
                            int stages, int stage, int table_len, int B, long n, void* stream) {
  if (nk < 0 || nk > 3 || stages < 1 || stages > 4 || stage < 0 || stage >= stages || table_len < stages)
    return S2S_ERR_SHAPE;
  const float* k[3] = {k1, k2, k3};
  if (!t_out || !table || !counter) return S2S_ERR_NULL;
  if (nk > 0 && (!x || !out)) return S2S_ERR_NULL;
  if (out && !x) return S2S_ERR_NULL;
  for (int j = 0; j < nk; ++j)
    if (!k[j]) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  if (misaligned(x) || misaligned(out)) return S2S_ERR_ALIGN;
  for (int j = 0; j < nk; ++j)
    if (misaligned(k[j])) return S2S_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const long n4 = n / 4;
  const dim3 grid(dp_grid_x(n4), B), block(kThreads);
  const f32x4 *X = (const f32x4*)x, *K0 = (const f32x4*)k1, *K1 = (const f32x4*)k2, *K2 = (const f32x4*)k3;
  f32x4* O = (f32x4*)out;
  if (!out) {
    hipLaunchKernelGGL(rk_time_kernel, dim3(1), block, 0, s, t_out, B, table, counter, stages, stage, table_len);
  } else {
    switch (nk) {
      case 0: hipLaunchKernelGGL(rk_stage_kernel<0>, grid, block, 0, s, X, X, X, X, 0.f, 0.f, 0.f, O, t_out, table,
                                 counter, stages, stage, table_len, n4); break;
      case 1: hipLaunchKernelGGL(rk_stage_kernel<1>, grid, block, 0, s, X, K0, K0, K0, c1, 0.f, 0.f, O, t_out, table,
                                 counter, stages, stage, table_len, n4); break;
      case 2: hipLaunchKernelGGL(rk_stage_kernel<2>, grid, block, 0, s, X, K0, K1, K0, c1, c2, 0.f, O, t_out, table,
                                 counter, stages, stage, table_len, n4); break;
      default: hipLaunchKernelGGL(rk_stage_kernel<3>, grid, block, 0, s, X, K0, K1, K2, c1, c2, c3, O, t_out, table,
                                  counter, stages, stage, table_len, n4); break;
    }
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_rk_combine(float* x, const float* k1, const float* k2, const float* k3, const float* k4, float c1,
                              float c2, float c3, float c4, int nk, int* counter, int B, long n, void* stream) {
  if (nk < 1 || nk > 4) return S2S_ERR_SHAPE;
  const float* k[4] = {k1, k2, k3, k4};
  if (!x || !counter) return S2S_ERR_NULL;
  for (int j = 0; j < nk; ++j)
    if (!k[j]) return S2S_ERR_NULL;
  if (check_bn(B, n)) return S2S_ERR_SHAPE;
  if (misaligned(x)) return S2S_ERR_ALIGN;
  for (int j = 0; j < nk; ++j)
    if (misaligned(k[j])) return S2S_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const long n4 = n / 4;
  const dim3 grid(dp_grid_x(n4), B), block(kThreads);
  f32x4* X = (f32x4*)x;
  const f32x4 *K0 = (const f32x4*)k1, *K1 = (const f32x4*)k2, *K2 = (const f32x4*)k3, *K3 = (const f32x4*)k4;
  switch (nk) {
    case 1: hipLaunchKernelGGL(rk_combine_kernel<1>, grid, block, 0, s, X, K0, K0, K0, K0, c1, 0.f, 0.f, 0.f, counter,
                               n4); break;
    case 2: hipLaunchKernelGGL(rk_combine_kernel<2>, grid, block, 0, s, X, K0, K1, K0, K0, c1, c2, 0.f, 0.f, counter,
                               n4); break;
    case 3: hipLaunchKernelGGL(rk_combine_kernel<3>, grid, block, 0, s, X, K0, K1, K2, K0, c1, c2, c3, 0.f, counter,
                               n4); break;
    default: hipLaunchKernelGGL(rk_combine_kernel<4>, grid, block, 0, s, X, K0, K1, K2, K3, c1, c2, c3, c4, counter,
                                n4); break;
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
