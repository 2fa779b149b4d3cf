// Hysteresis (double) thresholding: the dual-threshold byte mask and its counts.  DESIGN.md section 3.37.
//
//   s2s_hyst_mask      t int16 on the 1/1024 OD grid + the tissue byte -> one byte per pixel: bit 0 = tissue and
//                      t >= j_low (weak: the mask that is labelled), bit 1 = tissue, bit 2 = tissue and t >= j_high
//                      (strong: the marker); per-owner int64 counts of tissue, weak and strong pixels
//   s2s_hyst_finalize  burden = positive / max(tissue, 1) as a double, from device integers
//
// The selection itself (the weak components that hold a strong pixel) is s2s_objects_label_seeded of objects.hip on this
// byte with fg_bits = 1 and seed_bits = 4.  One pass over 3 bytes a pixel in, 1 byte out; the counts accumulate in
// registers and leave a workgroup as three 64-bit integer atomics, so they are exact in any order.  Nothing here
// allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int HY_MAX_SIDE = 32767;
constexpr int HY_MAX_B = 65535;
constexpr int HY_NB = 4096;

struct HyMask {
  const short* t;               // [B][rows][W]
  const unsigned char* tissue;  // the same, or null: every pixel is tissue
  int rows, W;                  // rows the buffers hold per sample
  int row0, nrows;              // the rows that are written and counted (the others are a band's halo)
  int spo;                      // samples per owner: 1, or B when pooled
  int j_low, j_high;
  unsigned char* mask;          // [B][nrows][W] with out_img elements per sample
  long out_img;
};

__global__ __launch_bounds__(256) void hy_zero_kernel(unsigned long long* __restrict__ counts, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) counts[i] = 0ull;
}

__device__ __forceinline__ unsigned long long hy_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// grid = (workgroups per owner, owners).  A workgroup counts fewer than 2^32 pixels (hy_blocks).
__global__ __launch_bounds__(256) void hy_mask_kernel(const HyMask p, unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long red[4][3];
  const int tid = threadIdx.x, owner = blockIdx.y;
  const long per = (long)p.nrows * p.W, total = per * p.spo;
  unsigned nt = 0, nw = 0, ns = 0;
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const long s = q / per, r = q - s * per;
    const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
    const long n = (long)owner * p.spo + s;
    const long i = (n * p.rows + p.row0 + y) * p.W + x;
    const int t = p.t[i];
    const bool tis = p.tissue ? p.tissue[i] != 0 : true;
    const bool weak = tis && t >= p.j_low, strong = tis && t >= p.j_high;
    p.mask[n * p.out_img + r] = (unsigned char)((weak ? 1 : 0) | (tis ? 2 : 0) | (strong ? 4 : 0));
    nt += tis ? 1u : 0u;
    nw += weak ? 1u : 0u;
    ns += strong ? 1u : 0u;
  }
  const unsigned long long v[3] = {hy_wave_sum(nt), hy_wave_sum(nw), hy_wave_sum(ns)};
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) red[tid >> 6][c] = v[c];
  }
  __syncthreads();
  if (tid < 3) {
    const unsigned long long s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (s) atomicAdd(counts + (long)owner * 3 + tid, s);
  }
}

__global__ __launch_bounds__(256) void hy_finalize_kernel(const long long* __restrict__ positive,
                                                          const long long* __restrict__ counts, long owners,
                                                          double* __restrict__ burden) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= owners) return;
  burden[o] = (double)positive[o] / (double)max(counts[3 * o], 1LL);
}

// workgroups per owner: 16 pixels a thread, at most 2048 workgroups in all; 0 when one would count 2^32 pixels or more
unsigned hy_blocks(long total, int owners) {
  long cap = 2048 / owners;
  if (cap < 1) cap = 1;
  long blocks = (total + 256L * 16 - 1) / (256L * 16);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (total + blocks - 1) / blocks >= (1L << 32) ? 0u : (unsigned)blocks;
}

}  // namespace

extern "C" int s2s_hyst_mask(const short* t, const void* tissue, int B, int rows, int W, int row0, int nrows, int j_low,
                             int j_high, int pool, int reset, long* counts, void* mask, long out_img, void* stream) {
  if (!t || !counts || !mask) return S2S_ERR_NULL;
  if (B < 1 || B > HY_MAX_B || rows < 1 || W < 1 || rows > HY_MAX_SIDE || W > HY_MAX_SIDE || row0 < 0 || nrows < 1 ||
      (long)row0 + nrows > rows || j_low < 0 || j_high > HY_NB - 1 || j_low > j_high)
    return S2S_ERR_SHAPE;
  if (B > 1 && out_img < (long)nrows * W) return S2S_ERR_SHAPE;
  const int owners = pool ? 1 : B;
  const unsigned blocks = hy_blocks((long)(pool ? B : 1) * nrows * W, owners);
  if (!blocks) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(unsigned long long), "int64 counts");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* c = (unsigned long long*)counts;
  if (reset) {
    hipLaunchKernelGGL(hy_zero_kernel, dim3((unsigned)cdiv(3 * owners, 256)), dim3(256), 0, s, c, 3L * owners);
    S2S_LAUNCH_CHECK();
  }
  HyMask p;
  p.t = t;
  p.tissue = reinterpret_cast<const unsigned char*>(tissue);
  p.rows = rows;
  p.W = W;
  p.row0 = row0;
  p.nrows = nrows;
  p.spo = pool ? B : 1;
  p.j_low = j_low;
  p.j_high = j_high;
  p.mask = reinterpret_cast<unsigned char*>(mask);
  p.out_img = out_img;
  hipLaunchKernelGGL(hy_mask_kernel, dim3(blocks, (unsigned)owners), dim3(256), 0, s, p, c);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_hyst_finalize(const long* positive, const long* counts, long owners, double* burden, void* stream) {
  if (!positive || !counts || !burden) return S2S_ERR_NULL;
  if (owners < 1 || owners > HY_MAX_B) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(hy_finalize_kernel, dim3((unsigned)((owners + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)positive, (const long long*)counts, owners, burden);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
