// Mask morphology and boundary metrics on an exact Euclidean distance transform of a byte mask.  DESIGN.md section 3.24.
//
//   s2s_morph_words               int32 words of scratch the distance entry points need
//   s2s_morph_edt                 mask [B][H][W] bytes (any row pitch) -> int32 squared distance to the nearest site
//                                 (background or foreground pixels), FAR = 2^31 - 1 where a sample has no site
//   s2s_morph_threshold           the same transform, stored as the byte D_fg <= r2 (dilate) or D_bg > r2 (erode)
//   s2s_morph_boundary            the boundary bytes: foreground with a 4-neighbour that is background or outside
//   s2s_morph_fill_holes(_words)  m | (background components that touch no border line), by s2s_objects_label
//   s2s_morph_boundary_agreement  two masks -> per-sample integer accumulators over the pooled boundary distances
//   s2s_morph_boundary_finalize   accumulators -> max_d2, pq_d2, sum_q8, within, counts, valid and the fp64 values
//
// Passes of one distance transform (each a launch of its own on the caller's stream, none waits for another workgroup):
//   bits    one thread per column and segment of MO_SEG = 64 rows: the sites of the segment as one 64-bit word.  The
//           threads of a wave run along x, so every row is one coalesced load.  The boundary flavour evaluates the
//           boundary rule on the mask bytes in this load; the boundary is never written out.
//   carry   one thread per column walks the segments down, then up: the row of the nearest site before / after each
//           segment (-1: none).  H / 64 steps instead of H.
//   column  one thread per column and segment: g[y][x] = vertical distance to the nearest site of column x, from the
//           segment's bits (count-leading / trailing-zeros instead of a scan) and its two carries; uint16, 65535 = none
//   row     D[y][x] = min over x' of (x - x')^2 + g[y][x']^2.  The row of g is staged in LDS; one thread per pixel
//           searches outward d = 0, 1, 2, ... on both sides and stops once d^2 >= the best so far (a candidate at offset
//           d costs at least d^2, so nothing better can follow) or d^2 > the caller's bound.  The loop is bounded by W.
//           Rows of at most MO_PACK / 2 pixels are packed, MO_PACK / W of them per workgroup.  The kernel is a template
//           on its epilogue: int32 D, the thresholded byte, or the agreement list.
// Agreement: per direction (sites = the boundary of one mask) the row pass runs at the pixels of the OTHER mask's boundary
// only and appends their D to a per-sample list (one atomic per wave to reserve places; the order in the list is
// irrelevant, every consumer is a multiset function).  Then a radix select of the k-th smallest on the 31-bit values:
// 11 + 10 + 10 bits, LDS-privatised histograms over the list, a one-workgroup kernel per sample between the passes that
// picks the bin; k = (q n + 99) / 100 is computed on the device from the list lengths.  The first histogram pass also
// takes max, sum of isqrt(65536 s) and #{s <= tol2} (per-wave reductions, then integer atomics).
//
// All sums are integers, so atomics in any order give the same bits.  Every word a pass reads was written by an earlier
// pass of the same call (the scratch holds the previous call's contents).  Nothing allocates, synchronises or reads back.
#include <limits.h>

#include "common.h"

extern "C" long s2s_objects_words(int B, int H, int W);
extern "C" int s2s_objects_label(const void* mask, long pitch, long img_stride, int fg_bits, int B, int H, int W,
                                 int connectivity, int min_area, int max_objects, int* scratch, int* labels, int* count,
                                 long* kept_pixels, int* largest, long* size_hist, int* tab_area, int* tab_bbox,
                                 long* tab_sums, void* stream);

namespace {

constexpr int MO_SEG = 64;            // rows per segment of the column pass (morphology.SEGMENT): one bit per row
constexpr int MO_MAX_SIDE = 32767;    // H^2 + W^2 < 2^31
constexpr int MO_FAR = INT_MAX;
constexpr int MO_NONE = 65535;        // g: no site in this column
constexpr int MO_PACK = 1024;         // pixels per workgroup of the row pass when rows are packed
constexpr int MO_ACC = 16;            // int32 words of accumulators per sample
constexpr int MO_BINS = 2048;         // histogram bins per sample (the widest digit has 11 bits)
// accumulator words: 0 |dP| (list 0), 1 |dT| (list 1), 2 max, 3 radix prefix, 4-5 sum_q8, 6-7 within, 8-9 remaining k, 10 pq
enum { ACC_NP = 0, ACC_NT = 1, ACC_MAX = 2, ACC_PREFIX = 3, ACC_SUM = 4, ACC_WITHIN = 6, ACC_K = 8, ACC_PQ = 10 };

enum { SITE_BG = 0, SITE_FG = 1, SITE_BOUNDARY = 2 };
enum { EP_D = 0, EP_LE = 1, EP_GT = 2, EP_AGREE = 3 };

struct MoMask {
  const unsigned char* m;
  long pitch, img;
  int H, W;
};
// nothing lies outside the image: a pixel out of range is neither foreground nor background
__device__ __forceinline__ bool mo_fg(const MoMask& k, int n, int y, int x) {
  if ((unsigned)y >= (unsigned)k.H || (unsigned)x >= (unsigned)k.W) return false;
  return k.m[(long)n * k.img + (long)y * k.pitch + x] != 0;
}
__device__ __forceinline__ bool mo_boundary(const MoMask& k, int n, int y, int x) {
  return mo_fg(k, n, y, x) && !(mo_fg(k, n, y - 1, x) && mo_fg(k, n, y + 1, x) && mo_fg(k, n, y, x - 1) && mo_fg(k, n, y, x + 1));
}
template <int SITE>
__device__ __forceinline__ bool mo_site(const MoMask& k, int n, int y, int x) {          // (y, x) inside the image
  if (SITE == SITE_BOUNDARY) return mo_boundary(k, n, y, x);
  return mo_fg(k, n, y, x) == (SITE == SITE_FG);
}

// ---- column pass -----------------------------------------------------------------------------------------------------
// bits [B][nseg][W]
template <int SITE>
__global__ __launch_bounds__(256) void mo_bits_kernel(const MoMask k, int nseg, unsigned long long* __restrict__ bits) {
  const int x = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, n = blockIdx.z;
  if (x >= k.W) return;
  const int y0 = s * MO_SEG, rows = min(MO_SEG, k.H - y0);
  unsigned long long b = 0;
  for (int r = 0; r < rows; ++r)
    if (mo_site<SITE>(k, n, y0 + r, x)) b |= 1ull << r;
  bits[((long)n * nseg + s) * k.W + x] = b;
}

// above / below [B][nseg][W]: the row of the nearest site before the segment's first row / after its last row, -1: none
__global__ __launch_bounds__(256) void mo_carry_kernel(const unsigned long long* __restrict__ bits, int nseg, int W,
                                                       int* __restrict__ above, int* __restrict__ below) {
  const int x = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (x >= W) return;
  const long base = (long)n * nseg * W + x;
  int run = -1;
  for (int s = 0; s < nseg; ++s) {
    const unsigned long long b = bits[base + (long)s * W];
    above[base + (long)s * W] = run;
    if (b) run = s * MO_SEG + 63 - __clzll((long long)b);
  }
  run = -1;
  for (int s = nseg - 1; s >= 0; --s) {
    const unsigned long long b = bits[base + (long)s * W];
    below[base + (long)s * W] = run;
    if (b) run = s * MO_SEG + __ffsll((long long)b) - 1;
  }
}

// g [B][H][W] uint16
__global__ __launch_bounds__(256) void mo_column_kernel(const unsigned long long* __restrict__ bits,
                                                        const int* __restrict__ above, const int* __restrict__ below,
                                                        int nseg, int H, int W, unsigned short* __restrict__ g) {
  const int x = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y, n = blockIdx.z;
  if (x >= W) return;
  const long c = ((long)n * nseg + s) * W + x;
  const unsigned long long b = bits[c];
  const int up0 = above[c], dn0 = below[c];
  const int y0 = s * MO_SEG, rows = min(MO_SEG, H - y0);
  unsigned short* out = g + ((long)n * H + y0) * W + x;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    const unsigned long long lo = r == 63 ? b : b & ((2ull << r) - 1ull), hi = b >> r;
    const int up = lo ? y0 + 63 - __clzll((long long)lo) : up0;
    const int dn = hi ? y + __ffsll((long long)hi) - 1 : dn0;
    int d = MO_NONE;
    if (up >= 0) d = y - up;
    if (dn >= 0) d = min(d, dn - y);
    out[(long)r * W] = (unsigned short)d;
  }
}

// ---- row pass --------------------------------------------------------------------------------------------------------
struct MoEp {
  int* d;                 // EP_D: [B][H][W]
  unsigned char* bytes;   // EP_LE / EP_GT: [B][H][W]
  int r2;
  MoMask other;           // EP_AGREE: the mask whose boundary pixels are sampled
  int* count;             //           its list length (one int of the sample's accumulators; stride MO_ACC)
  int* list;              //           [B][2][hw], this direction's half selected by the caller
  long list_stride;       //           2 hw
};

__device__ __forceinline__ int mo_search(const unsigned short* row, int x, int W, int bound) {
  const int gv = row[x];
  int best = gv == MO_NONE ? MO_FAR : gv * gv;
  const int dmax = max(x, W - 1 - x);
  for (int d = 1; d <= dmax; ++d) {
    const int d2 = d * d;
    if (d2 >= best || d2 > bound) break;
    if (x - d >= 0) {
      const int gl = row[x - d];
      if (gl != MO_NONE) best = min(best, d2 + gl * gl);
    }
    if (x + d < W) {
      const int gr = row[x + d];
      if (gr != MO_NONE) best = min(best, d2 + gr * gr);
    }
  }
  return best > bound ? MO_FAR : best;
}

// R rows per workgroup; dynamic LDS = R * W uint16
template <int EP>
__global__ __launch_bounds__(256) void mo_row_kernel(const unsigned short* __restrict__ g, int H, int W, int R, int bound,
                                                     const MoEp e) {
  extern __shared__ unsigned short sg[];
  const int n = blockIdx.y, y0 = blockIdx.x * R;
  const int total = min(R, H - y0) * W;                       // R * W <= max(MO_PACK, W): no overflow
  const long o = ((long)n * H + y0) * W;
  for (int i = threadIdx.x; i < total; i += 256) sg[i] = g[o + i];
  __syncthreads();
  for (int base = 0; base < total; base += 256) {             // wave-uniform trip count (the ballot below)
    const int i = base + threadIdx.x;
    const bool in = i < total;
    const int r = in ? i / W : 0, x = in ? i - r * W : 0;
    if (EP == EP_AGREE) {
      const bool take = in && mo_boundary(e.other, n, y0 + r, x);
      const int v = take ? mo_search(sg + r * W, x, W, bound) : 0;
      const unsigned long long mask = __ballot(take);
      if (mask) {
        const int lane = threadIdx.x & 63, leader = __ffsll((long long)mask) - 1;
        int at = 0;
        if (lane == leader) at = atomicAdd(e.count + (long)n * MO_ACC, __popcll(mask));
        at = __shfl(at, leader, 64);
        if (take) e.list[(long)n * e.list_stride + at + __popcll(mask & ((1ull << lane) - 1ull))] = v;
      }
    } else if (in) {
      const int v = mo_search(sg + r * W, x, W, bound);
      if (EP == EP_D) e.d[o + i] = v;
      if (EP == EP_LE) e.bytes[o + i] = v <= e.r2 ? 1 : 0;
      if (EP == EP_GT) e.bytes[o + i] = v > e.r2 ? 1 : 0;
    }
  }
}

// ---- small byte kernels ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mo_fill_kernel(int* __restrict__ p, long nwords) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < nwords) p[i] = 0;
}

// mode 0: the boundary bytes; mode 1: the inverted mask
__global__ __launch_bounds__(256) void mo_bytes_kernel(const MoMask k, int mode, unsigned char* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  if (x >= k.W) return;
  for (int y = blockIdx.y; y < k.H; y += gridDim.y)
    out[((long)n * k.H + y) * k.W + x] = (mode == 0 ? mo_boundary(k, n, y, x) : !mo_fg(k, n, y, x)) ? 1 : 0;
}

// ---- agreement: radix select and sums over the lists -------------------------------------------------------------------
// floor(sqrt(v)) for 0 <= v < 2^47
__device__ __forceinline__ long long mo_isqrt(long long v) {
  long long r = (long long)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// grid (blocks, 2 lists, B); pass 0: digit bits 30..20 and the sums, pass 1: bits 19..10, pass 2: bits 9..0
__global__ __launch_bounds__(256) void mo_hist_kernel(const int* __restrict__ list, long hw, int* acc, unsigned* hist,
                                                      int pass, int tol2) {
  __shared__ unsigned sh[MO_BINS];
  const int n = blockIdx.z, dir = blockIdx.y;
  int* a = acc + (long)n * MO_ACC;
  const int cnt = a[dir];
  if ((long)blockIdx.x * 256 >= cnt) return;                  // (the whole workgroup leaves)
  for (int j = threadIdx.x; j < MO_BINS; j += 256) sh[j] = 0;
  __syncthreads();
  const int prefix = a[ACC_PREFIX];
  const int* v = list + ((long)n * 2 + dir) * hw;
  int mx = 0;
  unsigned long long sum = 0, within = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (long)gridDim.x * 256) {
    const int s = v[i];
    if (pass == 0) {
      atomicAdd(&sh[s >> 20], 1u);
      mx = max(mx, s);
      sum += (unsigned long long)mo_isqrt(65536LL * s);
      within += s <= tol2 ? 1 : 0;
    } else if (pass == 1) {
      if ((s >> 20) == prefix) atomicAdd(&sh[(s >> 10) & 1023], 1u);
    } else {
      if ((s >> 10) == prefix) atomicAdd(&sh[s & 1023], 1u);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < MO_BINS; j += 256)
    if (sh[j]) atomicAdd(hist + (long)n * MO_BINS + j, sh[j]);
  if (pass == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mx = max(mx, __shfl_xor(mx, o, 64));
      sum += __shfl_xor(sum, o, 64);
      within += __shfl_xor(within, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMax(a + ACC_MAX, mx);
      atomicAdd((unsigned long long*)(a + ACC_SUM), sum);
      atomicAdd((unsigned long long*)(a + ACC_WITHIN), within);
    }
  }
}

// one workgroup per sample: the bin that holds the k-th smallest; the histogram is zeroed for the next pass
__global__ __launch_bounds__(256) void mo_pick_kernel(int* acc, unsigned* hist, int pass, int q) {
  __shared__ long long part[256];
  __shared__ int s_bin;
  __shared__ long long s_before;
  int* a = acc + (long)blockIdx.x * MO_ACC;
  unsigned* h = hist + (long)blockIdx.x * MO_BINS;
  const int tid = threadIdx.x;
  long long k = pass == 0 ? ((long long)q * ((long long)a[ACC_NP] + a[ACC_NT]) + 99) / 100 : *(long long*)(a + ACC_K);
  const int prefix = a[ACC_PREFIX];
  if (k < 1) k = 1;
  long long c[8], sum = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    c[j] = h[tid * 8 + j];
    sum += c[j];
    h[tid * 8 + j] = 0;
  }
  part[tid] = sum;
  if (tid == 0) s_bin = -1;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const long long u = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += u;
    __syncthreads();
  }
  long long before = part[tid] - sum;
  if (before < k && k <= part[tid]) {                          // exactly one thread when 1 <= k <= the total
    int j = 0;
    while (before + c[j] < k) before += c[j++];
    s_bin = tid * 8 + j;
    s_before = before;
  }
  __syncthreads();
  if (tid == 0) {
    const int bin = s_bin < 0 ? 0 : s_bin;                     // (an empty list: the finalize kernel overrides the result)
    *(long long*)(a + ACC_K) = s_bin < 0 ? 1 : k - s_before;
    if (pass == 0) a[ACC_PREFIX] = bin;
    if (pass == 1) a[ACC_PREFIX] = (prefix << 10) | bin;
    if (pass == 2) a[ACC_PQ] = (prefix << 10) | bin;
  }
}

struct MoResult {
  int *max_d2, *pq_d2, *valid;
  long long *sum_q8, *within, *n_pred, *n_target;
  double *hausdorff, *hd, *assd, *surface_dice;
};

__global__ void mo_finalize_kernel(const int* __restrict__ acc, int B, int H, int W, const MoResult r) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const int* a = acc + (long)n * MO_ACC;
  const long long np = a[ACC_NP], nt = a[ACC_NT], cnt = np + nt;
  int mx = a[ACC_MAX], pq = a[ACC_PQ], valid = 1;
  long long sum = *(const long long*)(a + ACC_SUM), within = *(const long long*)(a + ACC_WITHIN);
  if (np == 0 || nt == 0) {
    valid = 0;
    within = 0;
    mx = pq = cnt ? (H - 1) * (H - 1) + (W - 1) * (W - 1) : 0;
    sum = cnt * mo_isqrt(65536LL * mx);
  }
  r.max_d2[n] = mx;
  r.pq_d2[n] = pq;
  r.valid[n] = valid;
  r.sum_q8[n] = sum;
  r.within[n] = within;
  r.n_pred[n] = np;
  r.n_target[n] = nt;
  r.hausdorff[n] = sqrt((double)mx);
  r.hd[n] = sqrt((double)pq);
  r.assd[n] = cnt ? (double)sum / (double)(256 * cnt) : 0.0;
  r.surface_dice[n] = cnt ? (double)within / (double)cnt : 1.0;
}

// ---- hole filling ----------------------------------------------------------------------------------------------------
// flags [B][fw] words, one bit per label of the inverted mask met on the first or last row or column
__global__ __launch_bounds__(256) void mo_border_kernel(const int* __restrict__ labels, int H, int W, long fw,
                                                        unsigned* flags) {
  const int t = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  int y, x;
  if (t < W) { y = 0; x = t; }
  else if (t < 2 * W) { y = H - 1; x = t - W; }
  else if (t < 2 * W + H) { y = t - 2 * W; x = 0; }
  else if (t < 2 * W + 2 * H) { y = t - 2 * W - H; x = W - 1; }
  else return;
  const int lab = labels[((long)n * H + y) * W + x];
  if (lab <= 0 || (lab >> 5) >= fw) return;
  unsigned* f = flags + (long)n * fw + (lab >> 5);
  const unsigned bit = 1u << (lab & 31);
  if (!(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(f, bit);
}

__global__ __launch_bounds__(256) void mo_holes_kernel(const MoMask k, const int* __restrict__ labels, long fw,
                                                       const unsigned* __restrict__ flags, unsigned char* __restrict__ out) {
  const int x = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  if (x >= k.W) return;
  for (int y = blockIdx.y; y < k.H; y += gridDim.y) {
    const long i = ((long)n * k.H + y) * k.W + x;
    bool on = mo_fg(k, n, y, x);
    if (!on) {
      const int lab = labels[i];
      on = lab > 0 && (lab >> 5) < fw && !((flags[(long)n * fw + (lab >> 5)] >> (lab & 31)) & 1u);
    }
    out[i] = on ? 1 : 0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
bool mo_shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= MO_MAX_SIDE && W <= MO_MAX_SIDE;
}
bool mo_mask_ok(long pitch, long img, int B, int H, int W) { return pitch >= W && (B == 1 || img >= pitch * (long)H); }

struct MoLayout {
  long acc, hist, bits, above, below, g, list, total;      // offsets in int32 words
};
MoLayout mo_layout(int B, int H, int W, bool agreement) {
  const long hw = (long)H * W, cols = (long)B * cdiv(H, MO_SEG) * W;
  MoLayout L;
  long off = 0;
  L.acc = off;
  L.hist = off + (long)B * MO_ACC;
  if (agreement) off += (long)B * (MO_ACC + MO_BINS);       // (even: the 64-bit words below stay aligned)
  L.bits = off; off += 2 * cols;
  L.above = off; off += cols;
  L.below = off; off += cols;
  L.g = off; off += ((long)B * hw + 1) / 2;
  L.list = off;
  if (agreement) off += 2 * (long)B * hw;
  L.total = off;
  return L;
}
long mo_flag_words(long hw) { return (hw / 2 + 2 + 31) / 32; }

dim3 mo_rows_grid(int B, int H, int W) { return dim3((unsigned)cdiv(W, 256), (unsigned)(H < 1024 ? H : 1024), (unsigned)B); }

// the three column launches and the row launch of one transform
template <int SITE, int EP>
void mo_transform(const MoMask& k, int B, int bound, int* scratch, const MoLayout& L, const MoEp& e, hipStream_t s) {
  const int H = k.H, W = k.W, nseg = cdiv(H, MO_SEG), xb = cdiv(W, 256);
  unsigned long long* bits = (unsigned long long*)(scratch + L.bits);
  int *above = scratch + L.above, *below = scratch + L.below;
  unsigned short* g = (unsigned short*)(scratch + L.g);
  hipLaunchKernelGGL(mo_bits_kernel<SITE>, dim3(xb, nseg, B), dim3(256), 0, s, k, nseg, bits);
  hipLaunchKernelGGL(mo_carry_kernel, dim3(xb, B), dim3(256), 0, s, bits, nseg, W, above, below);
  hipLaunchKernelGGL(mo_column_kernel, dim3(xb, nseg, B), dim3(256), 0, s, bits, above, below, nseg, H, W, g);
  const int R = W >= MO_PACK ? 1 : MO_PACK / W;
  hipLaunchKernelGGL(mo_row_kernel<EP>, dim3(cdiv(H, R), B), dim3(256), (size_t)R * W * sizeof(unsigned short), s, g, H, W,
                     R, bound, e);
}

}  // namespace

extern "C" long s2s_morph_words(int B, int H, int W, int agreement) {
  if (!mo_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  return mo_layout(B, H, W, agreement != 0).total;
}

extern "C" int s2s_morph_edt(const void* mask, long pitch, long img_stride, int B, int H, int W, int to_foreground,
                             int max_d2, int* scratch, int* out, void* stream) {
  if (!mask || !scratch || !out) return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W) || !mo_mask_ok(pitch, img_stride, B, H, W) || max_d2 < 0 || (to_foreground & ~1))
    return S2S_ERR_SHAPE;
  const MoMask k{(const unsigned char*)mask, pitch, img_stride, H, W};
  const MoLayout L = mo_layout(B, H, W, false);
  MoEp e{};
  e.d = out;
  if (to_foreground) mo_transform<SITE_FG, EP_D>(k, B, max_d2, scratch, L, e, (hipStream_t)stream);
  else mo_transform<SITE_BG, EP_D>(k, B, max_d2, scratch, L, e, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_morph_threshold(const void* mask, long pitch, long img_stride, int B, int H, int W, int erode, int r2,
                                   int* scratch, void* out, void* stream) {
  if (!mask || !scratch || !out) return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W) || !mo_mask_ok(pitch, img_stride, B, H, W) || r2 < 0 || r2 == MO_FAR || (erode & ~1))
    return S2S_ERR_SHAPE;
  const MoMask k{(const unsigned char*)mask, pitch, img_stride, H, W};
  const MoLayout L = mo_layout(B, H, W, false);
  MoEp e{};
  e.bytes = (unsigned char*)out;
  e.r2 = r2;
  // the search may stop at r2: whatever lies beyond is reported as FAR, which is on the same side of the threshold
  if (erode) mo_transform<SITE_BG, EP_GT>(k, B, r2, scratch, L, e, (hipStream_t)stream);
  else mo_transform<SITE_FG, EP_LE>(k, B, r2, scratch, L, e, (hipStream_t)stream);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_morph_boundary(const void* mask, long pitch, long img_stride, int B, int H, int W, void* out,
                                  void* stream) {
  if (!mask || !out) return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W) || !mo_mask_ok(pitch, img_stride, B, H, W)) return S2S_ERR_SHAPE;
  const MoMask k{(const unsigned char*)mask, pitch, img_stride, H, W};
  hipLaunchKernelGGL(mo_bytes_kernel, mo_rows_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, k, 0, (unsigned char*)out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" long s2s_morph_fill_holes_words(int B, int H, int W) {
  if (!mo_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  const long hw = (long)H * W;
  // statistics of the labelling (kept 2, histogram 64, count 1, largest 1 words per sample), flags, labels, the inverted
  // mask, the labelling's own scratch
  return (long)B * 68 + (long)B * mo_flag_words(hw) + (long)B * hw + ((long)B * hw + 3) / 4 + s2s_objects_words(B, H, W);
}

extern "C" int s2s_morph_fill_holes(const void* mask, long pitch, long img_stride, int B, int H, int W, int connectivity,
                                    int* scratch, void* out, void* stream) {
  if (!mask || !scratch || !out) return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W) || !mo_mask_ok(pitch, img_stride, B, H, W) || (connectivity != 4 && connectivity != 8))
    return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W, fw = mo_flag_words(hw);
  const MoMask k{(const unsigned char*)mask, pitch, img_stride, H, W};
  long* kept = (long*)scratch;                                  // [B]
  long* hist = kept + B;                                        // [B][32]
  int* count = scratch + (long)B * 66;
  int* largest = count + B;
  unsigned* flags = (unsigned*)(scratch + (long)B * 68);
  int* labels = scratch + (long)B * 68 + (long)B * fw;
  unsigned char* inv = (unsigned char*)(labels + (long)B * hw);
  int* obj = labels + (long)B * hw + ((long)B * hw + 3) / 4;
  const long zero = (long)B * 68 + (long)B * fw;
  hipLaunchKernelGGL(mo_fill_kernel, dim3((unsigned)((zero + 255) / 256)), dim3(256), 0, s, scratch, zero);
  hipLaunchKernelGGL(mo_bytes_kernel, mo_rows_grid(B, H, W), dim3(256), 0, s, k, 1, inv);
  const int rc = s2s_objects_label(inv, W, hw, 255, B, H, W, connectivity, 1, 0, obj, labels, count, kept, largest, hist,
                                   nullptr, nullptr, nullptr, stream);
  if (rc != S2S_OK) return rc;
  hipLaunchKernelGGL(mo_border_kernel, dim3((unsigned)cdiv(2 * W + 2 * H, 256), (unsigned)B), dim3(256), 0, s, labels, H, W,
                     fw, flags);
  hipLaunchKernelGGL(mo_holes_kernel, mo_rows_grid(B, H, W), dim3(256), 0, s, k, labels, fw, flags, (unsigned char*)out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_morph_boundary_agreement(const void* pred, long pred_pitch, long pred_img, const void* target,
                                            long target_pitch, long target_img, int B, int H, int W, int tol2,
                                            int percentile, int* scratch, void* stream) {
  if (!pred || !target || !scratch) return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W) || !mo_mask_ok(pred_pitch, pred_img, B, H, W) || !mo_mask_ok(target_pitch, target_img, B, H, W) ||
      tol2 < 0 || percentile < 1 || percentile > 100)
    return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  const MoMask p{(const unsigned char*)pred, pred_pitch, pred_img, H, W};
  const MoMask t{(const unsigned char*)target, target_pitch, target_img, H, W};
  const MoLayout L = mo_layout(B, H, W, true);
  int* acc = scratch + L.acc;
  unsigned* hist = (unsigned*)(scratch + L.hist);
  int* list = scratch + L.list;
  const long zero = (long)B * (MO_ACC + MO_BINS);
  hipLaunchKernelGGL(mo_fill_kernel, dim3((unsigned)((zero + 255) / 256)), dim3(256), 0, s, scratch, zero);
  MoEp e{};
  e.list_stride = 2 * hw;
  // list 0: from every pixel of the prediction's boundary to the target's; list 1: the other way round
  e.other = p; e.count = acc + ACC_NP; e.list = list;
  mo_transform<SITE_BOUNDARY, EP_AGREE>(t, B, MO_FAR, scratch, L, e, s);
  e.other = t; e.count = acc + ACC_NT; e.list = list + hw;
  mo_transform<SITE_BOUNDARY, EP_AGREE>(p, B, MO_FAR, scratch, L, e, s);
  const long want = (hw + 1023) / 1024;
  const dim3 hg((unsigned)(want < 256 ? want : 256), 2, (unsigned)B);
  for (int pass = 0; pass < 3; ++pass) {
    hipLaunchKernelGGL(mo_hist_kernel, hg, dim3(256), 0, s, list, hw, acc, hist, pass, tol2);
    hipLaunchKernelGGL(mo_pick_kernel, dim3((unsigned)B), dim3(256), 0, s, acc, hist, pass, percentile);
  }
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_morph_boundary_finalize(const int* scratch, int B, int H, int W, int* max_d2, int* pq_d2, long* sum_q8,
                                           long* within, long* boundary_pred, long* boundary_target, int* valid,
                                           double* hausdorff, double* hd, double* assd, double* surface_dice,
                                           void* stream) {
  if (!scratch || !max_d2 || !pq_d2 || !sum_q8 || !within || !boundary_pred || !boundary_target || !valid || !hausdorff ||
      !hd || !assd || !surface_dice)
    return S2S_ERR_NULL;
  if (!mo_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  const MoResult r{max_d2, pq_d2, valid, (long long*)sum_q8, (long long*)within, (long long*)boundary_pred,
                   (long long*)boundary_target, hausdorff, hd, assd, surface_dice};
  hipLaunchKernelGGL(mo_finalize_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, scratch, B, H, W, r);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
