// Stain object analysis: connected-component labelling of a byte mask, a minimum-area filter, raster-order numbering and
// per-object measurements, all on the GPU.  DESIGN.md section 3.19.
//
//   s2s_objects_words     int32 words of scratch a call needs
//   s2s_objects_label     mask [B][H][W] bytes (any row pitch), foreground = (byte & fg_bits) != 0, connectivity 4 or 8
//                         -> labels int32 [B][H][W] (0 = background or dropped, 1..count in raster order of each object's
//                         first pixel, the numbering of scipy.ndimage.label), per-sample count, kept pixels, largest area
//                         and a log2 size histogram, and optionally a table (area, bounding box, coordinate sums) of the
//                         objects numbered <= max_objects
//   s2s_objects_label_seeded  the same, of the components selected by what they contain: a component is kept iff
//                         (marked foreground pixels >= min_seed) != invert (binary reconstruction, hysteresis: DESIGN.md
//                         3.37).  Three more passes between flatten and the numbering stage, the parent array as the
//                         per-root counter: zero, seed (parent[root] += marked pixels, one atomic per wave and distinct
//                         root), gate (labels = -1 on the components not selected, the selected mask, the root counts)
//   s2s_objects_centroid  the table's coordinate sums -> fp32 centroids; rows at or beyond count are zeroed
//   s2s_objects_hits      two label images -> how many objects of each touch an object of the other
//   s2s_objects_scores    counts and hits -> recall, precision, F1, |count difference|
//   s2s_objects_density   kept pixels, tissue pixels, count -> burden and objects per square millimetre of tissue
//
// Passes of s2s_objects_label (every one a launch of its own on the caller's stream; no pass waits for another
// workgroup, so scheduling cannot hang any of them):
//   local    one workgroup labels a 32 x 64 tile in LDS: row runs by ballot, unions between rows by LDS atomicMin;
//            parent[i] = sample-wide raster index of the tile-local root, -1 for background
//   merge    one thread per pixel on a tile seam unites across it (lock-free union by minimum); EVERY access to parent in
//            this kernel is an agent-scope atomic: the XCDs' L2s are private and a plain load may see a stale line
//   flatten  labels[i] = root(i); parent is only read
//   zero     parent[root] = 0: from here on the parent array holds areas, then numbers, at the roots' places
//   area     parent[root] += pixels, one integer atomic per wave and distinct root
//   count    kept roots (area >= min_area) per chunk of 1024 raster indices
//   scan     exclusive scan of the chunk counts per sample (one workgroup per sample), count[n] = total
//   number   kept root -> chunk offset + rank in chunk + 1; dropped root -> 0; the per-sample statistics
//   relabel  labels[i] = number of its root; bounding boxes and coordinate sums, one atomic set per wave row and object
// Invariant: parent[i] <= i, and a root is the smallest raster index of its set, i.e. its component's first raster pixel:
// numbering the kept roots in raster order is numbering the objects by first pixel.  find() terminates because parents
// strictly decrease.  Everything accumulated is an integer, so atomics in any order give the same bits.
//
// The passes from zero on are the numbering stage, s2s_number_sets of objects_number.h: it takes any image of first-pixel
// raster indices, and s2s_split_label (split.hip) numbers its parts with the same launches.
//
// The scratch holds the previous call's contents: every word a pass reads was written by an earlier pass of the same call.
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include <limits.h>

#include "common.h"
#include "objects_number.h"

namespace {

constexpr int OT_H = 32, OT_W = 64;          // the local pass's tile (objects.TILE)
constexpr int OB_CHUNK = 1024;               // raster indices per numbering chunk
constexpr long OB_MAX_PIXELS = 2147483646L;  // per sample: 2^31 - 2

#define OB_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define OB_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// ---- union-find in LDS (one workgroup) -------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(int* lab, int i) {
  int p;
  while ((p = __hip_atomic_load(lab + i, OB_RLX_WG)) != i) i = p;
  return i;
}
__device__ __forceinline__ void lds_unite(int* lab, int a, int b) {
  for (;;) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(lab + b, a, OB_RLX_WG);    // the larger root goes under the smaller
    if (old == b) return;
    b = old;                                                           // b had been linked meanwhile: unite with its parent
  }
}

// ---- union-find in global memory, across workgroups: agent-scope atomics only ------------------------------------------
__device__ __forceinline__ int glb_find(int* parent, int i) {
  int p;
  while ((p = __hip_atomic_load(parent + i, OB_RLX_AGENT)) != i) i = p;
  return i;
}
__device__ __forceinline__ void glb_unite(int* parent, int a, int b) {
  for (;;) {
    a = glb_find(parent, a);
    b = glb_find(parent, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + b, a, OB_RLX_AGENT);
    if (old == b) return;
    b = old;
  }
}

struct ObMask {
  const unsigned char* m;
  long pitch, img;
  int fg;
  int H, W;
};
__device__ __forceinline__ bool ob_fg(const ObMask& k, int n, int y, int x) {
  return (k.m[(long)n * k.img + (long)y * k.pitch + x] & k.fg) != 0;
}

__global__ __launch_bounds__(256) void ob_local_kernel(const ObMask k, int tiles_x, int conn8, int* __restrict__ parent) {
  __shared__ int lab[OT_H * OT_W];
  __shared__ unsigned long long rowbits[OT_H];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int n = blockIdx.y;
  const int y0 = ty * OT_H, x0 = tx * OT_W, gx = x0 + lane;
  for (int r = wv; r < OT_H; r += 4) {
    const int gy = y0 + r;
    const bool f = gy < k.H && gx < k.W && ob_fg(k, n, gy, gx);
    const unsigned long long bits = __ballot(f);
    const unsigned long long below = ~bits & ((1ull << lane) - 1ull);        // background columns left of this lane
    const int start = below ? 64 - __clzll((long long)below) : 0;            // first column of this lane's run
    lab[r * OT_W + lane] = f ? r * OT_W + start : -1;
    if (lane == 0) rowbits[r] = bits;
  }
  __syncthreads();
  for (int r = wv; r < OT_H; r += 4) {
    if (r == 0) continue;
    const unsigned long long cur = rowbits[r], up = rowbits[r - 1];
    if (!((cur >> lane) & 1ull)) continue;
    const int i = r * OT_W + lane;
    const bool cl = lane > 0 && ((cur >> (lane - 1)) & 1ull), ul = lane > 0 && ((up >> (lane - 1)) & 1ull);
    if ((up >> lane) & 1ull) {
      // two overlapping runs meet first at a column where one of them starts: one union per pair is enough
      if (!cl || !ul) lds_unite(lab, i, i - OT_W);
    } else if (conn8) {
      if (ul && !cl) lds_unite(lab, i, i - OT_W - 1);       // with a left neighbour, that one has the run above it
      if (lane < 63 && ((up >> (lane + 1)) & 1ull)) lds_unite(lab, i, i - OT_W + 1);
    }
  }
  __syncthreads();
  int* out = parent + (long)n * k.H * k.W;
  for (int r = wv; r < OT_H; r += 4) {
    const int gy = y0 + r;
    if (gy >= k.H || gx >= k.W) continue;
    int p = lab[r * OT_W + lane];
    if (p >= 0) {
      int q;
      while ((q = lab[p]) != p) p = q;
      p = (int)((long)(y0 + (p >> 6)) * k.W + x0 + (p & 63));
    }
    out[(long)gy * k.W + gx] = p;
  }
}

// One thread per pixel of a tile's top row (first n_h threads) or left column (the next n_v), first tile row / column
// excluded.  Between them they see every adjacent pixel pair that lies in two tiles, the diagonal pairs across a tile
// corner included (a top-row pixel looks up-left and up-right whatever tile column that is in).
__global__ __launch_bounds__(256) void ob_merge_kernel(const ObMask k, long n_h, long n_v, int conn8, int* parent) {
  long t = (long)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y, H = k.H, W = k.W;
  int* par = parent + (long)n * H * W;
  if (t < n_h) {
    const int s = (int)(t / W), x = (int)(t - (long)s * W), y = (s + 1) * OT_H;
    if (!ob_fg(k, n, y, x)) return;
    const int i = (int)((long)y * W + x);
    if (ob_fg(k, n, y - 1, x)) glb_unite(par, i, i - W);
    if (conn8) {
      if (x > 0 && ob_fg(k, n, y - 1, x - 1)) glb_unite(par, i, i - W - 1);
      if (x + 1 < W && ob_fg(k, n, y - 1, x + 1)) glb_unite(par, i, i - W + 1);
    }
    return;
  }
  t -= n_h;
  if (t >= n_v) return;
  const int s = (int)(t / H), y = (int)(t - (long)s * H), x = (s + 1) * OT_W;
  if (!ob_fg(k, n, y, x)) return;
  const int i = (int)((long)y * W + x);
  if (ob_fg(k, n, y, x - 1)) glb_unite(par, i, i - 1);
  if (conn8) {
    if (y > 0 && ob_fg(k, n, y - 1, x - 1)) glb_unite(par, i, i - W - 1);
    if (y + 1 < H && ob_fg(k, n, y + 1, x - 1)) glb_unite(par, i, i + W - 1);
  }
}

__global__ __launch_bounds__(256) void ob_flatten_kernel(const int* __restrict__ parent, long hw, int* __restrict__ labels) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const int* par = parent + (long)blockIdx.y * hw;
  int p = par[i];
  if (p >= 0) {
    int q;
    while ((q = par[p]) != p) p = q;
  }
  labels[(long)blockIdx.y * hw + i] = p;
}

__global__ __launch_bounds__(256) void ob_zero_kernel(const int* __restrict__ labels, long hw, int* __restrict__ area) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long o = (long)blockIdx.y * hw + i;
  if (labels[o] == (int)i) area[o] = 0;
}

// area[root] += 1 per pixel, as one atomic per wave and distinct root: a 60 000-pixel object costs ~1 000 atomics
__global__ __launch_bounds__(256) void ob_area_kernel(const int* __restrict__ labels, long hw, int* area) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int key = i < hw ? labels[(long)blockIdx.y * hw + i] : -1;
  int* a = area + (long)blockIdx.y * hw;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {                                        // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const int lk = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == lk);
    if (lane == leader) atomicAdd(a + lk, __popcll(same));
    todo &= ~same;
  }
}

// ---- seeded selection (s2s_objects_label_seeded): between flatten and the numbering stage ------------------
struct ObSeed {
  const unsigned char* marker;   // [B][H][.], a seed iff (byte & bits) != 0 on a foreground pixel
  long pitch, img;
  int bits;
  int min_seed, invert;
  const unsigned char* mask;     // the labelled mask (for bit 1 of out)
  long mask_pitch, mask_img;
  int keep_tissue;               // out keeps bit 1 of the mask byte (the stain-mask convention)
  unsigned char* out;            // [B][H][.] or null
  long out_pitch, out_img;
  int W;
};

__global__ __launch_bounds__(256) void ob_seed_zero_kernel(int B, int* __restrict__ candidates, int* __restrict__ seeded,
                                                           long long* __restrict__ seed_pixels) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= B) return;
  candidates[n] = 0;
  seeded[n] = 0;
  seed_pixels[n] = 0;
}

constexpr int OB_SEED_PER = 8;               // pixels a thread of the seed and gate passes: a workgroup covers 2048

// seeds[root] += the marked foreground pixels, one integer atomic per wave and distinct root (as ob_area_kernel); a wave
// whose 64 pixels all hold one root keeps that count over its rounds and adds it once.  seed_pixels[n] += their number,
// one atomic per workgroup (every workgroup of a sample adds to ONE address: with 256 pixels a workgroup these atomics,
// not the traffic, were the whole cost of the pass).  seeds is zero at the roots (ob_zero_kernel).
__global__ __launch_bounds__(256) void ob_seed_kernel(const int* __restrict__ labels, long hw, const ObSeed k, int* seeds,
                                                      long long* seed_pixels) {
  __shared__ int s_n;
  const int lane = threadIdx.x & 63, n = blockIdx.y;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int* a = seeds + (long)n * hw;
  int mine = 0, held_key = -1, held = 0;                // (held_*: wave-uniform)
#pragma unroll 2
  for (int j = 0; j < OB_SEED_PER; ++j) {
    const long i = ((long)blockIdx.x * OB_SEED_PER + j) * 256 + threadIdx.x;
    int key = -1;
    if (i < hw) {
      const int r = labels[(long)n * hw + i];
      if (r >= 0) {
        const unsigned y = (unsigned)i / (unsigned)k.W, x = (unsigned)i - y * (unsigned)k.W;
        if (k.marker[(long)n * k.img + (long)y * k.pitch + x] & k.bits) key = r;
      }
    }
    unsigned long long todo = __ballot(key >= 0);
    if (lane == 0) mine += __popcll(todo);
    while (todo) {                                      // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lk = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(key == lk);
      if (lk == held_key) {
        held += __popcll(same);
      } else {
        if (held && lane == 0) atomicAdd(a + held_key, held);
        held_key = lk;
        held = __popcll(same);
      }
      todo &= ~same;
    }
  }
  if (held && lane == 0) atomicAdd(a + held_key, held);
  if (lane == 0 && mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd((unsigned long long*)seed_pixels + n, (unsigned long long)s_n);
}

// labels[i] = -1 on the pixels of the components that are not selected; out = 1 on the selected pixels (| bit 1 of the
// mask byte); candidates / seeded: the roots, one atomic set per workgroup.  seeds is only read.
__global__ __launch_bounds__(256) void ob_gate_kernel(int* __restrict__ labels, const int* __restrict__ seeds, long hw,
                                                      const ObSeed k, int* candidates, int* seeded) {
  __shared__ int s_c[2];
  const int lane = threadIdx.x & 63, n = blockIdx.y;
  if (threadIdx.x < 2) s_c[threadIdx.x] = 0;
  __syncthreads();
  int nroot = 0, nhas = 0;                              // (lane 0 of each wave counts)
#pragma unroll 2
  for (int j = 0; j < OB_SEED_PER; ++j) {
    const long i = ((long)blockIdx.x * OB_SEED_PER + j) * 256 + threadIdx.x;
    bool root = false, has = false;
    if (i < hw) {
      const long o = (long)n * hw + i;
      const int r = labels[o];
      bool sel = false;
      if (r >= 0) {
        has = seeds[(long)n * hw + r] >= k.min_seed;
        sel = has != (k.invert != 0);
        root = r == (int)i;
        if (!sel) labels[o] = -1;
      }
      if (k.out) {
        const unsigned y = (unsigned)i / (unsigned)k.W, x = (unsigned)i - y * (unsigned)k.W;
        unsigned char v = sel ? 1 : 0;
        if (k.keep_tissue) v |= k.mask[(long)n * k.mask_img + (long)y * k.mask_pitch + x] & 2;
        k.out[(long)n * k.out_img + (long)y * k.out_pitch + x] = v;
      }
    }
    nroot += __popcll(__ballot(root));
    nhas += __popcll(__ballot(root && has));
  }
  if (lane == 0) {
    if (nroot) atomicAdd(&s_c[0], nroot);
    if (nhas) atomicAdd(&s_c[1], nhas);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_c[0]) atomicAdd(candidates + n, s_c[0]);
  if (threadIdx.x == 1 && s_c[1]) atomicAdd(seeded + n, s_c[1]);
}

// exclusive scan of one int per thread over the 256 threads; returns the thread's prefix, *total = the sum
__device__ __forceinline__ int block_exscan(int v, int* total) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();                                      // a previous call's readers have left wsum
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) base += w < wv ? wsum[w] : 0;
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return base + inc - v;
}

__device__ __forceinline__ int ob_kept4(const int* labels, const int* area, long base, long hw, int min_area, int* a4) {
  int flags = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = base + j;
    a4[j] = 0;
    if (i < hw && labels[i] == (int)i) {
      a4[j] = area[i];
      if (a4[j] >= min_area) flags |= 1 << j;
    }
  }
  return flags;
}

__global__ __launch_bounds__(256) void ob_count_kernel(const int* __restrict__ labels, const int* __restrict__ area,
                                                       long hw, int min_area, long nchunk, int* __restrict__ chunk) {
  const long off = (long)blockIdx.y * hw;
  int a4[4], total;
  const int flags = ob_kept4(labels + off, area + off, (long)blockIdx.x * OB_CHUNK + 4 * threadIdx.x, hw, min_area, a4);
  block_exscan(__popc(flags), &total);
  if (threadIdx.x == 0) chunk[(long)blockIdx.y * nchunk + blockIdx.x] = total;
}

// one workgroup per sample: chunk[c] <- the number of kept roots in the chunks before c
__global__ __launch_bounds__(256) void ob_scan_kernel(int* __restrict__ chunk, long nchunk, int* __restrict__ count) {
  int* c = chunk + (long)blockIdx.x * nchunk;
  int carry = 0;
  for (long b = 0; b < nchunk; b += 256) {
    const long i = b + threadIdx.x;
    const int v = i < nchunk ? c[i] : 0;
    int total;
    const int pre = block_exscan(v, &total);
    if (i < nchunk) c[i] = carry + pre;
    carry += total;
  }
  if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

struct ObTable {
  int max_objects;          // 0: no table
  int* area;                // [B][M]
  int* bbox;                // [B][M][4]  y0, x0, y1, x1, end-exclusive
  long long* sums;          // [B][M][2]  sum of y, sum of x
};

__global__ __launch_bounds__(256) void ob_number_kernel(const int* __restrict__ labels, int* __restrict__ area, long hw,
                                                        int min_area, long nchunk, const int* __restrict__ chunk,
                                                        long long* __restrict__ kept_pixels, int* __restrict__ largest,
                                                        long long* __restrict__ hist, const ObTable tb) {
  __shared__ unsigned long long s_kept;
  __shared__ int s_largest, s_hist[32];
  const int n = blockIdx.y;
  const long off = (long)n * hw, base = (long)blockIdx.x * OB_CHUNK + 4 * threadIdx.x;
  if (threadIdx.x < 32) s_hist[threadIdx.x] = 0;
  if (threadIdx.x == 32) s_kept = 0;
  if (threadIdx.x == 33) s_largest = 0;
  int a4[4], total;
  const int flags = ob_kept4(labels + off, area + off, base, hw, min_area, a4);
  int num = chunk[(long)n * nchunk + blockIdx.x] + block_exscan(__popc(flags), &total);   // (its barriers cover the zeroing)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = base + j;
    if (i >= hw || labels[off + i] != (int)i) continue;
    int mine = 0;
    if ((flags >> j) & 1) {
      mine = ++num;
      const int a = a4[j];
      atomicAdd(&s_kept, (unsigned long long)a);
      atomicMax(&s_largest, a);
      atomicAdd(&s_hist[31 - __clz(a)], 1);
      if (mine <= tb.max_objects) {
        const long row = (long)n * tb.max_objects + mine - 1;
        tb.area[row] = a;
        tb.bbox[4 * row] = INT_MAX;
        tb.bbox[4 * row + 1] = INT_MAX;
        tb.bbox[4 * row + 2] = 0;
        tb.bbox[4 * row + 3] = 0;
        tb.sums[2 * row] = 0;
        tb.sums[2 * row + 1] = 0;
      }
    }
    area[off + i] = mine;                    // the root's place now holds its number (0: dropped)
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    if (s_hist[threadIdx.x]) atomicAdd((unsigned long long*)hist + 32 * n + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
  } else if (threadIdx.x == 32) {
    if (s_kept) atomicAdd((unsigned long long*)kept_pixels + n, s_kept);
  } else if (threadIdx.x == 33) {
    if (s_largest) atomicMax(largest + n, s_largest);
  }
}

// A wave covers 64 consecutive pixels of ONE row, so per distinct object it knows the row, the count and, from the ballot
// alone, the first and last column and the sum of the columns.
__global__ __launch_bounds__(256) void ob_relabel_kernel(int* __restrict__ labels, const int* __restrict__ number, int H,
                                                         int W, const ObTable tb) {
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  const long off = (long)n * H * W;
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    int lab = 0;
    if (x < W) {
      const long i = off + (long)y * W + x;
      const int r = labels[i];
      lab = r >= 0 ? number[off + r] : 0;
      labels[i] = lab;
    }
    if (tb.max_objects == 0) continue;
    unsigned long long todo = __ballot(lab > 0 && lab <= tb.max_objects);
    while (todo) {                                      // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lk = __shfl(lab, leader, 64);
      const unsigned long long same = __ballot(lab == lk);
      if (lane == leader) {
        const int cnt = __popcll(same), xw = x - lane;  // the wave's first column
        const int first = __ffsll((long long)same) - 1, last = 63 - __clzll((long long)same);
        // sum of the set bits' positions, bit by bit of the position
        const int pos = __popcll(same & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(same & 0xCCCCCCCCCCCCCCCCull) +
                        4 * __popcll(same & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(same & 0xFF00FF00FF00FF00ull) +
                        16 * __popcll(same & 0xFFFF0000FFFF0000ull) + 32 * __popcll(same & 0xFFFFFFFF00000000ull);
        const long row = (long)n * tb.max_objects + lk - 1;
        atomicMin(tb.bbox + 4 * row, y);
        atomicMin(tb.bbox + 4 * row + 1, xw + first);
        atomicMax(tb.bbox + 4 * row + 2, y + 1);
        atomicMax(tb.bbox + 4 * row + 3, xw + last + 1);
        atomicAdd((unsigned long long*)tb.sums + 2 * row, (unsigned long long)((long long)y * cnt));
        atomicAdd((unsigned long long*)tb.sums + 2 * row + 1, (unsigned long long)((long long)xw * cnt + pos));
      }
      todo &= ~same;
    }
  }
}

__global__ __launch_bounds__(256) void ob_centroid_kernel(const int* __restrict__ count, const int* __restrict__ area,
                                                          const long long* __restrict__ sums, int M, long rows,
                                                          float* __restrict__ centroid) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int n = (int)(r / M), j = (int)(r - (long)n * M);
  float cy = 0.0f, cx = 0.0f;
  if (j < count[n]) {
    const double a = (double)area[r];
    cy = (float)((double)sums[2 * r] / a);
    cx = (float)((double)sums[2 * r + 1] / a);
  }
  centroid[2 * r] = cy;
  centroid[2 * r + 1] = cx;
}

// ---- paired hits -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ob_fill_kernel(int* __restrict__ p, long nwords) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < nwords) p[i] = 0;
}

// flags: [B][2][fw] words, one bit per object number; a label image holds numbers <= hw / 2 + 1 < 32 fw
__global__ __launch_bounds__(256) void ob_touch_kernel(const int* __restrict__ la, const int* __restrict__ lb, long hw,
                                                       long fw, unsigned* flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long o = (long)blockIdx.y * hw + i;
  const int a = la[o], b = lb[o];
  if (a <= 0 || b <= 0 || (a >> 5) >= fw || (b >> 5) >= fw) return;      // (numbers beyond hw / 2 + 1 cannot come from a labelling)
  unsigned* f = flags + (long)blockIdx.y * 2 * fw;
  const unsigned ba = 1u << (a & 31), bb = 1u << (b & 31);
  // most pixels of an object find its bit set already: look before the atomic (bits are only ever set, so a look can at worst miss one)
  if (!(__hip_atomic_load(f + (a >> 5), OB_RLX_AGENT) & ba)) atomicOr(f + (a >> 5), ba);
  if (!(__hip_atomic_load(f + fw + (b >> 5), OB_RLX_AGENT) & bb)) atomicOr(f + fw + (b >> 5), bb);
}

__global__ __launch_bounds__(256) void ob_hits_kernel(const unsigned* __restrict__ flags, long fw, int* hits) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const unsigned* f = flags + ((long)blockIdx.z * 2 + blockIdx.y) * fw;
  int c = i < fw ? __popc(f[i]) : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(hits + 2 * blockIdx.z + blockIdx.y, c);
}

// out [B][3] = recall, precision, f1; abs_err [B] = |count_pred - count_target|
__global__ void ob_scores_kernel(const int* __restrict__ count_pred, const int* __restrict__ count_target,
                                 const int* __restrict__ hits, int B, float* __restrict__ out, int* __restrict__ abs_err) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const int cp = count_pred[n], ct = count_target[n];
  const double rec = ct > 0 ? (double)hits[2 * n + 1] / (double)ct : (cp == 0 ? 1.0 : 0.0);
  const double pre = cp > 0 ? (double)hits[2 * n] / (double)cp : (ct == 0 ? 1.0 : 0.0);
  const double den = pre + rec;
  double f1 = 0.0;
  if (den > 0.0) {
    const double num = (2.0 * pre) * rec;
    f1 = num / den;
  }
  out[3 * n] = (float)rec;
  out[3 * n + 1] = (float)pre;
  out[3 * n + 2] = (float)f1;
  abs_err[n] = abs(cp - ct);
}

__global__ void ob_density_kernel(const long long* __restrict__ kept, const long long* __restrict__ tissue,
                                  const int* __restrict__ count, int B, double mm2_per_pixel, float* __restrict__ burden,
                                  double* __restrict__ per_mm2) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B) return;
  const long long t = tissue[n];
  burden[n] = (float)((double)kept[n] / (double)max(t, 1LL));
  if (per_mm2) {
    const double mm2 = (double)t * mm2_per_pixel;
    per_mm2[n] = t > 0 ? (double)count[n] / mm2 : 0.0;
  }
}

bool ob_shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W <= OB_MAX_PIXELS;
}
long ob_flag_words(long hw) { return (hw / 2 + 2 + 31) / 32; }

// local, merge, flatten: labels[i] = the first raster pixel of i's component, -1 on background
void ob_roots(const ObMask& k, int B, int conn8, int* parent, int* labels, hipStream_t s) {
  const int H = k.H, W = k.W;
  const long hw = (long)H * W;
  const int tiles_y = cdiv(H, OT_H), tiles_x = cdiv(W, OT_W);
  const long tiles = (long)tiles_y * tiles_x, pix_blocks = (hw + 255) / 256;
  hipLaunchKernelGGL(ob_local_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, s, k, tiles_x, conn8, parent);
  const long n_h = (long)(tiles_y - 1) * W, n_v = (long)(tiles_x - 1) * H;
  if (n_h + n_v > 0)
    hipLaunchKernelGGL(ob_merge_kernel, dim3((unsigned)((n_h + n_v + 255) / 256), (unsigned)B), dim3(256), 0, s, k, n_h,
                       n_v, conn8, parent);
  hipLaunchKernelGGL(ob_flatten_kernel, dim3((unsigned)pix_blocks, (unsigned)B), dim3(256), 0, s, parent, hw, labels);
}

}  // namespace

// ---- the numbering stage (objects_number.h): zero, area, count, scan, number, relabel -----------------------------------
long s2s_number_chunks(long hw) { return (hw + OB_CHUNK - 1) / OB_CHUNK; }

void s2s_number_sets(int* labels, int* area, int* chunk, int B, int H, int W, int min_area, int max_objects, int* count,
                     long long* kept_pixels, int* largest, long long* size_hist, int* tab_area, int* tab_bbox,
                     long long* tab_sums, hipStream_t s) {
  const long hw = (long)H * W, nchunk = s2s_number_chunks(hw);
  const ObTable tb{max_objects, tab_area, tab_bbox, tab_sums};
  const dim3 pix((unsigned)((hw + 255) / 256), (unsigned)B), chunks((unsigned)nchunk, (unsigned)B);
  hipLaunchKernelGGL(ob_zero_kernel, pix, dim3(256), 0, s, labels, hw, area);
  hipLaunchKernelGGL(ob_area_kernel, pix, dim3(256), 0, s, labels, hw, area);
  hipLaunchKernelGGL(ob_count_kernel, chunks, dim3(256), 0, s, labels, area, hw, min_area, nchunk, chunk);
  hipLaunchKernelGGL(ob_scan_kernel, dim3((unsigned)B), dim3(256), 0, s, chunk, nchunk, count);
  hipLaunchKernelGGL(ob_number_kernel, chunks, dim3(256), 0, s, labels, area, hw, min_area, nchunk, chunk, kept_pixels,
                     largest, size_hist, tb);
  hipLaunchKernelGGL(ob_relabel_kernel, dim3((unsigned)cdiv(W, 256), (unsigned)(H < 65535 ? H : 65535), (unsigned)B),
                     dim3(256), 0, s, labels, area, H, W, tb);
}

extern "C" long s2s_objects_words(int B, int H, int W) {
  if (!ob_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  const long hw = (long)H * W;
  return (long)B * (hw + (hw + OB_CHUNK - 1) / OB_CHUNK);
}

extern "C" long s2s_objects_hit_words(int B, int H, int W) {
  if (!ob_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  return (long)B * 2 * ob_flag_words((long)H * W);
}

extern "C" int s2s_objects_label(const void* mask, long pitch, long img_stride, int fg_bits, int B, int H, int W,
                                 int connectivity, int min_area, int max_objects, int* scratch, int* labels, int* count,
                                 long* kept_pixels, int* largest, long* size_hist, int* tab_area, int* tab_bbox,
                                 long* tab_sums, void* stream) {
  if (!mask || !scratch || !labels || !count || !kept_pixels || !largest || !size_hist) return S2S_ERR_NULL;
  if (max_objects > 0 && (!tab_area || !tab_bbox || !tab_sums)) return S2S_ERR_NULL;
  if (!ob_shape_ok(B, H, W) || (connectivity != 4 && connectivity != 8) || min_area < 1 || max_objects < 0 ||
      fg_bits < 1 || fg_bits > 255 || pitch < W || (B > 1 && img_stride < pitch * (long)H) ||
      (long)B * max_objects > 0x7fffffffL)
    return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  if ((long)cdiv(H, OT_H) * cdiv(W, OT_W) > 0x7fffffffL) return S2S_ERR_SHAPE;
  int* parent = scratch;
  int* chunk = scratch + (long)B * hw;
  const ObMask k{(const unsigned char*)mask, pitch, img_stride, fg_bits, H, W};
  ob_roots(k, B, connectivity == 8, parent, labels, s);
  s2s_number_sets(labels, parent, chunk, B, H, W, min_area, max_objects, count, (long long*)kept_pixels, largest,
                  (long long*)size_hist, tab_area, tab_bbox, (long long*)tab_sums, s);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objects_label_seeded(const void* mask, long pitch, long img_stride, int fg_bits, const void* marker,
                                        long marker_pitch, long marker_img_stride, int seed_bits, int min_seed,
                                        int invert, int B, int H, int W, int connectivity, int min_area,
                                        int max_objects, int* scratch, int* labels, int* count, long* kept_pixels,
                                        int* largest, long* size_hist, int* tab_area, int* tab_bbox, long* tab_sums,
                                        void* out_mask, long out_pitch, long out_img_stride, int* candidates,
                                        int* seeded, long* seed_pixels, void* stream) {
  if (!mask || !marker || !scratch || !labels || !count || !kept_pixels || !largest || !size_hist || !candidates ||
      !seeded || !seed_pixels)
    return S2S_ERR_NULL;
  if (max_objects > 0 && (!tab_area || !tab_bbox || !tab_sums)) return S2S_ERR_NULL;
  if (!ob_shape_ok(B, H, W) || (connectivity != 4 && connectivity != 8) || min_area < 1 || max_objects < 0 ||
      fg_bits < 1 || fg_bits > 255 || pitch < W || (B > 1 && img_stride < pitch * (long)H) ||
      (long)B * max_objects > 0x7fffffffL)
    return S2S_ERR_SHAPE;
  if (seed_bits < 1 || seed_bits > 255 || min_seed < 1 || (invert != 0 && invert != 1) || marker_pitch < W ||
      (B > 1 && marker_img_stride < marker_pitch * (long)H))
    return S2S_ERR_SHAPE;
  if (out_mask && (out_pitch < W || (B > 1 && out_img_stride < out_pitch * (long)H))) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  if ((long)cdiv(H, OT_H) * cdiv(W, OT_W) > 0x7fffffffL) return S2S_ERR_SHAPE;
  int* parent = scratch;
  int* chunk = scratch + (long)B * hw;
  const ObMask k{(const unsigned char*)mask, pitch, img_stride, fg_bits, H, W};
  ob_roots(k, B, connectivity == 8, parent, labels, s);
  ObSeed sd;
  sd.marker = (const unsigned char*)marker;
  sd.pitch = marker_pitch;
  sd.img = marker_img_stride;
  sd.bits = seed_bits;
  sd.min_seed = min_seed;
  sd.invert = invert;
  sd.mask = k.m;
  sd.mask_pitch = pitch;
  sd.mask_img = img_stride;
  sd.keep_tissue = fg_bits == 1;
  sd.out = (unsigned char*)out_mask;
  sd.out_pitch = out_pitch;
  sd.out_img = out_img_stride;
  sd.W = W;
  const dim3 pix((unsigned)((hw + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(ob_seed_zero_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, B, candidates, seeded,
                     (long long*)seed_pixels);
  hipLaunchKernelGGL(ob_zero_kernel, pix, dim3(256), 0, s, labels, hw, parent);
  const dim3 pix8((unsigned)((hw + 256L * OB_SEED_PER - 1) / (256L * OB_SEED_PER)), (unsigned)B);
  hipLaunchKernelGGL(ob_seed_kernel, pix8, dim3(256), 0, s, labels, hw, sd, parent, (long long*)seed_pixels);
  hipLaunchKernelGGL(ob_gate_kernel, pix8, dim3(256), 0, s, labels, parent, hw, sd, candidates, seeded);
  s2s_number_sets(labels, parent, chunk, B, H, W, min_area, max_objects, count, (long long*)kept_pixels, largest,
                  (long long*)size_hist, tab_area, tab_bbox, (long long*)tab_sums, s);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objects_centroid(const int* count, const int* tab_area, const long* tab_sums, int B, int max_objects,
                                    float* centroid, void* stream) {
  if (!count || !tab_area || !tab_sums || !centroid) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || max_objects < 1 || (long)B * max_objects > 0x7fffffffL) return S2S_ERR_SHAPE;
  const long rows = (long)B * max_objects;
  hipLaunchKernelGGL(ob_centroid_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, count,
                     tab_area, (const long long*)tab_sums, max_objects, rows, centroid);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objects_hits(const int* labels_pred, const int* labels_target, int B, int H, int W, int* scratch,
                                int* hits, void* stream) {
  if (!labels_pred || !labels_target || !scratch || !hits) return S2S_ERR_NULL;
  if (!ob_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W, fw = ob_flag_words(hw);
  hipLaunchKernelGGL(ob_fill_kernel, dim3((unsigned)(((long)B * 2 * fw + 255) / 256)), dim3(256), 0, s, scratch,
                     (long)B * 2 * fw);
  hipLaunchKernelGGL(ob_fill_kernel, dim3(cdiv(2 * B, 256)), dim3(256), 0, s, hits, 2L * B);
  hipLaunchKernelGGL(ob_touch_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)B), dim3(256), 0, s, labels_pred,
                     labels_target, hw, fw, (unsigned*)scratch);
  hipLaunchKernelGGL(ob_hits_kernel, dim3((unsigned)((fw + 255) / 256), 2, (unsigned)B), dim3(256), 0, s,
                     (const unsigned*)scratch, fw, hits);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objects_scores(const int* count_pred, const int* count_target, const int* hits, int B, float* out,
                                  int* abs_err, void* stream) {
  if (!count_pred || !count_target || !hits || !out || !abs_err) return S2S_ERR_NULL;
  if (B < 1 || B > 65535) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(ob_scores_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, count_pred, count_target,
                     hits, B, out, abs_err);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_objects_density(const long* kept_pixels, const long* tissue, const int* count, int B,
                                   const double* mm2_per_pixel, float* burden, double* per_mm2, void* stream) {
  if (!kept_pixels || !tissue || !count || !burden || (mm2_per_pixel && !per_mm2)) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || (mm2_per_pixel && !(*mm2_per_pixel > 0.0))) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(ob_density_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)kept_pixels, (const long long*)tissue, count, B,
                     mm2_per_pixel ? *mm2_per_pixel : 0.0, burden, mm2_per_pixel ? per_mm2 : nullptr);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
