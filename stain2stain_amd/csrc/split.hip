// Splitting touching objects at their necks: a two-level steepest ascent on the exact squared distance map.  DESIGN.md
// section 3.27.
//
//   s2s_split_words   int32 words of scratch a call needs
//   s2s_split_label   d2 int32 [B][H][W] (s2s_morph_edt, to_foreground = 0; foreground = d2 > 0) -> labels, count, the
//                     statistics and tables of s2s_objects_label over the PARTS, and the number of basins
//
// With key(p) = (d2[p], y W + x), a strict total order, and neighbours = the 4 or 8 foreground neighbours:
//   ascent   up(p) = the neighbour of largest key if that exceeds key(p), else p; root(p) = the fixed point; a basin is a
//            set of equal root, its peak P = d2[root]
//   best     over the neighbouring pairs (p, q) with a = root(p) != b = root(q) and key(b) > key(a), the largest
//            (min(d2[p], d2[q]), b): the thickest neck of a towards a higher basin
//   join     a links to b iff P(a) <= core2 or m 2^20 >= neck_q^2 P(a); links rise in key, so they form a forest, and a
//            part is a tree of it.  One round: nothing is looked at again after a join.
// Every choice is a maximum over a strict total order and every accumulated value is an integer, so scheduling and the
// order of the atomics cannot change a bit of the result.
//
// Passes (every one a launch of its own on the caller's stream; no pass waits for another workgroup):
//   ascent   one workgroup per 32 x 64 tile, d2 and a one-pixel halo in LDS; the chain of every pixel is followed inside
//            the tile in LDS, so ptr[i] = the chain's root if it lies in the tile, else its first pixel outside
//            (-1: background); zeroes the pixel's best slot and the sample's basin count
//   resolve  ptr[i] = the fixed point of ptr from i.  It reads pointers the same launch overwrites: every access is an
//            agent-scope atomic, every value a pixel can hold lies on its own chain between it and the root, and only a
//            root points to itself, so what a thread happens to see changes how many steps it takes and nothing else
//   best     64-bit atomicMax of (m << 32 | b) into the slot of root(p), reduced over the lanes of equal root first;
//            pixels whose neighbours share their root (nearly all) contribute nothing
//   link     per root: the join rule; ptr[a] = b on a join (a root's own slot: no other thread of the launch reads it);
//            first[a] = INT_MAX; counts the basins, one atomicAdd per workgroup of 4096 pixels
//   resolve  again: ptr[i] = the root of i's part
//   first    first[part root] = the smallest raster index of the part, one atomicMin per wave and distinct part
//   labels   labels[i] = first[ptr[i]], -1 on the background: the input of the numbering stage of s2s_objects_label
//   zero, area, count, scan, number, relabel: s2s_number_sets (objects_number.h, objects.hip)
//
// The scratch holds the previous call's contents: every word a pass reads was written by an earlier pass of the same call.
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include <limits.h>

#include "common.h"
#include "objects_number.h"

namespace {

constexpr int ST_H = 32, ST_W = 64;          // the ascent pass's tile (split.TILE)
constexpr int SH_W = ST_W + 2, SH_H = ST_H + 2;
constexpr int SP_MAX_SIDE = 32767;
constexpr int SP_LINK_SPAN = 4096;           // raster indices per workgroup of the link pass

#define SP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// (da, ia) > (db, ib) lexicographically
__device__ __forceinline__ bool sp_key_gt(int da, int ia, int db, int ib) { return da > db || (da == db && ia > ib); }

__global__ __launch_bounds__(256) void sp_ascent_kernel(const int* __restrict__ d2, int H, int W, int tiles_x, int conn8,
                                                        int* __restrict__ ptr, unsigned long long* __restrict__ best,
                                                        int* __restrict__ basins) {
  __shared__ int s_d[SH_H * SH_W];
  __shared__ int s_p[SH_H * SH_W];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int n = blockIdx.y;
  const int y0 = ty * ST_H, x0 = tx * ST_W;
  const long off = (long)n * H * W;
  if (blockIdx.x == 0 && threadIdx.x == 0) basins[n] = 0;
  for (int c = threadIdx.x; c < SH_H * SH_W; c += 256) {
    const int r = c / SH_W, gy = y0 + r - 1, gx = x0 + (c - r * SH_W) - 1;
    s_d[c] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? d2[off + (long)gy * W + gx] : 0;   // outside the image: background
    s_p[c] = c;                                                                             // halo and background: terminal
  }
  __syncthreads();
  for (int r = wv; r < ST_H; r += 4) {
    const int c = (r + 1) * SH_W + lane + 1;
    const int d = s_d[c];
    if (d <= 0) continue;
    int bd = d, bc = c;                       // inside one tile the halo coordinate orders pixels as the raster index does
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0)) continue;
        const int q = c + dy * SH_W + dx, dq = s_d[q];
        if (dq > 0 && sp_key_gt(dq, q, bd, bc)) { bd = dq; bc = q; }
      }
    s_p[c] = bc;
  }
  __syncthreads();
  for (int r = wv; r < ST_H; r += 4) {
    const int gy = y0 + r, gx = x0 + lane;
    if (gy >= H || gx >= W) continue;
    int c = (r + 1) * SH_W + lane + 1, p = -1;
    if (s_d[c] > 0) {
      int q;
      while ((q = s_p[c]) != c) c = q;        // keys rise strictly along the chain: it ends, at a root or in the halo
      const int cr = c / SH_W;
      p = (int)((long)(y0 + cr - 1) * W + x0 + (c - cr * SH_W) - 1);
    }
    const long i = off + (long)gy * W + gx;
    ptr[i] = p;
    best[i] = 0ull;
  }
}

// ptr[i] <- the fixed point of ptr from i.  See the header: agent-scope atomics only, result independent of the interleaving.
__global__ __launch_bounds__(256) void sp_resolve_kernel(int* ptr, long hw) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  int* p = ptr + (long)blockIdx.y * hw;
  int r = __hip_atomic_load(p + i, SP_RLX_AGENT);
  if (r < 0) return;
  const int r0 = r;
  int q;
  while ((q = __hip_atomic_load(p + r, SP_RLX_AGENT)) != r) r = q;
  if (r != r0) __hip_atomic_store(p + i, r, SP_RLX_AGENT);
}

__global__ __launch_bounds__(256) void sp_best_kernel(const int* __restrict__ d2, const int* __restrict__ root, int H, int W,
                                                      int conn8, unsigned long long* best) {
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  const long off = (long)n * H * W;
  const int* d = d2 + off;
  const int* rt = root + off;
  unsigned long long* bs = best + off;
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    int a = -1;
    unsigned long long cand = 0ull;
    if (x < W) {
      const int i = y * W + x;
      a = rt[i];
      if (a >= 0) {
        const int dp = d[i];
        int da = 0;
        for (int dy = -1; dy <= 1; ++dy) {
          const int yy = y + dy;
          if (yy < 0 || yy >= H) continue;
          for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if ((dy == 0 && dx == 0) || (!conn8 && dy != 0 && dx != 0) || xx < 0 || xx >= W) continue;
            const int q = yy * W + xx, b = rt[q];
            if (b < 0 || b == a) continue;
            if (da == 0) da = d[a];
            if (!sp_key_gt(d[b], b, da, a)) continue;
            const unsigned long long c = ((unsigned long long)(unsigned)min(dp, d[q]) << 32) | (unsigned)b;
            cand = c > cand ? c : cand;
          }
        }
      }
    }
    unsigned long long todo = __ballot(cand != 0ull);
    while (todo) {                                        // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int la = __shfl(a, leader, 64);
      const bool mine = cand != 0ull && a == la;
      unsigned long long v = mine ? cand : 0ull;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
      }
      // the slot only grows, so a look can at worst miss a larger value and cost one atomic
      if (lane == leader && __hip_atomic_load(bs + la, SP_RLX_AGENT) < v) __hip_atomic_fetch_max(bs + la, v, SP_RLX_AGENT);
      todo &= ~__ballot(mine);
    }
  }
}

__global__ __launch_bounds__(256) void sp_link_kernel(const int* __restrict__ d2, int* __restrict__ ptr,
                                                      const unsigned long long* __restrict__ best, long hw,
                                                      long long neck2, int core2, int* __restrict__ first, int* basins) {
  __shared__ int s_roots[4];
  const long off = (long)blockIdx.y * hw;
  int roots = 0;
  for (int j = 0; j < SP_LINK_SPAN; j += 256) {
    const long i = (long)blockIdx.x * SP_LINK_SPAN + j + threadIdx.x;
    if (i >= hw || ptr[off + i] != (int)i) continue;
    ++roots;
    const unsigned long long bm = best[off + i];
    first[off + i] = INT_MAX;
    if (bm) {
      const long long m = (long long)(bm >> 32), P = d2[off + i];
      if (P <= core2 || (m << 20) >= neck2 * P) ptr[off + i] = (int)(unsigned)(bm & 0xffffffffull);
    }
  }
  // every add goes to the sample's one counter: one per workgroup, not one per wave (32 000 basins of a 4096^2 field
  // cost 0.3 ms that way)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) roots += __shfl_xor(roots, o, 64);
  if ((threadIdx.x & 63) == 0) s_roots[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = s_roots[0] + s_roots[1] + s_roots[2] + s_roots[3];
    if (total) atomicAdd(basins + blockIdx.y, total);
  }
}

// Raster indices rise with the lane, so the first lane of a part in the wave holds the part's smallest index of the wave.
__global__ __launch_bounds__(256) void sp_first_kernel(const int* __restrict__ ptr, long hw, int* first) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int key = i < hw ? ptr[(long)blockIdx.y * hw + i] : -1;
  int* f = first + (long)blockIdx.y * hw;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {                                        // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const int lk = __shfl(key, leader, 64);
    if (lane == leader) atomicMin(f + lk, (int)i);
    todo &= ~__ballot(key == lk);
  }
}

__global__ __launch_bounds__(256) void sp_labels_kernel(const int* __restrict__ ptr, const int* __restrict__ first, long hw,
                                                        int* __restrict__ labels) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const long off = (long)blockIdx.y * hw;
  const int r = ptr[off + i];
  labels[off + i] = r >= 0 ? first[off + r] : -1;
}

bool sp_shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= SP_MAX_SIDE && W <= SP_MAX_SIDE;
}

}  // namespace

// best (two words a pixel, first: 8-byte aligned), ptr, first, chunk counts
extern "C" long s2s_split_words(int B, int H, int W) {
  if (!sp_shape_ok(B, H, W)) return S2S_ERR_SHAPE;
  const long hw = (long)H * W;
  return (long)B * (4 * hw + s2s_number_chunks(hw));
}

extern "C" int s2s_split_label(const int* d2, int B, int H, int W, int connectivity, int neck_q, int core2, int min_area,
                               int max_objects, int* scratch, int* labels, int* count, int* basins, long* kept_pixels,
                               int* largest, long* size_hist, int* tab_area, int* tab_bbox, long* tab_sums, void* stream) {
  if (!d2 || !scratch || !labels || !count || !basins || !kept_pixels || !largest || !size_hist) return S2S_ERR_NULL;
  if (max_objects > 0 && (!tab_area || !tab_bbox || !tab_sums)) return S2S_ERR_NULL;
  if (!sp_shape_ok(B, H, W) || (connectivity != 4 && connectivity != 8) || neck_q < 0 || neck_q > 1024 || core2 < 0 ||
      min_area < 1 || max_objects < 0 || (long)B * max_objects > 0x7fffffffL)
    return S2S_ERR_SHAPE;
  if ((uintptr_t)scratch & 7) return S2S_ERR_ALIGN;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  hipStream_t s = (hipStream_t)stream;
  const long hw = (long)H * W;
  const int tiles_x = cdiv(W, ST_W);
  const unsigned tiles = (unsigned)(cdiv(H, ST_H) * tiles_x);
  unsigned long long* best = (unsigned long long*)scratch;
  int* ptr = scratch + 2 * (long)B * hw;
  int* first = ptr + (long)B * hw;
  int* chunk = first + (long)B * hw;
  const int conn8 = connectivity == 8;
  const dim3 pix((unsigned)((hw + 255) / 256), (unsigned)B);
  hipLaunchKernelGGL(sp_ascent_kernel, dim3(tiles, (unsigned)B), dim3(256), 0, s, d2, H, W, tiles_x, conn8, ptr, best,
                     basins);
  hipLaunchKernelGGL(sp_resolve_kernel, pix, dim3(256), 0, s, ptr, hw);
  hipLaunchKernelGGL(sp_best_kernel, dim3((unsigned)cdiv(W, 256), (unsigned)H, (unsigned)B), dim3(256), 0, s, d2,
                     (const int*)ptr, H, W, conn8, best);
  hipLaunchKernelGGL(sp_link_kernel, dim3((unsigned)((hw + SP_LINK_SPAN - 1) / SP_LINK_SPAN), (unsigned)B), dim3(256), 0,
                     s, d2, ptr, (const unsigned long long*)best, hw, (long long)neck_q * neck_q, core2, first, basins);
  hipLaunchKernelGGL(sp_resolve_kernel, pix, dim3(256), 0, s, ptr, hw);
  hipLaunchKernelGGL(sp_first_kernel, pix, dim3(256), 0, s, (const int*)ptr, hw, first);
  hipLaunchKernelGGL(sp_labels_kernel, pix, dim3(256), 0, s, (const int*)ptr, (const int*)first, hw, labels);
  s2s_number_sets(labels, ptr, chunk, B, H, W, min_area, max_objects, count, (long long*)kept_pixels, largest,
                  (long long*)size_hist, tab_area, tab_bbox, (long long*)tab_sums, s);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
