// Result rendering: class / label overlays with outlines, heat-map overlays, comparisons of two regions and box
// thumbnails, all over uint8 regions.  DESIGN.md section 3.32.
//
//   s2s_render_classes_u8   base blended with a palette colour per class byte, outlines on class borders
//   s2s_render_labels_u8    the same from an int32 label image (label_components, stain_objects, split_objects)
//   s2s_render_heat_u8      base blended with a colour table indexed by a node map, nearest cell or interpolated
//   s2s_render_compare_u8   checkerboard, blend or amplified difference of two regions
//   s2s_box_down_u8         box average (image) or box maximum (mask) by an integer factor
//
// Arithmetic (normative; restated in include/stain2stain_hip.h).  mix(b, c, a) = (b (256 - a) + c a + 128) >> 8 per
// channel, a in 0 .. 256: a = 0 gives b, a = 256 gives c.  Everything is integer and computed from global coordinates,
// so the bytes do not depend on the banding: a launch writes rows [row0, row0 + rows); an input read at neighbouring
// rows (the class mask, the label image, the thumbnail's source) is present at rows [src_row0, src_row0 + src_rows).
//
// Mapping (that of wp_warp_kernel).  A wave owns 256 consecutive output pixels of one row, a lane four of them; a
// workgroup is four waves on four consecutive rows; the grid strides over tiles, at most 65 536 workgroups.  The row
// index is wave-uniform, so the row quantities of the heat interpolation and the checkerboard live in scalar registers.
// A lane's 12 image bytes are read as four aligned dwords rebuilt with v_alignbyte_b32 where those dwords lie inside
// the buffer and byte by byte otherwise (the first and last bytes of a buffer); they go out as three dwords where the
// lane has four pixels and the address is dword-aligned, bytes otherwise.  A dword load may cover bytes of a neighbouring
// lane's pixels; only the lane's own bytes are used, which is what lets out alias base.  No LDS, no atomics.
//
// Nothing here allocates, synchronises or reads back to the host.  All index arithmetic is 64-bit.
#include "common.h"

namespace {

constexpr int RD_MAX_SIDE = 1 << 30;
constexpr int RD_MAX_R = 4;                                  // edge radius
constexpr int RD_MAX_CELL = 1 << 14;                         // heat: span^2 * 65280 stays below 2^46
constexpr int RD_MAX_NODES = 65536;
constexpr int RD_DMAX = 65280;                               // 255 * 256
constexpr int RD_MAX_F = 256;
constexpr int RD_WAVES = 4;                                  // output rows per workgroup
constexpr int RD_PX = 256;                                   // pixels of a row per wave: 64 lanes x 4
constexpr long RD_MAX_BLOCKS = 65536;
constexpr int RD_F64_NODE = 1 << 20;                         // nodes within this take the float64 blend

__device__ __forceinline__ unsigned rd_mix(unsigned b, unsigned c, unsigned a) { return (b * (256u - a) + c * a + 128u) >> 8; }

__device__ __forceinline__ unsigned rd_byte(const unsigned (&t)[3], int i) { return (t[i >> 2] >> (8 * (i & 3))) & 255u; }

// Bytes p[0 .. 12) as three dwords.  Where the four aligned dwords around them lie inside [lo, hi) they are loaded
// whole; otherwise only bytes [k0, k1), which the caller knows to be inside the buffer, are read and the rest are 0.
__device__ __forceinline__ void rd_load12(const unsigned char* p, int k0, int k1, const unsigned char* lo,
                                          const unsigned char* hi, unsigned (&t)[3]) {
  const unsigned o = (unsigned)((uintptr_t)p & 3);
  const unsigned char* q = p - o;
  if (q >= lo && q + 16 <= hi) {
    const unsigned* u = reinterpret_cast<const unsigned*>(q);
    const unsigned a0 = u[0], a1 = u[1], a2 = u[2], a3 = u[3];
    t[0] = __builtin_amdgcn_alignbyte(a1, a0, o);
    t[1] = __builtin_amdgcn_alignbyte(a2, a1, o);
    t[2] = __builtin_amdgcn_alignbyte(a3, a2, o);
  } else {
    t[0] = 0; t[1] = 0; t[2] = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      if (k >= k0 && k < k1) t[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
    }
  }
}

// Bytes p[0 .. n), n in 1 .. 4, as one dword; the bytes from n on are unspecified.
__device__ __forceinline__ unsigned rd_load4(const unsigned char* p, int n, const unsigned char* lo, const unsigned char* hi) {
  const unsigned o = (unsigned)((uintptr_t)p & 3);
  const unsigned char* q = p - o;
  if (q >= lo && q + 8 <= hi) {
    const unsigned* u = reinterpret_cast<const unsigned*>(q);
    return __builtin_amdgcn_alignbyte(u[1], u[0], o);
  }
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < n) v |= (unsigned)p[k] << (8 * k);
  }
  return v;
}

// Zero every byte of t from nbytes on (nbytes in 0 .. 12).
__device__ __forceinline__ void rd_keep(unsigned (&t)[3], int nbytes) {
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const int n = nbytes - 4 * w;
    t[w] = n >= 4 ? t[w] : (n <= 0 ? 0u : (t[w] & ((1u << (8 * n)) - 1u)));
  }
}

__device__ __forceinline__ void rd_store12(unsigned char* o, int npx, const unsigned (&t)[3]) {
  if (npx == 4 && ((uintptr_t)o & 3) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<unsigned*>(o)[q] = t[q];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      if (k < npx * 3) o[k] = (unsigned char)rd_byte(t, k);
    }
  }
}

__device__ __forceinline__ void rd_pack(const unsigned (&v)[12], unsigned (&t)[3]) {
#pragma unroll
  for (int q = 0; q < 3; ++q) t[q] = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
}

// ---- class and label overlays -------------------------------------------------------------------------------------------
struct RdClassArgs {
  const unsigned char* base;                                 // row row0
  const unsigned char* base_end;
  long base_pitch;
  const unsigned char* mask;                                 // row mask_row0: class bytes, or int32 labels
  const unsigned char* mask_end;
  long mask_pitch;
  const unsigned char* palette;                              // [256][3]
  const int* fill_alpha;                                     // [256]
  unsigned char* out;                                        // row row0
  long out_pitch;
  int mask_row0, mask_rows, row0, rows, H, W, r, edge_alpha, edge_rgb, inplace;
  long nchunk, tiles;
};

template <bool LABELS>
__global__ __launch_bounds__(256) void rd_classes_kernel(const RdClassArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long rg = t / A.nchunk, chunk = t - rg * A.nchunk;
    const long yl = rg * RD_WAVES + wave;                    // row of this launch's band: wave-uniform
    const long x0 = chunk * RD_PX + 4L * lane;
    if (yl >= A.rows || x0 >= A.W) continue;
    const long y = (long)A.row0 + yl;
    const int npx = (int)min(4L, (long)A.W - x0);
    // ---- identity and colour index of the lane's pixels
    int id[4] = {0, 0, 0, 0}, ci[4] = {0, 0, 0, 0};
    const unsigned char* mrow = A.mask + (y - A.mask_row0) * A.mask_pitch;
    if (LABELS) {
      const int* lrow = reinterpret_cast<const int*>(mrow);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < npx) {
          const int L = lrow[x0 + j];
          id[j] = L > 0 ? L : 0;
          ci[j] = L > 0 ? (int)((unsigned)(L - 1) % 255u) + 1 : 0;
        }
      }
    } else {
      const unsigned w = rd_load4(mrow + x0, npx, A.mask, A.mask_end);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < npx) { id[j] = (int)((w >> (8 * j)) & 255u); ci[j] = id[j]; }
      }
    }
    // ---- the edge test: identities over the diamond |dy| + |dx| <= r, -1 outside the region
    bool edge[4] = {false, false, false, false};
    if (A.r >= 1 && (id[0] | id[1] | id[2] | id[3]) != 0) {
#pragma unroll 1
      for (int dy = -A.r; dy <= A.r; ++dy) {
        const int h = A.r - (dy < 0 ? -dy : dy);
        const long yy = y + dy;
        int seg[12];                                         // columns x0 - 4 .. x0 + 7 of row yy
#pragma unroll
        for (int k = 0; k < 12; ++k) seg[k] = -1;
        if (yy >= 0 && yy < A.H && yy >= A.mask_row0 && yy < (long)A.mask_row0 + A.mask_rows) {
          const unsigned char* nrow = A.mask + (yy - A.mask_row0) * A.mask_pitch;
          if (LABELS) {
            const int* lrow = reinterpret_cast<const int*>(nrow);
#pragma unroll
            for (int k = 0; k < 12; ++k) {
              const long c = x0 - 4 + k;
              if (k >= 4 - h && k < 8 + h && c >= 0 && c < A.W) {
                const int L = lrow[c];
                seg[k] = L > 0 ? L : 0;
              }
            }
          } else {
            const int k0 = (int)max(4L - h, 4L - x0), k1 = (int)min(8L + h, 4L + A.W - x0);
            unsigned w[3];
            rd_load12(nrow + (x0 - 4), k0, k1, A.mask, A.mask_end, w);
#pragma unroll
            for (int k = 0; k < 12; ++k) {
              if (k >= k0 && k < k1) seg[k] = (int)rd_byte(w, k);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
          for (int dx = -RD_MAX_R; dx <= RD_MAX_R; ++dx) {
            const int adx = dx < 0 ? -dx : dx;
            if (adx <= h && (dx != 0 || dy != 0)) edge[j] = edge[j] || seg[4 + j + dx] != id[j];
          }
        }
      }
    }
    // ---- colours
    unsigned al[4], col[4];
    bool change = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      al[j] = 0; col[j] = 0;
      if (j < npx) {
        const bool e = edge[j] && id[j] != 0;
        int a = e ? A.edge_alpha : A.fill_alpha[ci[j]];
        a = a < 0 ? 0 : (a > 256 ? 256 : a);
        al[j] = (unsigned)a;
        if (a != 0) {
          change = true;
          if (e && A.edge_rgb >= 0) {
            col[j] = (unsigned)A.edge_rgb;
          } else {
            const unsigned char* pc = A.palette + 3 * ci[j];
            col[j] = ((unsigned)pc[0] << 16) | ((unsigned)pc[1] << 8) | (unsigned)pc[2];
          }
        }
      }
    }
    if (!change && A.inplace) continue;                      // out is base: nothing to write
    const unsigned char* bp = A.base + yl * A.base_pitch + x0 * 3;
    unsigned b[3], v[12], o[3];
    rd_load12(bp, 0, 3 * npx, A.base, A.base_end, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[3 * j + c] = rd_mix(rd_byte(b, 3 * j + c), (col[j] >> (8 * (2 - c))) & 255u, al[j]);
    }
    rd_pack(v, o);
    rd_store12(A.out + yl * A.out_pitch + x0 * 3, npx, o);
  }
}

// ---- heat map -----------------------------------------------------------------------------------------------------------
// floor(n / den) for den > 0, |n| < 2^62, |n / den| < 2^32 (warp.hip's wp_floor_div).
__device__ __forceinline__ long rd_floor_div(long n, long den) {
  long q = (long)floor((double)n / (double)den);
  const long r = n - q * den;
  if (r < 0) --q;
  else if (r >= den) ++q;
  return q;
}

struct RdHeatArgs {
  const unsigned char* base;
  const unsigned char* base_end;
  long base_pitch;
  const int* Q;
  const unsigned char* lut;                                  // [256][3]
  unsigned char* out;
  long out_pitch;
  int row0, rows, H, W, cell, Gy, Gx, alpha, min_index, inplace;
  long nchunk, tiles;
};

template <int SMOOTH>
__global__ __launch_bounds__(256) void rd_heat_kernel(const RdHeatArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const long span = 2L * A.cell;
  const double spand = (double)span, dend = spand * spand, invd = 1.0 / dend;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long rg = t / A.nchunk, chunk = t - rg * A.nchunk;
    const long yl = rg * RD_WAVES + wave;
    const long x0 = chunk * RD_PX + 4L * lane;
    if (yl >= A.rows || x0 >= A.W) continue;
    const long y = (long)A.row0 + yl;
    const int npx = (int)min(4L, (long)A.W - x0);
    int idx[4] = {0, 0, 0, 0};
    if (SMOOTH) {
      // ---- the row axis, shared by the wave
      long gy0 = 0, gy1 = 0, wy = 0;
      if (A.Gy >= 2) {
        const long u = 2 * y + 1 - A.cell;
        gy0 = u < 0 ? 0 : (long)((unsigned)u / (unsigned)span);
        gy0 = gy0 > A.Gy - 2 ? A.Gy - 2 : gy0;
        gy1 = gy0 + 1;
        wy = u - gy0 * span;
        wy = wy < 0 ? 0 : (wy > span ? span : wy);
      }
      const int* f0 = A.Q + gy0 * A.Gx;
      const int* f1 = A.Q + gy1 * A.Gx;
      // ---- the column axis: the unclamped node index g and remainder r of the lane's first pixel, then steps of 2
      long g = 0, r = 0;
      if (A.Gx >= 2) {
        const long u = 2 * x0 + 1 - A.cell;                  // > -span
        g = u < 0 ? -1 : (long)((unsigned)u / (unsigned)span);
        r = u - g * span;
      }
      long cur = -1;
      int d00 = 0, d01 = 0, d10 = 0, d11 = 0;
      bool f64 = false;
      double v0 = 0.0, v1 = 0.0;                             // the vertical blends of the two node columns
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < npx) {
          long gx0 = 0, gx1 = 0, wx = 0;
          if (A.Gx >= 2) {
            gx0 = g < 0 ? 0 : (g > A.Gx - 2 ? A.Gx - 2 : g);
            gx1 = gx0 + 1;
            wx = r + (g - gx0) * span;
            wx = wx < 0 ? 0 : (wx > span ? span : wx);
            r += 2;
            if (r >= span) { r -= span; ++g; }
          }
          if (gx0 != cur) {
            cur = gx0;
            d00 = f0[gx0]; d01 = f0[gx1]; d10 = f1[gx0]; d11 = f1[gx1];
            const int lo = min(min(d00, d01), min(d10, d11)), hi = max(max(d00, d01), max(d10, d11));
            f64 = lo >= -RD_F64_NODE && hi <= RD_F64_NODE;
            if (f64) {
              const double a = (double)(span - wy), b = (double)wy;
              v0 = a * (double)d00 + b * (double)d10; v1 = a * (double)d01 + b * (double)d11;
            }
          }
          long d;
          if (f64) {                                         // exact: every product and sum an integer below 2^53
            const double x = (spand - (double)wx) * v0 + (double)wx * v1 + 0.5 * dend;
            double q = floor(x * invd);
            const double rem = fma(-q, dend, x);
            if (rem < 0.0) q -= 1.0;
            else if (rem >= dend) q += 1.0;
            d = (long)q;
          } else {
            const long top = (span - wx) * d00 + wx * d01, bot = (span - wx) * d10 + wx * d11;
            d = rd_floor_div((span - wy) * top + wy * bot + span * span / 2, span * span);
          }
          d = d < 0 ? 0 : (d > RD_DMAX ? RD_DMAX : d);
          idx[k] = (int)((d + 128) >> 8);
        }
      }
    } else {
      long gy = (long)((unsigned)y / (unsigned)A.cell);
      gy = gy > A.Gy - 1 ? A.Gy - 1 : gy;
      const int* f0 = A.Q + gy * A.Gx;
      long g = (long)((unsigned)x0 / (unsigned)A.cell);
      long r = x0 - g * A.cell;
      long cur = -1;
      int d = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < npx) {
          const long gx = g > A.Gx - 1 ? A.Gx - 1 : g;
          if (gx != cur) {
            cur = gx;
            d = f0[gx];
            d = d < 0 ? 0 : (d > RD_DMAX ? RD_DMAX : d);
          }
          idx[k] = (d + 128) >> 8;
          if (++r >= A.cell) { r = 0; ++g; }
        }
      }
    }
    bool change = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) change = change || (k < npx && idx[k] >= A.min_index);
    if (!change && A.inplace) continue;
    const unsigned char* bp = A.base + yl * A.base_pitch + x0 * 3;
    unsigned b[3], v[12], o[3];
    rd_load12(bp, 0, 3 * npx, A.base, A.base_end, b);
    int have = -1;
    unsigned c0 = 0, c1 = 0, c2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool on = k < npx && idx[k] >= A.min_index;
      if (on && idx[k] != have) {
        have = idx[k];
        const unsigned char* pc = A.lut + 3 * have;
        c0 = pc[0]; c1 = pc[1]; c2 = pc[2];
      }
      const unsigned a = on ? (unsigned)A.alpha : 0u;
      v[3 * k] = rd_mix(rd_byte(b, 3 * k), c0, a);
      v[3 * k + 1] = rd_mix(rd_byte(b, 3 * k + 1), c1, a);
      v[3 * k + 2] = rd_mix(rd_byte(b, 3 * k + 2), c2, a);
    }
    rd_pack(v, o);
    rd_store12(A.out + yl * A.out_pitch + x0 * 3, npx, o);
  }
}

// ---- comparison ---------------------------------------------------------------------------------------------------------
struct RdCompareArgs {
  const unsigned char* a;
  const unsigned char* a_end;
  long a_pitch;
  const unsigned char* b;
  const unsigned char* b_end;
  long b_pitch;
  unsigned char* out;
  long out_pitch;
  int row0, rows, H, W, mode, cell, alpha, gain;
  long nchunk, tiles;
};

__global__ __launch_bounds__(256) void rd_compare_kernel(const RdCompareArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long rg = t / A.nchunk, chunk = t - rg * A.nchunk;
    const long yl = rg * RD_WAVES + wave;
    const long x0 = chunk * RD_PX + 4L * lane;
    if (yl >= A.rows || x0 >= A.W) continue;
    const long y = (long)A.row0 + yl;
    const int npx = (int)min(4L, (long)A.W - x0);
    bool sel[4] = {false, false, false, false};              // mode 0: the pixel is b's
    bool need_a = true, need_b = true;
    if (A.mode == 0) {
      const unsigned cy = (unsigned)y / (unsigned)A.cell;    // wave-uniform
      unsigned g = (unsigned)x0 / (unsigned)A.cell;
      long r = x0 - (long)g * A.cell;
      need_a = false; need_b = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < npx) {
          sel[k] = ((cy + g) & 1u) != 0;
          need_a = need_a || !sel[k];
          need_b = need_b || sel[k];
          if (++r >= A.cell) { r = 0; ++g; }
        }
      }
    }
    unsigned ta[3] = {0, 0, 0}, tb[3] = {0, 0, 0}, v[12], o[3];
    if (need_a) rd_load12(A.a + yl * A.a_pitch + x0 * 3, 0, 3 * npx, A.a, A.a_end, ta);
    if (need_b) rd_load12(A.b + yl * A.b_pitch + x0 * 3, 0, 3 * npx, A.b, A.b_end, tb);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const unsigned pa = rd_byte(ta, i), pb = rd_byte(tb, i);
      if (A.mode == 0) {
        v[i] = sel[i / 3] ? pb : pa;
      } else if (A.mode == 1) {
        v[i] = rd_mix(pa, pb, (unsigned)A.alpha);
      } else {
        const unsigned d = (pa > pb ? pa - pb : pb - pa) * (unsigned)A.gain;
        v[i] = d > 255u ? 255u : d;
      }
    }
    rd_pack(v, o);
    rd_store12(A.out + yl * A.out_pitch + x0 * 3, npx, o);
  }
}

// ---- thumbnails ---------------------------------------------------------------------------------------------------------
struct RdBoxArgs {
  const unsigned char* src;                                  // row src_row0
  const unsigned char* src_end;
  long src_pitch;
  unsigned char* out;                                        // output row row0
  long out_pitch;
  int src_row0, row0, rows, H, W, Wo, f;
  long nchunk, tiles;
};

// A lane owns four consecutive output pixels: 4 f consecutive source columns of f source rows.  Image: a block row is
// walked four source pixels (12 bytes) at a time.  Mask: four bytes at a time.
template <int C>
__global__ __launch_bounds__(256) void rd_box_kernel(const RdBoxArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long rg = t / A.nchunk, chunk = t - rg * A.nchunk;
    const long yl = rg * RD_WAVES + wave;
    const long x0 = chunk * RD_PX + 4L * lane;               // output column
    if (yl >= A.rows || x0 >= A.Wo) continue;
    const long Y = (long)A.row0 + yl;                        // output row
    const int npx = (int)min(4L, (long)A.Wo - x0);
    const long sy0 = Y * A.f;
    const int nh = (int)min((long)A.f, (long)A.H - sy0);     // source rows of the block inside the region
    const unsigned char* srow = A.src + (sy0 - A.src_row0) * A.src_pitch;
    if (C == 3) {
      unsigned char* op = A.out + yl * A.out_pitch + x0 * 3;
      unsigned o[3];
      if (A.f == 1) {                                        // a copy
        rd_load12(srow + x0 * 3, 0, 3 * npx, A.src, A.src_end, o);
        rd_store12(op, npx, o);
        continue;
      }
      unsigned v[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[3 * j] = 0; v[3 * j + 1] = 0; v[3 * j + 2] = 0;
        if (j < npx) {
          const long sx0 = (x0 + j) * A.f;
          const int nw = (int)min((long)A.f, (long)A.W - sx0);
          unsigned s0 = 0, s1 = 0, s2 = 0;
          for (int dy = 0; dy < nh; ++dy) {
            const unsigned char* p = srow + dy * A.src_pitch + sx0 * 3;
            for (int c = 0; c < nw; c += 4) {
              const int n = min(4, nw - c);
              unsigned w[3];
              rd_load12(p + 3 * c, 0, 3 * n, A.src, A.src_end, w);
              rd_keep(w, 3 * n);
              s0 += rd_byte(w, 0) + rd_byte(w, 3) + rd_byte(w, 6) + rd_byte(w, 9);
              s1 += rd_byte(w, 1) + rd_byte(w, 4) + rd_byte(w, 7) + rd_byte(w, 10);
              s2 += rd_byte(w, 2) + rd_byte(w, 5) + rd_byte(w, 8) + rd_byte(w, 11);
            }
          }
          const unsigned n = (unsigned)nh * (unsigned)nw;    // <= 65536; 2 sum + n < 2^26
          v[3 * j] = (2u * s0 + n) / (2u * n);
          v[3 * j + 1] = (2u * s1 + n) / (2u * n);
          v[3 * j + 2] = (2u * s2 + n) / (2u * n);
        }
      }
      rd_pack(v, o);
      rd_store12(op, npx, o);
    } else {
      unsigned v[4] = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < npx) {
          const long sx0 = (x0 + j) * A.f;
          const int nw = (int)min((long)A.f, (long)A.W - sx0);
          unsigned m = 0;
          for (int dy = 0; dy < nh; ++dy) {
            const unsigned char* p = srow + dy * A.src_pitch + sx0;
            for (int c = 0; c < nw; c += 4) {
              const int n = min(4, nw - c);
              unsigned w = rd_load4(p + c, n, A.src, A.src_end);
              w = n >= 4 ? w : (w & ((1u << (8 * n)) - 1u));
              m = max(max(m, w & 255u), max(max((w >> 8) & 255u, (w >> 16) & 255u), w >> 24));
            }
          }
          v[j] = m;
        }
      }
      unsigned char* op = A.out + yl * A.out_pitch + x0;
      if (npx == 4 && ((uintptr_t)op & 3) == 0) {
        *reinterpret_cast<unsigned*>(op) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < npx) op[k] = (unsigned char)v[k];
        }
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
inline bool rd_bad_band(int H, int W, int row0, int rows) {
  return H < 1 || W < 1 || H > RD_MAX_SIDE || W > RD_MAX_SIDE || row0 < 0 || rows < 1 || rows > H - row0;
}

inline unsigned rd_grid(long W, long rows, long* nchunk, long* tiles) {
  *nchunk = (W + RD_PX - 1) / RD_PX;
  *tiles = *nchunk * ((rows + RD_WAVES - 1) / RD_WAVES);
  return (unsigned)(*tiles < RD_MAX_BLOCKS ? *tiles : RD_MAX_BLOCKS);
}

int rd_classes(bool labels, const void* base, long base_pitch, const void* mask, long mask_pitch, int mask_row0,
               int mask_rows, const void* palette, const int* fill_alpha, int r, int edge_alpha, int edge_rgb, int H, int W,
               int row0, int rows, void* out, long out_pitch, void* stream) {
  if (!base || !mask || !palette || !fill_alpha || !out) return S2S_ERR_NULL;
  if (rd_bad_band(H, W, row0, rows)) return S2S_ERR_SHAPE;
  if (r < 0 || r > RD_MAX_R || edge_alpha < 0 || edge_alpha > 256 || edge_rgb < -1 || edge_rgb > 0xFFFFFF) return S2S_ERR_SHAPE;
  if (mask_row0 < 0 || mask_rows < 1 || mask_rows > H - mask_row0) return S2S_ERR_SHAPE;
  const long lo = (long)row0 - r, hi = (long)row0 + rows + r;
  if (mask_row0 > (lo < 0 ? 0 : lo) || (long)mask_row0 + mask_rows < (hi > H ? (long)H : hi)) return S2S_ERR_SHAPE;
  const long rowb = 3L * W, mrowb = (labels ? 4L : 1L) * W;
  if (base_pitch < rowb || out_pitch < rowb || mask_pitch < mrowb) return S2S_ERR_SHAPE;
  if (labels && (mask_pitch % 4) != 0) return S2S_ERR_SHAPE;
  if (labels && ((uintptr_t)mask & 3) != 0) return S2S_ERR_ALIGN;
  RdClassArgs A;
  A.base = (const unsigned char*)base; A.base_pitch = base_pitch;
  A.base_end = A.base + (long)(rows - 1) * base_pitch + rowb;
  A.mask = (const unsigned char*)mask; A.mask_pitch = mask_pitch;
  A.mask_end = A.mask + (long)(mask_rows - 1) * mask_pitch + mrowb;
  A.palette = (const unsigned char*)palette; A.fill_alpha = fill_alpha;
  A.out = (unsigned char*)out; A.out_pitch = out_pitch;
  A.mask_row0 = mask_row0; A.mask_rows = mask_rows; A.row0 = row0; A.rows = rows; A.H = H; A.W = W; A.r = r;
  A.edge_alpha = edge_alpha; A.edge_rgb = edge_rgb;
  A.inplace = (out == base && out_pitch == base_pitch) ? 1 : 0;
  const unsigned blocks = rd_grid(W, rows, &A.nchunk, &A.tiles);
  if (labels) hipLaunchKernelGGL(rd_classes_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(rd_classes_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

// base, out: rows [row0, row0 + rows) of uint8 [H][W][3] regions, pitches in bytes, any pitch >= 3 W and any base
// alignment; out may be base itself (same pointer and pitch).  mask: rows [mask_row0, mask_row0 + mask_rows) of the uint8
// [H][W] class mask, any pitch >= W.  palette DEVICE uint8 [256][3], fill_alpha DEVICE int [256] (clamped to 0 .. 256 by
// the kernel); edge_rgb -1 (the palette colour) or 0xRRGGBB.  Shape status unless the mask rows present cover
// [max(0, row0 - r), min(H, row0 + rows + r)), for r outside 0 .. 4, edge_alpha outside 0 .. 256, H or W outside
// 1 .. 2^30, rows outside the region or a pitch smaller than a row.  One launch.
extern "C" int s2s_render_classes_u8(const void* base, long base_pitch, const void* mask, long mask_pitch, int mask_row0,
                                     int mask_rows, const void* palette, const int* fill_alpha, int r, int edge_alpha,
                                     int edge_rgb, int H, int W, int row0, int rows, void* out, long out_pitch,
                                     void* stream) {
  return rd_classes(false, base, base_pitch, mask, mask_pitch, mask_row0, mask_rows, palette, fill_alpha, r, edge_alpha,
                    edge_rgb, H, W, row0, rows, out, out_pitch, stream);
}

// The same from an int32 label image [H][W]: labels_pitch in bytes, a multiple of 4 and >= 4 W, the pointer dword-aligned
// (the alignment status otherwise).  Identity max(L, 0); colour index 0 for L <= 0, else ((L - 1) mod 255) + 1.
extern "C" int s2s_render_labels_u8(const void* base, long base_pitch, const int* labels, long labels_pitch, int labels_row0,
                                    int labels_rows, const void* palette, const int* fill_alpha, int r, int edge_alpha,
                                    int edge_rgb, int H, int W, int row0, int rows, void* out, long out_pitch,
                                    void* stream) {
  return rd_classes(true, base, base_pitch, labels, labels_pitch, labels_row0, labels_rows, palette, fill_alpha, r,
                    edge_alpha, edge_rgb, H, W, row0, rows, out, out_pitch, stream);
}

// base, out as above.  Q DEVICE int [Gy][Gx], any values (the kernel clamps d to 0 .. 65280); lut DEVICE uint8 [256][3].
// Shape status for cell outside 1 .. 2^14, Gy not in {H / cell, ceil(H / cell)} or below 1 (Gx alike), Gy Gx > 65536,
// alpha or min_index outside 0 .. 256, smooth not 0 or 1, and the region conditions above.  One launch.
extern "C" int s2s_render_heat_u8(const void* base, long base_pitch, const int* Q, int Gy, int Gx, int cell, const void* lut,
                                  int alpha, int min_index, int smooth, int H, int W, int row0, int rows, void* out,
                                  long out_pitch, void* stream) {
  if (!base || !Q || !lut || !out) return S2S_ERR_NULL;
  if (rd_bad_band(H, W, row0, rows)) return S2S_ERR_SHAPE;
  if (cell < 1 || cell > RD_MAX_CELL) return S2S_ERR_SHAPE;
  if (Gy < 1 || Gx < 1 || (long)Gy * Gx > RD_MAX_NODES) return S2S_ERR_SHAPE;
  if ((Gy != H / cell && Gy != (H + cell - 1) / cell) || (Gx != W / cell && Gx != (W + cell - 1) / cell)) return S2S_ERR_SHAPE;
  if (alpha < 0 || alpha > 256 || min_index < 0 || min_index > 256 || smooth < 0 || smooth > 1) return S2S_ERR_SHAPE;
  const long rowb = 3L * W;
  if (base_pitch < rowb || out_pitch < rowb) return S2S_ERR_SHAPE;
  RdHeatArgs A;
  A.base = (const unsigned char*)base; A.base_pitch = base_pitch;
  A.base_end = A.base + (long)(rows - 1) * base_pitch + rowb;
  A.Q = Q; A.lut = (const unsigned char*)lut;
  A.out = (unsigned char*)out; A.out_pitch = out_pitch;
  A.row0 = row0; A.rows = rows; A.H = H; A.W = W; A.cell = cell; A.Gy = Gy; A.Gx = Gx; A.alpha = alpha;
  A.min_index = min_index;
  A.inplace = (out == base && out_pitch == base_pitch) ? 1 : 0;
  const unsigned blocks = rd_grid(W, rows, &A.nchunk, &A.tiles);
  if (smooth) hipLaunchKernelGGL(rd_heat_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(rd_heat_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// a, b, out: rows [row0, row0 + rows) of three uint8 [H][W][3] regions.  mode 0 checkerboard of cell x cell squares
// (a where (y / cell + x / cell) is even), 1 mix(a, b, alpha), 2 min(255, |a - b| gain).  Shape status for mode outside
// 0 .. 2, cell outside 1 .. 2^30, alpha outside 0 .. 256, gain outside 1 .. 255 (each whatever the mode), and the region
// conditions above.  One launch.
extern "C" int s2s_render_compare_u8(const void* a, long a_pitch, const void* b, long b_pitch, int mode, int cell, int alpha,
                                     int gain, int H, int W, int row0, int rows, void* out, long out_pitch, void* stream) {
  if (!a || !b || !out) return S2S_ERR_NULL;
  if (rd_bad_band(H, W, row0, rows)) return S2S_ERR_SHAPE;
  if (mode < 0 || mode > 2 || cell < 1 || cell > RD_MAX_SIDE || alpha < 0 || alpha > 256 || gain < 1 || gain > 255) return S2S_ERR_SHAPE;
  const long rowb = 3L * W;
  if (a_pitch < rowb || b_pitch < rowb || out_pitch < rowb) return S2S_ERR_SHAPE;
  RdCompareArgs A;
  A.a = (const unsigned char*)a; A.a_pitch = a_pitch; A.a_end = A.a + (long)(rows - 1) * a_pitch + rowb;
  A.b = (const unsigned char*)b; A.b_pitch = b_pitch; A.b_end = A.b + (long)(rows - 1) * b_pitch + rowb;
  A.out = (unsigned char*)out; A.out_pitch = out_pitch;
  A.row0 = row0; A.rows = rows; A.H = H; A.W = W; A.mode = mode; A.cell = cell; A.alpha = alpha; A.gain = gain;
  const unsigned blocks = rd_grid(W, rows, &A.nchunk, &A.tiles);
  hipLaunchKernelGGL(rd_compare_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// src: rows [src_row0, src_row0 + src_rows) of a uint8 [H][W][C] region, C = 3 (box average, floor((2 sum + n) / (2 n))
// over the n pixels of the block inside the region) or 1 (box maximum); out: rows [row0, row0 + rows) of the uint8
// [ceil(H / f)][ceil(W / f)][C] result.  Shape status unless the source rows present cover [row0 f, min(H, (row0 + rows)
// f)), for f outside 1 .. 256, C not 1 or 3, H or W outside 1 .. 2^30, output rows outside the result or a pitch
// smaller than a row.  One launch.
extern "C" int s2s_box_down_u8(const void* src, long src_pitch, int src_row0, int src_rows, int H, int W, int C, int f,
                               int row0, int rows, void* out, long out_pitch, void* stream) {
  if (!src || !out) return S2S_ERR_NULL;
  if (C != 1 && C != 3) return S2S_ERR_SHAPE;
  if (H < 1 || W < 1 || H > RD_MAX_SIDE || W > RD_MAX_SIDE || f < 1 || f > RD_MAX_F) return S2S_ERR_SHAPE;
  const int Ho = (H + f - 1) / f, Wo = (W + f - 1) / f;
  if (row0 < 0 || rows < 1 || rows > Ho - row0) return S2S_ERR_SHAPE;
  if (src_row0 < 0 || src_rows < 1 || src_rows > H - src_row0) return S2S_ERR_SHAPE;
  const long lo = (long)row0 * f, hi = ((long)row0 + rows) * f;
  if (src_row0 > lo || (long)src_row0 + src_rows < (hi > H ? (long)H : hi)) return S2S_ERR_SHAPE;
  if (src_pitch < (long)W * C || out_pitch < (long)Wo * C) return S2S_ERR_SHAPE;
  RdBoxArgs A;
  A.src = (const unsigned char*)src; A.src_pitch = src_pitch;
  A.src_end = A.src + (long)(src_rows - 1) * src_pitch + (long)W * C;
  A.out = (unsigned char*)out; A.out_pitch = out_pitch;
  A.src_row0 = src_row0; A.row0 = row0; A.rows = rows; A.H = H; A.W = W; A.Wo = Wo; A.f = f;
  const unsigned blocks = rd_grid(Wo, rows, &A.nchunk, &A.tiles);
  if (C == 3) hipLaunchKernelGGL(rd_box_kernel<3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(rd_box_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
