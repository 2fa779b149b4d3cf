// Dense region alignment: a measured shift field is cleaned on the device, interpolated to a sub-pixel displacement
// per pixel and the target region (or a mask) is resampled through it.  DESIGN.md section 3.22.
//
//   s2s_field_clean      outlier rejection against the neighbours' lower median, then a Jacobi fill of every cell
//                        without a usable shift from its known neighbours; one workgroup
//   s2s_warp_region_u8   the hot kernel: out[y][x] = the region sampled at (y, x) + d(y, x), bilinear for images,
//                        nearest for masks, a fill outside the region; one launch per band of output rows
//
// Units and arithmetic (normative; restated in include/stain2stain_hip.h).  A displacement is in 1/16 pixel.  A field is
// D int [Gy][Gx][2] = (dy, dx); node (gy, gx) is the centre of cell (gy, gx) of the H x W region, Gy = H / cell, Gx =
// W / cell.  In doubled coordinates span = 2 cell; per axis u = 2 p + 1 - cell; for G >= 2: g0 = clamp(floor(u / span),
// 0, G - 2), g1 = g0 + 1, w = clamp(u - g0 span, 0, span); for G = 1: g0 = g1 = 0, w = 0.  In 64 bits
//   num = (span - wy) ((span - wx) D[y0][x0] + wx D[y0][x1]) + wy ((span - wx) D[y1][x0] + wx D[y1][x1])
//   d   = clamp(floor((num + span^2 / 2) / span^2), -16 max_shift, 16 max_shift)        per component.
// With cell <= 2^14 and any int32 node, |num| < 2^30 * 2^31: no overflow.  The clamp is applied here, so no field
// content moves a read further than max_shift + 1 rows or columns from its pixel, which is what the entry point has
// validated against the rows present.
//
// The warp kernel.  A wave owns 256 consecutive pixels of one output row, a lane four of them; a workgroup is four
// waves on four consecutive rows.  The row index is wave-uniform, so y0, y1, wy and span - wy live in scalar registers.
// The x axis is walked incrementally (one division per lane, not per pixel).  The field nodes are read straight from
// memory, and only when a lane's node column changes: a wave touches 256 / cell + 2 node columns of two node rows (48
// bytes at cell 256), a whole field is at most 512 KiB, so they stay in the vector L1 / L2 and staging them in LDS would
// add a barrier to save nothing.
//
// The displacement.  Where the four nodes lie within +-2^20 (every field a search can produce: the clamp is at 2^14) the
// blend runs in float64, where it is exact: the vertical blends are below 2^35, num + span^2 / 2 below 2^51, every
// product and sum an integer below 2^53; the quotient is estimated with a reciprocal and settled by one exact
// fma remainder.  Other nodes take the same formula in int64.  Both give the floor of the definition.
//
// The gather.  An image lane whose four pixels read four consecutive source columns of one source row pair, all
// inside the rows present (the common case: the displacement changes by less than a pixel over four pixels), loads the
// 15 bytes of each of the two rows as five aligned dwords and rebuilds them with v_alignbyte_b32, where those dwords lie
// inside the source buffer; any other lane (borders, ragged ends, a field that tears) reads its taps byte by byte with
// the fill test.  12 output bytes go out as three dwords where the address allows, bytes otherwise; a mask lane stores
// one dword.  All index arithmetic is 64-bit.
//
// Nothing here allocates, synchronises or reads back to the host.
#include "common.h"

namespace {

constexpr int WP_MAX_SHIFT = 1024;
constexpr int WP_MAX_CELLS = 65536;
constexpr int WP_MAX_CELL = 1 << 14;                         // span^2 * 2^31 stays below 2^62
constexpr int WP_WAVES = 4;                                  // output rows per workgroup
constexpr int WP_PX = 256;                                   // pixels of a row per wave: 64 lanes x 4
constexpr long WP_MAX_BLOCKS = 65536;
constexpr int WP_CLEAN_THREADS = 1024;

// floor(n / den) for den > 0, |n| < 2^62, |n / den| < 2^32: the float64 quotient is within one of the truth (relative
// error 2^-52 of a quotient below 2^32), one exact correction step each way settles it.
__device__ __forceinline__ long wp_floor_div(long n, long den) {
  long q = (long)floor((double)n / (double)den);
  const long r = n - q * den;
  if (r < 0) --q;
  else if (r >= den) ++q;
  return q;
}

// One displacement component at blend weights (span - wx, wx) x (span - wy, wy), clamped to +-lim.
__device__ __forceinline__ long wp_blend(long d00, long d01, long d10, long d11, long wx, long wy, long span, long lim) {
  const long top = (span - wx) * d00 + wx * d01, bot = (span - wx) * d10 + wx * d11;
  const long num = (span - wy) * top + wy * bot;
  const long d = wp_floor_div(num + span * span / 2, span * span);
  return d < -lim ? -lim : (d > lim ? lim : d);
}

constexpr int WP_F64_NODE = 1 << 20;                         // nodes within this take the float64 blend

// The same from the two vertical blends v0, v1 (integers below 2^35 held in float64) at the integer weight wx:
// x = (span - wx) v0 + wx v1 + span^2 / 2 is an exact integer below 2^51; q = floor(x inv) is within one of floor(x /
// den) (|q| <= 2^21, relative error 2^-51); r = x - q den is exact in one fma.
__device__ __forceinline__ long wp_blend_f64(double v0, double v1, double wx, double span, double den, double inv,
                                             double lim) {
  const double x = (span - wx) * v0 + wx * v1 + 0.5 * den;
  double q = floor(x * inv);
  const double r = fma(-q, den, x);
  if (r < 0.0) q -= 1.0;
  else if (r >= den) q += 1.0;
  return (long)fmin(fmax(q, -lim), lim);
}

struct WpArgs {
  const unsigned char* src;                                  // row src_row0 of the region
  const unsigned char* src_end;                              // one past the last byte of the last row present
  long src_pitch;
  const int* field;
  unsigned char* out;                                        // row row0 of the result
  long out_pitch;
  int row_lo, row_hi;                                        // region rows that may be read: present and inside [0, H)
  int src_row0, row0, rows, H, W, cell, Gy, Gx, max_shift;
  unsigned fill;
  long nchunk, tiles;
};

template <int C>
__global__ __launch_bounds__(256) void wp_warp_kernel(const WpArgs A) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const long span = 2L * A.cell, lim = 16L * A.max_shift;
  const double spand = (double)span, dend = spand * spand, invd = 1.0 / dend, limd = (double)lim;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long rg = t / A.nchunk, chunk = t - rg * A.nchunk;
    const long yl = rg * WP_WAVES + wave;                    // row of this launch's band: wave-uniform
    const long x0 = chunk * WP_PX + 4L * lane;
    if (yl >= A.rows || x0 >= A.W) continue;
    const long y = (long)A.row0 + yl;
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
    const int* f0 = A.field + 2 * gy0 * A.Gx;
    const int* f1 = A.field + 2 * gy1 * A.Gx;
    // ---- the column axis: the unclamped node index g and remainder r of the lane's first pixel, then steps of 2
    long g = 0, r = 0;
    if (A.Gx >= 2) {
      const long u = 2 * x0 + 1 - A.cell;                    // > -span
      g = u < 0 ? -1 : (long)((unsigned)u / (unsigned)span);
      r = u - g * span;
    }
    const int npx = (int)min(4L, (long)A.W - x0);
    unsigned v[4 * C];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) v[k] = A.fill;
    // ---- the sample position of every pixel, in 1/16 px
    long sys[4] = {0, 0, 0, 0}, sxs[4] = {0, 0, 0, 0};
    long cur = -1;                                           // the node column the registers below hold
    int2 d00 = {0, 0}, d01 = {0, 0}, d10 = {0, 0}, d11 = {0, 0};
    bool f64 = false;
    double v0y = 0.0, v1y = 0.0, v0x = 0.0, v1x = 0.0;       // the vertical blends of the two node columns
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
          d00 = *reinterpret_cast<const int2*>(f0 + 2 * gx0); d01 = *reinterpret_cast<const int2*>(f0 + 2 * gx1);
          d10 = *reinterpret_cast<const int2*>(f1 + 2 * gx0); d11 = *reinterpret_cast<const int2*>(f1 + 2 * gx1);
          const int lo = min(min(min(d00.x, d00.y), min(d01.x, d01.y)), min(min(d10.x, d10.y), min(d11.x, d11.y)));
          const int hi = max(max(max(d00.x, d00.y), max(d01.x, d01.y)), max(max(d10.x, d10.y), max(d11.x, d11.y)));
          f64 = lo >= -WP_F64_NODE && hi <= WP_F64_NODE;
          if (f64) {
            const double a = (double)(span - wy), b = (double)wy;
            v0y = a * (double)d00.x + b * (double)d10.x; v1y = a * (double)d01.x + b * (double)d11.x;
            v0x = a * (double)d00.y + b * (double)d10.y; v1x = a * (double)d01.y + b * (double)d11.y;
          }
        }
        if (f64) {
          sys[k] = 16 * y + wp_blend_f64(v0y, v1y, (double)wx, spand, dend, invd, limd);
          sxs[k] = 16 * (x0 + k) + wp_blend_f64(v0x, v1x, (double)wx, spand, dend, invd, limd);
        } else {
          sys[k] = 16 * y + wp_blend(d00.x, d01.x, d10.x, d11.x, wx, wy, span, lim);
          sxs[k] = 16 * (x0 + k) + wp_blend(d00.y, d01.y, d10.y, d11.y, wx, wy, span, lim);
        }
      }
    }
    // ---- the wide gather: four consecutive source columns of one row pair, whole dwords inside the buffer
    bool wide = false;
    if (C == 3) {
      const long iy = sys[0] >> 4, ix = sxs[0] >> 4;
      wide = npx == 4 && (sys[1] >> 4) == iy && (sys[2] >> 4) == iy && (sys[3] >> 4) == iy && (sxs[1] >> 4) == ix + 1 &&
             (sxs[2] >> 4) == ix + 2 && (sxs[3] >> 4) == ix + 3 && iy >= A.row_lo && iy + 1 < A.row_hi && ix >= 0 &&
             ix + 4 < A.W;
      const unsigned char* p0 = A.src + (iy - A.src_row0) * A.src_pitch + ix * 3;     // dereferenced only when wide
      const unsigned char* p1 = p0 + A.src_pitch;
      const unsigned o0 = (unsigned)((uintptr_t)p0 & 3), o1 = (unsigned)((uintptr_t)p1 & 3);
      const unsigned char* q0 = p0 - o0;
      const unsigned char* q1 = p1 - o1;                     // q0 <= q1: a row is at least 3 bytes
      wide = wide && q0 >= A.src && q1 + 20 <= A.src_end;
      if (wide) {
        unsigned t0[4], t1[4];                               // bytes p0[0 .. 16) and p1[0 .. 16); 15 are used
        {
          const unsigned* u0 = reinterpret_cast<const unsigned*>(q0);
          const unsigned* u1 = reinterpret_cast<const unsigned*>(q1);
          const unsigned a0 = u0[0], a1 = u0[1], a2 = u0[2], a3 = u0[3], a4 = u0[4];
          const unsigned b0 = u1[0], b1 = u1[1], b2 = u1[2], b3 = u1[3], b4 = u1[4];
          t0[0] = __builtin_amdgcn_alignbyte(a1, a0, o0); t0[1] = __builtin_amdgcn_alignbyte(a2, a1, o0);
          t0[2] = __builtin_amdgcn_alignbyte(a3, a2, o0); t0[3] = __builtin_amdgcn_alignbyte(a4, a3, o0);
          t1[0] = __builtin_amdgcn_alignbyte(b1, b0, o1); t1[1] = __builtin_amdgcn_alignbyte(b2, b1, o1);
          t1[2] = __builtin_amdgcn_alignbyte(b3, b2, o1); t1[3] = __builtin_amdgcn_alignbyte(b4, b3, o1);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned fy = (unsigned)(sys[k] & 15), fx = (unsigned)(sxs[k] & 15);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int i = 3 * k + c, j = i + 3;
            const unsigned p00 = (t0[i >> 2] >> (8 * (i & 3))) & 255u, p01 = (t0[j >> 2] >> (8 * (j & 3))) & 255u;
            const unsigned p10 = (t1[i >> 2] >> (8 * (i & 3))) & 255u, p11 = (t1[j >> 2] >> (8 * (j & 3))) & 255u;
            v[i] = ((16u - fy) * ((16u - fx) * p00 + fx * p01) + fy * ((16u - fx) * p10 + fx * p11) + 128u) >> 8;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < npx && !wide) {
        const long sy = sys[k], sx = sxs[k];
        if (C == 1) {
          const long iy = (sy + 8) >> 4, ix = (sx + 8) >> 4;
          if (iy >= A.row_lo && iy < A.row_hi && ix >= 0 && ix < A.W) v[k] = A.src[(iy - A.src_row0) * A.src_pitch + ix];
        } else {
          const long iy = sy >> 4, ix = sx >> 4;
          const unsigned fy = (unsigned)(sy & 15), fx = (unsigned)(sx & 15);
          const bool r0 = iy >= A.row_lo && iy < A.row_hi, r1 = iy + 1 >= A.row_lo && iy + 1 < A.row_hi;
          const bool c0 = ix >= 0 && ix < A.W, c1 = ix + 1 >= 0 && ix + 1 < A.W;
          const unsigned char* p0 = A.src + (iy - A.src_row0) * A.src_pitch + ix * 3;
          const unsigned char* p1 = p0 + A.src_pitch;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const unsigned p00 = (r0 && c0) ? p0[c] : A.fill, p01 = (r0 && c1) ? p0[3 + c] : A.fill;
            const unsigned p10 = (r1 && c0) ? p1[c] : A.fill, p11 = (r1 && c1) ? p1[3 + c] : A.fill;
            v[3 * k + c] = ((16u - fy) * ((16u - fx) * p00 + fx * p01) + fy * ((16u - fx) * p10 + fx * p11) + 128u) >> 8;
          }
        }
      }
    }
    unsigned char* o = A.out + yl * A.out_pitch + x0 * C;
    if (npx == 4 && ((uintptr_t)o & 3) == 0) {
#pragma unroll
      for (int q = 0; q < C; ++q)
        reinterpret_cast<unsigned*>(o)[q] = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4 * C; ++k) {
        if (k < npx * C) o[k] = (unsigned char)v[k];
      }
    }
  }
}

// ---- cleaning ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool wp_reliable(const int* shift, const unsigned char* reliable, long c, int max_shift) {
  const int dy = shift[2 * c], dx = shift[2 * c + 1];
  return reliable[c] != 0 && dy >= -max_shift && dy <= max_shift && dx >= -max_shift && dx <= max_shift;
}

// Element (n - 1) / 2 of the sorted valid values among v[0..8): the one with at most k values below it and more than k
// values not above it.  Static indexing only, so everything stays in registers.
__device__ __forceinline__ int wp_lower_median(const int (&v)[8], const bool (&ok)[8], int n) {
  const int k = (n - 1) / 2;
  int med = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int lt = 0, le = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lt += (ok[j] && v[j] < v[i]) ? 1 : 0;
      le += (ok[j] && v[j] <= v[i]) ? 1 : 0;
    }
    if (ok[i] && lt <= k && k < le) med = v[i];
  }
  return med;
}

// One workgroup.  work: int [2][G][3] = (dy, dx, known) of the two Jacobi states.  The workgroup barrier orders the
// global-memory states between iterations (one CU, one vector L1); nothing spins and the loop is counted.
__global__ __launch_bounds__(WP_CLEAN_THREADS) void wp_clean_kernel(const int* shift, const unsigned char* reliable, int Gy,
                                                                    int Gx, int max_dev, int max_shift, int* field,
                                                                    unsigned char* kept, int* stats, int* work) {
  __shared__ int s_kept, s_unknown[3];
  const int G = Gy * Gx, tid = threadIdx.x;
  if (tid == 0) { s_kept = 0; s_unknown[0] = 0; s_unknown[1] = 0; s_unknown[2] = 0; }
  __syncthreads();
  // ---- outliers, judged against the input state, and the seed
  int nk = 0, nu = 0;
  for (int c = tid; c < G; c += WP_CLEAN_THREADS) {
    const int gy = c / Gx, gx = c - gy * Gx;
    bool keep = wp_reliable(shift, reliable, c, max_shift);
    const int dy = shift[2L * c], dx = shift[2L * c + 1];
    if (keep) {
      int vy[8], vx[8];
      bool ok[8];
      int n = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int q = k < 4 ? k : k + 1;                     // the 3 x 3 neighbourhood without its centre
        const int ny = gy + q / 3 - 1, nx = gx + q % 3 - 1;
        ok[k] = false; vy[k] = 0; vx[k] = 0;
        if (ny >= 0 && ny < Gy && nx >= 0 && nx < Gx) {
          const long m = (long)ny * Gx + nx;
          if (wp_reliable(shift, reliable, m, max_shift)) {
            ok[k] = true; vy[k] = shift[2 * m]; vx[k] = shift[2 * m + 1];
            ++n;
          }
        }
      }
      if (n >= 3) {
        const int ey = abs(dy - wp_lower_median(vy, ok, n)), ex = abs(dx - wp_lower_median(vx, ok, n));
        if (max(ey, ex) > max_dev) keep = false;
      }
    }
    work[3L * c] = keep ? (int)(16u * (unsigned)dy) : 0;   // |dy| <= 1024 where kept
    work[3L * c + 1] = keep ? (int)(16u * (unsigned)dx) : 0;
    work[3L * c + 2] = keep ? 1 : 0;
    kept[c] = keep ? 1 : 0;
    nk += keep ? 1 : 0;
    nu += keep ? 0 : 1;
  }
  if (nk) atomicAdd(&s_kept, nk);
  if (nu) atomicAdd(&s_unknown[0], nu);
  __syncthreads();
  const int nkept = s_kept;
  int unknown = s_unknown[0];
  // ---- fill: Jacobi, each iteration reads the previous state; known cells spread one cell per iteration
  const int maxit = max(Gy, Gx);
  int it = 0, cur = 0;
  if (nkept > 0) {
    for (; it < maxit && unknown > 0; ++it) {
      const int* a = work + (cur ? 3L * G : 0L);
      int* b = work + (cur ? 0L : 3L * G);
      const int slot = (it + 1) % 3;
      if (tid == 0) s_unknown[(it + 2) % 3] = 0;               // last read before the previous barrier
      int left = 0;
      for (int c = tid; c < G; c += WP_CLEAN_THREADS) {
        int vy = a[3L * c], vx = a[3L * c + 1], known = a[3L * c + 2];
        if (!known) {
          const int gy = c / Gx, gx = c - gy * Gx;
          int n = 0, sy = 0, sx = 0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int q = k < 4 ? k : k + 1;
            const int ny = gy + q / 3 - 1, nx = gx + q % 3 - 1;
            if (ny >= 0 && ny < Gy && nx >= 0 && nx < Gx) {
              const long m = (long)ny * Gx + nx;
              if (a[3 * m + 2]) { sy += a[3 * m]; sx += a[3 * m + 1]; ++n; }
            }
          }
          if (n > 0) {                                       // floor((2 sum + n) / (2 n)); |sum| <= 8 * 16 * 1024
            const int ty = 2 * sy + n, tx = 2 * sx + n, den = 2 * n;
            vy = ty / den - ((ty % den) < 0 ? 1 : 0);
            vx = tx / den - ((tx % den) < 0 ? 1 : 0);
            known = 1;
          } else {
            ++left;
          }
        }
        b[3L * c] = vy; b[3L * c + 1] = vx; b[3L * c + 2] = known;
      }
      if (left) atomicAdd(&s_unknown[slot], left);
      __syncthreads();
      unknown = s_unknown[slot];
      cur ^= 1;
    }
  }
  const int* a = work + (cur ? 3L * G : 0L);
  for (int c = tid; c < G; c += WP_CLEAN_THREADS) {
    const bool known = nkept > 0 && a[3L * c + 2] != 0;
    field[2L * c] = known ? a[3L * c] : 0;
    field[2L * c + 1] = known ? a[3L * c + 1] : 0;
  }
  if (tid == 0) { stats[0] = nkept; stats[1] = it; }
}

}  // namespace

// shift: DEVICE int [Gy][Gx][2] in pixels; reliable: DEVICE uint8 [Gy][Gx]; a cell counts as reliable when its byte is
// not 0 and max(|dy|, |dx|) <= max_shift.  field: int [Gy][Gx][2] in 1/16 px; kept: uint8 [Gy][Gx]; stats: int [2] =
// cells kept, fill iterations run; work: int [6 Gy Gx], scratch.  Shape status for Gy Gx outside 1 .. 65536, max_shift
// outside 0 .. 1024 or max_dev < 0.  One launch of one workgroup.
extern "C" int s2s_field_clean(const int* shift, const void* reliable, int Gy, int Gx, int max_dev, int max_shift,
                               int* field, void* kept, int* stats, int* work, void* stream) {
  if (!shift || !reliable || !field || !kept || !stats || !work) return S2S_ERR_NULL;
  if (Gy < 1 || Gx < 1 || (long)Gy * Gx > WP_MAX_CELLS) return S2S_ERR_SHAPE;
  if (max_shift < 0 || max_shift > WP_MAX_SHIFT || max_dev < 0) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(wp_clean_kernel, dim3(1), dim3(WP_CLEAN_THREADS), 0, (hipStream_t)stream, shift,
                     (const unsigned char*)reliable, Gy, Gx, max_dev, max_shift, field, (unsigned char*)kept, stats, work);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// src: rows [src_row0, src_row0 + src_rows) of a uint8 [H][W][C] region, C = 3 (bilinear) or 1 (nearest), src_pitch in
// bytes, any pitch >= W C and any base alignment; field: DEVICE int [Gy][Gx][2] in 1/16 px, any values; out: rows
// [row0, row0 + rows) of the result, out_pitch in bytes.  Shape status when the rows present do not cover
// [max(0, row0 - max_shift - 1), min(H, row0 + rows + max_shift + 1)), when Gy != H / cell, Gx != W / cell, cell < 1 or
// cell > 2^14, Gy Gx outside 1 .. 65536, max_shift outside 0 .. 1024, or a pitch is smaller than a row.  One launch.
extern "C" int s2s_warp_region_u8(const void* src, long src_pitch, int src_row0, int src_rows, const int* field, int Gy,
                                  int Gx, int cell, int max_shift, int H, int W, int C, int fill, int row0, int rows,
                                  void* out, long out_pitch, void* stream) {
  if (!src || !field || !out) return S2S_ERR_NULL;
  if (C != 1 && C != 3) return S2S_ERR_SHAPE;
  if (H < 1 || W < 1 || H > (1 << 29) || W > (1 << 29) || fill < 0 || fill > 255) return S2S_ERR_SHAPE;
  if (cell < 1 || cell > WP_MAX_CELL || Gy != H / cell || Gx != W / cell) return S2S_ERR_SHAPE;
  if (Gy < 1 || Gx < 1 || (long)Gy * Gx > WP_MAX_CELLS) return S2S_ERR_SHAPE;
  if (max_shift < 0 || max_shift > WP_MAX_SHIFT) return S2S_ERR_SHAPE;
  if (row0 < 0 || rows < 1 || rows > H - row0) return S2S_ERR_SHAPE;
  if (src_row0 < 0 || src_rows < 1 || src_rows > H - src_row0) return S2S_ERR_SHAPE;
  const long lo = (long)row0 - max_shift - 1, hi = (long)row0 + rows + max_shift + 1;
  if (src_row0 > (lo < 0 ? 0 : lo) || (long)src_row0 + src_rows < (hi > H ? (long)H : hi)) return S2S_ERR_SHAPE;
  const long rowb = (long)W * C;
  if (src_pitch < rowb || out_pitch < rowb) return S2S_ERR_SHAPE;
  WpArgs A;
  A.src = (const unsigned char*)src; A.src_pitch = src_pitch; A.field = field;
  A.src_end = A.src + (long)(src_rows - 1) * src_pitch + rowb;
  A.out = (unsigned char*)out; A.out_pitch = out_pitch;
  A.row_lo = src_row0; A.row_hi = src_row0 + src_rows;
  A.src_row0 = src_row0; A.row0 = row0; A.rows = rows; A.H = H; A.W = W; A.cell = cell; A.Gy = Gy; A.Gx = Gx;
  A.max_shift = max_shift; A.fill = (unsigned)fill;
  A.nchunk = ((long)W + WP_PX - 1) / WP_PX;
  A.tiles = A.nchunk * (((long)rows + WP_WAVES - 1) / WP_WAVES);
  const unsigned blocks = (unsigned)(A.tiles < WP_MAX_BLOCKS ? A.tiles : WP_MAX_BLOCKS);
  if (C == 3) hipLaunchKernelGGL(wp_warp_kernel<3>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  else hipLaunchKernelGGL(wp_warp_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
