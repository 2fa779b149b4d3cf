// Rigid region pre-alignment: block-averaged structure maps of a whole region and a resampling of a region through a
// rotation about a centre plus a translation, optionally followed by the dense displacement of a shift field.
// DESIGN.md section 3.30.
//
//   s2s_structure_overview_u8   uint8 RGB -> the structure byte of section 3.21, averaged over ds x ds blocks, ds a power
//                               of two up to 64; one bandwidth-bound pass over the bytes
//   s2s_rigid_warp_u8           out[p] = tgt[C + R (p + d - C) + t], bilinear or nearest, a fill outside the region; one
//                               launch per band of output rows, a batch of transforms in one launch
//
// Units and arithmetic (normative; restated in include/stain2stain_hip.h).  A transform is six 64-bit integers
// (c, s, ty, tx, Cy, Cx): cosine and sine in Q24, the translation in 1/16 pixel, the doubled centre.  The kernel clamps c
// and s to +-2^24, ty and tx to +-2^36, Cy and Cx to +-2^24; H and W are at most 2^20.  For output pixel (y, x) with the
// displacement (dy, dx) in 1/16 pixel (0 without a field; with one, the dense displacement of section 3.22, clamped to
// +-16 max_shift), all in 64 bits:
//   Uy = 32 y + 2 dy - 16 Cy            Ux = 32 x + 2 dx - 16 Cx
//   Vy = c Uy - s Ux                    Vx = s Uy + c Ux
//   sy = ((Vy + Cy 2^28 + 2^24) >> 25) + ty       sx likewise with Cx, tx
// |U| < 2^29, so |V| < 2^54 and every intermediate stays below 2^55.  Sampling is that of warp.hip: bilinear taps at
// iy = sy >> 4, fy = sy & 15 with the fill for a tap outside, + 128 and >> 8; nearest (sy + 8) >> 4.  Every bounds test
// runs in 64 bits on the sample position itself, so whatever the six numbers hold no read leaves the rows present.
//
// The overview kernel.  A wave owns one row of blocks and 256 consecutive pixels of it, a lane four pixels: it loads the
// four aligned dwords that hold its 12 bytes of each of the ds rows (bytes at the ragged ends and at the ends of the
// buffer), rebuilds them with v_alignbyte_b32, and adds the four structure bytes to four vertical sums in a loop over
// the rows.  A block of ds >= 4 pixels is ds / 4 neighbouring lanes: the horizontal sum is taken inside the lane and
// then across lanes with shuffles.  Every block belongs to one wave, so nothing is combined in memory.  The q table is
// staged in LDS as rg_map_kernel stages it.
//
// The warp kernel.  A workgroup owns a tile of 16 output rows x 64 pixels, a wave four rows of it, a lane four
// consecutive pixels of one row: under a rotation the source footprint of the tile stays compact.  V is affine in x, so
// a lane takes it once with multiplies and steps it by (-32 s, 32 c) per pixel; a field adds 2 (c dy - s dx) and
// 2 (s dy + c dx), exact in integers.  The dense displacement restates warp.hip's definition in int64 per pixel (the
// float64 blend of warp.hip is not shared: that translation unit is untouched).  The gather and the stores are those of
// wp_warp_kernel: a lane whose four pixels read four consecutive columns of one row pair takes five aligned dwords of
// each row, any other lane reads its taps byte by byte with the fill test; 12 bytes go out as three dwords where the
// address allows.
//
// Nothing here allocates, synchronises or reads back to the host.
#include "common.h"

namespace {

constexpr int RD_MAX_DS = 64;                                 // 64^2 * 255 < 2^32
constexpr int RD_PX = 256;                                   // pixels of a row per wave of the overview kernel
constexpr int RD_TILE_H = 16;                                // the warp kernel's tile: rows
constexpr int RD_TILE_W = 64;                                // and pixels
constexpr long RD_MAX_BLOCKS = 65536;
constexpr int RD_MAX_SIZE = 1 << 20;
constexpr int RD_MAX_SHIFT = 1024;                           // as WP_MAX_SHIFT, WP_MAX_CELLS and WP_MAX_CELL of warp.hip
constexpr int RD_MAX_CELLS = 65536;
constexpr int RD_MAX_CELL = 1 << 14;

struct RdMapParams {
  const unsigned char* img;
  const unsigned char* img_end;                              // one past the last byte of the last row present
  long pitch;
  unsigned char* out;
  int h, w, ds, wr, wg, wb;
  int q[256];
};

__global__ __launch_bounds__(256) void rd_overview_kernel(const RdMapParams P) {
  __shared__ int lq[256];
  lq[threadIdx.x] = P.q[threadIdx.x];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int ds = P.ds, g = ds >> 2;                          // g: the lanes of one block, ds >= 4
  const int lg = 31 - __clz(ds), sh = 2 * lg;                // log2 of the block's side and area
  const long Wv = (long)P.w * ds;                            // the pixels of a row that lie in whole blocks
  const long nchunk = (Wv + RD_PX - 1) / RD_PX;
  const long tiles = nchunk * P.h;
  for (long t = (long)blockIdx.x * 4 + wave; t < tiles; t += (long)gridDim.x * 4) {    // wave-uniform
    const long by = t / nchunk, chunk = t - by * nchunk;
    const long x0 = chunk * RD_PX + 4L * lane;
    const long left = Wv - x0;
    const int npx = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    unsigned s[4] = {0u, 0u, 0u, 0u};                        // the vertical sums of the lane's four pixels
    if (npx > 0) {
      const unsigned char* p = P.img + by * ds * P.pitch + 3 * x0;
#pragma unroll 4
      for (int v = 0; v < ds; ++v, p += P.pitch) {
        const unsigned o = (unsigned)((uintptr_t)p & 3);
        const unsigned char* q = p - o;
        unsigned d[3] = {0u, 0u, 0u};                        // bytes p[0 .. 12)
        if (npx == 4 && q >= P.img && q + 16 <= P.img_end) {
          const unsigned* u = reinterpret_cast<const unsigned*>(q);
          const unsigned a0 = u[0], a1 = u[1], a2 = u[2], a3 = u[3];
          d[0] = __builtin_amdgcn_alignbyte(a1, a0, o);
          d[1] = __builtin_amdgcn_alignbyte(a2, a1, o);
          d[2] = __builtin_amdgcn_alignbyte(a3, a2, o);
        } else {
#pragma unroll
          for (int i = 0; i < 12; ++i) {
            if (i < 3 * npx) d[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < npx) {
            const unsigned r = (d[(3 * k) >> 2] >> (8 * ((3 * k) & 3))) & 255u;
            const unsigned gr = (d[(3 * k + 1) >> 2] >> (8 * ((3 * k + 1) & 3))) & 255u;
            const unsigned b = (d[(3 * k + 2) >> 2] >> (8 * ((3 * k + 2) & 3))) & 255u;
            const int acc = P.wr * lq[r] + P.wg * lq[gr] + P.wb * lq[b];
            s[k] += (unsigned)min(max((acc + (1 << 15)) >> 16, 0), 255);
          }
        }
      }
    }
    unsigned char* o = P.out + by * P.w;
    if (ds == 1) {
      unsigned char* oo = o + x0;
      if (npx == 4 && ((uintptr_t)oo & 3) == 0) {
        *reinterpret_cast<unsigned*>(oo) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k < npx) oo[k] = (unsigned char)s[k];
        }
      }
    } else if (ds == 2) {                                    // Wv is even: npx is 0, 2 or 4
      if (npx >= 2) o[x0 >> 1] = (unsigned char)((s[0] + s[1] + 2u) >> 2);
      if (npx == 4) o[(x0 >> 1) + 1] = (unsigned char)((s[2] + s[3] + 2u) >> 2);
    } else {                                                 // Wv is a multiple of 4: npx is 0 or 4, alike in a block
      unsigned tot = s[0] + s[1] + s[2] + s[3];
      for (int m = 1; m < g; m <<= 1) tot += (unsigned)__shfl_xor((int)tot, m, 64);      // every lane of the wave
      if (npx == 4 && (lane & (g - 1)) == 0) o[x0 >> lg] = (unsigned char)((tot + ((1u << sh) >> 1)) >> sh);
    }
  }
}

// ---- the warp ---------------------------------------------------------------------------------------------------------
struct RdArgs {
  const unsigned char* src;                                  // row src_row0 of the region
  const unsigned char* src_end;                              // one past the last byte of the last row present
  long src_pitch;
  const long long* transform;
  const int* field;
  unsigned char* out;                                        // row row0 of the first result
  long out_pitch, out_img;
  int row_lo, row_hi;                                        // region rows that may be read: present and inside [0, H)
  int src_row0, row0, rows, H, W, cell, Gy, Gx, max_shift;
  unsigned fill;
  long ntx, tiles;
};

__device__ __forceinline__ long rd_clamp(long v, long lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

// floor(n / den) for den > 0, |n| < 2^62, |n / den| < 2^32: the float64 quotient is within one of the truth, one exact
// correction step each way settles it (as wp_floor_div of warp.hip).
__device__ __forceinline__ long rd_floor_div(long n, long den) {
  long q = (long)floor((double)n / (double)den);
  const long r = n - q * den;
  if (r < 0) --q;
  else if (r >= den) ++q;
  return q;
}

__device__ __forceinline__ long rd_blend(long d00, long d01, long d10, long d11, long wx, long wy, long span, long lim) {
  const long top = (span - wx) * d00 + wx * d01, bot = (span - wx) * d10 + wx * d11;
  const long num = (span - wy) * top + wy * bot;
  return rd_clamp(rd_floor_div(num + span * span / 2, span * span), lim);
}

// The dense displacement of section 3.22 at the pixels (y, x0 .. x0 + npx) of the region, in 1/16 pixel.
__device__ __forceinline__ void rd_dense(const RdArgs& A, long y, long x0, int npx, long (&dys)[4], long (&dxs)[4]) {
  const long span = 2L * A.cell, lim = 16L * A.max_shift;
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
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < npx) {
      long gx0 = 0, gx1 = 0, wx = 0;
      if (A.Gx >= 2) {
        const long u = 2 * (x0 + k) + 1 - A.cell;
        gx0 = u < 0 ? 0 : (long)((unsigned)u / (unsigned)span);
        gx0 = gx0 > A.Gx - 2 ? A.Gx - 2 : gx0;
        gx1 = gx0 + 1;
        wx = u - gx0 * span;
        wx = wx < 0 ? 0 : (wx > span ? span : wx);
      }
      const int2 d00 = *reinterpret_cast<const int2*>(f0 + 2 * gx0), d01 = *reinterpret_cast<const int2*>(f0 + 2 * gx1);
      const int2 d10 = *reinterpret_cast<const int2*>(f1 + 2 * gx0), d11 = *reinterpret_cast<const int2*>(f1 + 2 * gx1);
      dys[k] = rd_blend(d00.x, d01.x, d10.x, d11.x, wx, wy, span, lim);
      dxs[k] = rd_blend(d00.y, d01.y, d10.y, d11.y, wx, wy, span, lim);
    }
  }
}

template <int C, bool NEAREST>
__global__ __launch_bounds__(256) void rd_warp_kernel(const RdArgs A) {
  const long long* T = A.transform + 6L * blockIdx.y;
  const long c = rd_clamp(T[0], 1L << 24), s = rd_clamp(T[1], 1L << 24);
  const long ty = rd_clamp(T[2], 1L << 36), tx = rd_clamp(T[3], 1L << 36);
  const long Cy = rd_clamp(T[4], 1L << 24), Cx = rd_clamp(T[5], 1L << 24);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ly = wave * 4 + (lane >> 4), lx = (lane & 15) * 4;
  unsigned char* outb = A.out + (long)blockIdx.y * A.out_img;
  for (long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
    const long tr = t / A.ntx, tc = t - tr * A.ntx;
    const long yl = tr * RD_TILE_H + ly, x0 = tc * RD_TILE_W + lx;
    if (yl >= A.rows || x0 >= A.W) continue;
    const long y = (long)A.row0 + yl;
    const int npx = (int)min(4L, (long)A.W - x0);
    // ---- the sample position of every pixel, in 1/16 px
    long dys[4] = {0, 0, 0, 0}, dxs[4] = {0, 0, 0, 0};
    if (A.field) rd_dense(A, y, x0, npx, dys, dxs);
    const long Uy = 32 * y - 16 * Cy, Ux = 32 * x0 - 16 * Cx;
    long Vy = c * Uy - s * Ux + Cy * (1L << 28) + (1L << 24);
    long Vx = s * Uy + c * Ux + Cx * (1L << 28) + (1L << 24);
    long sys[4], sxs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long vy = Vy + 2 * (c * dys[k] - s * dxs[k]), vx = Vx + 2 * (s * dys[k] + c * dxs[k]);
      sys[k] = (vy >> 25) + ty;
      sxs[k] = (vx >> 25) + tx;
      Vy -= 32 * s;
      Vx += 32 * c;
    }
    unsigned v[4 * C];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) v[k] = A.fill;
    // ---- the wide gather: four consecutive source columns of one row pair, whole dwords inside the buffer
    bool wide = false;
    if (C == 3 && !NEAREST) {
      const long iy = sys[0] >> 4, ix = sxs[0] >> 4;
      wide = npx == 4 && (sys[1] >> 4) == iy && (sys[2] >> 4) == iy && (sys[3] >> 4) == iy && (sxs[1] >> 4) == ix + 1 &&
             (sxs[2] >> 4) == ix + 2 && (sxs[3] >> 4) == ix + 3 && iy >= A.row_lo && iy + 1 < A.row_hi && ix >= 0 &&
             ix + 4 < A.W;
      const long off = wide ? (iy - A.src_row0) * A.src_pitch + ix * 3 : 0L;
      const unsigned char* p0 = A.src + off;
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
          for (int ch = 0; ch < 3; ++ch) {
            const int i = 3 * k + ch, j = i + 3;
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
        if (NEAREST) {
          const long iy = (sy + 8) >> 4, ix = (sx + 8) >> 4;
          if (iy >= A.row_lo && iy < A.row_hi && ix >= 0 && ix < A.W) {
            const unsigned char* p = A.src + (iy - A.src_row0) * A.src_pitch + ix * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) v[C * k + ch] = p[ch];
          }
        } else {
          const long iy = sy >> 4, ix = sx >> 4;
          const unsigned fy = (unsigned)(sy & 15), fx = (unsigned)(sx & 15);
          const bool r0 = iy >= A.row_lo && iy < A.row_hi, r1 = iy + 1 >= A.row_lo && iy + 1 < A.row_hi;
          const bool c0 = ix >= 0 && ix < A.W, c1 = ix + 1 >= 0 && ix + 1 < A.W;
          if ((r0 || r1) && (c0 || c1)) {                    // p0 may lie just before the buffer: r0, c0 guard it
            const unsigned char* p0 = A.src + (iy - A.src_row0) * A.src_pitch + ix * C;
            const unsigned char* p1 = p0 + A.src_pitch;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
              const unsigned p00 = (r0 && c0) ? p0[ch] : A.fill, p01 = (r0 && c1) ? p0[C + ch] : A.fill;
              const unsigned p10 = (r1 && c0) ? p1[ch] : A.fill, p11 = (r1 && c1) ? p1[C + ch] : A.fill;
              v[C * k + ch] = ((16u - fy) * ((16u - fx) * p00 + fx * p01) + fy * ((16u - fx) * p10 + fx * p11) + 128u) >> 8;
            }
          }
        }
      }
    }
    unsigned char* o = outb + yl * A.out_pitch + x0 * C;
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

}  // namespace

// img: rows of a uint8 [H][W][3] region, pitch in bytes (any pitch >= 3 W, any base alignment); q_table: HOST int [256];
// w: HOST int [3]; ds: a power of two in 1 .. 64.  out: uint8 [H / ds][W / ds], contiguous: whole blocks only.  Shape
// status for another ds, H or W below ds or above 2^30, a pitch below a row, a negative table entry or weights that
// could overflow the int32 accumulator.  One launch.
extern "C" int s2s_structure_overview_u8(const void* img, long pitch, int H, int W, const int* q_table, const int* w,
                                         int ds, void* out, void* stream) {
  if (!img || !q_table || !w || !out) return S2S_ERR_NULL;
  if (ds < 1 || ds > RD_MAX_DS || (ds & (ds - 1)) != 0) return S2S_ERR_SHAPE;
  if (H < ds || W < ds || H > (1 << 30) || W > (1 << 30)) return S2S_ERR_SHAPE;
  if (pitch < 3L * W) return S2S_ERR_SHAPE;
  long bound = 1L << 15;                                     // |acc + 2^15| must fit int32
  int qmax = 0;
  for (int i = 0; i < 256; ++i) {
    if (q_table[i] < 0) return S2S_ERR_SHAPE;
    if (q_table[i] > qmax) qmax = q_table[i];
  }
  for (int c = 0; c < 3; ++c) bound += (long)qmax * (w[c] < 0 ? -(long)w[c] : (long)w[c]);
  if (bound > 2147483647L) return S2S_ERR_SHAPE;
  RdMapParams P;
  P.img = (const unsigned char*)img; P.pitch = pitch;
  P.img_end = P.img + (long)(H - 1) * pitch + 3L * W;
  P.out = (unsigned char*)out;
  P.h = H / ds; P.w = W / ds; P.ds = ds;
  P.wr = w[0]; P.wg = w[1]; P.wb = w[2];
  for (int i = 0; i < 256; ++i) P.q[i] = q_table[i];
  const long tiles = (((long)P.w * ds + RD_PX - 1) / RD_PX) * P.h;
  long blocks = (tiles + 3) / 4;
  if (blocks > RD_MAX_BLOCKS) blocks = RD_MAX_BLOCKS;
  hipLaunchKernelGGL(rd_overview_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// src: rows [src_row0, src_row0 + src_rows) of a uint8 [H][W][C] region, C = 3 or 1, src_pitch in bytes, any pitch >= W C
// and any base alignment; transform: DEVICE long [A][6] = (c, s, ty, tx, Cy, Cx), any values; field: DEVICE int
// [Gy][Gx][2] in 1/16 px, any values, or null (Gy, Gx, cell and max_shift are then ignored); nearest: 0 bilinear, 1
// nearest.  out: rows [row0, row0 + rows) of A results out_img bytes apart, out_pitch in bytes.  A tap on a row that is
// not present takes the fill, as a tap outside the region does: the caller provides the rows the band reads.  Shape
// status for H or W outside 1 .. 2^20, A outside 1 .. 65535, a bad C, fill or band, a pitch smaller than a row, results
// that overlap, and with a field for Gy != H / cell, Gx != W / cell, cell outside 1 .. 2^14, Gy Gx outside 1 .. 65536 or
// max_shift outside 0 .. 1024.  One launch.
extern "C" int s2s_rigid_warp_u8(const void* src, long src_pitch, int src_row0, int src_rows, const long* transform, int A,
                                 const int* field, int Gy, int Gx, int cell, int max_shift, int H, int W, int C,
                                 int nearest, int fill, int row0, int rows, void* out, long out_pitch, long out_img,
                                 void* stream) {
  if (!src || !transform || !out) return S2S_ERR_NULL;
  if (C != 1 && C != 3) return S2S_ERR_SHAPE;
  if (H < 1 || W < 1 || H > RD_MAX_SIZE || W > RD_MAX_SIZE || fill < 0 || fill > 255) return S2S_ERR_SHAPE;
  if (A < 1 || A > 65535 || (nearest != 0 && nearest != 1)) return S2S_ERR_SHAPE;
  if (field) {
    if (cell < 1 || cell > RD_MAX_CELL || Gy != H / cell || Gx != W / cell) return S2S_ERR_SHAPE;
    if (Gy < 1 || Gx < 1 || (long)Gy * Gx > RD_MAX_CELLS) return S2S_ERR_SHAPE;
    if (max_shift < 0 || max_shift > RD_MAX_SHIFT) return S2S_ERR_SHAPE;
  }
  if (row0 < 0 || rows < 1 || rows > H - row0) return S2S_ERR_SHAPE;
  if (src_row0 < 0 || src_rows < 1 || src_rows > H - src_row0) return S2S_ERR_SHAPE;
  const long rowb = (long)W * C;
  if (src_pitch < rowb || out_pitch < rowb) return S2S_ERR_SHAPE;
  if (A > 1 && out_img < out_pitch * (long)rows) return S2S_ERR_SHAPE;
  RdArgs R;
  R.src = (const unsigned char*)src; R.src_pitch = src_pitch;
  R.src_end = R.src + (long)(src_rows - 1) * src_pitch + rowb;
  R.transform = (const long long*)transform; R.field = field;
  R.out = (unsigned char*)out; R.out_pitch = out_pitch; R.out_img = out_img;
  R.row_lo = src_row0; R.row_hi = src_row0 + src_rows;
  R.src_row0 = src_row0; R.row0 = row0; R.rows = rows; R.H = H; R.W = W;
  R.cell = field ? cell : 1; R.Gy = field ? Gy : 1; R.Gx = field ? Gx : 1; R.max_shift = field ? max_shift : 0;
  R.fill = (unsigned)fill;
  R.ntx = ((long)W + RD_TILE_W - 1) / RD_TILE_W;
  R.tiles = R.ntx * (((long)rows + RD_TILE_H - 1) / RD_TILE_H);
  const dim3 grid((unsigned)(R.tiles < RD_MAX_BLOCKS ? R.tiles : RD_MAX_BLOCKS), (unsigned)A);
  hipStream_t st = (hipStream_t)stream;
  if (C == 3 && !nearest) hipLaunchKernelGGL((rd_warp_kernel<3, false>), grid, dim3(256), 0, st, R);
  else if (C == 3) hipLaunchKernelGGL((rd_warp_kernel<3, true>), grid, dim3(256), 0, st, R);
  else if (!nearest) hipLaunchKernelGGL((rd_warp_kernel<1, false>), grid, dim3(256), 0, st, R);
  else hipLaunchKernelGGL((rd_warp_kernel<1, true>), grid, dim3(256), 0, st, R);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
