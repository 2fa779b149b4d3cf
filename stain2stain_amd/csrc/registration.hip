// Paired tile registration: the integer shift between a source tile and its target, by an exhaustive zero-mean
// normalised cross-correlation (ZNCC) search over integer "structure" bytes.  DESIGN.md section 3.21.
//
//   s2s_structure_map_u8   uint8 RGB -> one structure byte per pixel (one stain's concentration on the integer OD
//                          table of stain_norm.hip), optionally block-averaged by 2 or 4
//   s2s_register_sums      the hot kernel: n, sum a, sum a^2 of the template and sum b, sum b^2, sum a b of every shifted
//                          window, all int64
//   s2s_register_pick      the float64 score of every shift from those integers, the total-order pick, the margin
//   s2s_shift_tiles_u8     out[y][x] = img[y + dy][x + dx] with a fill outside the image
//
// Geometry of the search.  Maps a, b: uint8 [B][h][w], radius R, S = 2R + 1, a per-sample centre (cy, cx) from device
// memory.  my = R + |cy|, mx = R + |cx| (64 bits); the template is a[my : h - my, mx : w - mx], th x tw pixels.  Shift
// row iy in 0..S-1 stands for dy = cy + iy - R, so its window starts at b row my + dy = (|cy| + cy) + iy =: by0 + iy and
// ends at by0 + iy + th - 1 <= (h - 1) + cy - |cy| <= h - 1; columns alike.  A sample whose template is empty reads
// nothing.  Whatever the centre holds, no read leaves [0, h) x [0, w).
//
// The sums kernel.  A workgroup owns one sample, RG_DYB = 8 consecutive shift rows, a band of RG_RB = 32 template rows
// and a chunk of RG_CW = 256 template columns.  It stages the band of `a` (zero rows around it, zero bytes after the
// chunk) and the 39 rows of `b` that the 8 x 32 (shift row, template row) pairs touch, 2R bytes wider than the chunk,
// in LDS as dwords, once.  A lane owns one shift column ix and every ng-th dword column j of the chunk (ng = 256 / S
// lane groups): it rebuilds the b dword at byte offset ix + 4 j from two aligned LDS dwords with v_alignbyte_b32, takes
// sum b and sum b^2 of that row with two v_dot4_u32_u8, and one v_dot4_u32_u8 against each of the eight `a` dwords of
// the shift rows that see this b row, which slide through registers as the b row advances.  The zero padding of `a`
// makes every (b row, shift row) pair outside the band contribute 0, so the inner loop has no conditions.  uint32
// accumulators see at most 40 x 64 dot4 of at most 2^18 each (< 2^30); they are widened to 64 bits when the workgroup
// combines its lane groups in LDS and adds the result to the zeroed tables with 64-bit integer atomics: integer sums, so
// the result does not depend on the order.
//
// Nothing here allocates, synchronises or reads back to the host.
#include "common.h"

namespace {

constexpr int RG_MAX_R = 32;
constexpr int RG_MAX_S = 2 * RG_MAX_R + 1;
constexpr long RG_MAX_N = 1L << 18;                          // template pixels: n * sum(a b) stays below 2^53
constexpr int RG_DYB = 8;                                    // shift rows per workgroup
constexpr int RG_RB = 32;                                    // template rows per band
constexpr int RG_CW = 256;                                   // template columns per chunk
constexpr int RG_CWD = RG_CW / 4;
constexpr int RG_L = RG_RB + RG_DYB;                         // staged b rows (the last one is always zero)
constexpr int RG_BW = (RG_CW + 2 * RG_MAX_R) / 4 + 1;        // dwords of a staged b row
constexpr int RG_AROWS = RG_RB + 2 * (RG_DYB - 1) + 1;       // the band between two runs of zero rows
constexpr int RG_MAP_BLOCKS = 16384;

struct RgGeom {
  bool valid;
  int th, tw, my, mx, by0, bx0;
};

// The template and window origin of sample s; everything that depends on the centre in 64 bits.
__device__ __forceinline__ RgGeom rg_geom(const int* center, int s, int h, int w, int R, long* cy_out, long* cx_out) {
  const long cy = center ? (long)center[2 * (long)s] : 0L, cx = center ? (long)center[2 * (long)s + 1] : 0L;
  const long acy = cy < 0 ? -cy : cy, acx = cx < 0 ? -cx : cx;
  const long my = R + acy, mx = R + acx;
  const long th = (long)h - 2 * my, tw = (long)w - 2 * mx;
  RgGeom g;
  g.valid = th >= 1 && tw >= 1;
  g.th = g.valid ? (int)th : 0; g.tw = g.valid ? (int)tw : 0;
  g.my = g.valid ? (int)my : 0; g.mx = g.valid ? (int)mx : 0;
  g.by0 = g.valid ? (int)(acy + cy) : 0; g.bx0 = g.valid ? (int)(acx + cx) : 0;
  if (cy_out) *cy_out = cy;
  if (cx_out) *cx_out = cx;
  return g;
}

// Bytes p[0 .. nb) (nb in 1..4) as a little-endian dword, the rest zero.  Two aligned dword loads where both lie inside
// [lo, hi), bytes otherwise: p has any alignment.
__device__ __forceinline__ unsigned rg_load4(const unsigned char* p, int nb, const unsigned char* lo,
                                             const unsigned char* hi) {
  const unsigned off = (unsigned)((uintptr_t)p & 3);
  const unsigned char* q = p - off;
  unsigned v = 0;
  if (q >= lo && q + 8 <= hi) {
    const unsigned w0 = reinterpret_cast<const unsigned*>(q)[0], w1 = reinterpret_cast<const unsigned*>(q)[1];
    v = __builtin_amdgcn_alignbyte(w1, w0, off);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nb) v |= (unsigned)p[k] << (8 * k);
    }
  }
  return nb >= 4 ? v : (v & ((1u << (8 * nb)) - 1u));
}

__global__ __launch_bounds__(256) void rg_sums_kernel(const unsigned char* a, const unsigned char* b, long total, int h,
                                                      int w, int R, const int* center, int nchunk,
                                                      unsigned long long* tsum, unsigned long long* sums) {
  __shared__ unsigned lb[RG_L * RG_BW];
  __shared__ unsigned la[RG_AROWS * RG_CWD];
  __shared__ unsigned long long red[RG_DYB * RG_MAX_S * 3 + 2];
  const int tid = threadIdx.x, s = blockIdx.z, iy0 = blockIdx.y * RG_DYB;
  const int band = blockIdx.x / nchunk, chunk = blockIdx.x - band * nchunk;
  const RgGeom G = rg_geom(center, s, h, w, R, nullptr, nullptr);
  if (!G.valid) return;                                      // uniform in the workgroup; no pixel of the sample is read
  const int r0 = band * RG_RB, c0 = chunk * RG_CW;
  if (r0 >= G.th || c0 >= G.tw) return;
  const int S = 2 * R + 1;
  const int rb = min(RG_RB, G.th - r0), cw = min(RG_CW, G.tw - c0);
  const int cwd = (cw + 3) >> 2;
  const int ndy = min(RG_DYB, S - iy0);
  const long plane = (long)h * w;

  // ---- stage: `a` band with its zero surround, the b rows iy0 + r0 + [0, rb + ndy - 1), zero elsewhere
  const unsigned char* ab = a + (long)s * plane + (long)(G.my + r0) * w + G.mx + c0;
  for (int i = tid; i < RG_AROWS * RG_CWD; i += 256) {
    const int row = i / RG_CWD, d = i - row * RG_CWD;
    const int rl = row - (RG_DYB - 1);
    unsigned v = 0;
    if (rl >= 0 && rl < rb && 4 * d < cw) v = rg_load4(ab + (long)rl * w + 4 * d, min(4, cw - 4 * d), a, a + total);
    la[i] = v;
  }
  const int bcols = cw + 2 * R, brows = rb + ndy - 1;
  const unsigned char* bb = b + (long)s * plane + (long)(G.by0 + iy0 + r0) * w + G.bx0 + c0;
  for (int i = tid; i < RG_L * RG_BW; i += 256) {
    const int l = i / RG_BW, d = i - l * RG_BW;
    unsigned v = 0;
    if (l < brows && 4 * d < bcols) v = rg_load4(bb + (long)l * w + 4 * d, min(4, bcols - 4 * d), b, b + total);
    lb[i] = v;
  }
  for (int i = tid; i < RG_DYB * RG_MAX_S * 3 + 2; i += 256) red[i] = 0ull;
  __syncthreads();

  // ---- the template's own sums, once per (band, chunk): the workgroups of the first shift-row block
  if (blockIdx.y == 0) {
    unsigned s1 = 0, s2 = 0;                                 // at most 12 dwords per lane
    for (int i = tid; i < RG_AROWS * RG_CWD; i += 256) {
      const unsigned v = la[i];
      s1 = __builtin_amdgcn_udot4(v, 0x01010101u, s1, false);
      s2 = __builtin_amdgcn_udot4(v, v, s2, false);
    }
    atomicAdd(&red[RG_DYB * RG_MAX_S * 3], (unsigned long long)s1);
    atomicAdd(&red[RG_DYB * RG_MAX_S * 3 + 1], (unsigned long long)s2);
  }

  // ---- the products
  const int ng = 256 / S;
  const int g = tid / S, ix = tid - g * S;
  if (g < ng) {
    unsigned acc[RG_DYB], rs[RG_L], rq[RG_L];
#pragma unroll
    for (int k = 0; k < RG_DYB; ++k) acc[k] = 0u;
#pragma unroll
    for (int l = 0; l < RG_L; ++l) rs[l] = rq[l] = 0u;
    const unsigned sh = (unsigned)(ix & 3);
    const int dq = ix >> 2;
    for (int j = g; j < cwd; j += ng) {
      const int left = cw - 4 * j;                           // bytes of this dword inside the chunk
      const unsigned m = left >= 4 ? 0xffffffffu : ((1u << (8 * left)) - 1u);
      unsigned win[RG_DYB];                                  // slot k % RG_DYB holds padded `a` row k
#pragma unroll
      for (int k = 0; k < RG_DYB - 1; ++k) win[k] = la[k * RG_CWD + j];
#pragma unroll
      for (int l = 0; l < RG_L; ++l) {
        win[(l + RG_DYB - 1) % RG_DYB] = la[(l + RG_DYB - 1) * RG_CWD + j];
        const unsigned lo = lb[l * RG_BW + dq + j], hi = lb[l * RG_BW + dq + j + 1];
        const unsigned bs = __builtin_amdgcn_alignbyte(hi, lo, sh);
        const unsigned bm = bs & m;
        rs[l] = __builtin_amdgcn_udot4(bm, 0x01010101u, rs[l], false);
        rq[l] = __builtin_amdgcn_udot4(bm, bm, rq[l], false);
#pragma unroll
        for (int k = 0; k < RG_DYB; ++k)                     // shift row iy0 + k pairs b row l with template row l - k
          acc[k] = __builtin_amdgcn_udot4(win[(l + RG_DYB - 1 - k) % RG_DYB], bs, acc[k], false);
      }
    }
    // sum b and sum b^2 of shift row iy0 + k: the b rows k .. k + rb - 1
#pragma unroll
    for (int k = 0; k < RG_DYB; ++k) {
      unsigned sb = 0u, sq = 0u;
      if (rb == RG_RB) {
#pragma unroll
        for (int l = k; l < k + RG_RB; ++l) { sb += rs[l]; sq += rq[l]; }
      } else {
#pragma unroll
        for (int l = k; l < k + RG_RB; ++l) {
          if (l < k + rb) { sb += rs[l]; sq += rq[l]; }
        }
      }
      if (k < ndy) {
        unsigned long long* r = &red[(k * S + ix) * 3];
        atomicAdd(r, (unsigned long long)sb);
        atomicAdd(r + 1, (unsigned long long)sq);
        atomicAdd(r + 2, (unsigned long long)acc[k]);
      }
    }
  }
  __syncthreads();

  // ---- 64-bit integer atomics into the zeroed tables
  unsigned long long* out = sums + ((long)s * S + iy0) * S * 3;
  for (int i = tid; i < ndy * S * 3; i += 256) atomicAdd(out + i, red[i]);
  if (blockIdx.y == 0) {
    if (tid < 2) atomicAdd(tsum + 3L * s + 1 + tid, red[RG_DYB * RG_MAX_S * 3 + tid]);
    if (tid == 2 && blockIdx.x == 0) tsum[3L * s] = (unsigned long long)((long)G.th * G.tw);
  }
}

// float64 score of one shift; va != 0.  No add follows a multiply: nothing here can contract to an FMA.
__device__ __forceinline__ double rg_score(long long n, long long sa, long long va, const long long* e) {
  const long long sb = e[0], sbb = e[1], sab = e[2];
  const long long vb = n * sbb - sb * sb;
  const long long num = n * sab - sa * sb;
  if (vb == 0) return 0.0;
  const double prod = (double)va * (double)vb;
  return (double)num / sqrt(prod);
}

// (score, d2, linear index iy * S + ix): higher score, then nearer the centre, then smaller dy, then smaller dx
__device__ __forceinline__ bool rg_better(double s1, int d1, int i1, double s2, int d2, int i2) {
  if (s1 != s2) return s1 > s2;
  if (d1 != d2) return d1 < d2;
  return i1 < i2;
}

__device__ __forceinline__ int rg_clamp_i32(long v) {
  return (int)(v < -2147483648L ? -2147483648L : (v > 2147483647L ? 2147483647L : v));
}

__global__ __launch_bounds__(256) void rg_pick_kernel(const long long* tsum, const long long* sums, const int* center,
                                                      int R, int ds, int* shift, double* score, int* valid) {
  __shared__ double ps[256];
  __shared__ int pd[256], pi[256];
  __shared__ double centre_score;
  const int tid = threadIdx.x, s = blockIdx.x, S = 2 * R + 1;
  const long cy = center ? (long)center[2L * s] : 0L, cx = center ? (long)center[2L * s + 1] : 0L;
  const long long n = tsum[3L * s], sa = tsum[3L * s + 1], saa = tsum[3L * s + 2];
  const long long va = n * saa - sa * sa;
  if (n <= 0 || va == 0) {                                   // uniform in the workgroup
    if (tid == 0) {
      shift[2L * s] = rg_clamp_i32(cy * ds); shift[2L * s + 1] = rg_clamp_i32(cx * ds);
      score[3L * s] = 0.0; score[3L * s + 1] = 0.0; score[3L * s + 2] = 0.0;
      valid[s] = 0;
    }
    return;
  }
  const long long* e = sums + (long)s * S * S * 3;
  double bs = -1.0e300;
  int bd = 0x7fffffff, bi = 0x7fffffff;
  for (int i = tid; i < S * S; i += 256) {
    const int iy = i / S, ix = i - iy * S;
    const double sc = rg_score(n, sa, va, e + 3L * i);
    const int d2 = (iy - R) * (iy - R) + (ix - R) * (ix - R);
    if (d2 == 0) centre_score = sc;
    if (rg_better(sc, d2, i, bs, bd, bi)) { bs = sc; bd = d2; bi = i; }
  }
  ps[tid] = bs; pd[tid] = bd; pi[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o && rg_better(ps[tid + o], pd[tid + o], pi[tid + o], ps[tid], pd[tid], pi[tid])) {
      ps[tid] = ps[tid + o]; pd[tid] = pd[tid + o]; pi[tid] = pi[tid + o];
    }
    __syncthreads();
  }
  const double best = ps[0];
  const int py = pi[0] / S, px = pi[0] - py * S;
  __syncthreads();
  // the best score outside the 3 x 3 neighbourhood of the peak
  double other = -1.0e300;
  if (R >= 2) {
    for (int i = tid; i < S * S; i += 256) {
      const int iy = i / S, ix = i - iy * S;
      if (abs(iy - py) > 1 || abs(ix - px) > 1) other = fmax(other, rg_score(n, sa, va, e + 3L * i));
    }
  }
  ps[tid] = other;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) ps[tid] = fmax(ps[tid], ps[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    shift[2L * s] = rg_clamp_i32((cy + py - R) * ds); shift[2L * s + 1] = rg_clamp_i32((cx + px - R) * ds);
    score[3L * s] = best; score[3L * s + 1] = centre_score; score[3L * s + 2] = R >= 2 ? best - ps[0] : 0.0;
    valid[s] = 1;
  }
}

struct RgMapParams {
  const unsigned char* img;
  long pitch, img_stride;
  unsigned char* out;
  int H, W, h, w, ds, wr, wg, wb;
  int q[256];
};

// One lane: four consecutive structure bytes of one output row.
__global__ __launch_bounds__(256) void rg_map_kernel(const RgMapParams P) {
  __shared__ int lq[256];
  lq[threadIdx.x] = P.q[threadIdx.x];
  __syncthreads();
  const int s = blockIdx.y, ds = P.ds, nq = (P.w + 3) >> 2;
  const long quads = (long)P.h * nq;
  const unsigned char* base = P.img + (long)s * P.img_stride;
  unsigned char* obase = P.out + (long)s * P.h * P.w;
  const int area = ds * ds;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const int y = (int)(i / nq), x0 = 4 * (int)(i - (long)y * nq);
    const int px = min(4, P.w - x0);
    unsigned f[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < px) {
        int sum = 0;
        for (int v = 0; v < ds; ++v) {
          const unsigned char* p = base + ((long)y * ds + v) * P.pitch + 3L * ((long)(x0 + k) * ds);
          for (int u = 0; u < ds; ++u, p += 3) {
            const int acc = P.wr * lq[p[0]] + P.wg * lq[p[1]] + P.wb * lq[p[2]];
            sum += min(max((acc + (1 << 15)) >> 16, 0), 255);
          }
        }
        f[k] = (unsigned)((sum + area / 2) / area);
      }
    }
    unsigned char* o = obase + (long)y * P.w + x0;
    if (px == 4 && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<unsigned*>(o) = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < px) o[k] = (unsigned char)f[k];
      }
    }
  }
}

// One lane: four consecutive output bytes of one row (a row is W * C bytes).
__global__ __launch_bounds__(256) void rg_shift_kernel(const unsigned char* img, long pitch, long img_stride, int H, int W,
                                                       int C, const int* shift, unsigned fill, unsigned char* out,
                                                       long out_pitch, long out_img) {
  const int s = blockIdx.y;
  const long dy = shift[2L * s], dx = shift[2L * s + 1];
  const int rowb = W * C, nq = (rowb + 3) >> 2;
  const long quads = (long)H * nq;
  const unsigned char* base = img + (long)s * img_stride;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long)gridDim.x * 256) {
    const int y = (int)(i / nq), xb0 = 4 * (int)(i - (long)y * nq);
    const int nb = min(4, rowb - xb0);
    const long sy = (long)y + dy;
    unsigned v[4] = {fill, fill, fill, fill};
    if (sy >= 0 && sy < H) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nb) {
          const int x = (xb0 + k) / C, c = (xb0 + k) - x * C;
          const long sx = (long)x + dx;
          if (sx >= 0 && sx < W) v[k] = base[sy * pitch + sx * C + c];
        }
      }
    }
    unsigned char* o = out + (long)s * out_img + (long)y * out_pitch + xb0;
    if (nb == 4 && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<unsigned*>(o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nb) o[k] = (unsigned char)v[k];
      }
    }
  }
}

bool rg_bad_search(int B, int h, int w, int R) {
  if (B < 1 || B > 65535 || R < 0 || R > RG_MAX_R || h < 1 || w < 1) return true;
  if (h <= 2 * R || w <= 2 * R) return true;
  return (long)(h - 2 * R) * (long)(w - 2 * R) > RG_MAX_N;
}

unsigned rg_blocks(long quads) {
  long blocks = (quads + 255) / 256;
  if (blocks > RG_MAP_BLOCKS) blocks = RG_MAP_BLOCKS;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

// img: uint8 [B][H][W][3] with pitch / img_stride in bytes (any pitch >= 3 W, any base alignment; samples may interleave,
// as the cells of one row of a region do); q_table: HOST int [256]; w: HOST int [3]; ds: 1, 2 or 4.  out: uint8
// [B][H / ds][W / ds], contiguous.
extern "C" int s2s_structure_map_u8(const void* img, long pitch, long img_stride, int B, int H, int W, const int* q_table,
                                    const int* w, int ds, void* out, void* stream) {
  if (!img || !q_table || !w || !out) return S2S_ERR_NULL;
  if (ds != 1 && ds != 2 && ds != 4) return S2S_ERR_SHAPE;
  if (B < 1 || B > 65535 || H < ds || W < ds || H > (1 << 30) || W > (1 << 30)) return S2S_ERR_SHAPE;
  if (pitch < 3L * W || (B > 1 && img_stride < 1)) return S2S_ERR_SHAPE;
  long bound = 1L << 15;                                     // |acc + 2^15| must fit int32
  int qmax = 0;
  for (int i = 0; i < 256; ++i) {
    if (q_table[i] < 0) return S2S_ERR_SHAPE;
    if (q_table[i] > qmax) qmax = q_table[i];
  }
  for (int c = 0; c < 3; ++c) bound += (long)qmax * (w[c] < 0 ? -(long)w[c] : (long)w[c]);
  if (bound > 2147483647L) return S2S_ERR_SHAPE;
  RgMapParams P;
  P.img = (const unsigned char*)img; P.pitch = pitch; P.img_stride = img_stride;
  P.out = (unsigned char*)out;
  P.H = H; P.W = W; P.h = H / ds; P.w = W / ds; P.ds = ds;
  P.wr = w[0]; P.wg = w[1]; P.wb = w[2];
  for (int i = 0; i < 256; ++i) P.q[i] = q_table[i];
  hipLaunchKernelGGL(rg_map_kernel, dim3(rg_blocks((long)P.h * cdiv(P.w, 4)), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, P);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// a, b: uint8 [B][h][w], contiguous; center: DEVICE int [B][2] = (cy, cx), or null for zeros; tsum: long [B][3] =
// n, sum a, sum a^2; sums: long [B][S][S][3] = sum b, sum b^2, sum a b, S = 2 R + 1.  Both tables are zeroed here, on
// the stream.  Refuses R > 32, h <= 2 R, w <= 2 R and (h - 2 R)(w - 2 R) > 2^18 with the shape status.
extern "C" int s2s_register_sums(const void* a, const void* b, int B, int h, int w, int R, const int* center, long* tsum,
                                 long* sums, void* stream) {
  if (!a || !b || !tsum || !sums) return S2S_ERR_NULL;
  if (rg_bad_search(B, h, w, R)) return S2S_ERR_SHAPE;
  const int S = 2 * R + 1;
  if (hipMemsetAsync(tsum, 0, sizeof(long) * 3 * (size_t)B, (hipStream_t)stream) != hipSuccess) return S2S_ERR_LAUNCH;
  if (hipMemsetAsync(sums, 0, sizeof(long) * 3 * (size_t)B * S * S, (hipStream_t)stream) != hipSuccess)
    return S2S_ERR_LAUNCH;
  const int nband = cdiv(h - 2 * R, RG_RB), nchunk = cdiv(w - 2 * R, RG_CW);
  const dim3 grid((unsigned)(nband * nchunk), (unsigned)cdiv(S, RG_DYB), (unsigned)B);
  hipLaunchKernelGGL(rg_sums_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char*)a,
                     (const unsigned char*)b, (long)B * h * w, h, w, R, center, nchunk, (unsigned long long*)tsum,
                     (unsigned long long*)sums);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// tsum, sums, center as above.  shift: int [B][2] = (dy, dx) * ds, full-resolution pixels; score: double [B][3] = best,
// centre, margin; valid: int [B].
extern "C" int s2s_register_pick(const long* tsum, const long* sums, const int* center, int B, int R, int ds, int* shift,
                                 double* score, int* valid, void* stream) {
  if (!tsum || !sums || !shift || !score || !valid) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || R < 0 || R > RG_MAX_R) return S2S_ERR_SHAPE;
  if (ds != 1 && ds != 2 && ds != 4) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(rg_pick_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const long long*)tsum,
                     (const long long*)sums, center, R, ds, shift, score, valid);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// img: uint8 [B][H][W][C], C = 1 or 3, pitch / img_stride in bytes; shift: DEVICE int [B][2] = (dy, dx), any values;
// out[b][y][x] = img[b][y + dy][x + dx] inside the image, else fill; out_pitch / out_img in bytes.
extern "C" int s2s_shift_tiles_u8(const void* img, long pitch, long img_stride, int B, int H, int W, int C,
                                  const int* shift, int fill, void* out, long out_pitch, long out_img, void* stream) {
  if (!img || !shift || !out) return S2S_ERR_NULL;
  if (C != 1 && C != 3) return S2S_ERR_SHAPE;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 29) || W > (1 << 29) || fill < 0 || fill > 255)
    return S2S_ERR_SHAPE;
  const long rowb = (long)W * C;
  if (pitch < rowb || (B > 1 && img_stride < 1)) return S2S_ERR_SHAPE;
  if (out_pitch < rowb || (B > 1 && out_img < out_pitch * (long)H)) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(rg_shift_kernel, dim3(rg_blocks((long)H * ((rowb + 3) / 4)), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned char*)img, pitch, img_stride, H, W, C, shift, (unsigned)fill,
                     (unsigned char*)out, out_pitch, out_img);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
