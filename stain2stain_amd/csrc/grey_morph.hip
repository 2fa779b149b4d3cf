// Stain background subtraction: grey-scale erosion, dilation, opening, closing and the two top-hats by a flat disc or
// square, the integer box mean, the concentration bins of one stain and the corrected counts.  DESIGN.md section 3.36.
//
//   s2s_grey_words             the int32 words of scratch s2s_grey_morph needs
//   s2s_grey_morph             uint8 or int16 [B][H][.] (any row pitch) -> the same dtype, dense; the six operations
//   s2s_grey_box_mean          int16 >= 0 -> s = (2 sum + n) / (2 n) over the in-image pixels of a (2 smooth + 1)^2 window
//   s2s_grey_bins_u8 / _f32    b = bin(c_stain) of every pixel as int16 (no tissue gate) and the tissue flag as a byte
//   s2s_grey_corrected         t = max(b - bg, 0); tissue, positive (t >= j) and sum of t per owner, the histogram of t
//                              over tissue, the mask byte (bit 0 positive, bit 1 tissue) and t itself on request
//   s2s_grey_corrected_finalize  burden = positive / max(tissue, 1) and mean_t = sum_t / max(tissue, 1) as doubles
//   s2s_grey_pair / _finalize  pixels positive in both of two mask-byte batches; burdens, their difference, Dice, IoU
//
// Definition.  Footprint "disc": {(dy, dx): dy^2 + dx^2 <= r2}, r2 = floor(radius^2), the convention of morphology.hip;
// "square": |dy|, |dx| <= r.  There is nothing outside the image: a minimum or maximum runs over the in-image pixels of
// the footprint only.  erode = min, dilate = max, open = dilate(erode), close = erode(dilate), tophat = x - open(x),
// bothat = close(x) - x, the differences formed in 32 bits and saturated to the dtype.
//
// How.  A flat footprint is a stack of row spans [x - w(dy), x + w(dy)].  The minimum of a span of any length is the
// minimum of two overlapping power-of-two windows, so the span tables M_k[y][x] = min(x .. x + 2^k - 1, clipped to the
// row) are built once per pass (gm_level_kernel, k = 0 .. floor(log2(longest span))) and the gather takes, per output
// pixel and dy, min(M_k[y + dy][xl], M_k[y + dy][xr - 2^k + 1]) with [xl, xr] the span clipped to the row and
// k = floor(log2(xr - xl + 1)): two row segments per dy that neighbouring lanes read side by side, work linear in the
// radius.  Everything is integer minima, maxima, sums and differences: bit-equal run to run and for every banding.
//
// bin(c) = clamp(ceil(c * 1024) - 1, 0, 4095) with the loads, the table, the products and the sums of
// stain_calibrate.hip, so bin >= j <=> c > j / 1024 and the corrected numbers reduce to stain_quantify's when nothing
// is subtracted.  The counting kernel keeps a uint32 histogram in LDS, counts bin 0 (most of a top-hat) in a register,
// and flushes with 64-bit integer atomics: exact in any order.
//
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int GM_MAX_RADIUS = 128;           // background.MAX_RADIUS
constexpr int GM_MAX_SMOOTH = 16;            // background.MAX_SMOOTH
constexpr int GM_MAX_SIDE = 32767;
constexpr int GM_MAX_B = 65535;
constexpr int GM_NB = 4096;
constexpr float GM_BINS_PER_OD = 1024.0f;
constexpr int GM_TX = 64, GM_TY = 4;         // a workgroup's tile: one wave per row, so dy and w(dy) are wave-uniform

enum { GM_U8 = 0, GM_I16 = 1 };
enum { GM_ERODE = 0, GM_DILATE = 1, GM_OPEN = 2, GM_CLOSE = 3, GM_TOPHAT = 4, GM_BOTHAT = 5 };
enum { GM_DISC = 0, GM_SQUARE = 1 };
enum { GM_TO_PLANE = 0, GM_VALUE = 1, GM_X_MINUS = 2, GM_MINUS_X = 3 };

struct GmPix {
  int n, y, x;
  bool in;
  long i;                      // index into a dense [B][H][W] array
};
__device__ __forceinline__ GmPix gm_pix(int H, int W) {
  GmPix p;
  p.x = blockIdx.x * GM_TX + threadIdx.x;
  p.y = blockIdx.y * GM_TY + threadIdx.y;
  p.n = blockIdx.z;
  p.in = p.x < W && p.y < H;
  p.i = ((long)p.n * H + p.y) * W + p.x;
  return p;
}

__device__ __forceinline__ int gm_load(const void* src, int dtype, long off) {
  return dtype == GM_U8 ? (int)reinterpret_cast<const unsigned char*>(src)[off]
                        : (int)reinterpret_cast<const short*>(src)[off];
}
__device__ __forceinline__ void gm_store(void* dst, int dtype, long off, int v) {
  if (dtype == GM_U8)
    reinterpret_cast<unsigned char*>(dst)[off] = (unsigned char)min(max(v, 0), 255);
  else
    reinterpret_cast<short*>(dst)[off] = (short)min(max(v, -32768), 32767);
}

template <bool MAX>
__device__ __forceinline__ int gm_op(int a, int b) {
  return MAX ? max(a, b) : min(a, b);
}

// M_0: the source as a dense int16 plane
__global__ __launch_bounds__(256) void gm_level0_kernel(const void* __restrict__ src, int dtype, long pitch, long img,
                                                        int H, int W, short* __restrict__ dst) {
  const GmPix p = gm_pix(H, W);
  if (p.in) dst[p.i] = (short)gm_load(src, dtype, (long)p.n * img + (long)p.y * pitch + p.x);
}

// M_k[x] = op(M_{k-1}[x], M_{k-1}[x + half]), the second term only where it lies in the row
template <bool MAX>
__global__ __launch_bounds__(256) void gm_level_kernel(const short* __restrict__ prev, short* __restrict__ next, int half,
                                                       int H, int W) {
  const GmPix p = gm_pix(H, W);
  if (!p.in) return;
  int v = prev[p.i];
  if (p.x + half < W) v = gm_op<MAX>(v, (int)prev[p.i + half]);
  next[p.i] = (short)v;
}

struct GmGather {
  const short* planes;         // [levels][B][H][W]
  long plane;                  // B H W
  int H, W, R;                 // R: the largest |dy| of the footprint
  int mode, dtype;
  const void* src;             // the operation's input (GM_X_MINUS, GM_MINUS_X)
  long pitch, img;
  void* dst;                   // dense [B][H][W]: int16 (GM_TO_PLANE) or dtype
  unsigned w4[GM_MAX_RADIUS / 4 + 1];        // half-width of the span at |dy|: byte |dy| & 3 of word |dy| >> 2
};

__device__ __forceinline__ int gm_w(const GmGather& p, int dy) { return (int)((p.w4[dy >> 2] >> (8 * (dy & 3))) & 255u); }

// The rows y0..y1 of one output pixel, four at a time so that eight loads are in flight (a gather with two is bound by
// their latency).  The last group takes row y1 again where it runs past it: a row taken twice changes no minimum.
// CLIPPED = false: no span of this wave leaves the row, so k is that of the full span and wave-uniform like w.
template <bool MAX, bool CLIPPED>
__device__ __forceinline__ int gm_rows(const GmGather& p, const short* base, int y, int x, int y0, int y1) {
  int acc = MAX ? -32768 : 32767;
  for (int yy = y0; yy <= y1; yy += 4) {
    int a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int yu = min(yy + u, y1);
      const int w = gm_w(p, abs(yu - y));
      const short* row = base + (long)yu * p.W;
      if (CLIPPED) {
        const int xl = max(x - w, 0), xr = min(x + w, p.W - 1);
        const int k = 31 - __clz(xr - xl + 1);                 // xl .. xl + 2^k - 1 and xr - 2^k + 1 .. xr cover the span
        const short* rk = row + (long)k * p.plane;
        a[u] = rk[xl];
        b[u] = rk[xr - (1 << k) + 1];
      } else {
        const int k = 31 - __builtin_clz(2 * w + 1);
        const short* rk = row + (long)k * p.plane;
        a[u] = rk[x - w];
        b[u] = rk[x + w - (1 << k) + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = gm_op<MAX>(acc, gm_op<MAX>(a[u], b[u]));
  }
  return acc;
}

// One wave per row of the tile: dy, w(dy) and the rows' addresses are wave-uniform (scalar loads of the table, scalar
// address arithmetic).  The waves within R columns of the left or right edge take k per lane.
template <bool MAX>
__global__ __launch_bounds__(256) void gm_gather_kernel(const GmGather p) {
  const int y = blockIdx.y * GM_TY + __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int xw = blockIdx.x * GM_TX, x = xw + threadIdx.x, n = blockIdx.z;
  if (y >= p.H || x >= p.W) return;
  const int y0 = max(y - p.R, 0), y1 = min(y + p.R, p.H - 1);
  const short* base = p.planes + (long)n * p.H * p.W;
  const bool clipped = xw - p.R < 0 || xw + GM_TX - 1 + p.R > p.W - 1;         // uniform
  const int acc = clipped ? gm_rows<MAX, true>(p, base, y, x, y0, y1) : gm_rows<MAX, false>(p, base, y, x, y0, y1);
  const long i = ((long)n * p.H + y) * p.W + x;
  if (p.mode == GM_TO_PLANE) {
    reinterpret_cast<short*>(p.dst)[i] = (short)acc;
  } else if (p.mode == GM_VALUE) {
    gm_store(p.dst, p.dtype, i, acc);
  } else {
    const int v = gm_load(p.src, p.dtype, (long)n * p.img + (long)y * p.pitch + x);
    gm_store(p.dst, p.dtype, i, p.mode == GM_X_MINUS ? v - acc : acc - v);
  }
}

// s = (2 sum + n) / (2 n) over the in-image pixels of the window; values >= 0
__global__ __launch_bounds__(256) void gm_box_mean_kernel(const short* __restrict__ src, int H, int W, int smooth,
                                                          short* __restrict__ dst) {
  const GmPix p = gm_pix(H, W);
  if (!p.in) return;
  const int y0 = max(p.y - smooth, 0), y1 = min(p.y + smooth, H - 1);
  const int x0 = max(p.x - smooth, 0), x1 = min(p.x + smooth, W - 1);
  const short* base = src + (long)p.n * H * W;
  int sum = 0;
  for (int yy = y0; yy <= y1; ++yy) {
    const short* row = base + (long)yy * W;
    for (int xx = x0; xx <= x1; ++xx) sum += row[xx];
  }
  const int n = (y1 - y0 + 1) * (x1 - x0 + 1);
  dst[p.i] = (short)((2 * sum + n) / (2 * n));
}

// ---- the concentration bins -----------------------------------------------------------------------------------------
struct GmBins {
  const void* img;
  long pitch, stride, chan;    // bytes (uint8) or elements (fp32)
  int rows, W, white, black;
  float mr, mg, mb;            // the stain's column of the unmixing matrix
  float od[256];
};

// the save conversion, the concentration and the bin: the operations of stain_calibrate.hip, one by one
__device__ __forceinline__ unsigned gm_quantise(float x) {
#pragma clang fp contract(off)
  const float h = x * 0.5f;
  const float u = (h + 0.5f) * 255.0f;
  return (unsigned)(int)fminf(fmaxf(u, 0.0f), 255.0f);
}
__device__ __forceinline__ float gm_conc(float odr, float odg, float odb, float mr, float mg, float mb) {
#pragma clang fp contract(off)
  const float pr = odr * mr, pg = odg * mg, pb = odb * mb;
  const float s = pr + pg;
  return s + pb;
}
__device__ __forceinline__ int gm_bin(float c) {
#pragma clang fp contract(off)
  const float s = c * GM_BINS_PER_OD;
  const float t = ceilf(s) - 1.0f;
  return (int)fminf(fmaxf(t, 0.0f), (float)(GM_NB - 1));
}

template <bool F32>
__global__ __launch_bounds__(256) void gm_bins_kernel(const GmBins p, short* __restrict__ bins,
                                                      unsigned char* __restrict__ tissue) {
  __shared__ float lut[256];
  lut[threadIdx.y * GM_TX + threadIdx.x] = p.od[threadIdx.y * GM_TX + threadIdx.x];
  __syncthreads();
  const GmPix q = gm_pix(p.rows, p.W);
  if (!q.in) return;
  unsigned r, g, b;
  if (F32) {
    const float* px = reinterpret_cast<const float*>(p.img) + (long)q.n * p.stride + (long)q.y * p.pitch + q.x;
    r = gm_quantise(px[0]);
    g = gm_quantise(px[p.chan]);
    b = gm_quantise(px[2 * p.chan]);
  } else {
    const unsigned char* px =
        reinterpret_cast<const unsigned char*>(p.img) + (long)q.n * p.stride + (long)q.y * p.pitch + 3L * q.x;
    r = px[0];
    g = px[1];
    b = px[2];
  }
  bins[q.i] = (short)gm_bin(gm_conc(lut[r], lut[g], lut[b], p.mr, p.mg, p.mb));
  if (tissue) tissue[q.i] = (unsigned char)is_tissue(r, g, b, p.white, p.black);
}

// ---- the corrected counts -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gm_zero_kernel(unsigned long long* __restrict__ a, long na,
                                                      unsigned long long* __restrict__ b, long nb) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < na; i += (long)gridDim.x * 256) a[i] = 0ull;
  if (b) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += (long)gridDim.x * 256) b[i] = 0ull;
  }
}

__device__ __forceinline__ unsigned long long gm_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

struct GmCorrected {
  const short* bins;           // [B][rows][W]
  const short* bg;             // the same, or null: nothing is subtracted
  const unsigned char* tissue; // the same
  int rows, W;                 // rows the buffers hold per sample
  int row0, nrows;             // the rows that count (the others are a band's halo)
  int spo;                     // samples per owner: 1, or B when pooled
  int j, stain;
  unsigned char* mask;         // [B][nrows][.] with out_img elements per sample, or null
  short* corrected;            // the same, or null
  long out_img;
};

// grid = (workgroups per owner, owners).  A workgroup counts fewer than 2^32 pixels (gm_count_blocks).
__global__ __launch_bounds__(256) void gm_corrected_kernel(const GmCorrected p, unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ hist) {
  __shared__ unsigned h[GM_NB];
  __shared__ unsigned long long red[4][4];
  const int tid = threadIdx.x, owner = blockIdx.y;
  for (int i = tid; i < GM_NB; i += 256) h[i] = 0u;
  __syncthreads();
  const long per = (long)p.nrows * p.W, total = per * p.spo;
  unsigned long long nt = 0, np = 0, st = 0, n0 = 0;
  for (long q = (long)blockIdx.x * 256 + tid; q < total; q += (long)gridDim.x * 256) {
    const long s = q / per, r = q - s * per;
    const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
    const long n = (long)owner * p.spo + s;
    const long i = (n * p.rows + p.row0 + y) * p.W + x;
    const int t = max((int)p.bins[i] - (p.bg ? (int)p.bg[i] : 0), 0);
    const bool tis = p.tissue[i] != 0, pos = tis && t >= p.j;
    const long o = n * p.out_img + (long)y * p.W + x;
    if (p.mask) p.mask[o] = (unsigned char)((pos ? 1 : 0) | (tis ? 2 : 0));
    if (p.corrected) p.corrected[o] = (short)t;
    if (tis) {
      nt += 1;
      np += pos ? 1 : 0;
      st += (unsigned long long)t;
      if (t == 0)
        n0 += 1;
      else
        atomicAdd(&h[min(t, GM_NB - 1)], 1u);
    }
  }
  const unsigned long long v[4] = {gm_wave_sum(nt), gm_wave_sum(np), gm_wave_sum(st), gm_wave_sum(n0)};
  if ((tid & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[tid >> 6][c] = v[c];
  }
  __syncthreads();                             // (also ends the LDS updates)
  unsigned long long* hrow = hist + ((long)owner * 3 + p.stain) * GM_NB;
  if (tid < 4) {
    const unsigned long long s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (s) atomicAdd(tid < 3 ? counts + (long)owner * 3 + tid : hrow, s);
  }
  for (int i = tid; i < GM_NB; i += 256) {
    const unsigned c = h[i];
    if (c) atomicAdd(hrow + i, (unsigned long long)c);
  }
}

__global__ __launch_bounds__(256) void gm_corrected_finalize_kernel(const long long* __restrict__ counts, long owners,
                                                                    double* __restrict__ out) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= owners) return;
  const double den = (double)max(counts[3 * o], 1LL);
  out[2 * o] = (double)counts[3 * o + 1] / den;
  out[2 * o + 1] = (double)counts[3 * o + 2] / den;
}

// both[n] += the pixels whose bit 0 is set in both masks; grid = (workgroups per sample, B)
__global__ __launch_bounds__(256) void gm_pair_kernel(const unsigned char* __restrict__ a,
                                                      const unsigned char* __restrict__ b, long n,
                                                      unsigned long long* __restrict__ both) {
  __shared__ unsigned long long red[4];
  const int tid = threadIdx.x;
  const long off = (long)blockIdx.y * n;
  unsigned long long c = 0;
  for (long i = (long)blockIdx.x * 256 + tid; i < n; i += (long)gridDim.x * 256) c += (a[off + i] & b[off + i] & 1);
  c = gm_wave_sum(c);
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(both + blockIdx.y, s);
  }
}

// the convention of sq_finalize_kernel's paired form, in doubles: Dice and IoU are 1 when both masks are empty
__global__ __launch_bounds__(256) void gm_pair_finalize_kernel(const long long* __restrict__ ca,
                                                               const long long* __restrict__ cb,
                                                               const long long* __restrict__ both, int B,
                                                               double* __restrict__ out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= B) return;
  const double na = (double)ca[3 * n + 1], nb = (double)cb[3 * n + 1], bo = (double)both[n];
  const double ba = na / (double)max(ca[3 * n], 1LL), bb = nb / (double)max(cb[3 * n], 1LL);
  const double uni = na + nb - bo;
  const bool empty = uni == 0.0;
  out[5 * n] = ba;
  out[5 * n + 1] = bb;
  out[5 * n + 2] = fabs(ba - bb);
  out[5 * n + 3] = empty ? 1.0 : 2.0 * bo / (na + nb);
  out[5 * n + 4] = empty ? 1.0 : bo / uni;
}

// ---- host side ------------------------------------------------------------------------------------------------------
int gm_isqrt(int v) {
  int r = 0;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

int gm_check_shape(int B, int H, int W) {
  return (B < 1 || B > GM_MAX_B || H < 1 || W < 1 || H > GM_MAX_SIDE || W > GM_MAX_SIDE) ? S2S_ERR_SHAPE : S2S_OK;
}

// the largest |dy| (= the largest half-width) of a footprint, or a status
int gm_extent(int footprint, int size) {
  if (footprint == GM_DISC) return (size < 0 || size > GM_MAX_RADIUS * GM_MAX_RADIUS) ? S2S_ERR_SHAPE : gm_isqrt(size);
  if (footprint == GM_SQUARE) return (size < 0 || size > GM_MAX_RADIUS) ? S2S_ERR_SHAPE : size;
  return S2S_ERR_SHAPE;
}

// span tables a pass needs: k = 0 .. floor(log2(longest clipped span))
int gm_levels(int R, int W) {
  const int len = 2 * R + 1 < W ? 2 * R + 1 : W;
  int k = 0;
  while ((2 << k) <= len) ++k;
  return k + 1;
}

dim3 gm_grid(int B, int H, int W) { return dim3(cdiv(W, GM_TX), cdiv(H, GM_TY), B); }

int gm_pass(const void* src, int dtype, long pitch, long img, int B, int H, int W, bool mx, int levels, short* planes,
            GmGather g, hipStream_t s) {
  const dim3 grid = gm_grid(B, H, W), block(GM_TX, GM_TY);
  const long N = (long)B * H * W;
  hipLaunchKernelGGL(gm_level0_kernel, grid, block, 0, s, src, dtype, pitch, img, H, W, planes);
  S2S_LAUNCH_CHECK();
  for (int k = 1; k < levels; ++k) {
    if (mx)
      hipLaunchKernelGGL(gm_level_kernel<true>, grid, block, 0, s, planes + (k - 1) * N, planes + k * N, 1 << (k - 1), H, W);
    else
      hipLaunchKernelGGL(gm_level_kernel<false>, grid, block, 0, s, planes + (k - 1) * N, planes + k * N, 1 << (k - 1), H, W);
    S2S_LAUNCH_CHECK();
  }
  g.planes = planes;
  g.plane = N;
  if (mx)
    hipLaunchKernelGGL(gm_gather_kernel<true>, grid, block, 0, s, g);
  else
    hipLaunchKernelGGL(gm_gather_kernel<false>, grid, block, 0, s, g);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

// workgroups per owner for `total` pixels; 0: a uint32 LDS bin could wrap
unsigned gm_count_blocks(long total, int owners) {
  long cap = 2048 / owners;
  if (cap < 1) cap = 1;
  long blocks = (total + 256L * 16 - 1) / (256L * 16);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (total + blocks - 1) / blocks >= (1L << 32) ? 0u : (unsigned)blocks;
}

int gm_fill_bins(GmBins& p, int B, int rows, int W, const float* od_table, const float* unmix, int white, int black,
                 int stain) {
  if (!od_table || !unmix) return S2S_ERR_NULL;
  if (gm_check_shape(B, rows, W) != S2S_OK || stain < 0 || stain > 2 || white < 1 || white > 256 || black < 0 ||
      black > 255)
    return S2S_ERR_SHAPE;
  p.rows = rows;
  p.W = W;
  p.white = white;
  p.black = black;
  p.mr = unmix[stain];
  p.mg = unmix[3 + stain];
  p.mb = unmix[6 + stain];
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  p.chan = 0;
  return S2S_OK;
}

}  // namespace

extern "C" long s2s_grey_words(int B, int H, int W, int footprint, int size) {
  if (gm_check_shape(B, H, W) != S2S_OK) return S2S_ERR_SHAPE;
  const int R = gm_extent(footprint, size);
  if (R < 0) return R;
  const long N = (long)B * H * W;
  return ((gm_levels(R, W) + 1) * N + 1) / 2;             // the span tables and one intermediate plane, int16 each
}

extern "C" int s2s_grey_morph(const void* src, int dtype, long pitch, long img_stride, int B, int H, int W, int op,
                              int footprint, int size, int* scratch, void* out, void* stream) {
  if (!src || !scratch || !out) return S2S_ERR_NULL;
  if (dtype != GM_U8 && dtype != GM_I16) return S2S_ERR_DTYPE;
  if (gm_check_shape(B, H, W) != S2S_OK || op < GM_ERODE || op > GM_BOTHAT) return S2S_ERR_SHAPE;
  if (pitch < W || (B > 1 && img_stride < pitch * (long)H)) return S2S_ERR_SHAPE;
  const int R = gm_extent(footprint, size);
  if (R < 0) return R;
  GmGather g;
  g.H = H;
  g.W = W;
  g.R = R;
  g.dtype = dtype;
  g.src = src;
  g.pitch = pitch;
  g.img = img_stride;
  for (int i = 0; i <= GM_MAX_RADIUS / 4; ++i) g.w4[i] = 0u;
  for (int dy = 0; dy <= R; ++dy)
    g.w4[dy >> 2] |= (unsigned)(footprint == GM_DISC ? gm_isqrt(size - dy * dy) : R) << (8 * (dy & 3));
  const int levels = gm_levels(R, W);
  const long N = (long)B * H * W;
  short* planes = reinterpret_cast<short*>(scratch);
  short* mid = planes + levels * N;
  hipStream_t s = (hipStream_t)stream;
  if (op == GM_ERODE || op == GM_DILATE) {
    g.mode = GM_VALUE;
    g.dst = out;
    return gm_pass(src, dtype, pitch, img_stride, B, H, W, op == GM_DILATE, levels, planes, g, s);
  }
  const bool first_max = op == GM_CLOSE || op == GM_BOTHAT;
  g.mode = GM_TO_PLANE;
  g.dst = mid;
  if (int rc = gm_pass(src, dtype, pitch, img_stride, B, H, W, first_max, levels, planes, g, s)) return rc;
  g.mode = op == GM_TOPHAT ? GM_X_MINUS : op == GM_BOTHAT ? GM_MINUS_X : GM_VALUE;
  g.dst = out;
  return gm_pass(mid, GM_I16, W, (long)H * W, B, H, W, !first_max, levels, planes, g, s);
}

extern "C" int s2s_grey_box_mean(const short* src, int B, int H, int W, int smooth, short* out, void* stream) {
  if (!src || !out) return S2S_ERR_NULL;
  if (gm_check_shape(B, H, W) != S2S_OK || smooth < 0 || smooth > GM_MAX_SMOOTH) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(gm_box_mean_kernel, gm_grid(B, H, W), dim3(GM_TX, GM_TY), 0, (hipStream_t)stream, src, H, W, smooth,
                     out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_bins_u8(const void* img, long pitch, long img_stride, int B, int rows, int W,
                                const float* od_table, const float* unmix, int white, int black, int stain, short* bins,
                                void* tissue, void* stream) {
  if (!img || !bins) return S2S_ERR_NULL;
  GmBins p;
  if (int rc = gm_fill_bins(p, B, rows, W, od_table, unmix, white, black, stain)) return rc;
  if (pitch < 3L * W || (B > 1 && img_stride < pitch * (long)rows)) return S2S_ERR_SHAPE;
  p.img = img;
  p.pitch = pitch;
  p.stride = img_stride;
  hipLaunchKernelGGL(gm_bins_kernel<false>, gm_grid(B, rows, W), dim3(GM_TX, GM_TY), 0, (hipStream_t)stream, p, bins,
                     reinterpret_cast<unsigned char*>(tissue));
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_bins_f32(const float* img, int B, int H, int W, const float* od_table, const float* unmix,
                                 int white, int black, int stain, short* bins, void* tissue, void* stream) {
  if (!img || !bins) return S2S_ERR_NULL;
  GmBins p;
  if (int rc = gm_fill_bins(p, B, H, W, od_table, unmix, white, black, stain)) return rc;
  p.img = img;
  p.pitch = W;
  p.chan = (long)H * W;
  p.stride = 3L * H * W;
  hipLaunchKernelGGL(gm_bins_kernel<true>, gm_grid(B, H, W), dim3(GM_TX, GM_TY), 0, (hipStream_t)stream, p, bins,
                     reinterpret_cast<unsigned char*>(tissue));
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_corrected(const short* bins, const short* bg, const void* tissue, int B, int rows, int W,
                                  int row0, int nrows, int j, int stain, int pool, int reset, long* counts, long* hist,
                                  void* mask, short* corrected, long out_img, void* stream) {
  if (!bins || !tissue || !counts || !hist) return S2S_ERR_NULL;
  if (gm_check_shape(B, rows, W) != S2S_OK || row0 < 0 || nrows < 1 || (long)row0 + nrows > rows || j < 1 ||
      j > GM_NB - 1 || stain < 0 || stain > 2)
    return S2S_ERR_SHAPE;
  if ((mask || corrected) && B > 1 && out_img < (long)nrows * W) return S2S_ERR_SHAPE;
  const int owners = pool ? 1 : B;
  const unsigned blocks = gm_count_blocks((long)(pool ? B : 1) * nrows * W, owners);
  if (!blocks) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(unsigned long long), "int64 counts");
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* c = (unsigned long long*)counts;
  unsigned long long* h = (unsigned long long*)hist;
  if (reset) {
    const long n = (long)owners * 3 * GM_NB;
    const long zb = (n + 255) / 256;
    hipLaunchKernelGGL(gm_zero_kernel, dim3((unsigned)(zb > 1024 ? 1024 : zb)), dim3(256), 0, s, h, n, c, 3L * owners);
    S2S_LAUNCH_CHECK();
  }
  GmCorrected p;
  p.bins = bins;
  p.bg = bg;
  p.tissue = reinterpret_cast<const unsigned char*>(tissue);
  p.rows = rows;
  p.W = W;
  p.row0 = row0;
  p.nrows = nrows;
  p.spo = pool ? B : 1;
  p.j = j;
  p.stain = stain;
  p.mask = reinterpret_cast<unsigned char*>(mask);
  p.corrected = corrected;
  p.out_img = out_img;
  hipLaunchKernelGGL(gm_corrected_kernel, dim3(blocks, (unsigned)owners), dim3(256), 0, s, p, c, h);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_corrected_finalize(const long* counts, long owners, double* out, void* stream) {
  if (!counts || !out) return S2S_ERR_NULL;
  if (owners < 1 || owners > GM_MAX_B) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(gm_corrected_finalize_kernel, dim3((unsigned)((owners + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (const long long*)counts, owners, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_pair(const void* mask_a, const void* mask_b, int B, int H, int W, long* both, void* stream) {
  if (!mask_a || !mask_b || !both) return S2S_ERR_NULL;
  if (gm_check_shape(B, H, W) != S2S_OK) return S2S_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* o = (unsigned long long*)both;
  hipLaunchKernelGGL(gm_zero_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, s, o, (long)B,
                     (unsigned long long*)nullptr, 0L);
  S2S_LAUNCH_CHECK();
  const long n = (long)H * W;
  long blocks = (n + 256L * 16 - 1) / (256L * 16);
  const long cap = 2048 / B < 1 ? 1 : 2048 / B;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(gm_pair_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s,
                     reinterpret_cast<const unsigned char*>(mask_a), reinterpret_cast<const unsigned char*>(mask_b), n, o);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_grey_pair_finalize(const long* counts_a, const long* counts_b, const long* both, int B, double* out,
                                      void* stream) {
  if (!counts_a || !counts_b || !both || !out) return S2S_ERR_NULL;
  if (B < 1 || B > GM_MAX_B) return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(gm_pair_finalize_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)counts_a, (const long long*)counts_b, (const long long*)both, B, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
