// Tile quality control: focus (variance of the Laplacian), marker ink and dark-artefact counts of windows of a uint8 RGB
// image, per tile of a batch, per tile of a region's plan or per cell of a region's map.  DESIGN.md section 3.23.
//
//   s2s_qc_chunks       chunks per window: the size of a slab
//   s2s_qc_windows_u8   one pass over image rows [row0, row1) of every window: eight int64 partial sums per chunk
//   s2s_qc_finalize     partials -> int64 counts [owners][8], stored or added to what counts holds, and the five fp64
//                       values of the counts as they then stand
//
// Definition, all integer.  mx / mn = max / min(R, G, B); tissue = mn < white and mx >= black (is_tissue, common.h);
// Y = (77 R + 150 G + 29 B + 128) >> 8; L(y, x) = Y(y-1, x) + Y(y+1, x) + Y(y, x-1) + Y(y, x+1) - 4 Y(y, x).  A focus
// pixel is a tissue pixel with 1 <= y <= H - 2 and 1 <= x <= W - 2 OF THE IMAGE: its neighbours may lie outside the
// window.  green = tissue and G - max(R, B) >= ink_chroma; blue = tissue and B - R >= ink_chroma and G >= R;
// dark = tissue and mx < dark.  Per window (its rectangle clipped to the image):
//   tissue, focus pixels, sum L, sum L^2 (both over focus pixels), sum Y over tissue, green, blue, dark.
// A numpy int64 restatement is bit-equal, and the counts of disjoint windows that tile an image add up to the image's.
//
// A window is cut into chunks of QC_CH rows x QC_CW columns, and ONE WAVE reduces one chunk: a lane owns four
// consecutive pixels of a row (three dword loads where the twelve bytes are 4-byte aligned, bytes otherwise) and walks
// down the chunk's rows with the luma of the previous, the current and the next row in registers, so a row is loaded
// once per chunk.  The left and right neighbours come from the adjacent lanes by wave shuffles; lanes 0 and 63 load the
// one pixel beside the chunk themselves.  The row above the first and the row below the last are read for their luma
// only.  A lane's sums fit 32 bits (sum L^2 <= 64 * 1020^2); a chunk's do not, so sum L^2 is widened before the wave
// butterfly.  Lane 0 stores the chunk's eight sums at a place that depends on the chunk's position in the launch's
// window list alone: no atomics, no LDS, nothing shared between waves.  A launch writes every slot of its slab, zeros
// for a chunk with no row in [row0, row1), so nothing depends on what the buffer held; int64 sums make the result
// independent of the banding and of the order.
//
// Nothing here allocates, synchronises or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int QC_CH = 16, QC_CW = 256;       // rows x columns of one wave's chunk (qc.CHUNK_ROWS is QC_CH)
constexpr int QC_K = 8;                      // 8-byte slots per chunk and per owner
constexpr int QC_D = 5;                      // fp64 values per owner: focus, tissue_frac, ink_frac, dark_frac, mean_luma

struct QcParams {
  const unsigned char* img;
  long pitch, img_stride;     // bytes
  const int* origins;         // [n][2] = (top, left), any values
  int H, W;                   // the whole image
  int band_top;               // image row of img's first row
  int n, win_h, win_w, ncy, ncx;
  int row0, row1;             // image rows this launch accounts for
  int white, black, ink, dark;
  long total;                 // n * ncy * ncx chunks per sample
};

struct QcRow {
  unsigned v[12];             // v[3 j + c] of the lane's four pixels
  int y[4];                   // their luma
  int yh;                     // lanes 0 / 63: the luma of the pixel left / right of the chunk
};

__device__ __forceinline__ int qc_luma(unsigned r, unsigned g, unsigned b) { return (int)((77u * r + 150u * g + 29u * b + 128u) >> 8); }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One image row: the lane's pixels x .. x + 3 that lie in [lo, hi), and pixel hx when hv (lanes 0 and 63).  Every pixel
// read lies inside the image; what is not read is 0 and is never used (a focus pixel's neighbours are in the image).
__device__ __forceinline__ void qc_load_row(const unsigned char* __restrict__ row, int x, int lo, int hi, int hx, bool hv,
                                            QcRow& r) {
  if (x >= lo && x + 4 <= hi && ((uintptr_t)(row + 3L * x) & 3) == 0) {
    const unsigned* q = reinterpret_cast<const unsigned*>(row + 3L * x);
    const unsigned w0 = q[0], w1 = q[1], w2 = q[2];                  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
    r.v[0] = w0 & 255; r.v[1] = (w0 >> 8) & 255; r.v[2] = (w0 >> 16) & 255;
    r.v[3] = w0 >> 24; r.v[4] = w1 & 255; r.v[5] = (w1 >> 8) & 255;
    r.v[6] = (w1 >> 16) & 255; r.v[7] = w1 >> 24; r.v[8] = w2 & 255;
    r.v[9] = (w2 >> 8) & 255; r.v[10] = (w2 >> 16) & 255; r.v[11] = w2 >> 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x + j >= lo && x + j < hi) {
        const unsigned char* q = row + 3L * (x + j);
        r.v[3 * j] = q[0]; r.v[3 * j + 1] = q[1]; r.v[3 * j + 2] = q[2];
      } else {
        r.v[3 * j] = r.v[3 * j + 1] = r.v[3 * j + 2] = 0;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) r.y[j] = qc_luma(r.v[3 * j], r.v[3 * j + 1], r.v[3 * j + 2]);
  r.yh = 0;
  if (hv) {
    const unsigned char* q = row + 3L * hx;
    r.yh = qc_luma(q[0], q[1], q[2]);
  }
}

__global__ __launch_bounds__(256) void qc_windows_kernel(const QcParams p, long long* __restrict__ slab) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);          // the wave's chunk: (window, cy, cx)
  if (t >= p.total) return;
  const int b = blockIdx.y;
  const int cx = (int)(t % p.ncx);
  const long u = t / p.ncx;
  const int cy = (int)(u % p.ncy), w = (int)(u / p.ncy);
  const long top = p.origins[2 * w], left = p.origins[2 * w + 1];
  const long ya = top + (long)cy * QC_CH, xa = left + (long)cx * QC_CW;
  const long y0l = max(max(ya, 0L), (long)p.row0), y1l = min(min(ya + QC_CH, top + p.win_h), (long)min(p.H, p.row1));
  const long x0l = max(xa, 0L), x1l = min(min(xa + QC_CW, left + p.win_w), (long)p.W);
  long long* out = slab + ((long)b * p.total + t) * QC_K;
  if (y0l >= y1l || x0l >= x1l) {                                     // wave-uniform: nothing of this chunk in range
    if (lane < QC_K) out[lane] = 0;
    return;
  }
  // a chunk that is not empty lies within 256 columns and 16 rows of the image: everything fits an int from here on
  const int y0 = (int)y0l, y1 = (int)y1l, x0 = (int)x0l, x1 = (int)x1l;
  const int x = (int)xa + 4 * lane;
  const int hi = min(x1 + 1, p.W);                                    // the lanes' own pixels: [x0, hi)
  const int hx = lane == 0 ? (int)xa - 1 : (int)xa + QC_CW;
  const bool hv = (lane == 0 || lane == 63) && hx >= 0 && hx < p.W;
  const unsigned char* base = p.img + (long)b * p.img_stride - (long)p.band_top * p.pitch;

  QcRow cur, nxt;
  int yp[4] = {0, 0, 0, 0};
  if (y0 > 0) {
    qc_load_row(base + (long)(y0 - 1) * p.pitch, x, x0, hi, hx, hv, nxt);
#pragma unroll
    for (int j = 0; j < 4; ++j) yp[j] = nxt.y[j];
  }
  qc_load_row(base + (long)y0 * p.pitch, x, x0, hi, hx, hv, cur);
  int acc[QC_K] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int y = y0; y < y1; ++y) {
    if (y + 1 < p.H) {
      qc_load_row(base + (long)(y + 1) * p.pitch, x, x0, hi, hx, hv, nxt);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) nxt.y[j] = 0;
    }
    int yl = __shfl_up(cur.y[3], 1, 64), yr = __shfl_down(cur.y[0], 1, 64);
    if (lane == 0) yl = cur.yh;
    if (lane == 63) yr = cur.yh;
    const bool row_focus = y >= 1 && y <= p.H - 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xx = x + j;
      const unsigned r = cur.v[3 * j], g = cur.v[3 * j + 1], bl = cur.v[3 * j + 2];
      const int Y = cur.y[j];
      const int t1 = (xx >= x0 && xx < x1) ? is_tissue(r, g, bl, p.white, p.black) : 0;
      const int mx = (int)max(r, max(g, bl));
      const int f = (t1 && row_focus && xx >= 1 && xx <= p.W - 2) ? 1 : 0;
      const int L = yp[j] + nxt.y[j] + (j == 0 ? yl : cur.y[j - 1]) + (j == 3 ? yr : cur.y[j + 1]) - 4 * Y;
      acc[0] += t1;
      acc[1] += f;
      acc[2] += f ? L : 0;
      acc[3] += f ? L * L : 0;
      acc[4] += t1 ? Y : 0;
      acc[5] += (t1 && (int)g - (int)max(r, bl) >= p.ink) ? 1 : 0;
      acc[6] += (t1 && (int)bl - (int)r >= p.ink && g >= r) ? 1 : 0;
      acc[7] += (t1 && mx < p.dark) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) yp[j] = cur.y[j];
    cur = nxt;
  }
  long long s[QC_K];
#pragma unroll
  for (int k = 0; k < QC_K; ++k) s[k] = k == 3 ? wave_sum_ll((long long)acc[k]) : (long long)wave_sum_i(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < QC_K; ++k) out[k] = s[k];
  }
}

// one workgroup per owner (window w = owner % n of its sample): thread t adds chunks t, t + 256, ..., then a tree; int64,
// so any order gives the same.  Thread 0 then takes the five fp64 values from the owner's counts as they now stand, every
// quotient, product and difference rounded on its own (no fma), 0 where the denominator is 0.
__global__ __launch_bounds__(256) void qc_finalize_kernel(const long long* __restrict__ slab, int nchunk, int accumulate,
                                                          const int* __restrict__ origins, int n, int H, int W, int win_h,
                                                          int win_w, long long* __restrict__ counts,
                                                          double* __restrict__ derived) {
#pragma clang fp contract(off)
  __shared__ long long red[QC_K][256];
  const long o = blockIdx.x;
  const int tid = threadIdx.x;
  long long s[QC_K] = {0, 0, 0, 0, 0, 0, 0, 0};
  const long long* pp = slab + o * nchunk * QC_K;
  for (int i = tid; i < nchunk; i += 256) {
#pragma unroll
    for (int k = 0; k < QC_K; ++k) s[k] += pp[(long)i * QC_K + k];
  }
#pragma unroll
  for (int k = 0; k < QC_K; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < QC_K; ++k) red[k][tid] += red[k][tid + h];
    }
    __syncthreads();
  }
  if (tid < QC_K) {
    red[tid][0] += accumulate ? counts[o * QC_K + tid] : 0;
    counts[o * QC_K + tid] = red[tid][0];
  }
  __syncthreads();
  if (tid != 0) return;
  const int w = (int)(o % n);
  const long top = origins[2 * w], left = origins[2 * w + 1];
  const long hh = min(top + win_h, (long)H) - max(top, 0L), ww = min(left + win_w, (long)W) - max(left, 0L);
  const long long area = (hh > 0 && ww > 0) ? hh * ww : 0;
  const long long tissue = red[0][0], fn = red[1][0];
  const double t = (double)tissue, f = (double)fn;
  double* d = derived + o * QC_D;
  double focus = 0.0;
  if (fn > 0) {
    const double mean = (double)red[2][0] / f, msq = (double)red[3][0] / f;
    const double sq = mean * mean;
    focus = msq - sq;
  }
  d[0] = focus;
  d[1] = area > 0 ? t / (double)area : 0.0;
  d[2] = tissue > 0 ? (double)(red[5][0] + red[6][0]) / t : 0.0;
  d[3] = tissue > 0 ? (double)red[7][0] / t : 0.0;
  d[4] = tissue > 0 ? (double)red[4][0] / t : 0.0;
}

long qc_chunks(int win_h, int win_w) { return (long)cdiv(win_h, QC_CH) * cdiv(win_w, QC_CW); }

}  // namespace

extern "C" int s2s_qc_chunks(int win_h, int win_w) {
  if (win_h < 1 || win_w < 1 || win_h > (1 << 30) || win_w > (1 << 30)) return S2S_ERR_SHAPE;
  const long n = qc_chunks(win_h, win_w);
  return n > (1L << 30) ? S2S_ERR_SHAPE : (int)n;
}

extern "C" int s2s_qc_windows_u8(const void* img, long pitch, long img_stride, int B, int band_top, int band_h, int H,
                                 int W, const int* origins, int n, int win_h, int win_w, int row0, int row1, int white,
                                 int black, int ink_chroma, int dark, long* slab, void* stream) {
  if (!img || !origins || !slab) return S2S_ERR_NULL;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  if (B < 1 || B > 65535 || n < 1) return S2S_ERR_SHAPE;
  if (H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || win_h < 1 || win_w < 1 || win_h > (1 << 30) || win_w > (1 << 30))
    return S2S_ERR_SHAPE;
  if (white < 1 || white > 256 || black < 0 || black > 255 || ink_chroma < 1 || ink_chroma > 255 || dark < 0 || dark > 256)
    return S2S_ERR_SHAPE;
  if (pitch < 3L * W || band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && img_stride < pitch * (long)band_h) return S2S_ERR_SHAPE;
  if (row0 < 0 || row1 <= row0 || row1 > H) return S2S_ERR_SHAPE;
  // the buffer must hold the rows [row0 - 1, row1] that exist
  if (band_top > (row0 > 0 ? row0 - 1 : 0) || (long)band_top + band_h < (row1 < H ? row1 + 1 : H)) return S2S_ERR_SHAPE;
  const long per = qc_chunks(win_h, win_w);
  if (per > (1L << 30) || per * n > (1L << 32)) return S2S_ERR_SHAPE;       // grid.x = ceil(total / 4) stays below 2^31
  QcParams p;
  p.img = (const unsigned char*)img;
  p.pitch = pitch;
  p.img_stride = img_stride;
  p.origins = origins;
  p.H = H;
  p.W = W;
  p.band_top = band_top;
  p.n = n;
  p.win_h = win_h;
  p.win_w = win_w;
  p.ncy = cdiv(win_h, QC_CH);
  p.ncx = cdiv(win_w, QC_CW);
  p.row0 = row0;
  p.row1 = row1;
  p.white = white;
  p.black = black;
  p.ink = ink_chroma;
  p.dark = dark;
  p.total = per * n;
  hipLaunchKernelGGL(qc_windows_kernel, dim3((unsigned)((p.total + 3) / 4), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, p, (long long*)slab);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_qc_finalize(const long* slab, long owners, int nchunk, int accumulate, const int* origins, int n,
                               int H, int W, int win_h, int win_w, long* counts, double* derived, void* stream) {
  if (!slab || !origins || !counts || !derived) return S2S_ERR_NULL;
  if (owners < 1 || owners > 0x7fffffffL || nchunk < 1 || nchunk > (1 << 30) || n < 1 || owners % n) return S2S_ERR_SHAPE;
  if (H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || win_h < 1 || win_w < 1 || win_h > (1 << 30) || win_w > (1 << 30))
    return S2S_ERR_SHAPE;
  hipLaunchKernelGGL(qc_finalize_kernel, dim3((unsigned)owners), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)slab, nchunk, accumulate, origins, n, H, W, win_h, win_w, (long long*)counts,
                     derived);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
