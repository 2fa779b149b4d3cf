// Zonal stain quantification: the burden, the concentration and the objects of a stain per class of a zone map.
// DESIGN.md section 3.34.
//
//   s2s_zonal_u8 / _f32            table long [owners][Z][8] += pixels, tissue, positive_0..2, sum q_0..2 of the owner's
//                                  pixels by their zone byte; unzoned long [owners] += the pixels whose byte is >= Z
//   s2s_zonal_pair_u8 / _f32       table long [owners][Z][6] for one stain of a prediction a and a target b: pixels,
//                                  tissue_a, tissue_b, positive in both, in a only, in b only
//   s2s_zonal_finalize             the fp64 burdens, mean concentrations, fractions, Dice and IoU of every (owner, zone)
//   s2s_zonal_object_overlap       overlap int [B][M][Z] += the pixels of object m + 1 in zone z; area, count
//   s2s_zonal_object_assign        the zone of every object (largest overlap, ties to the smaller zone) and, per zone, the
//                                  objects assigned to it and their pixels
//   s2s_zonal_object_density       objects per square millimetre of a zone's tissue
//   s2s_zonal_bands                two squared distance maps -> zone bytes: bands from the rim inwards and outwards
//
// Concentration, tissue and positive are those of stain_quant.hip (the same table, the same three products and two sums
// under fp contract(off), the same save conversion for fp32 input); q = min((int)rintf(fmaxf(c, 0) * 1024), 4095) is the
// grid of object_features.hip, summed over TISSUE pixels only.
//
// An OWNER is one sample, or the whole batch (pool).  A workgroup never spans two owners: grid = (workgroups per owner,
// owners).  It keeps a uint32 table [Z][8] in LDS.  Zones are large areas, so nearly every wave meets ONE zone: 64 lanes
// times 8 columns would then queue on eight LDS addresses.  Where a ballot says that every pixel of the wave has the same
// zone byte, the wave sums first (popcounts of ballots for the counts, a butterfly for the sums of q) and lanes 0..7 add
// one column each; any other wave merges inside a lane where its four zones agree and takes plain LDS atomics.  The
// non-zero rows are flushed with 64-bit integer atomics: integer sums, so the result is bit-equal run to run and for
// every split into bands or calls.
//
// Nothing here allocates, synchronises, reads the environment or reads back to the host, so the launches may be captured.
#include "common.h"

namespace {

constexpr int ZN_MAX_Z = 256;                // zones of one map: a byte
constexpr int ZN_CUS = 256;                  // the grid is sized to one resident round of workgroups
constexpr int ZN_RESIDENT_TABLE = 8, ZN_RESIDENT_PAIR = 7;   // workgroups a CU holds at once: 48..50 and 51..69 VGPRs a lane
constexpr int ZN_RESIDENT = 8;               // the small kernels: 8 workgroups of four waves fill a CU's wave slots
constexpr int ZN_QUADS = 8;                  // quads a lane should at least have before another workgroup is worth its flush
constexpr long ZN_MAX_PIXELS = 1L << 40;     // pixels of one owner in one launch
constexpr long ZN_MAX_WG_PIXELS = 1L << 20;  // pixels of one workgroup: 2^20 * 4095 < 2^32, a uint32 cell cannot wrap
constexpr int ZN_MAX_SIDE = 32767;           // the object and band calls (s2s_objfeat_shape, s2s_morph_edt)
constexpr int ZN_MAX_EDGES = 126;            // 2 n + 2 zones fit a byte with 255 left for "no zone"
constexpr int ZN_FAR = 0x7fffffff;

// scripts/zonal_bench.py --ablate: the library built with -DS2S_ABLATE sends every wave down the plain LDS atomics (the
// results are the same), which is the "before" of the one-zone wave path
#ifdef S2S_ABLATE
constexpr bool ZN_WAVE_PATH = false;
#else
constexpr bool ZN_WAVE_PATH = true;
#endif

enum { ZN_U8 = 0, ZN_F32 = 1 };

#define ZN_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct ZnParams {
  const void* a;
  const void* b;              // paired form only
  const unsigned char* z;
  long pitch_a, img_a;        // row pitch and sample stride: bytes (uint8) or elements (fp32)
  long pitch_b, img_b;
  long pitch_z, img_z;        // bytes
  long chan;                  // fp32: elements per channel plane
  int rows, W;                // rows the buffers hold per sample (the band), columns
  int spo;                    // samples per owner: 1, or B when pooled
  int white, black;
  int Z;
  int stain;                  // paired form only
  float m[9];                 // m[3 * channel + stain]
  float thr[3];
  float od[256];
};

// the save conversion of region_finalize_kernel / image_quality(quantize=True)
__device__ __forceinline__ unsigned zn_quantise(float x) {
#pragma clang fp contract(off)
  const float h = x * 0.5f;
  const float u = (h + 0.5f) * 255.0f;
  return (unsigned)(int)fminf(fmaxf(u, 0.0f), 255.0f);
}

// px (1..4) consecutive pixels of one row from column x0 on: v[3 j + c] (the loads of sn_load_quad / sc_load_quad)
template <int LOADER>
__device__ __forceinline__ void zn_load_quad(const void* base, long row_off, long chan, int x0, int px, unsigned* v) {
  if (LOADER == ZN_U8) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + row_off + 3L * x0;
    if (px == 4 && ((uintptr_t)p & 3) == 0) {
      const unsigned w0 = reinterpret_cast<const unsigned*>(p)[0];   // r0 g0 b0 r1
      const unsigned w1 = reinterpret_cast<const unsigned*>(p)[1];   // g1 b1 r2 g2
      const unsigned w2 = reinterpret_cast<const unsigned*>(p)[2];   // b2 r3 g3 b3
      v[0] = w0 & 255; v[1] = (w0 >> 8) & 255; v[2] = (w0 >> 16) & 255;
      v[3] = w0 >> 24; v[4] = w1 & 255; v[5] = (w1 >> 8) & 255;
      v[6] = (w1 >> 16) & 255; v[7] = w1 >> 24; v[8] = w2 & 255;
      v[9] = (w2 >> 8) & 255; v[10] = (w2 >> 16) & 255; v[11] = w2 >> 24;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) { v[3 * j] = p[3 * j]; v[3 * j + 1] = p[3 * j + 1]; v[3 * j + 2] = p[3 * j + 2]; }
      }
    }
  } else {
    const float* p = reinterpret_cast<const float*>(base) + row_off + x0;
    if (px == 4 && ((uintptr_t)p & 15) == 0 && (chan & 3) == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p + c * chan);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[3 * j + c] = zn_quantise(q[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < px) {
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * j + c] = zn_quantise(p[c * chan + j]);
        }
      }
    }
  }
}

// the zone bytes of the same px pixels: one dword where the address allows it
__device__ __forceinline__ void zn_load_zones(const unsigned char* p, int px, unsigned* zb) {
  if (px == 4 && ((uintptr_t)p & 3) == 0) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
    zb[0] = w & 255; zb[1] = (w >> 8) & 255; zb[2] = (w >> 16) & 255; zb[3] = w >> 24;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) zb[j] = p[j];
    }
  }
}

// ((od_r m_r) + (od_g m_g)) + (od_b m_b): plain operators under the pragma keep every product and sum rounded on its
// own (see sq_conc)
__device__ __forceinline__ float zn_conc(float odr, float odg, float odb, float mr, float mg, float mb) {
#pragma clang fp contract(off)
  const float pr = odr * mr, pg = odg * mg, pb = odb * mb;
  const float s = pr + pg;
  return s + pb;
}

// the grid of of_q (object_features.hip)
__device__ __forceinline__ unsigned zn_q(float c) {
#pragma clang fp contract(off)
  return (unsigned)min((int)rintf(fmaxf(c, 0.0f) * 1024.0f), 4095);
}

__device__ __forceinline__ unsigned zn_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum over the wave of a per-lane count in 0..7, from three ballots
__device__ __forceinline__ unsigned zn_wave_count(unsigned c) {
  return (unsigned)(__popcll(__ballot(c & 1u)) + 2 * __popcll(__ballot(c & 2u)) + 4 * __popcll(__ballot(c & 4u)));
}

// quad q of an owner -> (sample, row, first column, pixels)
struct ZnQuad {
  int n, y, x0, px;
};
__device__ __forceinline__ ZnQuad zn_quad(const ZnParams& p, int owner, long q, int nq, long per) {
  long s = 0, r = q;
  if (p.spo > 1) {                             // uniform: only a pooled batch pays for the 64-bit division
    s = q / per;
    r = q - s * per;
  }
  int y, xq;
  if (per <= 0x7fffffffL) {                    // uniform
    y = (int)((unsigned)r / (unsigned)nq);
    xq = (int)((unsigned)r - (unsigned)y * (unsigned)nq);
  } else {
    y = (int)(r / nq);
    xq = (int)(r - (long)y * nq);
  }
  return ZnQuad{owner * p.spo + (int)s, y, 4 * xq, min(4, p.W - 4 * xq)};
}

// A pixel's columns travel packed in two words, so that a lane's four pixels stay in eight registers.  Single (8
// columns): w0 = the five 0 / 1 columns in bits 0..4, q_0 in bits 5..16, q_1 in bits 17..28; w1 = q_2.  Paired (6
// columns): w0 = the six 0 / 1 columns; w1 is not used.
template <int NC>
__device__ __forceinline__ unsigned zn_col(unsigned w0, unsigned w1, int c) {
  if (NC == 6) return (w0 >> c) & 1u;
  return c < 5 ? (w0 >> c) & 1u : c == 5 ? (w0 >> 5) & 4095u : c == 6 ? (w0 >> 17) & 4095u : w1;
}

// A lane brings px (0..4) pixels: zone bytes zb[j] and the packed columns w0[j], w1[j], zero beyond px; the first NCNT
// columns are 0 / 1 per pixel, the others sums of q.  Every lane of the wave is here (lanes past the owner's last quad
// with px = 0) and lane 0 has a pixel.  tab[z][NC] += the columns; unz += the pixels whose byte is >= Z.
template <int NC, int NCNT>
__device__ __forceinline__ void zn_accumulate(unsigned* tab, int lane, int px, const unsigned* zb, const unsigned* w0,
                                              const unsigned* w1, int Z, int& unz) {
  const unsigned z0 = zb[0];
  bool lane_same = true;
#pragma unroll
  for (int j = 1; j < 4; ++j) lane_same = lane_same && (j >= px || zb[j] == z0);
  const unsigned zref = (unsigned)__builtin_amdgcn_readfirstlane((int)z0);
  const bool agree = px == 0 || (lane_same && z0 == zref);
  unsigned f[NC];                              // the lane's pixels folded: what it adds where its zones agree
#pragma unroll
  for (int c = 0; c < NC; ++c)
    f[c] = (zn_col<NC>(w0[0], w1[0], c) + zn_col<NC>(w0[1], w1[1], c)) + (zn_col<NC>(w0[2], w1[2], c) + zn_col<NC>(w0[3], w1[3], c));
  if (ZN_WAVE_PATH && __ballot(!agree) == 0ull) {   // wave-uniform: one zone for the whole wave
    if (zref >= (unsigned)Z) {
      unz += px;
      return;
    }
    unsigned mine = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const unsigned s = c < NCNT ? zn_wave_count(f[c]) : zn_wave_sum(f[c]);
      if (lane == c) mine = s;
    }
    if (lane < NC && mine) atomicAdd(&tab[zref * NC + lane], mine);
  } else if (lane_same) {
    if (px > 0) {
      if (z0 >= (unsigned)Z) {
        unz += px;
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (f[c]) atomicAdd(&tab[z0 * NC + c], f[c]);
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        if (zb[j] >= (unsigned)Z) {
          unz += 1;
        } else {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const unsigned v = zn_col<NC>(w0[j], w1[j], c);
            if (v) atomicAdd(&tab[zb[j] * NC + c], v);
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void zn_zero_kernel(unsigned long long* __restrict__ table, long n,
                                                      unsigned long long* __restrict__ unzoned, int nu) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) table[i] = 0ull;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < nu; i += 256) unzoned[i] = 0ull;
  }
}

// the workgroup's table and its unzoned count -> the owner's
template <int NC>
__device__ __forceinline__ void zn_flush(const unsigned* tab, int* red, int unz, int Z, int owner,
                                         unsigned long long* table, unsigned long long* unzoned) {
  const int tid = threadIdx.x;
  int s = unz;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();                             // (also ends the LDS updates)
  if (tid == 0) {
    const long long u = (long long)red[0] + red[1] + red[2] + red[3];
    if (u) __hip_atomic_fetch_add(unzoned + owner, (unsigned long long)u, ZN_RLX_AGENT);
  }
  for (int i = tid; i < Z * NC; i += 256) {
    const unsigned c = tab[i];
    if (c) __hip_atomic_fetch_add(table + (long)owner * Z * NC + i, (unsigned long long)c, ZN_RLX_AGENT);
  }
}

// LDS: the 256-entry OD table and unsigned [Z][8].  A workgroup takes fewer than 2^20 pixels (zn_blocks), so a cell
// holds less than 2^20 * 4095 < 2^32.
template <int LOADER>
__global__ __launch_bounds__(256) void zn_table_kernel(const ZnParams p, unsigned long long* __restrict__ table,
                                                       unsigned long long* __restrict__ unzoned) {
  __shared__ float lut[256];
  __shared__ unsigned tab[ZN_MAX_Z * 8];
  __shared__ int red[4];
  const int tid = threadIdx.x, lane = tid & 63, owner = blockIdx.y;
  lut[tid] = p.od[tid];                        // 256 lanes, 256 entries
  for (int i = tid; i < p.Z * 8; i += 256) tab[i] = 0u;
  __syncthreads();
  const int nq = (p.W + 3) >> 2;
  const long per = (long)p.rows * nq, total = per * p.spo;
  int unz = 0;
  // the wave's first quad is wave-uniform, so every lane stays in the loop while lane 0 has work
  for (long q0 = (long)blockIdx.x * 256 + (tid & ~63); q0 < total; q0 += (long)gridDim.x * 256) {
    const long q = q0 + lane;
    unsigned v[12] = {}, zb[4] = {}, w0[4] = {}, w1[4] = {};
    int px = 0;
    if (q < total) {
      const ZnQuad d = zn_quad(p, owner, q, nq, per);
      px = d.px;
      zn_load_quad<LOADER>(p.a, (long)d.n * p.img_a + (long)d.y * p.pitch_a, p.chan, d.x0, d.px, v);
      zn_load_zones(p.z + (long)d.n * p.img_z + (long)d.y * p.pitch_z + d.x0, d.px, zb);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const bool t = is_tissue(v[3 * j], v[3 * j + 1], v[3 * j + 2], p.white, p.black);
        const float odr = lut[v[3 * j]], odg = lut[v[3 * j + 1]], odb = lut[v[3 * j + 2]];
        unsigned w = t ? 3u : 1u, q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float c = zn_conc(odr, odg, odb, p.m[k], p.m[3 + k], p.m[6 + k]);
          w |= (t && c > p.thr[k]) ? 4u << k : 0u;
          q[k] = t ? zn_q(c) : 0u;
        }
        w0[j] = w | q[0] << 5 | q[1] << 17;
        w1[j] = q[2];
      }
    }
    zn_accumulate<8, 5>(tab, lane, px, zb, w0, w1, p.Z, unz);
  }
  zn_flush<8>(tab, red, unz, p.Z, owner, table, unzoned);
}

// LDS: the OD table and unsigned [Z][6]
template <int LOADER>
__global__ __launch_bounds__(256) void zn_pair_kernel(const ZnParams p, unsigned long long* __restrict__ table,
                                                      unsigned long long* __restrict__ unzoned) {
  __shared__ float lut[256];
  __shared__ unsigned tab[ZN_MAX_Z * 6];
  __shared__ int red[4];
  const int tid = threadIdx.x, lane = tid & 63, owner = blockIdx.y;
  const float mr = p.m[p.stain], mg = p.m[3 + p.stain], mb = p.m[6 + p.stain];
  const float thr = p.stain == 0 ? p.thr[0] : p.stain == 1 ? p.thr[1] : p.thr[2];
  lut[tid] = p.od[tid];
  for (int i = tid; i < p.Z * 6; i += 256) tab[i] = 0u;
  __syncthreads();
  const int nq = (p.W + 3) >> 2;
  const long per = (long)p.rows * nq, total = per * p.spo;
  int unz = 0;
  for (long q0 = (long)blockIdx.x * 256 + (tid & ~63); q0 < total; q0 += (long)gridDim.x * 256) {
    const long q = q0 + lane;
    unsigned va[12] = {}, vb[12] = {}, zb[4] = {}, w0[4] = {}, w1[4] = {};
    int px = 0;
    if (q < total) {
      const ZnQuad d = zn_quad(p, owner, q, nq, per);
      px = d.px;
      zn_load_quad<LOADER>(p.a, (long)d.n * p.img_a + (long)d.y * p.pitch_a, p.chan, d.x0, d.px, va);
      zn_load_quad<LOADER>(p.b, (long)d.n * p.img_b + (long)d.y * p.pitch_b, p.chan, d.x0, d.px, vb);
      zn_load_zones(p.z + (long)d.n * p.img_z + (long)d.y * p.pitch_z + d.x0, d.px, zb);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < px) {
        const bool ta = is_tissue(va[3 * j], va[3 * j + 1], va[3 * j + 2], p.white, p.black);
        const bool tb = is_tissue(vb[3 * j], vb[3 * j + 1], vb[3 * j + 2], p.white, p.black);
        const float ca = zn_conc(lut[va[3 * j]], lut[va[3 * j + 1]], lut[va[3 * j + 2]], mr, mg, mb);
        const float cb = zn_conc(lut[vb[3 * j]], lut[vb[3 * j + 1]], lut[vb[3 * j + 2]], mr, mg, mb);
        const bool pa = ta && ca > thr, pb = tb && cb > thr;
        w0[j] = 1u | (ta ? 2u : 0u) | (tb ? 4u : 0u) | ((pa && pb) ? 8u : 0u) | ((pa && !pb) ? 16u : 0u) |
                ((!pa && pb) ? 32u : 0u);
      }
    }
    zn_accumulate<6, 6>(tab, lane, px, zb, w0, w1, p.Z, unz);
  }
  zn_flush<6>(tab, red, unz, p.Z, owner, table, unzoned);
}

// One thread per (owner, zone).  The order of operations is the one include/stain2stain_hip.h spells out; no contraction.
__global__ __launch_bounds__(256) void zn_finalize_kernel(const long long* __restrict__ table,
                                                          const long long* __restrict__ unzoned, long cells, int Z,
                                                          int paired, double* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  if (paired) {
    const long long* t = table + i * 6;
    const long long ta = t[1], tb = t[2], both = t[3], na = t[3] + t[4], nb = t[3] + t[5], uni = t[3] + t[4] + t[5];
    const double ba = (double)na / (double)max(ta, 1LL);
    const double bb = (double)nb / (double)max(tb, 1LL);
    double* o = out + i * 5;
    o[0] = ba;
    o[1] = bb;
    o[2] = fabs(ba - bb);
    o[3] = (na + nb) == 0 ? 1.0 : (double)(2 * both) / (double)(na + nb);
    o[4] = uni == 0 ? 1.0 : (double)both / (double)uni;
    return;
  }
  const long owner = i / Z;
  const long long* t = table + i * 8;
  const long long pixels = t[0], tissue = t[1];
  long long all = unzoned[owner];
  for (int z = 0; z < Z; ++z) all += table[(owner * Z + z) * 8];
  const double td = (double)max(tissue, 1LL);
  double* o = out + i * 8;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = (double)t[2 + k] / td;
    const double mq = (double)t[5 + k] / td;
    o[3 + k] = mq / 1024.0;
  }
  o[6] = (double)tissue / (double)max(pixels, 1LL);
  o[7] = (double)pixels / (double)max(all, 1LL);
}

// ---- objects by zone ---------------------------------------------------------------------------------------------------
// Four pixels per lane.  A pixel whose label is in 1..M has the key (label - 1) (Z + 1) + min(zone byte, Z).  A round
// takes the first pending key of the first pending lane; every lane counts its pixels of that key, three ballots sum the
// counts over the wave, and lane 0 adds to overlap (zoned keys), lane 1 to area: rounds = distinct keys of the wave (the
// scheme of of_accumulate).
__global__ __launch_bounds__(256) void zn_object_overlap_kernel(const int* __restrict__ labels,
                                                                const unsigned char* __restrict__ zones, long pitch_z,
                                                                long img_z, int H, int W, int Z, int M,
                                                                int* __restrict__ overlap, int* __restrict__ area,
                                                                int* __restrict__ count) {
  __shared__ int s_top;
  const int tid = threadIdx.x, lane = tid & 63, n = blockIdx.y;
  if (tid == 0) s_top = 0;
  __syncthreads();
  const int nq = (W + 3) >> 2;
  const long total = (long)H * nq;             // < 2^31
  const int* lab = labels + (long)n * H * W;
  const unsigned char* zn = zones + (long)n * img_z;
  const unsigned Z1 = (unsigned)Z + 1u;
  int top = 0;
  for (long q0 = (long)blockIdx.x * 256 + (tid & ~63); q0 < total; q0 += (long)gridDim.x * 256) {
    const long q = q0 + lane;
    int l[4] = {0, 0, 0, 0};
    unsigned zb[4] = {};
    int px = 0;
    if (q < total) {
      const int y = (int)((unsigned)q / (unsigned)nq), x0 = 4 * (int)((unsigned)q - (unsigned)y * (unsigned)nq);
      px = min(4, W - x0);
      const int* lp = lab + (long)y * W + x0;
      if (px == 4 && ((uintptr_t)lp & 15) == 0) {
        const int4 q4 = *reinterpret_cast<const int4*>(lp);
        l[0] = q4.x; l[1] = q4.y; l[2] = q4.z; l[3] = q4.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < px) l[j] = lp[j];
      }
      zn_load_zones(zn + (long)y * pitch_z + x0, px, zb);
    }
    unsigned pend = 0, key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      top = max(top, l[j]);
      if (l[j] > 0 && l[j] <= M) pend |= 1u << j;
      key[j] = (unsigned)(l[j] - 1) * Z1 + min(zb[j], (unsigned)Z);
    }
    unsigned long long todo = __ballot(pend != 0);
    while (todo) {                                            // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned first = (pend & 1) ? key[0] : (pend & 2) ? key[1] : (pend & 4) ? key[2] : key[3];
      const unsigned lk = (unsigned)__shfl((int)first, leader, 64);
      unsigned c = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (((pend >> j) & 1) && key[j] == lk) {
          c += 1;
          pend &= ~(1u << j);
        }
      }
      todo = __ballot(pend != 0);
      const int cnt = (int)zn_wave_count(c);
      const unsigned m = lk / Z1, zc = lk - m * Z1;
      const long row = (long)n * M + m;
      if (lane == 0 && zc < (unsigned)Z) __hip_atomic_fetch_add(overlap + row * Z + zc, cnt, ZN_RLX_AGENT);
      if (lane == 1) __hip_atomic_fetch_add(area + row, cnt, ZN_RLX_AGENT);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
  if (lane == 0 && top > 0) atomicMax(&s_top, top);
  __syncthreads();
  if (tid == 0 && s_top > 0) __hip_atomic_fetch_max(count + n, s_top, ZN_RLX_AGENT);
}

// One wave per object row: the arg-max in the strict order (larger overlap, then smaller zone).
__global__ __launch_bounds__(256) void zn_object_assign_kernel(const int* __restrict__ overlap, const int* __restrict__ area,
                                                               const int* __restrict__ count, long rows, int M, int Z,
                                                               int* __restrict__ zone, long long* __restrict__ zone_pixels,
                                                               unsigned long long* __restrict__ objects,
                                                               unsigned long long* __restrict__ object_pixels) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                    // wave-uniform
  const long n = row / M;
  const int m = (int)(row - n * M);
  const bool live = m < min(count[n], M);
  int best = 0, bz = Z;
  if (live) {
    for (int z = lane; z < Z; z += 64) {                      // ascending z: the first maximum stays
      const int v = overlap[row * Z + z];
      if (v > best) {
        best = v;
        bz = z;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int ov = __shfl_xor(best, o, 64), oz = __shfl_xor(bz, o, 64);
    if (ov > best || (ov == best && oz < bz)) {
      best = ov;
      bz = oz;
    }
  }
  if (lane == 0) {
    if (live && best > 0) {
      zone[row] = bz;
      zone_pixels[row] = best;
      __hip_atomic_fetch_add(objects + n * Z + bz, 1ull, ZN_RLX_AGENT);
      __hip_atomic_fetch_add(object_pixels + n * Z + bz, (unsigned long long)area[row], ZN_RLX_AGENT);
    } else {
      zone[row] = -1;
      zone_pixels[row] = 0;
    }
  }
}

// per_mm2 = (double)objects / ((double)tissue * scale), 0 without tissue
__global__ __launch_bounds__(256) void zn_density_kernel(const long long* __restrict__ objects,
                                                         const long long* __restrict__ table, long cells, double scale,
                                                         double* __restrict__ per_mm2) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const long long tissue = table[i * 8 + 1];
  const double areamm = (double)tissue * scale;
  per_mm2[i] = tissue > 0 ? (double)objects[i] / areamm : 0.0;
}

// ---- distance bands ----------------------------------------------------------------------------------------------------
struct ZnEdges {
  int n;
  int e[ZN_MAX_EDGES];
};

// #{i : d > E_i}, E ascending in LDS: the first index whose E is not below d
__device__ __forceinline__ int zn_band(const int* E, int n, int d) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (E[mid] < d) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned zn_band_byte(const int* E, int n, int side, int dbg, int dfg) {
  if (dbg > 0) return side == 2 ? 255u : (unsigned)zn_band(E, n, dbg);           // foreground: d2_bg > 0
  return side == 1 ? 255u : (unsigned)(n + 1 + zn_band(E, n, dfg));
}

// side 0: both, 1: inside, 2: outside.  The maps and the result are dense; four pixels per lane, one dword store.
__global__ __launch_bounds__(256) void zn_bands_kernel(const int* __restrict__ d2_bg, const int* __restrict__ d2_fg,
                                                       long pixels, const ZnEdges ed, int side,
                                                       unsigned char* __restrict__ out) {
  __shared__ int E[128];
  if (threadIdx.x < 128) E[threadIdx.x] = threadIdx.x < ed.n ? ed.e[threadIdx.x] : ZN_FAR;
  __syncthreads();
  const long nq = (pixels + 3) >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
    const long i = 4 * q;
    if (i + 4 <= pixels) {                     // (the bases are 16- and 4-byte aligned: the entry point checks)
      const int4 a = *reinterpret_cast<const int4*>(d2_bg + i), b = *reinterpret_cast<const int4*>(d2_fg + i);
      const unsigned w = zn_band_byte(E, ed.n, side, a.x, b.x) | zn_band_byte(E, ed.n, side, a.y, b.y) << 8 |
                         zn_band_byte(E, ed.n, side, a.z, b.z) << 16 | zn_band_byte(E, ed.n, side, a.w, b.w) << 24;
      *reinterpret_cast<unsigned*>(out + i) = w;
    } else {
      for (long k = i; k < pixels; ++k) out[k] = (unsigned char)zn_band_byte(E, ed.n, side, d2_bg[k], d2_fg[k]);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int zn_fill(ZnParams& p, int B, int rows, int H, int W, int Z, const float* od_table, const float* unmix, int white,
            int black, int pool) {
  if (!od_table || !unmix) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 30) || W > (1 << 30) || white < 1 || white > 256 || black < 0 ||
      black > 255 || Z < 1 || Z > ZN_MAX_Z)
    return S2S_ERR_SHAPE;
  if ((long)H * W > ZN_MAX_PIXELS / (pool ? B : 1)) return S2S_ERR_SHAPE;     // an owner holds at most 2^40 pixels
  p.rows = rows;
  p.W = W;
  p.spo = pool ? B : 1;
  p.white = white;
  p.black = black;
  p.Z = Z;
  p.stain = 0;
  for (int i = 0; i < 9; ++i) p.m[i] = unmix[i];
  for (int i = 0; i < 3; ++i) p.thr[i] = unmix[9 + i];
  for (int i = 0; i < 256; ++i) p.od[i] = od_table[i];
  p.b = nullptr;
  p.pitch_b = p.img_b = 0;
  p.chan = 0;
  return S2S_OK;
}

// workgroups per owner, all owners together at most one resident round (a second round would run at a fraction of the
// machine); 0: a workgroup would take 2^20 pixels or more and a uint32 LDS cell could wrap
unsigned zn_blocks(long quads, int owners, int resident) {
  long cap = (long)ZN_CUS * resident / owners;
  if (cap < 1) cap = 1;
  long blocks = (quads + 256L * ZN_QUADS - 1) / (256L * ZN_QUADS);
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const long per_thread = (quads + blocks * 256 - 1) / (blocks * 256);
  return per_thread * 1024 >= ZN_MAX_WG_PIXELS ? 0u : (unsigned)blocks;
}

int zn_layout(long pitch, long img, int channels, int B, int band_top, int band_h, int H, int W) {
  if (pitch < (long)channels * W || band_top < 0 || band_h < 1 || (long)band_top + band_h > H) return S2S_ERR_SHAPE;
  if (B > 1 && img < pitch * (long)band_h) return S2S_ERR_SHAPE;
  return S2S_OK;
}

template <int LOADER>
int zn_launch(const ZnParams& p, int B, int pool, bool paired, int reset, long* table, long* unzoned, hipStream_t s) {
  const int owners = pool ? 1 : B;
  const unsigned blocks = zn_blocks((long)p.spo * p.rows * cdiv(p.W, 4), owners, paired ? ZN_RESIDENT_PAIR : ZN_RESIDENT_TABLE);
  if (!blocks) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(unsigned long long), "int64 counts");
  unsigned long long* t = (unsigned long long*)table;
  unsigned long long* u = (unsigned long long*)unzoned;
  if (reset) {
    const long n = (long)owners * p.Z * (paired ? 6 : 8);
    const long zb = (n + 255) / 256;
    hipLaunchKernelGGL(zn_zero_kernel, dim3((unsigned)(zb > 1024 ? 1024 : zb)), dim3(256), 0, s, t, n, u, owners);
    S2S_LAUNCH_CHECK();
  }
  const dim3 grid(blocks, (unsigned)owners);
  if (paired) hipLaunchKernelGGL(zn_pair_kernel<LOADER>, grid, dim3(256), 0, s, p, t, u);
  else hipLaunchKernelGGL(zn_table_kernel<LOADER>, grid, dim3(256), 0, s, p, t, u);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

}  // namespace

extern "C" int s2s_zonal_u8(const void* img, long pitch, long img_stride, const void* zones, long zone_pitch,
                            long zone_stride, int B, int band_top, int band_h, int H, int W, int num_zones,
                            const float* od_table, const float* unmix, int white, int black, int pool, int reset,
                            long* table, long* unzoned, void* stream) {
  if (!img || !zones || !table || !unzoned) return S2S_ERR_NULL;
  ZnParams p;
  int rc = zn_fill(p, B, band_h, H, W, num_zones, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = zn_layout(pitch, img_stride, 3, B, band_top, band_h, H, W);
  if (rc == S2S_OK) rc = zn_layout(zone_pitch, zone_stride, 1, B, band_top, band_h, H, W);
  if (rc != S2S_OK) return rc;
  p.a = img;
  p.pitch_a = pitch;
  p.img_a = img_stride;
  p.z = (const unsigned char*)zones;
  p.pitch_z = zone_pitch;
  p.img_z = zone_stride;
  return zn_launch<ZN_U8>(p, B, pool, false, reset, table, unzoned, (hipStream_t)stream);
}

extern "C" int s2s_zonal_f32(const float* img, const void* zones, long zone_pitch, long zone_stride, int B, int H, int W,
                             int num_zones, const float* od_table, const float* unmix, int white, int black, int pool,
                             int reset, long* table, long* unzoned, void* stream) {
  if (!img || !zones || !table || !unzoned) return S2S_ERR_NULL;
  ZnParams p;
  int rc = zn_fill(p, B, H, H, W, num_zones, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = zn_layout(zone_pitch, zone_stride, 1, B, 0, H, H, W);
  if (rc != S2S_OK) return rc;
  p.a = img;
  p.pitch_a = W;
  p.chan = (long)H * W;
  p.img_a = 3L * H * W;
  p.z = (const unsigned char*)zones;
  p.pitch_z = zone_pitch;
  p.img_z = zone_stride;
  return zn_launch<ZN_F32>(p, B, pool, false, reset, table, unzoned, (hipStream_t)stream);
}

extern "C" int s2s_zonal_pair_u8(const void* a, long pitch_a, long img_a, const void* b, long pitch_b, long img_b,
                                 const void* zones, long zone_pitch, long zone_stride, int B, int band_top, int band_h,
                                 int H, int W, int num_zones, const float* od_table, const float* unmix, int white,
                                 int black, int stain, int pool, int reset, long* table, long* unzoned, void* stream) {
  if (!a || !b || !zones || !table || !unzoned) return S2S_ERR_NULL;
  ZnParams p;
  int rc = zn_fill(p, B, band_h, H, W, num_zones, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = zn_layout(pitch_a, img_a, 3, B, band_top, band_h, H, W);
  if (rc == S2S_OK) rc = zn_layout(pitch_b, img_b, 3, B, band_top, band_h, H, W);
  if (rc == S2S_OK) rc = zn_layout(zone_pitch, zone_stride, 1, B, band_top, band_h, H, W);
  if (rc != S2S_OK) return rc;
  if (stain < 0 || stain > 2) return S2S_ERR_SHAPE;
  p.a = a;
  p.pitch_a = pitch_a;
  p.img_a = img_a;
  p.b = b;
  p.pitch_b = pitch_b;
  p.img_b = img_b;
  p.z = (const unsigned char*)zones;
  p.pitch_z = zone_pitch;
  p.img_z = zone_stride;
  p.stain = stain;
  return zn_launch<ZN_U8>(p, B, pool, true, reset, table, unzoned, (hipStream_t)stream);
}

extern "C" int s2s_zonal_pair_f32(const float* a, const float* b, const void* zones, long zone_pitch, long zone_stride,
                                  int B, int H, int W, int num_zones, const float* od_table, const float* unmix,
                                  int white, int black, int stain, int pool, int reset, long* table, long* unzoned,
                                  void* stream) {
  if (!a || !b || !zones || !table || !unzoned) return S2S_ERR_NULL;
  ZnParams p;
  int rc = zn_fill(p, B, H, H, W, num_zones, od_table, unmix, white, black, pool);
  if (rc == S2S_OK) rc = zn_layout(zone_pitch, zone_stride, 1, B, 0, H, H, W);
  if (rc != S2S_OK) return rc;
  if (stain < 0 || stain > 2) return S2S_ERR_SHAPE;
  p.a = a;
  p.b = b;
  p.pitch_a = p.pitch_b = W;
  p.chan = (long)H * W;
  p.img_a = p.img_b = 3L * H * W;
  p.z = (const unsigned char*)zones;
  p.pitch_z = zone_pitch;
  p.img_z = zone_stride;
  p.stain = stain;
  return zn_launch<ZN_F32>(p, B, pool, true, reset, table, unzoned, (hipStream_t)stream);
}

extern "C" int s2s_zonal_finalize(const long* table, const long* unzoned, long owners, int num_zones, int paired,
                                  double* out, void* stream) {
  if (!table || !out || (!paired && !unzoned)) return S2S_ERR_NULL;
  if (owners < 1 || owners > 0x7fffffffL || num_zones < 1 || num_zones > ZN_MAX_Z) return S2S_ERR_SHAPE;
  static_assert(sizeof(long) == sizeof(long long), "int64 counts");
  const long cells = owners * num_zones;
  hipLaunchKernelGGL(zn_finalize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)table, (const long long*)unzoned, cells, num_zones, paired ? 1 : 0, out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

static int zn_object_shape(int B, int H, int W, int Z, int M) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > ZN_MAX_SIDE || W > ZN_MAX_SIDE || Z < 1 || Z > ZN_MAX_Z || M < 1)
    return S2S_ERR_SHAPE;
  if ((long)B * M >= (1L << 31) || (long)B * M * Z >= (1L << 31)) return S2S_ERR_SHAPE;
  return S2S_OK;
}

extern "C" int s2s_zonal_object_overlap(const int* labels, const void* zones, long zone_pitch, long zone_stride, int B,
                                        int H, int W, int num_zones, int max_objects, int* overlap, int* area, int* count,
                                        void* stream) {
  if (!labels || !zones || !overlap || !area || !count) return S2S_ERR_NULL;
  int rc = zn_object_shape(B, H, W, num_zones, max_objects);
  if (rc == S2S_OK) rc = zn_layout(zone_pitch, zone_stride, 1, B, 0, H, H, W);
  if (rc != S2S_OK) return rc;
  const long quads = (long)H * cdiv(W, 4);
  long cap = (long)ZN_CUS * ZN_RESIDENT / B;
  if (cap < 1) cap = 1;
  long blocks = (quads + 256L * ZN_QUADS - 1) / (256L * ZN_QUADS);
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(zn_object_overlap_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     labels, (const unsigned char*)zones, zone_pitch, zone_stride, H, W, num_zones, max_objects, overlap,
                     area, count);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_zonal_object_assign(const int* overlap, const int* area, const int* count, int B, int num_zones,
                                       int max_objects, int* zone, long* zone_pixels, long* objects, long* object_pixels,
                                       void* stream) {
  if (!overlap || !area || !count || !zone || !zone_pixels || !objects || !object_pixels) return S2S_ERR_NULL;
  const int rc = zn_object_shape(B, 1, 1, num_zones, max_objects);
  if (rc != S2S_OK) return rc;
  const long rows = (long)B * max_objects;
  hipLaunchKernelGGL(zn_object_assign_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, overlap,
                     area, count, rows, max_objects, num_zones, zone, (long long*)zone_pixels,
                     (unsigned long long*)objects, (unsigned long long*)object_pixels);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_zonal_object_density(const long* objects, const long* table, long owners, int num_zones,
                                        const double* scale, double* per_mm2, void* stream) {
  if (!objects || !table || !scale || !per_mm2) return S2S_ERR_NULL;
  if (owners < 1 || owners > 0x7fffffffL || num_zones < 1 || num_zones > ZN_MAX_Z || !(scale[0] > 0.0) ||
      !(scale[0] < 1e300))
    return S2S_ERR_SHAPE;
  const long cells = owners * num_zones;
  hipLaunchKernelGGL(zn_density_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)objects, (const long long*)table, cells, scale[0], per_mm2);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}

extern "C" int s2s_zonal_bands(const int* d2_bg, const int* d2_fg, int B, int H, int W, const int* edges2, int n, int side,
                               void* out, void* stream) {
  if (!d2_bg || !d2_fg || !edges2 || !out) return S2S_ERR_NULL;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > ZN_MAX_SIDE || W > ZN_MAX_SIDE || n < 1 || n > ZN_MAX_EDGES ||
      side < 0 || side > 2)
    return S2S_ERR_SHAPE;
  ZnEdges ed;
  ed.n = n;
  for (int i = 0; i < ZN_MAX_EDGES; ++i) ed.e[i] = ZN_FAR;
  for (int i = 0; i < n; ++i) {
    if (edges2[i] < 0 || edges2[i] >= ZN_FAR || (i > 0 && edges2[i] < edges2[i - 1])) return S2S_ERR_SHAPE;
    ed.e[i] = edges2[i];
  }
  if (((uintptr_t)d2_bg & 15) || ((uintptr_t)d2_fg & 15) || ((uintptr_t)out & 3)) return S2S_ERR_ALIGN;
  const long pixels = (long)B * H * W;
  long blocks = ((pixels + 3) / 4 + 255) / 256;
  if (blocks > ZN_CUS * ZN_RESIDENT) blocks = ZN_CUS * ZN_RESIDENT;
  hipLaunchKernelGGL(zn_bands_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d2_bg, d2_fg, pixels, ed,
                     side, (unsigned char*)out);
  S2S_LAUNCH_CHECK();
  return S2S_OK;
}
