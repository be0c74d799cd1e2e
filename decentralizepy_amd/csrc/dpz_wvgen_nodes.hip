// Generic-filter multilevel DWT / IDWT of every node of a table per launch (dpz_dwt_generic_nodes /
// dpz_idwt_generic_nodes): the transforms of the batched JWINS round for every wavelet and level
// the fused sym2 kernels do not serve (decentralizepy_amd/gossip_jwins_batch.py,
// JwinsWaveletBatchRound).  Per node bit for bit dpz_dwt_generic / dpz_idwt_generic, that is
// PyWavelets 1.1.1 (mode "symmetric"); the summation orders are written at the head of
// dpz_wvgen.hip and -ffp-contract=off is load-bearing here as there.
//
// One launch per level, the grid tiles x (node, stream); stream 0 is W(x), stream 1 W(x - x0).
//
// Forward.  A block owns WN_T consecutive output pairs (approximation, detail) of one (node,
// stream) and stages the 2 WN_T + F - 2 inputs they read into LDS once, with 16-byte loads where
// the group lies inside the row (rows are 16-byte aligned) and pywt's half-sample symmetric
// extension resolved per element at the two array ends only.  The staged tile is split into its
// two polyphase halves: E[q] = x~[base + 2q], O[q] = x~[base + 2q + 1] with base = 2 o0 - F + 2,
// so that output o0 + r reads, for the tap pair (2jj, 2jj + 1), O[r + F/2 - 1 - jj] and then
// E[r + F/2 - 1 - jj]: consecutive lanes read consecutive LDS words (an interleaved tile would be
// read at a stride of two words, two lanes to a bank).  A thread owns the WN_R outputs r = tid +
// 256 c; the tap loop is the outer one, so the four taps of a pair are read once (scalar loads:
// every tap index is wave-uniform) for all of the thread's sums, and each LDS value feeds both
// filters.  The outputs past the input's end (i = 2o + 1 >= n, fewer than F/2 per level) take
// pywt's other order (extension terms first) in a second pass, with per-lane tap indices served
// from a 2F-float LDS copy of the taps.  At level 1 of the pair mode the block reads x and x0
// from HBM once and forms both the x tile and the fl(x - x0) tile from them.
// Intermediate approximations ping-pong in the workspace (per node and stream two rows of
// up4(len[1]) floats); details and the top approximation go straight into the coefficient rows,
// added there in accumulate mode (stream 1 only; no rewind mask: the batched encode rewinds).
//
// Inverse.  A block owns 2 WN_T consecutive outputs of one node's level: it stages WN_T + F/2 - 1
// values of a and of d, and each thread forms both parities y[2m], y[2m + 1] of its WN_R
// positions from the same LDS reads: four sums, (0 + sa) + sd each, stored as one 8-byte word.
//
// LDS per block: forward 2 (WN_T + 32) floats per staged stream + 128 taps = 8.75 KiB (17 KiB
// for the level-1 pair), inverse 8.25 KiB: 9 or more blocks fit a CU's 160 KiB, more than its 8
// resident blocks of 256 threads.
#include "dpz_wvgen.h"

namespace dpz {

constexpr int WN_T = 1024;                   // output pairs (forward) / positions (inverse) a block
constexpr int WN_R = WN_T / 256;             // of them a thread
constexpr int WN_HALF = WN_T + WG_FMAX / 2;  // one LDS array; WN_T + F/2 - 1 words of it are used
static_assert(WN_T % 256 == 0 && WN_HALF % 4 == 0, "whole threads, whole 16-byte groups");

struct WnDwtNode {  // 4 64-bit words
  const float* x;
  const float* x0;
  float* cx;  // or NULL
  float* cd;  // or NULL
};
static_assert(sizeof(WnDwtNode) == 32, "4 64-bit words");

struct WnIdwtNode {  // 2 64-bit words
  const float* coeffs;
  float* out;
};
static_assert(sizeof(WnIdwtNode) == 16, "2 64-bit words");

// one level's launch
struct WnLevel {
  const void* tab;
  const float* bank;
  float* ws;
  int64_t nin, nout;  // forward: input / output length; inverse: len[l] / outputs written
  int64_t doff;       // cD_l in the coefficient row
  int64_t wsrow;      // floats a workspace row (4 per node: stream, ping-pong)
  int F, l, level;
  int S, s0;  // forward past level 1: streams in the grid's y, the first of them
  int acc;    // forward: stream 1 adds into its coefficient row
};

__device__ __forceinline__ float* wn_ws_row(const WnLevel& P, int node, int s, int l) {
  return P.ws + (size_t)(4 * node + 2 * s + (l & 1)) * (size_t)P.wsrow;
}

// MODE 0: one stream from one row (x at level 1, the workspace after it); 1: fl(x - x0), level 1;
// 2: both, level 1.  E / O: the polyphase halves of x~[base, base + 2 half), [0] the block's
// first (or only) stream, [1] the difference in MODE 2.
template <int MODE>
__device__ __forceinline__ void wn_stage(const float* __restrict__ in,
                                         const float* __restrict__ in0, int64_t n, int64_t base,
                                         int half, float (*E)[WN_HALF], float (*O)[WN_HALF]) {
  const int64_t g0 = base & ~(int64_t)3;  // base is even: g0 - base is 0 or -2
  const int nvec = (int)((base + 2 * half - g0 + 3) >> 2);
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const int64_t g = g0 + 4 * (int64_t)v;
    float a[4], b[4];
    if (g >= 0 && g + 3 < n) {
      const float4 q = *reinterpret_cast<const float4*>(in + g);
      a[0] = q.x, a[1] = q.y, a[2] = q.z, a[3] = q.w;
      if (MODE != 0) {
        const float4 q0 = *reinterpret_cast<const float4*>(in0 + g);
        b[0] = q0.x, b[1] = q0.y, b[2] = q0.z, b[3] = q0.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t p = wg_ext(g + k, n);
        const bool ok = p >= 0 && p < n;  // past one reflection: read by no output that is stored
        a[k] = ok ? in[p] : 0.0f;
        if (MODE != 0) b[k] = ok ? in0[p] : 0.0f;
      }
    }
    const int q = (int)(g - base) >> 1;  // -1 for the two words before base
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (q + h < 0 || q + h >= half) continue;
      if (MODE == 1) {
        E[0][q + h] = a[2 * h] - b[2 * h];
        O[0][q + h] = a[2 * h + 1] - b[2 * h + 1];
      } else {
        E[0][q + h] = a[2 * h];
        O[0][q + h] = a[2 * h + 1];
      }
      if (MODE == 2) {
        E[1][q + h] = a[2 * h] - b[2 * h];
        O[1][q + h] = a[2 * h + 1] - b[2 * h + 1];
      }
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(256) wn_dwt_kernel(const WnLevel P) {
  constexpr int NS = MODE == 2 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float E[NS][WN_HALF];
  __shared__ __attribute__((aligned(16))) float O[NS][WN_HALF];
  __shared__ float tp[2 * WG_FMAX];  // dec_lo, dec_hi: the overhang outputs' per-lane tap reads
  const int tid = threadIdx.x;
  const int F = P.F, F2 = F >> 1;
  const int node = MODE == 0 ? (int)blockIdx.y / P.S : (int)blockIdx.y;
  const int s = MODE == 0 ? P.s0 + (int)blockIdx.y % P.S : (MODE == 1 ? 1 : 0);
  const WnDwtNode nd = static_cast<const WnDwtNode*>(P.tab)[node];
  const float* in = (MODE != 0 || P.l == 1) ? nd.x : wn_ws_row(P, node, s, P.l - 1);
  const float* __restrict__ lo = P.bank;
  const float* __restrict__ hi = P.bank + F;
  const int64_t n = P.nin;
  const int64_t o0 = (int64_t)blockIdx.x * WN_T;
  const int half = WN_T + F2 - 1;
  if (tid < 2 * F) tp[tid] = P.bank[tid];
  wn_stage<MODE>(in, nd.x0, n, 2 * o0 - F + 2, half, E, O);
  __syncthreads();

  float sa[NS][WN_R], sd[NS][WN_R];
#pragma unroll
  for (int k = 0; k < NS; ++k)
#pragma unroll
    for (int c = 0; c < WN_R; ++c) sa[k][c] = 0.0f, sd[k][c] = 0.0f;
  for (int jj = 0; jj < F2; ++jj) {  // taps 2jj (an odd sample), then 2jj + 1 (the even before it)
    const float l0 = lo[2 * jj], l1 = lo[2 * jj + 1], h0 = hi[2 * jj], h1 = hi[2 * jj + 1];
    const int q = F2 - 1 - jj + tid;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int c = 0; c < WN_R; ++c) {
        const float vo = O[k][q + 256 * c], ve = E[k][q + 256 * c];
        sa[k][c] = sa[k][c] + l0 * vo;
        sd[k][c] = sd[k][c] + h0 * vo;
        sa[k][c] = sa[k][c] + l1 * ve;
        sd[k][c] = sd[k][c] + h1 * ve;
      }
  }

  const bool top = P.l == P.level;
#pragma unroll
  for (int c = 0; c < WN_R; ++c) {
    const int r = tid + 256 * c;
    const int64_t o = o0 + r;
    if (o >= P.nout) continue;
    const int64_t i = 2 * o + 1;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      float a = sa[k][c], d = sd[k][c];
      if (i >= n) {  // the right overhang: the e extension terms first, j = e-1 .. 0, then e .. F-1
        const int e = (int)(i - n + 1);
        a = 0.0f, d = 0.0f;
        for (int j = e - 1; j >= 0; --j) {
          const int p = 2 * r + F - 1 - j;
          const float v = (p & 1) ? O[k][p >> 1] : E[k][p >> 1];
          a = a + tp[j] * v;
          d = d + tp[F + j] * v;
        }
        for (int j = e; j < F; ++j) {
          const int p = 2 * r + F - 1 - j;
          const float v = (p & 1) ? O[k][p >> 1] : E[k][p >> 1];
          a = a + tp[j] * v;
          d = d + tp[F + j] * v;
        }
      }
      const int st = s + k;
      float* const coeffs = st ? nd.cd : nd.cx;
      float* const dout = coeffs + P.doff;
      const bool acc = P.acc && st == 1;
      if (!top) wn_ws_row(P, node, st, P.l)[o] = a;
      else coeffs[o] = acc ? coeffs[o] + a : a;
      dout[o] = acc ? dout[o] + d : d;
    }
  }
}

// cnt words of src from g0 on into dst (zero past len), 16-byte loads where src + g0 allows
__device__ __forceinline__ void wn_stage_lin(float* dst, const float* __restrict__ src, int64_t g0,
                                             int cnt, int64_t len) {
  const bool vec = aligned16(src + g0);
  for (int v = threadIdx.x; 4 * v < cnt; v += 256) {
    const int64_t g = g0 + 4 * (int64_t)v;
    float4 q;
    if (vec && g + 3 < len) {
      q = *reinterpret_cast<const float4*>(src + g);
    } else {
      q.x = g < len ? src[g] : 0.0f;
      q.y = g + 1 < len ? src[g + 1] : 0.0f;
      q.z = g + 2 < len ? src[g + 2] : 0.0f;
      q.w = g + 3 < len ? src[g + 3] : 0.0f;
    }
    *reinterpret_cast<float4*>(dst + 4 * v) = q;  // cnt < WN_HALF, which is a multiple of 4
  }
}

__global__ void __launch_bounds__(256) wn_idwt_kernel(const WnLevel P) {
  __shared__ __attribute__((aligned(16))) float A[WN_HALF];
  __shared__ __attribute__((aligned(16))) float D[WN_HALF];
  const int tid = threadIdx.x;
  const int F = P.F, F2 = F >> 1;
  const int node = blockIdx.y;
  const WnIdwtNode nd = static_cast<const WnIdwtNode*>(P.tab)[node];
  const float* a = P.l == P.level ? nd.coeffs : wn_ws_row(P, node, 0, P.l + 1);
  float* const y = P.l == 1 ? nd.out : wn_ws_row(P, node, 0, P.l);
  const float* __restrict__ rl = P.bank + 2 * F;
  const float* __restrict__ rh = P.bank + 3 * F;
  const int64_t m0 = (int64_t)blockIdx.x * WN_T;
  wn_stage_lin(A, a, m0, WN_T + F2 - 1, P.nin);
  wn_stage_lin(D, nd.coeffs + P.doff, m0, WN_T + F2 - 1, P.nin);
  __syncthreads();

  float sa[2][WN_R], sd[2][WN_R];
#pragma unroll
  for (int c = 0; c < WN_R; ++c) sa[0][c] = sa[1][c] = sd[0][c] = sd[1][c] = 0.0f;
  for (int j = 0; j < F2; ++j) {
    const float r0 = rl[2 * j], r1 = rl[2 * j + 1], h0 = rh[2 * j], h1 = rh[2 * j + 1];
    const int q = F2 - 1 - j + tid;
#pragma unroll
    for (int c = 0; c < WN_R; ++c) {
      const float va = A[q + 256 * c], vd = D[q + 256 * c];
      sa[0][c] = sa[0][c] + r0 * va;
      sa[1][c] = sa[1][c] + r1 * va;
      sd[0][c] = sd[0][c] + h0 * vd;
      sd[1][c] = sd[1][c] + h1 * vd;
    }
  }
#pragma unroll
  for (int c = 0; c < WN_R; ++c) {
    const int64_t o = 2 * (m0 + tid + 256 * c);
    float2 v;
    v.x = 0.0f + sa[0][c];
    v.x = v.x + sd[0][c];
    v.y = 0.0f + sa[1][c];
    v.y = v.y + sd[1][c];
    if (o + 1 < P.nout) *reinterpret_cast<float2*>(y + o) = v;  // rows are 16-byte aligned
    else if (o < P.nout) y[o] = v.x;
  }
}

static inline bool wn_row16(uint64_t p) { return (p & 15u) == 0; }

static inline int64_t wn_wsrow(const WgLevels& L) { return (L.len[1] + 3) & ~(int64_t)3; }

static size_t wn_ws_bytes(int m, const WgLevels& L, int level) {
  // per node: two streams x two ping-pong rows of the longest intermediate approximation
  return level >= 2 ? (size_t)m * 4 * (size_t)wn_wsrow(L) * sizeof(float) : 0;
}

static unsigned wn_tiles(int64_t n) { return (unsigned)((n + WN_T - 1) / WN_T); }

}  // namespace dpz

using namespace dpz;

extern "C" int64_t dpz_wvgen_tile_width(void) { return WN_T; }

extern "C" size_t dpz_wavelet_generic_nodes_workspace_bytes(int m, int64_t n, int level,
                                                            int flen) {
  WgLevels L;
  if (m < 1 || !wg_levels(n, level, flen, &L)) return 0;
  return wn_ws_bytes(m, L, level);
}

extern "C" int dpz_dwt_generic_nodes(int m, const void* table, const void* host_table, int64_t n,
                                     int level, const float* bank, int flen, int accumulate,
                                     void* ws, size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || !bank || n <= 0) return DPZ_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(table) & 7u) return DPZ_ERR_ARG;
  const uint64_t* h = static_cast<const uint64_t*>(host_table);
  const bool wx = h[2] != 0, wd = h[3] != 0;
  for (int j = 0; j < m; ++j) {  // every check on the host copy, before anything is enqueued
    const uint64_t* e = h + 4 * (size_t)j;
    if ((e[2] != 0) != wx || (e[3] != 0) != wd) return DPZ_ERR_ARG;  // one set of outputs
    if (!e[0] || (wd && !e[1])) return DPZ_ERR_ARG;
    if (!wn_row16(e[0]) || !wn_row16(e[1]) || !wn_row16(e[2]) || !wn_row16(e[3]))
      return DPZ_ERR_ARG;
  }
  if (accumulate && !wd) return DPZ_ERR_ARG;
  if (m > 32767) return DPZ_ERR_UNSUPPORTED;  // (node, stream) in the grid's y
  WgLevels L;
  if (!wg_levels(n, level, flen, &L)) return DPZ_ERR_UNSUPPORTED;
  if (!wx && !wd) return DPZ_OK;
  if (level >= 2 && ws && (reinterpret_cast<uintptr_t>(ws) & 15u)) return DPZ_ERR_ARG;
  if (level >= 2 && (!ws || ws_bytes < wn_ws_bytes(m, L, level))) return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  WnLevel P;
  P.tab = table, P.bank = bank, P.ws = static_cast<float*>(ws), P.wsrow = wn_wsrow(L);
  P.F = flen, P.level = level, P.acc = accumulate ? 1 : 0;
  P.S = (wx ? 1 : 0) + (wd ? 1 : 0), P.s0 = wx ? 0 : 1;
  for (int l = 1; l <= level; ++l) {
    P.l = l, P.nin = L.len[l - 1], P.nout = L.len[l], P.doff = L.doff[l];
    const unsigned tiles = wn_tiles(P.nout);
    if (l > 1) {
      DPZ_TIMED(DPZ_KT_DWT, st,
                wn_dwt_kernel<0><<<dim3(tiles, (unsigned)(m * P.S)), 256, 0, st>>>(P));
    } else if (wx && wd) {
      DPZ_TIMED(DPZ_KT_DWT, st, wn_dwt_kernel<2><<<dim3(tiles, (unsigned)m), 256, 0, st>>>(P));
    } else if (wd) {
      DPZ_TIMED(DPZ_KT_DWT, st, wn_dwt_kernel<1><<<dim3(tiles, (unsigned)m), 256, 0, st>>>(P));
    } else {
      DPZ_TIMED(DPZ_KT_DWT, st, wn_dwt_kernel<0><<<dim3(tiles, (unsigned)m), 256, 0, st>>>(P));
    }
  }
  return DPZ_OK;
}

extern "C" int dpz_idwt_generic_nodes(int m, const void* table, const void* host_table, int64_t n,
                                      int level, const float* bank, int flen, void* ws,
                                      size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || !bank || n <= 0) return DPZ_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(table) & 7u) return DPZ_ERR_ARG;
  const uint64_t* h = static_cast<const uint64_t*>(host_table);
  for (int j = 0; j < m; ++j) {
    const uint64_t* e = h + 2 * (size_t)j;
    if (!e[0] || !e[1] || !wn_row16(e[0]) || !wn_row16(e[1])) return DPZ_ERR_ARG;
  }
  if (m > 32767) return DPZ_ERR_UNSUPPORTED;
  WgLevels L;
  if (!wg_levels(n, level, flen, &L)) return DPZ_ERR_UNSUPPORTED;
  if (level >= 2 && ws && (reinterpret_cast<uintptr_t>(ws) & 15u)) return DPZ_ERR_ARG;
  if (level >= 2 && (!ws || ws_bytes < wn_ws_bytes(m, L, level))) return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  WnLevel P;
  P.tab = table, P.bank = bank, P.ws = static_cast<float*>(ws), P.wsrow = wn_wsrow(L);
  P.F = flen, P.level = level, P.acc = 0, P.S = 1, P.s0 = 0;
  for (int l = level; l >= 1; --l) {
    // y has 2 (len_l - F/2 + 1) values = len_{l-1} or len_{l-1} + 1: pywt trims the one extra
    // before the next level, and n are kept of the last
    P.l = l, P.nin = L.len[l], P.nout = L.len[l - 1], P.doff = L.doff[l];
    DPZ_TIMED(DPZ_KT_IDWT, st,
              wn_idwt_kernel<<<dim3(wn_tiles((P.nout + 1) / 2), (unsigned)m), 256, 0, st>>>(P));
  }
  return DPZ_OK;
}
