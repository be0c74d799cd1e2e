// The windowed, one-read selection of the whole-topology round encodes: the second core beside
// select_nodes<Policy> (dpz_select_nodes.h), written against the same policy, with the same
// results bit for bit.  m nodes, the node in the grid's second dimension.
//
// A node keeps, per k slot, the exact threshold key T of its last selection (the prior).  The key
// window around it is the single-node path's (dpz_topk.h HINT_LO / HINT_HI, the +-1/16 window):
// lo = bits(T (1 - 1/16)), hi = bits(T (1 + 1/16)), both ends inside.  Three launches, then the
// exact core's launch set, which every node that hit leaves at once:
//
//   filter   the only stream over the input.  A block owns EX_CHUNK contiguous elements of one
//            node's row, each of its 4 waves WIN_R of them (a segment).  A wave forms the key
//            through the policy, which stores the key row (and does what the exact core's first
//            pass does: an idle node's full share), counts key > hi and appends every element
//            with key >= lo to the segment's own list: 4 ballots and mbcnt give the lane its
//            place, the entries go through the wave's ring in LDS and leave it 256 at a time, so
//            that the list stores are whole lines.  Indices ascend within a list and the lists
//            are in segment order: no atomic decides an order.  A list that would pass its
//            capacity stops growing; its count says so (the node misses).  Whole segments of
//            16-byte aligned rows are software-pipelined: the float4 loads of group j + 1 are
//            issued before group j is consumed (policy members raw4 / form4).
//   resolve  one block of 1024 per node.  Sums the segments' counts; with a usable window, no
//            overflow and above_hi <= k - 1 < above_lo it finds the exact k-th largest key T among
//            the candidates' keys by a 10/11/10-bit radix histogram in LDS and the ties to take.
//            T inside [lo, hi] is a hit: the block then counts key > T and key == T per segment
//            (a wave per list), scans them (ties go to the lowest indices, the rule of
//            select_scan_kernel), writes the row header and T as the slot's next prior.
//            status: 0 = no usable prior (the exact core runs), 1 = hit, 2 = miss (it runs too).
//   write    nodes that hit only: the ordered compaction FROM THE LISTS, a wave per segment;
//            every selected element goes through the policy's store.
//   exact    select_nodes<P>'s nine kernels in their WIN form: a node whose status is 1 leaves
//            every kernel before any barrier, as an idle node does; the first pass reads the key
//            row the filter stored (nothing is formed twice); the scan ends by writing its T as
//            the slot's prior.  Round 0, a changed k and every miss go this way, on the device:
//            nothing is read back.
// Integer atomics (LDS histograms) only; the result does not depend on the grid.
//
// The policy's further members:
//   kslot(nd, a)          the node's prior slot (< WIN_SLOTS); a prior counts only for the k it
//                         was found with
//   Raw, raw4(nd, a, i0, Raw&), form4(nd, a, i0, const Raw&, c)
//                         load4<true> of a whole aligned group, split at the loads' use
// store() gets the element's c from the list (an entry is c's bits and the index).
#pragma once
#include "dpz_select_nodes.h"

namespace dpz {

constexpr int WIN_R = EX_CHUNK / 4;  // elements per wave segment
constexpr int WIN_GROUPS = WIN_R / 256;
constexpr int WIN_RING = 512;        // entries of a wave's LDS ring (a group adds up to 256)
constexpr int WIN_FLUSH = 256;       // entries per flush: 2 x 1 KiB of whole lines
static_assert(WIN_R % 256 == 0 && WIN_R < 0x10000, "whole groups; two 16-bit counts per segment");

// The workspace: [status, m words][exact core, m node_ws][m window areas]; ctrl .. cidx are
// offsets into a node's window area, whose control block is a WinCtrl (dpz_select_nodes.h).  The
// lists weigh 8 * cap / WIN_R bytes per element: 2 n bytes per node up to alpha = 1/16.
struct WinWs {
  size_t status_bytes, exact_bytes;
  size_t ctrl, cnt, above, off, eqb, cbits, cidx, node_total, total;
  int64_t nseg, cap;
};

// The list capacity per segment, sized as the single-node path sizes its lists (fast_geom): a
// quarter of the segment, or 1.25 alpha + 5 % of it where alpha = k / n is above 1/16.
static inline int64_t win_cap(int64_t n, int64_t k) {
  const int64_t R = WIN_R;
  int64_t cap = ((R / 4) + 63) & ~int64_t(63);
  if (k > n / 16) {
    const double frac = 1.25 * (double)k / (double)n + 0.05;
    cap = ((int64_t)(frac * (double)R) + 63) & ~int64_t(63);
    if (cap > R) cap = R;
  }
  return cap < 64 ? 64 : cap;
}

static inline WinWs win_ws(int m, int64_t n, int64_t k) {
  WinWs L;
  L.nseg = node_ws(n).nblk * 4;
  L.cap = win_cap(n, k);
  L.status_bytes = align256((size_t)m * 4);
  L.exact_bytes = (size_t)m * node_ws(n).total;
  size_t o = 0;
  L.ctrl = o; o += align256(sizeof(WinCtrl));
  L.cnt = o; o += align256((size_t)L.nseg * 4);
  L.above = o; o += align256((size_t)L.nseg * 4);
  L.off = o; o += align256((size_t)L.nseg * 4);
  L.eqb = o; o += align256((size_t)L.nseg * 4);
  L.cbits = o; o += align256((size_t)L.nseg * L.cap * 4);
  L.cidx = o; o += align256((size_t)L.nseg * L.cap * 4);
  L.node_total = o;
  L.total = L.status_bytes + L.exact_bytes + (size_t)m * L.node_total;
  return L;
}

template <class A>
struct WinArgs {
  A p;  // the engine's
  uint32_t* status;
  char* ws;  // the nodes' window areas
  WinWs L;
  int64_t n;
};

// lanes below this one whose bit is set
__device__ __forceinline__ uint32_t win_mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The window of a prior threshold key; false: no usable prior.
__device__ __forceinline__ bool win_window(uint32_t T, uint32_t pk, uint32_t k, uint32_t& lo,
                                           uint32_t& hi) {
  lo = 0xFFFFFFFFu;
  hi = 0u;
  if (pk != k || T == 0u || T >= 0x7F800000u) return false;
  const float t = __uint_as_float(T);
  lo = __float_as_uint(t * HINT_LO);
  hi = __float_as_uint(t * HINT_HI);  // inf at most
  return true;
}

// One group of a wave: the 4 elements c of every lane from i0 (cnt inside), into the ring.
__device__ __forceinline__ void win_stage(const float c[4], int cnt, uint32_t i0, uint32_t lo,
                                          uint32_t hi, uint32_t* ring, uint32_t* gbits,
                                          uint32_t* gidx, uint32_t cap, int lane, uint32_t& run,
                                          uint32_t& flushed, uint32_t& above) {
  bool f[4];
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t kk = key_of(c[e]);
    f[e] = e < cnt && kk >= lo;
    above += (e < cnt && kk > hi) ? 1u : 0u;
    const uint64_t b = __ballot(f[e]);
    pre += win_mbcnt(b);
    tot += (uint32_t)__popcll(b);
  }
  if (!tot) return;  // uniform over the wave
  if (run <= cap) {  // a list past its capacity has stopped; its count stays above cap
    uint32_t p = run + pre;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (f[e]) {
        ring[2 * (p & (WIN_RING - 1))] = __float_as_uint(c[e]);
        ring[2 * (p & (WIN_RING - 1)) + 1] = i0 + e;
        ++p;
      }
    }
  }
  run += tot;
  if (run <= cap && run - flushed >= WIN_FLUSH) {
    __builtin_amdgcn_s_waitcnt(0xC07F);  // this wave's ring writes done
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int q = 0; q < WIN_FLUSH / 64; ++q) {
      const uint32_t j = flushed + q * 64 + lane;  // < run <= cap
      gbits[j] = ring[2 * (j & (WIN_RING - 1))];
      gidx[j] = ring[2 * (j & (WIN_RING - 1)) + 1];
    }
    __builtin_amdgcn_wave_barrier();
    flushed += WIN_FLUSH;
  }
}

template <class P>
__global__ void __launch_bounds__(256) window_filter_kernel(const WinArgs<typename P::Args> a) {
  __shared__ uint32_t rings[4][2 * WIN_RING];
  const typename P::Node nd = a.p.tab[blockIdx.y];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) {  // uniform over the block, before any barrier
      P::idle_share(nd, a.n);
      return;
    }
  }
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  char* ws = a.ws + (size_t)blockIdx.y * a.L.node_total;
  WinCtrl* ctrl = reinterpret_cast<WinCtrl*>(ws + a.L.ctrl);
  const int64_t seg = (int64_t)blockIdx.x * 4 + wid;
  const int64_t beg = seg * WIN_R;
  const bool vec = P::template vec<true>(nd, a.p);
  const bool whole = vec && beg + WIN_R <= a.n;
  const uint32_t slot = P::kslot(nd, a.p) & (WIN_SLOTS - 1);
  // the prior's loads and the first group's are issued together, then waited on
  const uint32_t pT = ctrl->prior_T[slot], pk = ctrl->prior_k[slot];
  typename P::Raw raw[2];
  if (whole) P::raw4(nd, a.p, beg + lane * 4, raw[0]);
  uint32_t lo, hi;
  win_window(pT, pk, P::k(nd, a.p, a.n), lo, hi);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->lo = lo;
    ctrl->hi = hi;
  }
  uint32_t* ring = rings[wid];
  const uint32_t cap = (uint32_t)a.L.cap;
  uint32_t* gbits = reinterpret_cast<uint32_t*>(ws + a.L.cbits) + (size_t)seg * cap;
  uint32_t* gidx = reinterpret_cast<uint32_t*>(ws + a.L.cidx) + (size_t)seg * cap;
  uint32_t run = 0, flushed = 0, above = 0;
  if (whole) {
#pragma unroll
    for (int j = 0; j < WIN_GROUPS; ++j) {
      const int64_t i0 = beg + j * 256 + lane * 4;
      if (j + 1 < WIN_GROUPS) P::raw4(nd, a.p, i0 + 256, raw[(j + 1) & 1]);
      float c[4];
      P::form4(nd, a.p, i0, raw[j & 1], c);
      win_stage(c, 4, (uint32_t)i0, lo, hi, ring, gbits, gidx, cap, lane, run, flushed, above);
    }
  } else {
    for (int j = 0; j < WIN_GROUPS; ++j) {
      if (beg + j * 256 >= a.n) break;  // uniform over the wave
      const int64_t i0 = beg + j * 256 + lane * 4;
      float c[4];
      const int cnt = P::template load4<true>(nd, a.p, i0, a.n, vec, c);
      win_stage(c, cnt, (uint32_t)i0, lo, hi, ring, gbits, gidx, cap, lane, run, flushed, above);
    }
  }
  if (run <= cap && run > flushed) {  // what the ring still holds: fewer than WIN_FLUSH entries
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t j = flushed + lane; j < run; j += 64) {
      gbits[j] = ring[2 * (j & (WIN_RING - 1))];
      gidx[j] = ring[2 * (j & (WIN_RING - 1)) + 1];
    }
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) above += __shfl_xor(above, d, 64);
  if (lane == 0 && seg < a.L.nseg) {
    reinterpret_cast<uint32_t*>(ws + a.L.cnt)[seg] = run;
    reinterpret_cast<uint32_t*>(ws + a.L.above)[seg] = above;
  }
}

// The digit of the krem-th largest key among the candidates whose bits above the digit match pfx:
// an LDS histogram of NB bins over the lists, then the descending scan of select_resolve_kernel.
template <int PASS>
__device__ __forceinline__ void win_digit(const uint32_t* __restrict__ cbits,
                                          const uint32_t* __restrict__ cnt, int64_t nseg,
                                          uint32_t cap, uint32_t* h, uint32_t* wsum,
                                          uint32_t* res, uint32_t& pfx, uint32_t& krem) {
  constexpr int NB = (PASS == 1) ? 2048 : 1024;
  constexpr int SH = (PASS == 0) ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int PER = NB / 1024;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = threadIdx.x; b < NB; b += 1024) h[b] = 0;
  __syncthreads();
  for (int64_t s = wid; s < nseg; s += 16) {
    const uint32_t c = cnt[s];
    const uint32_t* lst = cbits + (size_t)s * cap;
    for (uint32_t j = lane; j < c; j += 64) {
      const uint32_t kk = key_of(__uint_as_float(lst[j]));
      if (PASS == 0) {
        atomicAdd(&h[kk >> 21], 1u);
      } else if (PASS == 1) {
        if ((kk >> 21) == (pfx >> 21)) atomicAdd(&h[(kk >> 10) & 2047u], 1u);
      } else {
        if ((kk >> 10) == (pfx >> 10)) atomicAdd(&h[kk & 1023u], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t hv[PER];
  uint32_t local = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {  // descending bins
    hv[q] = h[NB - 1 - (threadIdx.x * PER + q)];
    local += hv[q];
  }
  uint32_t tot;
  uint32_t before = block_excl_scan(local, wsum, &tot);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (before < krem && krem <= before + hv[q]) {
      res[0] = pfx | ((uint32_t)(NB - 1 - (threadIdx.x * PER + q)) << SH);
      res[1] = krem - before;
    }
    before += hv[q];
  }
  __syncthreads();
  pfx = res[0];
  krem = res[1];
  __syncthreads();
}

template <class P>
__global__ void __launch_bounds__(1024) window_resolve_kernel(const WinArgs<typename P::Args> a) {
  __shared__ uint32_t h[2048];
  __shared__ uint32_t wsum[16];
  __shared__ uint64_t wsum64[16];
  __shared__ uint32_t res[2];
  const typename P::Node nd = a.p.tab[blockIdx.x];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) {  // uniform over the block: a full share leaves the priors alone
      if (threadIdx.x == 0) a.status[blockIdx.x] = 0;
      return;
    }
  }
  char* ws = a.ws + (size_t)blockIdx.x * a.L.node_total;
  WinCtrl* ctrl = reinterpret_cast<WinCtrl*>(ws + a.L.ctrl);
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(ws + a.L.cnt);
  const uint32_t* abv = reinterpret_cast<const uint32_t*>(ws + a.L.above);
  const uint32_t* cbits = reinterpret_cast<const uint32_t*>(ws + a.L.cbits);
  const uint32_t cap = (uint32_t)a.L.cap;
  const uint32_t k = P::k(nd, a.p, a.n);
  const uint32_t lo = ctrl->lo, hi = ctrl->hi;
  if (lo > hi) {  // no usable prior: uniform over the block
    if (threadIdx.x == 0) a.status[blockIdx.x] = 0;
    return;
  }
  uint64_t part = 0;  // candidates in the low 31 bits, key > hi above them: n < 2^31
  int ov = 0;
  for (int64_t s = threadIdx.x; s < a.L.nseg; s += 1024) {
    const uint32_t c = cnt[s];
    part += (uint64_t)c + ((uint64_t)abv[s] << 31);
    ov |= c > cap;
  }
  const bool over = __syncthreads_or(ov);
  uint64_t tot64;
  block_excl_scan64(part, wsum64, &tot64);
  const uint64_t above_lo = tot64 & 0x7FFFFFFFull, above_hi = tot64 >> 31;
  bool hit = !over && above_hi <= (uint64_t)k - 1 && (uint64_t)k - 1 < above_lo;
  uint32_t T = 0, ties = 0;
  if (hit) {  // uniform over the block
    uint32_t pfx = 0, krem = k;
    win_digit<0>(cbits, cnt, a.L.nseg, cap, h, wsum, res, pfx, krem);
    win_digit<1>(cbits, cnt, a.L.nseg, cap, h, wsum, res, pfx, krem);
    win_digit<2>(cbits, cnt, a.L.nseg, cap, h, wsum, res, pfx, krem);
    T = pfx;
    ties = krem;
    hit = T >= lo && T <= hi;
  }
  if (!hit) {
    if (threadIdx.x == 0) a.status[blockIdx.x] = 2;
    return;
  }
  // key > T and key == T of every list, a wave per list
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* soff = reinterpret_cast<uint32_t*>(ws + a.L.off);
  uint32_t* seqb = reinterpret_cast<uint32_t*>(ws + a.L.eqb);
  for (int64_t s = wid; s < a.L.nseg; s += 16) {
    const uint32_t c = cnt[s];
    const uint32_t* lst = cbits + (size_t)s * cap;
    uint32_t v = 0;
    for (uint32_t j = lane; j < c; j += 64) {
      const uint32_t kk = key_of(__uint_as_float(lst[j]));
      v += (kk > T ? 1u : 0u) + (kk == T ? 0x10000u : 0u);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    if (lane == 0) {
      soff[s] = v & 0xFFFFu;
      seqb[s] = v >> 16;
    }
  }
  __syncthreads();
  // every list's output offset and the ties before it: select_scan_kernel's rule
  uint64_t carry_eq = 0, carry_off = 0;
  for (int64_t base = 0; base < a.L.nseg; base += 1024) {
    const int64_t b = base + threadIdx.x;
    const uint64_t gt = b < a.L.nseg ? soff[b] : 0;
    const uint64_t eq = b < a.L.nseg ? seqb[b] : 0;
    uint64_t te;
    const uint64_t eqb = block_excl_scan64(eq, wsum64, &te) + carry_eq;
    uint64_t take = 0;
    if (ties > eqb) take = (ties - eqb) < eq ? (ties - eqb) : eq;
    uint64_t ts;
    const uint64_t off = block_excl_scan64(gt + take, wsum64, &ts) + carry_off;
    if (b < a.L.nseg) {
      soff[b] = (uint32_t)off;
      seqb[b] = (uint32_t)(eqb < ties ? eqb : ties);
    }
    carry_eq += te;
    carry_off += ts;
  }
  if (threadIdx.x == 0) {
    if constexpr (P::kHeader) P::header(nd, a.p, carry_off);
    ctrl->T = T;
    ctrl->ties = ties;
    ctrl->prior_T[P::kslot(nd, a.p) & (WIN_SLOTS - 1)] = T;  // prior_k is k already
    a.status[blockIdx.x] = 1;
  }
}

template <class P>
__global__ void __launch_bounds__(256) window_write_kernel(const WinArgs<typename P::Args> a) {
  if (a.status[blockIdx.y] != 1) return;  // uniform over the block
  const typename P::Node nd = a.p.tab[blockIdx.y];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t seg = (int64_t)blockIdx.x * 4 + wid;
  char* ws = a.ws + (size_t)blockIdx.y * a.L.node_total;
  const WinCtrl* ctrl = reinterpret_cast<const WinCtrl*>(ws + a.L.ctrl);
  const uint32_t T = ctrl->T, ties = ctrl->ties;
  const uint32_t cap = (uint32_t)a.L.cap;
  const uint32_t c = reinterpret_cast<const uint32_t*>(ws + a.L.cnt)[seg];  // <= cap: a hit
  const uint32_t off0 = reinterpret_cast<const uint32_t*>(ws + a.L.off)[seg];
  const uint32_t eqb = reinterpret_cast<const uint32_t*>(ws + a.L.eqb)[seg];
  const uint32_t quota = ties > eqb ? ties - eqb : 0u;
  const uint32_t slots = P::slots(nd, a.p, a.n);
  const uint32_t* lbits = reinterpret_cast<const uint32_t*>(ws + a.L.cbits) + (size_t)seg * cap;
  const uint32_t* lidx = reinterpret_cast<const uint32_t*>(ws + a.L.cidx) + (size_t)seg * cap;
  uint32_t g_run = 0, q_run = 0;
  for (uint32_t base = 0; base < c; base += 64) {  // uniform over the wave
    const uint32_t j = base + lane;
    const bool in = j < c;
    const uint32_t bits = in ? lbits[j] : 0u;
    const uint32_t idx = in ? lidx[j] : 0u;
    const uint32_t kk = key_of(__uint_as_float(bits));
    const bool gt = in && kk > T, eq = in && kk == T;
    const uint64_t bg = __ballot(gt), be = __ballot(eq);
    const uint32_t g = g_run + win_mbcnt(bg), q = q_run + win_mbcnt(be);
    bool sel = false;
    uint32_t pos = 0;
    if (gt) {
      sel = true;
      pos = off0 + g + (q < quota ? q : quota);
    } else if (eq && q < quota) {
      sel = true;
      pos = off0 + g + q;
    }
    if (sel && pos < slots && (int64_t)idx < a.n)
      P::store(nd, a.p, pos, (int64_t)idx, __uint_as_float(bits));
    g_run += (uint32_t)__popcll(bg);
    q_run += (uint32_t)__popcll(be);
  }
}

// The policy of the exact core behind the window launches: what the first pass forms and an idle
// node shares has been stored by the filter.
template <class P>
struct Stored : P {
  static __device__ __forceinline__ void idle_share(const typename P::Node, int64_t) {}
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const typename P::Node nd, const typename P::Args a) {
    return P::template vec<false>(nd, a);
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const typename P::Node nd, const typename P::Args a,
                                              int64_t i0, int64_t n, bool v, float c[4]) {
    return P::template load4<false>(nd, a, i0, n, v, c);
  }
};

// The windowed selection of m nodes on the stream: ws holds win_ws(m, n, kcap).total bytes, zero
// before its first call and the caller's between calls; kcap sizes the lists (the largest k).
template <class P>
int select_window_nodes(int m, const typename P::Args& args, int64_t n, int64_t kcap, void* ws,
                        hipStream_t st) {
  WinArgs<typename P::Args> a;
  a.p = args;
  a.L = win_ws(m, n, kcap);
  a.status = static_cast<uint32_t*>(ws);
  char* exact = static_cast<char*>(ws) + a.L.status_bytes;
  a.ws = exact + a.L.exact_bytes;
  a.n = n;
  const dim3 grid((unsigned)(a.L.nseg / 4), (unsigned)m);
  DPZ_TIMED(DPZ_KT_TOPK_FILTER, st, window_filter_kernel<P><<<grid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_TOPK_RESOLVE, st, window_resolve_kernel<P><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_TOPK_COMPACT, st, window_write_kernel<P><<<grid, 256, 0, st>>>(a));
  SelectWin w;
  w.status = a.status;
  w.ctrl = a.ws + a.L.ctrl;
  w.stride = a.L.node_total;
  return select_nodes<Stored<P>, Stored<P>, true>(m, args, n, exact, st, w);
}

}  // namespace dpz
