// The walk fold: one wave per contiguous element range, payload cursors, no barriers.  Four
// kernels: fold_walk_kernel (1..4 payloads), fold_walk_groups_kernel (5..16 payloads, four at a
// time), fold_walk_batch_kernel (several nodes' 1..4-payload folds in one launch) and
// fold_walk_any_kernel (several nodes' folds of any payload count, sparse and dense payloads
// mixed, in one launch; a node's payloads past the 16th in further launches).  fold_batch_plan
// decides which of the two batch kernels, if any, a dpz_decode_average_batch call takes.
// The tile folds need the tile-offsets pre-pass (fold_offsets_kernel reads every
// payload index once more: 35-100 us of 25 M x 16 payloads at JWINS alphas) and block barriers
// per tile or per payload.  Here each wave owns a contiguous run of tiles of TE = 64 * EPL
// elements and walks every payload's sorted entries with a cursor:
//  * start: a 64-ary search (64 probes per step, one wave-wide load) finds each payload's first
//    entry of the wave's range: <= 6 dependent steps for any k, all payloads' probes in flight;
//  * per tile: a 64-entry window per payload (idx, val; one coalesced load each) is already in
//    registers; the entries inside the tile are its leading lanes (sorted), their count advances
//    the cursor, and the NEXT tile's windows, local values and dense payload values are issued
//    before this tile is folded;
//  * payload by payload, in the reference's order, the window's lanes write their values with a
//    (tile, payload) tag into the wave's own LDS row, and every lane folds its EPL elements
//      t = (tag == mine) ? value : local;  total = t_0*w_0 (+0 first with a zero base);
//      total += t_p*w_p;  total += w_self * local
//    (no block barrier: the row is the wave's own, LDS ops of one wave run in order).
// A window whose 64 entries all fall inside the tile (dense tiles) is followed by synchronous
// extra windows (correct, slower); EPL is chosen so a tile holds ~52 entries or fewer per
// payload on average (fold_plan, dpz_fold.hip).  Invalid payloads (unsorted / out of range)
// cannot write out of bounds.
#include <type_traits>
#include <vector>

#include "dpz_fold_cursor.h"

namespace dpz {

constexpr int FW_WAVES = 4;  // waves per block (256 threads)
// fold_walk_kernel's register bound (blocks per CU = waves per SIMD): the walk hides its window
// loads by occupancy (measured on MI355X, 3 payloads x alpha 0.4 at 128-element tiles: 125 -> 111
// us at 8 waves / SIMD).  The 4-group kernel is left unbounded: bounding it to 5 waves at
// 512-element tiles measured slower (16 x 0.1: 233 vs 222 us, profiles/r03_s2_fold_occ_ab.json).
#define FW_MINB_1(EPL) ((EPL) >= 16 ? 4 : ((EPL) >= 8 ? 5 : ((EPL) >= 4 ? 7 : 8)))

template <int EPL>
struct FwV {
  float v[EPL];
};

// A lane's EPL elements of a tile: contiguous for EPL <= 4; for EPL = 4C > 4, chunk c holds the
// lane's 4 elements at 256 c + 4 lane (every float4 wave-instruction reads 1 KB contiguous).
template <int EPL>
__device__ __forceinline__ int fw_elem(int lane, int e) {
  return EPL <= 4 ? lane * EPL + e : 256 * (e >> 2) + 4 * lane + (e & 3);
}

// Loads are branch-free (addresses clamped into [0, n); results past n are never stored), so
// the compiler counts them and waits only for the tile it folds, never for the next tile's loads
// in flight (a load under a branch makes it wait for everything: vmcnt(0)).  VEC kernels run
// when the operands are 16-byte aligned and n >= 1024: a vector group reaching past n is clamped
// to the last whole aligned group, and the ragged last tile reloads its values element-wise
// (sym2 level-4 coefficient arrays, M = 25,000,009 at C3, are not a multiple of 4).
template <bool VEC, int EPL>
__device__ __forceinline__ FwV<EPL> fw_load(const float* p, int64_t tlo, int lane, int64_t n) {
  FwV<EPL> r;
  if constexpr (VEC && EPL >= 4) {
    const int64_t last = (n & ~int64_t(3)) - 4;  // the last whole float4 group inside [0, n)
#pragma unroll
    for (int c = 0; c < EPL / 4; ++c) {
      const int64_t i0 = tlo + fw_elem<EPL>(lane, 4 * c);
      const int64_t q = i0 + 4 <= n ? i0 : last;
      const float4 v = *reinterpret_cast<const float4*>(p + q);
      r.v[4 * c] = v.x; r.v[4 * c + 1] = v.y; r.v[4 * c + 2] = v.z; r.v[4 * c + 3] = v.w;
    }
    return r;
  } else if constexpr (VEC && EPL == 2) {
    const int64_t i0 = tlo + 2 * lane;
    const int64_t q = i0 + 2 <= n ? i0 : (n & ~int64_t(1)) - 2;
    const float2 v = *reinterpret_cast<const float2*>(p + q);
    r.v[0] = v.x; r.v[1] = v.y;
    return r;
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int64_t i = tlo + fw_elem<EPL>(lane, e);
    r.v[e] = p[i < n ? i : n - 1];
  }
  return r;
}

// GUARD: the ragged last tile (elements past n are not stored).  NTS: non-temporal stores — the
// few-payload walk's output is a model that no later kernel of the step re-reads (same-box A/B on
// MI355X: C2 product path 72.0 -> 65.1 us, 64 MiB 91.0 -> 80.6 us, C4 round 5.72 -> 5.49 ms);
// the 16-payload JWINS fold keeps plain stores (its output feeds the IDWT right after)
template <bool VEC, int EPL, bool GUARD, bool NTS = false>
__device__ __forceinline__ void fw_store(float* p, int64_t tlo, int lane, int64_t n,
                                         const float (&r)[EPL]) {
  if constexpr (VEC && EPL >= 4) {
#pragma unroll
    for (int c = 0; c < EPL / 4; ++c) {
      const int64_t i0 = tlo + fw_elem<EPL>(lane, 4 * c);
      if (!GUARD || i0 + 4 <= n) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f v = {r[4 * c], r[4 * c + 1], r[4 * c + 2], r[4 * c + 3]};
        if (NTS) __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(p + i0));
        else *reinterpret_cast<v4f*>(p + i0) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < n) p[i0 + e] = r[4 * c + e];
      }
    }
    return;
  } else if constexpr (VEC && EPL == 2) {
    const int64_t i0 = tlo + 2 * lane;
    if (!GUARD || i0 + 2 <= n) {
      *reinterpret_cast<float2*>(p + i0) = make_float2(r[0], r[1]);
    } else if (i0 < n) {
      p[i0] = r[0];
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int64_t i = tlo + fw_elem<EPL>(lane, e);
    if (!GUARD || i < n) p[i] = r[e];
  }
}

// Sparse payloads only (dense ones take the classic kernels), a fresh total (a.first),
// n < 2^31 - 1024 (fold_plan), np <= NS.  NS payload slots, all compile-time: every slot's window
// of the NEXT tile is issued at the start of this tile (branch-free loads), so the loads are in
// flight while all of this tile's payloads fold.  The payloads' pointers, sizes, weights and
// cursors stay in scalar registers (NS is 4 everywhere: holding them one per lane for more slots
// measured slower than fold_walk_groups_kernel at 16 payloads, which is used there).
// One wave's run of tiles [t0, t1) of one fold (fold_walk_kernel; fold_walk_batch_kernel runs
// several folds' runs back to back).  wv / wt: the wave's LDS row; seq: the wave's tile sequence
// number, carried across runs so a stale tag of an earlier run never matches.
template <bool VEC, int EPL, int NS, class FA>
__device__ __forceinline__ void fold_walk_run(const FA& a, int64_t t0, int64_t t1, float* wv,
                                              uint32_t* wt, int lane, uint32_t& seq) {
  static_assert(NS <= 4, "every slot's parameters and cursor in scalar registers");
  constexpr int TE = 64 * EPL;
  const int64_t n = a.n;
  const int np = a.np;
  auto P_idx = [&](int p) { return a.p[p].idx; };
  auto P_val = [&](int p) { return a.p[p].val; };
  auto P_k = [&](int p) { return (int32_t)a.p[p].k; };
  auto P_w = [&](int p) { return a.p[p].w; };
  FwV<EPL> L, Ln;
  // ---- start cursors: lower_bound(idx_p, t0 * TE) ----
  // lane p: payload p's cursor (the next window's first entry)
  const int32_t curv = fw_start_cursors<NS>(
      np, (int32_t)(t0 * TE), lane, [&](int p) { return P_idx(p); },
      [&](int p) { return P_k(p); }, reinterpret_cast<const int32_t*>(a.local));
  L = fw_load<VEC, EPL>(a.local, t0 * TE, lane, n);
  int32_t cs[NS];
#pragma unroll
  for (int p = 0; p < NS; ++p) cs[p] = fw_uni(__builtin_amdgcn_readlane(curv, p));
  auto cur_of = [&](int p) { return cs[p]; };
  auto set_cur = [&](int p, int32_t v) { cs[p] = fw_uni(v); };
  // ---- one 64-entry window per slot: (idx, val) at cur + lane, branch-free loads of raw values
  // (lanes past k read entry 0 and are masked when the window is used) ----
  int32_t wi[NS], wn[NS];
  float wvv[NS], wvn[NS];
  auto load_window = [&](int p, int32_t& ix, float& vx, int32_t at) {
    const bool live = p < np;
    const int pc = live ? p : 0;
    const int32_t j = (live ? at : 0) + lane;
    const int32_t kp = P_k(pc);
    const int32_t k = live ? kp : 0;
    const int32_t jc = j < k ? j : 0;
    // an empty payload's arrays may be null: read a valid address instead (masked at use)
    const bool has = kp > 0;
    ix = (has ? P_idx(pc) : reinterpret_cast<const int32_t*>(a.local))[jc];
    vx = (has ? P_val(pc) : a.local)[jc];
  };
#pragma unroll
  for (int p = 0; p < NS; ++p) load_window(p, wi[p], wvv[p], cur_of(p));
  auto tile_body = [&](int64_t tile, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    const int64_t tlo = tile * TE;
    const int32_t tlo32 = (int32_t)tlo, thi32 = tlo32 + TE;
    // the run's last tile issues no windows past it: they re-request this tile's entries (L2)
    const bool more = tile + 1 < t1;
    // the ragged last tile: its vector groups past the last whole one were clamped on load
    if constexpr (GUARD && VEC) L = fw_load<false, EPL>(a.local, tlo, lane, n);
    // every slot: this tile's window start and entry count (the leading lanes below thi); the
    // cursors move to the next tile's windows, which are issued now with the next local values
    int32_t c0[NS], cnt[NS];
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      const bool live = p < np;
      c0[p] = live ? cur_of(p) : 0;
      const int32_t k = live ? P_k(p) : 0;
      cnt[p] = fw_lead(c0[p] + lane < k && wi[p] < thi32);
      if (live) set_cur(p, c0[p] + cnt[p]);
    }
#pragma unroll
    for (int p = 0; p < NS; ++p) load_window(p, wn[p], wvn[p], more ? cur_of(p) : c0[p]);
    // the next tile's local values; the run's last tile re-requests its own lines instead (L2
    // hits) — a load of the tile past the run fetched 1 / tpw more model bytes from HBM
    // (64 MiB, 3 payloads: 4 tiles per wave, PMC 97 MB fetched against 71 MB)
    Ln = fw_load<VEC, EPL>(a.local, tile + 1 < t1 ? tlo + TE : tlo, lane, n);
    float acc[EPL], base[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      base[e] = a.zero_base ? 0.0f : L.v[e];
      acc[e] = 0.0f;
    }
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      if (p >= np) break;
      const float w = P_w(p);
      const uint32_t tag = (seq << 4) | (uint32_t)p;
      {
        const uint32_t pos = (uint32_t)(wi[p] - tlo32);  // < TE: inside the tile
        if (lane < cnt[p] && pos < (uint32_t)TE) {
          wv[pos] = wvv[p];
          wt[pos] = tag;
        }
      }
      if (cnt[p] == 64) {  // a dense tile: this payload's further windows, synchronously
        const int32_t k = P_k(p);
        const int32_t* pi = P_idx(p);
        const float* pv = P_val(p);
        int32_t c = 64;
        for (int32_t j0 = c0[p] + 64;; j0 += 64) {
          const int32_t j = j0 + lane;
          const int32_t iv = j < k ? pi[j] : INT32_MAX;
          const int cc = fw_lead(iv < thi32);
          const uint32_t pos = (uint32_t)(iv - tlo32);
          if (lane < cc && pos < (uint32_t)TE) {
            wv[pos] = pv[j];
            wt[pos] = tag;
          }
          c += cc;
          if (cc < 64) break;
        }
        set_cur(p, c0[p] + c);
        load_window(p, wn[p], wvn[p], more ? cur_of(p) : c0[p]);  // this payload's next window moved
      }
      // the row is this wave's own and one wave's LDS instructions execute in order, so the
      // lanes' writes above are seen by the reads below with no wait; the scheduling barriers
      // only keep the compiler from moving LDS accesses across (no memory fence: a fence would
      // also wait for the next tile's loads in flight)
      __builtin_amdgcn_wave_barrier();
      uint32_t tg[EPL];
      float hv[EPL];
      if constexpr (EPL >= 4) {
#pragma unroll
        for (int c = 0; c < EPL / 4; ++c) {
          const int o = fw_elem<EPL>(lane, 4 * c);
          const uint4 t4 = *reinterpret_cast<const uint4*>(&wt[o]);
          const float4 h4 = *reinterpret_cast<const float4*>(&wv[o]);
          tg[4 * c] = t4.x; tg[4 * c + 1] = t4.y; tg[4 * c + 2] = t4.z; tg[4 * c + 3] = t4.w;
          hv[4 * c] = h4.x; hv[4 * c + 1] = h4.y; hv[4 * c + 2] = h4.z; hv[4 * c + 3] = h4.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          tg[e] = wt[lane * EPL + e];
          hv[e] = wv[lane * EPL + e];
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float tv = tg[e] == tag ? hv[e] : base[e];
        const float term = tv * w;
        acc[e] = p == 0 ? (a.zero_base ? 0.0f + term : term) : acc[e] + term;
      }
    }
    if (a.add_self) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = acc[e] + L.v[e] * a.w_self;
    }
    fw_store<VEC, EPL, GUARD, true>(a.out, tlo, lane, n, acc);
    if (a.out2) fw_store<VEC, EPL, GUARD, true>(a.out2, tlo, lane, n, acc);
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      wi[p] = wn[p];
      wvv[p] = wvn[p];
    }
    L = Ln;
    ++seq;
  };
  const int64_t tfull = n / TE;  // tiles wholly inside [0, n)
  const int64_t tf = t1 < tfull ? t1 : (tfull > t0 ? tfull : t0);
  for (int64_t tile = t0; tile < tf; ++tile) tile_body(tile, std::false_type{});
  if (tf < t1) tile_body(tf, std::true_type{});  // the global last tile, ragged
}

template <bool VEC, int EPL, int NS>
__global__ void __launch_bounds__(256, FW_MINB_1(EPL)) fold_walk_kernel(FoldArgs a, int64_t tpw) {
  constexpr int TE = 64 * EPL;
  __shared__ float s_val[FW_WAVES][TE];
  __shared__ uint32_t s_tag[FW_WAVES][TE];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wv = s_val[wid];
  uint32_t* wt = s_tag[wid];
#pragma unroll
  for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = 0xFFFFFFFFu;
  const int64_t ntl = (a.n + TE - 1) / TE;
  const int64_t gw = (int64_t)blockIdx.x * FW_WAVES + wid;
  const int64_t t0 = gw * tpw;
  const int64_t t1 = (t0 + tpw < ntl) ? t0 + tpw : ntl;
  if (t0 >= t1) return;  // no block barrier anywhere: a wave may leave alone
  uint32_t seq = 0;
  fold_walk_run<VEC, EPL, NS>(a, t0, t1, wv, wt, lane, seq);
}

// A node's plain Metro-Hastings walk fold of <= 4 sparse payloads (fold_walk_batch_kernel's
// kernel-argument table entry) and the view fold_walk_run reads it through.
struct FoldNode {
  const float* local;
  float* out;
  float* out2;
  int np;
  float w_self;
  FoldPayload p[4];
};
constexpr int FW_BATCH = 22;  // nodes per launch: the table stays within the 4 KB of arguments
struct FoldNodeBatch {
  FoldNode nd[FW_BATCH];
  int64_t n;
  int m;
  int add_self;
  // dpz_decode_average_batch_guarded: int32 words (the round's encode status words) that must
  // all be 0, or the launch writes nothing (nullptr: no guard)
  const int32_t* guard;
  int64_t guard_n;
};
static_assert(sizeof(FoldNodeBatch) <= 3584, "kernel arguments");
struct FoldNodeView {
  const float* local;
  float* out;
  float* out2;
  int64_t n;
  int np;
  int add_self;
  int zero_base;
  float w_self;
  const FoldPayload* p;
};

// ONE launch for the folds of up to FW_BATCH nodes of a gossip round (dpz_decode_average_batch:
// every node's fold a plain Metro-Hastings walk of <= 4 sparse payloads over the same n): the
// folds' tiles form one range [0, m * ntl) that the persistent grid's waves split into contiguous
// runs, a run crossing a node boundary continuing in the next node's fold.  One launch instead of
// m: the folds' start-up latencies (cursor searches, first windows) overlap and no launch drains
// alone (a full-GPU persistent grid per node serialises on a few streams).
template <bool VEC, int EPL>
__global__ void __launch_bounds__(256, FW_MINB_1(EPL)) fold_walk_batch_kernel(FoldNodeBatch b,
                                                                              int64_t tpw) {
  constexpr int TE = 64 * EPL;
  const int64_t ntl = (b.n + TE - 1) / TE;
  const int64_t m = b.m;
  __shared__ float s_val[FW_WAVES][TE];
  __shared__ uint32_t s_tag[FW_WAVES][TE];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wv = s_val[wid];
  uint32_t* wt = s_tag[wid];
#pragma unroll
  for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = 0xFFFFFFFFu;
  const int64_t gw = (int64_t)blockIdx.x * FW_WAVES + fw_uni(wid);
  if (b.guard) {  // a missed encode: no fold of this launch writes (the host re-runs the round)
    bool bad = false;
    for (int64_t i = lane; i < b.guard_n; i += 64) bad |= b.guard[i] != 0;
    if (__ballot(bad) != 0) return;  // every wave reads the same final words
  }
  int64_t g = gw * tpw;
  const int64_t gend = m * ntl;
  const int64_t g1 = g + tpw < gend ? g + tpw : gend;
  uint32_t seq = 0;
  while (g < g1) {
    const int64_t node = g / ntl;
    const int64_t lt0 = g - node * ntl;
    const int64_t lt1 = lt0 + (g1 - g) < ntl ? lt0 + (g1 - g) : ntl;
    const FoldNode& nd = b.nd[node];
    const FoldNodeView v{nd.local, nd.out, nd.out2, b.n, nd.np, b.add_self, 0, nd.w_self, nd.p};
    fold_walk_run<VEC, EPL, 4>(v, lt0, lt1, wv, wt, lane, seq);
    g += lt1 - lt0;
  }
}

constexpr int FW_G = 4;  // payloads per group: the windows of one group are in registers

// 5..16 sparse payloads (fold_walk_kernel's conditions otherwise).  The payloads are walked in
// groups of FW_G: the windows of the group being folded and of the next group (of this tile, or group 0 of the next tile) are in
// registers, so every window load is in flight while the group before it folds, with 16
// registers of windows whatever the payload count.  Cursors live one per lane (lane p: payload
// p) in one register.
template <bool VEC, int EPL, int DIST, bool W2>
__global__ void __launch_bounds__(256) fold_walk_groups_kernel(FoldArgs a, int64_t tpw) {
  constexpr int TE = 64 * EPL;
  __shared__ float s_val[FW_WAVES][TE];
  // tags: tile sequence << 4 | payload
  constexpr uint32_t SEQ_WRAP = 0x0FFFFFFFu;
  __shared__ uint32_t s_tag[FW_WAVES][TE];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wv = s_val[wid];
  uint32_t* wt = s_tag[wid];
#pragma unroll
  for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = ~0u;
  const int64_t n = a.n;
  const int64_t ntl = (n + TE - 1) / TE;
  const int64_t gw = (int64_t)blockIdx.x * FW_WAVES + wid;
  const int64_t t0 = gw * tpw;
  const int64_t t1 = (t0 + tpw < ntl) ? t0 + tpw : ntl;
  if (t0 >= t1) return;  // no block barrier anywhere: a wave may leave alone
  const int np = a.np;
  // DIST 1: the group loop is dynamic and the cursors live one per lane (lane p: payload p) in
  // one register
  const int ng = (np + FW_G - 1) / FW_G;
  // CT: every payload number in the loop is a compile-time constant (DIST 3, whose four groups
  // are unrolled): the cursors in scalar registers (no readlane / writelane round trips)
  constexpr bool CT = DIST == 3;
  const int lp = lane < np && lane < FOLD_MAXP ? lane : 0;
  const int32_t kl = lane < np ? (int32_t)a.p[lp].k : 0;
  // payload p's pointers and weight held by lane p, read back with readlane (no scalar loads of
  // the kernel arguments with a run-time payload number inside the loop)
  const uint64_t ipl = reinterpret_cast<uint64_t>(a.p[lp].idx);
  const uint64_t vpl = reinterpret_cast<uint64_t>(a.p[lp].val);
  const float wl = a.p[lp].w;
  auto rl64 = [](uint64_t v, int p) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, p);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), p);
    return ((uint64_t)hi << 32) | lo;
  };
  auto P_idx = [&](int p) { return reinterpret_cast<const int32_t*>(rl64(ipl, p)); };
  auto P_val = [&](int p) { return reinterpret_cast<const float*>(rl64(vpl, p)); };
  auto P_k = [&](int p) { return fw_uni(__builtin_amdgcn_readlane(kl, p)); };
  auto P_w = [&](int p) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), p));
  };
  static_assert(DIST == 1 || DIST == 3, "DIST 3: four groups");
  int32_t cs[FOLD_MAXP];  // CT: the cursors (scalar registers)
  FwV<EPL> L, Ln;
  // ---- start cursors: lower_bound(idx_p, t0 * TE) ----
  int32_t curv = fw_start_cursors<FOLD_MAXP>(
      np, (int32_t)(t0 * TE), lane, [&](int p) { return P_idx(p); },
      [&](int p) { return P_k(p); }, reinterpret_cast<const int32_t*>(a.local));
  L = fw_load<VEC, EPL>(a.local, t0 * TE, lane, n);
  if (CT) {
#pragma unroll
    for (int q = 0; q < FOLD_MAXP; ++q) cs[q] = fw_uni(__builtin_amdgcn_readlane(curv, q));
  }
  auto cur_of = [&](int p) { return CT ? cs[p] : fw_uni(__builtin_amdgcn_readlane(curv, p)); };
  auto set_cur = [&](int p, int32_t v) {
    if (CT) cs[p] = fw_uni(v);
    else curv = lane == p ? v : curv;
  };
  // ---- the windows of one group: (idx, val) at cur + lane, branch-free loads of raw values
  // (lanes past k read entry 0 and are masked when the window is used) ----
  // W2: 128-entry windows (entries cur + lane and cur + 64 + lane), so a tile of ~50 entries per
  // payload on average rarely overflows into the synchronous path (whose loads, the youngest in
  // flight, make the wave wait for every window load issued ahead: vmcnt(0))
  constexpr int NSL = DIST == 3 ? FW_G : 2;
  constexpr int NW2 = W2 ? NSL : 1;
  int32_t WI[NSL][FW_G], WI2[NW2][FW_G];
  float WV[NSL][FW_G], WV2[NW2][FW_G];
  auto load_group = [&](int g, int sl) {
#pragma unroll
    for (int q = 0; q < FW_G; ++q) {
      const int p = g * FW_G + q;
      const bool live = p < np;
      const int pc = live ? p : 0;
      const int32_t j = (live ? cur_of(pc) : 0) + lane;
      const int32_t kp = P_k(pc);
      const int32_t k = live ? kp : 0;
      const int32_t jc = j < k ? j : 0;
      // an empty payload's arrays may be null: read a valid address instead (masked at use)
      const bool has = kp > 0;
      const auto* ip = as_global(has ? P_idx(pc) : reinterpret_cast<const int32_t*>(a.local));
      const auto* vp = as_global(has ? P_val(pc) : a.local);
      WI[sl][q] = ip[jc];
      WV[sl][q] = vp[jc];
      if constexpr (W2) {
        const int32_t jc2 = j + 64 < k ? j + 64 : 0;
        WI2[sl][q] = ip[jc2];
        WV2[sl][q] = vp[jc2];
      }
    }
  };
  // DIST 1: the windows of the group being folded and of the next one (wi, wn);
  // DIST 3 (four groups, 13..16 payloads): all four groups' windows in registers, each group's
  // issued three groups ahead (into the slot the group before it just freed), so three groups'
  // loads are in flight while one folds
  if constexpr (DIST == 3) {
    load_group(0, 0);
    load_group(1, 1);
    load_group(2, 2);
  } else {
    load_group(0, 0);
  }
  uint32_t seq = 0;
  auto tile_body = [&](int64_t tile, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    const int64_t tlo = tile * TE;
    const int32_t tlo32 = (int32_t)tlo, thi32 = tlo32 + TE;
    // the ragged last tile: its vector groups past the last whole one were clamped on load
    if constexpr (GUARD && VEC) L = fw_load<false, EPL>(a.local, tlo, lane, n);
    // the next tile's local values; the run's last tile re-requests its own lines instead (L2
    // hits) — a load of the tile past the run fetched 1 / tpw more model bytes from HBM
    // (64 MiB, 3 payloads: 4 tiles per wave, PMC 97 MB fetched against 71 MB)
    Ln = fw_load<VEC, EPL>(a.local, tile + 1 < t1 ? tlo + TE : tlo, lane, n);
    float acc[EPL], base[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      base[e] = a.zero_base ? 0.0f : L.v[e];
      acc[e] = 0.0f;
    }
    // one group: its windows (wi, wvv) are in registers; `issue` starts a later group's loads
    // once this group's cursors have advanced
    auto fold_group = [&](int g, int sl, auto issue) {
      const int32_t (&wi)[FW_G] = WI[sl];
      const float (&wvv)[FW_G] = WV[sl];
      // this group's window starts; the entries of the tile are the leading lanes below thi
      int32_t c0[FW_G], cnt[FW_G];
#pragma unroll
      for (int q = 0; q < FW_G; ++q) {
        const int p = g * FW_G + q;
        const bool live = p < np;
        c0[q] = live ? cur_of(p) : 0;
        const int32_t k = live ? P_k(p) : 0;
        cnt[q] = fw_lead(c0[q] + lane < k && wi[q] < thi32);
        if (W2 && cnt[q] == 64) cnt[q] += fw_lead(c0[q] + 64 + lane < k && WI2[W2 ? sl : 0][q] < thi32);
        // the next tile's window start of this payload (a full window is finished in its phase)
        if (live) set_cur(p, c0[q] + cnt[q]);
      }
      issue();
#pragma unroll
      for (int q = 0; q < FW_G; ++q) {
        const int p = g * FW_G + q;
        if (p >= np) break;
        const float w = P_w(p);
        const uint32_t tag = (seq << 4) | (uint32_t)p;
        {
          const uint32_t pos = (uint32_t)(wi[q] - tlo32);  // < TE: inside the tile
          if (lane < cnt[q] && pos < (uint32_t)TE) {
            wv[pos] = wvv[q];
            wt[pos] = tag;
          }
          if constexpr (W2) {
            const uint32_t pos2 = (uint32_t)(WI2[sl][q] - tlo32);
            if (lane + 64 < cnt[q] && pos2 < (uint32_t)TE) {
              wv[pos2] = WV2[sl][q];
              wt[pos2] = tag;
            }
          }
        }
        constexpr int WN = W2 ? 128 : 64;
        if (cnt[q] == WN) {  // a dense tile: this payload's further windows, synchronously
          const int32_t k = P_k(p);
          const int32_t* pi = P_idx(p);
          const float* pv = P_val(p);
          int32_t c = WN;
          for (int32_t j0 = c0[q] + WN;; j0 += 64) {
            const int32_t j = j0 + lane;
            const int32_t iv = j < k ? as_global(pi)[j] : INT32_MAX;
            const int cc = fw_lead(iv < thi32);
            const uint32_t pos = (uint32_t)(iv - tlo32);
            if (lane < cc && pos < (uint32_t)TE) {
              wv[pos] = as_global(pv)[j];
              wt[pos] = tag;
            }
            c += cc;
            if (cc < 64) break;
          }
          set_cur(p, c0[q] + c);
          // the next tile's window of this group moved (DIST 1, one group: already issued)
          if (DIST == 1 && ng == 1) load_group(0, 1);
        }
        // the row is this wave's own and one wave's LDS instructions execute in order, so the
        // lanes' writes above are seen by the reads below with no wait; the scheduling barriers
        // only keep the compiler from moving LDS accesses across (no memory fence: a fence
        // would also wait for the next windows in flight)
        __builtin_amdgcn_wave_barrier();
        uint32_t tg[EPL];
        float hv[EPL], tv[EPL];
        if constexpr (EPL >= 4) {
#pragma unroll
          for (int c = 0; c < EPL / 4; ++c) {
            const int o = fw_elem<EPL>(lane, 4 * c);
            const uint4 t4 = *reinterpret_cast<const uint4*>(&wt[o]);
            tg[4 * c] = t4.x; tg[4 * c + 1] = t4.y; tg[4 * c + 2] = t4.z; tg[4 * c + 3] = t4.w;
            const float4 h4 = *reinterpret_cast<const float4*>(&wv[o]);
            hv[4 * c] = h4.x; hv[4 * c + 1] = h4.y; hv[4 * c + 2] = h4.z; hv[4 * c + 3] = h4.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            tg[e] = wt[lane * EPL + e];
            hv[e] = wv[lane * EPL + e];
          }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          tv[e] = tg[e] == tag ? hv[e] : base[e];
          const float term = tv[e] * w;
          acc[e] = p == 0 ? (a.zero_base ? 0.0f + term : term) : acc[e] + term;
        }
      }
    };
    if constexpr (DIST == 3) {
      // group g of this tile issues group g + 3: group 3 of this tile (g = 0), else group g - 1
      // of the next tile, into the slot group g - 1 freed
#pragma unroll
      for (int g = 0; g < FW_G; ++g) {
        fold_group(g, g, [&] {
          const int s3 = (g + 3) & (FW_G - 1);
          load_group(s3, s3);
        });
      }
    } else {
      for (int g = 0; g < ng; ++g) {
        // the next group's windows (this tile's next group, or group 0 of the next tile)
        fold_group(g, 0, [&] { load_group(g + 1 < ng ? g + 1 : 0, 1); });
#pragma unroll
        for (int q = 0; q < FW_G; ++q) {
          WI[0][q] = WI[1][q];
          WV[0][q] = WV[1][q];
          if constexpr (W2) {
            WI2[0][q] = WI2[W2 ? 1 : 0][q];
            WV2[0][q] = WV2[W2 ? 1 : 0][q];
          }
        }
      }
    }
    if (a.add_self) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = acc[e] + L.v[e] * a.w_self;
    }
    fw_store<VEC, EPL, GUARD>(a.out, tlo, lane, n, acc);
    if (a.out2) fw_store<VEC, EPL, GUARD>(a.out2, tlo, lane, n, acc);
    L = Ln;
    if (++seq == SEQ_WRAP) {  // tags restart: no stale tag of this row may match a new one
      seq = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = ~0u;
    }
  };
  const int64_t tfull = n / TE;  // tiles wholly inside [0, n)
  const int64_t tf = t1 < tfull ? t1 : (tfull > t0 ? tfull : t0);
  for (int64_t tile = t0; tile < tf; ++tile) tile_body(tile, std::false_type{});
  if (tf < t1) tile_body(tf, std::true_type{});  // the global last tile, ragged
}

// ---- the any-degree batch: several nodes' folds of 1..16 payloads, sparse or dense, a fresh or
// a continued total, in one launch (fold_walk_any_kernel) ----
// The kernel-argument table of one launch: slots of 24 bytes, the launch's m nodes first, then
// the nodes' payloads packed in node order (a node's payloads start at slot m + p0).  146 slots:
// 22 nodes of <= 4 payloads (110 slots), 8 nodes of 16 (136), 29 nodes of 4.
struct FoldAnyNode {
  const float* local;
  float* out;
  float w_self;
  uint16_t p0;  // the node's first payload in the launch's packed payload list
  uint8_t np;   // payloads of this launch, 1..FOLD_MAXP
  uint8_t fl;   // FA_*
};
struct FoldAnyPayload {
  const int32_t* idx;  // nullptr: dense (val has n entries)
  const float* val;
  int32_t k;
  float w;
};
constexpr int FA_FIRST = 1;  // the launch starts the node's total (else it continues from out)
constexpr int FA_LAST = 2;   // the node's last group: the self term and the copy over local
constexpr int FA_DENSE = 4;  // one of the group's payloads is dense
constexpr int FA_LOCAL = 8;  // DPZ_FOLD_ALSO_LOCAL (written with FA_LAST only)
constexpr int FA_SLOTS = 146;
union FoldAnySlot {
  FoldAnyNode nd;
  FoldAnyPayload p;
};
struct FoldAnyBatch {
  FoldAnySlot s[FA_SLOTS];
  int64_t n;
  const int32_t* guard;  // as FoldNodeBatch::guard
  int64_t guard_n;
  int m;
  int add_self;
};
static_assert(sizeof(FoldAnySlot) == 24 && sizeof(FoldAnyBatch) <= 3584, "kernel arguments");
// a node's payloads read through the table: p[i] is the node's i-th payload
struct FoldAnyPayloads {
  const FoldAnySlot* s;
  __device__ __forceinline__ const FoldAnyPayload& operator[](int i) const { return s[i].p; }
};
// fold_walk_run's view of a node of the table (<= 4 sparse payloads, a fresh total)
struct FoldAnyView {
  const float* local;
  float* out;
  float* out2;
  int64_t n;
  int np;
  int add_self;
  int zero_base;
  float w_self;
  FoldAnyPayloads p;
};

// One wave's run of tiles [t0, t1) of one node's group of 1..16 payloads: the body of
// fold_walk_groups_kernel in its one-group-ahead form with 64-entry windows (four payloads per
// group; the next group's windows, of this tile or group 0 of the next tile, in flight while a
// group folds), with what that kernel does not take:
//  * DENSE: a dense payload's tile values are a straight row load, issued with its group's
//    windows (branch-free: a sparse slot re-reads the first tile of local, cache hits), and its
//    slot of the window machinery is an empty payload (k = 0: no cursor search, no entries);
//  * CONT: the total continues from out (a node's 17th payload on: t_p * w_p added to the stored
//    total, as dpz_decode_average's later groups do).
// pp: the group's payloads in the kernel-argument table.  Plain stores (the >= 5-payload output
// feeds a kernel right after, as fold_walk_groups_kernel's).
template <int EPL, bool DENSE, bool CONT>
__device__ __forceinline__ void fold_any_run(const FoldAnyView& a, int64_t t0, int64_t t1,
                                             float* wv, uint32_t* wt, int lane, uint32_t& seq) {
  constexpr int TE = 64 * EPL;
  constexpr uint32_t SEQ_WRAP = 0x0FFFFFFFu;
  const int64_t n = a.n;
  const int np = a.np;
  const int ng = (np + FW_G - 1) / FW_G;
  const int lp = lane < np && lane < FOLD_MAXP ? lane : 0;
  // payload p's pointers, size and weight held by lane p, read back with readlane
  const uint64_t ipl = reinterpret_cast<uint64_t>(a.p[lp].idx);
  const uint64_t vpl = reinterpret_cast<uint64_t>(a.p[lp].val);
  const float wl = a.p[lp].w;
  // bit p: payload p is dense; its window slot is an empty payload
  const uint32_t dmask = DENSE ? (uint32_t)__ballot(lane < np && ipl == 0) & 0xFFFFu : 0u;
  const int32_t kl = (lane < np && !((dmask >> lp) & 1u)) ? a.p[lp].k : 0;
  auto rl64 = [](uint64_t v, int p) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, p);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), p);
    return ((uint64_t)hi << 32) | lo;
  };
  auto P_idx = [&](int p) { return reinterpret_cast<const int32_t*>(rl64(ipl, p)); };
  auto P_val = [&](int p) { return reinterpret_cast<const float*>(rl64(vpl, p)); };
  auto P_k = [&](int p) { return fw_uni(__builtin_amdgcn_readlane(kl, p)); };
  auto P_w = [&](int p) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), p));
  };
  auto is_dense = [&](int p) { return DENSE && ((dmask >> p) & 1u) != 0; };
  FwV<EPL> L, Ln;
  // ---- start cursors: lower_bound(idx_p, t0 * TE) (a dense payload: k = 0, no search) ----
  int32_t curv = fw_start_cursors<FOLD_MAXP>(
      np, (int32_t)(t0 * TE), lane, [&](int p) { return P_idx(p); },
      [&](int p) { return P_k(p); }, reinterpret_cast<const int32_t*>(a.local));
  L = fw_load<true, EPL>(a.local, t0 * TE, lane, n);
  auto cur_of = [&](int p) { return fw_uni(__builtin_amdgcn_readlane(curv, p)); };
  auto set_cur = [&](int p, int32_t v) { curv = lane == p ? v : curv; };
  // ---- the windows of one group (slot 0: the group being folded, 1: the next one) and, DENSE,
  // the tile values of its dense payloads at tile start dlo ----
  int32_t WI[2][FW_G];
  float WV[2][FW_G];
  FwV<EPL> DV[2][FW_G];  // (DENSE only)
  auto load_group = [&](int g, int sl, int64_t dlo) {
#pragma unroll
    for (int q = 0; q < FW_G; ++q) {
      const int p = g * FW_G + q;
      const bool live = p < np;
      const int pc = live ? p : 0;
      const int32_t j = (live ? cur_of(pc) : 0) + lane;
      const int32_t kp = P_k(pc);
      const int32_t k = live ? kp : 0;
      const int32_t jc = j < k ? j : 0;
      // an empty slot reads a valid address instead (masked at use)
      const bool has = kp > 0;
      const auto* ip = as_global(has ? P_idx(pc) : reinterpret_cast<const int32_t*>(a.local));
      const auto* vp = as_global(has ? P_val(pc) : a.local);
      WI[sl][q] = ip[jc];
      WV[sl][q] = vp[jc];
      if constexpr (DENSE) {
        const bool dn = live && is_dense(pc);
        DV[sl][q] = fw_load<true, EPL>(dn ? P_val(pc) : a.local, dn ? dlo : 0, lane, n);
      }
    }
  };
  load_group(0, 0, t0 * TE);
  auto tile_body = [&](int64_t tile, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    const int64_t tlo = tile * TE;
    const int32_t tlo32 = (int32_t)tlo, thi32 = tlo32 + TE;
    // the next tile (the run's last tile re-requests its own lines: fold_walk_run)
    const int64_t nlo = tile + 1 < t1 ? tlo + TE : tlo;
    // the ragged last tile: its vector groups past the last whole one were clamped on load
    if constexpr (GUARD) L = fw_load<false, EPL>(a.local, tlo, lane, n);
    Ln = fw_load<true, EPL>(a.local, nlo, lane, n);
    float acc[EPL], base[EPL];
    if constexpr (CONT) {
      const FwV<EPL> O = GUARD ? fw_load<false, EPL>(a.out, tlo, lane, n)
                               : fw_load<true, EPL>(a.out, tlo, lane, n);
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = O.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) base[e] = L.v[e];
    for (int g = 0; g < ng; ++g) {
      const int32_t (&wi)[FW_G] = WI[0];
      const float (&wvv)[FW_G] = WV[0];
      // this group's window starts; the entries of the tile are the leading lanes below thi
      int32_t c0[FW_G], cnt[FW_G];
#pragma unroll
      for (int q = 0; q < FW_G; ++q) {
        const int p = g * FW_G + q;
        const bool live = p < np;
        c0[q] = live ? cur_of(p) : 0;
        const int32_t k = live ? P_k(p) : 0;
        cnt[q] = fw_lead(c0[q] + lane < k && wi[q] < thi32);
        if (live) set_cur(p, c0[q] + cnt[q]);
      }
      // the next group's windows: this tile's next group, or group 0 of the next tile
      const bool wrap = g + 1 >= ng;
      load_group(wrap ? 0 : g + 1, 1, wrap ? nlo : tlo);
#pragma unroll
      for (int q = 0; q < FW_G; ++q) {
        const int p = g * FW_G + q;
        if (p >= np) break;
        const float w = P_w(p);
        const bool dn = is_dense(p);
        const uint32_t tag = (seq << 4) | (uint32_t)p;
        {
          const uint32_t pos = (uint32_t)(wi[q] - tlo32);  // < TE: inside the tile
          if (lane < cnt[q] && pos < (uint32_t)TE) {
            wv[pos] = wvv[q];
            wt[pos] = tag;
          }
        }
        if (cnt[q] == 64) {  // a dense tile: this payload's further windows, synchronously
          const int32_t k = P_k(p);
          const int32_t* pi = P_idx(p);
          const float* pv = P_val(p);
          int32_t c = 64;
          for (int32_t j0 = c0[q] + 64;; j0 += 64) {
            const int32_t j = j0 + lane;
            const int32_t iv = j < k ? as_global(pi)[j] : INT32_MAX;
            const int cc = fw_lead(iv < thi32);
            const uint32_t pos = (uint32_t)(iv - tlo32);
            if (lane < cc && pos < (uint32_t)TE) {
              wv[pos] = as_global(pv)[j];
              wt[pos] = tag;
            }
            c += cc;
            if (cc < 64) break;
          }
          set_cur(p, c0[q] + c);
          // one group: the next tile's windows of this group are already issued, and moved
          if (ng == 1) load_group(0, 1, nlo);
        }
        if constexpr (DENSE && GUARD) {  // the ragged tile's clamped vector groups
          if (dn) DV[0][q] = fw_load<false, EPL>(P_val(p), tlo, lane, n);
        }
        // (the wave's own LDS row, in order: fold_walk_run)
        __builtin_amdgcn_wave_barrier();
        uint32_t tg[EPL];
        float hv[EPL];
        if constexpr (EPL >= 4) {
#pragma unroll
          for (int c = 0; c < EPL / 4; ++c) {
            const int o = fw_elem<EPL>(lane, 4 * c);
            const uint4 t4 = *reinterpret_cast<const uint4*>(&wt[o]);
            tg[4 * c] = t4.x; tg[4 * c + 1] = t4.y; tg[4 * c + 2] = t4.z; tg[4 * c + 3] = t4.w;
            const float4 h4 = *reinterpret_cast<const float4*>(&wv[o]);
            hv[4 * c] = h4.x; hv[4 * c + 1] = h4.y; hv[4 * c + 2] = h4.z; hv[4 * c + 3] = h4.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            tg[e] = wt[lane * EPL + e];
            hv[e] = wv[lane * EPL + e];
          }
        }
        __builtin_amdgcn_wave_barrier();
        const bool first_term = !CONT && p == 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          float tv = tg[e] == tag ? hv[e] : base[e];
          if constexpr (DENSE) tv = dn ? DV[0][q].v[e] : tv;
          const float term = tv * w;
          acc[e] = first_term ? term : acc[e] + term;
        }
      }
#pragma unroll
      for (int q = 0; q < FW_G; ++q) {
        WI[0][q] = WI[1][q];
        WV[0][q] = WV[1][q];
        if constexpr (DENSE) DV[0][q] = DV[1][q];
      }
    }
    if (a.add_self) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = acc[e] + L.v[e] * a.w_self;
    }
    fw_store<true, EPL, GUARD>(a.out, tlo, lane, n, acc);
    if (a.out2) fw_store<true, EPL, GUARD>(a.out2, tlo, lane, n, acc);
    L = Ln;
    if (++seq == SEQ_WRAP) {  // tags restart: no stale tag of this row may match a new one
      seq = 0;
#pragma unroll
      for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = ~0u;
    }
  };
  const int64_t tfull = n / TE;  // tiles wholly inside [0, n)
  const int64_t tf = t1 < tfull ? t1 : (tfull > t0 ? tfull : t0);
  for (int64_t tile = t0; tile < tf; ++tile) tile_body(tile, std::false_type{});
  if (tf < t1) tile_body(tf, std::true_type{});  // the global last tile, ragged
}

// ONE launch for the folds of the table's nodes (fold_batch_walk, the batches
// fold_walk_batch_kernel does not take): as there, the nodes' tiles form one range [0, m * ntl)
// that the persistent grid's waves split into contiguous runs, a run crossing a node boundary
// continuing in the next node's fold; no block barrier, one LDS row per wave.  A node of <= 4
// sparse payloads runs fold_walk_run, any other fold_any_run.  Dense payloads only at
// EPL <= 4 (fold_batch_plan: a dense payload's tile values are EPL registers per slot).
template <int EPL>
__global__ void __launch_bounds__(256) fold_walk_any_kernel(FoldAnyBatch b, int64_t tpw) {
  constexpr int TE = 64 * EPL;
  const int64_t ntl = (b.n + TE - 1) / TE;
  const int64_t m = b.m;
  __shared__ float s_val[FW_WAVES][TE];
  __shared__ uint32_t s_tag[FW_WAVES][TE];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wv = s_val[wid];
  uint32_t* wt = s_tag[wid];
#pragma unroll
  for (int e = 0; e < EPL; ++e) wt[lane + 64 * e] = 0xFFFFFFFFu;
  const int64_t gw = (int64_t)blockIdx.x * FW_WAVES + fw_uni(wid);
  if (b.guard) {  // a missed encode: no fold of this launch writes (the host re-runs the round)
    bool bad = false;
    for (int64_t i = lane; i < b.guard_n; i += 64) bad |= b.guard[i] != 0;
    if (__ballot(bad) != 0) return;  // every wave reads the same final words
  }
  int64_t g = gw * tpw;
  const int64_t gend = m * ntl;
  const int64_t g1 = g + tpw < gend ? g + tpw : gend;
  uint32_t seq = 0;
  while (g < g1) {
    const int64_t node = g / ntl;
    const int64_t lt0 = g - node * ntl;
    const int64_t lt1 = lt0 + (g1 - g) < ntl ? lt0 + (g1 - g) : ntl;
    const FoldAnyNode& nd = b.s[node].nd;
    const int fl = nd.fl;
    const bool last = (fl & FA_LAST) != 0;
    const FoldAnyView v{nd.local,
                        nd.out,
                        (last && (fl & FA_LOCAL)) ? const_cast<float*>(nd.local) : nullptr,
                        b.n,
                        nd.np,
                        (last && b.add_self) ? 1 : 0,
                        0,
                        nd.w_self,
                        FoldAnyPayloads{&b.s[m + nd.p0]}};
    if (!(fl & FA_FIRST)) {
      fold_any_run<EPL, (EPL <= 4), true>(v, lt0, lt1, wv, wt, lane, seq);
    } else if (fl & FA_DENSE) {
      if constexpr (EPL <= 4) fold_any_run<EPL, true, false>(v, lt0, lt1, wv, wt, lane, seq);
    } else if (nd.np <= 4) {
      fold_walk_run<true, EPL, 4>(v, lt0, lt1, wv, wt, lane, seq);
    } else {
      fold_any_run<EPL, false, false>(v, lt0, lt1, wv, wt, lane, seq);
    }
    g += lt1 - lt0;
  }
}

// The walk grid over `tiles` tiles: a persistent grid of what the CUs hold (`blocks` on entry),
// each wave a contiguous run of tpw tiles.
static int64_t walk_grid(int64_t tiles, int64_t& blocks) {
  const int64_t need = (tiles + FW_WAVES - 1) / FW_WAVES;
  if (blocks > need) blocks = need;
  if (blocks < 1) blocks = 1;
  return (tiles + blocks * FW_WAVES - 1) / (blocks * FW_WAVES);
}

// f(integral_constant<EPL>) for a run-time epl
template <class F>
static int with_epl(int epl, F f) {
  switch (epl) {
    case 16: return f(std::integral_constant<int, 16>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 2>{});
  }
}

// DIST 0: fold_walk_kernel (1..4 payloads); 1 / 3: the groups kernel
template <bool VEC, int EPL, int DIST, bool W2>
static int launch_walk_t(const FoldArgs& fa, hipStream_t st) {
  static const int slots = [] {
    if constexpr (DIST == 0) return cu_slots(reinterpret_cast<const void*>(fold_walk_kernel<VEC, EPL, 4>), 256, 0);
    else return cu_slots(reinterpret_cast<const void*>(fold_walk_groups_kernel<VEC, EPL, DIST, W2>), 256, 0);
  }();
  int64_t blocks = slots;
  // DPZ_WALK_BLOCKS=N: the walk grid at N blocks (diagnostic build, A/B)
  if (DPZ_KNOB_INT(WALK_BLOCKS, 0) > 0) blocks = DPZ_KNOB_INT(WALK_BLOCKS, 0);
  const int64_t tpw = walk_grid((fa.n + 64 * EPL - 1) / (64 * EPL), blocks);
  if constexpr (DIST == 0) {
    DPZ_TIMED(DPZ_KT_FOLD, st, (fold_walk_kernel<VEC, EPL, 4><<<(unsigned)blocks, 256, 0, st>>>(fa, tpw)));
  } else {
    DPZ_TIMED(DPZ_KT_FOLD, st,
              (fold_walk_groups_kernel<VEC, EPL, DIST, W2><<<(unsigned)blocks, 256, 0, st>>>(fa, tpw)));
  }
  return DPZ_OK;
}

template <bool VEC, int EPL>
static int launch_walk_e(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st) {
  if (pl.engine == DPZ_FOLD_ENGINE_WALK) return launch_walk_t<VEC, EPL, 0, false>(fa, st);
  const bool w2 = pl.win == 128;
  if (pl.dist == 3)
    return w2 ? launch_walk_t<VEC, EPL, 3, true>(fa, st) : launch_walk_t<VEC, EPL, 3, false>(fa, st);
  return w2 ? launch_walk_t<VEC, EPL, 1, true>(fa, st) : launch_walk_t<VEC, EPL, 1, false>(fa, st);
}

// The plan's walk kernel (fold_plan: VEC, the tile size 64 * EPL from the densest payload, and
// for 5..16 payloads how far ahead and how wide the windows are).
int launch_walk(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st) {
  return with_epl(pl.epl, [&](auto e) {
    constexpr int EPL = decltype(e)::value;
    return pl.vec ? launch_walk_e<true, EPL>(fa, pl, st) : launch_walk_e<false, EPL>(fa, pl, st);
  });
}

template <int EPL>
static int launch_walk_batch_t(const FoldNodeBatch& b, hipStream_t st) {
  static const int slots =
      cu_slots(reinterpret_cast<const void*>(fold_walk_batch_kernel<true, EPL>), 256, 0);
  int64_t blocks = slots;
  const int64_t tpw = walk_grid((int64_t)b.m * ((b.n + 64 * EPL - 1) / (64 * EPL)), blocks);
  DPZ_TIMED(DPZ_KT_FOLD, st, (fold_walk_batch_kernel<true, EPL><<<(unsigned)blocks, 256, 0, st>>>(b, tpw)));
  return DPZ_OK;
}

template <int EPL>
static int launch_walk_any_t(const FoldAnyBatch& b, hipStream_t st) {
  static const int slots =
      cu_slots(reinterpret_cast<const void*>(fold_walk_any_kernel<EPL>), 256, 0);
  int64_t blocks = slots;
  const int64_t tpw = walk_grid((int64_t)b.m * ((b.n + 64 * EPL - 1) / (64 * EPL)), blocks);
  DPZ_TIMED(DPZ_KT_FOLD, st, (fold_walk_any_kernel<EPL><<<(unsigned)blocks, 256, 0, st>>>(b, tpw)));
  return DPZ_OK;
}

// The nodes of the next launch of pass r of the any-degree batch, from node j0 on: pass r folds
// payloads [16 r, 16 r + 16) of every node that has them (a finished node is skipped), and a
// launch takes nodes, in order, while their slots (one per node, one per payload) fit the table.
// Returns the node after the launch's last; *nodes: the nodes the launch folds.
static int fold_any_chunk(int m, const int* n_payloads, int r, int j0, int* nodes) {
  int slots = 0, cnt = 0, j = j0;
  for (; j < m; ++j) {
    const int left = n_payloads[j] - r * FOLD_MAXP;
    if (left <= 0) continue;
    const int g = left < FOLD_MAXP ? left : FOLD_MAXP;
    if (slots + 1 + g > FA_SLOTS) break;
    slots += 1 + g;
    ++cnt;
  }
  *nodes = cnt;
  return j;
}

// How dpz_decode_average_batch folds a batch (dpz_debug_fold_batch_plan; fold_batch_walk launches
// by the same plan).  Pure: no HIP call.  dense[i] != 0: payload i of the flattened payload list
// is dense (nullptr: none); aligned: every local, out and dense row is 16-byte aligned.
struct FoldBatchPlan {
  int path;      // 0: node after node, 1: fold_walk_batch_kernel, 2: fold_walk_any_kernel
  int launches;  // the kernel launches of the call
  int first;     // nodes of the first launch
  int passes;    // ceil(largest payload count / 16)
  int epl;       // paths 1, 2: the walk's elements per lane
};
static FoldBatchPlan fold_batch_plan_one_launch(int m, int64_t n, const int* n_payloads,
                                                const int64_t* k, const int* dense, int flags,
                                                int aligned) {
  FoldBatchPlan bp{};
  int maxnp = 0;
  for (int j = 0; j < m; ++j) maxnp = n_payloads[j] > maxnp ? n_payloads[j] : maxnp;
  bp.passes = (maxnp + FOLD_MAXP - 1) / FOLD_MAXP;
  if (DPZ_KNOB_INT(FOLD_BATCH, 1) == 0) return bp;  // diagnostic build: per-node launches (A/B)
  if (m < 2 || (flags & ~(DPZ_FOLD_SELF | DPZ_FOLD_ALSO_LOCAL)) || !aligned) return bp;
  if (n < 1024 || n >= (int64_t(1) << 31) - 1024) return bp;
  int64_t kmax = 0;
  bool any_dense = false;
  int64_t off = 0;
  for (int j = 0; j < m; ++j) {
    const int np = n_payloads[j];
    if (np < 1) return bp;
    for (int i = 0; i < np; ++i) {
      const int64_t kk = k[off + i];
      if (dense && dense[off + i]) {
        if (kk != n) return bp;
        any_dense = true;
      } else {
        if (kk < 1 || kk > n) return bp;  // sparse, non-empty
        if (kk > kmax) kmax = kk;
      }
    }
    off += np;
  }
  // a dense payload may be another node's local row, which DPZ_FOLD_ALSO_LOCAL overwrites
  // during the same launch
  if (any_dense && (flags & DPZ_FOLD_ALSO_LOCAL)) return bp;
  // the walk's tile size: the plan of a fold of the batch's densest sparse payload
  FoldShape sh{};
  sh.n = n; sh.np = 1; sh.k[0] = kmax > 0 ? kmax : 1; sh.flags = DPZ_FOLD_SELF; sh.fresh = 1;
  sh.aligned = 1;
  const FoldPlan pl = fold_plan(sh);
  if (pl.engine != DPZ_FOLD_ENGINE_WALK) return bp;  // (a forced kind: per-node launches)
  bp.epl = pl.epl;
  if (!any_dense && maxnp <= 4) {
    bp.path = 1;
    bp.launches = (m + FW_BATCH - 1) / FW_BATCH;
    bp.first = m < FW_BATCH ? m : FW_BATCH;
    return bp;
  }
  bp.path = 2;
  // a dense payload's tile values are EPL registers per window slot: tiles of <= 256 elements
  if (any_dense && bp.epl > 4) bp.epl = 4;
  bp.launches = 0;
  for (int r = 0; r < bp.passes; ++r)
    for (int j = 0; j < m;) {
      int cnt = 0;
      j = fold_any_chunk(m, n_payloads, r, j, &cnt);
      if (cnt > 0 && bp.launches++ == 0) bp.first = cnt;
    }
  return bp;
}

static FoldBatchPlan fold_batch_plan(int m, int64_t n, const int* n_payloads, const int64_t* k,
                                     const int* dense, int flags, int aligned) {
  FoldBatchPlan bp = fold_batch_plan_one_launch(m, n, n_payloads, k, dense, flags, aligned);
  if (bp.path != 0) return bp;
  // node after node: every group of <= 16 payloads its own plan (the offsets pre-pass counts)
  bp.first = m > 0 ? 1 : 0;
  int64_t off = 0;
  for (int j = 0; j < m; ++j) {
    const int np = n_payloads[j];
    for (int base = 0; base == 0 || base < np; base += FOLD_MAXP) {
      FoldShape sh{};
      sh.n = n > 0 ? n : 1;
      sh.np = (np - base) < FOLD_MAXP ? (np - base) : FOLD_MAXP;
      sh.flags = flags; sh.fresh = base == 0; sh.aligned = aligned;
      for (int i = 0; i < sh.np; ++i) {
        sh.k[i] = k[off + base + i];
        if (dense && dense[off + base + i]) sh.dense_mask |= 1u << i;
      }
      const FoldPlan pl = fold_plan(sh);
      bp.launches += (pl.offsets ? 1 : 0) + (pl.engine != DPZ_FOLD_ENGINE_NONE ? 1 : 0);
    }
    off += np;
  }
  return bp;
}

// dpz_decode_average_batch's one-launch paths over 16-byte aligned rows of the same n, flags
// within DPZ_FOLD_SELF | DPZ_FOLD_ALSO_LOCAL: fold_walk_batch_kernel when every node's fold is a
// plain Metro-Hastings walk of 1..4 sparse payloads, else fold_walk_any_kernel (any payload
// count >= 1, more than 16 in further launches that continue the total; dense payloads without
// DPZ_FOLD_ALSO_LOCAL).  Returns 1 (nothing enqueued) when the batch does not qualify.
int fold_batch_walk(int m, const float* const* local, float* const* out, int64_t n,
                    const int* n_payloads, const int32_t* const* idx, const float* const* vals,
                    const int64_t* k, const float* w, const float* w_self, int flags,
                    hipStream_t st, const int32_t* guard, int64_t guard_n) {
  // (every array this path reads is checked here: a null one falls through to the per-node
  // validation, which returns DPZ_ERR_ARG)
  if (m < 2 || !w || !idx || !vals || !k || !n_payloads || !local || !out) return 1;
  int64_t off = 0;
  int aligned = 1;
  for (int j = 0; j < m; ++j) {
    if (n_payloads[j] < 1 || !local[j] || !out[j] || local[j] == out[j]) return 1;
    if (((reinterpret_cast<uintptr_t>(local[j]) | reinterpret_cast<uintptr_t>(out[j])) & 15u) != 0)
      aligned = 0;
    off += n_payloads[j];
  }
  std::vector<int> dense((size_t)off);
  for (int64_t i = 0; i < off; ++i) {
    if (!vals[i]) return 1;
    dense[i] = idx[i] ? 0 : 1;
    if (dense[i] && (reinterpret_cast<uintptr_t>(vals[i]) & 15u) != 0) aligned = 0;
  }
  const FoldBatchPlan bp = fold_batch_plan(m, n, n_payloads, k, dense.data(), flags, aligned);
  if (bp.path == 0) return 1;
  if (bp.path == 2) {
    std::vector<int64_t> first((size_t)m);  // node j's first payload in the flattened list
    off = 0;
    for (int j = 0; j < m; ++j) {
      first[j] = off;
      off += n_payloads[j];
    }
    for (int r = 0; r < bp.passes; ++r)
      for (int j0 = 0; j0 < m;) {
        int cnt = 0;
        const int j1 = fold_any_chunk(m, n_payloads, r, j0, &cnt);
        if (cnt > 0) {
          FoldAnyBatch b{};
          b.n = n;
          b.m = cnt;
          b.add_self = (flags & DPZ_FOLD_SELF) ? 1 : 0;
          b.guard = guard;
          b.guard_n = guard ? guard_n : 0;
          int c = 0, p0 = 0;
          for (int j = j0; j < j1; ++j) {
            const int left = n_payloads[j] - r * FOLD_MAXP;
            if (left <= 0) continue;
            const int g = left < FOLD_MAXP ? left : FOLD_MAXP;
            FoldAnyNode& nd = b.s[c].nd;
            nd.local = local[j];
            nd.out = out[j];
            nd.w_self = w_self ? w_self[j] : 0.0f;
            nd.p0 = (uint16_t)p0;
            nd.np = (uint8_t)g;
            int fl = (r == 0 ? FA_FIRST : 0) | (left <= FOLD_MAXP ? FA_LAST : 0) |
                     ((flags & DPZ_FOLD_ALSO_LOCAL) ? FA_LOCAL : 0);
            for (int i = 0; i < g; ++i) {
              const int64_t s = first[j] + (int64_t)r * FOLD_MAXP + i;
              FoldAnyPayload& p = b.s[cnt + p0 + i].p;
              p.idx = idx[s];
              p.val = vals[s];
              p.k = (int32_t)k[s];
              p.w = w[s];
              if (!idx[s]) fl |= FA_DENSE;
            }
            nd.fl = (uint8_t)fl;
            p0 += g;
            ++c;
          }
          const int rc = with_epl(bp.epl, [&](auto e) { return launch_walk_any_t<decltype(e)::value>(b, st); });
          if (rc != DPZ_OK) return rc;
        }
        j0 = j1;
      }
    return DPZ_OK;
  }
  const FoldPlan pl{DPZ_FOLD_ENGINE_WALK, 1, bp.epl};
  off = 0;
  for (int j0 = 0; j0 < m; j0 += FW_BATCH) {
    FoldNodeBatch b{};
    b.n = n;
    b.m = (m - j0) < FW_BATCH ? (m - j0) : FW_BATCH;
    b.add_self = (flags & DPZ_FOLD_SELF) ? 1 : 0;
    b.guard = guard;
    b.guard_n = guard ? guard_n : 0;
    for (int j = 0; j < b.m; ++j) {
      FoldNode& nd = b.nd[j];
      const int jj = j0 + j;
      nd.local = local[jj];
      nd.out = out[jj];
      nd.out2 = (flags & DPZ_FOLD_ALSO_LOCAL) ? const_cast<float*>(local[jj]) : nullptr;
      nd.np = n_payloads[jj];
      nd.w_self = w_self ? w_self[jj] : 0.0f;
      for (int i = 0; i < nd.np; ++i) {
        nd.p[i].idx = idx[off + i];
        nd.p[i].val = vals[off + i];
        nd.p[i].k = k[off + i];
        nd.p[i].w = w[off + i];
      }
      off += nd.np;
    }
    const int rc = with_epl(pl.epl, [&](auto e) { return launch_walk_batch_t<decltype(e)::value>(b, st); });
    if (rc != DPZ_OK) return rc;
  }
  return DPZ_OK;
}

}  // namespace dpz

extern "C" int dpz_debug_fold_batch_plan(int m, int64_t n, const int* n_payloads, const int64_t* k,
                                         const int* dense, int flags, int aligned,
                                         int* plan_out) {
  if (m < 0 || n <= 0 || !n_payloads || !k || !plan_out) return DPZ_ERR_ARG;
  for (int j = 0; j < m; ++j)
    if (n_payloads[j] < 0) return DPZ_ERR_ARG;
  const dpz::FoldBatchPlan bp = dpz::fold_batch_plan(m, n, n_payloads, k, dense, flags, aligned);
  plan_out[0] = bp.path;
  plan_out[1] = bp.launches;
  plan_out[2] = bp.first;
  plan_out[3] = bp.passes;
  return DPZ_OK;
}
