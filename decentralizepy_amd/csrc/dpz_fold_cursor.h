// Wave-level cursor searches over sorted payload indices, shared by the walk, merge and patch
// units: a wave's first entry of an element range (64-ary lower bounds) and the count of a sorted
// window's leading lanes.
#pragma once
#include "dpz_fold.h"

namespace dpz {

// the leading lanes whose index lies below `hi` (a sorted window): 0..64
__device__ __forceinline__ int fw_lead(bool in) {
  const uint64_t b = __ballot(in);
  return ~b == 0 ? 64 : (int)__builtin_ctzll(~b);
}

__device__ __forceinline__ int32_t fw_uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// lower_bound(idx_p, e0_of(p)) of every payload p < np (np <= NSX) as lane p's value: 64-ary searches
// (one wave-wide probe load per step) run in LOCK STEP over the payloads, so each round's np probe
// loads are in flight together and a wave's start costs ~log64(k) dependent round trips, not np
// times that (16 payloads at k = 2.5 M: 4 rounds instead of 64 dependent loads).  Probe loads are
// branch-free (an idle payload re-reads a valid word: entry 0 of `dflt`) so the compiler waits once
// per round.  idx_of(p) / k_of(p) take compile-time p.  The patch decode's sub-range searches.
template <int NSX, class IdxOf, class KOf, class E0Of>
__device__ __forceinline__ int32_t fw_lower_bounds(int np, E0Of e0_of, int lane, IdxOf idx_of,
                                                   KOf k_of, const int32_t* dflt) {
  int32_t slo[NSX], shi[NSX];
#pragma unroll
  for (int p = 0; p < NSX; ++p) {
    slo[p] = 0;
    shi[p] = p < np ? k_of(p) : 0;
  }
  for (;;) {
    int32_t xv[NSX], st[NSX];
    bool act = false;
#pragma unroll
    for (int p = 0; p < NSX; ++p) {
      const bool on = shi[p] > slo[p];
      act |= on;
      const int32_t len = shi[p] - slo[p];
      st[p] = on ? (len <= 64 ? 1 : (len + 63) / 64) : 0;
      const int64_t q = (int64_t)slo[p] + (int64_t)lane * st[p];
      const bool ok = on && q < shi[p];
      const auto* ip = as_global(on ? idx_of(p) : dflt);
      xv[p] = ip[ok ? q : (on ? (int64_t)slo[p] : 0)];
    }
    if (!act) break;
#pragma unroll
    for (int p = 0; p < NSX; ++p) {
      if (st[p] == 0) continue;  // uniform
      const int64_t q = (int64_t)slo[p] + (int64_t)lane * st[p];
      const int32_t c = (int32_t)__popcll(__ballot(q < shi[p] && xv[p] < e0_of(p)));  // a prefix
      if (st[p] == 1) {
        slo[p] += c;
        shi[p] = slo[p];
      } else {
        const int32_t nlo = c > 0 ? slo[p] + (c - 1) * st[p] + 1 : slo[p];
        const int64_t nhi = (int64_t)slo[p] + (int64_t)c * st[p];
        shi[p] = nhi < shi[p] ? (int32_t)nhi : shi[p];
        slo[p] = nlo;
      }
    }
  }
  int32_t cur = 0;
#pragma unroll
  for (int p = 0; p < NSX; ++p) cur = lane == p ? slo[p] : cur;
  return cur;
}

// A wave's start cursors, lower_bound(idx_p, e0) as lane p's value, one payload after the other.
// The lock-step search above, and the first tile's local values issued ahead of the search, were
// measured and not kept (MI355X, 96-node C4 round on 3 streams, fold leg: 3.00 ms sequential +
// local after, 3.14 sequential + local first, 3.42 / 3.33 lock step; 16-payload groups kernel at
// alpha 0.02 / 0.1 / 0.2: 122.1 / 170.2 / 255.2 us sequential vs 128.7 / 171.1 / 261.4): under
// concurrent codecs the lock-step probes delay every wave's first window.
template <int NSX, class IdxOf, class KOf>
__device__ __forceinline__ int32_t fw_start_cursors(int np, int32_t e0, int lane, IdxOf idx_of,
                                                    KOf k_of, const int32_t* dflt) {
  int32_t curv = 0;
#pragma unroll
  for (int p = 0; p < NSX; ++p) {
    if (p >= np) break;
    const int32_t* ip = idx_of(p);
    int32_t lo = 0, hi = k_of(p);
    while (hi > lo) {
      const int32_t len = hi - lo;
      const int32_t stride = len <= 64 ? 1 : (len + 63) / 64;
      const int64_t q = (int64_t)lo + (int64_t)lane * stride;
      const bool ok = q < hi;
      const int32_t x = ip[ok ? q : lo];
      const int32_t c = (int32_t)__popcll(__ballot(ok && x < e0));  // a prefix
      if (stride == 1) {
        lo += c;
        break;
      }
      const int32_t nlo = c > 0 ? lo + (c - 1) * stride + 1 : lo;
      const int64_t nhi = (int64_t)lo + (int64_t)c * stride;
      hi = nhi < hi ? (int32_t)nhi : hi;
      lo = nlo;
    }
    curv = lane == p ? lo : curv;
  }
  return curv;
}

}  // namespace dpz
