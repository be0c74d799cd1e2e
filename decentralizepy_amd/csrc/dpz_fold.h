// The sparse fold's shared types: the kernel arguments every engine takes, the plan that picks an
// engine for one group of payloads (fold_plan, dpz_fold.hip) and the engines' launches.
#pragma once
#include "dpz_common.h"

namespace dpz {

#ifndef DPZ_FOLD_TS
#define DPZ_FOLD_TS 12
#endif
constexpr int FOLD_TILE_SHIFT = DPZ_FOLD_TS;
constexpr int FOLD_TILE = 1 << FOLD_TILE_SHIFT;
constexpr int FOLD_MAXP = 16;  // payloads per launch (longer lists are chained)
// the 4-slot group kernel's window of average entries per tile (fold_plan; dpz_fold_tile.hip)
constexpr int FG_CAP = 6144;  // entries held per round (>= one payload's 4096)
#ifndef DPZ_FOLD_GROUP_MIN
#define DPZ_FOLD_GROUP_MIN 1536
#endif
constexpr int64_t FOLD_GROUP_MIN = DPZ_FOLD_GROUP_MIN;

struct FoldPayload {
  const int32_t* idx;  // nullptr: dense payload (vals has n entries)
  const float* val;
  int64_t k;
  float w;
};

struct FoldArgs {
  const float* local;
  float* out;
  float* out2;  // DPZ_FOLD_ALSO_LOCAL: the result also over local (in place), else nullptr
  const int32_t* starts;  // [np][ntiles + 1]
  int64_t n;
  int64_t ntiles;
  int np;
  int first;        // total starts from payload 0 (else continue from out)
  int add_self;     // add local * w_self at the end
  int replace_only; // out = t_0
  int zero_base;    // sparse payloads contribute 0 off their entries; first term = +0 + t0*w0
  int all_sparse;   // no dense payload in this group: the one-phase hit-chain path may run
  uint32_t dense_mask;  // bit p: payload p is dense (idx == nullptr)
  float w_self;
  FoldPayload p[FOLD_MAXP];
};

// A payload pointer rebuilt from lane registers (readlane) or read back from an LDS table has lost
// its address space: loads through it compile to FLAT loads, which count on lgkmcnt as well as vmcnt, so every LDS wait
// of the fold would also wait for the window loads in flight.  Global loads count on vmcnt only.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* as_global(const T* p) {
  return (const __attribute__((address_space(1))) T*)p;
}

// one payload term of the fold in the reference's fp32 order: the first term of a fresh total is
// t*w (+0 first with a zero base), later terms add; replace-only keeps the payload value
__device__ __forceinline__ void fold_term(float& acc, float tv, float w, bool first_term,
                                          int replace_only, int zero_base) {
  if (replace_only) {
    acc = tv;
  } else {
    const float term = tv * w;
    acc = first_term ? (zero_base ? 0.0f + term : term) : acc + term;
  }
}

static inline int64_t fold_ntiles(int64_t n) { return (n + FOLD_TILE - 1) / FOLD_TILE; }

// ---- the plan: which engine folds one group of <= FOLD_MAXP payloads, and how ----
struct FoldShape {
  int64_t n;
  int np;                // payloads of this group, 0 .. FOLD_MAXP
  int64_t k[FOLD_MAXP];
  float w[FOLD_MAXP];
  uint32_t dense_mask;   // bit p: payload p is dense
  int flags;             // the call's DPZ_FOLD_* flags
  int fresh;             // the group starts the total (the first group, no DPZ_FOLD_ACCUMULATE)
  int aligned;           // local, out and every dense payload's values are 16-byte aligned
};
struct FoldPlan {
  int engine;   // DPZ_FOLD_ENGINE_*
  int vec;      // classic, group, walk: the float4 kernels
  int epl;      // walk: elements per lane (the tile holds 64 * epl)
  int dist;     // walk groups: windows issued 1 or 3 groups ahead
  int win;      // walk groups: 64- or 128-entry windows
  int ept;      // merge: elements per thread
  int eqw;      // merge: every weight equal
  int offsets;  // the tile-offsets pre-pass runs first
  int chains;   // FoldArgs::all_sparse: the classic kernel may take its hit-chain path
};
// Pure: no HIP call, no state (the diagnostic build reads its DPZ_* switches here).
FoldPlan fold_plan(const FoldShape& s);

// Blocks a persistent grid of `kernel` keeps resident: CUs x max(1, occupancy).  Call sites cache
// it per kernel in a function-local static.
int cu_slots(const void* kernel, int threads, size_t dynamic_lds);

// ---- the engines (one unit each; fa.starts / fa.ntiles are set by the caller) ----
int launch_fold_offsets(const FoldArgs& fa, int32_t* starts, hipStream_t st);  // dpz_fold_tile.hip
int launch_fold_classic(const FoldArgs& fa, bool vec, hipStream_t st);
int launch_fold_group(const FoldArgs& fa, bool vec, hipStream_t st);
int launch_walk(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st);       // dpz_fold_walk.hip
int launch_merge(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st);      // dpz_fold_merge.hip
int launch_fold_patch(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st); // dpz_fold_patch.hip

}  // namespace dpz
