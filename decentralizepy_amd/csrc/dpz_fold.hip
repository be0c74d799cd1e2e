// Batched decode (replace) + Metro-Hastings weighted fold over a gossip round's payloads.
//
// Replaces (reference sacs-epfl/decentralizepy, src/decentralizepy/):
//   sharing/PartialModel.py:257-303  deserialized_model: T = cat(local); T[idx] = params
//   sharing/Sharing.py:156-190       _averaging: total = T_0*w_0; total += T_i*w_i; += (1-sum)*local
//   sharing/Sharing.py:200-229       _averaging_server: w = 1/n, no self term
//   sharing/JWINS/Wavelet.py:269-309 the same fold on wavelet coefficients
//
// This unit validates the call, plans each group of <= 16 payloads (fold_plan) and launches the
// plan's engine.  Six engines, one unit each, all in the reference's fp32 order:
//   offsets + classic  dpz_fold_tile.hip   whatever no other engine takes: dense payloads, a
//                                          continued total, replace-only, no payloads
//   4-slot group       dpz_fold_tile.hip   >= 8 sparse payloads, 1536 .. 12288 entries per tile
//   walk               dpz_fold_walk.hip   a fresh all-sparse total of <= 4 payloads
//   walk groups        dpz_fold_walk.hip   ... of 5..16 payloads at 0.0175 <= k/n <= 0.21
//   merge              dpz_fold_merge.hip  ... of >= 6 payloads with <= 0.33 n entries in all
//   patch / replace    dpz_fold_patch.hip  DPZ_FOLD_BASE_READY; one sparse payload replaced/added
#include "dpz_fold.h"
#include "dpz_replace.h"

namespace dpz {

int cu_slots(const void* kernel, int threads, size_t dynamic_lds) {
  int dev = 0, cus = 256, per = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, dynamic_lds) != hipSuccess ||
      per < 1)
    per = 1;
  return cus * per;
}

// The thresholds are MI355X measurements at M = 25 M (tools/diag/fold_kinds.py, merge_time.py):
//  * merge against walk (profiles/r06_merge_time.jsonl): 16 x 0.005 88 vs 125 us, 16 x 0.01 105 vs
//    126, 16 x 0.02 129 vs 133, 8 x 0.01 69 vs 79; 16 x 0.03 173 vs 132, 3 x 0.01 at 64 MiB 41 vs 33;
//  * walk against the tile folds (profiles/r03_s2_fold_a001.jsonl): a node's few neighbours at
//    any alpha; 16 x 0.015 hit-chain 137 vs walk 147 us, 16 x 0.02 163 vs 149;
//  * the walk's tile: the largest that holds about one window per payload on average — fewer
//    tiles mean fewer window loads and LDS passes per element, and an overflowing window is
//    re-read synchronously (profiles/r03_s3_walk_win_sweep.txt: 16 x 0.1 at 512-element tiles 215
//    us, 1024: 283, 256: 287; 3 x 0.1: 64 / 72 / 77 us); 13..16 payloads above dens 0.055 take
//    128-entry windows (16 x 0.15: 297 -> 247 us, 16 x 0.2: 309 -> 266 against 64-entry windows
//    at 256-element tiles);
//  * 4-slot group against classic (25 M x 16): alpha 0.04 463 -> 193 us, 0.1 345 -> 284; the
//    hit-chain path stays faster at alpha 0.01, the phase path at 0.2 x 16 and for dense payloads.
// Diagnostic build: DPZ_FOLD_KIND=1 / 2 / 4 / 8 forces the classic / 4-slot group / walk / merge
// fold (a forced kind that cannot take the group runs the classic kernel), DPZ_FOLD_PHASES=1 the
// classic kernel's phase path, DPZ_FOLD_GROUP=0 / 1 the group kernel; DPZ_FOLD_WALK_EPL,
// DPZ_FOLD_WIN, DPZ_FOLD_DIST and DPZ_MERGE_EPT override the walk's and merge's parameters.
FoldPlan fold_plan(const FoldShape& s) {
  FoldPlan pl{};
  const int64_t n = s.n;
  const int np = s.np;
  const bool replace_only = (s.flags & DPZ_FOLD_REPLACE_ONLY) != 0;
  int64_t etot = 0;  // entries of the sparse payloads; dens: the densest one's k / n
  double dens = 0.0;
  for (int i = 0; i < np; ++i)
    if (!((s.dense_mask >> i) & 1u)) {
      etot += s.k[i];
      if ((double)s.k[i] / (double)n > dens) dens = (double)s.k[i] / (double)n;
    }
  if (s.flags & DPZ_FOLD_BASE_READY) {  // only the hit elements are rewritten
    if (etot == 0) return pl;
    pl.engine = np == 1 ? DPZ_FOLD_ENGINE_PATCH1 : DPZ_FOLD_ENGINE_PATCH;
    pl.offsets = np > 1;
    return pl;
  }
  pl.engine = DPZ_FOLD_ENGINE_CLASSIC;
  pl.vec = s.aligned;
  if (np == 0) return pl;  // out = w_self * local (self term only) or zeros
  // one sparse payload replaced or added: the range-partitioned chunk kernel (an empty or dense
  // payload takes the folds below, add-only with weight 1 and the self term)
  if ((replace_only || (s.flags & DPZ_FOLD_ADD_ONLY)) && np == 1 && !(s.dense_mask & 1u) &&
      s.k[0] > 0 && s.aligned) {
    pl.engine = DPZ_FOLD_ENGINE_REPLACE;
    return pl;
  }
  const bool all_sparse = s.dense_mask == 0 && DPZ_KNOB_INT(FOLD_PHASES, 0) == 0;
  pl.chains = all_sparse;
  const bool fresh_sparse = !replace_only && s.fresh && all_sparse;
  const int kind = (int)DPZ_KNOB_INT(FOLD_KIND, 0);
  const double avg = (double)etot / (double)np / (double)n;
  const bool merge_ok = fresh_sparse && n >= 1024 && n < (int64_t(1) << 31) - 8192 && s.aligned;
  bool use_merge = merge_ok && np >= 6 && (double)etot <= 0.33 * (double)n;
  if (kind) use_merge = merge_ok && kind == 8;
  if (use_merge) {
    pl.engine = DPZ_FOLD_ENGINE_MERGE;
    pl.ept = (int)DPZ_KNOB_INT(MERGE_EPT, 8);
    if (pl.ept != 4 && pl.ept != 8 && pl.ept != 16) pl.ept = 8;
    pl.eqw = 1;
    for (int i = 1; i < np; ++i) pl.eqw = pl.eqw && s.w[i] == s.w[0];
    return pl;
  }
  const bool walk_ok = fresh_sparse && n < (int64_t(1) << 31) - 1024;
  bool use_walk = walk_ok && (np <= 4 || (avg >= 0.0175 && avg <= 0.21));
  if (kind) use_walk = walk_ok && kind == 4;
  if (use_walk) {
    const bool four = np > 12;  // four groups of four payloads
    pl.engine = np <= 4 ? DPZ_FOLD_ENGINE_WALK : DPZ_FOLD_ENGINE_WALK_GROUPS;
    pl.vec = s.aligned && n >= 1024;
    pl.epl = dens <= 0.055 ? 16 : (dens <= 0.105 ? 8 : (dens <= 0.21 ? 4 : 2));
    bool w2 = false;
    if (four && dens > 0.055 && dens <= 0.21) {
      w2 = true;
      pl.epl = dens <= 0.105 ? 16 : 8;
    }
    const int e = (int)DPZ_KNOB_INT(FOLD_WALK_EPL, 0);
    if (e == 16 || e == 8 || e == 4 || e == 2) pl.epl = e;
    if (DPZ_KNOB_STR(FOLD_WIN)) w2 = DPZ_KNOB_INT(FOLD_WIN, 64) == 128;
    pl.win = (np > 4 && w2) ? 128 : 64;
    // 13..16 payloads: windows issued three groups ahead (DPZ_FOLD_DIST=1: one group ahead)
    pl.dist = (four && DPZ_KNOB_INT(FOLD_DIST, 3) != 1) ? 3 : 1;
    return pl;
  }
  pl.offsets = s.dense_mask != (1u << np) - 1u;  // any sparse payload
  if (all_sparse && !replace_only) {
    const int64_t ntiles = fold_ntiles(n);
    bool use_group = np >= 8 && etot > FOLD_GROUP_MIN * ntiles && etot <= 2 * (int64_t)FG_CAP * ntiles;
    if (DPZ_KNOB_STR(FOLD_GROUP)) use_group = DPZ_KNOB_INT(FOLD_GROUP, 0) != 0;
    if (kind) use_group = kind == 2;
    if (use_group) pl.engine = DPZ_FOLD_ENGINE_GROUP;
  }
  return pl;
}

// the plan's launches for one group
static int fold_run(const FoldPlan& pl, const FoldArgs& fa, int32_t* starts, int add,
                    hipStream_t st) {
  if (pl.offsets) {
    const int rc = launch_fold_offsets(fa, starts, st);
    if (rc != DPZ_OK) return rc;
  }
  switch (pl.engine) {
    case DPZ_FOLD_ENGINE_NONE: return DPZ_OK;
    case DPZ_FOLD_ENGINE_REPLACE:
      return launch_replace(ReplaceJob{fa.local, fa.p[0].idx, fa.p[0].val, fa.p[0].k, fa.n, fa.out,
                                       0, replace_chunks(fa.p[0].k), add}, st);
    case DPZ_FOLD_ENGINE_PATCH1:
    case DPZ_FOLD_ENGINE_PATCH: return launch_fold_patch(fa, pl, st);
    case DPZ_FOLD_ENGINE_MERGE: return launch_merge(fa, pl, st);
    case DPZ_FOLD_ENGINE_WALK:
    case DPZ_FOLD_ENGINE_WALK_GROUPS: return launch_walk(fa, pl, st);
    case DPZ_FOLD_ENGINE_GROUP: return launch_fold_group(fa, pl.vec != 0, st);
    default: return launch_fold_classic(fa, pl.vec != 0, st);
  }
}

}  // namespace dpz

using namespace dpz;

extern "C" int dpz_debug_fold_plan(int64_t n, int n_payloads, const int64_t* k, const int* dense,
                                   const float* w, int flags, int fresh, int aligned,
                                   int* plan_out) {
  if (n <= 0 || n_payloads < 0 || n_payloads > FOLD_MAXP || (n_payloads > 0 && !k) || !plan_out)
    return DPZ_ERR_ARG;
  FoldShape s{};
  s.n = n; s.np = n_payloads; s.flags = flags; s.fresh = fresh; s.aligned = aligned;
  for (int i = 0; i < n_payloads; ++i) {
    s.k[i] = k[i];
    s.w[i] = w ? w[i] : 0.0f;
    if (dense && dense[i]) s.dense_mask |= 1u << i;
  }
  const FoldPlan pl = fold_plan(s);
  const int v[DPZ_FOLD_PLAN_INTS] = {pl.engine, pl.vec, pl.epl, pl.dist, pl.win,
                                     pl.ept,    pl.eqw, pl.offsets, pl.chains};
  for (int i = 0; i < DPZ_FOLD_PLAN_INTS; ++i) plan_out[i] = v[i];
  return DPZ_OK;
}

extern "C" size_t dpz_decode_workspace_bytes(int64_t n, int n_payloads) {
  const int64_t np = n_payloads < FOLD_MAXP ? (n_payloads > 0 ? n_payloads : 1) : FOLD_MAXP;
  return (size_t)np * (size_t)(fold_ntiles(n > 0 ? n : 1) + 1) * sizeof(int32_t);
}

extern "C" int dpz_decode_average(const float* local, int64_t n, int n_payloads,
                                  const int32_t* const* idx, const float* const* vals,
                                  const int64_t* k, const float* w, float w_self, int flags,
                                  float* out, void* ws, size_t ws_bytes, dpz_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n < 0 || n_payloads < 0) return DPZ_ERR_ARG;
  if (n == 0) return DPZ_OK;
  if (!local || !out || local == out) return DPZ_ERR_ARG;
  const bool replace_only = (flags & DPZ_FOLD_REPLACE_ONLY) != 0;
  const bool add_only = (flags & DPZ_FOLD_ADD_ONLY) != 0;
  const bool zero_base = (flags & DPZ_FOLD_ZERO_BASE) != 0;
  if ((replace_only || add_only) && n_payloads != 1) return DPZ_ERR_ARG;
  const bool also_local = (flags & DPZ_FOLD_ALSO_LOCAL) != 0;
  if (also_local && (replace_only || add_only)) return DPZ_ERR_ARG;
  float* const out2 = also_local ? const_cast<float*>(local) : nullptr;
  if (replace_only && add_only) return DPZ_ERR_ARG;
  if (n_payloads > 0 && (!vals || !k || (!replace_only && !add_only && !w))) return DPZ_ERR_ARG;
  // payload i is dense (a full model) iff idx[i] == NULL and k[i] == n
  auto is_dense = [&](int i) { return (!idx || !idx[i]) && k[i] == n; };
  for (int i = 0; i < n_payloads; ++i) {
    if (k[i] < 0 || k[i] > n) return DPZ_ERR_ARG;
    if (!vals[i] && k[i] > 0) return DPZ_ERR_ARG;
    if (!is_dense(i) && k[i] > 0 && (!idx || !idx[i])) return DPZ_ERR_ARG;
  }
  if (!ws || ws_bytes < dpz_decode_workspace_bytes(n, n_payloads)) return DPZ_ERR_WORKSPACE;
  int32_t* starts = static_cast<int32_t*>(ws);
  if (flags & DPZ_FOLD_BASE_READY) {
    // out holds the no-hit base of exactly this fold (dpz_topk_encode_foldbase over local with
    // these weights): only the plain Metro-Hastings form of one group of sparse payloads
    if (flags & ~(DPZ_FOLD_BASE_READY | DPZ_FOLD_SELF)) return DPZ_ERR_ARG;
    if (!(flags & DPZ_FOLD_SELF) || n_payloads < 1 || n_payloads > FOLD_MAXP) return DPZ_ERR_ARG;
    if (n >= (int64_t(1) << 31) - 1024) return DPZ_ERR_UNSUPPORTED;
    FoldArgs fa{};
    FoldShape sh{};
    fa.local = local; fa.out = out; fa.starts = starts; fa.n = n; fa.ntiles = fold_ntiles(n);
    fa.np = n_payloads; fa.w_self = w_self;
    sh.n = n; sh.np = n_payloads; sh.flags = flags;
    for (int i = 0; i < n_payloads; ++i) {
      if (is_dense(i)) return DPZ_ERR_ARG;
      fa.p[i].idx = (idx && idx[i]) ? idx[i] : reinterpret_cast<const int32_t*>(local);
      fa.p[i].val = vals[i] ? vals[i] : local;
      fa.p[i].k = sh.k[i] = k[i];
      fa.p[i].w = sh.w[i] = w[i];
    }
    return fold_run(fold_plan(sh), fa, starts, 0, st);
  }
  bool vec = ((reinterpret_cast<uintptr_t>(local) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  for (int i = 0; i < n_payloads; ++i)
    if (is_dense(i) && (reinterpret_cast<uintptr_t>(vals[i]) & 15u)) vec = false;
  // no payloads: the classic kernel adds the self term to zeros (or to the running total)
  if (n_payloads == 0 && !(flags & DPZ_FOLD_ACCUMULATE))
    DPZ_HIP_TRY(hipMemsetAsync(out, 0, n * sizeof(float), st));
  for (int base = 0; base == 0 || base < n_payloads; base += FOLD_MAXP) {
    FoldArgs fa{};
    FoldShape sh{};
    fa.local = local; fa.out = out; fa.out2 = out2; fa.starts = starts; fa.n = n;
    fa.ntiles = fold_ntiles(n);
    fa.np = (n_payloads - base) < FOLD_MAXP ? (n_payloads - base) : FOLD_MAXP;
    sh.n = n; sh.np = fa.np; sh.flags = flags; sh.aligned = vec;
    sh.fresh = (base == 0 && !(flags & DPZ_FOLD_ACCUMULATE)) ? 1 : 0;
    fa.first = fa.np > 0 ? sh.fresh : 0;
    fa.add_self = (base + fa.np == n_payloads && ((flags & DPZ_FOLD_SELF) || add_only)) ? 1 : 0;
    // over local only with the last group: the earlier groups' launches still read local
    if (base + fa.np != n_payloads) fa.out2 = nullptr;
    fa.replace_only = replace_only ? 1 : 0;
    fa.zero_base = ((zero_base || add_only) && fa.np > 0) ? 1 : 0;
    fa.w_self = add_only ? 1.0f : w_self;
    for (int i = 0; i < fa.np; ++i) {
      // an empty sparse payload gets a dummy non-null idx (never read: its range is empty)
      fa.p[i].idx = is_dense(base + i) ? nullptr
                    : ((idx && idx[base + i]) ? idx[base + i] : reinterpret_cast<const int32_t*>(starts));
      fa.p[i].val = vals[base + i];
      fa.p[i].k = sh.k[i] = k[base + i];
      fa.p[i].w = sh.w[i] = (replace_only || add_only) ? 1.0f : w[base + i];
      if (!fa.p[i].idx) fa.dense_mask |= 1u << i;
    }
    sh.dense_mask = fa.dense_mask;
    const FoldPlan pl = fold_plan(sh);
    fa.all_sparse = pl.chains;
    const int rc = fold_run(pl, fa, starts, add_only ? 1 : 0, st);
    if (rc != DPZ_OK) return rc;
  }
  return DPZ_OK;
}

extern "C" int dpz_replace_slice(const float* local, int64_t n, int64_t offset,
                                 const int32_t* idx, const float* vals, int64_t k, float* out,
                                 dpz_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n < 0 || k < 0 || offset < 0) return DPZ_ERR_ARG;
  if (n == 0) return DPZ_OK;
  if (!local || !out || local == out || (k > 0 && (!idx || !vals))) return DPZ_ERR_ARG;
  if (!aligned16(local) || !aligned16(out)) return DPZ_ERR_ARG;
  if (k == 0) {
    DPZ_HIP_TRY(hipMemcpyAsync(out, local, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return DPZ_OK;
  }
  return launch_replace(ReplaceJob{local, idx, vals, k, n, out, 0, replace_chunks(k), 0, offset}, st);
}
