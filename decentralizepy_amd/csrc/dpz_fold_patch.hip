// The folds that touch only what the payloads hit: the standalone replace / add of one sparse
// payload (replace_kernel), the fold base on its own (fold_base_kernel) and the rewrite of the hit
// elements over a ready base (DPZ_FOLD_BASE_READY: fold_patch_kernel, fold_patch1_kernel).
#include "dpz_fold_cursor.h"
#include "dpz_replace.h"

namespace dpz {

// Replace-only decode of ONE sparse payload (reference PartialModel.py:257-303, T[idx] = params):
// one 256-thread block per chunk of RP_E payload entries (dpz_replace.h).
// Standalone replace: one wave per chunk of RP_E entries (~1,600 elements at 1 %), a grid of
// many short blocks (measured on MI355X: shorter than persistent waves walking the chunks with
// the next chunk's entries prefetched, and than 64-entry chunks per 256-thread block).
__global__ void __launch_bounds__(256) replace_kernel(ReplaceJob j) { replace_block(j, blockIdx.x); }

int launch_replace(const ReplaceJob& j, hipStream_t st) {
  if (j.c1 > j.c0)
    DPZ_TIMED(DPZ_KT_FOLD, st, replace_kernel<<<(unsigned)((j.c1 - j.c0 + 3) / 4), 256, 0, st>>>(j));
  return DPZ_OK;
}

// ---- the fold base on its own (dpz_topk_encode_foldbase off the pipelined filter) -------------
template <bool VEC>
__global__ void __launch_bounds__(256) fold_base_kernel(const float* __restrict__ x, int64_t n,
                                                        FoldBase fb, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (VEC) {
    const int64_t n4 = n >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += stride) {
      const float4 v = reinterpret_cast<const float4*>(x)[g];
      reinterpret_cast<float4*>(out)[g] = make_float4(fb.of(v.x), fb.of(v.y), fb.of(v.z), fb.of(v.w));
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
      out[i] = fb.of(x[i]);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = fb.of(x[i]);
  }
}

int launch_fold_base(const float* x, int64_t n, const FoldBase& fb, float* out, hipStream_t st) {
  if (n <= 0) return DPZ_OK;
  const int64_t groups = (n + 3) / 4;
  unsigned nb = (unsigned)((groups + 255) / 256);
  if (nb > 4096) nb = 4096;
  if (aligned16(x) && aligned16(out))
    DPZ_TIMED(DPZ_KT_FOLD, st, fold_base_kernel<true><<<nb, 256, 0, st>>>(x, n, fb, out));
  else
    DPZ_TIMED(DPZ_KT_FOLD, st, fold_base_kernel<false><<<nb, 256, 0, st>>>(x, n, fb, out));
  return DPZ_OK;
}

// ---- DPZ_FOLD_BASE_READY: rewrite only the elements the payloads hit --------------------------
// out already holds the fold of every element's local value alone (FoldBase::of, written by the
// encoder's filter); an element hit by one or more payloads is folded here exactly, in the
// reference's order (payload terms in payload order, then the self term).  Block b owns the
// 4096-element tile b: its payload runs come from fold_offsets_kernel's tile starts (one coalesced
// pre-pass over the payload indices, so a block's chain is starts -> entries -> local gather ->
// store), staged in LDS, and each entry whose element no EARLIER payload hits (an LDS binary
// search per earlier run) folds that element: the local value gathered once, the later payloads'
// values by LDS binary search.  A tile whose runs exceed the LDS stage is processed in halves,
// the sub-ranges' runs found by lock-step searches (adversarially clustered payloads; always
// terminates: one element holds <= 16 entries).  Bytes: the payload entries, a local gather and
// an out write per hit element.
constexpr int PT_CAP = 1024;  // entries staged per pass (8 KB of LDS: 8 blocks per CU)
constexpr int PT_EPT = PT_CAP / 256;

__device__ __forceinline__ int pt_find(const int32_t* sidx, int b, int e, int32_t key) {
  // position of key in the sorted LDS run [b, e), or -1
  while (b < e) {
    const int m = (b + e) >> 1;
    const int32_t v = sidx[m];
    if (v < key) b = m + 1;
    else if (v > key) e = m;
    else return m;
  }
  return -1;
}

__global__ void __launch_bounds__(256) fold_patch_kernel(FoldArgs a, int64_t range) {
  // range == FOLD_TILE: the first pass takes its runs from a.starts (fold_offsets_kernel)
  __shared__ int32_t s_idx[PT_CAP];
  __shared__ float s_val[PT_CAP];
  __shared__ int32_t s_rlo[FOLD_MAXP], s_rhi[FOLD_MAXP], s_off[FOLD_MAXP + 1];
  const int t = threadIdx.x, wid = t >> 6, lane = t & 63;
  const int np = a.np;
  const int64_t n = a.n;
  const int64_t b_lo = (int64_t)blockIdx.x * range;
  const int64_t b_hi = b_lo + range < n ? b_lo + range : n;
  int64_t cur = b_lo, len = b_hi - b_lo;
  bool from_starts = a.starts != nullptr;
  while (cur < b_hi) {
    const int64_t s_end = cur + len < b_hi ? cur + len : b_hi;
    if (from_starts) {  // the whole tile: runs from the pre-pass
      if (t < np) {
        const int32_t* st = a.starts + (int64_t)t * (a.ntiles + 1);
        s_rlo[t] = st[blockIdx.x];
        s_rhi[t] = st[blockIdx.x + 1];
      }
    } else {
    // runs of [cur, s_end): wave w searches payloads w, w + 4, w + 8, w + 12, both ends, in lock
    // step (virtual search q: payload w + 4 (q & 3), target q < 4 ? cur : s_end)
      const int32_t lo32 = (int32_t)cur, hi32 = (int32_t)s_end;
      const int32_t r = fw_lower_bounds<8>(
          8, [&](int q) { return q < 4 ? lo32 : hi32; }, lane,
          [&](int q) { return a.p[wid + 4 * (q & 3)].idx; },
          [&](int q) {
            const int pp = wid + 4 * (q & 3);
            return pp < np ? (int32_t)a.p[pp].k : 0;
          },
          reinterpret_cast<const int32_t*>(a.local));
      if (lane < 8) {
        const int pp = wid + 4 * (lane & 3);
        if (pp < np) {
          if (lane < 4) s_rlo[pp] = r;
          else s_rhi[pp] = r;
        }
      }
    }
    from_starts = false;
    __syncthreads();
    if (t == 0) {
      int32_t o = 0;
      for (int p = 0; p < np; ++p) {
        s_off[p] = o;
        o += s_rhi[p] > s_rlo[p] ? s_rhi[p] - s_rlo[p] : 0;
      }
      s_off[np] = o;
    }
    __syncthreads();
    const int total = s_off[np];
    if (total > PT_CAP) {  // uniform: halve the range and search again
      len = (s_end - cur + 1) / 2;
      __syncthreads();
      continue;
    }
    // stage the runs (payload-major, each run sorted)
    for (int j = t; j < total; j += 256) {
      int p = 0;
      while (p + 1 < np && j >= s_off[p + 1]) ++p;
      const int64_t src = (int64_t)s_rlo[p] + (j - s_off[p]);
      s_idx[j] = as_global(a.p[p].idx)[src];
      s_val[j] = as_global(a.p[p].val)[src];
    }
    __syncthreads();
    // owners: entry j of payload p folds its element iff no earlier payload's run holds it; the
    // local values of every owned element are gathered before any later-payload search
    int32_t ee[PT_EPT];
    int pj[PT_EPT];
    float xv[PT_EPT];
#pragma unroll
    for (int i = 0; i < PT_EPT; ++i) {
      const int j = t + 256 * i;
      ee[i] = -1;
      pj[i] = 0;
      if (j < total) {
        int p = 0;
        while (p + 1 < np && j >= s_off[p + 1]) ++p;
        const int32_t e = s_idx[j];
        bool own = e >= cur && e < s_end;  // an invalid (unsorted) payload cannot write outside
        for (int q = 0; q < p && own; ++q) own = pt_find(s_idx, s_off[q], s_off[q + 1], e) < 0;
        if (own) {
          ee[i] = e;
          pj[i] = p;
        }
      }
      xv[i] = a.local[ee[i] >= 0 ? ee[i] : 0];
    }
#pragma unroll
    for (int i = 0; i < PT_EPT; ++i) {
      if (ee[i] < 0) continue;
      const int j = t + 256 * i;
      const int p = pj[i];
      const float x = xv[i];
      float acc = 0.0f;
      for (int q = 0; q < np; ++q) {
        float v = x;
        if (q == p) {
          v = s_val[j];
        } else if (q > p) {
          const int pos = pt_find(s_idx, s_off[q], s_off[q + 1], ee[i]);
          if (pos >= 0) v = s_val[pos];
        }
        const float term = v * a.p[q].w;
        acc = q == 0 ? term : acc + term;
      }
      acc = acc + x * a.w_self;
      a.out[ee[i]] = acc;
    }
    __syncthreads();  // the stage is reused by the next sub-range
    cur = s_end;
    len = b_hi - cur;
  }
}

// One payload: its indices are unique, so every hit element is hit once and each entry folds its
// element alone (out[e] = v·w + x[e]·w_self, the reference's order) — no tile runs, no pre-pass.
// Four entries per thread, strided by the block so the idx / val loads stay coalesced; the local
// gathers of all four are issued before any store.
__global__ void __launch_bounds__(256) fold_patch1_kernel(const int32_t* __restrict__ idx,
                                                          const float* __restrict__ val, int64_t k,
                                                          const float* __restrict__ local,
                                                          float* __restrict__ out, int64_t n,
                                                          float w, float w_self) {
  const int64_t j0 = (int64_t)blockIdx.x * 1024 + threadIdx.x;
  int32_t e[4];
  float v[4], xv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t j = j0 + 256 * i;
    e[i] = j < k ? idx[j] : -1;
    v[i] = j < k ? val[j] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (e[i] >= n) e[i] = -1;  // an invalid payload cannot write outside
    xv[i] = local[e[i] >= 0 ? e[i] : 0];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (e[i] < 0) continue;
    const float acc = v[i] * w;
    out[e[i]] = acc + xv[i] * w_self;
  }
}

// one payload: fold_patch1_kernel; more: fold_patch_kernel over the pre-pass's tile starts
int launch_fold_patch(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st) {
  if (pl.engine == DPZ_FOLD_ENGINE_PATCH1) {
    const int64_t k = fa.p[0].k;
    DPZ_TIMED(DPZ_KT_FOLD, st,
              fold_patch1_kernel<<<(unsigned)((k + 1023) / 1024), 256, 0, st>>>(
                  fa.p[0].idx, fa.p[0].val, k, fa.local, fa.out, fa.n, fa.p[0].w, fa.w_self));
    return DPZ_OK;
  }
  DPZ_TIMED(DPZ_KT_FOLD, st, fold_patch_kernel<<<(unsigned)fa.ntiles, 256, 0, st>>>(fa, FOLD_TILE));
  return DPZ_OK;
}

}  // namespace dpz
