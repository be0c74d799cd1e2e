// The batched exact radix selection of the whole-topology round encodes (dpz_choco.hip,
// dpz_stc.hip, dpz_topkacc.hip, dpz_jwins.hip, dpz_fftround.hip): m nodes, the node in the grid's
// second dimension, one memset and nine launches whatever m is.
//
// The pass structure is that of the single-node exact selection (dpz_topk_exact.hip) with a
// control block, a 4096-bin histogram area and four per-chunk count arrays per node (node_ws).
// Three histogram passes (10/11/10 bits of the key |c|), each followed by a 1-block-per-node
// resolve, give T, the k-th largest key, and the number of ties at T to take; a count pass counts
// key > T and key == T per chunk of EX_CHUNK elements, a 1-block-per-node scan gives every chunk
// its output offset and its share of the ties in index order (ties go to the lowest indices), and
// the ordered compaction hands every selected element, ascending, with its slot to the engine.
// No float atomics; the result does not depend on the grid.
//
// What an engine is to the selection is its policy, a struct of static members:
//   Node, Args            the node table's record and the by-value arguments (Args::tab is the
//                         table); First, the optional second policy of select_nodes, is the policy
//                         of the first histogram pass alone (the same Node and Args)
//   kAllTies              false: exactly k are selected, ties at T to the lowest indices;
//                         true: every key >= max(T, 1) is (all ties, no zero keys)
//   kIdleNodes            idle(nd): every kernel's blocks leave such a node at once, the first
//                         histogram pass after idle_share(nd, n)
//   kHeader               the scan's thread 0 calls header(nd, a, count), count the selected
//   k(nd, a, n)           the node's k; slots(nd, a, n) its output slots, never written past
//   vec<FIRST>(nd, a)     whether load4<FIRST> may move float4s
//   load4<FIRST>(nd, a, i0, n, vec, c)
//                         the values c whose keys |c| are selected, of the 4 elements from i0
//                         (zeros past n); returns how many lie inside.  FIRST: the first
//                         histogram pass, where an engine that keeps a key row forms and stores
//                         it: every group of 4 belongs to exactly one thread of the grid.  Every
//                         later pass reads what was stored and forms nothing again.
//   store(nd, a, pos, i, c)
//                         element i, selected, goes to slot pos; the thread owns element i
// The members take the node record and the Args BY VALUE.  Taken by reference, the record's
// address escapes until the members are inlined, the compiler no longer sees that the rows it
// names are global memory, and the kernels address them with flat instead of global instructions
// (measured on MI355X: the STC compaction 9 % slower at 96 x 11 M).
#pragma once
#include <algorithm>

#include "dpz_common.h"
#include "dpz_topk.h"

namespace dpz {

struct NodeWs {  // one node's share of the workspace
  size_t ctrl, hist, bgt, beq, boff, beqb, total;
  int64_t nblk;
};

static inline NodeWs node_ws(int64_t n) {
  NodeWs L;
  L.nblk = std::max<int64_t>(1, (n + EX_CHUNK - 1) / EX_CHUNK);
  size_t o = 0;
  L.ctrl = o; o += align256(sizeof(TopkCtrl));
  L.hist = o; o += align256(4096 * 4);
  L.bgt = o; o += align256((size_t)L.nblk * 4);
  L.beq = o; o += align256((size_t)L.nblk * 4);
  L.boff = o; o += align256((size_t)L.nblk * 4);
  L.beqb = o; o += align256((size_t)L.nblk * 4);
  L.total = o;
  return L;
}

template <class A>
struct SelectArgs {
  A p;  // the engine's
  char* ws;
  NodeWs L;
  int64_t n;
};

__device__ __forceinline__ int count4(int64_t i0, int64_t n) {
  const int64_t rem = n - i0;
  return rem >= 4 ? 4 : (rem > 0 ? (int)rem : 0);
}

// c = r's 4 elements from i0 (zeros past n); returns how many lie inside
__device__ __forceinline__ int load_c4(const float* __restrict__ r, int64_t i0, int64_t n,
                                       bool vec, float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 q = *reinterpret_cast<const float4*>(r + i0);
    c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = e < cnt ? r[i0 + e] : 0.0f;
  }
  return cnt;
}

// key > T in the low half, key == T in the high half: a chunk holds 8192 < 2^16 elements
__device__ __forceinline__ uint32_t count_gt_eq(const float c[4], int cnt, uint32_t T) {
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < cnt) {
      const uint32_t kk = key_of(c[e]);
      v += (kk > T ? 1u : 0u) + (kk == T ? 0x10000u : 0u);
    }
  }
  return v;
}
static_assert(EX_CHUNK < 0x10000, "two 16-bit counts per chunk");

// The threshold and the ties at it to take, as count / scan / write use them.  All ties: key >=
// max(T, 1) is key > max(T, 1) - 1 with no ties taken (T == 0: fewer than k nonzeros, the zeros
// stay home).
template <class P>
__device__ __forceinline__ void select_rule(const TopkCtrl* ctrl, uint32_t& T, uint32_t& ties) {
  T = ctrl->prefix;
  ties = ctrl->krem;
  if constexpr (P::kAllTies) {
    T = (T ? T : 1u) - 1u;
    ties = 0;
  }
}

template <class P, int PASS>
__global__ void __launch_bounds__(256) select_hist_kernel(const SelectArgs<typename P::Args> a) {
  constexpr int NB = (PASS == 1) ? 2048 : 1024;
  constexpr int HOFF = (PASS == 0) ? 0 : (PASS == 1 ? 1024 : 3072);
  __shared__ uint32_t h[NB];
  const typename P::Node nd = a.p.tab[blockIdx.y];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) {  // uniform over the block, before any barrier
      if (PASS == 0) P::idle_share(nd, a.n);
      return;
    }
  }
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0;
  __syncthreads();
  char* ws = a.ws + (size_t)blockIdx.y * a.L.total;
  const uint32_t pfx =
      (PASS == 0) ? 0u : reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->prefix;
  uint32_t* ghist = reinterpret_cast<uint32_t*>(ws + a.L.hist) + HOFF;
  const bool vec = P::template vec<PASS == 0>(nd, a.p);
  const int64_t ngroups = (a.n + 3) >> 2;
  // every group of 4 belongs to exactly one thread of the grid: a key is formed and stored once
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    float c[4];
    const int cnt = P::template load4<PASS == 0>(nd, a.p, g * 4, a.n, vec, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t kk = key_of(c[e]);
        if (PASS == 0) {
          atomicAdd(&h[kk >> 21], 1u);
        } else if (PASS == 1) {
          if ((kk >> 21) == (pfx >> 21)) atomicAdd(&h[(kk >> 10) & 2047u], 1u);
        } else {
          if ((kk >> 10) == (pfx >> 10)) atomicAdd(&h[kk & 1023u], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += 256) {
    const uint32_t v = h[b];
    if (v) atomicAdd(&ghist[b], v);
  }
}

// One block of 1024 threads per node: the digit that holds the krem-th largest key.
template <class P, int PASS>
__global__ void __launch_bounds__(1024)
    select_resolve_kernel(const SelectArgs<typename P::Args> a) {
  constexpr int NB = (PASS == 1) ? 2048 : 1024;
  constexpr int HOFF = (PASS == 0) ? 0 : (PASS == 1 ? 1024 : 3072);
  constexpr int SH = (PASS == 0) ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int PER = NB / 1024;
  __shared__ uint32_t wsum[16];
  const typename P::Node nd = a.p.tab[blockIdx.x];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) return;  // uniform over the block
  }
  char* ws = a.ws + (size_t)blockIdx.x * a.L.total;
  TopkCtrl* ctrl = reinterpret_cast<TopkCtrl*>(ws + a.L.ctrl);
  const uint32_t* ghist = reinterpret_cast<const uint32_t*>(ws + a.L.hist) + HOFF;
  const uint32_t krem = (PASS == 0) ? P::k(nd, a.p, a.n) : ctrl->krem;
  const uint32_t pfx = (PASS == 0) ? 0u : ctrl->prefix;
  __syncthreads();  // every thread has read ctrl before one of them rewrites it
  uint32_t hv[PER];
  uint32_t local = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {  // descending bins
    hv[q] = ghist[NB - 1 - (threadIdx.x * PER + q)];
    local += hv[q];
  }
  uint32_t tot;
  uint32_t before = block_excl_scan(local, wsum, &tot);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (before < krem && krem <= before + hv[q]) {
      const uint32_t d = NB - 1 - (threadIdx.x * PER + q);
      ctrl->prefix = pfx | (d << SH);
      ctrl->krem = krem - before;  // after the last pass: the ties at T to take
    }
    before += hv[q];
  }
}

template <class P>
__global__ void __launch_bounds__(256) select_count_kernel(const SelectArgs<typename P::Args> a) {
  __shared__ uint32_t wsum[16];
  const typename P::Node nd = a.p.tab[blockIdx.y];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) return;  // uniform over the block
  }
  char* ws = a.ws + (size_t)blockIdx.y * a.L.total;
  uint32_t T, ties;
  select_rule<P>(reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl), T, ties);
  const bool vec = P::template vec<false>(nd, a.p);
  const int64_t lo = (int64_t)blockIdx.x * EX_CHUNK;
  uint32_t v = 0;
  for (int r = 0; r < EX_CHUNK / 1024; ++r) {
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    if (i0 >= a.n) break;
    float c[4];
    const int cnt = P::template load4<false>(nd, a.p, i0, a.n, vec, c);
    v += count_gt_eq(c, cnt, T);
  }
  uint32_t tot;
  block_excl_scan(v, wsum, &tot);
  if (threadIdx.x == 0) {
    reinterpret_cast<uint32_t*>(ws + a.L.bgt)[blockIdx.x] = tot & 0xFFFFu;
    reinterpret_cast<uint32_t*>(ws + a.L.beq)[blockIdx.x] = tot >> 16;
  }
}

// One block of 1024 threads per node: every chunk's output offset and the ties before it (its
// share of the allotment follows: ties go to the lowest indices), and the engine's row header.
template <class P>
__global__ void __launch_bounds__(1024) select_scan_kernel(const SelectArgs<typename P::Args> a) {
  __shared__ uint64_t wsum[16];
  const typename P::Node nd = a.p.tab[blockIdx.x];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) return;  // uniform over the block
  }
  char* ws = a.ws + (size_t)blockIdx.x * a.L.total;
  uint32_t T, ties32;
  select_rule<P>(reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl), T, ties32);
  const uint64_t ties = ties32;
  const uint32_t* bgt = reinterpret_cast<const uint32_t*>(ws + a.L.bgt);
  const uint32_t* beq = reinterpret_cast<const uint32_t*>(ws + a.L.beq);
  uint32_t* boff = reinterpret_cast<uint32_t*>(ws + a.L.boff);
  uint32_t* beqb = reinterpret_cast<uint32_t*>(ws + a.L.beqb);
  uint64_t carry_eq = 0, carry_off = 0;
  for (int64_t base = 0; base < a.L.nblk; base += 1024) {
    const int64_t b = base + threadIdx.x;
    const uint64_t gt = b < a.L.nblk ? bgt[b] : 0;
    const uint64_t eq = b < a.L.nblk ? beq[b] : 0;
    uint64_t te;
    const uint64_t eqb = block_excl_scan64(eq, wsum, &te) + carry_eq;
    uint64_t take = 0;
    if (ties > eqb) take = (ties - eqb) < eq ? (ties - eqb) : eq;
    uint64_t ts;
    const uint64_t off = block_excl_scan64(gt + take, wsum, &ts) + carry_off;
    if (b < a.L.nblk) {
      boff[b] = (uint32_t)off;
      beqb[b] = (uint32_t)(eqb < ties ? eqb : ties);
    }
    carry_eq += te;
    carry_off += ts;
  }
  if constexpr (P::kHeader) {
    if (threadIdx.x == 0) P::header(nd, a.p, carry_off);
  }
}

template <class P>
__global__ void __launch_bounds__(256) select_write_kernel(const SelectArgs<typename P::Args> a) {
  __shared__ uint32_t wsum[16];
  const typename P::Node nd = a.p.tab[blockIdx.y];
  if constexpr (P::kIdleNodes) {
    if (P::idle(nd)) return;  // uniform over the block
  }
  const uint32_t slots = P::slots(nd, a.p, a.n);
  char* ws = a.ws + (size_t)blockIdx.y * a.L.total;
  uint32_t T, ties;
  select_rule<P>(reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl), T, ties);
  const uint32_t off0 = reinterpret_cast<const uint32_t*>(ws + a.L.boff)[blockIdx.x];
  const uint32_t eqb = reinterpret_cast<const uint32_t*>(ws + a.L.beqb)[blockIdx.x];
  const uint32_t quota = ties > eqb ? ties - eqb : 0u;
  const bool vec = P::template vec<false>(nd, a.p);
  const int64_t lo = (int64_t)blockIdx.x * EX_CHUNK;
  uint32_t gt_run = 0, eq_run = 0;
  for (int r = 0; r < EX_CHUNK / 1024; ++r) {
    if (lo + r * 1024 >= a.n) break;  // uniform
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    float c[4];
    const int cnt = P::template load4<false>(nd, a.p, i0, a.n, vec, c);
    uint32_t tot;
    const uint32_t ex = block_excl_scan(count_gt_eq(c, cnt, T), wsum, &tot);
    uint32_t g = gt_run + (ex & 0xFFFFu);
    uint32_t q = eq_run + (ex >> 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t kk = key_of(c[e]);
        bool sel = false;
        uint32_t pos = 0;
        if (kk > T) {
          sel = true;
          pos = off0 + g + (q < quota ? q : quota);
          ++g;
        } else if (kk == T) {
          if (q < quota) {
            sel = true;
            pos = off0 + g + q;
          }
          ++q;
        }
        // exactly k: pos < k always; all ties: what is past the slots is reported, never written
        if (sel && pos < slots) P::store(nd, a.p, pos, i0 + e, c[e]);
      }
    }
    gt_run += tot & 0xFFFFu;
    eq_run += tot >> 16;
  }
}

// The selection of m nodes on the stream: ws holds m * node_ws(n).total bytes.
template <class P, class First = P>
int select_nodes(int m, const typename P::Args& args, int64_t n, void* ws, hipStream_t st) {
  SelectArgs<typename P::Args> a;
  a.p = args;
  a.ws = static_cast<char*>(ws);
  a.L = node_ws(n);
  a.n = n;
  // every node's control block and histograms (the chunk arrays are written before they are read)
  DPZ_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)m * a.L.total, st));
  const int64_t groups = (n + 3) / 4;
  const unsigned hb = (unsigned)std::min<int64_t>(EX_HIST_BLOCKS, (groups + 255) / 256);
  const dim3 hgrid(hb, (unsigned)m), cgrid((unsigned)a.L.nblk, (unsigned)m);
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, select_hist_kernel<First, 0><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, select_resolve_kernel<P, 0><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, select_hist_kernel<P, 1><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, select_resolve_kernel<P, 1><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, select_hist_kernel<P, 2><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, select_resolve_kernel<P, 2><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_COUNT, st, select_count_kernel<P><<<cgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_SCAN, st, select_scan_kernel<P><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_WRITE, st, select_write_kernel<P><<<cgrid, 256, 0, st>>>(a));
  return DPZ_OK;
}

}  // namespace dpz
