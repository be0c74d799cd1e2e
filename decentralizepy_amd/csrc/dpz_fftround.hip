// The selection of a batched FFT round (decentralizepy_amd/gossip_fft.py; reference
// sharing/JWINS/FFT.py:132-211 `apply_fft` + `serialized_model` over
// sharing/PartialModel.py:305-331 `_pre_step` on complex coefficients, models/Model.py:53-64).
//
// dpz_cplx_encode_nodes: the exact top-k of |c| over the M complex coefficients of m nodes, the
// node in the grid's second dimension, one k and one DPZ_ACC_* mode per call.  A self-contained
// sibling of dpz_jwins_encode_nodes (a control block, histograms and chunk counts per node; one
// memset and nine launches whatever m is).  Per node, change = F(x - x0):
//   the first histogram pass does cplx_key_kernel's accumulation step (NONE: c = change;
//   ACCUMULATE: acc += change, c = acc; ADD: c = change + acc, acc untouched), stores
//   key[i] = sqrtf(re re + im im) (every product and sum rounded on its own, the square root
//   correctly rounded) into the node's fp32 key row and counts its top 10 bits.  Every later pass
//   reads the key row alone (4 M bytes).  Three histogram passes (10/11/10 bits of the key), each
//   followed by a 1-block-per-node resolve, give T, the k-th largest key, and the number of ties
//   at T to take; a count pass, a 1-block-per-node scan and the ordered compaction write, per
//   selected coefficient i ascending, pair_out = (2 i, 2 i + 1) (the float-pair entries the fold
//   over the (re, im) view reads), val_out = vals_src[i], counter[i] += 1 (a plain store: the
//   element has one owner) and (+0, +0) into acc[i] when the node has an accumulator.  Exactly k
//   entries; ties at T go to the lowest indices.
// No float atomics; the result does not depend on the grid.  Finite inputs only.
#include <algorithm>

#include "dpz_common.h"
#include "dpz_topk.h"

namespace {

using dpz::aligned16;
using dpz::block_excl_scan;
using dpz::block_excl_scan64;
using dpz::key_of;
using dpz::TopkCtrl;

constexpr int64_t MAX_ELEMS = int64_t(1) << 30;  // 2 i + 1 stays an int32
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes
constexpr int HIST_BLOCKS = dpz::EX_HIST_BLOCKS;

struct CxNode {  // 8 64-bit words of the node table
  const float2* change;  // F(x - x0)
  float2* acc;           // or NULL (DPZ_ACC_NONE)
  const float2* vals;    // the payload's value source, F(x)
  float* key;            // M fp32: scratch
  int32_t* counter;      // or NULL
  int2* pair_out;        // k pairs
  float2* val_out;       // k complex
  uint64_t pad;
};
static_assert(sizeof(CxNode) == 64, "8 64-bit words");

struct EncWs {  // one node's share of the workspace
  size_t ctrl, hist, bgt, beq, boff, beqb, total;
  int64_t nblk;
};

EncWs enc_ws(int64_t n) {
  EncWs L;
  L.nblk = std::max<int64_t>(1, (n + CHUNK - 1) / CHUNK);
  size_t o = 0;
  L.ctrl = o; o += dpz::align256(sizeof(TopkCtrl));
  L.hist = o; o += dpz::align256(4096 * 4);
  L.bgt = o; o += dpz::align256((size_t)L.nblk * 4);
  L.beq = o; o += dpz::align256((size_t)L.nblk * 4);
  L.boff = o; o += dpz::align256((size_t)L.nblk * 4);
  L.beqb = o; o += dpz::align256((size_t)L.nblk * 4);
  L.total = o;
  return L;
}

struct EncArgs {
  const CxNode* tab;
  char* ws;
  size_t per_node;
  EncWs L;
  int64_t n;   // M, the coefficients of a node
  uint32_t k;  // 1 <= k <= n
};

__device__ __forceinline__ int count4(int64_t i0, int64_t n) {
  const int64_t rem = n - i0;
  return rem >= 4 ? 4 : (rem > 0 ? (int)rem : 0);
}

// c = the key row's 4 elements from i0 (zeros past n); returns how many lie inside
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

// the keys of the 4 coefficients from i0 after the accumulation step, stored into the key row:
// cplx_key_kernel's arithmetic, element by element
template <int MODE>
__device__ __forceinline__ int form_c4(const CxNode& nd, int64_t i0, int64_t n, float c[4]) {
  const int cnt = count4(i0, n);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c[e] = 0.0f;
    if (e < cnt) {
      float2 v = nd.change[i0 + e];
      if (MODE == DPZ_ACC_ACCUMULATE) {
        float2 a = nd.acc[i0 + e];
        a.x = a.x + v.x;
        a.y = a.y + v.y;
        nd.acc[i0 + e] = a;
        v = a;
      } else if (MODE == DPZ_ACC_ADD) {
        const float2 a = nd.acc[i0 + e];
        v.x = v.x + a.x;
        v.y = v.y + a.y;
      }
      const float re2 = v.x * v.x;
      const float im2 = v.y * v.y;
      c[e] = sqrtf(re2 + im2);  // correctly rounded (llvm.sqrt without afn)
      nd.key[i0 + e] = c[e];
    }
  }
  return cnt;
}

// P = 0 forms the keys (MODE); P = 1, 2 read them
template <int P, int MODE>
__global__ void __launch_bounds__(256) cplx_hist_kernel(const EncArgs a) {
  constexpr int NB = (P == 1) ? 2048 : 1024;
  constexpr int HOFF = (P == 0) ? 0 : (P == 1 ? 1024 : 3072);
  __shared__ uint32_t h[NB];
  const CxNode nd = a.tab[blockIdx.y];
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0;
  __syncthreads();
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const uint32_t pfx = (P == 0) ? 0u : reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->prefix;
  uint32_t* ghist = reinterpret_cast<uint32_t*>(ws + a.L.hist) + HOFF;
  const bool vec = aligned16(nd.key);
  const int64_t ngroups = (a.n + 3) >> 2;
  // every group of 4 belongs to exactly one thread of the grid: the key is formed and stored once
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    float c[4];
    const int cnt = (P == 0) ? form_c4<MODE>(nd, g * 4, a.n, c) : load_c4(nd.key, g * 4, a.n, vec, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t kk = key_of(c[e]);
        if (P == 0) {
          atomicAdd(&h[kk >> 21], 1u);
        } else if (P == 1) {
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
template <int P>
__global__ void __launch_bounds__(1024) cplx_resolve_kernel(const EncArgs a) {
  constexpr int NB = (P == 1) ? 2048 : 1024;
  constexpr int HOFF = (P == 0) ? 0 : (P == 1 ? 1024 : 3072);
  constexpr int SH = (P == 0) ? 21 : (P == 1 ? 10 : 0);
  constexpr int PER = NB / 1024;
  __shared__ uint32_t wsum[16];
  char* ws = a.ws + (size_t)blockIdx.x * a.per_node;
  TopkCtrl* ctrl = reinterpret_cast<TopkCtrl*>(ws + a.L.ctrl);
  const uint32_t* ghist = reinterpret_cast<const uint32_t*>(ws + a.L.hist) + HOFF;
  const uint32_t krem = (P == 0) ? a.k : ctrl->krem;
  const uint32_t pfx = (P == 0) ? 0u : ctrl->prefix;
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
static_assert(CHUNK < 0x10000, "two 16-bit counts per chunk");

__global__ void __launch_bounds__(256) cplx_count_kernel(const EncArgs a) {
  __shared__ uint32_t wsum[16];
  const CxNode nd = a.tab[blockIdx.y];
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const uint32_t T = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->prefix;
  const bool vec = aligned16(nd.key);
  const int64_t lo = (int64_t)blockIdx.x * CHUNK;
  uint32_t v = 0;
  for (int r = 0; r < CHUNK / 1024; ++r) {
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    if (i0 >= a.n) break;
    float c[4];
    const int cnt = load_c4(nd.key, i0, a.n, vec, c);
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
// share of the allotment follows: ties go to the lowest indices).
__global__ void __launch_bounds__(1024) cplx_scan_kernel(const EncArgs a) {
  __shared__ uint64_t wsum[16];
  char* ws = a.ws + (size_t)blockIdx.x * a.per_node;
  const uint64_t ties = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->krem;
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
}

__global__ void __launch_bounds__(256) cplx_write_kernel(const EncArgs a) {
  __shared__ uint32_t wsum[16];
  const CxNode nd = a.tab[blockIdx.y];
  const uint32_t k = a.k;
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const TopkCtrl* ctrl = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl);
  const uint32_t T = ctrl->prefix;
  const uint32_t ties = ctrl->krem;
  const uint32_t off0 = reinterpret_cast<const uint32_t*>(ws + a.L.boff)[blockIdx.x];
  const uint32_t eqb = reinterpret_cast<const uint32_t*>(ws + a.L.beqb)[blockIdx.x];
  const uint32_t quota = ties > eqb ? ties - eqb : 0u;
  const bool vec = aligned16(nd.key);
  const int64_t lo = (int64_t)blockIdx.x * CHUNK;
  uint32_t gt_run = 0, eq_run = 0;
  for (int r = 0; r < CHUNK / 1024; ++r) {
    if (lo + r * 1024 >= a.n) break;  // uniform
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    float c[4];
    const int cnt = load_c4(nd.key, i0, a.n, vec, c);
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
        if (sel && pos < k) {  // pos < k always; the slot is never written past
          const int64_t i = i0 + e;  // this thread owns coefficient i: plain stores
          nd.pair_out[pos] = make_int2((int32_t)(2 * i), (int32_t)(2 * i + 1));
          nd.val_out[pos] = nd.vals[i];
          if (nd.counter) nd.counter[i] = nd.counter[i] + 1;
          if (nd.acc) nd.acc[i] = make_float2(0.0f, 0.0f);  // the rewind (Model.py:53-64)
        }
      }
    }
    gt_run += tot & 0xFFFFu;
    eq_run += tot >> 16;
  }
}

}  // namespace

extern "C" int64_t dpz_cplx_chunk_elems(void) { return CHUNK; }

extern "C" size_t dpz_cplx_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * enc_ws(n).total;
}

extern "C" int dpz_cplx_encode_nodes(int m, const void* node_table, int64_t n, int64_t k,
                                     int acc_mode, void* ws, size_t ws_bytes,
                                     dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS || k < 1 || k > n) return DPZ_ERR_ARG;
  if (acc_mode != DPZ_ACC_NONE && acc_mode != DPZ_ACC_ACCUMULATE && acc_mode != DPZ_ACC_ADD)
    return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 3u))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_cplx_encode_workspace_bytes(m, n)) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  EncArgs a;
  a.tab = static_cast<const CxNode*>(node_table);
  a.ws = static_cast<char*>(ws);
  a.L = enc_ws(n);
  a.per_node = a.L.total;
  a.n = n;
  a.k = (uint32_t)k;
  // every node's control block and histograms (the chunk arrays are written before they are read)
  DPZ_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)m * a.per_node, st));
  const int64_t groups = (n + 3) / 4;
  const unsigned hb = (unsigned)std::min<int64_t>(HIST_BLOCKS, (groups + 255) / 256);
  const dim3 hgrid(hb, (unsigned)m), cgrid((unsigned)a.L.nblk, (unsigned)m);
  switch (acc_mode) {
    case DPZ_ACC_ACCUMULATE:
      DPZ_TIMED(DPZ_KT_EXACT_HIST, st, cplx_hist_kernel<0, DPZ_ACC_ACCUMULATE><<<hgrid, 256, 0, st>>>(a));
      break;
    case DPZ_ACC_ADD:
      DPZ_TIMED(DPZ_KT_EXACT_HIST, st, cplx_hist_kernel<0, DPZ_ACC_ADD><<<hgrid, 256, 0, st>>>(a));
      break;
    default:
      DPZ_TIMED(DPZ_KT_EXACT_HIST, st, cplx_hist_kernel<0, DPZ_ACC_NONE><<<hgrid, 256, 0, st>>>(a));
  }
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, cplx_resolve_kernel<0><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, cplx_hist_kernel<1, DPZ_ACC_NONE><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, cplx_resolve_kernel<1><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, cplx_hist_kernel<2, DPZ_ACC_NONE><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, cplx_resolve_kernel<2><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_COUNT, st, cplx_count_kernel<<<cgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_SCAN, st, cplx_scan_kernel<<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_WRITE, st, cplx_write_kernel<<<cgrid, 256, 0, st>>>(a));
  return DPZ_OK;
}
