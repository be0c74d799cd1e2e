// The selection of a batched FFT round (decentralizepy_amd/gossip_fft.py; reference
// sharing/JWINS/FFT.py:132-211 `apply_fft` + `serialized_model` over
// sharing/PartialModel.py:305-331 `_pre_step` on complex coefficients, models/Model.py:53-64).
//
// dpz_cplx_encode_nodes: the exact top-k of |c| over the M complex coefficients of m nodes, the
// one k and one DPZ_ACC_* mode per call: the selection of dpz_select_nodes.h under CxPolicy.  Per
// node, change = F(x - x0):
//   the first histogram pass does cplx_key_kernel's accumulation step (NONE: c = change;
//   ACCUMULATE: acc += change, c = acc; ADD: c = change + acc, acc untouched) and stores
//   key[i] = sqrtf(re re + im im) (every product and sum rounded on its own, the square root
//   correctly rounded) into the node's fp32 key row.  Every later pass reads the key row alone
//   (4 M bytes).  The compaction writes, per selected coefficient i ascending,
//   pair_out = (2 i, 2 i + 1) (the float-pair entries the fold over the (re, im) view reads),
//   val_out = vals_src[i], counter[i] += 1 (a plain store: the element has one owner) and
//   (+0, +0) into acc[i] when the node has an accumulator.  Exactly k entries; ties at the k-th
//   largest key go to the lowest indices.
// No float atomics; the result does not depend on the grid.  Finite inputs only.
#include <algorithm>

#include "dpz_common.h"
#include "dpz_select_nodes.h"

namespace {

using dpz::aligned16;
using dpz::count4;
using dpz::load_c4;

constexpr int64_t MAX_ELEMS = int64_t(1) << 30;  // 2 i + 1 stays an int32
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes

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

struct CxArgs {
  const CxNode* tab;
  uint32_t k;  // 1 <= k <= n, n = M, the coefficients of a node
};

// the keys of the 4 coefficients from i0 after the accumulation step, stored into the key row:
// cplx_key_kernel's arithmetic, element by element
template <int MODE>
__device__ __forceinline__ int form_c4(const CxNode nd, int64_t i0, int64_t n, float c[4]) {
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

// MODE: the first histogram pass's; every other kernel is CxPolicy<DPZ_ACC_NONE>'s
template <int MODE>
struct CxPolicy {  // dpz_select_nodes.h
  using Node = CxNode;
  using Args = CxArgs;
  static constexpr bool kAllTies = false, kIdleNodes = false, kHeader = false;
  static __device__ __forceinline__ uint32_t k(const Node, const Args a, int64_t) { return a.k; }
  static __device__ __forceinline__ uint32_t slots(const Node, const Args a, int64_t) {
    return a.k;
  }
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const Node nd, const Args) {
    return aligned16(nd.key);
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const Node nd, const Args, int64_t i0, int64_t n,
                                              bool vec, float c[4]) {
    return FIRST ? form_c4<MODE>(nd, i0, n, c) : load_c4(nd.key, i0, n, vec, c);
  }
  // this thread owns coefficient i: plain stores
  static __device__ __forceinline__ void store(const Node nd, const Args, uint32_t pos,
                                               int64_t i, float) {
    nd.pair_out[pos] = make_int2((int32_t)(2 * i), (int32_t)(2 * i + 1));
    nd.val_out[pos] = nd.vals[i];
    if (nd.counter) nd.counter[i] = nd.counter[i] + 1;
    if (nd.acc) nd.acc[i] = make_float2(0.0f, 0.0f);  // the rewind (Model.py:53-64)
  }
};
using CxRead = CxPolicy<DPZ_ACC_NONE>;

}  // namespace

extern "C" int64_t dpz_cplx_chunk_elems(void) { return CHUNK; }

extern "C" size_t dpz_cplx_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * dpz::node_ws(n).total;
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
  CxArgs a;
  a.tab = static_cast<const CxNode*>(node_table);
  a.k = (uint32_t)k;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (acc_mode) {
    case DPZ_ACC_ACCUMULATE:
      return dpz::select_nodes<CxRead, CxPolicy<DPZ_ACC_ACCUMULATE>>(m, a, n, ws, st);
    case DPZ_ACC_ADD:
      return dpz::select_nodes<CxRead, CxPolicy<DPZ_ACC_ADD>>(m, a, n, ws, st);
    default:
      return dpz::select_nodes<CxRead, CxRead>(m, a, n, ws, st);
  }
}
