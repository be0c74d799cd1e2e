// The selection of a batched JWINS round (decentralizepy_amd/gossip_jwins_batch.py; reference
// sharing/JWINS/Wavelet.py:142-231 `apply_wavelet` + `serialized_model` over
// sharing/PartialModel.py:305-331 `_pre_step` with accumulate_averaging_changes).
//
// dpz_jwins_encode_nodes: the exact selection of m nodes (dpz_select_nodes.h) under JwPolicy,
// each node with ITS OWN k (JWINS draws alpha per node and round) and with the values taken from a
// row other than the one the key is formed from.  Per node, c = W(x - x0):
//   1 <= k <= n   the first histogram pass forms the key vector fl(c + acc) once (8 n bytes read)
//                 and stores it IN PLACE into the c row (4 n written): the round has no further
//                 use for W(x - x0), and the fold overwrites the row afterwards.  Every later pass
//                 reads the c row alone (4 n).  The compaction writes idx ascending /
//                 val = vals_src[idx] into the node's slots, counter[idx] += 1 (a plain store: the
//                 element has one owner) and +0 into acc[idx].  Exactly k entries; ties at the
//                 k-th largest key go to the lowest indices.
//   k == 0        a full share (Wavelet.py:185-192): the first pass stores +0 to all of acc and,
//                 if val_out is set, copies vals_src to val_out (n floats).  No other pass
//                 touches the node: its blocks leave at once.
// The resolve, scan and compaction read the node's k from the table.  No float atomics; the
// result does not depend on the grid.  Finite inputs only.
#include <algorithm>

#include "dpz_common.h"
#include "dpz_select_nodes.h"

namespace {

using dpz::aligned16;
using dpz::count4;
using dpz::load_c4;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes

struct JwNode {  // 8 64-bit words of the node table
  float* c;            // W(x - x0); the key vector after the first pass
  float* acc;
  const float* vals;   // the payload's value source, W(x)
  int32_t* counter;    // or NULL
  int32_t* idx_out;    // k entries (unused with k == 0)
  float* val_out;      // k entries; with k == 0: n entries, or NULL for no copy
  uint64_t k;          // 0: a full share
  uint64_t pad;
};
static_assert(sizeof(JwNode) == 64, "8 64-bit words");

struct JwArgs {
  const JwNode* tab;
};

// the node's k; a k past n (the caller's error, refused by the Python wrapper) selects all n, so
// that no pass writes outside the node's rows
__device__ __forceinline__ uint32_t node_k(const JwNode nd, int64_t n) {
  return nd.k > (uint64_t)n ? (uint32_t)n : (uint32_t)nd.k;
}

// key = fl(c + acc) of the 4 elements from i0, stored in place into the c row
__device__ __forceinline__ int form_c4(const JwNode nd, int64_t i0, int64_t n, bool vec,
                                       float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(nd.c + i0);
    const float4 q = *reinterpret_cast<const float4*>(nd.acc + i0);
    c[0] = a.x + q.x, c[1] = a.y + q.y, c[2] = a.z + q.z, c[3] = a.w + q.w;
    *reinterpret_cast<float4*>(nd.c + i0) = make_float4(c[0], c[1], c[2], c[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[e] = 0.0f;
      if (e < cnt) {
        c[e] = nd.c[i0 + e] + nd.acc[i0 + e];
        nd.c[i0 + e] = c[e];
      }
    }
  }
  return cnt;
}

// a full share: acc = +0 everywhere, val_out = vals_src when set
__device__ __forceinline__ void full_share(const JwNode nd, int64_t n) {
  const bool vz = aligned16(nd.acc);
  const bool vc = nd.val_out && aligned16(nd.vals) && aligned16(nd.val_out);
  const int64_t ngroups = (n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * 4;
    const int cnt = count4(i0, n);
    if (vz && cnt == 4) {
      *reinterpret_cast<float4*>(nd.acc + i0) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int e = 0; e < cnt; ++e) nd.acc[i0 + e] = 0.0f;
    }
    if (nd.val_out) {
      if (vc && cnt == 4) {
        *reinterpret_cast<float4*>(nd.val_out + i0) =
            *reinterpret_cast<const float4*>(nd.vals + i0);
      } else {
        for (int e = 0; e < cnt; ++e) nd.val_out[i0 + e] = nd.vals[i0 + e];
      }
    }
  }
}

struct JwPolicy {  // dpz_select_nodes.h; the key row is c
  using Node = JwNode;
  using Args = JwArgs;
  static constexpr bool kAllTies = false, kIdleNodes = true, kHeader = false;
  static __device__ __forceinline__ bool idle(const Node nd) { return nd.k == 0; }
  static __device__ __forceinline__ void idle_share(const Node nd, int64_t n) {
    full_share(nd, n);
  }
  static __device__ __forceinline__ uint32_t k(const Node nd, const Args, int64_t n) {
    return node_k(nd, n);
  }
  static __device__ __forceinline__ uint32_t slots(const Node nd, const Args, int64_t n) {
    return node_k(nd, n);
  }
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const Node nd, const Args) {
    return aligned16(nd.c) && (!FIRST || aligned16(nd.acc));
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const Node nd, const Args, int64_t i0, int64_t n,
                                              bool vec, float c[4]) {
    return FIRST ? form_c4(nd, i0, n, vec, c) : load_c4(nd.c, i0, n, vec, c);
  }
  // this thread owns element i: plain stores
  static __device__ __forceinline__ void store(const Node nd, const Args, uint32_t pos,
                                               int64_t i, float) {
    nd.idx_out[pos] = (int32_t)i;
    nd.val_out[pos] = nd.vals[i];
    if (nd.counter) nd.counter[i] = nd.counter[i] + 1;
    nd.acc[i] = 0.0f;  // the rewind: what was sent is no longer owed
  }
};

}  // namespace

extern "C" int64_t dpz_jwins_chunk_elems(void) { return CHUNK; }

extern "C" size_t dpz_jwins_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * dpz::node_ws(n).total;
}

extern "C" int dpz_jwins_encode_nodes(int m, const void* node_table, int64_t n, void* ws,
                                      size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 3u))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_jwins_encode_workspace_bytes(m, n)) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  JwArgs a;
  a.tab = static_cast<const JwNode*>(node_table);
  return dpz::select_nodes<JwPolicy>(m, a, n, ws, static_cast<hipStream_t>(stream));
}
