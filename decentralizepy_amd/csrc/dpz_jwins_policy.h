// JwNode, JwArgs and JwPolicy: the selection policy of the batched JWINS round, shared by
// dpz_jwins.hip (the exact selection) and dpz_jwins_window.hip (the windowed selection).  See
// dpz_jwins.hip for the semantics.
#pragma once
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
  uint64_t slot;       // the windowed selection's prior slot of this k (else unused)
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
  // dpz_select_window_nodes.h: the prior slot of the node's k; load4<true> of a whole aligned
  // group, split at the loads' use
  static __device__ __forceinline__ uint32_t kslot(const Node nd, const Args) {
    return (uint32_t)nd.slot;
  }
  struct Raw {
    float4 a, q;
  };
  static __device__ __forceinline__ void raw4(const Node nd, const Args, int64_t i0, Raw& r) {
    r.a = *reinterpret_cast<const float4*>(nd.c + i0);
    r.q = *reinterpret_cast<const float4*>(nd.acc + i0);
  }
  static __device__ __forceinline__ void form4(const Node nd, const Args, int64_t i0,
                                               const Raw& r, float c[4]) {
    c[0] = r.a.x + r.q.x, c[1] = r.a.y + r.q.y, c[2] = r.a.z + r.q.z, c[3] = r.a.w + r.q.w;
    *reinterpret_cast<float4*>(nd.c + i0) = make_float4(c[0], c[1], c[2], c[3]);
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
