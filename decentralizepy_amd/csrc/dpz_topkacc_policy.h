// AccNode, AccArgs and AccPolicy: the selection policy of the top-k round with accumulated changes,
// shared by dpz_topkacc.hip (the exact selection, the post step) and dpz_topkacc_window.hip (the
// windowed selection).  See dpz_topkacc.hip for the semantics.
#pragma once
#include "dpz_common.h"
#include "dpz_select_nodes.h"

namespace {

using dpz::aligned16;
using dpz::count4;
using dpz::load_c4;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int HEADER = 4;                 // int32 words in front of a row's idx / val slots
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes
constexpr int POST_BLOCKS = 1024;

__host__ __device__ __forceinline__ int64_t up4(int64_t v) { return (v + 3) & ~int64_t(3); }

struct AccNode {  // 6 64-bit words of the node table
  const float* x;
  const float* x0;
  float* acc;
  float* key;        // DPZ_ACC_ADD: n floats of scratch; DPZ_ACC_ACCUMULATE: unused (acc is the row)
  int32_t* counter;  // or NULL
  int32_t* row;      // [count lo, count hi, status, 0 | up4(k) idx | up4(k) val]
};
static_assert(sizeof(AccNode) == 48, "6 64-bit words");

struct AccArgs {
  const AccNode* tab;
  uint32_t k;
  int64_t cap;
  int add;  // DPZ_ACC_ADD: the key row is nd.key; else acc
};

// c = fl(acc + fl(x - x0)) of the 4 elements from i0, stored into the key row
__device__ __forceinline__ int form_c4(const AccNode nd, float* __restrict__ kr, int64_t i0,
                                       int64_t n, bool vec, float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(nd.x + i0);
    const float4 b = *reinterpret_cast<const float4*>(nd.x0 + i0);
    const float4 q = *reinterpret_cast<const float4*>(nd.acc + i0);
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    c[0] = q.x + d0, c[1] = q.y + d1, c[2] = q.z + d2, c[3] = q.w + d3;
    *reinterpret_cast<float4*>(kr + i0) = make_float4(c[0], c[1], c[2], c[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[e] = 0.0f;
      if (e < cnt) {
        const float d = nd.x[i0 + e] - nd.x0[i0 + e];
        c[e] = nd.acc[i0 + e] + d;
        kr[i0 + e] = c[e];
      }
    }
  }
  return cnt;
}

struct AccPolicy {  // dpz_select_nodes.h
  using Node = AccNode;
  using Args = AccArgs;
  static constexpr bool kAllTies = false, kIdleNodes = false, kHeader = true;
  static __device__ __forceinline__ float* key_row(const Node nd, const Args a) {
    return a.add ? nd.key : nd.acc;
  }
  static __device__ __forceinline__ uint32_t k(const Node, const Args a, int64_t) { return a.k; }
  static __device__ __forceinline__ uint32_t slots(const Node, const Args a, int64_t) {
    return a.k;
  }
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const Node nd, const Args a) {
    return aligned16(key_row(nd, a)) &&
           (!FIRST || (aligned16(nd.x) && aligned16(nd.x0) && aligned16(nd.acc)));
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const Node nd, const Args a, int64_t i0,
                                              int64_t n, bool vec, float c[4]) {
    float* kr = key_row(nd, a);
    return FIRST ? form_c4(nd, kr, i0, n, vec, c) : load_c4(kr, i0, n, vec, c);
  }
  // dpz_select_window_nodes.h: one k, one prior slot; load4<true> of a whole aligned group, split
  // at the loads' use
  static __device__ __forceinline__ uint32_t kslot(const Node, const Args) { return 0; }
  struct Raw {
    float4 a, b, q;
  };
  static __device__ __forceinline__ void raw4(const Node nd, const Args, int64_t i0, Raw& r) {
    r.a = *reinterpret_cast<const float4*>(nd.x + i0);
    r.b = *reinterpret_cast<const float4*>(nd.x0 + i0);
    r.q = *reinterpret_cast<const float4*>(nd.acc + i0);
  }
  static __device__ __forceinline__ void form4(const Node nd, const Args a, int64_t i0,
                                               const Raw& r, float c[4]) {
    const float d0 = r.a.x - r.b.x, d1 = r.a.y - r.b.y, d2 = r.a.z - r.b.z, d3 = r.a.w - r.b.w;
    c[0] = r.q.x + d0, c[1] = r.q.y + d1, c[2] = r.q.z + d2, c[3] = r.q.w + d3;
    *reinterpret_cast<float4*>(key_row(nd, a) + i0) = make_float4(c[0], c[1], c[2], c[3]);
  }
  // exactly k are selected; k < 2^31: the int64's high word is 0
  static __device__ __forceinline__ void header(const Node nd, const Args a, uint64_t) {
    nd.row[0] = (int32_t)a.k;
    nd.row[1] = 0;
    nd.row[2] = 0;
    nd.row[3] = 0;
  }
  // this thread owns element i: plain stores
  static __device__ __forceinline__ void store(const Node nd, const Args a, uint32_t pos,
                                               int64_t i, float) {
    nd.row[HEADER + pos] = (int32_t)i;
    reinterpret_cast<float*>(nd.row + HEADER + a.cap)[pos] = nd.x[i];
    if (nd.counter) nd.counter[i] = nd.counter[i] + 1;
    nd.acc[i] = 0.0f;  // the rewind: what was sent is no longer owed
  }
};

}  // namespace
