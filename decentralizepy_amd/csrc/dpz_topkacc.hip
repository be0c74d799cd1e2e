// A top-k round with accumulated changes (decentralizepy_amd/gossip_topkacc.py; reference
// sharing/PartialModel.py:305-331 `_pre_step` with accumulation = True, :188-255 the selection,
// the counter and the rewind, :333-353 `_post_step`).
//
// dpz_topkacc_encode_nodes: the exact-k selection of m nodes (dpz_select_nodes.h) under
// AccPolicy.  The first histogram pass forms the key vector c once from x, x0 and acc (12 N bytes
// read) and stores it (4 N written) into the node's key row:
//   DPZ_ACC_ACCUMULATE  c = fl(acc + fl(x - x0)), the key row is acc itself: the reference's
//                       `accumulated_changes += change`, stored in place (every group of 4
//                       elements belongs to exactly one thread of the grid);
//   DPZ_ACC_ADD         c = fl(fl(x - x0) + acc), the key row is a scratch row of the caller's;
//                       acc is not written before the rewind.
// Every later pass reads the key row alone (4 N).  The compaction writes idx / val = x[i]
// ascending into the node's row, counter[i] += 1 (a plain store: the element has one owner) and
// +0 into acc[i].  Exactly k entries per row, ties at the k-th largest key to the lowest indices;
// x and x0 are never written.
//
// dpz_topkacc_post_nodes: `_post_step` with accumulate_averaging_changes of m nodes in one launch
// over the same node table: acc = fl(acc + fl(x - x0)), x the averaged model and x0 the model the
// round started from.
#include <algorithm>

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

// ---- post step ----------------------------------------------------------------------------------
struct PostArgs {
  const AccNode* tab;
  int64_t n;
};

__global__ void __launch_bounds__(256) topkacc_post_kernel(const PostArgs a) {
  const AccNode nd = a.tab[blockIdx.y];
  const bool vec = aligned16(nd.x) && aligned16(nd.x0) && aligned16(nd.acc);
  const int64_t ngroups = (a.n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * 4;
    const int cnt = count4(i0, a.n);
    if (vec && cnt == 4) {
      const float4 x = *reinterpret_cast<const float4*>(nd.x + i0);
      const float4 b = *reinterpret_cast<const float4*>(nd.x0 + i0);
      const float4 q = *reinterpret_cast<const float4*>(nd.acc + i0);
      const float d0 = x.x - b.x, d1 = x.y - b.y, d2 = x.z - b.z, d3 = x.w - b.w;
      *reinterpret_cast<float4*>(nd.acc + i0) =
          make_float4(q.x + d0, q.y + d1, q.z + d2, q.w + d3);
    } else {
      for (int e = 0; e < cnt; ++e) {
        const float d = nd.x[i0 + e] - nd.x0[i0 + e];
        nd.acc[i0 + e] = nd.acc[i0 + e] + d;
      }
    }
  }
}

}  // namespace

extern "C" int64_t dpz_topkacc_chunk_elems(void) { return CHUNK; }

extern "C" size_t dpz_topkacc_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * dpz::node_ws(n).total;
}

extern "C" int dpz_topkacc_encode_nodes(int m, const void* node_table, int64_t n, int64_t k,
                                        int mode, void* ws, size_t ws_bytes,
                                        dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS || k < 1 || k > n) return DPZ_ERR_ARG;
  if (mode != DPZ_ACC_ACCUMULATE && mode != DPZ_ACC_ADD) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 3u))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_topkacc_encode_workspace_bytes(m, n)) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  AccArgs a;
  a.tab = static_cast<const AccNode*>(node_table);
  a.k = (uint32_t)k;
  a.cap = up4(k);
  a.add = mode == DPZ_ACC_ADD;
  return dpz::select_nodes<AccPolicy>(m, a, n, ws, static_cast<hipStream_t>(stream));
}

extern "C" int dpz_topkacc_post_nodes(int m, const void* node_table, int64_t n,
                                      dpz_stream_t stream) {
  if (m < 1 || !node_table || n < 1 || n >= MAX_ELEMS) return DPZ_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(node_table) & 7u) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  PostArgs a;
  a.tab = static_cast<const AccNode*>(node_table);
  a.n = n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t groups = (n + 3) / 4;
  const dim3 grid((unsigned)std::min<int64_t>(POST_BLOCKS, (groups + 255) / 256), (unsigned)m);
  DPZ_TIMED(DPZ_KT_ACCUMULATE, st, topkacc_post_kernel<<<grid, 256, 0, st>>>(a));
  return DPZ_OK;
}
