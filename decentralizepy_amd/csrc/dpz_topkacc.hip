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
#include "dpz_topkacc_policy.h"

namespace {

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
