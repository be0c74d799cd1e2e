// dpz_topkacc_encode_nodes_window: dpz_topkacc_encode_nodes (dpz_topkacc.hip) with the windowed
// one-read selection of dpz_select_window_nodes.h under the same AccPolicy.
#include "dpz_select_window_nodes.h"
#include "dpz_topkacc_policy.h"

extern "C" size_t dpz_topkacc_encode_window_workspace_bytes(int m, int64_t n, int64_t k) {
  if (m < 1 || n < 1 || k < 1 || k > n) return 0;
  return dpz::win_ws(m, n, k).total;
}

extern "C" int dpz_topkacc_encode_nodes_window(int m, const void* node_table, int64_t n,
                                               int64_t k, int mode, void* ws, size_t ws_bytes,
                                               dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS || k < 1 || k > n) return DPZ_ERR_ARG;
  if (mode != DPZ_ACC_ACCUMULATE && mode != DPZ_ACC_ADD) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 255u))
    return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_topkacc_encode_window_workspace_bytes(m, n, k)) return DPZ_ERR_WORKSPACE;
  AccArgs a;
  a.tab = static_cast<const AccNode*>(node_table);
  a.k = (uint32_t)k;
  a.cap = up4(k);
  a.add = mode == DPZ_ACC_ADD;
  return dpz::select_window_nodes<AccPolicy>(m, a, n, k, ws, static_cast<hipStream_t>(stream));
}
