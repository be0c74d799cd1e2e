// dpz_jwins_encode_nodes_window: dpz_jwins_encode_nodes (dpz_jwins.hip) with the windowed one-read
// selection of dpz_select_window_nodes.h under the same JwPolicy.
#include "dpz_jwins_policy.h"
#include "dpz_select_window_nodes.h"

extern "C" int dpz_jwins_window_slots(void) { return dpz::WIN_SLOTS; }

extern "C" size_t dpz_jwins_encode_window_workspace_bytes(int m, int64_t n, int64_t kmax) {
  if (m < 1 || n < 1 || kmax < 1 || kmax > n) return 0;
  return dpz::win_ws(m, n, kmax).total;
}

extern "C" int dpz_jwins_encode_nodes_window(int m, const void* node_table, int64_t n,
                                             int64_t kmax, void* ws, size_t ws_bytes,
                                             dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS || kmax < 1 || kmax > n) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 255u))
    return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_jwins_encode_window_workspace_bytes(m, n, kmax)) return DPZ_ERR_WORKSPACE;
  JwArgs a;
  a.tab = static_cast<const JwNode*>(node_table);
  return dpz::select_window_nodes<JwPolicy>(m, a, n, kmax, ws, static_cast<hipStream_t>(stream));
}
