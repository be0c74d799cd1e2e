// The quantiser of dpz_quant.hip for a round's nodes at once (decentralizepy_amd/gossip_quant.py):
// the same statistics and pack blocks (dpz_quant.h), the node as the grid's second dimension, two
// launches whatever the node count.  Every node has its own max words and chunk sums in the
// workspace and writes straight into its packed row [count (int64), status, 0 | the info record |
// body]; nothing is read back.
#include "dpz_quant.h"

namespace {

using namespace dpz;

// one node: 2 64-bit words of the table
struct QNode {
  const float* x;
  int32_t* row;
};
static_assert(sizeof(QNode) == 16, "2 64-bit words");

// workspace: m x 256 max words (zeroed before every call), then m x chunks sums
__device__ __forceinline__ float* node_sums(uint32_t* ws, int m, int node, int64_t nchunks) {
  return reinterpret_cast<float*>(ws + (size_t)m * Q_SLOTS) + (size_t)node * nchunks;
}

__global__ void __launch_bounds__(Q_THREADS)
quant_stats_nodes_kernel(const QNode* __restrict__ tab, int64_t n, int m, uint32_t* ws) {
  __shared__ StatsLds s;
  const int node = blockIdx.y;
  const float* x = tab[node].x;
  quant_stats_block(x, n, aligned16(x) ? 1 : 0, ws + (size_t)node * Q_SLOTS,
                    node_sums(ws, m, node, quant_chunks(n)), blockIdx.x, s);
}

__global__ void __launch_bounds__(Q_THREADS)
quant_pack_nodes_kernel(const QNode* __restrict__ tab, int64_t n, int k, int m, uint32_t* ws,
                        int64_t cap_dwords) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Q_PACK_LDS];
  const int node = blockIdx.y;
  const QNode nd = tab[node];
  uint32_t* row = reinterpret_cast<uint32_t*>(nd.row);
  const QuantParams q = quant_pack_body(
      nd.x, n, k, aligned16(nd.x) ? 1 : 0, ws + (size_t)node * Q_SLOTS,
      node_sums(ws, m, node, quant_chunks(n)), row + QROW_BODY, cap_dwords, nd.row + QROW_INFO,
      blockIdx.x, lds);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    row[QROW_COUNT] = (uint32_t)n;  // n < 2^31: the int64 count as two words
    row[QROW_COUNT + 1] = 0u;
    row[QROW_STATUS] = (uint32_t)q.status;
    row[QROW_STATUS + 1] = 0u;
  }
}

}  // namespace

extern "C" size_t dpz_quant_encode_nodes_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1 || n >= Q_NMAX) return 0;
  return (size_t)m * (Q_WS_SUMS + 4 * (size_t)quant_chunks(n));
}

extern "C" int64_t dpz_quant_row_words(int64_t n, int slot_bits) {
  if (n < 1 || n >= Q_NMAX || slot_bits < 2 || slot_bits > 32) return 0;
  return QROW_BODY + (n * slot_bits + 31) / 32;
}

extern "C" int dpz_quant_encode_nodes(int m, const void* node_table, int64_t n, int64_t k,
                                      int slot_bits, void* ws, size_t ws_bytes,
                                      dpz_stream_t stream) {
  if (m < 1 || n < 1 || k < 1 || k > ((int64_t)1 << 30) || slot_bits < 2 || slot_bits > 32)
    return DPZ_ERR_ARG;
  if (!node_table || !ws || (reinterpret_cast<uintptr_t>(ws) & 15u) ||
      (reinterpret_cast<uintptr_t>(node_table) & 7u))
    return DPZ_ERR_ARG;
  if (n >= Q_NMAX || m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_quant_encode_nodes_workspace_bytes(m, n)) return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DPZ_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)m * Q_WS_SUMS, st));
  const QNode* tab = static_cast<const QNode*>(node_table);
  const dim3 sgrid((unsigned)quant_chunks(n), (unsigned)m);
  DPZ_TIMED(DPZ_KT_QUANT_STATS, st,
            quant_stats_nodes_kernel<<<sgrid, Q_THREADS, 0, st>>>(tab, n, m,
                                                                  static_cast<uint32_t*>(ws)));
  const dim3 pgrid((unsigned)((n + Q_SPAN - 1) / Q_SPAN) + 1, (unsigned)m);
  DPZ_TIMED(DPZ_KT_QUANT_PACK, st,
            quant_pack_nodes_kernel<<<pgrid, Q_THREADS, 0, st>>>(
                tab, n, (int)k, m, static_cast<uint32_t*>(ws), (n * slot_bits + 31) / 32));
  return DPZ_OK;
}
