// The quantiser of dpz_quant.hip for the value lists of a sparse round (EliasQuantization over
// PartialModel / Wavelet / JWINS payloads: decentralizepy_amd/gossip_round.py): m lists, each with
// its own count and slot, quantised in two launches and decoded in one, whatever m is.
//
// Encode.  A statistics launch, grid (chunks of the largest count, nodes): a block writes its
// chunk's max|v| bits and pairwise fp32 sum (quant_stats_chunk, dpz_quant.h) to words of its own,
// so nothing is zeroed first and no atomic runs.  A pack launch, grid (1 + spans of the largest
// count, nodes): every block takes the max over its node's chunk words and derives the node's
// parameters (quant_params); block 0 chains the chunk sums and writes the info record
// (quant_info_block); block b > 0 stages the bit-reversed fields of span b - 1 in LDS (16-byte
// loads of a 16-byte aligned list, per-element loads otherwise: decided per node here) and then
// owns WORDS of the stream: a lane assembles one 32-bit word in registers from the at most
// 2 + 32/w fields that touch it and stores it.  Blocks past their node's count exit.
//
// Decode.  One launch, grid (tiles of the largest count, nodes): w and scale come from the row's
// header on the device.  A block owns a tile of SQ_TILE values, which starts on a dword of the
// body; it stages the tile's dwords in LDS (16-byte loads of an aligned body) and every lane
// extracts four consecutive MSB-first fields per step, stored as one 16-byte store where the
// output is aligned.  status[j] is written by the node's first block; a refused node writes
// nothing else and reads only its header.
#include "dpz_quant.h"

namespace {

using namespace dpz;

// one entry of either table: 4 64-bit words
struct SqNode {
  uint64_t a;          // encode: val (fp32)          decode: coded row
  int64_t count;
  uint64_t b;          // encode: out row             decode: out (fp32)
  int64_t slot_words;  // int32 words of the row's slot, the 8 info words included
};
static_assert(sizeof(SqNode) == 32, "4 64-bit words");

constexpr int64_t SQ_NMAX = (int64_t)1 << 30;
constexpr int SQ_TILE = 4096;  // decode: values per block, 4 per lane and step

// workspace: m x C max words, then m x C chunk sums, C = the chunks of the largest count
__device__ __forceinline__ float* sq_sums(uint32_t* ws, int m, int64_t C) {
  return reinterpret_cast<float*>(ws + (size_t)m * C);
}

__global__ void __launch_bounds__(Q_THREADS)
squant_stats_nodes_kernel(const SqNode* __restrict__ tab, int m, int64_t C, uint32_t* ws) {
  __shared__ StatsLds s;
  const int node = blockIdx.y;
  const int64_t n = tab[node].count;
  if ((int64_t)blockIdx.x >= quant_chunks(n)) return;
  const float* x = reinterpret_cast<const float*>(tab[node].a);
  float chunk = 0.0f;
  uint32_t bm = 0;
  quant_stats_chunk(x, n, aligned16(x) ? 1 : 0, blockIdx.x, s, chunk, bm);
  if (threadIdx.x == 0) {
    ws[(size_t)node * C + blockIdx.x] = bm;
    sq_sums(ws, m, C)[(size_t)node * C + blockIdx.x] = chunk;
  }
}

__global__ void __launch_bounds__(Q_THREADS)
squant_pack_nodes_kernel(const SqNode* __restrict__ tab, int m, int k, int64_t C, uint32_t* ws) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Q_PACK_LDS];
  const int node = blockIdx.y, tid = threadIdx.x;
  const SqNode nd = tab[node];
  const int64_t n = nd.count;
  const int64_t spans = (n + Q_SPAN - 1) / Q_SPAN;
  if ((int64_t)blockIdx.x > spans) return;
  // max|v|: over the node's chunk words, then over the block
  const int64_t nch = quant_chunks(n);
  const uint32_t* maxw = ws + (size_t)node * C;
  uint32_t mb = 0;
  for (int64_t c = tid; c < nch; c += Q_THREADS) {
    const uint32_t o = maxw[c];
    mb = o > mb ? o : mb;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_xor(mb, d, 64);
    mb = o > mb ? o : mb;
  }
  if ((tid & 63) == 0) lds[tid >> 6] = mb;
  __syncthreads();
  mb = lds[0];
#pragma unroll
  for (int w = 1; w < Q_THREADS / 64; ++w) mb = lds[w] > mb ? lds[w] : mb;
  __syncthreads();
  const QuantParams q = quant_params(mb, n, k, nd.slot_words - QI_WORDS);
  int32_t* row = reinterpret_cast<int32_t*>(nd.b);
  if (blockIdx.x == 0) {
    quant_info_block(q, n, k, sq_sums(ws, m, C) + (size_t)node * C, row, lds);
    return;
  }
  if (q.status != 0) return;

  // the fields of span b: index e of the span at lds[qpad(e)], zero past the list's end
  const float* x = reinterpret_cast<const float*>(nd.a);
  const int vec = aligned16(x) ? 1 : 0;
  const int w = q.w;
  const int64_t blk = (int64_t)blockIdx.x - 1, base = blk * Q_SPAN;
#pragma unroll
  for (int it = 0; it < Q_SPAN / (4 * Q_THREADS); ++it) {
    const int e = it * 4 * Q_THREADS + 4 * tid;
    const int64_t i = base + e;
    uint32_t f[4] = {0u, 0u, 0u, 0u};
    if (vec && i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(x + i);
      f[0] = quant_field(v.x, q.norm, q.off, w);
      f[1] = quant_field(v.y, q.norm, q.off, w);
      f[2] = quant_field(v.z, q.norm, q.off, w);
      f[3] = quant_field(v.w, q.norm, q.off, w);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (i + c < n) f[c] = quant_field(x[i + c], q.norm, q.off, w);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[qpad(e + c)] = f[c];
  }
  __syncthreads();

  // word d of the span covers its stream bits [32 d, 32 d + 32): the fields floor(32 d / w) ..
  // floor((32 d + 31) / w), the first and the last possibly in part.  The span is a multiple of
  // 32 values, so it starts on a word and its Q_THREADS * w words hold no other span's bits.
  uint32_t* out = reinterpret_cast<uint32_t*>(row + QI_WORDS);
  const int64_t ndw = (n * w + 31) / 32;
  const int64_t gbase = blk * Q_THREADS * w;
  for (int d = tid; d < Q_THREADS * w; d += Q_THREADS) {
    if (gbase + d >= ndw) break;
    const int bit0 = 32 * d;
    const int i0 = bit0 / w;
    int i1 = (bit0 + 31) / w;
    i1 = i1 < Q_SPAN ? i1 : Q_SPAN - 1;
    uint32_t word = 0;
    for (int i = i0; i <= i1; ++i) {
      const int sh = i * w - bit0;  // in (-w, 32)
      const uint32_t f = lds[qpad(i)];
      word |= sh >= 0 ? f << sh : f >> -sh;
    }
    out[gbase + d] = word;
  }
}

__global__ void __launch_bounds__(Q_THREADS)
squant_decode_nodes_kernel(const SqNode* __restrict__ tab, uint32_t* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[SQ_TILE + 4];
  const int node = blockIdx.y, tid = threadIdx.x;
  const SqNode nd = tab[node];
  const int32_t* row = reinterpret_cast<const int32_t*>(nd.a);
  const int64_t n = nd.count, cap = nd.slot_words - QI_WORDS;
  const int hs = row[QI_STATUS], w = row[QI_W];
  const float scale = __int_as_float(row[QI_SCALE]);
  uint32_t bad = 0;
  if (hs != 0)
    bad = (uint32_t)hs;
  else if (w < 2 || w > 32)
    bad = 5;  // no width of the format
  else if ((n * w + 31) / 32 > cap)
    bad = 6;  // the count's bits pass the slot
  if (blockIdx.x == 0 && tid == 0) status[node] = bad;
  const int64_t v0 = (int64_t)blockIdx.x * SQ_TILE;
  if (bad || v0 >= n) return;

  // the tile's dwords: it starts at stream bit v0 * w, a multiple of 32 (of 128 dwords even)
  const uint32_t* body = reinterpret_cast<const uint32_t*>(row + QI_WORDS);
  const int64_t ndw = (n * w + 31) / 32, d0 = v0 / 32 * w;
  const int nd_t = (int)((ndw - d0) < (SQ_TILE / 32) * w ? (ndw - d0) : (SQ_TILE / 32) * w);
  const int vec_in = aligned16(body) ? 1 : 0;
  for (int e = 4 * tid; e < nd_t; e += 4 * Q_THREADS) {
    if (vec_in && e + 3 < nd_t) {
      *reinterpret_cast<uint4*>(lds + e) = *reinterpret_cast<const uint4*>(body + d0 + e);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e + c < nd_t) lds[e + c] = body[d0 + e + c];
    }
  }
  __syncthreads();

  float* out = reinterpret_cast<float*>(nd.b);
  const int vec_out = aligned16(out) ? 1 : 0;
#pragma unroll
  for (int it = 0; it < SQ_TILE / (4 * Q_THREADS); ++it) {
    const int l0 = it * 4 * Q_THREADS + 4 * tid;
    const int64_t i0 = v0 + l0;
    if (i0 >= n) break;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (i0 + c < n) v[c] = quant_value(quant_int(lds, nd_t, l0 + c, w), w, scale);
    if (vec_out && i0 + 3 < n) {
      *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (i0 + c < n) out[i0 + c] = v[c];
    }
  }
}

// every check of a table on its host copy; the largest count in *max_count
int sq_check_table(int m, const void* host_table, unsigned a_mask, unsigned b_mask,
                   int64_t* max_count) {
  const SqNode* h = static_cast<const SqNode*>(host_table);
  int64_t mc = 0;
  for (int j = 0; j < m; ++j) {
    if (!h[j].a || !h[j].b || (h[j].a & a_mask) || (h[j].b & b_mask)) return DPZ_ERR_ARG;
    if (h[j].count < 1 || h[j].count > SQ_NMAX) return DPZ_ERR_ARG;
    if (h[j].slot_words < QI_WORDS || h[j].slot_words >= Q_NMAX) return DPZ_ERR_ARG;
    mc = h[j].count > mc ? h[j].count : mc;
  }
  *max_count = mc;
  return DPZ_OK;
}

}  // namespace

extern "C" int64_t dpz_squant_row_words(int64_t count, int64_t k) {
  if (count < 1 || count > SQ_NMAX || k < 1 || k > ((int64_t)1 << 30)) return 0;
  int wmax = 2;  // bit_length(k) + 1
  while ((k >> (wmax - 1)) != 0) ++wmax;
  return QI_WORDS + (count * wmax + 31) / 32;
}

extern "C" size_t dpz_squant_encode_nodes_workspace_bytes(int m, int64_t max_count) {
  if (m < 1 || max_count < 1 || max_count > SQ_NMAX) return 0;
  return (size_t)m * 8 * (size_t)quant_chunks(max_count);
}

extern "C" int dpz_squant_encode_nodes(int m, const void* table, const void* host_table, int64_t k,
                                       void* ws, size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || k < 1 || k > ((int64_t)1 << 30)) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 7u))
    return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  int64_t max_count = 0;
  const int rc = sq_check_table(m, host_table, 3u, 3u, &max_count);
  if (rc != DPZ_OK) return rc;
  if (!ws || ws_bytes < dpz_squant_encode_nodes_workspace_bytes(m, max_count))
    return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SqNode* tab = static_cast<const SqNode*>(table);
  const int64_t C = quant_chunks(max_count);
  const dim3 sgrid((unsigned)C, (unsigned)m);
  DPZ_TIMED(DPZ_KT_QUANT_STATS, st,
            squant_stats_nodes_kernel<<<sgrid, Q_THREADS, 0, st>>>(tab, m, C,
                                                                   static_cast<uint32_t*>(ws)));
  const dim3 pgrid((unsigned)((max_count + Q_SPAN - 1) / Q_SPAN) + 1, (unsigned)m);
  DPZ_TIMED(DPZ_KT_QUANT_PACK, st,
            squant_pack_nodes_kernel<<<pgrid, Q_THREADS, 0, st>>>(tab, m, (int)k, C,
                                                                  static_cast<uint32_t*>(ws)));
  return DPZ_OK;
}

extern "C" int dpz_squant_decode_nodes(int m, const void* table, const void* host_table,
                                       uint32_t* status, dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || !status) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(status) & 3u))
    return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  int64_t max_count = 0;
  const int rc = sq_check_table(m, host_table, 3u, 3u, &max_count);
  if (rc != DPZ_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((max_count + SQ_TILE - 1) / SQ_TILE), (unsigned)m);
  DPZ_TIMED(DPZ_KT_QUANT_UNPACK, st,
            squant_decode_nodes_kernel<<<grid, Q_THREADS, 0, st>>>(
                static_cast<const SqNode*>(table), status));
  return DPZ_OK;
}
