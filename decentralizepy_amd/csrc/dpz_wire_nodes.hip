// The wire streams of a rank's nodes in one launch set: per node the Elias-gamma stream of its
// ascending indices (dpz_elias.hip's format, the reference's Elias.compress bytes) and the
// block-floating stream of its values (dpz_fpz.hip's format), every node with its own count.
//
// Replaces the node-by-node loop of dpz_elias_encode + dpz_fpz_encode (six launches and two host
// synchronisations a node) behind the reference's per-message
//   compression/EliasFpzip.py:19-51       compress / compress_float
//   communication/TCP.py:110-131          total_bytes, total_data_per_n
// with THREE launches whatever the node count and no host synchronisation.
//
// Work split.  A chunk is 1024 consecutive entries of one node's lists: one Elias block of
// EL_CODES gaps AND four value blocks of FZ_B values, so one workgroup of four waves owns both
// legs of the same chunk.  The grid is (chunks of the longest node, node): a workgroup past its
// node's last chunk leaves at once (the project's habit for unequal rows; a prefix table of
// (node, chunk) pairs would need an upload that depends on the counts, and the idle workgroups
// cost one table read each).
//   size   per chunk: the code-bit total of its gaps (bit 63 set when a gap is zero or negative)
//          and the word count of each of its four value blocks.  The chunk's 1025 indices are
//          staged into LDS by coalesced loads; a thread then reads the five it needs from LDS.
//   scan   one workgroup of 1024 threads per node: exclusive scans of both legs' block sizes, the
//          stream lengths into sizes[node], the status word, the go / no-go flags of the pack;
//          where the index stream is written its trailer, padding and zeroed boundary words,
//          where the value stream is written its header and block table.
//   pack   per chunk: the gaps' codes are OR-ed into an LDS image of the chunk's words (staged
//          indices again), interior words stored, the two words shared with the neighbouring
//          chunks OR-ed into global memory; each wave assembles one value block's planes in its
//          own LDS stage and stores whole words.
// LDS of the pack: 1025 staged indices, 2018 code words, four stages of 258 words: 16.4 KB.
// No float atomics (the integer ORs commute); nothing depends on the grid.
#include "dpz_common.h"
#include "dpz_wire.h"

#include <math.h>

namespace dpz {

static_assert(EL_CODES == 4 * FZ_B, "a chunk is one Elias block and one value block per wave");
constexpr uint64_t WN_BAD = 1ull << 63;  // in a chunk's bit total: a zero or negative gap
constexpr uint32_t WN_ST_LIST = 1u, WN_ST_IDX_CAP = 2u, WN_ST_VAL_CAP = 4u;  // status bits
constexpr uint32_t WN_GO_IDX = 1u, WN_GO_VAL = 2u;                           // pack flags

struct WireNode {  // one table entry: 8 64-bit words
  const int32_t* idx;  // 0: a full share, no index stream
  const float* val;
  int64_t count;
  uint32_t* idx_out;  // 0: size only
  uint32_t* val_out;  // 0: size only
  int64_t idx_cap, val_cap;  // bytes
  uint64_t zero;
};
static_assert(sizeof(WireNode) == 64, "8 words");

struct WireWs {  // the workspace's arrays; node j's rows start at j * nb (4 j nb for the values)
  uint32_t* go;        // [m] pack flags
  uint64_t* el_bits;   // [m][nb] code bits of a chunk | WN_BAD
  uint64_t* el_off;    // [m][nb] bit offset of a chunk
  uint32_t* fz_words;  // [m][4 nb] words of a value block
  uint32_t* fz_off;    // [m][4 nb] word offset of a value block in the block area
  int64_t nb;          // chunks of the longest node (>= 1)
};

__device__ __forceinline__ int64_t wn_codes(const WireNode& nd) { return nd.idx ? nd.count - 1 : 0; }

// Chunk c's gaps: its indices idx[1024 c .. 1024 c + nc] go through LDS once; thread t gets codes
// 4 t .. 4 t + 3 (len 0 past the chunk's nc codes; a zero gap is a 1-bit code, reported in *bad).
__device__ __forceinline__ void wn_gaps(const int32_t* __restrict__ idx, int64_t ncodes, int64_t c,
                                        int32_t* s_idx, uint32_t g[4], uint32_t len[4],
                                        int* bad) {
  const int64_t c0 = c * EL_CODES;
  const int nc = (int)((ncodes - c0) < EL_CODES ? (ncodes - c0) : EL_CODES);
  for (int i = threadIdx.x; i <= nc; i += 256) s_idx[i] = idx[c0 + i];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * threadIdx.x + e;
    g[e] = 0;
    len[e] = 0;
    if (j < nc) {
      g[e] = (uint32_t)(s_idx[j + 1] - s_idx[j]);
      if (g[e] == 0 || (int32_t)g[e] < 0) *bad = 1;
      len[e] = g[e] ? code_len(g[e]) : 1u;
    }
  }
}

__global__ void __launch_bounds__(256) wire_size_kernel(const WireNode* __restrict__ tab, int prec,
                                                        int mb, WireWs ws) {
  __shared__ int32_t s_idx[EL_CODES + 1];
  __shared__ uint64_t wsum[16];
  const int64_t node = blockIdx.y, c = blockIdx.x;
  const WireNode nd = tab[node];
  const int64_t ncodes = wn_codes(nd);
  if (c * EL_CODES < ncodes) {  // the same for the whole workgroup: barriers inside
    uint32_t g[4], len[4];
    int bad = 0;
    wn_gaps(nd.idx, ncodes, c, s_idx, g, len, &bad);
    uint64_t tot;
    block_excl_scan64((uint64_t)len[0] + len[1] + len[2] + len[3], wsum, &tot);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) ws.el_bits[node * ws.nb + c] = tot | (bad ? WN_BAD : 0ull);
  }
  const int64_t nblk = (nd.count + FZ_B - 1) / FZ_B;
  const int64_t b = c * 4 + (threadIdx.x >> 6);
  if (b < nblk) {
    const int lane = threadIdx.x & 63;
    uint32_t u[4], emin;
    int cnt, w;
    fz_load(nd.val, nd.count, b, prec, lane, u, &cnt, &emin, &w);
    if (lane == 0) ws.fz_words[node * 4 * ws.nb + b] = fz_words(cnt, w, mb);
  }
}

// Every loop below gives block b to thread b % 1024, so a thread reads back only its own stores.
__global__ void __launch_bounds__(1024) wire_scan_kernel(const WireNode* __restrict__ tab,
                                                         int prec, WireWs ws,
                                                         int64_t* __restrict__ sizes,
                                                         uint32_t* __restrict__ status) {
  __shared__ uint64_t wsum[16];
  const int64_t node = blockIdx.x;
  const WireNode nd = tab[node];
  const int64_t ncodes = wn_codes(nd);
  const int64_t nch = (ncodes + EL_CODES - 1) / EL_CODES;
  const int64_t nblk = (nd.count + FZ_B - 1) / FZ_B;
  const uint64_t* el_bits = ws.el_bits + node * ws.nb;
  uint64_t* el_off = ws.el_off + node * ws.nb;
  const uint32_t* fzw = ws.fz_words + node * 4 * ws.nb;
  uint32_t* fz_off = ws.fz_off + node * 4 * ws.nb;
  uint64_t L = 0;  // the totals come back to every thread: L and W are the same in all of them
  int bad = 0;
  for (int64_t b0 = 0; b0 < nch; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const uint64_t raw = b < nch ? el_bits[b] : 0;
    if (raw & WN_BAD) bad = 1;
    uint64_t tot;
    const uint64_t ex = block_excl_scan64(raw & ~WN_BAD, wsum, &tot) + L;
    if (b < nch) el_off[b] = ex;
    L += tot;
  }
  bad = __syncthreads_or(bad);
  uint64_t W = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = block_excl_scan64(b < nblk ? fzw[b] : 0, wsum, &tot) + W;
    if (b < nblk) fz_off[b] = (uint32_t)ex;
    W += tot;
  }
  const uint64_t nbits = L + 128;
  const uint64_t nbytes = nd.idx ? (nbits + 7) >> 3 : 0;
  const uint64_t nwords = (nbytes + 3) >> 2;
  const uint64_t vbytes = 4 * (4 + (uint64_t)nblk + 1 + W);
  const bool idx_fits = 4 * nwords <= (uint64_t)nd.idx_cap;
  const bool val_fits = vbytes <= (uint64_t)nd.val_cap;
  const bool go_idx = nd.idx && nd.idx_out && !bad && idx_fits;
  const bool go_val = nd.val_out && val_fits;
  if (threadIdx.x == 0) {
    sizes[2 * node] = (int64_t)nbytes;
    sizes[2 * node + 1] = (int64_t)vbytes;
    status[node] = (bad ? WN_ST_LIST : 0u) |
                   (nd.idx && nd.idx_out && !idx_fits ? WN_ST_IDX_CAP : 0u) |
                   (nd.val_out && !val_fits ? WN_ST_VAL_CAP : 0u);
    ws.go[node] = (go_idx ? WN_GO_IDX : 0u) | (go_val ? WN_GO_VAL : 0u);
  }
  if (go_idx) {
    uint32_t* out32 = nd.idx_out;
    const uint64_t tail_w0 = L >> 5;
    // the words two chunks share are OR-ed by the pack: zero them (below the tail, written next)
    for (int64_t b = threadIdx.x; b < nch; b += 1024) {
      const uint64_t o = el_off[b], n = el_bits[b];
      const uint64_t wf = o >> 5, wl = (o + n - 1) >> 5;
      if (wf < tail_w0) out32[wf] = 0u;
      if (wl < tail_w0) out32[wl] = 0u;
    }
    // tail words: zero padding + trailer (int64 LE first, int64 LE nbits) in byte order; the
    // bytes of the last word past the stream keep their content
    const uint64_t first = (uint64_t)(int64_t)nd.idx[0];
    for (uint64_t w = tail_w0 + threadIdx.x; w < nwords; w += 1024) {
      uint32_t val = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint64_t B = 4 * w + j;
        uint32_t byte = 0;
        if (B >= nbytes - 16 && B < nbytes - 8) byte = (uint32_t)(first >> (8 * (B - (nbytes - 16)))) & 0xFFu;
        else if (B >= nbytes - 8 && B < nbytes) byte = (uint32_t)(nbits >> (8 * (B - (nbytes - 8)))) & 0xFFu;
        val |= byte << (8 * j);
      }
      if (w == nwords - 1 && (nbytes & 3u)) val |= out32[w] & (0xFFFFFFFFu << (8 * (nbytes & 3u)));
      out32[w] = val;
    }
  }
  if (go_val) {
    uint32_t* out32 = nd.val_out;
    for (int64_t b = threadIdx.x; b < nblk; b += 1024) out32[4 + b] = fz_off[b];
    if (threadIdx.x == 0) {
      out32[0] = FZ_MAGIC;
      out32[1] = (uint32_t)nd.count;
      out32[2] = (uint32_t)prec;
      out32[3] = (uint32_t)nblk;
      out32[4 + nblk] = (uint32_t)W;
    }
  }
}

__global__ void __launch_bounds__(256) wire_pack_kernel(const WireNode* __restrict__ tab, int prec,
                                                        int mb, WireWs ws) {
  constexpr int MAXW = (EL_CODES * 63 + 31) / 32 + 2;
  __shared__ int32_t s_idx[EL_CODES + 1];
  __shared__ uint32_t words[MAXW];
  __shared__ uint64_t wsum[16];
  __shared__ uint32_t stage[4][FZ_MAXW + 1];
  const int64_t node = blockIdx.y, c = blockIdx.x;
  const uint32_t go = ws.go[node];
  if (!go) return;
  const WireNode nd = tab[node];
  const int64_t ncodes = wn_codes(nd);
  if ((go & WN_GO_IDX) && c * EL_CODES < ncodes) {  // the same for the whole workgroup
    const uint64_t B0 = ws.el_off[node * ws.nb + c];
    const uint64_t B1 = B0 + ws.el_bits[node * ws.nb + c];  // no WN_BAD: such a node does not go
    const uint64_t w0 = B0 >> 5, w1 = (B1 - 1) >> 5;
    const int nw = (int)(w1 - w0 + 1);
    for (int w = threadIdx.x; w < nw; w += 256) words[w] = 0u;
    uint32_t g[4], len[4];
    int bad = 0;
    wn_gaps(nd.idx, ncodes, c, s_idx, g, len, &bad);
    uint64_t tot;
    uint64_t off = block_excl_scan64((uint64_t)len[0] + len[1] + len[2] + len[3], wsum, &tot) + B0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // after the scan's barriers: the image is zeroed
      if (g[e]) {
        const uint32_t l = (len[e] - 1) >> 1;
        const uint32_t n = l + 1;
        const uint64_t rel = off + l - 32 * w0;  // value bits start here
        const int wi = (int)(rel >> 5);
        const uint32_t b = (uint32_t)(rel & 31);
        const uint64_t v64 = (uint64_t)g[e] << (64 - b - n);
        const uint32_t hi = (uint32_t)(v64 >> 32), lo = (uint32_t)v64;
        if (hi) atomicOr(&words[wi], hi);
        if (lo) atomicOr(&words[wi + 1], lo);
      }
      off += len[e];
    }
    __syncthreads();
    uint32_t* out32 = nd.idx_out;
    for (int w = threadIdx.x; w < nw; w += 256) {
      const uint32_t val = __builtin_bswap32(words[w]);
      if (w == 0 || w == nw - 1) {
        if (val) atomicOr(&out32[w0 + w], val);
      } else {
        out32[w0 + w] = val;
      }
    }
  }
  const int64_t nblk = (nd.count + FZ_B - 1) / FZ_B;
  const int wid = threadIdx.x >> 6;
  const int64_t b = c * 4 + wid;
  if ((go & WN_GO_VAL) && b < nblk)  // whole waves, wave-level barriers only
    fz_pack_block(nd.val, nd.count, b, prec, mb, threadIdx.x & 63, stage[wid],
                  nd.val_out + 4 + nblk + 1 + ws.fz_off[node * 4 * ws.nb + b]);
}

static inline size_t wn_al256(size_t v) { return (v + 255) & ~size_t(255); }

static inline int64_t wn_chunks(int64_t max_count) {
  const int64_t nb = (max_count + EL_CODES - 1) / EL_CODES;
  return nb > 0 ? nb : 1;
}

}  // namespace dpz

using namespace dpz;

extern "C" int64_t dpz_elias_bound_bytes(int64_t k, int64_t n) {
  if (k < 2) return 0;
  const int64_t c = k - 1, s = n - 1;
  if (s < c) return dpz_elias_max_bytes(k);  // no ascending list of k indices lies below n
  // a code is 2 floor(log2 g) + 1 <= 2 log2 g + 1 bits and log2 is concave: c codes whose gaps
  // sum to at most s take at most x = c (2 log2(s / c) + 1) bits.  A stream's bit count is an
  // integer, so floor(x) bounds it; the slack covers the rounding of x and leaves an integer x
  // (gaps of one power of two: s / c and its log2 are exact) unchanged
  const double x = (double)c * (2.0 * log2((double)s / (double)c) + 1.0);
  int64_t bits = (int64_t)floor(x + x * 1e-12 + 1e-6);
  if (bits > 63 * c) bits = 63 * c;
  bits += 128;
  return ((bits + 31) / 32) * 4 + 16;
}

extern "C" size_t dpz_wire_nodes_workspace_bytes(int m, int64_t max_count) {
  if (m < 1 || max_count < 0 || max_count > FZ_MAXN) return 0;
  const size_t nb = (size_t)wn_chunks(max_count);
  return wn_al256((size_t)m * 4) + (size_t)m * nb * (2 * 8 + 2 * 4 * 4);
}

extern "C" int dpz_wire_encode_nodes(int m, const void* table, const void* host_table,
                                     int precision, int64_t* sizes, uint32_t* status, void* ws,
                                     size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || !sizes || !status) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(sizes) & 7u) ||
      (reinterpret_cast<uintptr_t>(status) & 3u) || (reinterpret_cast<uintptr_t>(ws) & 7u))
    return DPZ_ERR_ARG;
  int prec = 0;
  const int mb = fz_mbits(precision, &prec);
  if (mb < 0) return DPZ_ERR_UNSUPPORTED;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  const uint64_t* h = static_cast<const uint64_t*>(host_table);
  int64_t max_count = 0;
  bool any_out = false;
  for (int j = 0; j < m; ++j) {  // every check on the host copy, before anything is enqueued
    const uint64_t* e = h + 8 * (size_t)j;
    const int64_t count = (int64_t)e[2], idx_cap = (int64_t)e[5], val_cap = (int64_t)e[6];
    if (count < 0 || count > FZ_MAXN || (count > 0 && !e[1])) return DPZ_ERR_ARG;
    if (e[0] && count < 2) return DPZ_ERR_ARG;  // the reference's Elias.compress raises IndexError
    if (!e[0] && e[3]) return DPZ_ERR_ARG;      // an index slot without indices
    if ((e[0] | e[1] | e[3] | e[4]) & 3u) return DPZ_ERR_ARG;
    if (idx_cap < 0 || val_cap < 0 || e[7]) return DPZ_ERR_ARG;
    max_count = count > max_count ? count : max_count;
    any_out = any_out || e[3] || e[4];
  }
  if (!ws || ws_bytes < dpz_wire_nodes_workspace_bytes(m, max_count)) return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  WireWs w;
  w.nb = wn_chunks(max_count);
  char* p = static_cast<char*>(ws);
  const size_t rows = (size_t)m * (size_t)w.nb;
  w.go = reinterpret_cast<uint32_t*>(p);
  w.el_bits = reinterpret_cast<uint64_t*>(p + wn_al256((size_t)m * 4));
  w.el_off = w.el_bits + rows;
  w.fz_words = reinterpret_cast<uint32_t*>(w.el_off + rows);
  w.fz_off = w.fz_words + 4 * rows;
  const WireNode* tab = static_cast<const WireNode*>(table);
  const dim3 grid((unsigned)w.nb, (unsigned)m);
  // timed under the value coder's names: the value leg is the longer one of every payload
  DPZ_TIMED(DPZ_KT_FPZ_SIZE, st, wire_size_kernel<<<grid, 256, 0, st>>>(tab, prec, mb, w));
  DPZ_TIMED(DPZ_KT_FPZ_SCAN, st, wire_scan_kernel<<<(unsigned)m, 1024, 0, st>>>(tab, prec, w, sizes, status));
  if (any_out) DPZ_TIMED(DPZ_KT_FPZ_PACK, st, wire_pack_kernel<<<grid, 256, 0, st>>>(tab, prec, mb, w));
  return DPZ_OK;
}
