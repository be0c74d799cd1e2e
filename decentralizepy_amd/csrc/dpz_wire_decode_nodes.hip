// The receiving half of the wire: the Elias-gamma index stream and the block-floating value stream
// of every node of a table decoded in one launch set (the formats of dpz_elias.hip and dpz_fpz.hip,
// the sending half is dpz_wire_nodes.hip).
//
// Replaces the node-by-node loop of dpz_elias_decode_async + dpz_fpz_decode (three launches, a
// memset and a check kernel for the indices and one launch for the values, per node, with nbits
// and first read from the trailer on the host) behind the reference's per-message
//   compression/EliasFpzip.py:53-87       decompress / decompress_float
//   compression/Elias.py:54-97            Elias.decompress
// with THREE launches whatever the node count, no memset, nothing read back and no host
// synchronisation: the host knows every node's count and slot caps, the stream lengths are two
// device words per node (a row of the encoder's sizes, or a received row's header) and the
// trailer's nbits / first are read on the device by every workgroup that needs them.
//
// Work split.  The grid of the first and third launch is (workgroups of the longest node, node);
// a workgroup past its node's work leaves at once.
//   spec     a workgroup of four waves owns four 1024-bit index chunks AND four 256-value blocks:
//            each wave parses its chunk from all 63 possible entry offsets (exit offset, code
//            count, gap sum per entry: dpz_wire.h's parse) and then decodes its value block, which
//            needs nothing from the index leg.  A bad value block sets the workgroup's word of a
//            flag row, so the status needs neither a memset nor an atomic.
//   resolve  one workgroup of FOUR waves and 17 KB of LDS per node (the single-stream kernel holds
//            128 KB and 1024 threads for any stream, which wastes a CU on the 13-chunk streams of a
//            round).  A stream of at most one super map (64 chunks) is walked by wave 0 alone from
//            one staged 4 KB map.  Longer streams keep the super-map chain: the waves build the
//            64-chunk super maps into the workspace, the chain runs through them in LDS tiles of
//            256 supers, then the waves walk their supers' true paths.  The per-chunk code counts
//            and gap sums at the true entries are scanned into output positions and base values;
//            the node's status word and its go flag are written here.
//   write    one wave per chunk of a node that goes: lane 0 walks the true path ONCE, recording
//            the bit position of every code into LDS; then all 64 lanes extract gaps in rounds of
//            64 codes, prefix-sum them across the wave and store 64 consecutive indices.
// Gap sums are kept modulo 2^32: an int32 index is the low word of first + the running sum.
// Every read is bounded by the slot cap (the device-side lengths are checked against it first),
// every write by the node's count.  No float arithmetic; nothing depends on the grid.
#include "dpz_common.h"
#include "dpz_wire.h"

namespace dpz {

static_assert(EL_SUPER == 64, "a super map is walked by one wave, one chunk per lane in the scans");
constexpr uint32_t WD_ST_STREAM = 1u, WD_ST_COUNT = 2u, WD_ST_VALUES = 4u;  // status bits
constexpr int WD_TILE = 256;  // super maps per LDS tile of the chain (the four staging slots)

struct WireDecNode {  // one table entry: 8 64-bit words
  const uint32_t* idx_in;  // 0: a full share, no index stream
  const uint32_t* val_in;
  int64_t count;
  int32_t* idx_out;
  float* val_out;
  const int64_t* sizes;  // DEVICE {index stream bytes, value stream bytes}
  int64_t idx_cap, val_cap;  // bytes
};
static_assert(sizeof(WireDecNode) == 64, "8 words");

struct WireDecWs {  // the workspace's arrays; node j's rows start at j * nch (j * nvb, j * nsup)
  uint32_t* go;       // [m] the write launch runs for this node
  uint32_t* vbad;     // [m][nvb] a value workgroup met a bad block
  uint8_t* exit_tab;  // [m][nch][64] exit offset per entry offset
  uint32_t* cnt_tab;  // [m][nch][64] codes walked
  uint32_t* sum_tab;  // [m][nch][64] their gap sum mod 2^32
  uint32_t* centry;   // [m][nch] true entry offset
  uint32_t* cpos;     // [m][nch] codes before the chunk
  uint32_t* cbase;    // [m][nch] gap sum before the chunk
  uint8_t* sup_tab;   // [m][nsup][64] super maps
  int64_t nch, nvb, nsup;
};

struct WdIdx {  // what a node's index stream says about itself
  bool ok;
  uint64_t L, nwords_in;
  int64_t nch;
  uint32_t first;  // the low word: indices are int32
};

// sizes[0] against the cap, then the trailer (int64 LE first, int64 LE nbits, byte-aligned only)
// against the byte length.  The same in every thread of every workgroup of the node.
__device__ __forceinline__ WdIdx wd_idx_header(const WireDecNode& nd) {
  WdIdx h = {false, 0, 0, 0, 0};
  const int64_t ib = nd.sizes[0];
  if (ib < 16 || ib > nd.idx_cap) return h;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(nd.idx_in) + (ib - 16);
  uint64_t first = 0, nbits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    first |= (uint64_t)p[j] << (8 * j);
    nbits |= (uint64_t)p[8 + j] << (8 * j);
  }
  if (nbits < 128 || nbits - 128 > (uint64_t)(ib - 16) * 8) return h;
  h.ok = true;
  h.L = nbits - 128;
  h.nwords_in = (uint64_t)(ib - 16 + 3) / 4;  // code + padding words; within ib <= idx_cap
  h.nch = (int64_t)((h.L + EL_CHUNK - 1) / EL_CHUNK);  // <= ceil(8 idx_cap / 1024) = a ws row
  h.first = (uint32_t)first;
  return h;
}

// sizes[1] against the cap, then the stream's header against (count, precision); *area = the words
// its block area may hold
__device__ __forceinline__ bool wd_val_header(const WireDecNode& nd, int prec, int64_t nblk,
                                              int64_t* area) {
  const int64_t vb = nd.sizes[1];
  if (vb < 0 || vb > nd.val_cap || (vb & 3) || vb < 4 * (4 + nblk + 1 + nblk)) return false;
  *area = vb / 4 - (4 + nblk + 1);
  const uint32_t* in32 = nd.val_in;
  return in32[0] == FZ_MAGIC && in32[1] == (uint32_t)nd.count && in32[2] == (uint32_t)prec &&
         in32[3] == (uint32_t)nblk;
}

__global__ void __launch_bounds__(256) wd_spec_kernel(const WireDecNode* __restrict__ tab,
                                                      int prec, int mb, WireDecWs ws) {
  __shared__ uint32_t st[4][EL_STAGE];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = blockIdx.y, g = blockIdx.x;
  const WireDecNode nd = tab[node];
  if (nd.idx_in) {
    const WdIdx h = wd_idx_header(nd);
    if (h.ok && 4 * g < h.nch) {  // the same for the whole workgroup: a barrier inside
      const int64_t c = 4 * g + wid;
      el_stage_chunk(nd.idx_in, h.nwords_in, c, c < h.nch, lane, st[wid]);
      __syncthreads();
      if (c < h.nch) {
        uint32_t cnt;
        uint64_t gsum;
        const uint8_t ex = el_parse_chunk(st[wid], c, h.L, lane, &cnt, &gsum);
        const int64_t o = (node * ws.nch + c) * 64 + lane;
        ws.exit_tab[o] = ex;
        ws.cnt_tab[o] = cnt;
        ws.sum_tab[o] = (uint32_t)gsum;
      }
    }
  }
  const int64_t nblk = (nd.count + FZ_B - 1) / FZ_B;
  if (4 * g < nblk) {  // whole workgroup again
    int64_t area = 0;
    const bool hdr = wd_val_header(nd, prec, nblk, &area);
    const int64_t b = 4 * g + wid;
    const int bad = !hdr || (b < nblk && !fz_decode_block(nd.val_in, area, nd.count, nblk, b, mb,
                                                          lane, nd.val_out));
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) ws.vbad[node * ws.nvb + g] = (uint32_t)any;
  }
}

__global__ void __launch_bounds__(256) wd_resolve_kernel(const WireDecNode* __restrict__ tab,
                                                         int prec, WireDecWs ws,
                                                         uint32_t* __restrict__ status) {
  __shared__ uint32_t stab[4][EL_SUPER * 16];  // per-wave staged chunk maps; the chain's tile
  __shared__ uint8_t sent[4][EL_SUPER];
  __shared__ uint8_t sentry[EL_MAX_SUPER + 1];
  __shared__ uint64_t wsum[16];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = blockIdx.x;
  const WireDecNode nd = tab[node];
  // the value leg's verdict: the header (also with no block at all) and the workgroups' flags
  const int64_t nblk = (nd.count + FZ_B - 1) / FZ_B;
  int64_t area = 0;
  int vb = !wd_val_header(nd, prec, nblk, &area);
  for (int64_t i = threadIdx.x; i < (nblk + 3) / 4; i += 256) vb |= ws.vbad[node * ws.nvb + i] != 0;
  uint32_t stw = __syncthreads_or(vb) ? WD_ST_VALUES : 0u;
  WdIdx h = {true, 0, 0, 0, 0};
  if (nd.idx_in) h = wd_idx_header(nd);
  if (!nd.idx_in || !h.ok) {  // the same in every thread
    if (threadIdx.x == 0) {
      status[node] = stw | (nd.idx_in ? WD_ST_STREAM : 0u);
      ws.go[node] = 0u;
    }
    return;
  }
  const int64_t nch = h.nch, S = (nch + EL_SUPER - 1) / EL_SUPER;
  const uint8_t* exit_tab = ws.exit_tab + node * ws.nch * 64;
  const uint32_t* cnt_tab = ws.cnt_tab + node * ws.nch * 64;
  const uint32_t* sum_tab = ws.sum_tab + node * ws.nch * 64;
  uint32_t* centry = ws.centry + node * ws.nch;
  uint32_t* cpos = ws.cpos + node * ws.nch;
  uint32_t* cbase = ws.cbase + node * ws.nch;
  uint8_t* sup = ws.sup_tab + node * ws.nsup * 64;
  const uint8_t* map = reinterpret_cast<const uint8_t*>(stab[wid]);
  auto stage = [&](int64_t s) {  // the chunk maps of super-chunk s -> this wave's LDS slot
    const int64_t c0 = s * EL_SUPER;
    const int64_t nc = (nch - c0) < EL_SUPER ? (nch - c0) : EL_SUPER;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(exit_tab + c0 * 64);
    for (int w = lane; w < nc * 16; w += 64) stab[wid][w] = src[w];
    return (int)nc;
  };
  int bad = 0;
  if (threadIdx.x == 0) sentry[0] = 0;
  if (S > 1) {
    // a) super maps: lane o walks the chunk maps of super-chunk s from entry o
    for (int64_t s0 = 0; s0 < S; s0 += 4) {
      const int64_t s = s0 + wid;
      int nc = 0;
      if (s < S) nc = stage(s);
      __syncthreads();
      if (s < S) {
        uint32_t e = lane < 63 ? lane : 0xFF;
        for (int j = 0; j < nc && e < 63; ++j) e = map[j * 64 + e];
        sup[s * 64 + lane] = (uint8_t)(e < 63 ? e : 0xFF);
      }
      __syncthreads();
    }
    // b) chain the super maps from entry 0, a tile of them in LDS at a time
    uint8_t* tile = reinterpret_cast<uint8_t*>(&stab[0][0]);
    for (int64_t t0 = 0; t0 < S; t0 += WD_TILE) {
      const int64_t nt = (S - t0) < WD_TILE ? (S - t0) : WD_TILE;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(sup + t0 * 64);
      for (int w = threadIdx.x; w < nt * 16; w += 256) (&stab[0][0])[w] = src[w];
      __syncthreads();
      if (threadIdx.x == 0) {
        uint32_t e = sentry[t0];
        for (int64_t s = 0; s < nt; ++s) {
          e = (e < 63) ? tile[s * 64 + e] : 0xFF;
          sentry[t0 + s + 1] = (uint8_t)e;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  // c) per-chunk true entries (lane 0 walks), then counts and gap sums (all lanes)
  for (int64_t s0 = 0; s0 < S; s0 += 4) {
    const int64_t s = s0 + wid;
    if (S == 1 && wid != 0) break;  // a short stream is wave 0's alone: wave-level barriers only
    int nc = 0;
    if (s < S) nc = stage(s);
    if (S > 1) __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (s < S && lane == 0) {
      uint32_t e = sentry[s];
      for (int j = 0; j < nc; ++j) {
        sent[wid][j] = (uint8_t)e;
        e = (e < 63) ? map[j * 64 + e] : 0xFF;
      }
      if (s == S - 1 && e != 0) bad = 1;  // the true path must end exactly at L
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (s < S && lane < nc) {
      const int64_t c = s * EL_SUPER + lane;
      const uint32_t e = sent[wid][lane];
      centry[c] = e;
      cpos[c] = e < 63 ? cnt_tab[c * 64 + e] : 0u;
      cbase[c] = e < 63 ? sum_tab[c * 64 + e] : 0u;
      if (e >= 63) bad = 1;
    }
    if (S > 1) __syncthreads();
  }
  bad = __syncthreads_or(bad);
  // d) exclusive scans of counts and gap sums over chunks (in place; a thread reads back only
  // what it stored, or what the barrier above made visible)
  uint64_t carry_n = 0, carry_s = 0;
  for (int64_t c0 = 0; c0 < nch; c0 += 256) {
    const int64_t c = c0 + threadIdx.x;
    const uint64_t n = c < nch ? cpos[c] : 0;
    const uint64_t sm = c < nch ? cbase[c] : 0;
    uint64_t tn, ts;
    const uint64_t pn = block_excl_scan64(n, wsum, &tn) + carry_n;
    const uint64_t ps = block_excl_scan64(sm, wsum, &ts) + carry_s;
    if (c < nch) {
      cpos[c] = (uint32_t)pn;
      cbase[c] = (uint32_t)ps;
    }
    carry_n += tn;
    carry_s += ts;
  }
  if (threadIdx.x == 0) {
    if (bad) stw |= WD_ST_STREAM;
    else if ((int64_t)carry_n + 1 != nd.count) stw |= WD_ST_COUNT;
    status[node] = stw;
    ws.go[node] = (stw & (WD_ST_STREAM | WD_ST_COUNT)) ? 0u : 1u;
  }
}

__global__ void __launch_bounds__(256) wd_write_kernel(const WireDecNode* __restrict__ tab,
                                                       WireDecWs ws) {
  __shared__ uint32_t st[4][EL_STAGE];
  __shared__ uint16_t starts[4][EL_CHUNK];  // bit position of every code of the chunk's true path
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t node = blockIdx.y, g = blockIdx.x;
  if (!ws.go[node]) return;
  const WireDecNode nd = tab[node];
  const WdIdx h = wd_idx_header(nd);  // ok: the node goes
  if (4 * g >= h.nch) return;         // the same for the whole workgroup
  const int64_t c = 4 * g + wid;
  el_stage_chunk(nd.idx_in, h.nwords_in, c, c < h.nch, lane, st[wid]);
  __syncthreads();
  if (c >= h.nch) return;
  const int64_t row = node * ws.nch + c;
  const uint32_t entry = ws.centry[row];  // < 63: the node goes
  const int n = (int)ws.cnt_tab[row * 64 + entry];  // codes of the true path, <= EL_CHUNK
  const int64_t o = 1 + (int64_t)ws.cpos[row];
  uint32_t run = h.first + ws.cbase[row];
  if (c == 0 && lane == 0) nd.idx_out[0] = (int32_t)h.first;
  if (lane == 0) {
    uint32_t pos = entry;
    for (int i = 0; i < n && i < EL_CHUNK; ++i) {
      starts[wid][i] = (uint16_t)pos;
      const uint64_t w = window64(st[wid], pos);
      pos += 2u * (uint32_t)__clzll((long long)(w | 1ull)) + 1u;
      if (pos >= EL_CHUNK + 63) pos = EL_CHUNK + 62;  // unreachable on a resolved path
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int r = 0; r < n && r < EL_CHUNK; r += 64) {
    const int i = r + lane;
    uint32_t gap = 0;
    if (i < n) {
      const uint64_t w = window64(st[wid], starts[wid][i]);
      const uint32_t z = (uint32_t)__clzll((long long)(w | 1ull)) & 31u;
      gap = (uint32_t)((w << z) >> (63 - z));
    }
    uint32_t x = gap;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (i < n && o + i < nd.count) nd.idx_out[o + i] = (int32_t)(run + x);
    run += __shfl(x, 63, 64);
  }
}

static inline size_t wd_al256(size_t v) { return (v + 255) & ~size_t(255); }

struct WdDims {
  int64_t nch, nvb, nsup, nb;
};

static inline WdDims wd_dims(int64_t max_idx_cap, int64_t max_count) {
  WdDims d;
  d.nch = (max_idx_cap * 8 + EL_CHUNK - 1) / EL_CHUNK;
  d.nch = d.nch > 0 ? d.nch : 1;
  d.nvb = (max_count + 4 * FZ_B - 1) / (4 * FZ_B);
  d.nvb = d.nvb > 0 ? d.nvb : 1;
  d.nsup = (d.nch + EL_SUPER - 1) / EL_SUPER;
  const int64_t ncg = (d.nch + 3) / 4;
  d.nb = ncg > d.nvb ? ncg : d.nvb;
  return d;
}

}  // namespace dpz

using namespace dpz;

extern "C" int64_t dpz_fpz_bound_bytes(int64_t n, int precision) {
  int prec = 0;
  const int mb = fz_mbits(precision, &prec);
  if (n < 0 || mb < 0) return 0;
  const int64_t nblk = (n + FZ_B - 1) / FZ_B;
  // a block: the meta word, 8 sign words, 64 exponent words at w = 8, 8 mb mantissa words
  return 4 * (4 + nblk + 1 + nblk * (int64_t)(73 + 8 * mb));
}

extern "C" size_t dpz_wire_decode_nodes_workspace_bytes(int m, int64_t max_idx_cap,
                                                        int64_t max_count) {
  if (m < 1 || max_idx_cap < 0 || max_count < 0 || max_count > FZ_MAXN) return 0;
  const WdDims d = wd_dims(max_idx_cap, max_count);
  if (d.nsup > EL_MAX_SUPER) return 0;
  const size_t M = (size_t)m;
  return wd_al256(M * 4) + wd_al256(M * d.nvb * 4) + M * d.nch * (64 * 9 + 3 * 4) +
         wd_al256(M * d.nsup * 64);
}

extern "C" int dpz_wire_decode_nodes(int m, const void* table, const void* host_table,
                                     int precision, uint32_t* status, void* ws, size_t ws_bytes,
                                     dpz_stream_t stream) {
  if (m < 1 || !table || !host_table || !status) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(status) & 3u) ||
      (reinterpret_cast<uintptr_t>(ws) & 7u))
    return DPZ_ERR_ARG;
  int prec = 0;
  const int mb = fz_mbits(precision, &prec);
  if (mb < 0) return DPZ_ERR_UNSUPPORTED;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  const uint64_t* h = static_cast<const uint64_t*>(host_table);
  int64_t max_count = 0, max_cap = 0;
  for (int j = 0; j < m; ++j) {  // every check on the host copy, before anything is enqueued
    const uint64_t* e = h + 8 * (size_t)j;
    const int64_t count = (int64_t)e[2], idx_cap = (int64_t)e[6], val_cap = (int64_t)e[7];
    if (count < 0 || count > FZ_MAXN || !e[1] || !e[5] || (count > 0 && !e[4])) return DPZ_ERR_ARG;
    if (e[0] && (count < 2 || !e[3])) return DPZ_ERR_ARG;  // no Elias stream holds one index
    if (!e[0] && e[3]) return DPZ_ERR_ARG;                 // an index list without a stream
    if (((e[0] | e[1] | e[3] | e[4]) & 3u) || (e[5] & 7u)) return DPZ_ERR_ARG;
    if (idx_cap < 0 || val_cap < 0) return DPZ_ERR_ARG;
    max_count = count > max_count ? count : max_count;
    if (e[0]) max_cap = idx_cap > max_cap ? idx_cap : max_cap;
  }
  const WdDims d = wd_dims(max_cap, max_count);
  if (d.nsup > EL_MAX_SUPER) return DPZ_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < dpz_wire_decode_nodes_workspace_bytes(m, max_cap, max_count))
    return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t M = (size_t)m, rows = M * (size_t)d.nch;
  WireDecWs w;
  w.nch = d.nch;
  w.nvb = d.nvb;
  w.nsup = d.nsup;
  char* p = static_cast<char*>(ws);
  w.go = reinterpret_cast<uint32_t*>(p); p += wd_al256(M * 4);
  w.vbad = reinterpret_cast<uint32_t*>(p); p += wd_al256(M * d.nvb * 4);
  w.cnt_tab = reinterpret_cast<uint32_t*>(p); p += rows * 64 * 4;
  w.sum_tab = reinterpret_cast<uint32_t*>(p); p += rows * 64 * 4;
  w.exit_tab = reinterpret_cast<uint8_t*>(p); p += rows * 64;
  w.centry = reinterpret_cast<uint32_t*>(p); p += rows * 4;
  w.cpos = reinterpret_cast<uint32_t*>(p); p += rows * 4;
  w.cbase = reinterpret_cast<uint32_t*>(p); p += rows * 4;
  w.sup_tab = reinterpret_cast<uint8_t*>(p);
  const WireDecNode* tab = static_cast<const WireDecNode*>(table);
  const dim3 grid((unsigned)d.nb, (unsigned)m), wgrid((unsigned)((d.nch + 3) / 4), (unsigned)m);
  DPZ_TIMED(DPZ_KT_ELIAS_SPEC, st, wd_spec_kernel<<<grid, 256, 0, st>>>(tab, prec, mb, w));
  DPZ_TIMED(DPZ_KT_ELIAS_RESOLVE, st, wd_resolve_kernel<<<(unsigned)m, 256, 0, st>>>(tab, prec, w, status));
  if (max_cap > 0) DPZ_TIMED(DPZ_KT_ELIAS_WRITE, st, wd_write_kernel<<<wgrid, 256, 0, st>>>(tab, w));
  return DPZ_OK;
}
