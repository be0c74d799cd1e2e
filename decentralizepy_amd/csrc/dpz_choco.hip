// A Choco-SGD round of a rank's nodes (decentralizepy_amd/gossip_choco.py; reference
// sharing/Choco.py:186-207 the threshold sparsification, :359-453 the round).
//
// dpz_choco_encode_nodes: `_pre_step` + `serialized_model` of m nodes: the selection of
// dpz_select_nodes.h under ChocoPolicy.  d = fl(x - x_hat) is formed on the fly in every pass and
// never stored (every pass reads x and x_hat alone); with T the k-th largest key |d|, every i with
// key_i >= T and key_i != 0 (all ties, no exact zeros) goes in ascending order into the node's
// packed row, and what is past the row's cap is reported by its status word, never written.
//
// dpz_choco_fold_nodes: `_averaging` of m receivers in one launch.  A block owns a column tile of
// one receiver: the tile of s and of x_hat sits in LDS, each payload's first entry inside the tile
// is found by a wave-wide 64-ary search over its ascending indices, the payloads are applied one
// after another (a payload's indices are unique, so its entries update in parallel; a barrier
// between payloads keeps the fold order), the receiver's own payload last (x_hat += q, s += q
// w_self), then x and s are written once, and x_hat where the own payload changed it (the other
// float4 groups keep their bits: 12 N bytes read, 8 N + 16 per entry written).
//
// Why skipping a payload's missing entries is exact: the dense form adds fl(0 * w) = +-0 to s
// and +0 to x_hat at an element the payload does not name, and v + (+-0) has the bits of v for
// every v except -0 (where -0 + +0 = +0).  s and x_hat never hold -0: they start at +0, a sum
// in round-to-nearest is -0 only when both terms are -0, and neither the running s (+0 or
// nonzero or an exact cancellation, which is +0) nor x_hat + q (q is never a zero: key 0 is not
// selected) can be the first -0.  NaN and infinities propagate the same way in both forms as long
// as the weights are finite, which the host check enforces.
#include <algorithm>
#include <cmath>
#include <vector>

#include "dpz_common.h"
#include "dpz_select_nodes.h"

namespace {

using dpz::aligned16;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int HEADER = 4;                 // int32 words in front of a row's idx / val slots
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes
constexpr int TILE = 4096;                // fold: elements of one receiver a block owns
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_GROUP = 8;             // payloads whose first entries a thread keeps in flight

// ---- encode -------------------------------------------------------------------------------------
struct ChocoNode {  // 4 64-bit words of the node table
  const float* x;
  const float* xh;
  int32_t* row;     // [count lo, count hi, status, 0 | cap idx | cap val]
  uint64_t pad;
};
static_assert(sizeof(ChocoNode) == 32, "4 64-bit words");

struct ChocoArgs {
  const ChocoNode* tab;
  uint32_t k;
  int64_t cap;
};

// d = fl(x - x_hat) of the 4 elements from i0 (zeros past n); returns how many lie inside
__device__ __forceinline__ int load_d4(const float* __restrict__ x, const float* __restrict__ xh,
                                       int64_t i0, int64_t n, bool vec, float d[4]) {
  const int cnt = dpz::count4(i0, n);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(x + i0);
    const float4 b = *reinterpret_cast<const float4*>(xh + i0);
    d[0] = a.x - b.x, d[1] = a.y - b.y, d[2] = a.z - b.z, d[3] = a.w - b.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = e < cnt ? x[i0 + e] - xh[i0 + e] : 0.0f;
  }
  return cnt;
}

struct ChocoPolicy {  // dpz_select_nodes.h; no key row: every pass forms d from x and x_hat
  using Node = ChocoNode;
  using Args = ChocoArgs;
  static constexpr bool kAllTies = true, kIdleNodes = false, kHeader = true;
  static __device__ __forceinline__ uint32_t k(const Node, const Args a, int64_t) { return a.k; }
  static __device__ __forceinline__ uint32_t slots(const Node, const Args a, int64_t) {
    return (uint32_t)a.cap;
  }
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const Node nd, const Args) {
    return aligned16(nd.x) && aligned16(nd.xh);
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const Node nd, const Args, int64_t i0, int64_t n,
                                              bool vec, float d[4]) {
    return load_d4(nd.x, nd.xh, i0, n, vec, d);
  }
  // count < 2^31: the int64's high word is 0; an overflow is reported by the status word
  static __device__ __forceinline__ void header(const Node nd, const Args a, uint64_t count) {
    nd.row[0] = (int32_t)count;
    nd.row[1] = 0;
    nd.row[2] = count > (uint64_t)a.cap ? 1 : 0;
    nd.row[3] = 0;
  }
  static __device__ __forceinline__ void store(const Node nd, const Args a, uint32_t pos,
                                               int64_t i, float d) {
    nd.row[HEADER + pos] = (int32_t)i;
    reinterpret_cast<float*>(nd.row + HEADER + a.cap)[pos] = d;
  }
};

// ---- fold ---------------------------------------------------------------------------------------
struct ChocoRecv {  // 6 64-bit words
  float* x;
  float* xh;
  float* s;
  const int32_t* self_row;
  float w_self;
  int32_t self_cap;
  int32_t start;  // its list: entries [start, start + count)
  int32_t count;
};
static_assert(sizeof(ChocoRecv) == 48, "6 64-bit words");

struct ChocoEntry {  // 2 64-bit words
  const int32_t* row;
  float w;
  int32_t cap;
};
static_assert(sizeof(ChocoEntry) == 16, "2 64-bit words");

struct FoldArgs {
  const ChocoRecv* recv;
  const ChocoEntry* ent;
  int64_t n;
  float step;
  const int32_t* guard;
  int64_t guard_n;
};

// First e in [0, cnt) with idx[e] >= target (cnt if none), idx ascending: a 64-ary search, every
// lane of the wave probes one position per step (3 steps for 110,000 entries).  Whatever the data
// holds, the result lies in [0, cnt].
__device__ __forceinline__ int wave_lower_bound(const int32_t* __restrict__ idx, int cnt,
                                                int target) {
  const int lane = threadIdx.x & 63;
  int lo = 0, len = cnt;
  while (len > 0) {
    const int step = (len + 63) >> 6;
    const int pos = lo + (lane + 1) * step - 1;
    const bool less = pos < lo + len && idx[pos] < target;
    const int c = __popcll(__ballot(less));
    const int nlo = lo + c * step;
    const int rem = lo + len - nlo;
    len = rem < step - 1 ? rem : step - 1;
    lo = nlo;
  }
  return lo;
}

struct PayRef {  // a payload as the fold reads it
  const int32_t* idx;
  const float* val;
  int cnt;
  float w;
};

__device__ __forceinline__ PayRef pay_ref(const int32_t* row, int32_t cap, float w) {
  PayRef p;
  const int c = row[0];  // the int64 count's low word
  p.cnt = c < 0 ? 0 : (c > cap ? cap : c);
  p.idx = row + HEADER;
  p.val = reinterpret_cast<const float*>(row + HEADER + cap);
  p.w = w;
  return p;
}

__global__ void __launch_bounds__(FOLD_THREADS) choco_fold_kernel(const FoldArgs a) {
  __shared__ float s_l[TILE];
  __shared__ float h_l[TILE];
  __shared__ int lo_l[FOLD_GROUP];
  __shared__ uint8_t hdirty[TILE / 4];  // a float4 group of x_hat the own payload changed
  const int tid = threadIdx.x;
  {  // a slot overflowed somewhere in this round: nothing is written at all
    int bad = 0;
    for (int64_t i = tid; i < a.guard_n; i += FOLD_THREADS) bad |= a.guard[i] != 0;
    if (__syncthreads_or(bad)) return;
  }
  const ChocoRecv rc = a.recv[blockIdx.y];
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  const int tlen = (int)(a.n - t0 < TILE ? a.n - t0 : TILE);
  const int t_end = (int)(t0 + tlen);  // n < 2^31
  const bool vec = aligned16(rc.x) && aligned16(rc.xh) && aligned16(rc.s);
  float xr[TILE / FOLD_THREADS];  // this thread's x: group g = tid + 256 i, elements 4 g .. 4 g + 3
#pragma unroll
  for (int i = 0; i < TILE / (4 * FOLD_THREADS); ++i) {
    const int q = (tid + FOLD_THREADS * i) * 4;
    hdirty[q >> 2] = 0;
    if (vec && q + 4 <= tlen) {
      const float4 sv = *reinterpret_cast<const float4*>(rc.s + t0 + q);
      const float4 hv = *reinterpret_cast<const float4*>(rc.xh + t0 + q);
      const float4 xv = *reinterpret_cast<const float4*>(rc.x + t0 + q);
      *reinterpret_cast<float4*>(s_l + q) = sv;
      *reinterpret_cast<float4*>(h_l + q) = hv;
      xr[4 * i] = xv.x, xr[4 * i + 1] = xv.y, xr[4 * i + 2] = xv.z, xr[4 * i + 3] = xv.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = q + e < tlen;
        s_l[q + e] = in ? rc.s[t0 + q + e] : 0.0f;
        h_l[q + e] = in ? rc.xh[t0 + q + e] : 0.0f;
        xr[4 * i + e] = in ? rc.x[t0 + q + e] : 0.0f;
      }
    }
  }
  // the list, then the receiver's own payload as its last member
  const int total = rc.count + 1;
  for (int base = 0; base < total; base += FOLD_GROUP) {
    const int gs = total - base < FOLD_GROUP ? total - base : FOLD_GROUP;
    __syncthreads();  // the tile is staged / the last group is applied; lo_l is free
    for (int g = tid >> 6; g < gs; g += FOLD_THREADS / 64) {  // a wave per payload
      const int p = base + g;
      const PayRef pr = p < rc.count
                            ? pay_ref(a.ent[rc.start + p].row, a.ent[rc.start + p].cap, 0.0f)
                            : pay_ref(rc.self_row, rc.self_cap, 0.0f);
      const int lo = wave_lower_bound(pr.idx, pr.cnt, (int)t0);
      if ((tid & 63) == 0) lo_l[g] = lo;
    }
    __syncthreads();
    // every payload's first entry for this thread, all loads in flight before the first use
    int pj[FOLD_GROUP];
    float pv[FOLD_GROUP];
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) {
      pj[g] = t_end;
      pv[g] = 0.0f;
      if (g < gs) {
        const int p = base + g;
        const PayRef pr = p < rc.count
                              ? pay_ref(a.ent[rc.start + p].row, a.ent[rc.start + p].cap, 0.0f)
                              : pay_ref(rc.self_row, rc.self_cap, 0.0f);
        const int e = lo_l[g] + tid;
        if (e < pr.cnt) {
          pj[g] = pr.idx[e];
          pv[g] = pr.val[e];
        }
      }
    }
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) {
      if (g < gs) {  // uniform
        const int p = base + g;
        const bool self = p == rc.count;
        const PayRef pr = self ? pay_ref(rc.self_row, rc.self_cap, rc.w_self)
                               : pay_ref(a.ent[rc.start + p].row, a.ent[rc.start + p].cap,
                                         a.ent[rc.start + p].w);
        int j = pj[g];
        float v = pv[g];
        int e = lo_l[g] + tid;
        while (j < t_end) {  // ascending: the first entry past the tile ends this thread's walk
          const uint32_t jj = (uint32_t)(j - (int)t0);
          if (jj < (uint32_t)tlen) {
            if (self) {
              h_l[jj] = h_l[jj] + v;
              hdirty[jj >> 2] = 1;
            }
            const float term = v * pr.w;
            s_l[jj] = s_l[jj] + term;
          }
          e += FOLD_THREADS;
          if (e >= pr.cnt) break;
          j = pr.idx[e];
          v = pr.val[e];
        }
        __syncthreads();  // the next payload may name the same elements
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TILE / (4 * FOLD_THREADS); ++i) {
    const int q = (tid + FOLD_THREADS * i) * 4;
    float so[4], ho[4], xo[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      so[e] = s_l[q + e];
      ho[e] = h_l[q + e];
      const float diff = so[e] - ho[e];
      const float stepv = a.step * diff;
      xo[e] = xr[4 * i + e] + stepv;
    }
    if (vec && q + 4 <= tlen) {
      *reinterpret_cast<float4*>(rc.x + t0 + q) = make_float4(xo[0], xo[1], xo[2], xo[3]);
      *reinterpret_cast<float4*>(rc.s + t0 + q) = make_float4(so[0], so[1], so[2], so[3]);
      if (hdirty[q >> 2])  // elsewhere x_hat keeps its bits: nothing to write
        *reinterpret_cast<float4*>(rc.xh + t0 + q) = make_float4(ho[0], ho[1], ho[2], ho[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (q + e < tlen) {
          rc.x[t0 + q + e] = xo[e];
          rc.s[t0 + q + e] = so[e];
          rc.xh[t0 + q + e] = ho[e];
        }
      }
    }
  }
}

struct Span {
  uintptr_t lo, hi;
  bool written;
};

}  // namespace

extern "C" int64_t dpz_choco_chunk_elems(void) { return CHUNK; }
extern "C" int64_t dpz_choco_tile_elems(void) { return TILE; }

extern "C" size_t dpz_choco_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * dpz::node_ws(n).total;
}

extern "C" int dpz_choco_encode_nodes(int m, const void* node_table, int64_t n, int64_t k,
                                      int64_t cap, void* ws, size_t ws_bytes,
                                      dpz_stream_t stream) {
  if (m < 1 || n < 1 || k < 1 || k > n || cap < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || cap >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_choco_encode_workspace_bytes(m, n)) return DPZ_ERR_WORKSPACE;
  ChocoArgs a;
  a.tab = static_cast<const ChocoNode*>(node_table);
  a.k = (uint32_t)k;
  a.cap = cap;
  return dpz::select_nodes<ChocoPolicy>(m, a, n, ws, static_cast<hipStream_t>(stream));
}

extern "C" int dpz_choco_fold_nodes(int m, const void* fold_table, const void* host_table,
                                    int64_t n_entries, int64_t n, float step_size,
                                    const int32_t* guard, int64_t guard_n, dpz_stream_t stream) {
  if (m < 1 || n < 1 || n_entries < 0 || !fold_table || !host_table) return DPZ_ERR_ARG;
  if (guard_n < 0 || (guard_n > 0 && !guard) || !std::isfinite(step_size)) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  // the table: m receivers of 6 words, then n_entries list entries of 2 words
  const ChocoRecv* h_recv = static_cast<const ChocoRecv*>(host_table);
  const ChocoEntry* h_ent = reinterpret_cast<const ChocoEntry*>(h_recv + m);
  const uintptr_t row_bytes = (uintptr_t)n * sizeof(float);
  std::vector<Span> spans;
  spans.reserve((size_t)(4 * m + n_entries));
  auto packed = [&](const int32_t* row, int32_t cap) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(row);
    spans.push_back({p, p + (uintptr_t)(HEADER + 2 * (int64_t)cap) * 4, false});
  };
  for (int j = 0; j < m; ++j) {
    const ChocoRecv& r = h_recv[j];
    if (!r.x || !r.xh || !r.s || !r.self_row || r.self_cap < 1) return DPZ_ERR_ARG;
    if (!std::isfinite(r.w_self)) return DPZ_ERR_ARG;
    if (r.count < 0 || r.start < 0 || (int64_t)r.start + r.count > n_entries) return DPZ_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(r.self_row) & 3u) return DPZ_ERR_ARG;
    for (float* p : {r.x, r.xh, r.s}) {
      if (reinterpret_cast<uintptr_t>(p) & 3u) return DPZ_ERR_ARG;
      spans.push_back({reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + row_bytes,
                       true});
    }
    packed(r.self_row, r.self_cap);
    for (int p = 0; p < r.count; ++p) {
      const ChocoEntry& e = h_ent[r.start + p];
      if (!e.row || e.cap < 1 || !std::isfinite(e.w)) return DPZ_ERR_ARG;
      if (reinterpret_cast<uintptr_t>(e.row) & 3u) return DPZ_ERR_ARG;
      packed(e.row, e.cap);
    }
  }
  // receivers write in place while others read payloads: a written row may touch no other row
  std::sort(spans.begin(), spans.end(), [](const Span& p, const Span& q) { return p.lo < q.lo; });
  uintptr_t end_written = 0, end_any = 0;
  for (const Span& sp : spans) {
    if (sp.lo < end_written || (sp.written && sp.lo < end_any)) return DPZ_ERR_ARG;
    if (sp.written) end_written = std::max(end_written, sp.hi);
    end_any = std::max(end_any, sp.hi);
  }
  FoldArgs a;
  a.recv = static_cast<const ChocoRecv*>(fold_table);
  a.ent = reinterpret_cast<const ChocoEntry*>(a.recv + m);
  a.n = n;
  a.step = step_size;
  a.guard = guard;
  a.guard_n = guard_n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n + TILE - 1) / TILE), (unsigned)m);
  DPZ_TIMED(DPZ_KT_FOLD, st, choco_fold_kernel<<<grid, FOLD_THREADS, 0, st>>>(a));
  return DPZ_OK;
}
