// An STC round of a federation (decentralizepy_amd/gossip_stc.py; reference sharing/STC.py:
// 259-270 + 308-316 the client's encode, :333-362 the server's average, :318-331 its broadcast,
// :281-306 the receipt).
//
// dpz_stc_encode_nodes: the exact-k selection of m nodes (dpz_select_nodes.h) under StcPolicy.
// The first histogram pass forms c = fl(fl(x - prev) + r), stores it into r and x into prev; every
// later pass reads r alone (4 N bytes instead of 12 N).  Nothing recomputes c as Choco's passes
// recompute d: r has to be rewritten with c anyway (r = c outside the selection), so the store is
// no extra traffic, and after it prev already holds x, from which c could not be formed again.  A
// node in server form (x == NULL) has c in r already.  The compaction writes idx / val = r[i]
// ascending into the node's row and stores +0 to r[i] of what it sent.  Exactly k entries per row,
// ties at the k-th largest key to the lowest indices.
//
// dpz_stc_server_fold: the server's `_averaging_server` in one launch.  A block owns a tile of
// r_s and keeps the tile's `total` in LDS, starting at +0; each payload's first entry inside the
// tile is found by a wave-wide 64-ary search over its ascending indices; the payloads are applied
// in list order (one payload's entries in parallel, a barrier between payloads); then
// r_s = fl(r_s + total) is written once: r_s holds c_s, the server's change vector.
//
// Why skipping a payload's missing entries in `total` is exact: the dense form adds
// fl(0 * w) = +0 (w = 1 / n_workers > 0) at an element the payload does not name, and t + (+0) has
// the bits of t for every t except -0.  total never holds -0: it starts at +0 and a
// round-to-nearest sum is -0 only when both terms are -0.
//
// dpz_stc_apply_nodes: `process_received` of m models in one launch, in place:
// x[idx[e]] = fl(x[idx[e]] + val[e]) over the broadcast row's entries.  An element the row does not
// name keeps its bits (the reference's dense flat + T turns a -0 there into +0: DESIGN.md 3.15).
#include <algorithm>
#include <cmath>

#include "dpz_common.h"
#include "dpz_select_nodes.h"

namespace {

using dpz::aligned16;
using dpz::count4;
using dpz::load_c4;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int HEADER = 4;                 // int32 words in front of a row's idx / val slots
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes
constexpr int TILE = 8192;                // fold: elements of r_s a block owns
constexpr int FOLD_THREADS = 256;
constexpr int FOLD_GROUP = 8;             // payloads whose first entries a thread keeps in flight
constexpr int APPLY_THREADS = 256;

__host__ __device__ __forceinline__ int64_t up4(int64_t v) { return (v + 3) & ~int64_t(3); }

// ---- encode -------------------------------------------------------------------------------------
struct StcNode {  // 4 64-bit words of the node table
  const float* x;   // NULL: server form, r already holds c
  float* prev;
  float* r;
  int32_t* row;     // [count lo, count hi, status, 0 | up4(k) idx | up4(k) val]
};
static_assert(sizeof(StcNode) == 32, "4 64-bit words");

struct StcArgs {
  const StcNode* tab;
  uint32_t k;
  int64_t cap;
};

// c = fl(fl(x - prev) + r) of the 4 elements from i0, stored into r, and x into prev
__device__ __forceinline__ int form_c4(const StcNode nd, int64_t i0, int64_t n, bool vec,
                                       float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(nd.x + i0);
    const float4 b = *reinterpret_cast<const float4*>(nd.prev + i0);
    const float4 q = *reinterpret_cast<const float4*>(nd.r + i0);
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    c[0] = d0 + q.x, c[1] = d1 + q.y, c[2] = d2 + q.z, c[3] = d3 + q.w;
    *reinterpret_cast<float4*>(nd.r + i0) = make_float4(c[0], c[1], c[2], c[3]);
    *reinterpret_cast<float4*>(nd.prev + i0) = a;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[e] = 0.0f;
      if (e < cnt) {
        const float xv = nd.x[i0 + e];
        const float d = xv - nd.prev[i0 + e];
        c[e] = d + nd.r[i0 + e];
        nd.r[i0 + e] = c[e];
        nd.prev[i0 + e] = xv;
      }
    }
  }
  return cnt;
}

struct StcPolicy {  // dpz_select_nodes.h; the key row is r
  using Node = StcNode;
  using Args = StcArgs;
  static constexpr bool kAllTies = false, kIdleNodes = false, kHeader = true;
  static __device__ __forceinline__ uint32_t k(const Node, const Args a, int64_t) { return a.k; }
  static __device__ __forceinline__ uint32_t slots(const Node, const Args a, int64_t) {
    return a.k;
  }
  template <bool FIRST>
  static __device__ __forceinline__ bool vec(const Node nd, const Args) {
    const bool form = FIRST && nd.x != nullptr;
    return aligned16(nd.r) && (!form || (aligned16(nd.x) && aligned16(nd.prev)));
  }
  template <bool FIRST>
  static __device__ __forceinline__ int load4(const Node nd, const Args, int64_t i0, int64_t n,
                                              bool vec, float c[4]) {
    const bool form = FIRST && nd.x != nullptr;
    return form ? form_c4(nd, i0, n, vec, c) : load_c4(nd.r, i0, n, vec, c);
  }
  // exactly k are selected; k < 2^31: the int64's high word is 0
  static __device__ __forceinline__ void header(const Node nd, const Args a, uint64_t) {
    nd.row[0] = (int32_t)a.k;
    nd.row[1] = 0;
    nd.row[2] = 0;
    nd.row[3] = 0;
  }
  static __device__ __forceinline__ void store(const Node nd, const Args a, uint32_t pos,
                                               int64_t i, float c) {
    nd.row[HEADER + pos] = (int32_t)i;
    reinterpret_cast<float*>(nd.row + HEADER + a.cap)[pos] = c;
    nd.r[i] = 0.0f;  // sent: the residual keeps what was not
  }
};

// ---- server fold --------------------------------------------------------------------------------
struct StcPay {  // 2 64-bit words
  const int32_t* row;
  float w;
  int32_t pad;
};
static_assert(sizeof(StcPay) == 16, "2 64-bit words");

struct FoldArgs {
  const StcPay* pay;
  int n_pay;
  int64_t n;
  int k;
  int64_t cap;
  float* r_s;
};

// First e in [0, cnt) with idx[e] >= target (cnt if none), idx ascending: a 64-ary search, every
// lane of the wave probes one position per step.  Whatever the data holds, the result lies in
// [0, cnt] and no probe leaves [0, cnt).
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

__device__ __forceinline__ int row_count(const int32_t* row, int k) {
  const int c = row[0];  // the int64 count's low word
  return c < 0 ? 0 : (c > k ? k : c);
}

__global__ void __launch_bounds__(FOLD_THREADS) stc_fold_kernel(const FoldArgs a) {
  __shared__ __attribute__((aligned(16))) float tot_l[TILE];
  __shared__ int lo_l[FOLD_GROUP];
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  const int tlen = (int)(a.n - t0 < TILE ? a.n - t0 : TILE);
  const int t_end = (int)(t0 + tlen);  // n < 2^31
  for (int q = tid * 4; q < TILE; q += FOLD_THREADS * 4)
    *reinterpret_cast<float4*>(tot_l + q) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int base = 0; base < a.n_pay; base += FOLD_GROUP) {
    const int gs = a.n_pay - base < FOLD_GROUP ? a.n_pay - base : FOLD_GROUP;
    __syncthreads();  // the tile is zeroed / the last group is applied; lo_l is free
    for (int g = tid >> 6; g < gs; g += FOLD_THREADS / 64) {  // a wave per payload
      const int32_t* row = a.pay[base + g].row;
      const int lo = wave_lower_bound(row + HEADER, row_count(row, a.k), (int)t0);
      if ((tid & 63) == 0) lo_l[g] = lo;
    }
    __syncthreads();
    // every payload's first entry for this thread, all loads in flight before the first use
    int pj[FOLD_GROUP], pc[FOLD_GROUP];
    float pv[FOLD_GROUP];
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) {
      pj[g] = t_end;
      pv[g] = 0.0f;
      pc[g] = 0;
      if (g < gs) {
        const int32_t* row = a.pay[base + g].row;
        pc[g] = row_count(row, a.k);
        const int e = lo_l[g] + tid;
        if (e < pc[g]) {
          pj[g] = row[HEADER + e];
          pv[g] = reinterpret_cast<const float*>(row + HEADER + a.cap)[e];
        }
      }
    }
#pragma unroll
    for (int g = 0; g < FOLD_GROUP; ++g) {
      if (g < gs) {  // uniform
        const StcPay p = a.pay[base + g];
        const int32_t* idx = p.row + HEADER;
        const float* val = reinterpret_cast<const float*>(p.row + HEADER + a.cap);
        int j = pj[g];
        float v = pv[g];
        int e = lo_l[g] + tid;
        while (j < t_end) {  // ascending: the first entry past the tile ends this thread's walk
          const uint32_t jj = (uint32_t)(j - (int)t0);
          if (jj < (uint32_t)tlen) {  // below the tile (unsorted data) or outside [0, n): skipped
            const float term = v * p.w;
            tot_l[jj] = tot_l[jj] + term;
          }
          e += FOLD_THREADS;
          if (e >= pc[g]) break;
          j = idx[e];
          v = val[e];
        }
        __syncthreads();  // the next payload may name the same elements
      }
    }
  }
  __syncthreads();
  const bool vec = aligned16(a.r_s);
  for (int q = tid * 4; q < tlen; q += FOLD_THREADS * 4) {
    if (vec && q + 4 <= tlen) {
      const float4 rv = *reinterpret_cast<const float4*>(a.r_s + t0 + q);
      const float4 tv = *reinterpret_cast<const float4*>(tot_l + q);
      *reinterpret_cast<float4*>(a.r_s + t0 + q) =
          make_float4(rv.x + tv.x, rv.y + tv.y, rv.z + tv.z, rv.w + tv.w);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (q + e < tlen) a.r_s[t0 + q + e] = a.r_s[t0 + q + e] + tot_l[q + e];
    }
  }
}

// ---- apply --------------------------------------------------------------------------------------
struct ApplyArgs {
  float* const* tab;
  int64_t n;
  int k;
  int64_t cap;
  const int32_t* row;
};

__global__ void __launch_bounds__(APPLY_THREADS) stc_apply_kernel(const ApplyArgs a) {
  float* x = a.tab[blockIdx.y];
  const int cnt = row_count(a.row, a.k);
  const int32_t* idx = a.row + HEADER;
  const float* val = reinterpret_cast<const float*>(a.row + HEADER + a.cap);
  for (int64_t e = (int64_t)blockIdx.x * APPLY_THREADS + threadIdx.x; e < cnt;
       e += (int64_t)gridDim.x * APPLY_THREADS) {
    const int j = idx[e];
    if ((uint32_t)j < (uint64_t)a.n) x[j] = x[j] + val[e];  // unique indices: no atomics
  }
}

}  // namespace

extern "C" int64_t dpz_stc_chunk_elems(void) { return CHUNK; }
extern "C" int64_t dpz_stc_tile_elems(void) { return TILE; }

extern "C" size_t dpz_stc_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * dpz::node_ws(n).total;
}

extern "C" int dpz_stc_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, void* ws,
                                    size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || n < 1 || k < 1 || k > n || !node_table || !ws) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 3u))
    return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_stc_encode_workspace_bytes(m, n)) return DPZ_ERR_WORKSPACE;
  StcArgs a;
  a.tab = static_cast<const StcNode*>(node_table);
  a.k = (uint32_t)k;
  a.cap = up4(k);
  return dpz::select_nodes<StcPolicy>(m, a, n, ws, static_cast<hipStream_t>(stream));
}

extern "C" int dpz_stc_server_fold(int n_payloads, const void* table, const void* host_table,
                                   int64_t n, int64_t k, float* r_s, dpz_stream_t stream) {
  if (n_payloads < 1 || n < 1 || k < 1 || k > n || !table || !host_table || !r_s)
    return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(r_s) & 3u) || (reinterpret_cast<uintptr_t>(table) & 7u))
    return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS) return DPZ_ERR_UNSUPPORTED;
  const StcPay* h = static_cast<const StcPay*>(host_table);
  const uintptr_t s_lo = reinterpret_cast<uintptr_t>(r_s);
  const uintptr_t s_hi = s_lo + (uintptr_t)n * sizeof(float);
  const uintptr_t row_bytes = (uintptr_t)(HEADER + 2 * up4(k)) * 4;
  for (int p = 0; p < n_payloads; ++p) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(h[p].row);
    if (!lo || (lo & 3u) || !std::isfinite(h[p].w)) return DPZ_ERR_ARG;
    // r_s is written while the rows are read
    if (lo < s_hi && s_lo < lo + row_bytes) return DPZ_ERR_ARG;
  }
  FoldArgs a;
  a.pay = static_cast<const StcPay*>(table);
  a.n_pay = n_payloads;
  a.n = n;
  a.k = (int)k;
  a.cap = up4(k);
  a.r_s = r_s;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = (unsigned)((n + TILE - 1) / TILE);
  DPZ_TIMED(DPZ_KT_FOLD, st, stc_fold_kernel<<<grid, FOLD_THREADS, 0, st>>>(a));
  return DPZ_OK;
}

extern "C" int dpz_stc_apply_nodes(int m, const void* table, int64_t n, int64_t k,
                                   const int32_t* row, dpz_stream_t stream) {
  if (m < 1 || n < 1 || k < 1 || k > n || !table || !row) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(row) & 3u) || (reinterpret_cast<uintptr_t>(table) & 7u))
    return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  ApplyArgs a;
  a.tab = static_cast<float* const*>(table);
  a.n = n;
  a.k = (int)k;
  a.cap = up4(k);
  a.row = row;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)std::min<int64_t>(1024, (k + APPLY_THREADS - 1) / APPLY_THREADS),
                  (unsigned)m);
  DPZ_TIMED(DPZ_KT_SCATTER, st, stc_apply_kernel<<<grid, APPLY_THREADS, 0, st>>>(a));
  return DPZ_OK;
}
