// Dense folds of a round's nodes in one launch (decentralizepy_amd/gossip_epidemic.py): every
// payload is a full model, so a receiver's fold is a weighted sum over whole source rows, in the
// fp32 order of the dense-payload DPZ_FOLD_SELF form of dpz_decode_average (dpz_fold_tile.hip fold_kernel):
//   t = fl(v_0 w_0);  t = fl(t + fl(v_i w_i)) in list order;  out = fl(t + fl(local w_self)),
// products and sums rounded separately (-ffp-contract=off), and a receiver with an empty list
// gets a bitwise copy of its own row.
//
// Two kernels, both one launch for all receivers:
//  - staged: a workgroup owns a column tile; each thread loads its 4-element column of EVERY
//    source row into LDS once (at most STAGE_GROUP loads in flight), then walks every receiver's
//    list reading lds[src][its column].  A thread reads back only what it wrote itself: no
//    barrier, and consecutive lanes sit on consecutive 16-byte slots (no bank conflict); the LDS
//    is a per-thread row file that can be indexed at run time.  Each distinct row is read from
//    memory once per round instead of once per receiver.
//  - direct: grid = tiles x receivers, each receiver streams its sources from global memory.
// The table (source pointers, receivers, list entries) is read with wave-uniform indices.
#include "dpz_common.h"

namespace {

using dpz::aligned16;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int LDS_BYTES = 64 * 1024;  // per workgroup: at least 2 workgroups per CU of 160 KiB
constexpr int STAGE_GROUP = 16;       // float4 loads a thread keeps in flight while staging
constexpr int DIRECT_GROUP = 8;       // ... and while a receiver streams its list
constexpr int DIRECT_THREADS = 256;

// one receiver: 4 64-bit words of the table
struct DenseRecv {
  float* out;
  int32_t self;   // index of its own row among the sources
  float w_self;
  int32_t start;  // its list: entries [start, start + count)
  int32_t count;
  uint64_t pad;
};
static_assert(sizeof(DenseRecv) == 32, "4 64-bit words");

struct DenseEntry {
  int32_t src;
  float w;
};
static_assert(sizeof(DenseEntry) == 8, "one 64-bit word");

struct DenseArgs {
  const float* const* srcs;  // n_src rows
  const DenseRecv* recv;     // m receivers
  const DenseEntry* ent;     // n_entries list entries
  int64_t n;
  int n_src;
  int m;
};

struct F4 {
  float v[4];
};

// a thread's column [q, q + 4) of a row: one 16-byte load on the vector path when it lies whole
// inside the row, element by element otherwise (packed rows, the n % 4 tail)
template <bool VEC>
__device__ __forceinline__ F4 load_col(const float* __restrict__ row, int64_t q, int64_t n,
                                       bool full) {
  F4 r;
  if (VEC && full) {
    const float4 t = *reinterpret_cast<const float4*>(row + q);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = q + i < n ? row[q + i] : 0.0f;
  }
  return r;
}

template <bool VEC>
__device__ __forceinline__ void store_col(float* out, int64_t q, int64_t n, bool full,
                                          const F4& t) {
  if (VEC && full) {
    *reinterpret_cast<float4*>(out + q) = make_float4(t.v[0], t.v[1], t.v[2], t.v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q + i < n) out[q + i] = t.v[i];
  }
}

// the host validated its own copy of the table; an index is clamped all the same so that a
// table that differs from it cannot send a read outside the staged rows
__device__ __forceinline__ int clamp_src(int32_t s, int n_src) {
  return (int)min((uint32_t)s, (uint32_t)(n_src - 1));
}

template <bool VEC>
__global__ void __launch_bounds__(256)
dense_staged_kernel(const DenseArgs a) {
  extern __shared__ float4 lds[];  // [n_src][blockDim.x]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t q = ((int64_t)blockIdx.x * nt + tid) * 4;
  if (q >= a.n) return;  // no barrier below: a thread reads only the slots it wrote
  const bool full = q + 4 <= a.n;
  for (int g = 0; g < a.n_src; g += STAGE_GROUP) {
    F4 r[STAGE_GROUP];
    if (g + STAGE_GROUP <= a.n_src) {  // a whole group: the loads back to back, then the writes
#pragma unroll
      for (int i = 0; i < STAGE_GROUP; ++i) r[i] = load_col<VEC>(a.srcs[g + i], q, a.n, full);
#pragma unroll
      for (int i = 0; i < STAGE_GROUP; ++i)
        lds[(g + i) * nt + tid] = make_float4(r[i].v[0], r[i].v[1], r[i].v[2], r[i].v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < STAGE_GROUP; ++i)
        if (g + i < a.n_src) r[i] = load_col<VEC>(a.srcs[g + i], q, a.n, full);
#pragma unroll
      for (int i = 0; i < STAGE_GROUP; ++i)
        if (g + i < a.n_src)
          lds[(g + i) * nt + tid] = make_float4(r[i].v[0], r[i].v[1], r[i].v[2], r[i].v[3]);
    }
  }
  for (int j = 0; j < a.m; ++j) {  // uniform over the block
    const DenseRecv rc = a.recv[j];
    const float4 l = lds[clamp_src(rc.self, a.n_src) * nt + tid];
    F4 t = {};
    if (rc.count <= 0) {  // nothing received: the model stays, bit for bit
      t.v[0] = l.x, t.v[1] = l.y, t.v[2] = l.z, t.v[3] = l.w;
    } else {
      const DenseEntry* __restrict__ e = a.ent + rc.start;
      for (int p = 0; p < rc.count; ++p) {
        const float w = e[p].w;
        const float4 v = lds[clamp_src(e[p].src, a.n_src) * nt + tid];
        const float term[4] = {v.x * w, v.y * w, v.z * w, v.w * w};
#pragma unroll
        for (int i = 0; i < 4; ++i) t.v[i] = p ? t.v[i] + term[i] : term[i];
      }
      t.v[0] = t.v[0] + l.x * rc.w_self;
      t.v[1] = t.v[1] + l.y * rc.w_self;
      t.v[2] = t.v[2] + l.z * rc.w_self;
      t.v[3] = t.v[3] + l.w * rc.w_self;
    }
    store_col<VEC>(rc.out, q, a.n, full, t);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(DIRECT_THREADS)
dense_direct_kernel(const DenseArgs a) {
  const DenseRecv rc = a.recv[blockIdx.y];
  const int64_t q = ((int64_t)blockIdx.x * DIRECT_THREADS + threadIdx.x) * 4;
  if (q >= a.n) return;
  const bool full = q + 4 <= a.n;
  const F4 l = load_col<VEC>(a.srcs[clamp_src(rc.self, a.n_src)], q, a.n, full);
  F4 t = l;
  if (rc.count > 0) {
    const DenseEntry* __restrict__ e = a.ent + rc.start;
    for (int g = 0; g < rc.count; g += DIRECT_GROUP) {
      F4 r[DIRECT_GROUP];
      float w[DIRECT_GROUP];
      const int cnt = min(rc.count - g, DIRECT_GROUP);  // uniform over the block
#pragma unroll
      for (int i = 0; i < DIRECT_GROUP; ++i)
        if (cnt == DIRECT_GROUP || i < cnt) {
          w[i] = e[g + i].w;
          r[i] = load_col<VEC>(a.srcs[clamp_src(e[g + i].src, a.n_src)], q, a.n, full);
        }
#pragma unroll
      for (int i = 0; i < DIRECT_GROUP; ++i)
        if (cnt == DIRECT_GROUP || i < cnt) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float term = r[i].v[c] * w[i];
            t.v[c] = (g + i) ? t.v[c] + term : term;
          }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) t.v[c] = t.v[c] + l.v[c] * rc.w_self;
  }
  store_col<VEC>(rc.out, q, a.n, full, t);
}

// [p, p + n floats) and [r, r + n floats) share a byte
bool rows_overlap(const float* p, const float* r, int64_t n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(r);
  const uintptr_t len = (uintptr_t)n * sizeof(float);
  return a < b + len && b < a + len;
}

}  // namespace

extern "C" int64_t dpz_dense_tile_elems(int n_src) {
  if (n_src < 1) return 0;
  for (int64_t tile = 1024; tile >= 256; tile >>= 1)
    if ((int64_t)n_src * tile * (int64_t)sizeof(float) <= LDS_BYTES) return tile;
  return 0;
}

// Auto: the staged path when a tile fits, it at least halves the row reads (2 n_src <= the direct
// path's sum(count + 1)) AND the tiles fill the machine: a staged workgroup walks every receiver
// alone, so its grid is the tiles only, against tiles x receivers.  Measured on MI355X (16 nodes,
// 7 senders each, tile 1024, tools/bench_epidemic_round.py): 88 tiles 19.4 against 7.7 us direct,
// 196 tiles 19.9 against 11.1; 391 tiles 25.7 against 35.0, 10,743 tiles 497 against 1021.  The
// threshold sits at the measured winning end: 1.5 workgroups per CU.
constexpr int64_t STAGED_MIN_TILES = 384;

extern "C" int dpz_dense_auto_mode(int n_src, int64_t row_reads, int64_t n) {
  const int64_t tile = dpz_dense_tile_elems(n_src);
  if (tile == 0 || n < 1) return DPZ_DENSE_DIRECT;
  const bool staged = 2 * (int64_t)n_src <= row_reads && (n + tile - 1) / tile >= STAGED_MIN_TILES;
  return staged ? DPZ_DENSE_STAGED : DPZ_DENSE_DIRECT;
}

extern "C" int dpz_dense_average_nodes(int m, const void* fold_table, const void* host_table,
                                       int64_t n_entries, int n_src, int64_t n, int mode,
                                       dpz_stream_t stream) {
  if (m < 1 || n < 1 || n_src < 1 || n_entries < 0 || !fold_table || !host_table)
    return DPZ_ERR_ARG;
  if (mode < DPZ_DENSE_AUTO || mode > DPZ_DENSE_DIRECT) return DPZ_ERR_ARG;
  // the table: n_src source pointers, m receivers, n_entries list entries, in 64-bit words
  const char* hb = static_cast<const char*>(host_table);
  const float* const* h_srcs = reinterpret_cast<const float* const*>(hb);
  const DenseRecv* h_recv = reinterpret_cast<const DenseRecv*>(hb + sizeof(void*) * (size_t)n_src);
  const DenseEntry* h_ent = reinterpret_cast<const DenseEntry*>(h_recv + m);
  bool vec = true;
  for (int s = 0; s < n_src; ++s) {
    if (!h_srcs[s]) return DPZ_ERR_ARG;
    vec = vec && aligned16(h_srcs[s]);
  }
  int64_t reads = 0;
  for (int j = 0; j < m; ++j) {
    const DenseRecv& r = h_recv[j];
    if (!r.out || r.self < 0 || r.self >= n_src) return DPZ_ERR_ARG;
    if (r.count < 0 || r.start < 0 || (int64_t)r.start + r.count > n_entries) return DPZ_ERR_ARG;
    for (int p = 0; p < r.count; ++p) {
      const int32_t s = h_ent[r.start + p].src;
      if (s < 0 || s >= n_src) return DPZ_ERR_ARG;
    }
    // receivers write while others still read: no out row may touch a source row
    for (int s = 0; s < n_src; ++s)
      if (rows_overlap(r.out, h_srcs[s], n)) return DPZ_ERR_ARG;
    for (int i = 0; i < j; ++i)
      if (rows_overlap(r.out, h_recv[i].out, n)) return DPZ_ERR_ARG;
    vec = vec && aligned16(r.out);
    reads += (int64_t)r.count + 1;
  }
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  const int64_t tile = dpz_dense_tile_elems(n_src);
  if (mode == DPZ_DENSE_STAGED && tile == 0) return DPZ_ERR_UNSUPPORTED;
  const bool staged = mode == DPZ_DENSE_STAGED ||
                      (mode == DPZ_DENSE_AUTO &&
                       dpz_dense_auto_mode(n_src, reads, n) == DPZ_DENSE_STAGED);
  const char* db = static_cast<const char*>(fold_table);
  DenseArgs a;
  a.srcs = reinterpret_cast<const float* const*>(db);
  a.recv = reinterpret_cast<const DenseRecv*>(db + sizeof(void*) * (size_t)n_src);
  a.ent = reinterpret_cast<const DenseEntry*>(a.recv + m);
  a.n = n;
  a.n_src = n_src;
  a.m = m;
  hipStream_t st = (hipStream_t)stream;
  if (staged) {
    const int threads = (int)(tile / 4);
    const int64_t blocks = (n + tile - 1) / tile;
    const size_t lds = (size_t)n_src * (size_t)tile * sizeof(float);
    if (vec) dense_staged_kernel<true><<<(unsigned)blocks, threads, lds, st>>>(a);
    else dense_staged_kernel<false><<<(unsigned)blocks, threads, lds, st>>>(a);
  } else {
    const int64_t blocks = ((n + 3) / 4 + DIRECT_THREADS - 1) / DIRECT_THREADS;
    const dim3 grid((unsigned)blocks, (unsigned)m);
    if (vec) dense_direct_kernel<true><<<grid, DIRECT_THREADS, 0, st>>>(a);
    else dense_direct_kernel<false><<<grid, DIRECT_THREADS, 0, st>>>(a);
  }
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}
