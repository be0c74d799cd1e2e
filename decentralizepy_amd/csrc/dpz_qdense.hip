// Fused unpack-and-fold of the quantised full-model rounds (decentralizepy_amd/gossip_quant.py):
// dpz_dense.hip's fold of a round's nodes in one launch, with the sources read as packed
// quantised rows [count (int64), status, 0 | the info record | body] instead of fp32 rows.  A
// source's field width w and scale come from its row's header on the device (wave-uniform reads,
// different sources may differ); its value i is the MSB-first w-bit field at stream bits
// [i w, (i+1) w), decoded as dpz_quant_decode decodes it (dpz_quant.h quant_value).
// The receiver's own term is its fp32 model.  The fp32 order is the dense fold's:
//   t = fl(v_0 w_0);  t = fl(t + fl(v_i w_i)) in list order;  out = fl(t + fl(local w_self)),
// products and sums rounded separately (-ffp-contract=off); an empty list copies the own row.
//
//  - staged: a workgroup owns a column tile; each thread decodes its 4-element column of EVERY
//    source row into LDS once as fp32, then walks every receiver's list as dense_staged_kernel
//    does (a thread reads back only what it wrote: no barrier).  A tile is a multiple of 32
//    elements, so it starts on a dword boundary of every body whatever w is.
//  - direct: grid = tiles x receivers, each receiver unpacks its senders' fields.
// Both first read the guard words: if any is nonzero every out row becomes a bitwise copy of its
// own row, so a double-buffered caller can swap unconditionally while the round changes no model.
#include "dpz_quant.h"

namespace {

using namespace dpz;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int DIRECT_THREADS = 256;

// one receiver: 4 64-bit words of the table
struct QRecv {
  float* out;
  const float* own;
  float w_self;
  int32_t pad;
  int32_t start;  // its list: entries [start, start + count)
  int32_t count;
};
static_assert(sizeof(QRecv) == 32, "4 64-bit words");

struct QEntry {
  int32_t src;
  float w;
};
static_assert(sizeof(QEntry) == 8, "one 64-bit word");

struct QArgs {
  const uint32_t* const* srcs;  // n_src packed rows
  const QRecv* recv;            // m receivers
  const QEntry* ent;            // n_entries list entries
  int64_t n;
  int64_t cap_dwords;  // body dwords every source row holds
  int n_src;
  int m;
  const int32_t* guard;
  int64_t guard_n;
};

struct F4 {
  float v[4];
};

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

__device__ __forceinline__ int clamp_src(int32_t s, int n_src) {
  return (int)min((uint32_t)s, (uint32_t)(n_src - 1));
}

// a source row's header: the same for every lane.  w is clamped to the widths a stream can have
// and the readable dwords to the row's body, so that no header can send a read outside the row
struct QSrc {
  const uint32_t* body;
  int64_t ndw;
  float scale;
  int w;
};

__device__ __forceinline__ QSrc load_src(const uint32_t* __restrict__ row, int64_t n,
                                         int64_t cap_dwords) {
  QSrc s;
  s.w = min(max((int)row[QROW_INFO + QI_W], 2), 32);
  s.scale = __uint_as_float(row[QROW_INFO + QI_SCALE]);
  s.ndw = min((n * s.w + 31) / 32, cap_dwords);
  s.body = row + QROW_BODY;
  return s;
}

// The thread's column [q, q + 4) of a source in two steps, so that a group of sources has all
// its loads in flight before the first field is extracted.  q is a multiple of 4: the 4 fields
// are the 4 w bits from stream bit q w on, at most 5 dwords (31 + 128 bits); a dword outside the
// body reads as 0.
struct QRaw {
  uint32_t r0, r1, r2, r3, r4;
  int sh;  // the first field's bit in r0
  int w;
  float scale;
};

__device__ __forceinline__ QRaw load_raw(const QSrc& s, int64_t q) {
  QRaw a;
  const int64_t t = q * s.w, d = t >> 5;
  a.sh = (int)(t & 31);
  a.w = s.w;
  a.scale = s.scale;
  a.r0 = d < s.ndw ? s.body[d] : 0u;
  a.r1 = d + 1 < s.ndw ? s.body[d + 1] : 0u;
  a.r2 = d + 2 < s.ndw ? s.body[d + 2] : 0u;
  a.r3 = d + 3 < s.ndw ? s.body[d + 3] : 0u;
  a.r4 = d + 4 < s.ndw ? s.body[d + 4] : 0u;
  return a;
}

// dword k of the window (hi : lo) shifted right by sft bits, 0 <= sft <= 32
__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int sft) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sft);
}

// The fields as quant_int / quant_value give them; zero past the row's end.  The window is
// shifted down to its first field, then by w after each field: no register is indexed at run time.
__device__ __forceinline__ F4 decode_raw(const QRaw& a, int64_t q, int64_t n) {
  const uint32_t mask = a.w == 32 ? 0xFFFFFFFFu : ((1u << a.w) - 1u);
  const uint32_t half = (1u << (a.w - 1)) - 1u;
  uint32_t r0 = funnel(a.r1, a.r0, a.sh), r1 = funnel(a.r2, a.r1, a.sh);
  uint32_t r2 = funnel(a.r3, a.r2, a.sh), r3 = funnel(a.r4, a.r3, a.sh);  // 4 w <= 128 bits
  F4 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int32_t qv = (int32_t)((__brev(r0 & mask) >> (32 - a.w)) - half);
    r.v[i] = q + i < n ? quant_value(qv, a.w, a.scale) : 0.0f;
    r0 = funnel(r1, r0, a.w);
    r1 = funnel(r2, r1, a.w);
    r2 = funnel(r3, r2, a.w);
    r3 = funnel(0u, r3, a.w);
  }
  return r;
}

// sources a thread keeps in flight, 5 dword loads each: the staged kernel's occupancy is set by
// its LDS (2 workgroups per CU), the direct kernel's by its registers
constexpr int STAGE_GROUP = 8;
constexpr int DIRECT_GROUP = 4;

// a status word of this round is nonzero: uniform over the block (every thread must call)
__device__ __forceinline__ bool guard_tripped(const QArgs& a) {
  int bad = 0;
  for (int64_t i = threadIdx.x; i < a.guard_n; i += blockDim.x) bad |= a.guard[i] != 0;
  return __syncthreads_or(bad) != 0;
}

template <bool VEC>
__global__ void __launch_bounds__(256)
qdense_staged_kernel(const QArgs a) {
  extern __shared__ float4 lds[];  // [n_src][blockDim.x]
  const int tid = threadIdx.x, nt = blockDim.x;
  const bool bad = guard_tripped(a);
  const int64_t q = ((int64_t)blockIdx.x * nt + tid) * 4;
  if (q >= a.n) return;  // no barrier below: a thread reads only the slots it wrote
  const bool full = q + 4 <= a.n;
  if (bad) {
    for (int j = 0; j < a.m; ++j) {
      const QRecv rc = a.recv[j];
      store_col<VEC>(rc.out, q, a.n, full, load_col<VEC>(rc.own, q, a.n, full));
    }
    return;
  }
  for (int g = 0; g < a.n_src; g += STAGE_GROUP) {
    QRaw raw[STAGE_GROUP];
    const int cnt = min(a.n_src - g, STAGE_GROUP);  // uniform over the block
#pragma unroll
    for (int i = 0; i < STAGE_GROUP; ++i) {  // past the last source: the last one again, unused
      raw[i] = load_raw(load_src(a.srcs[min(g + i, a.n_src - 1)], a.n, a.cap_dwords), q);
    }
#pragma unroll
    for (int i = 0; i < STAGE_GROUP; ++i)
      if (cnt == STAGE_GROUP || i < cnt) {
        const F4 r = decode_raw(raw[i], q, a.n);
        lds[(g + i) * nt + tid] = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
      }
  }
  for (int j = 0; j < a.m; ++j) {  // uniform over the block
    const QRecv rc = a.recv[j];
    const F4 l = load_col<VEC>(rc.own, q, a.n, full);
    F4 t = l;  // nothing received: the model stays, bit for bit
    if (rc.count > 0) {
      const QEntry* __restrict__ e = a.ent + rc.start;
      for (int p = 0; p < rc.count; ++p) {
        const float w = e[p].w;
        const float4 v = lds[clamp_src(e[p].src, a.n_src) * nt + tid];
        const float term[4] = {v.x * w, v.y * w, v.z * w, v.w * w};
#pragma unroll
        for (int i = 0; i < 4; ++i) t.v[i] = p ? t.v[i] + term[i] : term[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) t.v[i] = t.v[i] + l.v[i] * rc.w_self;
    }
    store_col<VEC>(rc.out, q, a.n, full, t);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(DIRECT_THREADS)
qdense_direct_kernel(const QArgs a) {
  const bool bad = guard_tripped(a);
  const QRecv rc = a.recv[blockIdx.y];
  const int64_t q = ((int64_t)blockIdx.x * DIRECT_THREADS + threadIdx.x) * 4;
  if (q >= a.n) return;
  const bool full = q + 4 <= a.n;
  const F4 l = load_col<VEC>(rc.own, q, a.n, full);
  F4 t = l;
  if (rc.count > 0 && !bad) {
    const QEntry* __restrict__ e = a.ent + rc.start;
    for (int g = 0; g < rc.count; g += DIRECT_GROUP) {
      QRaw raw[DIRECT_GROUP];
      float w[DIRECT_GROUP];
      const int cnt = min(rc.count - g, DIRECT_GROUP);  // uniform over the block
#pragma unroll
      for (int i = 0; i < DIRECT_GROUP; ++i) {  // past the list's end: its last entry again, unused
        const QEntry en = e[min(g + i, rc.count - 1)];
        w[i] = en.w;
        raw[i] = load_raw(load_src(a.srcs[clamp_src(en.src, a.n_src)], a.n, a.cap_dwords), q);
      }
#pragma unroll
      for (int i = 0; i < DIRECT_GROUP; ++i)
        if (cnt == DIRECT_GROUP || i < cnt) {
          const F4 v = decode_raw(raw[i], q, a.n);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float term = v.v[c] * w[i];
            t.v[c] = (g + i) ? t.v[c] + term : term;
          }
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) t.v[c] = t.v[c] + l.v[c] * rc.w_self;
  }
  store_col<VEC>(rc.out, q, a.n, full, t);
}

// [p, p + lp bytes) and [r, r + lr bytes) share a byte
bool bytes_overlap(const void* p, uintptr_t lp, const void* r, uintptr_t lr) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(r);
  return a < b + lr && b < a + lp;
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int64_t dpz_qdense_tile_elems(int n_src) { return dpz_dense_tile_elems(n_src); }

// Auto: dpz_dense_auto_mode's rule (a tile fits, staging at least halves the row reads, at least
// 384 tiles); the figures measured for this kernel are in DESIGN.md 5.0e.
extern "C" int dpz_qdense_auto_mode(int n_src, int64_t row_reads, int64_t n) {
  return dpz_dense_auto_mode(n_src, row_reads, n);
}

extern "C" int dpz_qdense_average_nodes(int m, const void* fold_table, const void* host_table,
                                        int64_t n_entries, int n_src, int64_t n,
                                        int64_t cap_dwords, int mode, const int32_t* guard,
                                        int64_t guard_n, dpz_stream_t stream) {
  if (m < 1 || n < 1 || n_src < 1 || n_entries < 0 || cap_dwords < 1 || !fold_table ||
      !host_table)
    return DPZ_ERR_ARG;
  if (mode < DPZ_DENSE_AUTO || mode > DPZ_DENSE_DIRECT) return DPZ_ERR_ARG;
  if (guard_n < 0 || (guard_n > 0 && !guard) || !aligned4(guard)) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  if (cap_dwords > (n * 32 + 31) / 32) return DPZ_ERR_ARG;  // no stream is wider than 32 bits
  // the table: n_src packed-row pointers, m receivers, n_entries list entries, in 64-bit words
  const char* hb = static_cast<const char*>(host_table);
  const uint32_t* const* h_srcs = reinterpret_cast<const uint32_t* const*>(hb);
  const QRecv* h_recv = reinterpret_cast<const QRecv*>(hb + sizeof(void*) * (size_t)n_src);
  const QEntry* h_ent = reinterpret_cast<const QEntry*>(h_recv + m);
  const uintptr_t row_bytes = 4 * ((uintptr_t)QROW_BODY + (uintptr_t)cap_dwords);
  const uintptr_t len = (uintptr_t)n * sizeof(float);
  for (int s = 0; s < n_src; ++s)
    if (!h_srcs[s] || !aligned4(h_srcs[s])) return DPZ_ERR_ARG;
  bool vec = true;
  int64_t reads = 0;
  for (int j = 0; j < m; ++j) {
    const QRecv& r = h_recv[j];
    if (!r.out || !r.own || !aligned4(r.out) || !aligned4(r.own)) return DPZ_ERR_ARG;
    if (r.count < 0 || r.start < 0 || (int64_t)r.start + r.count > n_entries) return DPZ_ERR_ARG;
    for (int p = 0; p < r.count; ++p) {
      const int32_t s = h_ent[r.start + p].src;
      if (s < 0 || s >= n_src) return DPZ_ERR_ARG;
    }
    // receivers write while others still read: no out row may touch a packed row, an own row
    // (its own included) or another out row
    for (int s = 0; s < n_src; ++s)
      if (bytes_overlap(r.out, len, h_srcs[s], row_bytes)) return DPZ_ERR_ARG;
    for (int i = 0; i < m; ++i)
      if (bytes_overlap(r.out, len, h_recv[i].own, len)) return DPZ_ERR_ARG;
    for (int i = 0; i < j; ++i)
      if (bytes_overlap(r.out, len, h_recv[i].out, len)) return DPZ_ERR_ARG;
    vec = vec && aligned16(r.out) && aligned16(r.own);
    reads += (int64_t)r.count + 1;
  }
  const int64_t tile = dpz_qdense_tile_elems(n_src);
  if (mode == DPZ_DENSE_STAGED && tile == 0) return DPZ_ERR_UNSUPPORTED;
  const bool staged = mode == DPZ_DENSE_STAGED ||
                      (mode == DPZ_DENSE_AUTO &&
                       dpz_qdense_auto_mode(n_src, reads, n) == DPZ_DENSE_STAGED);
  const char* db = static_cast<const char*>(fold_table);
  QArgs a;
  a.srcs = reinterpret_cast<const uint32_t* const*>(db);
  a.recv = reinterpret_cast<const QRecv*>(db + sizeof(void*) * (size_t)n_src);
  a.ent = reinterpret_cast<const QEntry*>(a.recv + m);
  a.n = n;
  a.cap_dwords = cap_dwords;
  a.n_src = n_src;
  a.m = m;
  a.guard = guard;
  a.guard_n = guard_n;
  hipStream_t st = (hipStream_t)stream;
  if (staged) {
    const int threads = (int)(tile / 4);
    const int64_t blocks = (n + tile - 1) / tile;
    const size_t lds = (size_t)n_src * (size_t)tile * sizeof(float);
    if (vec) qdense_staged_kernel<true><<<(unsigned)blocks, threads, lds, st>>>(a);
    else qdense_staged_kernel<false><<<(unsigned)blocks, threads, lds, st>>>(a);
  } else {
    const int64_t blocks = ((n + 3) / 4 + DIRECT_THREADS - 1) / DIRECT_THREADS;
    const dim3 grid((unsigned)blocks, (unsigned)m);
    if (vec) qdense_direct_kernel<true><<<grid, DIRECT_THREADS, 0, st>>>(a);
    else qdense_direct_kernel<false><<<grid, DIRECT_THREADS, 0, st>>>(a);
  }
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}
