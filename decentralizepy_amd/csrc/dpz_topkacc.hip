// A top-k round with accumulated changes (decentralizepy_amd/gossip_topkacc.py; reference
// sharing/PartialModel.py:305-331 `_pre_step` with accumulation = True, :188-255 the selection,
// the counter and the rewind, :333-353 `_post_step`).
//
// dpz_topkacc_encode_nodes: the exact-k selection of m nodes, the node in the grid's second
// dimension.  The pass structure is that of dpz_stc_encode_nodes (a self-contained sibling: a
// control block, histograms and chunk counts per node).  The first histogram pass forms the key
// vector c once from x, x0 and acc (12 N bytes read) and stores it (4 N written) into the node's
// key row:
//   DPZ_ACC_ACCUMULATE  c = fl(acc + fl(x - x0)), the key row is acc itself: the reference's
//                       `accumulated_changes += change`, stored in place (every group of 4
//                       elements belongs to exactly one thread of the grid);
//   DPZ_ACC_ADD         c = fl(fl(x - x0) + acc), the key row is a scratch row of the caller's;
//                       acc is not written before the rewind.
// Every later pass reads the key row alone (4 N).  Three histogram passes (10/11/10 bits of the
// key |c|), each followed by a 1-block-per-node resolve, give T, the k-th largest key, and the
// number of ties at T to take; a count pass counts key > T and key == T per chunk, a
// 1-block-per-node scan gives every chunk its output offset and its share of the ties in index
// order (ties go to the lowest indices), and the ordered compaction writes idx / val = x[i]
// ascending into the node's row, counter[i] += 1 (a plain store: the element has one owner) and
// +0 into acc[i].  Exactly k entries per row; x and x0 are never written.
//
// dpz_topkacc_post_nodes: `_post_step` with accumulate_averaging_changes of m nodes in one launch
// over the same node table: acc = fl(acc + fl(x - x0)), x the averaged model and x0 the model the
// round started from.
#include <algorithm>

#include "dpz_common.h"
#include "dpz_topk.h"

namespace {

using dpz::aligned16;
using dpz::block_excl_scan;
using dpz::block_excl_scan64;
using dpz::key_of;
using dpz::TopkCtrl;

constexpr int64_t MAX_ELEMS = int64_t(1) << 31;
constexpr int HEADER = 4;                 // int32 words in front of a row's idx / val slots
constexpr int CHUNK = dpz::EX_CHUNK;      // elements per block of the count / compaction passes
constexpr int HIST_BLOCKS = dpz::EX_HIST_BLOCKS;
constexpr int POST_BLOCKS = 1024;

__host__ __device__ __forceinline__ int64_t up4(int64_t v) { return (v + 3) & ~int64_t(3); }

struct AccNode {  // 6 64-bit words of the node table
  const float* x;
  const float* x0;
  float* acc;
  float* key;        // DPZ_ACC_ADD: n floats of scratch; DPZ_ACC_ACCUMULATE: unused (acc is the row)
  int32_t* counter;  // or NULL
  int32_t* row;      // [count lo, count hi, status, 0 | up4(k) idx | up4(k) val]
};
static_assert(sizeof(AccNode) == 48, "6 64-bit words");

struct EncWs {  // one node's share of the workspace
  size_t ctrl, hist, bgt, beq, boff, beqb, total;
  int64_t nblk;
};

EncWs enc_ws(int64_t n) {
  EncWs L;
  L.nblk = std::max<int64_t>(1, (n + CHUNK - 1) / CHUNK);
  size_t o = 0;
  L.ctrl = o; o += dpz::align256(sizeof(TopkCtrl));
  L.hist = o; o += dpz::align256(4096 * 4);
  L.bgt = o; o += dpz::align256((size_t)L.nblk * 4);
  L.beq = o; o += dpz::align256((size_t)L.nblk * 4);
  L.boff = o; o += dpz::align256((size_t)L.nblk * 4);
  L.beqb = o; o += dpz::align256((size_t)L.nblk * 4);
  L.total = o;
  return L;
}

struct EncArgs {
  const AccNode* tab;
  char* ws;
  size_t per_node;
  EncWs L;
  int64_t n;
  uint32_t k;
  int64_t cap;
  int add;  // DPZ_ACC_ADD: the key row is nd.key; else acc
};

__device__ __forceinline__ float* key_row(const AccNode& nd, int add) {
  return add ? nd.key : nd.acc;
}

__device__ __forceinline__ int count4(int64_t i0, int64_t n) {
  const int64_t rem = n - i0;
  return rem >= 4 ? 4 : (rem > 0 ? (int)rem : 0);
}

// c = the key row's 4 elements from i0 (zeros past n); returns how many lie inside
__device__ __forceinline__ int load_c4(const float* __restrict__ r, int64_t i0, int64_t n,
                                       bool vec, float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 q = *reinterpret_cast<const float4*>(r + i0);
    c[0] = q.x, c[1] = q.y, c[2] = q.z, c[3] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) c[e] = e < cnt ? r[i0 + e] : 0.0f;
  }
  return cnt;
}

// c = fl(acc + fl(x - x0)) of the 4 elements from i0, stored into the key row
__device__ __forceinline__ int form_c4(const AccNode& nd, float* __restrict__ kr, int64_t i0,
                                       int64_t n, bool vec, float c[4]) {
  const int cnt = count4(i0, n);
  if (vec && cnt == 4) {
    const float4 a = *reinterpret_cast<const float4*>(nd.x + i0);
    const float4 b = *reinterpret_cast<const float4*>(nd.x0 + i0);
    const float4 q = *reinterpret_cast<const float4*>(nd.acc + i0);
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    c[0] = q.x + d0, c[1] = q.y + d1, c[2] = q.z + d2, c[3] = q.w + d3;
    *reinterpret_cast<float4*>(kr + i0) = make_float4(c[0], c[1], c[2], c[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      c[e] = 0.0f;
      if (e < cnt) {
        const float d = nd.x[i0 + e] - nd.x0[i0 + e];
        c[e] = nd.acc[i0 + e] + d;
        kr[i0 + e] = c[e];
      }
    }
  }
  return cnt;
}

template <int P>
__global__ void __launch_bounds__(256) topkacc_hist_kernel(const EncArgs a) {
  constexpr int NB = (P == 1) ? 2048 : 1024;
  constexpr int HOFF = (P == 0) ? 0 : (P == 1 ? 1024 : 3072);
  __shared__ uint32_t h[NB];
  for (int b = threadIdx.x; b < NB; b += 256) h[b] = 0;
  __syncthreads();
  const AccNode nd = a.tab[blockIdx.y];
  float* kr = key_row(nd, a.add);
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const uint32_t pfx = (P == 0) ? 0u : reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->prefix;
  uint32_t* ghist = reinterpret_cast<uint32_t*>(ws + a.L.hist) + HOFF;
  const bool vec = aligned16(kr) &&
                   (P != 0 || (aligned16(nd.x) && aligned16(nd.x0) && aligned16(nd.acc)));
  const int64_t ngroups = (a.n + 3) >> 2;
  // every group of 4 belongs to exactly one thread of the grid: c is formed and stored once
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    float c[4];
    const int cnt = (P == 0) ? form_c4(nd, kr, g * 4, a.n, vec, c)
                             : load_c4(kr, g * 4, a.n, vec, c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t kk = key_of(c[e]);
        if (P == 0) {
          atomicAdd(&h[kk >> 21], 1u);
        } else if (P == 1) {
          if ((kk >> 21) == (pfx >> 21)) atomicAdd(&h[(kk >> 10) & 2047u], 1u);
        } else {
          if ((kk >> 10) == (pfx >> 10)) atomicAdd(&h[kk & 1023u], 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NB; b += 256) {
    const uint32_t v = h[b];
    if (v) atomicAdd(&ghist[b], v);
  }
}

// One block of 1024 threads per node: the digit that holds the krem-th largest key.
template <int P>
__global__ void __launch_bounds__(1024) topkacc_resolve_kernel(const EncArgs a) {
  constexpr int NB = (P == 1) ? 2048 : 1024;
  constexpr int HOFF = (P == 0) ? 0 : (P == 1 ? 1024 : 3072);
  constexpr int SH = (P == 0) ? 21 : (P == 1 ? 10 : 0);
  constexpr int PER = NB / 1024;
  __shared__ uint32_t wsum[16];
  char* ws = a.ws + (size_t)blockIdx.x * a.per_node;
  TopkCtrl* ctrl = reinterpret_cast<TopkCtrl*>(ws + a.L.ctrl);
  const uint32_t* ghist = reinterpret_cast<const uint32_t*>(ws + a.L.hist) + HOFF;
  const uint32_t krem = (P == 0) ? a.k : ctrl->krem;
  const uint32_t pfx = (P == 0) ? 0u : ctrl->prefix;
  __syncthreads();  // every thread has read ctrl before one of them rewrites it
  uint32_t hv[PER];
  uint32_t local = 0;
#pragma unroll
  for (int q = 0; q < PER; ++q) {  // descending bins
    hv[q] = ghist[NB - 1 - (threadIdx.x * PER + q)];
    local += hv[q];
  }
  uint32_t tot;
  uint32_t before = block_excl_scan(local, wsum, &tot);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (before < krem && krem <= before + hv[q]) {
      const uint32_t d = NB - 1 - (threadIdx.x * PER + q);
      ctrl->prefix = pfx | (d << SH);
      ctrl->krem = krem - before;  // after the last pass: the ties at T to take
    }
    before += hv[q];
  }
}

// key > T in the low half, key == T in the high half: a chunk holds 8192 < 2^16 elements
__device__ __forceinline__ uint32_t count_gt_eq(const float c[4], int cnt, uint32_t T) {
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < cnt) {
      const uint32_t kk = key_of(c[e]);
      v += (kk > T ? 1u : 0u) + (kk == T ? 0x10000u : 0u);
    }
  }
  return v;
}
static_assert(CHUNK < 0x10000, "two 16-bit counts per chunk");

__global__ void __launch_bounds__(256) topkacc_count_kernel(const EncArgs a) {
  __shared__ uint32_t wsum[16];
  const AccNode nd = a.tab[blockIdx.y];
  const float* kr = key_row(nd, a.add);
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const uint32_t T = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->prefix;
  const bool vec = aligned16(kr);
  const int64_t lo = (int64_t)blockIdx.x * CHUNK;
  uint32_t v = 0;
  for (int r = 0; r < CHUNK / 1024; ++r) {
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    if (i0 >= a.n) break;
    float c[4];
    const int cnt = load_c4(kr, i0, a.n, vec, c);
    v += count_gt_eq(c, cnt, T);
  }
  uint32_t tot;
  block_excl_scan(v, wsum, &tot);
  if (threadIdx.x == 0) {
    reinterpret_cast<uint32_t*>(ws + a.L.bgt)[blockIdx.x] = tot & 0xFFFFu;
    reinterpret_cast<uint32_t*>(ws + a.L.beq)[blockIdx.x] = tot >> 16;
  }
}

// One block of 1024 threads per node: every chunk's output offset and the ties before it (its
// share of the allotment follows: ties go to the lowest indices), and the row's header.
__global__ void __launch_bounds__(1024) topkacc_scan_kernel(const EncArgs a) {
  __shared__ uint64_t wsum[16];
  const AccNode nd = a.tab[blockIdx.x];
  char* ws = a.ws + (size_t)blockIdx.x * a.per_node;
  const uint64_t ties = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl)->krem;
  const uint32_t* bgt = reinterpret_cast<const uint32_t*>(ws + a.L.bgt);
  const uint32_t* beq = reinterpret_cast<const uint32_t*>(ws + a.L.beq);
  uint32_t* boff = reinterpret_cast<uint32_t*>(ws + a.L.boff);
  uint32_t* beqb = reinterpret_cast<uint32_t*>(ws + a.L.beqb);
  uint64_t carry_eq = 0, carry_off = 0;
  for (int64_t base = 0; base < a.L.nblk; base += 1024) {
    const int64_t b = base + threadIdx.x;
    const uint64_t gt = b < a.L.nblk ? bgt[b] : 0;
    const uint64_t eq = b < a.L.nblk ? beq[b] : 0;
    uint64_t te;
    const uint64_t eqb = block_excl_scan64(eq, wsum, &te) + carry_eq;
    uint64_t take = 0;
    if (ties > eqb) take = (ties - eqb) < eq ? (ties - eqb) : eq;
    uint64_t ts;
    const uint64_t off = block_excl_scan64(gt + take, wsum, &ts) + carry_off;
    if (b < a.L.nblk) {
      boff[b] = (uint32_t)off;
      beqb[b] = (uint32_t)(eqb < ties ? eqb : ties);
    }
    carry_eq += te;
    carry_off += ts;
  }
  if (threadIdx.x == 0) {  // exactly k are selected; k < 2^31: the int64's high word is 0
    nd.row[0] = (int32_t)a.k;
    nd.row[1] = 0;
    nd.row[2] = 0;
    nd.row[3] = 0;
  }
}

__global__ void __launch_bounds__(256) topkacc_write_kernel(const EncArgs a) {
  __shared__ uint32_t wsum[16];
  const AccNode nd = a.tab[blockIdx.y];
  const float* kr = key_row(nd, a.add);
  char* ws = a.ws + (size_t)blockIdx.y * a.per_node;
  const TopkCtrl* ctrl = reinterpret_cast<const TopkCtrl*>(ws + a.L.ctrl);
  const uint32_t T = ctrl->prefix;
  const uint32_t ties = ctrl->krem;
  const uint32_t off0 = reinterpret_cast<const uint32_t*>(ws + a.L.boff)[blockIdx.x];
  const uint32_t eqb = reinterpret_cast<const uint32_t*>(ws + a.L.beqb)[blockIdx.x];
  const uint32_t quota = ties > eqb ? ties - eqb : 0u;
  const bool vec = aligned16(kr);
  int32_t* idx_out = nd.row + HEADER;
  float* val_out = reinterpret_cast<float*>(nd.row + HEADER + a.cap);
  const int64_t lo = (int64_t)blockIdx.x * CHUNK;
  uint32_t gt_run = 0, eq_run = 0;
  for (int r = 0; r < CHUNK / 1024; ++r) {
    if (lo + r * 1024 >= a.n) break;  // uniform
    const int64_t i0 = lo + r * 1024 + threadIdx.x * 4;
    float c[4];
    const int cnt = load_c4(kr, i0, a.n, vec, c);
    uint32_t tot;
    const uint32_t ex = block_excl_scan(count_gt_eq(c, cnt, T), wsum, &tot);
    uint32_t g = gt_run + (ex & 0xFFFFu);
    uint32_t q = eq_run + (ex >> 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const uint32_t kk = key_of(c[e]);
        bool sel = false;
        uint32_t pos = 0;
        if (kk > T) {
          sel = true;
          pos = off0 + g + (q < quota ? q : quota);
          ++g;
        } else if (kk == T) {
          if (q < quota) {
            sel = true;
            pos = off0 + g + q;
          }
          ++q;
        }
        if (sel && pos < a.k) {  // pos < k always; the slot is never written past
          const int64_t i = i0 + e;  // this thread owns element i: plain stores
          idx_out[pos] = (int32_t)i;
          val_out[pos] = nd.x[i];
          if (nd.counter) nd.counter[i] = nd.counter[i] + 1;
          nd.acc[i] = 0.0f;  // the rewind: what was sent is no longer owed
        }
      }
    }
    gt_run += tot & 0xFFFFu;
    eq_run += tot >> 16;
  }
}

// ---- post step ----------------------------------------------------------------------------------
struct PostArgs {
  const AccNode* tab;
  int64_t n;
};

__global__ void __launch_bounds__(256) topkacc_post_kernel(const PostArgs a) {
  const AccNode nd = a.tab[blockIdx.y];
  const bool vec = aligned16(nd.x) && aligned16(nd.x0) && aligned16(nd.acc);
  const int64_t ngroups = (a.n + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < ngroups;
       g += (int64_t)gridDim.x * 256) {
    const int64_t i0 = g * 4;
    const int cnt = count4(i0, a.n);
    if (vec && cnt == 4) {
      const float4 x = *reinterpret_cast<const float4*>(nd.x + i0);
      const float4 b = *reinterpret_cast<const float4*>(nd.x0 + i0);
      const float4 q = *reinterpret_cast<const float4*>(nd.acc + i0);
      const float d0 = x.x - b.x, d1 = x.y - b.y, d2 = x.z - b.z, d3 = x.w - b.w;
      *reinterpret_cast<float4*>(nd.acc + i0) =
          make_float4(q.x + d0, q.y + d1, q.z + d2, q.w + d3);
    } else {
      for (int e = 0; e < cnt; ++e) {
        const float d = nd.x[i0 + e] - nd.x0[i0 + e];
        nd.acc[i0 + e] = nd.acc[i0 + e] + d;
      }
    }
  }
}

}  // namespace

extern "C" int64_t dpz_topkacc_chunk_elems(void) { return CHUNK; }

extern "C" size_t dpz_topkacc_encode_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1) return 0;
  return (size_t)m * enc_ws(n).total;
}

extern "C" int dpz_topkacc_encode_nodes(int m, const void* node_table, int64_t n, int64_t k,
                                        int mode, void* ws, size_t ws_bytes,
                                        dpz_stream_t stream) {
  if (m < 1 || !node_table || !ws) return DPZ_ERR_ARG;
  if (n < 1 || n >= MAX_ELEMS || k < 1 || k > n) return DPZ_ERR_ARG;
  if (mode != DPZ_ACC_ACCUMULATE && mode != DPZ_ACC_ADD) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(node_table) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 3u))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_topkacc_encode_workspace_bytes(m, n)) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  EncArgs a;
  a.tab = static_cast<const AccNode*>(node_table);
  a.ws = static_cast<char*>(ws);
  a.L = enc_ws(n);
  a.per_node = a.L.total;
  a.n = n;
  a.k = (uint32_t)k;
  a.cap = up4(k);
  a.add = mode == DPZ_ACC_ADD;
  // every node's control block and histograms (the chunk arrays are written before they are read)
  DPZ_HIP_TRY(hipMemsetAsync(ws, 0, (size_t)m * a.per_node, st));
  const int64_t groups = (n + 3) / 4;
  const unsigned hb = (unsigned)std::min<int64_t>(HIST_BLOCKS, (groups + 255) / 256);
  const dim3 hgrid(hb, (unsigned)m), cgrid((unsigned)a.L.nblk, (unsigned)m);
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, topkacc_hist_kernel<0><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, topkacc_resolve_kernel<0><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, topkacc_hist_kernel<1><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, topkacc_resolve_kernel<1><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_HIST, st, topkacc_hist_kernel<2><<<hgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_RESOLVE, st, topkacc_resolve_kernel<2><<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_COUNT, st, topkacc_count_kernel<<<cgrid, 256, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_SCAN, st, topkacc_scan_kernel<<<m, 1024, 0, st>>>(a));
  DPZ_TIMED(DPZ_KT_EXACT_WRITE, st, topkacc_write_kernel<<<cgrid, 256, 0, st>>>(a));
  return DPZ_OK;
}

extern "C" int dpz_topkacc_post_nodes(int m, const void* node_table, int64_t n,
                                      dpz_stream_t stream) {
  if (m < 1 || !node_table || n < 1 || n >= MAX_ELEMS) return DPZ_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(node_table) & 7u) return DPZ_ERR_ARG;
  if (m > 65535) return DPZ_ERR_UNSUPPORTED;
  PostArgs a;
  a.tab = static_cast<const AccNode*>(node_table);
  a.n = n;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t groups = (n + 3) / 4;
  const dim3 grid((unsigned)std::min<int64_t>(POST_BLOCKS, (groups + 255) / 256), (unsigned)m);
  DPZ_TIMED(DPZ_KT_ACCUMULATE, st, topkacc_post_kernel<<<grid, 256, 0, st>>>(a));
  return DPZ_OK;
}
