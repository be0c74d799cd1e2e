// SubSampling's Bernoulli mask on the device (reference sharing/SubSampling.py:129-182, 235-308):
// a jump-ahead MT19937 that reproduces `torch.rand(n, generator=g) <= alpha` bit for bit, the
// mask-ordered gather `concated[mask]`, and the Metro-Hastings fold over payloads that carry a
// seed instead of an index list.  The GF(2) side (jump polynomials) is dpz_gf2.cpp; the
// identities are stated in dpz_mt.h.
#include <map>
#include <mutex>

#include "dpz_common.h"
#include "dpz_mt.h"

namespace dpz {
namespace mt {

constexpr int THREADS = 640;                    // 10 waves: one lane per state word (624) + 16 idle
constexpr int GROUP = 64;                       // elements per rank_tab entry (two mask words)
constexpr int CHUNK_WORDS = (int)(CHUNK / 32);  // mask words per chunk
constexpr int CHUNK_GROUPS = (int)(CHUNK / GROUP);
constexpr int BITS_PAD = 24;  // the last regeneration's ballots run past the chunk (zero bits)
constexpr int MAX_PAYLOADS = 16;
constexpr int WIN_FRONT = 16, WIN_BACK = 48;  // jump()'s masked reads around the two blocks
constexpr int WIN_WORDS = WIN_FRONT + 2 * N + WIN_BACK;
static_assert(CHUNK_GROUPS <= 2 * 512, "two rank groups per thread of the first 8 waves");

// rank_tab layout: [0, G) the exclusive popcount of each 64-element group inside its chunk,
// [G, G + chunks) the exclusive popcount of each chunk (G = ceil(n / 64)).
__host__ __device__ inline int64_t n_groups(int64_t n) { return (n + GROUP - 1) / GROUP; }
__host__ __device__ inline int64_t n_chunks(int64_t n) { return (n + CHUNK - 1) / CHUNK; }

// ---- device tables: the jump polynomials, copied once to each device that uses them ----------
struct DevTables {
  uint32_t* fine = nullptr;    // [COARSE][POLY_U32], row c = fine_poly(c) (row 0 unused)
  uint32_t* coarse = nullptr;  // [MAX_COARSE][POLY_U32]
  int have_fine = 1, have_coarse = 1;  // rows [1, have) are on the device
};
static std::mutex g_dev_mu;
static std::map<int, DevTables> g_dev_tabs;  // keyed by device ordinal

static int upload_rows(uint32_t* dev, int* have, int need, const uint32_t* (*poly)(int)) {
  for (; *have < need; ++*have) {
    const uint32_t* p = poly(*have);
    if (!p) return DPZ_ERR_INTERNAL;
    DPZ_HIP_TRY(hipMemcpy(dev + (size_t)*have * POLY_U32, p, POLY_U32 * sizeof(uint32_t),
                          hipMemcpyHostToDevice));
  }
  return DPZ_OK;
}

// rows [1, need_fine) / [1, need_coarse) of the tables on the current device
static int device_tables(int need_fine, int need_coarse, DevTables* out) {
  int dev = 0;
  DPZ_HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_dev_mu);
  DevTables& t = g_dev_tabs[dev];
  if (!t.fine) {
    uint32_t* d = nullptr;
    DPZ_HIP_TRY(hipMalloc(&d, (size_t)(COARSE + MAX_COARSE) * POLY_U32 * sizeof(uint32_t)));
    t.fine = d;
    t.coarse = d + (size_t)COARSE * POLY_U32;
  }
  int rc = upload_rows(t.fine, &t.have_fine, need_fine, fine_poly);
  if (rc == DPZ_OK) rc = upload_rows(t.coarse, &t.have_coarse, need_coarse, coarse_poly);
  *out = t;
  return rc;
}

// ---- the generator ---------------------------------------------------------------------------
// nw[0..623] = the 624 raw words after old[0..623].  Three dependent phases (a word needs the new
// word 227 places before it): [0, 227), [227, 454), [454, 624).  Every thread of the block calls.
__device__ __forceinline__ void next_block(const uint32_t* old, uint32_t* nw) {
  const int k = threadIdx.x;
  if (k < N - M) nw[k] = old[k + M] ^ twist(old[k], old[k + 1]);
  __syncthreads();
  if (k >= N - M && k < 2 * (N - M)) nw[k] = nw[k - (N - M)] ^ twist(old[k], old[k + 1]);
  __syncthreads();
  if (k >= 2 * (N - M) && k < N - 1) nw[k] = nw[k - (N - M)] ^ twist(old[k], old[k + 1]);
  if (k == N - 1) nw[k] = nw[M - 1] ^ twist(old[k], nw[0]);
  __syncthreads();
}

// win[0..623] holds a state; on return it holds the state J elements on, g = t^J mod phi:
// word j = XOR over the set bits i of g of x[i + j].  The sequence is generated 624 words at a
// time with two blocks resident (bits i of block b read x[i + j] in blocks b and b + 1); the
// bitmap is uniform over the block, so its words and the masks made from them are scalar.
// `win` has WIN_FRONT words in front and WIN_BACK behind it: a masked read of a bit outside
// [lo, hi) lands there.
__device__ __forceinline__ void jump(uint32_t* win, const uint32_t* __restrict__ poly) {
  const int j = threadIdx.x;  // lanes 624..639 read inside the padding and are discarded
  uint32_t acc = 0;
  next_block(win, win + N);
  for (int b = 0; b * N < DEG; ++b) {
    const int lo = b * N, hi = min(lo + N, DEG);  // bits [lo, hi) of g
    for (int pw = lo >> 5; pw <= (hi - 1) >> 5; ++pw) {
      uint32_t bits = __builtin_amdgcn_readfirstlane(poly[pw]);
      if (pw * 32 < lo) bits &= ~0u << (lo - pw * 32);
      if (pw * 32 + 32 > hi) bits &= ~0u >> (pw * 32 + 32 - hi);
      if (!bits) continue;
      // all 32 reads, each masked by its bit: independent LDS reads and no per-bit scalar
      // chain.  Iterating the set bits (find-first-set, clear, four reads a round) halves the
      // reads but measured 0.574 ms against 0.360 ms for the whole mask at 2^24.
      const uint32_t* src = win + (pw * 32 - lo) + j;
#pragma unroll
      for (int t = 0; t < 32; ++t) acc ^= src[t] & (0u - ((bits >> t) & 1u));
    }
    __syncthreads();
    const uint32_t up = j < N ? win[N + j] : 0u;  // slide: block b + 1 becomes the lower one
    __syncthreads();
    if (j < N) win[j] = up;
    __syncthreads();
    next_block(win, win + N);
  }
  if (j < N) win[j] = acc;
  __syncthreads();
}

__device__ __forceinline__ void init_state(uint32_t seed, uint32_t* st) {
  if (threadIdx.x == 0) {
    uint32_t s = seed;
    st[0] = s;
    for (int i = 1; i < N; ++i) {
      s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i;
      st[i] = s;
    }
  }
  __syncthreads();
}

// coarse launch: block d - 1 writes the state in front of element d * COARSE * CHUNK
__device__ __forceinline__ void coarse_body(uint32_t seed, const uint32_t* __restrict__ coarse,
                                            uint32_t* __restrict__ states) {
  __shared__ uint32_t winbuf[WIN_WORDS];
  uint32_t* win = winbuf + WIN_FRONT;
  const int d = blockIdx.x + 1;
  init_state(seed, win);
  jump(win, coarse + (size_t)d * POLY_U32);
  if (threadIdx.x < N) states[(size_t)d * N + threadIdx.x] = win[threadIdx.x];
}

__global__ void __launch_bounds__(THREADS)
mt_coarse_kernel(uint32_t seed, const uint32_t* __restrict__ coarse, uint32_t* __restrict__ states) {
  coarse_body(seed, coarse, states);
}

// the seeds and thresholds of one launch group of a batch, by value (as FoldArgs' payloads)
constexpr int MASK_GROUP = 64;
struct MaskBatchArgs {
  uint32_t seed[MASK_GROUP];
  int32_t thr[MASK_GROUP];
};

// batch: blockIdx.y is the mask; its states are row blockIdx.y of `states`
__global__ void __launch_bounds__(THREADS)
mt_coarse_batch_kernel(MaskBatchArgs a, const uint32_t* __restrict__ coarse,
                       uint32_t* __restrict__ states, int64_t states_stride) {
  coarse_body(a.seed[blockIdx.y], coarse, states + blockIdx.y * states_stride);
}

// one block per chunk: jump to the chunk's first element, regenerate the state ceil(len / 624)
// times, temper, compare, pack the chunk's mask words and its per-group exclusive popcounts
__device__ __forceinline__ void mask_body(uint32_t seed, int32_t thr, int64_t n,
                                          const uint32_t* __restrict__ fine,
                                          const uint32_t* __restrict__ states,
                                          uint32_t* __restrict__ mask,
                                          int32_t* __restrict__ rank_tab) {
  __shared__ uint32_t winbuf[WIN_WORDS];
  uint32_t* win = winbuf + WIN_FRONT;
  __shared__ uint32_t bits[CHUNK_WORDS + BITS_PAD];
  __shared__ uint32_t wsum[16];
  const int tid = threadIdx.x;
  const int64_t chunk = blockIdx.x;
  const int d = (int)(chunk / COARSE), c = (int)(chunk % COARSE);
  for (int i = tid; i < CHUNK_WORDS + BITS_PAD; i += THREADS) bits[i] = 0;
  if (d) {
    if (tid < N) win[tid] = states[(size_t)d * N + tid];
    __syncthreads();
  } else {
    init_state(seed, win);
  }
  if (c) jump(win, fine + (size_t)c * POLY_U32);

  const int64_t base = chunk * CHUNK;
  const int len = (int)min((int64_t)CHUNK, n - base);  // elements of this chunk
  const int lane = tid & 63;
  for (int r = 0; r * N < len; ++r) {
    const uint32_t* cur = win + (r & 1) * N;
    uint32_t* nxt = win + ((r + 1) & 1) * N;
    next_block(cur, nxt);  // nxt[m] is the raw word of element base + 624 r + m
    const int e = r * N + tid;
    bool sel = false;
    if (tid < N && e < len) sel = (int32_t)(temper(nxt[tid]) & 0xFFFFFFu) <= thr;
    const uint64_t bal = __ballot(sel);
    if (lane == 0 && bal) {  // the wave's 64 bits start at a multiple of 16 in the chunk
      const int o = r * N + (tid & ~63), w0 = o >> 5;
      if (o & 31) {
        atomicOr(&bits[w0], (uint32_t)(bal << 16));
        atomicOr(&bits[w0 + 1], (uint32_t)(bal >> 16));
        atomicOr(&bits[w0 + 2], (uint32_t)(bal >> 48));
      } else {
        atomicOr(&bits[w0], (uint32_t)bal);
        atomicOr(&bits[w0 + 1], (uint32_t)(bal >> 32));
      }
    }
  }
  __syncthreads();
  const int words = (len + 31) >> 5;
  uint32_t* mout = mask + chunk * CHUNK_WORDS;
  for (int i = tid; i < words; i += THREADS) mout[i] = bits[i];
  // exclusive popcounts: thread t < 512 owns groups 2t and 2t + 1 (words 4t .. 4t + 3)
  uint32_t c0 = 0, c1 = 0;
  if (tid < CHUNK_GROUPS / 2) {
    c0 = __popc(bits[4 * tid]) + __popc(bits[4 * tid + 1]);
    c1 = __popc(bits[4 * tid + 2]) + __popc(bits[4 * tid + 3]);
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan(c0 + c1, wsum, &total);
  const int64_t G = n_groups(n);
  const int groups = (len + GROUP - 1) / GROUP;
  int32_t* rout = rank_tab + chunk * CHUNK_GROUPS;
  if (2 * tid < groups) rout[2 * tid] = (int32_t)ex;
  if (2 * tid + 1 < groups) rout[2 * tid + 1] = (int32_t)(ex + c0);
  if (tid == 0) rank_tab[G + chunk] = (int32_t)total;  // made exclusive by mt_scan_kernel
}

__global__ void __launch_bounds__(THREADS)
mt_mask_kernel(uint32_t seed, int32_t thr, int64_t n, const uint32_t* __restrict__ fine,
               const uint32_t* __restrict__ states, uint32_t* __restrict__ mask,
               int32_t* __restrict__ rank_tab) {
  mask_body(seed, thr, n, fine, states, mask, rank_tab);
}

// batch: a grid of chunks x masks, blockIdx.y the mask (row blockIdx.y of every output)
__global__ void __launch_bounds__(THREADS)
mt_mask_batch_kernel(MaskBatchArgs a, int64_t n, const uint32_t* __restrict__ fine,
                     const uint32_t* __restrict__ states, int64_t states_stride,
                     uint32_t* __restrict__ mask, int64_t mask_stride,
                     int32_t* __restrict__ rank_tab, int64_t rank_stride) {
  const int64_t i = blockIdx.y;
  mask_body(a.seed[i], a.thr[i], n, fine, states + i * states_stride, mask + i * mask_stride,
            rank_tab + i * rank_stride);
}

// rank_tab[G + c]: chunk totals -> exclusive prefix, in place; *count = the number selected
__device__ __forceinline__ void scan_body(int32_t* __restrict__ chunk_tab, int chunks,
                                          int64_t* __restrict__ count) {
  __shared__ uint32_t wsum[16];
  uint32_t carry = 0;
  for (int b = 0; b < chunks; b += 1024) {
    const int i = b + threadIdx.x;
    const uint32_t v = i < chunks ? (uint32_t)chunk_tab[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan(v, wsum, &total);
    if (i < chunks) chunk_tab[i] = (int32_t)(carry + ex);
    carry += total;
  }
  if (threadIdx.x == 0) *count = (int64_t)carry;
}

__global__ void __launch_bounds__(1024)
mt_scan_kernel(int32_t* __restrict__ chunk_tab, int chunks, int64_t* __restrict__ count) {
  scan_body(chunk_tab, chunks, count);
}

// batch: one block per mask
__global__ void __launch_bounds__(1024)
mt_scan_batch_kernel(int32_t* __restrict__ rank_tab, int64_t rank_stride, int64_t G, int chunks,
                     int64_t* __restrict__ count) {
  scan_body(rank_tab + blockIdx.x * rank_stride + G, chunks, count + blockIdx.x);
}

// ---- consumers: four consecutive elements per thread -------------------------------------------
// the 4 mask bits of elements q .. q + 3 (q % 4 == 0) and the rank of the first selected one
__device__ __forceinline__ uint32_t quad_bits(const uint32_t* __restrict__ mask,
                                              const int32_t* __restrict__ rank_tab, int64_t q,
                                              int64_t words, int64_t G, int32_t* rank) {
  const int64_t g = q >> 6;
  const uint32_t lo = mask[2 * g];
  const uint32_t nib = ((q & 32 ? (2 * g + 1 < words ? mask[2 * g + 1] : 0u) : lo) >> (q & 31)) & 15u;
  if (nib) {
    const uint32_t hi = 2 * g + 1 < words ? mask[2 * g + 1] : 0u;
    const uint64_t m = ((uint64_t)hi << 32) | lo;
    *rank = rank_tab[G + (q >> 16)] + rank_tab[g] +
            __popcll(m & ((1ull << (q & 63)) - 1ull));
  }
  return nib;
}
static_assert(CHUNK == 1 << 16, "quad_bits takes the chunk of element q as q >> 16");

__global__ void __launch_bounds__(256)
mask_gather_kernel(const float* __restrict__ x, int64_t n, const uint32_t* __restrict__ mask,
                   const int32_t* __restrict__ rank_tab, float* __restrict__ vals,
                   int32_t* __restrict__ counter, int vec) {
  const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (q >= n) return;
  int32_t rank = 0;
  const uint32_t nib = quad_bits(mask, rank_tab, q, (n + 31) >> 5, n_groups(n), &rank);
  if (!nib) return;  // trailing mask bits are zero: a set bit is an element below n
  float v[4];
  if (vec && q + 4 <= n) {
    const float4 t = *reinterpret_cast<const float4*>(x + q);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q + i < n ? x[q + i] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if ((nib >> i) & 1u) {
      vals[rank++] = v[i];
      if (counter) counter[q + i] += 1;
    }
  }
}

struct FoldArgs {
  const uint32_t* mask[MAX_PAYLOADS];
  const int32_t* rank_tab[MAX_PAYLOADS];
  const float* vals[MAX_PAYLOADS];
  float w[MAX_PAYLOADS];
  float w_self;
  int np, self, acc;  // acc: out holds the running total of the payloads folded so far
};

__global__ void __launch_bounds__(256)
mask_fold_kernel(const float* __restrict__ local, int64_t n, FoldArgs a, float* out, int vec) {
  const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (q >= n) return;
  const int64_t words = (n + 31) >> 5, G = n_groups(n);
  const bool full = vec && q + 4 <= n;
  float x[4], t[4];
  if (full) {
    const float4 l = *reinterpret_cast<const float4*>(local + q);
    x[0] = l.x, x[1] = l.y, x[2] = l.z, x[3] = l.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = q + i < n ? local[q + i] : 0.0f;
  }
  if (a.acc) {
    if (full) {
      const float4 o = *reinterpret_cast<const float4*>(out + q);
      t[0] = o.x, t[1] = o.y, t[2] = o.z, t[3] = o.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = q + i < n ? out[q + i] : 0.0f;
    }
  }
  for (int p = 0; p < a.np; ++p) {  // uniform trip count; the library is built -ffp-contract=off
    int32_t rank = 0;
    const uint32_t nib = quad_bits(a.mask[p], a.rank_tab[p], q, words, G, &rank);
    const float w = a.w[p];
    const float* __restrict__ vals = a.vals[p];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = x[i];
      if ((nib >> i) & 1u) v = vals[rank++];
      const float term = w * v;
      t[i] = (p || a.acc) ? t[i] + term : term;
    }
  }
  if (a.self) {
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = t[i] + a.w_self * x[i];
  }
  if (full) {
    *reinterpret_cast<float4*>(out + q) = make_float4(t[0], t[1], t[2], t[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q + i < n) out[q + i] = t[i];
  }
}

// ---- a round's nodes in one launch: blockIdx.y is the node / the destination -----------------
// node table of dpz_mask_gather_nodes: 8 64-bit words per node
struct GatherNode {
  const float* x;
  const uint32_t* mask;
  const int32_t* rank_tab;
  float* vals;
  int32_t* counter;  // or null
  const int64_t* count;
  int32_t* status;
  uint64_t pad;
};
static_assert(sizeof(GatherNode) == 64, "8 64-bit words");

// mask_gather_kernel into a slot of `cap` values: a selected element whose rank is past the slot
// is not written (its counter still is), and the node's status word says so
__global__ void __launch_bounds__(256)
mask_gather_nodes_kernel(const GatherNode* __restrict__ tab, int64_t n, int64_t cap) {
  const GatherNode nd = tab[blockIdx.y];
  const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (q == 0) *nd.status = *nd.count > cap ? 1 : 0;
  if (q >= n) return;
  int32_t rank = 0;
  const uint32_t nib = quad_bits(nd.mask, nd.rank_tab, q, (n + 31) >> 5, n_groups(n), &rank);
  if (!nib) return;
  float v[4];
  if (aligned16(nd.x) && q + 4 <= n) {  // per row: packed rows of an n that is no multiple of 4
    const float4 t = *reinterpret_cast<const float4*>(nd.x + q);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q + i < n ? nd.x[q + i] : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if ((nib >> i) & 1u) {
      if (rank < cap) nd.vals[rank] = v[i];
      ++rank;
      if (nd.counter) nd.counter[q + i] += 1;
    }
  }
}

// fold table of dpz_mask_decode_average_nodes: 68 64-bit words per destination
struct FoldPayload {
  const uint32_t* mask;
  const int32_t* rank_tab;
  const float* vals;
  float w;
  uint32_t pad;
};
struct FoldDest {
  const float* local;
  float* out;
  float w_self;
  uint32_t pad0;
  int64_t np;
  FoldPayload p[MAX_PAYLOADS];
};
static_assert(sizeof(FoldDest) == 8 * (4 + 4 * MAX_PAYLOADS), "68 64-bit words");

// mask_fold_kernel (no running total) for every destination of a round, behind the guard words
__global__ void __launch_bounds__(256)
mask_fold_nodes_kernel(const FoldDest* __restrict__ tab, int64_t n, int self,
                       const int32_t* __restrict__ guard, int64_t guard_n) {
  if (guard) {  // a gather that overflowed its slot: no fold of this launch writes
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int64_t i = lane; i < guard_n; i += 64) bad |= guard[i] != 0;
    if (__ballot(bad) != 0) return;  // every wave reads the same final words
  }
  const FoldDest* __restrict__ d = tab + blockIdx.y;
  const int64_t q = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (q >= n) return;
  const float* __restrict__ local = d->local;
  float* out = d->out;
  const int np = (int)min(d->np, (int64_t)MAX_PAYLOADS);  // the host checked its own copy
  const int64_t words = (n + 31) >> 5, G = n_groups(n);
  const bool full = aligned16(local) && aligned16(out) && q + 4 <= n;
  float x[4], t[4];
  if (full) {
    const float4 l = *reinterpret_cast<const float4*>(local + q);
    x[0] = l.x, x[1] = l.y, x[2] = l.z, x[3] = l.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = q + i < n ? local[q + i] : 0.0f;
  }
  for (int p = 0; p < np; ++p) {  // uniform over the block: one destination per blockIdx.y
    int32_t rank = 0;
    const uint32_t nib = quad_bits(d->p[p].mask, d->p[p].rank_tab, q, words, G, &rank);
    const float w = d->p[p].w;
    const float* __restrict__ vals = d->p[p].vals;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = x[i];
      if ((nib >> i) & 1u) v = vals[rank++];
      const float term = w * v;
      t[i] = p ? t[i] + term : term;
    }
  }
  if (self) {
    const float ws = d->w_self;
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = t[i] + ws * x[i];
  }
  if (full) {
    *reinterpret_cast<float4*>(out + q) = make_float4(t[0], t[1], t[2], t[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (q + i < n) out[q + i] = t[i];
  }
}

static size_t states_bytes(int64_t n) {
  const int64_t coarse = (n_chunks(n) + COARSE - 1) / COARSE;  // coarse steps, the first at 0
  return coarse > 1 ? (size_t)coarse * N * sizeof(uint32_t) : 0;
}

}  // namespace mt
}  // namespace dpz

using namespace dpz::mt;

extern "C" {

int64_t dpz_mt_rank_entries(int64_t n) {
  if (n < 1 || n >= MAX_ELEMS) return -1;
  return n_groups(n) + n_chunks(n);
}

size_t dpz_mt_mask_workspace_bytes(int64_t n) {
  if (n < 1 || n >= MAX_ELEMS) return 0;
  return states_bytes(n) + 256;
}

int dpz_mt_mask(uint32_t seed, float alpha, int64_t n, uint32_t* mask, int32_t* rank_tab,
                int64_t* count_dev, void* ws, size_t ws_bytes, dpz_stream_t stream) {
  if (n < 1 || !mask || !rank_tab || !count_dev || !ws) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS) return DPZ_ERR_UNSUPPORTED;
  if (ws_bytes < dpz_mt_mask_workspace_bytes(n)) return DPZ_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = n_chunks(n);
  const int coarse = (int)((chunks + COARSE - 1) / COARSE);
  DevTables tab;
  const int rc = device_tables((int)(chunks < COARSE ? chunks : COARSE), coarse, &tab);
  if (rc != DPZ_OK) return rc;
  uint32_t* states = reinterpret_cast<uint32_t*>(ws);  // row d: the state at d * COARSE * CHUNK
  if (coarse > 1) {
    mt_coarse_kernel<<<(unsigned)(coarse - 1), THREADS, 0, st>>>(seed, tab.coarse, states);
    DPZ_LAUNCH_CHECK();
  }
  mt_mask_kernel<<<(unsigned)chunks, THREADS, 0, st>>>(seed, mask_threshold(alpha), n, tab.fine,
                                                        states, mask, rank_tab);
  DPZ_LAUNCH_CHECK();
  mt_scan_kernel<<<1, 1024, 0, st>>>(rank_tab + n_groups(n), (int)chunks, count_dev);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

size_t dpz_mt_mask_batch_workspace_bytes(int m, int64_t n) {
  if (m < 1 || n < 1 || n >= MAX_ELEMS) return 0;
  return (size_t)m * states_bytes(n) + 256;
}

int dpz_mt_mask_batch(int m, const uint32_t* seeds, const float* alphas, int64_t n, uint32_t* mask,
                      int64_t mask_stride, int32_t* rank_tab, int64_t rank_stride,
                      int64_t* count_dev, void* ws, size_t ws_bytes, dpz_stream_t stream) {
  if (m < 1 || n < 1 || !seeds || !alphas || !mask || !rank_tab || !count_dev || !ws)
    return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS) return DPZ_ERR_UNSUPPORTED;
  if (mask_stride < ((n + 31) >> 5) || (mask_stride & 3) ||
      rank_stride < n_groups(n) + n_chunks(n))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_mt_mask_batch_workspace_bytes(m, n)) return DPZ_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = n_chunks(n);
  const int coarse = (int)((chunks + COARSE - 1) / COARSE);
  DevTables tab;
  const int rc = device_tables((int)(chunks < COARSE ? chunks : COARSE), coarse, &tab);
  if (rc != DPZ_OK) return rc;
  uint32_t* states = reinterpret_cast<uint32_t*>(ws);  // mask i: rows [i * coarse, (i + 1) * coarse)
  const int64_t states_stride = coarse > 1 ? (int64_t)coarse * N : 0;
  for (int g0 = 0; g0 < m; g0 += MASK_GROUP) {  // one launch per MASK_GROUP masks: m <= 64, one
    const int gm = m - g0 < MASK_GROUP ? m - g0 : MASK_GROUP;
    MaskBatchArgs a;
    for (int i = 0; i < MASK_GROUP; ++i) {
      a.seed[i] = i < gm ? seeds[g0 + i] : 0u;
      a.thr[i] = i < gm ? mask_threshold(alphas[g0 + i]) : -1;
    }
    uint32_t* gs = states + g0 * states_stride;
    if (coarse > 1) {
      mt_coarse_batch_kernel<<<dim3((unsigned)(coarse - 1), (unsigned)gm), THREADS, 0, st>>>(
          a, tab.coarse, gs, states_stride);
      DPZ_LAUNCH_CHECK();
    }
    mt_mask_batch_kernel<<<dim3((unsigned)chunks, (unsigned)gm), THREADS, 0, st>>>(
        a, n, tab.fine, gs, states_stride, mask + g0 * mask_stride, mask_stride,
        rank_tab + g0 * rank_stride, rank_stride);
    DPZ_LAUNCH_CHECK();
  }
  mt_scan_batch_kernel<<<(unsigned)m, 1024, 0, st>>>(rank_tab, rank_stride, n_groups(n),
                                                     (int)chunks, count_dev);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

int dpz_mask_gather_nodes(int m, const void* node_table, int64_t n, int64_t cap,
                          dpz_stream_t stream) {
  if (m < 1 || n < 1 || cap < 1 || !node_table) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;
  mask_gather_nodes_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const GatherNode*>(node_table), n, cap);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

int dpz_mask_decode_average_nodes(int m, const void* fold_table, const int* n_payloads, int64_t n,
                                  int flags, const int32_t* guard, int64_t guard_n,
                                  dpz_stream_t stream) {
  if (m < 1 || n < 1 || !fold_table || !n_payloads || guard_n < 0 || (!guard && guard_n))
    return DPZ_ERR_ARG;
  if (flags & ~DPZ_FOLD_SELF) return DPZ_ERR_ARG;
  for (int j = 0; j < m; ++j)
    if (n_payloads[j] < 1) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || m > 65535) return DPZ_ERR_UNSUPPORTED;
  for (int j = 0; j < m; ++j)
    if (n_payloads[j] > MAX_PAYLOADS) return DPZ_ERR_UNSUPPORTED;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;
  mask_fold_nodes_kernel<<<dim3((unsigned)blocks, (unsigned)m), 256, 0, (hipStream_t)stream>>>(
      reinterpret_cast<const FoldDest*>(fold_table), n, (flags & DPZ_FOLD_SELF) ? 1 : 0,
      guard_n ? guard : nullptr, guard_n);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

int dpz_mask_gather(const float* x, int64_t n, const uint32_t* mask, const int32_t* rank_tab,
                    float* vals, int32_t* counter, dpz_stream_t stream) {
  if (n < 1 || !x || !mask || !rank_tab || !vals) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS) return DPZ_ERR_UNSUPPORTED;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;
  mask_gather_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
      x, n, mask, rank_tab, vals, counter, dpz::aligned16(x) ? 1 : 0);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

int dpz_mask_decode_average(const float* local, int64_t n, int n_payloads,
                            const uint32_t* const* mask, const int32_t* const* rank_tab,
                            const float* const* vals, const float* w, float w_self, int flags,
                            float* out, dpz_stream_t stream) {
  if (n < 1 || n_payloads < 1 || !local || !out || !mask || !rank_tab || !vals || !w)
    return DPZ_ERR_ARG;
  if (flags & ~(DPZ_FOLD_SELF | DPZ_FOLD_ACCUMULATE)) return DPZ_ERR_ARG;
  if (n >= MAX_ELEMS || n_payloads > MAX_PAYLOADS) return DPZ_ERR_UNSUPPORTED;
  FoldArgs a;
  for (int p = 0; p < n_payloads; ++p) {
    if (!mask[p] || !rank_tab[p] || !vals[p]) return DPZ_ERR_ARG;
    a.mask[p] = mask[p];
    a.rank_tab[p] = rank_tab[p];
    a.vals[p] = vals[p];
    a.w[p] = w[p];
  }
  for (int p = n_payloads; p < MAX_PAYLOADS; ++p) {
    a.mask[p] = nullptr, a.rank_tab[p] = nullptr, a.vals[p] = nullptr, a.w[p] = 0.0f;
  }
  a.w_self = w_self;
  a.np = n_payloads;
  a.self = (flags & DPZ_FOLD_SELF) ? 1 : 0;
  a.acc = (flags & DPZ_FOLD_ACCUMULATE) ? 1 : 0;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;
  mask_fold_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
      local, n, a, out, dpz::aligned16(local) && dpz::aligned16(out) ? 1 : 0);
  DPZ_LAUNCH_CHECK();
  return DPZ_OK;
}

}  // extern "C"
