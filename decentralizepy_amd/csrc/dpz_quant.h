// Device helpers of the fixed-ratio quantiser (dpz_quant.hip), shared with its batched form
// (dpz_quant_nodes.hip) and the fused unpack-and-fold (dpz_qdense.hip): the statistics block, the
// parameters that follow from max|x|, the pack block and the decode of one field.  A kernel owns
// the grid mapping and the LDS; the functions here take the block's chunk / span index.
#pragma once
#include "dpz_common.h"

namespace dpz {

constexpr int Q_THREADS = 256;
constexpr int Q_CHUNK = 8192;  // numpy's add.reduce block: one independent pairwise tree each
constexpr int Q_LEAF = 128;    // numpy's pairwise-sum leaf (PW_BLOCKSIZE)
constexpr int Q_SPAN = 8192;   // pack: values per block, 32 consecutive values per thread
constexpr int Q_TILE = 512;    // chunk sums per step of the sequential chain (2 per thread)
constexpr int Q_MAXLEAF = 128; // a partial chunk has < 8192 / 64 leaves
constexpr int64_t Q_NMAX = (int64_t)1 << 31;
static_assert(Q_TILE == 2 * Q_THREADS, "the chain stages two sums per thread");

// workspace of one vector: 256 running max|x| words, zeroed before every call (block b's atomic
// max goes to word b % 256: atomics on ONE word serialise at about 13 ns each, which alone took 27
// of the statistics pass's 31 us at 2048 blocks), and one fp32 sum per 8192-element chunk
constexpr int Q_SLOTS = Q_THREADS;
constexpr size_t Q_WS_SUMS = 4 * Q_SLOTS;

// info record (dpz_codec.h): int32 words
enum { QI_STATUS = 0, QI_W, QI_PAD, QI_SCALE, QI_NORM, QI_MAX, QI_SUM, QI_OFF, QI_WORDS };

// a node's packed row of the quantised rounds (dpz_codec.h): int32 words
// [count (int64), status, 0 | the info record | body dwords]
enum { QROW_COUNT = 0, QROW_STATUS = 2, QROW_INFO = 4, QROW_BODY = QROW_INFO + QI_WORDS };

__device__ __forceinline__ float absmax(float v, uint32_t& mx) {
  const uint32_t b = __float_as_uint(v) & 0x7FFFFFFFu;
  mx = b > mx ? b : mx;
  return __uint_as_float(b);
}

// numpy's pairwise leaf over a[0..len), len <= 128, by the 8 lanes of a group (j = lane & 7):
// for len >= 8 eight accumulators r_j = a[j] + a[8+j] + ..., combined as ((r0+r1)+(r2+r3)) +
// ((r4+r5)+(r6+r7)), then the len % 8 tail one by one; for len < 8 a sequential sum from 0.  Every
// lane of the group returns the sum.  fp32 addition is commutative, so the xor butterfly gives each
// lane the same bits as the written order.
__device__ __forceinline__ float leaf_sum(const float* __restrict__ a, int len, int j,
                                          uint32_t& mx) {
  const int body = len >= 8 ? len - (len & 7) : 0;
  float r = body ? absmax(a[j], mx) : 0.0f;
  for (int i = 8; i < body; i += 8) r = r + absmax(a[i + j], mx);
  r = r + __shfl_xor(r, 1, 64);
  r = r + __shfl_xor(r, 2, 64);
  r = r + __shfl_xor(r, 4, 64);
  if (!body) r = 0.0f;
  for (int i = body; i < len; ++i) r = r + absmax(a[i], mx);
  return r;
}

constexpr int Q_LSTRIDE = Q_LEAF + 8;  // staged leaf stride: the 8-byte reads of 8 leaves x 4
                                       // lanes (a half wave) then fall on 64 distinct banks

struct StatsLds {
  alignas(16) float stage[(Q_CHUNK / Q_LEAF) * Q_LSTRIDE];
  float leaf[64];
  int lf_off[Q_MAXLEAF], lf_len[Q_MAXLEAF], lf_dep[Q_MAXLEAF];
  float lf_sum[Q_MAXLEAF];
  int nleaf, owners0;
  uint32_t wmax[Q_THREADS / 64];
};

// The block of 8192-element chunk `chunk`: its pairwise sum goes to sums[chunk], its max|x| bits
// into one of the max words by an atomic max (order-free).  Nothing waits on another block.
__device__ __forceinline__ void quant_stats_block(const float* __restrict__ x, int64_t n, int vec,
                                                  uint32_t* maxw, float* sums, unsigned chunk_id,
                                                  StatsLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = tid >> 3, j = tid & 7;
  const int64_t base = (int64_t)chunk_id * Q_CHUNK;
  const int len = (int)((n - base) < Q_CHUNK ? (n - base) : Q_CHUNK);
  const float* a = x + base;
  uint32_t mx = 0;
  float chunk = 0.0f;

  if (len == Q_CHUNK && vec) {
    // a perfect tree over 64 leaves of 128.  The chunk comes in with coalesced 16-byte loads
    // (|x| and the max taken on the way) into a padded LDS image; then one leaf per 4 lanes: a
    // lane keeps two of the leaf's eight accumulators and reads 8 bytes of LDS per step
    {
#pragma unroll
      for (int i = 0; i < Q_CHUNK / (4 * Q_THREADS); ++i) {
        const int e = 4 * (tid + Q_THREADS * i);
        float4 v = *reinterpret_cast<const float4*>(a + e);
        v.x = absmax(v.x, mx);
        v.y = absmax(v.y, mx);
        v.z = absmax(v.z, mx);
        v.w = absmax(v.w, mx);
        *reinterpret_cast<float4*>(s.stage + (e >> 7) * Q_LSTRIDE + (e & (Q_LEAF - 1))) = v;
      }
      __syncthreads();
      const int l = tid >> 2, q = tid & 3;
      const float2* p = reinterpret_cast<const float2*>(s.stage + l * Q_LSTRIDE + 2 * q);
      float2 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = p[4 * i];
      float ra = v[0].x, rb = v[0].y;
#pragma unroll
      for (int i = 1; i < 16; ++i) {
        ra = ra + v[i].x;
        rb = rb + v[i].y;
      }
      float r = ra + rb;  // r0+r1 | r2+r3 | r4+r5 | r6+r7
      r = r + __shfl_xor(r, 1, 64);
      r = r + __shfl_xor(r, 2, 64);
      if (q == 0) s.leaf[l] = r;
    }
    __syncthreads();
    if (wid == 0) {
      float r = s.leaf[lane];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) r = r + __shfl_xor(r, d, 64);
      chunk = r;
    }
  } else {
    // the general recursion: halves of h = len/2 - (len/2) % 8 and len - h while len > 128.
    // Every leaf is at least 64 long, so it holds a multiple of 64: thread t walks from the root
    // to the leaf that holds element 64 t, and the thread with the leaf's first multiple owns it.
    bool owner = false;
    int off = 0, l = len, dep = 0;
    if (tid < Q_MAXLEAF && 64 * tid < len) {
      const int pos = 64 * tid;
      while (l > Q_LEAF) {
        const int h = l / 2 - (l / 2) % 8;
        if (pos < off + h) {
          l = h;
        } else {
          off += h;
          l -= h;
        }
        ++dep;
      }
      owner = tid == 0 || 64 * (tid - 1) < off;
    }
    const unsigned long long own = __ballot(owner);
    if (tid == 0) s.owners0 = __popcll(own);
    __syncthreads();
    if (wid < 2) {
      const int idx = __popcll(own & ((1ull << lane) - 1ull)) + (wid ? s.owners0 : 0);
      if (owner) {
        s.lf_off[idx] = off; s.lf_len[idx] = l; s.lf_dep[idx] = dep;
      }
      if (wid == 1 && lane == 0) s.nleaf = s.owners0 + __popcll(own);
    }
    __syncthreads();
    const int nl = s.nleaf;
    for (int q = g; q < nl; q += Q_THREADS / 8) {
      const float r = leaf_sum(a + s.lf_off[q], s.lf_len[q], j, mx);
      if (j == 0) s.lf_sum[q] = r;
    }
    __syncthreads();
    if (tid == 0) {
      // leaves in order with their depths: a finished subtree waits at its depth (depths on the
      // stack strictly increase, so one slot per depth) until its right sibling arrives
      float val[10] = {};
      uint32_t have = 0;
      for (int q = 0; q < nl; ++q) {
        float v = s.lf_sum[q];
        int d = s.lf_dep[q];
        while (d > 0 && ((have >> d) & 1u)) {
          float lhs = 0.0f;
#pragma unroll
          for (int e = 1; e < 10; ++e) lhs = e == d ? val[e] : lhs;
          v = lhs + v;
          have &= ~(1u << d);
          --d;
        }
#pragma unroll
        for (int e = 0; e < 10; ++e) val[e] = e == d ? v : val[e];
        have |= 1u << d;
      }
      chunk = val[0];
    }
  }

  // block max of |x| bits (a non-finite value has bits >= 0x7F800000)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_xor(mx, d, 64);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) s.wmax[wid] = mx;
  __syncthreads();
  if (tid == 0) {
    uint32_t bm = s.wmax[0];
    for (int w = 1; w < Q_THREADS / 64; ++w) bm = s.wmax[w] > bm ? s.wmax[w] : bm;
    __hip_atomic_fetch_max(&maxw[chunk_id % Q_SLOTS], bm, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    sums[chunk_id] = chunk;
  }
}

struct QuantParams {
  int status, w, pad;
  float norm, m;
  uint32_t off;  // p - 1
};

// What follows from max|x| alone: norm = fl(m / fl(k)), qmax = |rint(fl(m / norm))|, p = the
// power of two above qmax, w = log2(p) + 1; IEEE divisions, ties to even.
__device__ __forceinline__ QuantParams quant_params(uint32_t mb, int64_t n, int k,
                                                    int64_t cap_dwords) {
  QuantParams q;
  q.m = __uint_as_float(mb);
  q.status = mb >= 0x7F800000u ? 2 : (mb == 0 ? 1 : 0);
  q.norm = q.m / (float)k;
  q.w = 2; q.pad = 0; q.off = 1;
  if (q.status == 0 && !(q.norm > 0.0f)) q.status = 3;  // m / k underflows to zero
  if (q.status == 0) {
    const float r = fabsf(rintf(q.m / q.norm));
    if (!(r >= 1.0f && r < 2147483648.0f)) {
      q.status = 3;
    } else {
      const uint32_t qmax = (uint32_t)r;
      const int lg = 32 - __clz((int)qmax);  // log2 p
      q.w = lg + 1;
      if (q.w > 32) {
        q.status = 3;
      } else {
        q.off = (lg == 32 ? 0u : (1u << lg)) - 1u;
        q.pad = (int)((8 - ((n * q.w) & 7)) & 7);
        if ((n * q.w + 31) / 32 > cap_dwords) q.status = 4;  // the body buffer is too small
      }
    }
  }
  return q;
}

__device__ __forceinline__ int qpad(int i) { return i + (i >> 5); }

// The w-bit reversal of u = q + p - 1, to be placed LSB first.
__device__ __forceinline__ uint32_t quant_field(float x, float norm, uint32_t off, int w) {
  const int q = (int)rintf(x / norm);
  return __brev((uint32_t)q + off) >> (32 - w);
}

// 32 consecutive values make exactly w dwords: a thread owns 32 values and their w output words.
// Loads and stores stay coalesced through a padded LDS image (index i at i + i/32).  blk: the
// span [blk * Q_SPAN, (blk + 1) * Q_SPAN) of the vector.
template <int W>
__device__ __forceinline__ void pack_block(const float* __restrict__ x, int64_t n, int vec,
                                           const QuantParams& q, int w_rt, uint32_t* lds,
                                           uint32_t* __restrict__ out, int64_t blk) {
  const int w = W ? W : w_rt;
  const int tid = threadIdx.x;
  const int64_t base = blk * Q_SPAN;
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
  uint32_t f[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) f[c] = lds[33 * tid + c];
  __syncthreads();
  uint64_t acc = 0;
  int nb = 0, o = tid * w;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    acc |= (uint64_t)f[c] << nb;
    nb += w;
    if (nb >= 32) {
      lds[qpad(o)] = (uint32_t)acc;
      ++o;
      acc >>= 32;
      nb -= 32;
    }
  }
  __syncthreads();
  const int64_t ndw = (n * w + 31) / 32;
  const int64_t gbase = blk * Q_THREADS * w;
  for (int d = tid; d < Q_THREADS * w; d += Q_THREADS)
    if (gbase + d < ndw) out[gbase + d] = lds[qpad(d)];
}

constexpr int Q_PACK_LDS = Q_SPAN + Q_SPAN / 32;  // dwords of LDS of a pack block

// Block `bx` of the pack grid of one vector (1 + ceil(n / Q_SPAN) blocks): every block reduces
// the statistics pass's 256 max words; block 0 chains the chunk sums and writes the info record,
// block bx > 0 packs span bx - 1.  Returns the parameters (the same in every block).
__device__ __forceinline__ QuantParams quant_pack_body(const float* __restrict__ x, int64_t n,
                                                       int k, int vec, const uint32_t* maxw,
                                                       const float* sums,
                                                       uint32_t* __restrict__ out,
                                                       int64_t cap_dwords,
                                                       int32_t* __restrict__ info, unsigned bx,
                                                       uint32_t* lds) {
  // max|x|: every block reduces the statistics pass's 256 max words (one per thread)
  uint32_t mb = maxw[threadIdx.x];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_xor(mb, d, 64);
    mb = o > mb ? o : mb;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mb;
  __syncthreads();
  mb = lds[0];
#pragma unroll
  for (int w = 1; w < Q_THREADS / 64; ++w) mb = lds[w] > mb ? lds[w] : mb;
  __syncthreads();
  const QuantParams q = quant_params(mb, n, k, cap_dwords);
  if (bx == 0) {
    // the extra block, dispatched first: S = P(c0), then S = fl(S + P(cj)) in chunk order, a
    // sequential fp32 chain in one thread over sums staged in LDS, while the other blocks pack;
    // then the info record with scale = fl(fl(S / fl(n)) / fl(k))
    float* tile = reinterpret_cast<float*>(lds);
    const int64_t nchunks = (n + Q_CHUNK - 1) / Q_CHUNK;
    // Q_TILE sums per step, zero padded: S + 0 is S, and 0 + c0 is c0, so the chain can start
    // from 0 and run over whole groups of 16.  The next step's sums are in flight, and the next
    // group's LDS reads issued, while one thread adds.
    float S = 0.0f;
    const int t0 = threadIdx.x, t1 = threadIdx.x + Q_THREADS;
    float r0 = t0 < nchunks ? sums[t0] : 0.0f;
    float r1 = t1 < nchunks ? sums[t1] : 0.0f;
    const float4* t4 = reinterpret_cast<const float4*>(tile);
    for (int64_t b0 = 0; b0 < nchunks; b0 += Q_TILE) {
      const int cnt = (int)((nchunks - b0) < Q_TILE ? (nchunks - b0) : Q_TILE);
      tile[t0] = r0;
      tile[t1] = r1;
      __syncthreads();
      const int64_t nb = b0 + Q_TILE;
      r0 = nb + t0 < nchunks ? sums[nb + t0] : 0.0f;
      r1 = nb + t1 < nchunks ? sums[nb + t1] : 0.0f;
      if (threadIdx.x == 0) {
        const int groups = (cnt + 15) / 16;
        float4 cur[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) cur[c] = t4[c];
        for (int gq = 0; gq < groups; ++gq) {
          float4 nxt[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) nxt[c] = t4[(4 * (gq + 1) + c) & (Q_TILE / 4 - 1)];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            S = S + cur[c].x;
            S = S + cur[c].y;
            S = S + cur[c].z;
            S = S + cur[c].w;
            cur[c] = nxt[c];
          }
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      info[QI_STATUS] = q.status;
      info[QI_W] = q.w;
      info[QI_PAD] = q.pad;
      info[QI_SCALE] = (int32_t)__float_as_uint((S / (float)n) / (float)k);
      info[QI_NORM] = (int32_t)__float_as_uint(q.norm);
      info[QI_MAX] = (int32_t)__float_as_uint(q.m);
      info[QI_SUM] = (int32_t)__float_as_uint(S);
      info[QI_OFF] = (int32_t)q.off;
    }
    return q;
  }
  if (q.status != 0) return q;
  if (q.w == 16)
    pack_block<16>(x, n, vec, q, 16, lds, out, (int64_t)bx - 1);
  else
    pack_block<0>(x, n, vec, q, q.w, lds, out, (int64_t)bx - 1);
  return q;
}

// The value of the field at stream bits [i*w, (i+1)*w) of a body of ndw readable dwords, MSB
// first: float(double(u - 2^(w-1) + 1) * scale).  Up to w = 25 the quantised integer is exact in
// fp32 and its product with an fp32 scale has at most 48 significant bits, so the fp32 product
// rounds the same exact value once (subnormal results included) and gives the same bits.
__device__ __forceinline__ int32_t quant_int(const uint32_t* __restrict__ in, int64_t ndw,
                                             int64_t i, int w) {
  const uint32_t mask = w == 32 ? 0xFFFFFFFFu : ((1u << w) - 1u);
  const uint32_t half = (1u << (w - 1)) - 1u;
  const int64_t t = i * w, d = t >> 5;
  const uint64_t lo = d < ndw ? in[d] : 0u;
  const uint64_t hi = d + 1 < ndw ? in[d + 1] : 0u;
  const uint32_t fld = (uint32_t)(((hi << 32) | lo) >> (t & 31)) & mask;
  return (int32_t)((__brev(fld) >> (32 - w)) - half);
}

constexpr int Q_F32_MAX_W = 25;

__device__ __forceinline__ float quant_value(int32_t qv, int w, float scale) {
  return w <= Q_F32_MAX_W ? (float)qv * scale : (float)((double)qv * (double)scale);
}

__host__ __device__ __forceinline__ int64_t quant_chunks(int64_t n) { return (n + Q_CHUNK - 1) / Q_CHUNK; }

}  // namespace dpz
