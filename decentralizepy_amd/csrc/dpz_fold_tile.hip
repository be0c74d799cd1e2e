// The tile folds: the engines that need the tile-offsets pre-pass (every group the walk and merge
// folds do not take: dense payloads, a continued total, replace-only, very sparse or very dense
// groups).  Two launches per group of <= 16 payloads:
//  * fold_offsets_kernel: four payload entries per thread write, for every 4096-element output
//    tile that starts after the previous entry, the first entry index inside that tile
//    (start[p][t] = lower_bound(idx_p, t*4096)).  Coalesced over idx; replaces a dependent
//    binary search per tile.
//  * fold_kernel (the classic kernel): persistent blocks walk 4096-element tiles (the next
//    tile's entry ranges prefetched).  Every payload's entries of the tile are loaded up front,
//    flattened.  Then
//    - hit-chain path (no dense payload, <= FOLD_CAP entries in the tile): entries are pushed on
//      per-element hit chains in LDS in one pass; every element folds its base value alone
//      (packed fp32 pairs), and the tile's distinct hit elements, compacted to a list, are
//      folded exactly with their payload values (one thread each) and replace that result;
//    - phase path (dense payloads / dense alpha): per payload the block scatters the tile's hits
//      into an LDS value tile tagged with the payload number (the next payload's extra entries
//      prefetched meanwhile), and every thread folds its 8 elements:
//        t = (tag == p) ? hit : local;  total = (p == 0) ? t*w : total + t*w
//  * fold_group_kernel instead (the 4-slot group kernel), for all-sparse groups of >= 8 payloads
//    at moderate density: every entry of the tile loaded at tile start, payloads folded four at
//    a time from their own LDS value slots (two barriers per four payloads).
// All follow the reference's fp32 order exactly (library compiled with -ffp-contract=off).
// Algorithmic bytes: read local (4N) + write out (4N) + 8 bytes per payload entry.
#include "dpz_fold.h"

namespace dpz {

#ifndef DPZ_FOLD_THREADS
#define DPZ_FOLD_THREADS 512
#endif
constexpr int FOLD_THREADS = DPZ_FOLD_THREADS;
constexpr int FOLD_GROUPS = FOLD_TILE / (4 * FOLD_THREADS);  // float4 groups per thread
constexpr int FOLD_EQ = 4;  // payload entries per thread preloaded at tile start
constexpr int FOLD_POOL = 64;  // hit-chain path: elements hit by >= 3 payloads folded from LDS rows
constexpr int FOLD_NB = 4;  // phase path: next payload's extra entries per thread prefetched
// hit-chain path: per-element chain head (u32) + per-entry value and (next | payload << 16),
// the tile's local values and the distinct-hit list: 61 KB of LDS at 2816 entries (2 blocks of
// 512 threads per CU, as the registers allow)
constexpr int FOLD_CAP = FOLD_TILE / 16 * 11;
constexpr int FOLD_LDS_MASK = FOLD_TILE * 4 + FOLD_CAP * 8 + FOLD_TILE * 4 + FOLD_CAP * 2;
constexpr int FOLD_LDS_PHASE = FOLD_TILE * 4 + FOLD_TILE;
constexpr int FOLD_LDS_BYTES = FOLD_LDS_MASK > FOLD_LDS_PHASE ? FOLD_LDS_MASK : FOLD_LDS_PHASE;

// grid (ceil((kmax+1)/256), np): thread j of payload p handles entry j (j == k: end sentinel).
// grid (ceil((kmax + 1) / (4 * 256)), np): thread g of payload p handles entries 4g .. 4g + 3
// (j == k: the end sentinel); the four indices come in one 16-byte load when aligned.
template <int SHIFT>
__global__ void __launch_bounds__(256) fold_offsets_kernel(FoldArgs a, int32_t* starts,
                                                           int64_t ntiles) {
  const int p = blockIdx.y;
  const FoldPayload& P = a.p[p];
  if (!P.idx) return;
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const int64_t k = P.k;
  if (j0 > k) return;
  int32_t v[5];  // idx[j0 - 1 .. j0 + 3]
  v[0] = j0 == 0 ? 0 : P.idx[j0 - 1];
  if (j0 + 4 <= k && (reinterpret_cast<uintptr_t>(P.idx + j0) & 15u) == 0) {
    const int4 q = *reinterpret_cast<const int4*>(P.idx + j0);
    v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e + 1] = (j0 + e < k) ? P.idx[j0 + e] : 0;
  }
  int32_t* st = starts + (int64_t)p * (ntiles + 1);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t j = j0 + e;
    if (j > k) break;
    int64_t tprev = j == 0 ? -1 : ((int64_t)v[e] >> SHIFT);
    int64_t tcur = j == k ? ntiles : ((int64_t)v[e + 1] >> SHIFT);
    // an invalid payload (negative / too large / unsorted indices) must not write out of bounds
    if (tprev < -1) tprev = -1;
    if (tprev > ntiles) tprev = ntiles;
    if (tcur > ntiles) tcur = ntiles;
    for (int64_t t = tprev + 1; t <= tcur; ++t) st[t] = (int32_t)j;
  }
}

#ifdef DPZ_STAMPS  // diagnostic build only: per (block, tile iteration) phase stamps
__device__ unsigned long long g_fold_st[6][8192];
#define FSTAMP(i)                                                    \
  do {                                                               \
    if (threadIdx.x == 0 && it_ < 16 && blockIdx.x < 512)            \
      g_fold_st[i][blockIdx.x * 16 + it_] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define FSTAMP(i) do {} while (0)
#endif

template <bool VEC>
__global__ void __launch_bounds__(FOLD_THREADS, 4) fold_kernel(FoldArgs a) {
  // phase path: hv (value tile) + htag (payload tag); hit-mask path: msk + epos + ev
  __shared__ __attribute__((aligned(16))) uint8_t lds_raw[FOLD_LDS_BYTES];
  float* hv = reinterpret_cast<float*>(lds_raw);
  uint8_t* htag = lds_raw + FOLD_TILE * sizeof(float);
  __shared__ int32_t rng[FOLD_MAXP][2];
  __shared__ int32_t pre[FOLD_MAXP + 1];  // flattened entry offset of each payload's tile range
  const int t = threadIdx.x;
  // payload pointer table in LDS: the entry loads below pick their payload per lane, and a
  // per-lane index into the kernel-argument array is a dependent global load per tile
  __shared__ const __attribute__((address_space(1))) int32_t* s_idx[FOLD_MAXP];  // as_global
  __shared__ const __attribute__((address_space(1))) float* s_val[FOLD_MAXP];
  __shared__ uint32_t s_nhit;
  __shared__ uint32_t s_pool_n;                // rows of s_pool taken in this tile
  __shared__ float s_pool[FOLD_POOL][FOLD_MAXP];  // payload values of elements hit >= 3 times
  __shared__ float s_w[FOLD_MAXP];
  if (t == 0) {
    for (int p = 0; p < a.np; ++p) {
      s_idx[p] = as_global(a.p[p].idx);
      s_val[p] = as_global(a.p[p].val);
      s_w[p] = a.p[p].w;
    }
  }
  // persistent blocks: tile, tile + gridDim.x, ...; the next tile's entry ranges are loaded
  // while the current tile is folded
  int32_t nr0 = 0, nr1 = 0;
  const bool rng_lane = t < a.np && !((a.dense_mask >> t) & 1u);
  if (rng_lane && (int64_t)blockIdx.x < a.ntiles) {
    const int32_t* st = a.starts + (int64_t)t * (a.ntiles + 1);
    nr0 = st[blockIdx.x];
    nr1 = st[blockIdx.x + 1];
  }
  float L[4 * FOLD_GROUPS];
  // local values of tile `tl` into L: issued early, consumed a phase later (loads stay in
  // flight across the plain barriers in between)
  auto load_local = [&](int64_t tl) {
    const int64_t lo_ = tl * FOLD_TILE;
    const int64_t hi_ = (lo_ + FOLD_TILE < a.n) ? lo_ + FOLD_TILE : a.n;
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const int64_t i0 = lo_ + q * 4 * FOLD_THREADS + t * 4;
      if (VEC && i0 + 3 < hi_) {
        float4 v = *reinterpret_cast<const float4*>(a.local + i0);
        L[q * 4 + 0] = v.x; L[q * 4 + 1] = v.y; L[q * 4 + 2] = v.z; L[q * 4 + 3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) L[q * 4 + e] = i0 + e < hi_ ? a.local[i0 + e] : 0.0f;
      }
    }
  };
  if ((int64_t)blockIdx.x < a.ntiles) load_local(blockIdx.x);
  int it_ = -1;
  (void)it_;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
  ++it_;
  FSTAMP(0);
  const int64_t tlo = tile * FOLD_TILE;
  const int64_t thi = (tlo + FOLD_TILE < a.n) ? tlo + FOLD_TILE : a.n;
  if (t < 64) {
    // entry ranges and their flattened offsets (a wave scan; pre[u] = etot for u >= np)
    const int32_t c = (t < a.np && nr1 > nr0) ? nr1 - nr0 : 0;
    if (t < a.np) {
      rng[t][0] = nr0;
      rng[t][1] = nr1;
    }
    int32_t incl = c;
#pragma unroll
    for (int d = 1; d < FOLD_MAXP; d <<= 1) {
      const int32_t v = __shfl_up(incl, d, 64);
      if (t >= d) incl += v;
    }
    if (t < FOLD_MAXP) pre[t + 1] = incl;
    if (t == 0) pre[0] = 0;
  }
  if (rng_lane && tile + gridDim.x < a.ntiles) {
    const int32_t* st = a.starts + (int64_t)t * (a.ntiles + 1);
    nr0 = st[tile + gridDim.x];
    nr1 = st[tile + gridDim.x + 1];
  }

  // this thread's elements: q-th group = tlo + q*1024 + 4t .. +3; L (the local values) was
  // loaded ahead (prologue, or behind the previous tile's hit fold)
  float acc[4 * FOLD_GROUPS];
  if (!a.first) {
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const int64_t i0 = tlo + q * 4 * FOLD_THREADS + t * 4;
      if (VEC && i0 + 3 < thi) {
        float4 o = *reinterpret_cast<const float4*>(a.out + i0);
        acc[q * 4 + 0] = o.x; acc[q * 4 + 1] = o.y; acc[q * 4 + 2] = o.z; acc[q * 4 + 3] = o.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q * 4 + e] = i0 + e < thi ? a.out[i0 + e] : 0.0f;
      }
    }
  }
  bool l_ahead = false;  // L already holds the next tile's values

  __syncthreads();  // rng / pre visible
  FSTAMP(1);
  // every payload's entries of this tile (flattened, the first FOLD_EQ * FOLD_THREADS of them)
  // are loaded before any is used: one memory latency per tile instead of one per payload
  int ep[FOLD_EQ];
  int32_t ei[FOLD_EQ];
  float evl[FOLD_EQ];
  const int32_t etot = pre[a.np];
#pragma unroll
  for (int q = 0; q < FOLD_EQ; ++q) {
    const int32_t j = t + q * FOLD_THREADS;
    ep[q] = -1;
    ei[q] = 0;
    evl[q] = 0.0f;
    if (j < etot) {
      // payload of flattened entry j: binary search over pre[0..15] (pre[u] = etot > j for
      // u >= np), four dependent LDS reads instead of a read per payload
      int p = 0;
#pragma unroll
      for (int s = FOLD_MAXP / 2; s >= 1; s >>= 1) p += pre[p + s] <= j ? s : 0;
      const int64_t src = (int64_t)rng[p][0] + (j - pre[p]);
      ep[q] = p;
      ei[q] = s_idx[p][src];
      evl[q] = s_val[p][src];
    }
  }

  if (a.all_sparse && etot <= FOLD_CAP) {
    // Hit-chain path.  The fold is VALU-bound when every element runs the per-payload select
    // (16 payloads x 8 elements x ~6 instructions per thread), so it is split:
    //  A) every element folds its base value alone (no hits): 2 flops per payload term, packed;
    //  B) the tile's hit elements (~15 % at 16 payloads x 1 %), compacted to a list, are folded
    //     exactly with their payload values by one thread each and overwrite A's result.
    // Entries are pushed on per-element hit chains (head[pos] -> j -> ...) in one scatter phase.
    uint32_t* head = reinterpret_cast<uint32_t*>(lds_raw);
    uint32_t* meta = head + FOLD_TILE;                       // next (low 16) | payload << 16
    float* ev = reinterpret_cast<float*>(meta + FOLD_CAP);
    float* lv = ev + FOLD_CAP;                               // the tile's local values
    uint16_t* hitl = reinterpret_cast<uint16_t*>(lv + FOLD_TILE);  // distinct hit elements
    for (int j = t * 4; j < FOLD_TILE; j += 4 * FOLD_THREADS)
      *reinterpret_cast<uint4*>(&head[j]) = make_uint4(~0u, ~0u, ~0u, ~0u);
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q)
      *reinterpret_cast<float4*>(&lv[q * 4 * FOLD_THREADS + t * 4]) =
          make_float4(L[q * 4 + 0], L[q * 4 + 1], L[q * 4 + 2], L[q * 4 + 3]);
    if (t == 0) {
      s_nhit = 0;
      s_pool_n = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < FOLD_EQ; ++q) {
      if (ep[q] >= 0) {
        const int32_t j = t + q * FOLD_THREADS;
        const int64_t pos = (int64_t)ei[q] - tlo;
        ev[j] = evl[q];
        if (pos >= 0 && pos < FOLD_TILE) {  // guards against an unsorted caller array
          const uint32_t old = atomicExch(&head[pos], (uint32_t)j);
          meta[j] = (old & 0xFFFFu) | ((uint32_t)ep[q] << 16);
          if (old == ~0u) hitl[atomicAdd(&s_nhit, 1u)] = (uint16_t)pos;
        }
      }
    }
    for (int32_t j = FOLD_EQ * FOLD_THREADS + t; j < etot; j += FOLD_THREADS) {
      // payload of flattened entry j: binary search over pre[0..15] (pre[u] = etot > j for
      // u >= np), four dependent LDS reads instead of a read per payload
      int p = 0;
#pragma unroll
      for (int s = FOLD_MAXP / 2; s >= 1; s >>= 1) p += pre[p + s] <= j ? s : 0;
      const int64_t src = (int64_t)rng[p][0] + (j - pre[p]);
      const int64_t pos = (int64_t)s_idx[p][src] - tlo;
      ev[j] = s_val[p][src];
      if (pos >= 0 && pos < FOLD_TILE) {
        const uint32_t old = atomicExch(&head[pos], (uint32_t)j);
        meta[j] = (old & 0xFFFFu) | ((uint32_t)p << 16);
        if (old == ~0u) hitl[atomicAdd(&s_nhit, 1u)] = (uint16_t)pos;
      }
    }
    __syncthreads();
    FSTAMP(2);
    // A) base fold of this thread's elements; remember which of them carry hits
    uint32_t hitbits = 0;
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const uint4 h4 = *reinterpret_cast<const uint4*>(&head[q * 4 * FOLD_THREADS + t * 4]);
      hitbits |= ((h4.x != ~0u) ? 1u : 0u) << (4 * q);
      hitbits |= ((h4.y != ~0u) ? 1u : 0u) << (4 * q + 1);
      hitbits |= ((h4.z != ~0u) ? 1u : 0u) << (4 * q + 2);
      hitbits |= ((h4.w != ~0u) ? 1u : 0u) << (4 * q + 3);
    }
    {
      typedef float f2 __attribute__((ext_vector_type(2)));
      f2 b2[2 * FOLD_GROUPS], a2[2 * FOLD_GROUPS];
#pragma unroll
      for (int h = 0; h < 2 * FOLD_GROUPS; ++h) {
        b2[h] = a.zero_base ? f2{0.0f, 0.0f} : f2{L[2 * h], L[2 * h + 1]};
        a2[h] = f2{acc[2 * h], acc[2 * h + 1]};
      }
      if (a.replace_only) {
#pragma unroll
        for (int h = 0; h < 2 * FOLD_GROUPS; ++h) a2[h] = b2[h];
      } else {
        // weights from LDS (uniform reads); an unrolled loop over scalar weights spilled SGPRs
        // into VGPR lanes and cost occupancy
        int p0 = 0;
        if (a.first) {
          const float w = s_w[0];
          const f2 w2 = {w, w};
#pragma unroll
          for (int h = 0; h < 2 * FOLD_GROUPS; ++h) {
            const f2 term = b2[h] * w2;
            a2[h] = a.zero_base ? f2{0.0f, 0.0f} + term : term;
          }
          p0 = 1;
        }
        for (int p = p0; p < a.np; ++p) {
          const float w = s_w[p];
          const f2 w2 = {w, w};
#pragma unroll
          for (int h = 0; h < 2 * FOLD_GROUPS; ++h) a2[h] = a2[h] + b2[h] * w2;
        }
      }
#pragma unroll
      for (int h = 0; h < 2 * FOLD_GROUPS; ++h) {
        acc[2 * h] = a2[h].x;
        acc[2 * h + 1] = a2[h].y;
      }
    }
    // L is dead from here on (B and add_self read the LDS copy lv): the next tile's local
    // values load behind the hit fold and the stores
    if (tile + gridDim.x < a.ntiles) {
      load_local(tile + gridDim.x);
      l_ahead = true;
    }
    __syncthreads();  // every owner has read its hit flags before B overwrites head[]
    FSTAMP(3);
    // B) exact fold of the hit elements, two per thread with their chain walks interleaved
    //    (the walks are dependent LDS reads: one latency for both); the result replaces
    //    head[pos].  The usual one or two hits of an element fold branch-free; an element with
    //    three or more (rare) is refolded by the general chain walk.
    const uint32_t nhit = s_nhit;
    float wr[FOLD_MAXP];
#pragma unroll
    for (int p = 0; p < FOLD_MAXP; ++p) wr[p] = s_w[p];
    for (uint32_t s0 = t; s0 < nhit; s0 += 2 * FOLD_THREADS) {
      const uint32_t s1 = s0 + FOLD_THREADS;
      const bool two = s1 < nhit;
      int pos[2];
      pos[0] = hitl[s0];
      pos[1] = two ? hitl[s1] : pos[0];
      float bb[2], av[2], v1[2], v2[2];
      uint32_t p1[2], p2[2], more[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bb[h] = a.zero_base ? 0.0f : lv[pos[h]];
        av[h] = a.first ? 0.0f : a.out[tlo + pos[h]];
        const uint32_t c1 = head[pos[h]] & 0xFFFFu;
        const uint32_t m1 = meta[c1];
        p1[h] = m1 >> 16;
        v1[h] = ev[c1];
        const uint32_t c2 = m1 & 0xFFFFu;
        const uint32_t m2 = meta[c2 != 0xFFFFu ? c2 : c1];
        p2[h] = c2 != 0xFFFFu ? (m2 >> 16) : 0xFFFFu;
        v2[h] = ev[c2 != 0xFFFFu ? c2 : c1];
        more[h] = c2 != 0xFFFFu ? (m2 & 0xFFFFu) : 0xFFFFu;
      }
#pragma unroll
      for (int p = 0; p < FOLD_MAXP; ++p) {
        if (p >= a.np) break;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float tv = ((uint32_t)p == p1[h]) ? v1[h] : (((uint32_t)p == p2[h]) ? v2[h] : bb[h]);
          fold_term(av[h], tv, wr[p], a.first && p == 0, a.replace_only, a.zero_base);
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (more[h] != 0xFFFFu) {  // three or more hits (rare): walk the chain once into a row
          float acc = a.first ? 0.0f : a.out[tlo + pos[h]];
          const uint32_t row = atomicAdd(&s_pool_n, 1u);
          if (row < FOLD_POOL) {
            uint32_t mask = 0;
            for (uint32_t c = head[pos[h]] & 0xFFFFu; c != 0xFFFFu;) {
              const uint32_t m = meta[c];
              s_pool[row][m >> 16] = ev[c];
              mask |= 1u << (m >> 16);
              c = m & 0xFFFFu;
            }
            for (int p = 0; p < a.np; ++p) {
              const float tv = ((mask >> p) & 1u) ? s_pool[row][p] : bb[h];
              fold_term(acc, tv, wr[p], a.first && p == 0, a.replace_only, a.zero_base);
            }
          } else {  // the pool is full: a walk per payload
            for (int p = 0; p < a.np; ++p) {
              float tv = bb[h];
              for (uint32_t c = head[pos[h]] & 0xFFFFu; c != 0xFFFFu;) {
                const uint32_t m = meta[c];
                if ((m >> 16) == (uint32_t)p) {
                  tv = ev[c];
                  break;
                }
                c = m & 0xFFFFu;
              }
              fold_term(acc, tv, wr[p], a.first && p == 0, a.replace_only, a.zero_base);
            }
          }
          av[h] = acc;
        }
      }
      // every hit element's chain head is read above before any result overwrites it: each
      // element belongs to exactly one (thread, h), and only its own head[pos] is written
      head[pos[0]] = __float_as_uint(av[0]);
      if (two) head[pos[1]] = __float_as_uint(av[1]);
    }
    __syncthreads();
    FSTAMP(4);
    if (hitbits) {
#pragma unroll
      for (int q = 0; q < FOLD_GROUPS; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((hitbits >> (4 * q + e)) & 1u)
            acc[q * 4 + e] = __uint_as_float(head[q * 4 * FOLD_THREADS + t * 4 + e]);
    }
  } else {
  for (int j = t * 4; j < FOLD_TILE; j += 4 * FOLD_THREADS) *reinterpret_cast<uint32_t*>(&htag[j]) = 0xFFFFFFFFu;
  // entries of a payload past the preloaded ones (dense ranges, e.g. JWINS alpha 0.1-0.4):
  // the next payload's first FOLD_NB per thread are loaded while the current payload folds
  int32_t nbi[FOLD_NB];
  float nbv[FOLD_NB];
  auto prefetch = [&](int pp) {
#pragma unroll
    for (int u = 0; u < FOLD_NB; ++u) nbi[u] = -1;
    if (pp < a.np && !((a.dense_mask >> pp) & 1u)) {
      const int64_t first = (int64_t)FOLD_EQ * FOLD_THREADS - pre[pp];
      const int64_t j0 = rng[pp][0] + (first > 0 ? first : 0) + t;
      const int64_t e = rng[pp][1];
#pragma unroll
      for (int u = 0; u < FOLD_NB; ++u) {
        const int64_t j = j0 + (int64_t)u * FOLD_THREADS;
        if (j < e) {
          nbi[u] = s_idx[pp][j];
          nbv[u] = s_val[pp][j];
        }
      }
    }
  };
  prefetch(0);
  for (int p = 0; p < a.np; ++p) {
    const FoldPayload& P = a.p[p];
    __syncthreads();  // previous payload's reads of hv/htag done
    if (P.idx) {
#pragma unroll
      for (int q = 0; q < FOLD_EQ; ++q) {
        if (ep[q] == p) {
          const int64_t pos = (int64_t)ei[q] - tlo;
          if (pos >= 0 && pos < FOLD_TILE) {  // guards against an unsorted caller array
            hv[pos] = evl[q];
            htag[pos] = (uint8_t)p;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < FOLD_NB; ++u) {
        const int64_t pos = (int64_t)nbi[u] - tlo;
        if (pos >= 0 && pos < FOLD_TILE) {
          hv[pos] = nbv[u];
          htag[pos] = (uint8_t)p;
        }
      }
      // entries past the preloaded and prefetched ones: loaded here
      const int64_t b = rng[p][0], e = rng[p][1];
      const int64_t first = (int64_t)FOLD_EQ * FOLD_THREADS - pre[p];  // relative to b
      for (int64_t j = b + (first > 0 ? first : 0) + (int64_t)FOLD_NB * FOLD_THREADS + t; j < e;
           j += FOLD_THREADS) {
        const int64_t pos = (int64_t)P.idx[j] - tlo;
        if (pos >= 0 && pos < FOLD_TILE) {
          hv[pos] = P.val[j];
          htag[pos] = (uint8_t)p;
        }
      }
    }
    __syncthreads();
    prefetch(p + 1);
    const float w = P.w;
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const int j0 = q * 4 * FOLD_THREADS + t * 4;
      const int64_t i0 = tlo + j0;
      float tv[4];
      if (P.idx) {
        const float4 h4 = *reinterpret_cast<const float4*>(&hv[j0]);
        const uint32_t g4 = *reinterpret_cast<const uint32_t*>(&htag[j0]);
        const float hh[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          tv[e] = (((g4 >> (8 * e)) & 0xFFu) == (uint32_t)p) ? hh[e]
                                                               : (a.zero_base ? 0.0f : L[q * 4 + e]);
      } else {
        if (VEC && i0 + 3 < thi) {
          float4 v = *reinterpret_cast<const float4*>(P.val + i0);
          tv[0] = v.x; tv[1] = v.y; tv[2] = v.z; tv[3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) tv[e] = (i0 + e < thi) ? P.val[i0 + e] : 0.0f;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (a.replace_only) {
          acc[q * 4 + e] = tv[e];
        } else {
          const float term = tv[e] * w;
          acc[q * 4 + e] = (a.first && p == 0) ? (a.zero_base ? 0.0f + term : term)
                                               : acc[q * 4 + e] + term;
        }
      }
    }
  }
  }  // phase path
  if (a.add_self) {
    if (l_ahead) {  // hit-chain path: this tile's local values from the LDS copy
      const float* lv = reinterpret_cast<const float*>(lds_raw) + FOLD_TILE + 2 * FOLD_CAP;
#pragma unroll
      for (int q = 0; q < FOLD_GROUPS; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(&lv[q * 4 * FOLD_THREADS + t * 4]);
        acc[q * 4 + 0] = acc[q * 4 + 0] + v.x * a.w_self;
        acc[q * 4 + 1] = acc[q * 4 + 1] + v.y * a.w_self;
        acc[q * 4 + 2] = acc[q * 4 + 2] + v.z * a.w_self;
        acc[q * 4 + 3] = acc[q * 4 + 3] + v.w * a.w_self;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4 * FOLD_GROUPS; ++e) acc[e] = acc[e] + L[e] * a.w_self;
    }
  }
#pragma unroll
  for (int q = 0; q < FOLD_GROUPS; ++q) {
    const int64_t i0 = tlo + q * 4 * FOLD_THREADS + t * 4;
    if (VEC && i0 + 3 < thi) {
      const float4 r4 = make_float4(acc[q * 4 + 0], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]);
      *reinterpret_cast<float4*>(a.out + i0) = r4;
      // in place over local: every local read of this tile happened before (registers / LDS)
      if (a.out2) *reinterpret_cast<float4*>(a.out2 + i0) = r4;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < thi) {
          a.out[i0 + e] = acc[q * 4 + e];
          if (a.out2) a.out2[i0 + e] = acc[q * 4 + e];
        }
    }
  }
  if (!l_ahead && tile + gridDim.x < a.ntiles) load_local(tile + gridDim.x);
  __syncthreads();  // the next tile reuses rng / pre / the LDS tile
  FSTAMP(5);
  }  // tile loop
}

// ------------------------------------------------------------------------------------------------
// Slotted fold for dense all-sparse groups (JWINS alpha 0.1-0.4: thousands of entries per tile).
// The phase path pays a global load latency per payload (the next payload's entries arrive while
// only a short fold runs) and two barriers per payload.  Here every entry of the tile (up to
// FG_CAP per round) is loaded at tile start, into registers, and the payloads are folded
// FG_SLOTS at a time: each payload of a phase scatters into its own LDS value tile with a hit bit,
// then every thread folds its 8 elements over the phase's payloads in the reference's order
//   t = hit ? value : local;  total = (p == 0) ? t*w : total + t*w
// Hit flags are one byte per element (bit s: slot s hit), so the entries of a payload, sorted and
// spread over consecutive lanes, rarely collide in an LDS atomic; each thread clears its own
// elements' flags right after folding them, so a phase costs two barriers and no global round
// trip.
constexpr int FG_SLOTS = 4;                    // payloads per phase
constexpr int FG_EPT = FG_CAP / FOLD_THREADS;  // per thread
#ifndef DPZ_FG_HALVES
#define DPZ_FG_HALVES 2
#endif
constexpr int FG_HALVES = DPZ_FG_HALVES;  // entry load batches per round (register pressure)
static_assert(FG_CAP >= FOLD_TILE && FOLD_TILE <= 65536, "a round holds one payload's tile");
static_assert(FG_SLOTS <= 8, "slot flags are the bits of one byte per element");

template <bool VEC>
__global__ void __launch_bounds__(FOLD_THREADS, 4) fold_group_kernel(FoldArgs a) {
  __shared__ __attribute__((aligned(16))) float hv[FG_SLOTS][FOLD_TILE];
  __shared__ uint32_t hf[FOLD_TILE / 4];  // hit flags: byte e of word w = element 4w + e
  __shared__ int32_t rng[FOLD_MAXP][2];
  __shared__ int32_t pre[FOLD_MAXP + 1];
  __shared__ const __attribute__((address_space(1))) int32_t* s_idx[FOLD_MAXP];  // as_global
  __shared__ const __attribute__((address_space(1))) float* s_val[FOLD_MAXP];
  __shared__ float s_w[FOLD_MAXP];
  const int t = threadIdx.x;
  if (t == 0) {
    for (int p = 0; p < a.np; ++p) {
      s_idx[p] = as_global(a.p[p].idx);
      s_val[p] = as_global(a.p[p].val);
      s_w[p] = a.p[p].w;
    }
  }
#pragma unroll
  for (int q = 0; q < FOLD_GROUPS; ++q) hf[q * FOLD_THREADS + t] = 0;
  int32_t nr0 = 0, nr1 = 0;
  const bool rng_lane = t < a.np;
  if (rng_lane && (int64_t)blockIdx.x < a.ntiles) {
    const int32_t* st = a.starts + (int64_t)t * (a.ntiles + 1);
    nr0 = st[blockIdx.x];
    nr1 = st[blockIdx.x + 1];
  }
  float L[4 * FOLD_GROUPS];
  auto load_local = [&](int64_t tl) {
    const int64_t lo_ = tl * FOLD_TILE;
    const int64_t hi_ = (lo_ + FOLD_TILE < a.n) ? lo_ + FOLD_TILE : a.n;
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const int64_t i0 = lo_ + q * 4 * FOLD_THREADS + t * 4;
      if (VEC && i0 + 3 < hi_) {
        float4 v = *reinterpret_cast<const float4*>(a.local + i0);
        L[q * 4 + 0] = v.x; L[q * 4 + 1] = v.y; L[q * 4 + 2] = v.z; L[q * 4 + 3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) L[q * 4 + e] = i0 + e < hi_ ? a.local[i0 + e] : 0.0f;
      }
    }
  };
  if ((int64_t)blockIdx.x < a.ntiles) load_local(blockIdx.x);
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t tlo = tile * FOLD_TILE;
    const int64_t thi = (tlo + FOLD_TILE < a.n) ? tlo + FOLD_TILE : a.n;
    if (t < 64) {
      const int32_t c = (t < a.np && nr1 > nr0) ? nr1 - nr0 : 0;
      if (t < a.np) {
        rng[t][0] = nr0;
        rng[t][1] = nr1;
      }
      int32_t incl = c;
#pragma unroll
      for (int d = 1; d < FOLD_MAXP; d <<= 1) {
        const int32_t v = __shfl_up(incl, d, 64);
        if (t >= d) incl += v;
      }
      if (t < FOLD_MAXP) pre[t + 1] = incl;
      if (t == 0) pre[0] = 0;
    }
    if (rng_lane && tile + gridDim.x < a.ntiles) {
      const int32_t* st = a.starts + (int64_t)t * (a.ntiles + 1);
      nr0 = st[tile + gridDim.x];
      nr1 = st[tile + gridDim.x + 1];
    }
    typedef float f2v __attribute__((ext_vector_type(2)));
    f2v acc2[2 * FOLD_GROUPS];  // this thread's 8 running totals as packed pairs
    float base[4 * FOLD_GROUPS];  // a payload's value off its entries: local, or 0 (zero base)
#pragma unroll
    for (int e = 0; e < 4 * FOLD_GROUPS; ++e) base[e] = a.zero_base ? 0.0f : L[e];
#pragma unroll
    for (int h = 0; h < 2 * FOLD_GROUPS; ++h) acc2[h] = f2v{0.0f, 0.0f};
    if (!a.first) {
#pragma unroll
      for (int q = 0; q < FOLD_GROUPS; ++q) {
        const int64_t i0 = tlo + q * 4 * FOLD_THREADS + t * 4;
        float o[4];
        if (VEC && i0 + 3 < thi) {
          const float4 v = *reinterpret_cast<const float4*>(a.out + i0);
          o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = i0 + e < thi ? a.out[i0 + e] : 0.0f;
        }
        acc2[2 * q] = f2v{o[0], o[1]};
        acc2[2 * q + 1] = f2v{o[2], o[3]};
      }
    }
    __syncthreads();  // rng / pre visible; the previous tile's last phase is done
    for (int pa = 0; pa < a.np;) {
      // the round: payloads [pa, pb) whose entries of this tile fit FG_CAP (at least one)
      int pb = pa + 1;
      while (pb < a.np && pre[pb + 1] - pre[pa] <= FG_CAP) ++pb;
      const int32_t j0 = pre[pa], jn = pre[pb] - pre[pa];
      // entry u of this thread: ei = (position in the tile | payload << 16) or ~0 (absent /
      // outside the tile: an invalid payload cannot write out of bounds), ev = its value.
      // Loaded in FG_HALVES batches (fewer address registers live at once).
      uint32_t ei[FG_EPT];
      float ev[FG_EPT];
#pragma unroll
      for (int h = 0; h < FG_HALVES; ++h) {
        constexpr int HU = FG_EPT / FG_HALVES;
#pragma unroll
        for (int u = h * HU; u < (h + 1) * HU; ++u) {
          const int32_t j = t + u * FOLD_THREADS;
          ei[u] = 0;
          ev[u] = 0.0f;
          if (j < jn) {
            const int32_t jj = j0 + j;
            int p = 0;
#pragma unroll
            for (int s = FOLD_MAXP / 2; s >= 1; s >>= 1) p += pre[p + s] <= jj ? s : 0;
            const int64_t src = (int64_t)rng[p][0] + (jj - pre[p]);
            ei[u] = (uint32_t)s_idx[p][src];
            ev[u] = s_val[p][src];
          }
        }
#pragma unroll
        for (int u = h * HU; u < (h + 1) * HU; ++u) {
          // the entry's payload again (4 LDS reads): cheaper than holding it in registers
          uint32_t p = 0;
          {
            const int32_t jj = j0 + t + u * FOLD_THREADS;
#pragma unroll
            for (int s = FOLD_MAXP / 2; s >= 1; s >>= 1) p += pre[p + s] <= jj ? s : 0;
          }
          const int64_t pos = (int64_t)(int32_t)ei[u] - tlo;
          const bool in = t + u * FOLD_THREADS < jn && pos >= 0 && pos < FOLD_TILE;
          ei[u] = in ? ((uint32_t)pos | (p << 16)) : ~0u;
        }
      }
      for (int pbase = pa; pbase < pb; pbase += FG_SLOTS) {
        const int ns = (pb - pbase) < FG_SLOTS ? (pb - pbase) : FG_SLOTS;
        // scatter this phase's payloads into their slots
#pragma unroll
        for (int u = 0; u < FG_EPT; ++u) {
          const uint32_t s = (ei[u] >> 16) - (uint32_t)pbase;  // ~0 entries: s is huge
          if (s < (uint32_t)ns) {
            const uint32_t pos = ei[u] & 0xFFFFu;
            hv[s][pos] = ev[u];
            atomicOr(&hf[pos >> 2], (1u << s) << (8u * (pos & 3u)));
          }
        }
        __syncthreads();
        // fold the phase's payloads (this thread's own elements: flag word q * 512 + t)
        uint32_t fw[FOLD_GROUPS];
#pragma unroll
        for (int q = 0; q < FOLD_GROUPS; ++q) {
          fw[q] = hf[q * FOLD_THREADS + t];
          hf[q * FOLD_THREADS + t] = 0;  // read: cleared for the next phase (no one else reads it)
        }
        // packed fp32 pairs (v_pk_mul / v_pk_add: two elements per instruction, no FMA); the
        // first term of a fresh total (payload 0) is peeled off the loop
        for (int s = 0; s < ns; ++s) {
          const int p = pbase + s;
          const float w = s_w[p];
          const f2v w2 = {w, w};
          const bool first_term = a.first && p == 0;
#pragma unroll
          for (int q = 0; q < FOLD_GROUPS; ++q) {
            const int jt = q * 4 * FOLD_THREADS + t * 4;
            const uint32_t f = fw[q] >> s;  // bit 8e: element e hit by slot s
            const float4 h4 = *reinterpret_cast<const float4*>(&hv[s][jt]);
            const f2v t01 = {(f & 0x1u) ? h4.x : base[q * 4 + 0], (f & 0x100u) ? h4.y : base[q * 4 + 1]};
            const f2v t23 = {(f & 0x10000u) ? h4.z : base[q * 4 + 2], (f & 0x1000000u) ? h4.w : base[q * 4 + 3]};
            if (first_term) {
              const f2v z = {0.0f, 0.0f};
              acc2[2 * q] = a.zero_base ? z + t01 * w2 : t01 * w2;
              acc2[2 * q + 1] = a.zero_base ? z + t23 * w2 : t23 * w2;
            } else {
              acc2[2 * q] = acc2[2 * q] + t01 * w2;
              acc2[2 * q + 1] = acc2[2 * q + 1] + t23 * w2;
            }
          }
        }
        __syncthreads();  // slots and flags free for the next phase
      }
      pa = pb;
    }
    float acc[4 * FOLD_GROUPS];
#pragma unroll
    for (int h = 0; h < 2 * FOLD_GROUPS; ++h) {
      acc[2 * h] = acc2[h].x;
      acc[2 * h + 1] = acc2[h].y;
    }
    if (a.add_self) {
#pragma unroll
      for (int e = 0; e < 4 * FOLD_GROUPS; ++e) acc[e] = acc[e] + L[e] * a.w_self;
    }
#pragma unroll
    for (int q = 0; q < FOLD_GROUPS; ++q) {
      const int64_t i0 = tlo + q * 4 * FOLD_THREADS + t * 4;
      if (VEC && i0 + 3 < thi) {
        const float4 r4 =
            make_float4(acc[q * 4 + 0], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]);
        *reinterpret_cast<float4*>(a.out + i0) = r4;
        if (a.out2) *reinterpret_cast<float4*>(a.out2 + i0) = r4;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < thi) {
            a.out[i0 + e] = acc[q * 4 + e];
            if (a.out2) a.out2[i0 + e] = acc[q * 4 + e];
          }
      }
    }
    if (tile + gridDim.x < a.ntiles) load_local(tile + gridDim.x);
    // no barrier here: every read of rng / pre / the slots of this tile happened before the
    // last phase's barrier (a group with no payload has no phase: np == 0 never reaches here)
  }  // tile loop
}

// blocks of the persistent fold grid: what the CUs hold at once (occupancy API)
static unsigned fold_grid(int slots, int64_t ntiles) {
  // DPZ_FOLD_BLOCKS=N caps the grid at N blocks (diagnostic build; 0 = the occupancy slots)
  const int64_t cap = DPZ_KNOB_INT(FOLD_BLOCKS, 0);
  const int64_t g = cap > 0 ? cap : slots;
  return (unsigned)(ntiles < g ? (ntiles > 0 ? ntiles : 1) : g);
}

template <bool VEC>
static int launch_tile_t(const FoldArgs& fa, bool group, hipStream_t st) {
  if (group) {
    static const int slots = cu_slots(reinterpret_cast<const void*>(fold_group_kernel<VEC>), FOLD_THREADS, 0);
    DPZ_TIMED(DPZ_KT_FOLD, st, fold_group_kernel<VEC><<<fold_grid(slots, fa.ntiles), FOLD_THREADS, 0, st>>>(fa));
  } else {
    static const int slots = cu_slots(reinterpret_cast<const void*>(fold_kernel<VEC>), FOLD_THREADS, 0);
    DPZ_TIMED(DPZ_KT_FOLD, st, fold_kernel<VEC><<<fold_grid(slots, fa.ntiles), FOLD_THREADS, 0, st>>>(fa));
  }
  return DPZ_OK;
}

int launch_fold_classic(const FoldArgs& fa, bool vec, hipStream_t st) {
  return vec ? launch_tile_t<true>(fa, false, st) : launch_tile_t<false>(fa, false, st);
}

int launch_fold_group(const FoldArgs& fa, bool vec, hipStream_t st) {
  return vec ? launch_tile_t<true>(fa, true, st) : launch_tile_t<false>(fa, true, st);
}

// the pre-pass over the group's sparse payloads: starts[p][0 .. ntiles]
int launch_fold_offsets(const FoldArgs& fa, int32_t* starts, hipStream_t st) {
  int64_t kmax = -1;
  for (int i = 0; i < fa.np; ++i)
    if (fa.p[i].idx && fa.p[i].k > kmax) kmax = fa.p[i].k;
  if (kmax < 0) return DPZ_OK;
  dim3 og((unsigned)((kmax + 1 + 1023) / 1024), (unsigned)fa.np);
  DPZ_TIMED(DPZ_KT_FOLD_OFFSETS, st, fold_offsets_kernel<FOLD_TILE_SHIFT><<<og, 256, 0, st>>>(fa, starts, fa.ntiles));
  return DPZ_OK;
}

}  // namespace dpz

using namespace dpz;

#ifdef DPZ_STAMPS
extern "C" int dpz_debug_fold_stamps(unsigned long long* host_out, int reset) {
  if (host_out) DPZ_HIP_TRY(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fold_st), sizeof(g_fold_st)));
  if (reset) {
    static unsigned long long zero[6][8192];
    DPZ_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_fold_st), zero, sizeof(zero)));
  }
  return 0;
}
#endif
