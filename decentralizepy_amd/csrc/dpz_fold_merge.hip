// The merge fold: a group of sparse payloads merged per tile through an LDS hit mask
// (the JWINS receive, 16 payloads at alpha 0.01: reference Wavelet.py:269-309).
// A persistent block walks a contiguous run of TE-element tiles.  Wave w holds the 64-entry
// windows of payloads w, w + 4, w + 8, w + 12 (the next tile's windows and local values are
// issued one tile ahead, so the stream's loads are in flight while a tile is merged).  Per tile:
//   1. every payload's entries in the tile (the leading window lanes below the tile's end) set
//      bit p of their element's 16-bit word in an LDS mask; meanwhile every element folds its
//      local value alone (the no-hit base; the elements advance through the terms together);
//   2. each wave numbers its own elements' bits (a wave scan): every hit element gets a run of
//      value slots in the wave's region, in payload order (the rank of bit p among its bits);
//   3. every entry writes its value to its slot;
//   4. each wave lists its own hit elements (ballots) and its lanes fold them exactly — term p
//      = (bit p ? slot value : local) * w_p in payload order, then the self term (the
//      reference's fp32 order) — over the base.
// Three block barriers per tile.  Every element's local value and output are read / written
// once, every payload entry read once (extra windows of a payload denser than 64 entries per
// tile are re-read from L2).  A tile whose entries exceed a wave's value slots (1 per element;
// adversarial clustering) folds payload by payload instead.  Weights all equal (EQW: a regular
// graph's Metro-Hastings weights): the base is one product and np - 1 additions of it, the same
// bits as the general order.  (Two hit elements per lane at a time, two independent chains, was
// measured and not kept: C3 16 x 0.01 105 -> 111 us, 16 x 0.005 88 -> 106 at 4 waves per SIMD.)
#include "dpz_fold_cursor.h"

// (the kernel keeps its unqualified symbol name, which the recorded profiles carry: this unit's
// definitions sit outside namespace dpz)
using namespace dpz;

constexpr int FM_THREADS = 256;
constexpr int FM_WAVES = FM_THREADS / 64;
constexpr int FM_SLOTS = FOLD_MAXP / FM_WAVES;  // payload slots per wave: payload wid + 4 j

template <int EPT>
struct FmCfg {
  static constexpr int TE = FM_THREADS * EPT;  // elements per tile (= value slots per tile)
  static_assert(EPT % 4 == 0 && TE <= 65535, "float4 chunks, u16 slot offsets");
};

// element e of thread t (chunk e / 4 at (e / 4) * 4 * FM_THREADS + 4 t + e % 4: float4-coalesced)
__device__ __forceinline__ int fm_elem(int t, int e) {
  return (e >> 2) * (4 * FM_THREADS) + 4 * t + (e & 3);
}

// Branch-free (the compiler then waits only for the registers it uses, never for the next
// tile's loads in flight): a float4 group reaching past n reads the last whole group instead; the
// global last tile, if ragged, is reloaded element-wise by fm_load_tail before use.
template <int EPT>
__device__ __forceinline__ void fm_load(const float* __restrict__ p, int64_t tlo, int64_t n, int t,
                                        float (&v)[EPT]) {
  const int64_t last = (n & ~int64_t(3)) - 4;
#pragma unroll
  for (int c = 0; c < EPT / 4; ++c) {
    const int64_t i0 = tlo + fm_elem(t, 4 * c);
    const float4 q = *reinterpret_cast<const float4*>(p + (i0 + 4 <= n ? i0 : last));
    v[4 * c] = q.x; v[4 * c + 1] = q.y; v[4 * c + 2] = q.z; v[4 * c + 3] = q.w;
  }
}

template <int EPT>
__device__ __forceinline__ void fm_load_tail(const float* __restrict__ p, int64_t tlo, int64_t n,
                                             int t, float (&v)[EPT]) {
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int64_t i = tlo + fm_elem(t, e);
    v[e] = p[i < n ? i : n - 1];
  }
}

template <int EPT>
__device__ __forceinline__ void fm_store(float* __restrict__ p, int64_t tlo, int64_t n, int t,
                                         const float (&v)[EPT]) {
  constexpr int TE = FmCfg<EPT>::TE;
  typedef float v4f __attribute__((ext_vector_type(4)));
  if (tlo + TE <= n) {
#pragma unroll
    for (int c = 0; c < EPT / 4; ++c) {
      const v4f q = {v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]};
      __builtin_nontemporal_store(q, reinterpret_cast<v4f*>(p + tlo + fm_elem(t, 4 * c)));
    }
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int64_t i = tlo + fm_elem(t, e);
      if (i < n) p[i] = v[e];
    }
  }
}

template <int EPT, bool EQW>
__global__ void __launch_bounds__(FM_THREADS) __attribute__((amdgpu_waves_per_eu(EPT <= 8 ? 4 : 2, 8))) fold_merge_kernel(FoldArgs a, int64_t tpb, int abl) {
  using C = FmCfg<EPT>;
  constexpr int TE = C::TE;
  constexpr int WE = 64 * EPT;     // elements of one wave (its value slots: WE, 1 per element)
  // element e's payload bits: the 16-bit half (e & 1) of word e / 2 (np <= 16)
  __shared__ __attribute__((aligned(16))) uint32_t s_mask[2][TE / 2];
  __shared__ __attribute__((aligned(16))) uint16_t s_pre[TE];
  __shared__ __attribute__((aligned(16))) float s_x[TE];
  __shared__ float s_val[TE];
  __shared__ uint16_t s_list[TE];
  __shared__ uint32_t s_over[2];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t n = a.n;
  const int np = a.np;
  const int64_t ntl = (n + TE - 1) / TE;
  const int64_t t0 = (int64_t)blockIdx.x * tpb;
  const int64_t t1 = t0 + tpb < ntl ? t0 + tpb : ntl;
  if (t0 >= t1) return;  // uniform over the block
  // payload parameters: lane p holds payload p's, read back per slot / per chain step (readlane)
  const int lp = lane < np ? lane : 0;
  const uint64_t ipl = reinterpret_cast<uint64_t>(a.p[lp].k > 0 ? a.p[lp].idx
                                                                : reinterpret_cast<const int32_t*>(a.local));
  const uint64_t vpl = reinterpret_cast<uint64_t>(a.p[lp].k > 0 ? a.p[lp].val : a.local);
  const int32_t kl = lane < np ? (int32_t)a.p[lp].k : 0;
  const float wl = a.p[lp].w;
  auto rl64 = [](uint64_t v, int p) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, p);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), p);
    return ((uint64_t)hi << 32) | lo;
  };
  auto W = [&](int p) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), p)); };
  const int32_t* sidx[FM_SLOTS];
  const float* sval[FM_SLOTS];
  int32_t sk[FM_SLOTS];
#pragma unroll
  for (int j = 0; j < FM_SLOTS; ++j) {
    const int p = wid + FM_WAVES * j;
    const bool live = p < np;
    sidx[j] = reinterpret_cast<const int32_t*>(rl64(ipl, live ? p : 0));
    sval[j] = reinterpret_cast<const float*>(rl64(vpl, live ? p : 0));
    sk[j] = live ? fw_uni(__builtin_amdgcn_readlane(kl, p)) : 0;
  }
  const int nsl = np > wid ? (np - wid + FM_WAVES - 1) / FM_WAVES : 0;  // this wave's live slots
  for (int i = t; i < TE; i += FM_THREADS) (&s_mask[0][0])[i] = 0u;
  if (t < 2) s_over[t] = 0u;
  // start cursors: lower_bound(idx_p, t0 * TE) of this wave's payloads (lane j: slot j)
  const int32_t curv = fw_start_cursors<FM_SLOTS>(
      nsl, (int32_t)(t0 * TE), lane, [&](int j) { return sidx[j]; }, [&](int j) { return sk[j]; },
      reinterpret_cast<const int32_t*>(a.local));
  int32_t cs[FM_SLOTS];
#pragma unroll
  for (int j = 0; j < FM_SLOTS; ++j) cs[j] = fw_uni(__builtin_amdgcn_readlane(curv, j));
  int32_t wi[FM_SLOTS], wn[FM_SLOTS];
  float wv[FM_SLOTS], wvn[FM_SLOTS];
  auto load_window = [&](int j, int32_t c, int32_t& ix, float& vx) {
    const int32_t q = c + lane;
    const bool ok = q < sk[j];
    const int32_t qq = ok ? q : 0;
    ix = as_global(sidx[j])[qq];
    vx = as_global(sval[j])[qq];
    ix = ok ? ix : INT32_MAX;
  };
#pragma unroll
  for (int j = 0; j < FM_SLOTS; ++j) load_window(j, cs[j], wi[j], wv[j]);
  float L[EPT], Ln[EPT];
  fm_load<EPT>(a.local, t0 * TE, n, t, L);
  const float w0 = W(0);
  uint32_t buf = 0;
  const int zb = a.zero_base;
  __syncthreads();  // masks zeroed
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t tlo = tile * TE;
    const int32_t tlo32 = (int32_t)tlo, thi32 = tlo32 + TE;
    uint32_t* const mask = s_mask[buf];
    if (tlo + TE > n) fm_load_tail<EPT>(a.local, tlo, n, t, L);  // the ragged last tile
    // 1. mask bits of every payload's entries in the tile; the next tile's windows issued
    int32_t c0[FM_SLOTS], cfirst[FM_SLOTS];
#pragma unroll
    for (int j = 0; j < FM_SLOTS; ++j) {
      c0[j] = cs[j];
      cfirst[j] = 0;
      if (j >= nsl) continue;  // uniform
      const int p = wid + FM_WAVES * j;
      int32_t c = fw_lead(wi[j] < thi32);
      cfirst[j] = c;
      if (!(abl & 4)) {
        const uint32_t pos = (uint32_t)(wi[j] - tlo32);
        if (lane < c && pos < (uint32_t)TE) atomicOr(&mask[pos >> 1], 1u << (p + 16 * (pos & 1u)));
      }
      if (c == 64) {  // a payload denser than one window per tile: its further windows now
        for (int32_t q0 = cs[j] + 64;; q0 += 64) {
          const int32_t q = q0 + lane;
          const int32_t iv = q < sk[j] ? as_global(sidx[j])[q] : INT32_MAX;
          const int cc = fw_lead(iv < thi32);
          const uint32_t pos = (uint32_t)(iv - tlo32);
          if (lane < cc && pos < (uint32_t)TE) atomicOr(&mask[pos >> 1], 1u << (p + 16 * (pos & 1u)));
          c += cc;
          if (cc < 64) break;
        }
      }
      cs[j] = cs[j] + c;
    }
#pragma unroll
    for (int j = 0; j < FM_SLOTS; ++j) load_window(j, cs[j], wn[j], wvn[j]);
    fm_load<EPT>(a.local, tile + 1 < t1 ? tlo + TE : tlo, n, t, Ln);  // (the run's last: L2)
    // the base: every element's fold of its local value alone (the no-hit value); the elements
    // advance through the terms together (independent adds, one loop for all), while other
    // waves still set mask bits
    float base[EPT];
    if (abl & 8) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) base[e] = L[e];
    } else {
      float tw[EPT];
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        tw[e] = (zb ? 0.0f : L[e]) * w0;
        base[e] = zb ? 0.0f + tw[e] : tw[e];
      }
      for (int p = 1; p < np; ++p) {
        if (EQW) {
#pragma unroll
          for (int e = 0; e < EPT; ++e) base[e] = base[e] + tw[e];
        } else {
          const float w = W(p);
#pragma unroll
          for (int e = 0; e < EPT; ++e) base[e] = base[e] + (zb ? 0.0f : L[e]) * w;
        }
      }
      if (a.add_self) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) base[e] = base[e] + L[e] * a.w_self;
      }
    }
    __syncthreads();  // B1: the tile's mask is complete; the previous tile is done everywhere
    // 2. per-element value runs: each wave numbers its own elements' entries (slots of the
    // wave's region, in payload order per element); the local values staged for the hit folds
    uint32_t m[EPT];
#pragma unroll
    for (int c = 0; c < EPT / 4; ++c) {
      const uint2 q = *reinterpret_cast<const uint2*>(&mask[fm_elem(t, 4 * c) >> 1]);
      m[4 * c] = q.x & 0xFFFFu; m[4 * c + 1] = q.x >> 16;
      m[4 * c + 2] = q.y & 0xFFFFu; m[4 * c + 3] = q.y >> 16;
      *reinterpret_cast<float4*>(&s_x[fm_elem(t, 4 * c)]) =
          make_float4(L[4 * c], L[4 * c + 1], L[4 * c + 2], L[4 * c + 3]);
    }
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) mine += (uint32_t)__popc(m[e]);
    uint32_t wtot = 0;
    uint32_t run = (abl & 16) ? 0u : wave_excl_scan(mine, &wtot) + (uint32_t)(wid * WE);
    if (wtot > (uint32_t)WE && lane == 0) s_over[buf] = 1u;  // (uniform read after B3)
#pragma unroll
    for (int c = 0; c < EPT / 4; ++c) {
      uint32_t pr[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pr[e] = run < 65535u ? run : 65535u;
        run += (uint32_t)__popc(m[4 * c + e]);
      }
      *reinterpret_cast<uint2*>(&s_pre[fm_elem(t, 4 * c)]) =
          make_uint2(pr[0] | (pr[1] << 16), pr[2] | (pr[3] << 16));
    }
    __syncthreads();  // B3: every element's slot run known
    const bool over = s_over[buf] != 0u;  // uniform
    if (!over) {
      // 3. values into their slots (slot = the run start + the rank of bit p among the bits)
      if (!(abl & 2)) {
#pragma unroll
        for (int j = 0; j < FM_SLOTS; ++j) {
          if (j >= nsl) continue;
          const int p = wid + FM_WAVES * j;
          const uint32_t below = (1u << p) - 1u;
          auto place = [&](int32_t iv, float vv, bool in) {
            const uint32_t pos = (uint32_t)(iv - tlo32);
            if (in && pos < (uint32_t)TE) {
              const uint32_t mm = (mask[pos >> 1] >> (16 * (pos & 1u))) & 0xFFFFu;
              const uint32_t slot = (uint32_t)s_pre[pos] + (uint32_t)__popc(mm & below);
              if (slot < (uint32_t)TE) s_val[slot] = vv;
            }
          };
          place(wi[j], wv[j], lane < cfirst[j]);
          if (cfirst[j] == 64) {
            for (int32_t q0 = c0[j] + 64;; q0 += 64) {
              const int32_t q = q0 + lane;
              const bool ok = q < sk[j];
              const int32_t iv = ok ? as_global(sidx[j])[q] : INT32_MAX;
              const float vv = as_global(sval[j])[ok ? q : 0];
              const int cc = fw_lead(iv < thi32);
              place(iv, vv, lane < cc);
              if (cc < 64) break;
            }
          }
        }
      }
      __syncthreads();  // B4: every value in its slot
      // 4. the wave's own hit elements, listed (ballot order) and folded exactly by its lanes
      // (reference order: the payload terms, then the self term); results over the staged
      // local values, then over the base
      if (!(abl & 1)) {
        uint16_t* const wl_ = s_list + wid * WE;
        uint32_t nh = 0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const uint64_t b = __ballot(m[e] != 0u);
          if (m[e])
            wl_[nh + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                               __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] =
                (uint16_t)fm_elem(t, e);
          nh += (uint32_t)__popcll(b);
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = (uint32_t)lane; i < nh; i += 64) {
          const uint32_t pos = wl_[i];
          const uint32_t mm = (mask[pos >> 1] >> (16 * (pos & 1u))) & 0xFFFFu;
          const uint32_t sl = s_pre[pos];
          const float xv = s_x[pos];
          const float tb = zb ? 0.0f : xv;
          const int p0 = __ffs((int)mm) - 1;
          const uint32_t mm1 = mm & (mm - 1u);
          const int p1 = mm1 ? __ffs((int)mm1) - 1 : 32;
          const uint32_t mm2 = mm1 & (mm1 - 1u);
          const int p2 = mm2 ? __ffs((int)mm2) - 1 : 32;
          float acc;
          if (abl & 32) {  // (timing ablation: the chain skipped, its loads kept)
            acc = s_val[sl < (uint32_t)TE ? sl : 0u] + tb + (float)p0 + (float)p1 + (float)p2;
          } else if ((mm2 & (mm2 - 1u)) == 0u) {  // one to three payloads hit it (all but ~1e-4)
            const float v0 = s_val[sl < (uint32_t)TE ? sl : 0u];
            const float v1 = s_val[sl + 1u < (uint32_t)TE ? sl + 1u : 0u];
            const float v2 = s_val[sl + 2u < (uint32_t)TE ? sl + 2u : 0u];
            acc = 0.0f;
            if (EQW) {  // every product once (equal weights: the same bits as w_p each term)
              const float xw = tb * w0, v0w = v0 * w0, v1w = v1 * w0, v2w = v2 * w0;
#pragma unroll
              for (int p = 0; p < FOLD_MAXP; ++p) {
                if (p >= np) break;
                const float term = p == p0 ? v0w : (p == p1 ? v1w : (p == p2 ? v2w : xw));
                acc = p == 0 ? (zb ? 0.0f + term : term) : acc + term;
              }
            } else {
#pragma unroll
              for (int p = 0; p < FOLD_MAXP; ++p) {
                if (p >= np) break;
                const float tv = p == p0 ? v0 : (p == p1 ? v1 : (p == p2 ? v2 : tb));
                const float term = tv * W(p);
                acc = p == 0 ? (zb ? 0.0f + term : term) : acc + term;
              }
            }
          } else {  // four or more (adversarial overlap): payload by payload from the slots
            uint32_t s2 = sl;
            acc = 0.0f;
            for (int p = 0; p < np; ++p) {
              float tv = tb;
              if ((mm >> p) & 1u) {
                tv = s_val[s2 < (uint32_t)TE ? s2 : 0u];
                ++s2;
              }
              const float term = tv * W(p);
              acc = p == 0 ? (zb ? 0.0f + term : term) : acc + term;
            }
          }
          if (a.add_self) acc = acc + xv * a.w_self;
          s_x[pos] = acc;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < EPT / 4; ++c) {
          const float4 q = *reinterpret_cast<const float4*>(&s_x[fm_elem(t, 4 * c)]);
          const float h[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (m[4 * c + e]) base[4 * c + e] = h[e];
        }
      }
    } else {
      // more entries than a wave's value slots: payload by payload, an LDS value tile tagged
      // with p + 1 (adversarially clustered payloads)
      uint16_t* const tag = s_pre;  // (the runs are not used on this path)
      float* const vt = s_val;
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        base[e] = 0.0f;
        tag[fm_elem(t, e)] = 0;
      }
      __syncthreads();
      for (int p = 0; p < np; ++p) {
        if ((p & (FM_WAVES - 1)) == wid) {
          const int j = p / FM_WAVES;
          for (int32_t q0 = c0[j];; q0 += 64) {
            const int32_t q = q0 + lane;
            const bool ok = q < sk[j];
            const int32_t iv = ok ? as_global(sidx[j])[q] : INT32_MAX;
            const float vv = as_global(sval[j])[ok ? q : 0];
            const int cc = fw_lead(iv < thi32);
            const uint32_t pos = (uint32_t)(iv - tlo32);
            if (lane < cc && pos < (uint32_t)TE) {
              vt[pos] = vv;
              tag[pos] = (uint16_t)(p + 1);
            }
            if (cc < 64) break;
          }
        }
        __syncthreads();
        const float w = W(p);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
          const int el = fm_elem(t, e);
          const float tb = zb ? 0.0f : L[e];
          const float tv = tag[el] == (uint16_t)(p + 1) ? vt[el] : tb;
          const float term = tv * w;
          base[e] = p == 0 ? (zb ? 0.0f + term : term) : base[e] + term;
        }
        __syncthreads();
      }
      if (a.add_self) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) base[e] = base[e] + L[e] * a.w_self;
      }
    }
    fm_store<EPT>(a.out, tlo, n, t, base);
    if (a.out2) fm_store<EPT>(a.out2, tlo, n, t, base);
    // this buffer's mask words and overflow flag back to zero (the next tile uses the other pair)
#pragma unroll
    for (int c = 0; c < EPT / 4; ++c)
      *reinterpret_cast<uint2*>(&mask[fm_elem(t, 4 * c) >> 1]) = make_uint2(0u, 0u);
    if (t == 0) s_over[buf] = 0u;
    buf ^= 1u;
#pragma unroll
    for (int j = 0; j < FM_SLOTS; ++j) {
      wi[j] = wn[j];
      wv[j] = wvn[j];
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) L[e] = Ln[e];
  }
}

// The merge fold's launch: a persistent grid of what the CUs hold, each block a contiguous run.
template <int EPT, bool EQW>
static int launch_merge_t(const FoldArgs& fa, hipStream_t st) {
  static const int slots =
      cu_slots(reinterpret_cast<const void*>(fold_merge_kernel<EPT, EQW>), FM_THREADS, 0);
  constexpr int TE = FmCfg<EPT>::TE;
  const int64_t ntl = (fa.n + TE - 1) / TE;
  int64_t blocks = slots;
  if (DPZ_KNOB_INT(MERGE_BLOCKS, 0) > 0) blocks = DPZ_KNOB_INT(MERGE_BLOCKS, 0);
  if (blocks > ntl) blocks = ntl;
  if (blocks < 1) blocks = 1;
  const int64_t tpb = (ntl + blocks - 1) / blocks;
  blocks = (ntl + tpb - 1) / tpb;
  // DPZ_MERGE_ABL (diagnostic build, timing only: results then differ) skips phases: 1 the hit
  // folds, 2 the value placement, 4 the mask bits, 8 the base, 16 the scan
  const int abl = (int)DPZ_KNOB_INT(MERGE_ABL, 0);
  DPZ_TIMED(DPZ_KT_FOLD, st, (fold_merge_kernel<EPT, EQW><<<(unsigned)blocks, FM_THREADS, 0, st>>>(fa, tpb, abl)));
  return DPZ_OK;
}

// the plan's tile width (elements per thread) and equal-weights form
int dpz::launch_merge(const FoldArgs& fa, const FoldPlan& pl, hipStream_t st) {
  const bool eqw = pl.eqw != 0;
  switch (pl.ept) {
    case 4: return eqw ? launch_merge_t<4, true>(fa, st) : launch_merge_t<4, false>(fa, st);
    case 16: return eqw ? launch_merge_t<16, true>(fa, st) : launch_merge_t<16, false>(fa, st);
    default: return eqw ? launch_merge_t<8, true>(fa, st) : launch_merge_t<8, false>(fa, st);
  }
}
