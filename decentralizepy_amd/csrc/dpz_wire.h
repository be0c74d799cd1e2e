// The block geometry and the per-block device helpers of the two payload stream coders, shared by
// the single-stream kernels (dpz_elias.hip, dpz_fpz.hip) and the batched coder of a rank's nodes
// (dpz_wire_nodes.hip): one definition of the Elias code length and of the block-floating planes,
// so the batched streams are the single-stream bytes by construction.
#pragma once
#include "dpz_common.h"

namespace dpz {

// ---- Elias-gamma index gaps (format: dpz_elias.hip) ----------------------------------------------
constexpr int EL_CODES = 1024;   // codes per encode block (4 per thread)

__device__ __forceinline__ uint32_t code_len(uint32_t g) { return 2u * (31u - __clz(g)) + 1u; }

// ---- block-floating fp32 values (format: dpz_fpz.hip) --------------------------------------------
constexpr int FZ_B = 256;                      // values per block (4 per lane of one wave)
constexpr int FZ_MAXW = 1 + 8 + 8 * 8 + 8 * 23;  // words of a full block at w = 8, mb = 23
constexpr uint32_t FZ_MAGIC = 0x5A465044u;     // "DPFZ"
constexpr int64_t FZ_MAXN = int64_t(1) << 30;  // values a stream (block offsets stay 32-bit)

__device__ __forceinline__ int fz_bits(uint32_t v) { return v ? 32 - __clz(v) : 0; }

__device__ __forceinline__ uint32_t fz_words(int cnt, int w, int mb) {
  return 1u + (uint32_t)((cnt + 31) / 32) + (uint32_t)((cnt * w + 31) / 32) +
         (uint32_t)((cnt * mb + 31) / 32);
}

// the 4 values of this lane (block-relative j = 4 * lane + e); exponent range over the wave
__device__ __forceinline__ void fz_load(const float* __restrict__ x, int64_t n, int64_t b,
                                        int prec, int lane, uint32_t u[4], int* cnt_out,
                                        uint32_t* emin_out, int* w_out) {
  const int64_t base = b * FZ_B;
  const int cnt = (int)((n - base) < FZ_B ? (n - base) : FZ_B);
  const int64_t i0 = base + 4 * lane;
  if (4 * lane + 3 < cnt && aligned16(x)) {
    const float4 v = *reinterpret_cast<const float4*>(x + i0);
    u[0] = __float_as_uint(v.x); u[1] = __float_as_uint(v.y);
    u[2] = __float_as_uint(v.z); u[3] = __float_as_uint(v.w);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = (4 * lane + e < cnt) ? __float_as_uint(x[i0 + e]) : 0u;
  }
  if (prec < 32) {  // keep the top `prec` bits; from 10 bits on a NaN keeps a mantissa bit
    const uint32_t keep = ~((1u << (32 - prec)) - 1u);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t t = u[e] & keep;
      const bool nan = (u[e] & 0x7F800000u) == 0x7F800000u && (u[e] & 0x7FFFFFu) != 0u;
      u[e] = (prec >= 10 && nan && (t & 0x7FFFFFu) == 0u) ? (t | 0x400000u) : t;
    }
  }
  uint32_t lo = 255u, hi = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (4 * lane + e < cnt) {
      const uint32_t ex = (u[e] >> 23) & 0xFFu;
      lo = ex < lo ? ex : lo;
      hi = ex > hi ? ex : hi;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t l2 = __shfl_xor(lo, d, 64), h2 = __shfl_xor(hi, d, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  *cnt_out = cnt;
  *emin_out = lo;
  *w_out = fz_bits(hi - lo);
}

// OR `v` (at most 32 bits wide, `bits` of them) into the LDS bit stream at bit `pos`
__device__ __forceinline__ void fz_put(uint32_t* s, uint32_t pos, uint32_t v, int bits) {
  if (!bits) return;
  const uint32_t wi = pos >> 5, sh = pos & 31u;
  const uint64_t v64 = (uint64_t)v << sh;
  if ((uint32_t)v64) atomicOr(&s[wi], (uint32_t)v64);
  if (sh + bits > 32 && (uint32_t)(v64 >> 32)) atomicOr(&s[wi + 1], (uint32_t)(v64 >> 32));
}

// One wave packs block b of x into its LDS stage `s` (FZ_MAXW + 1 words) and stores the block's
// words to dst: the meta word, then the sign, exponent and mantissa planes.  Whole waves only.
__device__ __forceinline__ void fz_pack_block(const float* __restrict__ x, int64_t n, int64_t b,
                                              int prec, int mb, int lane, uint32_t* s,
                                              uint32_t* __restrict__ dst) {
  for (int q = lane; q < FZ_MAXW + 1; q += 64) s[q] = 0u;
  uint32_t u[4], emin;
  int cnt, w;
  fz_load(x, n, b, prec, lane, u, &cnt, &emin, &w);
  const uint32_t ps = 1u, pe = ps + (uint32_t)((cnt + 31) / 32);
  const uint32_t pm = pe + (uint32_t)((cnt * w + 31) / 32);
  const uint32_t nw = pm + (uint32_t)((cnt * mb + 31) / 32);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t j = 4u * lane + e;
    if ((int)j < cnt) {
      fz_put(s + ps, j, u[e] >> 31, 1);
      fz_put(s + pe, j * w, ((u[e] >> 23) & 0xFFu) - emin, w);
      fz_put(s + pm, j * mb, (u[e] & 0x7FFFFFu) >> (23 - mb), mb);
    }
  }
  if (lane == 0) s[0] = emin | ((uint32_t)w << 8) | ((uint32_t)mb << 16);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t q = lane; q < nw; q += 64) dst[q] = s[q];
}

// stored precision (32 = lossless) and mantissa bits of a requested precision; -1 if invalid
static inline int fz_mbits(int precision, int* prec_out) {
  if (precision < 0) return -1;
  if (precision == 0 || precision >= 32) {
    *prec_out = 32;
    return 23;
  }
  *prec_out = precision;
  return precision > 9 ? precision - 9 : 0;
}

}  // namespace dpz
