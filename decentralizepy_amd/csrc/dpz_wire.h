// The block geometry and the per-block device helpers of the two payload stream coders, shared by
// the single-stream kernels (dpz_elias.hip, dpz_fpz.hip) and the batched coder and decoder of a
// rank's nodes (dpz_wire_nodes.hip, dpz_wire_decode_nodes.hip): one definition of the Elias code
// length, of the speculative chunk parse and of the block-floating planes, so the batched streams
// are the single-stream bytes and the batched decode reads them the same way by construction.
#pragma once
#include "dpz_common.h"

namespace dpz {

// ---- Elias-gamma index gaps (format: dpz_elias.hip) ----------------------------------------------
constexpr int EL_CODES = 1024;   // codes per encode block (4 per thread)

__device__ __forceinline__ uint32_t code_len(uint32_t g) { return 2u * (31u - __clz(g)) + 1u; }

constexpr int EL_CHUNK = 1024;       // bits per decode chunk
constexpr int EL_CW = EL_CHUNK / 32;
constexpr int EL_STAGE = EL_CW + 4;  // staged words per chunk (a code may run 62 bits past)
constexpr int EL_SUPER = 64;         // chunks per super map
constexpr int EL_MAX_SUPER = 1024;   // => at most 2^26 code bits per stream

// 64 stream bits from bit `rel` of the staged (bit-ordered) words; reads words[rel / 32 + 2] at most
__device__ __forceinline__ uint64_t window64(const uint32_t* words, uint64_t rel) {
  const int wi = (int)(rel >> 5);
  const uint32_t sh = (uint32_t)(rel & 31);
  const uint64_t a = ((uint64_t)words[wi] << 32) | words[wi + 1];
  return sh ? ((a << sh) | (words[wi + 2] >> (32 - sh))) : a;
}

// Lanes 0 .. EL_STAGE - 1 of a wave stage chunk c's words in bit order (zero past the stream's
// nwords_in code words, and all of them for valid == false); the caller synchronises.
__device__ __forceinline__ void el_stage_chunk(const uint32_t* __restrict__ in32,
                                               uint64_t nwords_in, int64_t c, bool valid, int lane,
                                               uint32_t* st) {
  if (lane < EL_STAGE) {
    const uint64_t w = (uint64_t)c * EL_CW + lane;
    st[lane] = (valid && w < nwords_in) ? __builtin_bswap32(in32[w]) : 0u;
  }
}

// The speculative parse of chunk c of a stream of L code bits from its staged words: lane o walks
// the codes as if one started at bit o of the chunk.  Returns the exit offset into the next chunk
// (< 63; 0xFF for lane 63, a run of more than 31 zeros or no code), the codes walked, their gap sum.
__device__ __forceinline__ uint8_t el_parse_chunk(const uint32_t* st, int64_t c, uint64_t L,
                                                  int lane, uint32_t* cnt_out, uint64_t* sum_out) {
  const uint64_t cstart = (uint64_t)c * EL_CHUNK;
  const uint64_t cend = (cstart + EL_CHUNK < L) ? cstart + EL_CHUNK : L;
  uint64_t pos = cstart + lane;
  uint32_t cnt = 0;
  uint64_t gsum = 0;
  uint8_t ex = 0xFF;
  if (lane < 63 && pos < cend) {
    bool ok = true;
    while (pos < cend) {
      const uint64_t w = window64(st, pos - cstart);
      const uint32_t z = (uint32_t)__clzll((long long)w);
      if (w == 0 || z > 31) { ok = false; break; }
      const uint32_t n = z + 1;
      const uint64_t gv = (w << z) >> (64 - n);
      gsum += gv;
      ++cnt;
      pos += 2 * z + 1;
    }
    if (ok) ex = (uint8_t)(pos - cend);  // < 63
  } else if (lane < 63 && pos >= cend) {
    ex = (uint8_t)(pos - cend);  // entry beyond this (last) chunk's end
  }
  *cnt_out = cnt;
  *sum_out = gsum;
  return ex;
}

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

__device__ __forceinline__ uint32_t fz_get(const uint32_t* __restrict__ p, uint32_t pos, int bits) {
  if (!bits) return 0u;
  const uint32_t wi = pos >> 5, sh = pos & 31u;
  uint64_t v = p[wi];
  if (sh + bits > 32) v |= (uint64_t)p[wi + 1] << 32;
  return (uint32_t)(v >> sh) & (bits == 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u));
}

// One wave decodes block b of a stream of n values whose header the caller has checked: in32 is
// the whole stream, `area` the words its block area may hold.  Returns false, with nothing
// written, for a bad table entry or meta word; reads stay inside the block's table range, writes
// inside out[b * FZ_B, b * FZ_B + cnt).
__device__ __forceinline__ bool fz_decode_block(const uint32_t* __restrict__ in32, int64_t area,
                                                int64_t n, int64_t nblk, int64_t b, int mb,
                                                int lane, float* __restrict__ out) {
  const uint32_t* table = in32 + 4;
  const uint32_t off = table[b], end = table[b + 1];
  const int64_t base = b * FZ_B;
  const int cnt = (int)((n - base) < FZ_B ? (n - base) : FZ_B);
  if (off >= end || (int64_t)end > area) return false;
  const uint32_t* blk = in32 + 4 + nblk + 1 + off;
  const uint32_t meta = blk[0];
  const int w = (int)((meta >> 8) & 0xFFu);
  if (w > 8 || (int)((meta >> 16) & 0xFFu) != mb || end - off != fz_words(cnt, w, mb) ||
      (meta >> 24) != 0u)
    return false;
  const uint32_t emin = meta & 0xFFu;
  const uint32_t* ps = blk + 1;
  const uint32_t* pe = ps + (cnt + 31) / 32;
  const uint32_t* pm = pe + (cnt * w + 31) / 32;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t j = 4u * lane + e;
    uint32_t u = 0;
    if ((int)j < cnt) {
      u = (fz_get(ps, j, 1) << 31) | (((emin + fz_get(pe, j * w, w)) & 0xFFu) << 23) |
          (fz_get(pm, j * mb, mb) << (23 - mb));
    }
    v[e] = __uint_as_float(u);
  }
  const int64_t i0 = base + 4 * lane;
  if (4 * lane + 3 < cnt && aligned16(out)) {
    *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * lane + e < cnt) out[i0 + e] = v[e];
  }
  return true;
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
