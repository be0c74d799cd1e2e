// MT19937 jump-ahead: constants shared by the GF(2) host code (dpz_gf2.cpp) and the mask kernels
// (dpz_mt19937.hip).
//
// x[0..] are the raw (untempered) state words: x[0..623] after init_genrand(seed), then
// x[n+624] = x[n+397] ^ twist(x[n], x[n+1]); element e of torch.rand / numpy's stream is
// temper(x[624 + e]).  With g(t) = t^J mod phi(t) (phi: the degree-19937 characteristic
// polynomial), x[J+j] = XOR over {i : g_i = 1} of x[i+j] for j = 1..623, and for the top bit of
// x[J] (the recurrence never reads its other 31 bits).  So the state in front of element J is a
// GF(2) correlation of the first 19937 + 624 raw words with g, and g depends on J alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DPZ_MT_HD __host__ __device__
#else
#define DPZ_MT_HD  // plain C++ (dpz_gf2.cpp under a host compiler)
#endif

namespace dpz {
namespace mt {

constexpr int N = 624;               // state words
constexpr int M = 397;
constexpr int DEG = 19937;           // degree of phi
constexpr int POLY_U32 = 624;        // a jump polynomial as a bitmap: bit i of word i / 32
constexpr int64_t CHUNK = 1 << 16;   // elements per chunk (one block of the mask kernel)
constexpr int COARSE = 256;          // chunks per coarse step: two-level jumps above COARSE * CHUNK
constexpr int MAX_COARSE = 128;      // coarse steps: n < MAX_COARSE * COARSE * CHUNK = 2^31
constexpr int64_t MAX_ELEMS = (int64_t)MAX_COARSE * COARSE * CHUNK;

// Jump polynomials (host memory, POLY_U32 words, valid for the life of the process):
// fine_poly(c) = t^(c * CHUNK) mod phi, 1 <= c < COARSE; coarse_poly(d) = t^(d * COARSE * CHUNK)
// mod phi, 1 <= d < MAX_COARSE.  Built on first use up to the index asked for (g_c = g_{c-1} g_1),
// under one mutex; nullptr if the index is out of range or phi came out with another degree.
const uint32_t* fine_poly(int c);
const uint32_t* coarse_poly(int d);

DPZ_MT_HD inline uint32_t twist(uint32_t a, uint32_t b) {
  const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
  return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

DPZ_MT_HD inline uint32_t temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// torch's `rand(...) <= alpha` on the 24-bit draw: out24 <= threshold.  alpha is already fp32;
// -1 (nothing selected) for alpha < 0 or NaN, 2^24 selects everything.
inline int32_t mask_threshold(float alpha) {
  if (!(alpha >= 0.0f)) return -1;
  const double t = (double)alpha * 16777216.0;
  return t >= 16777216.0 ? (1 << 24) : (int32_t)t;  // t >= 0: the cast is floor
}

}  // namespace mt
}  // namespace dpz
