// GF(2) side of the MT19937 jump-ahead (dpz_mt.h): the characteristic polynomial phi by
// Berlekamp-Massey on one output bit, t^J mod phi by square-and-multiply, the lazily built
// per-process tables of jump polynomials, and the host replay of the stream through those
// tables (dpz_mt_raw_host).  Plain C++: no device code, no HIP call.
#include <stdint.h>
#include <string.h>

#include <array>
#include <mutex>
#include <vector>

#include "../../include/dpz_codec.h"
#include "dpz_mt.h"

namespace dpz {
namespace mt {
namespace {

constexpr int PW = (DEG + 63) / 64;  // 312 64-bit words hold a residue (degree < 19937)
using Poly = std::array<uint64_t, PW>;

void init_genrand(uint32_t seed, uint32_t* s) {
  s[0] = seed;
  for (int i = 1; i < N; ++i) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i;
}

// the next 624 raw words from the last 624
void next_block(const uint32_t* old, uint32_t* nw) {
  for (int k = 0; k < N - M; ++k) nw[k] = old[k + M] ^ twist(old[k], old[k + 1]);
  for (int k = N - M; k < N - 1; ++k) nw[k] = nw[k - (N - M)] ^ twist(old[k], old[k + 1]);
  nw[N - 1] = nw[M - 1] ^ twist(old[N - 1], nw[0]);
}

// Berlekamp-Massey over GF(2), bit-packed: the connection polynomial of s[0..ns) (bit i of
// `conn` = c_i, c_0 = 1, s[N] = sum_{i>=1} c_i s[N-i]); returns the linear complexity.
int berlekamp_massey(const std::vector<uint8_t>& s, std::vector<uint64_t>* conn) {
  const int ns = (int)s.size();
  const int nw = ns / 64 + 2;
  std::vector<uint64_t> C(nw, 0), B(nw, 0), T(nw), W(nw, 0);  // W: bit i = s[N - i]
  C[0] = B[0] = 1;
  int L = 0, m = 1;
  for (int n = 0; n < ns; ++n) {
    const int wl = n / 64 + 1;  // words that hold bits 0..n
    uint64_t carry = s[n];
    for (int i = 0; i < wl; ++i) {
      const uint64_t v = W[i];
      W[i] = (v << 1) | carry;
      carry = v >> 63;
    }
    uint64_t d = 0;
    for (int i = 0; i < wl; ++i) d ^= C[i] & W[i];
    if (__builtin_parityll(d)) {
      const bool grow = 2 * L <= n;
      if (grow) T = C;
      const int ws = m / 64, bs = m % 64;  // C ^= B << m
      for (int i = 0; i + ws < nw; ++i) {
        C[i + ws] ^= B[i] << bs;
        if (bs && i + ws + 1 < nw) C[i + ws + 1] ^= B[i] >> (64 - bs);
      }
      if (grow) {
        L = n + 1 - L;
        B.swap(T);
        m = 1;
      } else {
        ++m;
      }
    } else {
      ++m;
    }
  }
  *conn = C;
  return L;
}

struct Tables {
  bool tried = false, ok = false;
  std::vector<int> terms;    // exponents of phi below DEG (phi = t^DEG + sum t^e)
  std::vector<Poly> fine;    // fine[c] = t^(c * CHUNK) mod phi (fine[0] = 1)
  std::vector<Poly> coarse;  // coarse[d] = t^(d * COARSE * CHUNK) mod phi
};
std::mutex g_mu;
Tables g_tab;

// reduce a product (2 * PW words) modulo phi, in place; the residue is its low PW words
void reduce(uint64_t* c, const std::vector<int>& terms) {
  constexpr int KW = DEG / 64, KB = DEG % 64;  // t^DEG is bit KB of word KW
  for (int k = 2 * PW - 1; k >= KW; --k) {
    const int sh = k == KW ? KB : 0;
    for (;;) {  // a term within 64 of the top lands in the word being cleared: go round again
      const uint64_t w = c[k] >> sh;
      if (!w) break;
      c[k] ^= w << sh;
      const int base = 64 * k + sh - DEG;  // t^(DEG + base + b) = t^(base + b) * (phi - t^DEG)
      for (int e : terms) {
        const int p = base + e, pw = p / 64, pb = p % 64;
        c[pw] ^= w << pb;
        if (pb) c[pw + 1] ^= w >> (64 - pb);
      }
    }
  }
}

// a * b mod phi: a left-to-right comb with 4-bit windows, then reduce
Poly mulmod(const Poly& a, const Poly& b, const std::vector<int>& terms) {
  static thread_local std::vector<uint64_t> tab(16 * (PW + 1)), c(2 * PW + 2);
  for (int u = 0; u < 16; ++u) {  // tab[u] = u(t) * b(t), deg u < 4
    uint64_t* t = &tab[u * (PW + 1)];
    memset(t, 0, (PW + 1) * sizeof(uint64_t));
    for (int s = 0; s < 4; ++s) {
      if (!((u >> s) & 1)) continue;
      for (int i = 0; i < PW; ++i) {
        t[i] ^= b[i] << s;
        if (s) t[i + 1] ^= b[i] >> (64 - s);
      }
    }
  }
  std::fill(c.begin(), c.end(), 0);
  for (int k = 15; k >= 0; --k) {
    for (int j = 0; j < PW; ++j) {
      const unsigned u = (unsigned)(a[j] >> (4 * k)) & 15u;
      if (!u) continue;
      const uint64_t* t = &tab[u * (PW + 1)];
      uint64_t* dst = &c[j];
      for (int l = 0; l <= PW; ++l) dst[l] ^= t[l];
    }
    if (k) {
      for (int i = 2 * PW + 1; i > 0; --i) c[i] = (c[i] << 4) | (c[i - 1] >> 60);
      c[0] <<= 4;
    }
  }
  reduce(c.data(), terms);
  Poly r;
  memcpy(r.data(), c.data(), PW * sizeof(uint64_t));
  return r;
}

// phi, once per process (g_mu held): Berlekamp-Massey on bit 0 of x[1..] of a non-zero seed
bool ensure_phi() {
  Tables& t = g_tab;
  if (t.tried) return t.ok;
  t.tried = true;
  const int ns = 2 * DEG + 10;
  std::vector<uint8_t> s(ns);
  std::vector<uint32_t> a(N), b(N);
  init_genrand(4357u, a.data());
  int pos = 1, have = 0;  // s[have] = bit 0 of x[1 + have]
  while (have < ns) {
    for (; pos < N && have < ns; ++pos) s[have++] = a[pos] & 1u;
    next_block(a.data(), b.data());
    a.swap(b);
    pos = 0;
  }
  std::vector<uint64_t> conn;
  if (berlekamp_massey(s, &conn) != DEG) return false;
  for (int i = 1; i <= DEG; ++i)  // phi(t) = t^DEG * conn(1/t): coefficient of t^(DEG-i) = c_i
    if ((conn[i / 64] >> (i % 64)) & 1) t.terms.push_back(DEG - i);
  if (t.terms.empty() || t.terms.back() != 0) return false;  // phi is irreducible: phi(0) = 1
  t.fine.reserve(COARSE);
  t.coarse.reserve(MAX_COARSE);
  Poly one{};
  one[0] = 1;
  t.fine.push_back(one);
  t.coarse.push_back(one);
  t.ok = true;
  return true;
}

// tab[0..upto] by tab[i] = tab[i-1] * tab[1]; tab[1] = seed_pow(), a power of t by squarings
template <class F>
const uint32_t* poly_at(std::vector<Poly>& tab, int idx, int limit, F first) {
  if (idx < 1 || idx >= limit) return nullptr;
  std::lock_guard<std::mutex> lock(g_mu);
  if (!ensure_phi()) return nullptr;
  if (tab.size() < 2) tab.push_back(first());
  while ((int)tab.size() <= idx) tab.push_back(mulmod(tab.back(), tab[1], g_tab.terms));
  return reinterpret_cast<const uint32_t*>(tab[idx].data());  // little-endian: bit i of word i/32
}

Poly pow2k(Poly g, int squarings) {
  for (int i = 0; i < squarings; ++i) g = mulmod(g, g, g_tab.terms);
  return g;
}

constexpr int log2c(int64_t v) { return v <= 1 ? 0 : 1 + log2c(v / 2); }
static_assert((CHUNK & (CHUNK - 1)) == 0 && (COARSE & (COARSE - 1)) == 0, "powers of two");

// the state in front of element J of the stream that starts at `st`: acc[j] = XOR x[i + j]
void jump(const uint32_t* poly, uint32_t* st) {
  std::vector<uint32_t> x((DEG / N + 3) * N);
  memcpy(x.data(), st, N * sizeof(uint32_t));
  for (size_t b = N; b + N <= x.size(); b += N) next_block(&x[b - N], &x[b]);
  uint32_t acc[N] = {0};
  for (int i = 0; i < DEG; ++i) {
    if (!((poly[i / 32] >> (i % 32)) & 1u)) continue;
    const uint32_t* src = &x[i];
    for (int j = 0; j < N; ++j) acc[j] ^= src[j];
  }
  memcpy(st, acc, sizeof(acc));
}

}  // namespace

const uint32_t* fine_poly(int c) {
  return poly_at(g_tab.fine, c, COARSE, [] {
    Poly t{};
    t[0] = 2;  // t
    return pow2k(t, log2c(CHUNK));
  });
}

const uint32_t* coarse_poly(int d) {
  if (d < 1 || d >= MAX_COARSE) return nullptr;
  if (!fine_poly(1)) return nullptr;
  return poly_at(g_tab.coarse, d, MAX_COARSE, [] { return pow2k(g_tab.fine[1], log2c(COARSE)); });
}

}  // namespace mt
}  // namespace dpz

extern "C" {

int64_t dpz_mt_chunk_elems(void) { return dpz::mt::CHUNK; }

int64_t dpz_mt_coarse_chunks(void) { return dpz::mt::COARSE; }

int dpz_mt_raw_host(uint32_t seed, int64_t start, int64_t count, uint32_t* out) {
  using namespace dpz::mt;
  if (start < 0 || count < 0 || !out || start > MAX_ELEMS - count) return DPZ_ERR_ARG;
  uint32_t st[N], nw[N];
  int64_t e = start;
  const int64_t end = start + count;
  while (e < end) {
    const int64_t chunk = e / CHUNK;  // jump to the enclosing chunk, then step
    const int d = (int)(chunk / COARSE), c = (int)(chunk % COARSE);
    init_genrand(seed, st);
    if (d) {
      const uint32_t* g = coarse_poly(d);
      if (!g) return DPZ_ERR_INTERNAL;
      jump(g, st);
    }
    if (c) {
      const uint32_t* g = fine_poly(c);
      if (!g) return DPZ_ERR_INTERNAL;
      jump(g, st);
    }
    const int64_t stop = (chunk + 1) * CHUNK < end ? (chunk + 1) * CHUNK : end;
    for (int64_t base = chunk * CHUNK; base < stop; base += N) {
      next_block(st, nw);
      memcpy(st, nw, sizeof(st));
      for (int m = 0; m < N; ++m) {
        const int64_t el = base + m;
        if (el >= e && el < stop) out[el - start] = temper(st[m]);
      }
    }
    e = stop;
  }
  return DPZ_OK;
}

}  // extern "C"
