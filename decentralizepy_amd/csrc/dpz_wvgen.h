// The level rule and the symmetric extension shared by the generic-filter wavelet kernels
// (dpz_wvgen.hip, one node per call; dpz_wvgen_nodes.hip, every node of a table per launch).
#pragma once
#include "dpz_common.h"

namespace dpz {

constexpr int WG_FMAX = 64;
constexpr int WG_LMAX = 8;

struct WgLevels {
  int64_t len[WG_LMAX + 1];
  int64_t doff[WG_LMAX + 1];  // offset of cD_l in the coefficient array
  int64_t total;
};

static inline bool wg_levels(int64_t n, int level, int F, WgLevels* L) {
  if (n <= 0 || level < 1 || level > WG_LMAX || F < 2 || F > WG_FMAX || (F & 1)) return false;
  L->len[0] = n;
  for (int l = 1; l <= level; ++l) {
    if (L->len[l - 1] < F) return false;
    L->len[l] = (L->len[l - 1] + F - 1) / 2;
  }
  int64_t o = L->len[level];
  for (int l = level; l >= 1; --l) {
    L->doff[l] = o;
    o += L->len[l];
  }
  L->total = o;
  return true;
}

__device__ __forceinline__ int64_t wg_ext(int64_t p, int64_t n) {
  return p < 0 ? -1 - p : (p >= n ? 2 * n - 1 - p : p);
}

}  // namespace dpz
