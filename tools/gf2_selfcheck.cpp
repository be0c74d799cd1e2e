// Stand-alone check of the GF(2) jump-ahead (decentralizepy_amd/csrc/dpz_gf2.cpp) for a
// sanitizer build on the host: the characteristic polynomial, both table levels and a handful of
// jumps through dpz_mt_raw_host against plain stepping of MT19937.  No GPU, no Python:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/gf2_selfcheck.cpp decentralizepy_amd/csrc/dpz_gf2.cpp -pthread -o gf2_selfcheck
//   ./gf2_selfcheck
#include <stdint.h>
#include <stdio.h>

#include <thread>
#include <vector>

#include "../include/dpz_codec.h"

namespace {

struct Plain {  // MT19937 by the textbook, one output at a time
  uint32_t mt[624];
  int idx = 624;
  explicit Plain(uint32_t seed) {
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i;
  }
  uint32_t next() {
    if (idx == 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
        mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};

int check(uint32_t seed, const std::vector<int64_t>& starts, int64_t window) {
  int64_t last = 0;
  for (int64_t s : starts) last = s > last ? s : last;
  std::vector<uint32_t> ref((size_t)(last + window));
  Plain p(seed);
  for (auto& v : ref) v = p.next();
  std::vector<uint32_t> got((size_t)window);
  int bad = 0;
  for (int64_t s : starts) {
    const int rc = dpz_mt_raw_host(seed, s, window, got.data());
    int64_t diff = -1;
    for (int64_t i = 0; rc == 0 && i < window; ++i)
      if (got[(size_t)i] != ref[(size_t)(s + i)]) {
        diff = i;
        break;
      }
    if (rc != 0 || diff >= 0) {
      printf("seed %u start %lld: rc %d, first difference at %lld\n", seed, (long long)s, rc,
             (long long)diff);
      ++bad;
    }
  }
  return bad;
}

}  // namespace

int main() {
  const int64_t S = dpz_mt_chunk_elems(), C = dpz_mt_coarse_chunks();
  std::vector<int64_t> starts = {0, 1, 623, S - 3, S, 3 * S + 17, 7 * S - 700};
  if (C) {
    starts.push_back((C - 1) * S + 600);
    starts.push_back(C * S - 5);
    starts.push_back(C * S + S + 1);
  }
  int bad = 0;
  // two threads race to build the tables first: the mutex-guarded lazy build
  int bad_t[2] = {0, 0};
  std::thread a([&] { bad_t[0] = check(5489u, starts, 1300); });
  std::thread b([&] { bad_t[1] = check(0xFFFFFFFFu, starts, 1300); });
  a.join();
  b.join();
  bad += bad_t[0] + bad_t[1];
  uint32_t one = 0;
  bad += dpz_mt_raw_host(1u, -1, 1, &one) != DPZ_ERR_ARG;
  bad += dpz_mt_raw_host(1u, 0, 1, nullptr) != DPZ_ERR_ARG;
  printf(bad ? "FAILED: %d\n" : "gf2 selfcheck ok (%d failures)\n", bad);
  return bad ? 1 : 0;
}
