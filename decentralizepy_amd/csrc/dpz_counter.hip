// The share counter kept as a ring of sent index lists, applied on read (dpz_counter_flush).
//
// Reference: sharing/PartialModel.py:205-207 (`shared_parameters_counter[indices] += 1` every
// round) whose only reader is the node's end-of-run dump (node/DPSGDNode.py:186-194).  Updating
// the int32 counter in the encode costs one scattered read-modify-write per selected index: at
// 1 % density nearly every index owns its 128-byte line, ~95 bytes of HBM traffic each (compact's
// PMC at 64 MiB: 19.3 MB for 3.4 MB of payload).  Instead the plugin keeps each round's payload
// indices (already written: the wire payload itself) in a device ring and folds the ring into the
// counter when it is read or full:
//   SCATTER : one atomic per ring entry (very few entries: one launch, no pass over the tiles)
//   SWEEP   : a bounds pass over the entries (where each segment enters each tile: a segment is a
//             strictly ascending payload), then one block per tile of CT counters: the tile is
//             read into LDS, every segment's entries inside it (a contiguous range) are added
//             with LDS atomics, the tile is written back — 8n coalesced bytes + 8 per entry,
//             whatever the number of rounds in the ring.
//   SPARSE  : the same ownership and bounds, but the LDS tile holds only the counts (a byte
//             per counter, from zero) and only the 64-byte sectors (16 counters) that hold one
//             are read, added to and written back: the traffic follows the sectors the ring
//             touches, with no global atomic, and a block takes a quarter of the LDS.
// A batch (dpz_counter_flush_batch) runs the tiles of several counters in one bounds launch and
// one tile launch: block -> (counter, tile) through the kernel-argument table's tile prefix.
#include "dpz_common.h"

#include <cmath>
#include <vector>

namespace dpz {
namespace {

constexpr int CT = 8192;     // counters per sweep tile (32 KB of LDS)
constexpr int CSEGS = 64;    // ring segments per counter and launch (offsets are kernel arguments)
constexpr int CB = 8;        // counters per batched launch (their tables are kernel arguments)
// DPZ_COUNTER_AUTO (auto_form): a call of B counters takes the scatter form for a counter with
// fewer than AUTO_SCATTER / sqrt(B) entries per counter, else the sparse form
constexpr double AUTO_SCATTER = 0.045;

// One counter's share of a launch: CSEGS or fewer segments of its ring, at 32-bit offsets from
// `ring` (the host rebases `ring` at the group's first segment and keeps a group under 2^32).
struct CounterItem {
  int32_t* counter;
  const int32_t* ring;
  int32_t* bounds;           // [m][tiles + 1], written by the bounds launch
  int64_t n;
  int64_t tiles;
  int64_t tile0;             // the launch's first block of this counter
  uint32_t off[CSEGS + 1];   // segment r = ring[off[r], off[r + 1])
  int32_t m;
};

struct CounterTab {
  CounterItem it[CB];
  int32_t cnt;
};

__global__ void __launch_bounds__(256) counter_scatter_kernel(int32_t* __restrict__ counter,
                                                              int64_t n,
                                                              const int32_t* __restrict__ ring,
                                                              int64_t total) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * 256) {
    const uint32_t i = (uint32_t)ring[j];
    if ((int64_t)i < n) atomicAdd(&counter[i], 1);
  }
}

// bounds[r * (tiles + 1) + t] = the first position q of segment r (relative to its start) whose
// index is >= t * CT, for t = 0 .. tiles: entry q writes the tiles its index opens (those after
// the previous entry's tile up to its own), the segment's last entry the tiles after it — every
// word once for an ascending segment.  Replaces a per-tile binary search (a chain of ~17
// dependent loads per segment in every sweep block).  Grid: (entries, segment, counter).
__global__ void __launch_bounds__(256) counter_bounds_kernel(const CounterTab tab) {
  const CounterItem& it = tab.it[blockIdx.z];
  const int r = blockIdx.y;
  if (r >= it.m) return;
  const int64_t tiles = it.tiles;
  const int32_t* __restrict__ ring = it.ring;
  const int64_t b = it.off[r], len = (int64_t)it.off[r + 1] - b;
  int32_t* br = it.bounds + (int64_t)r * (tiles + 1);
  if (len == 0) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t <= tiles;
         t += (int64_t)gridDim.x * 256)
      br[t] = 0;
    return;
  }
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < len;
       q += (int64_t)gridDim.x * 256) {
    const int64_t tv = (int64_t)(uint32_t)ring[b + q] / CT;
    const int64_t tp = q > 0 ? (int64_t)(uint32_t)ring[b + q - 1] / CT : -1;
    const int64_t hi = tv < tiles ? tv : tiles;
    for (int64_t t = tp + 1; t <= hi; ++t) br[t] = (int32_t)q;
    if (q == len - 1)
      for (int64_t t = (tv + 1 > tp + 1 ? tv + 1 : tp + 1); t <= tiles; ++t) br[t] = (int32_t)len;
  }
}


// The tile's block: which (counter, tile) a block of a launch is, through the table's prefix.
struct TileOf {
  int b;
  int64_t bt, t0;
  int cnt;     // counters in the tile (the last one is ragged)
  bool full;   // a whole tile of a 16-byte aligned counter: the int4 paths
};

__device__ __forceinline__ TileOf tile_of(const CounterTab& tab) {
  TileOf o;
  o.b = 0;
  while (o.b + 1 < tab.cnt && (int64_t)blockIdx.x >= tab.it[o.b + 1].tile0) ++o.b;
  const CounterItem& it = tab.it[o.b];
  o.bt = (int64_t)blockIdx.x - it.tile0;
  o.t0 = o.bt * CT;
  const int64_t t1 = o.t0 + CT < it.n ? o.t0 + CT : it.n;
  o.cnt = (int)(t1 - o.t0);
  o.full = o.cnt == CT && (reinterpret_cast<uintptr_t>(it.counter) & 15u) == 0;
  return o;
}

// Where every segment enters and leaves the tile (the bounds table), scanned into ONE index
// space [0, total) over the tile's entries of all segments: sb[r] = segment r's first entry of
// the tile, pre[r] = the tile's entries of segments < r.  Ends with the block's barrier (which
// also orders the caller's LDS tile set-up); returns total.
__device__ __forceinline__ int32_t tile_ranges(const CounterItem& it, const TileOf& o, int64_t* sb,
                                               int32_t* pre) {
  const int t = threadIdx.x, m = it.m;
  // segment t's entries inside the tile: one contiguous range of an ascending segment (clamped
  // to the segment: bounds of a segment that is not ascending are not trusted)
  int64_t lo = 0, hi = 0;
  if (t < m) {
    const int64_t so = it.off[t], len = (int64_t)it.off[t + 1] - so;
    const int32_t* br = it.bounds + (int64_t)t * (it.tiles + 1) + o.bt;
    int64_t a = br[0], e = br[1];
    a = a < 0 ? 0 : (a > len ? len : a);
    e = e < a ? a : (e > len ? len : e);
    lo = so + a;
    hi = so + e;
  }
  if (t < 64) {  // a wave scan of the per-segment counts (m <= 64)
    const int32_t c = t < m ? (int32_t)(hi - lo) : 0;
    int32_t v = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t u = __shfl_up(v, d, 64);
      if (t >= d) v += u;
    }
    if (t < m) {
      sb[t] = lo;
      pre[t] = v - c;
    }
    if (t == 63) pre[m] = v;
  }
  __syncthreads();
  return pre[m];
}

// add(i) for every entry of the tile, i its position in the tile: every thread takes entries
// j, j + 256, ... of the index space — the ring loads are independent (a loop per segment had
// put one load round trip per segment in series: 64 rounds, ~50 us per launch).
template <class Add>
__device__ __forceinline__ void tile_entries(const CounterItem& it, const TileOf& o,
                                             const int64_t* sb, const int32_t* pre, int32_t total,
                                             Add add) {
  const int32_t* __restrict__ ring = it.ring;
  const int m = it.m;
  constexpr int U = 4;
  for (int32_t j0 = threadIdx.x; j0 < total; j0 += 256 * U) {
    int32_t v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t j = j0 + 256 * u;
      v[u] = -1;
      if (j < total) {
        int a = 0, b = m - 1;  // the segment r with pre[r] <= j < pre[r + 1]
        while (a < b) {
          const int c = (a + b + 1) >> 1;
          if (pre[c] <= j) a = c; else b = c - 1;
        }
        v[u] = ring[sb[a] + (j - pre[a])];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // inside the tile for an ascending segment; checked all the same (a caller's unsorted
      // segment must not write outside the tile)
      const int64_t i = (int64_t)v[u] - o.t0;
      if (v[u] >= 0 && i >= 0 && i < o.cnt) add((int)i);
    }
  }
}

// The dense form, one block per (counter, tile): the tile is read into LDS, counted and written
// back whole.
__global__ void __launch_bounds__(256) counter_sweep_kernel(const CounterTab tab) {
  __shared__ int32_t tile[CT];
  __shared__ int64_t sb[CSEGS];
  __shared__ int32_t pre[CSEGS + 1];
  const TileOf o = tile_of(tab);
  const CounterItem& it = tab.it[o.b];
  int32_t* __restrict__ counter = it.counter;
  const int t = threadIdx.x;
  if (o.full) {
    const int4* src = reinterpret_cast<const int4*>(counter + o.t0);
#pragma unroll
    for (int q = 0; q < CT / 1024; ++q) reinterpret_cast<int4*>(tile)[t + 256 * q] = src[t + 256 * q];
  } else {
    for (int i = t; i < o.cnt; i += 256) tile[i] = counter[o.t0 + i];
  }
  const int32_t total = tile_ranges(it, o, sb, pre);
  tile_entries(it, o, sb, pre, total, [&](int i) { atomicAdd(&tile[i], 1); });
  __syncthreads();
  if (o.full) {
    int4* dst = reinterpret_cast<int4*>(counter + o.t0);
#pragma unroll
    for (int q = 0; q < CT / 1024; ++q) dst[t + 256 * q] = reinterpret_cast<const int4*>(tile)[t + 256 * q];
  } else {
    for (int i = t; i < o.cnt; i += 256) counter[o.t0 + i] = tile[i];
  }
}

// The sparse form, one block per (counter, tile): the tile's counts start from zero in LDS, one
// byte per counter (a launch adds at most CSEGS = 64 to a counter: every segment is strictly
// ascending), so a 64-byte sector of the counter is one 16-byte row of LDS and a block takes
// 8 KB: twice the dense form's blocks per CU, which matters because a block is a chain of
// dependent round trips (bounds, ring, sector).  After the count only the sectors that hold
// one are read, added to and written: the block owns the tile, so plain loads and stores.  An
// unsorted caller's duplicates may carry between the bytes of one LDS word (counters of this
// tile); nothing is written outside the tile.
__global__ void __launch_bounds__(256, 8) counter_sparse_kernel(const CounterTab tab) {
  __shared__ uint32_t cnt4[CT / 4];  // byte i & 3 of word i >> 2 = the count of tile counter i
  __shared__ int64_t sb[CSEGS];
  __shared__ int32_t pre[CSEGS + 1];
  const TileOf o = tile_of(tab);
  const CounterItem& it = tab.it[o.b];
  int32_t* __restrict__ counter = it.counter;
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < CT / 4096; ++q) reinterpret_cast<int4*>(cnt4)[t + 256 * q] = int4{0, 0, 0, 0};
  const int32_t total = tile_ranges(it, o, sb, pre);
  if (total == 0) return;  // (uniform) no entry in this tile: nothing read or written
  tile_entries(it, o, sb, pre, total,
               [&](int i) { atomicAdd(&cnt4[i >> 2], 1u << (8 * (i & 3))); });
  __syncthreads();
  // the tile's whole sectors of a 16-byte aligned counter: thread t holds the 16-byte quarter
  // t + 256 q of sector (t + 256 q) / 4 (one LDS word); a sector is live when any of its four
  // quarters (adjacent lanes) counted.  All loads of a thread's sectors come before its stores.
  const int vec = (reinterpret_cast<uintptr_t>(counter) & 15u) == 0 ? (o.cnt & ~15) : 0;
  {
    constexpr int Q = CT / 1024;
    int4* g = reinterpret_cast<int4*>(counter + o.t0);
    uint32_t c[Q];
    int4 v[Q];
    bool live[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      c[q] = cnt4[t + 256 * q];
      uint32_t nz = c[q];
      nz |= __shfl_xor(nz, 1, 64);
      nz |= __shfl_xor(nz, 2, 64);
      live[q] = nz != 0 && 4 * (t + 256 * q) < vec;  // (vec % 16 == 0: a sector is in or out)
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (live[q]) v[q] = g[t + 256 * q];
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (live[q])
        g[t + 256 * q] = int4{v[q].x + (int)(c[q] & 255u), v[q].y + (int)((c[q] >> 8) & 255u),
                              v[q].z + (int)((c[q] >> 16) & 255u), v[q].w + (int)(c[q] >> 24)};
  }
  // the rest element-wise: the last partial sector, or the whole tile of an unaligned view
  constexpr int E = 4;
  for (int i0 = vec + t; i0 < o.cnt; i0 += 256 * E) {
    int32_t c[E], v[E];
#pragma unroll
    for (int u = 0; u < E; ++u) {
      const int i = i0 + 256 * u;
      c[u] = i < o.cnt ? (int32_t)((cnt4[i >> 2] >> (8 * (i & 3))) & 255u) : 0;
    }
#pragma unroll
    for (int u = 0; u < E; ++u)
      if (c[u] != 0) v[u] = counter[o.t0 + i0 + 256 * u];
#pragma unroll
    for (int u = 0; u < E; ++u)
      if (c[u] != 0) counter[o.t0 + i0 + 256 * u] = v[u] + c[u];
  }
}

struct Planned {   // one counter of a batch that takes the tiled forms
  const dpz_counter_item* src;
  int form;
  int next;        // first segment not yet flushed
};

// DPZ_COUNTER_AUTO: which counters of a call take the sparse form, the rest the scatter form.
// Measured on independent random rounds at 1 % and 10 % per round, n = 2^24 and 11 M (DESIGN
// §3.1, profiles/counter_flush_forms.jsonl):
//  - the scattered atomics run at their rate (22-27 G/s) however they are launched, while the
//    tiled forms pay two launches that the counters of a call share: alone the sparse form is
//    no slower than the scatter from 0.045 entries per counter, two counters to a call from
//    0.032, eight from 0.015 — AUTO_SCATTER / sqrt(B) fits the three.  B counts the counters
//    that take the sparse form: the largest set whose members all pass its own threshold;
//  - the dense sweep was faster than the sparse form in no call of one counter (0.01 to 6.4
//    entries per counter) and by at most 12 % in a few shared calls around 0.08-0.16, slower
//    in others: AUTO does not take it, DPZ_COUNTER_SWEEP does.
void auto_forms(std::vector<Planned>& plan) {
  size_t B = plan.size() + 1, pass = plan.size();
  while (pass < B) {  // (a counter that fails at B fails at every smaller B)
    B = pass;
    pass = 0;
    for (Planned& p : plan) {
      const double rho = (double)p.src->seg_off[p.src->m] / (double)p.src->n;
      if (p.form == DPZ_COUNTER_SPARSE && rho * std::sqrt((double)B) < AUTO_SCATTER)
        p.form = DPZ_COUNTER_SCATTER;
      pass += p.form == DPZ_COUNTER_SPARSE;
    }
  }
}

int validate(const dpz_counter_item& c) {
  if (c.n < 0 || c.m < 0 || c.n >= (int64_t(1) << 31)) return DPZ_ERR_ARG;
  if (c.m == 0 || c.n == 0) return DPZ_OK;
  if (!c.seg_off || c.seg_off[0] != 0) return DPZ_ERR_ARG;
  for (int r = 0; r < c.m; ++r)
    if (c.seg_off[r + 1] < c.seg_off[r] || c.seg_off[r + 1] - c.seg_off[r] > c.n)
      return DPZ_ERR_ARG;
  if (c.seg_off[c.m] > 0 && (!c.counter || !c.ring)) return DPZ_ERR_ARG;
  return DPZ_OK;
}

int flush_items(const dpz_counter_item* items, int count, int mode, hipStream_t st) {
  if (count < 0 || (count > 0 && !items)) return DPZ_ERR_ARG;
  if (mode < DPZ_COUNTER_AUTO || mode > DPZ_COUNTER_SPARSE) return DPZ_ERR_ARG;
  std::vector<Planned> plan;
  // every argument is checked before the first launch: a refused call has changed no counter
  for (int i = 0; i < count; ++i) {
    const int rc = validate(items[i]);
    if (rc != DPZ_OK) return rc;
  }
  for (int i = 0; i < count; ++i) {
    const dpz_counter_item& c = items[i];
    if (c.m == 0 || c.n == 0 || c.seg_off[c.m] == 0) continue;
    plan.push_back(Planned{&c, mode == DPZ_COUNTER_AUTO ? DPZ_COUNTER_SPARSE : mode, 0});
  }
  if (mode == DPZ_COUNTER_AUTO) auto_forms(plan);
  for (Planned& p : plan) {
    const dpz_counter_item& c = *p.src;
    if (p.form == DPZ_COUNTER_SCATTER)
      p.next = c.m;
    else if (!c.ws || c.ws_bytes < dpz_counter_flush_workspace_bytes(c.n))
      return DPZ_ERR_WORKSPACE;
  }
  for (const Planned& p : plan) {
    if (p.form != DPZ_COUNTER_SCATTER) continue;
    const dpz_counter_item& c = *p.src;
    const int64_t total = c.seg_off[c.m];
    int64_t g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    DPZ_TIMED(DPZ_KT_COUNTER, st,
              counter_scatter_kernel<<<(unsigned)g, 256, 0, st>>>(c.counter, c.n, c.ring, total));
  }
  // the tiled forms: every pass takes each remaining counter's next CSEGS segments, CB counters
  // to a launch (a counter is in a launch once: its tiles have one owner); the counters of the
  // sparse form and those of the dense form take launches of their own
  for (int dense = 0; dense < 2; ++dense) for (;;) {
    CounterTab tab{};
    int64_t blocks = 0, longest = 0;
    int mmax = 0;
    bool more = false;
    auto launch = [&]() -> int {
      int64_t gx = (longest + 255) / 256;
      gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
      DPZ_TIMED(DPZ_KT_COUNTER, st,
                counter_bounds_kernel<<<dim3((unsigned)gx, (unsigned)mmax, (unsigned)tab.cnt), 256,
                                        0, st>>>(tab));
      if (dense)
        DPZ_TIMED(DPZ_KT_COUNTER, st, counter_sweep_kernel<<<(unsigned)blocks, 256, 0, st>>>(tab));
      else
        DPZ_TIMED(DPZ_KT_COUNTER, st, counter_sparse_kernel<<<(unsigned)blocks, 256, 0, st>>>(tab));
      tab.cnt = 0;
      blocks = longest = 0;
      mmax = 0;
      return DPZ_OK;
    };
    for (Planned& p : plan) {
      const dpz_counter_item& c = *p.src;
      if (p.next >= c.m || (p.form == DPZ_COUNTER_SWEEP) != (dense != 0)) continue;
      CounterItem& it = tab.it[tab.cnt];
      const int64_t base = c.seg_off[p.next];
      int r = 0;
      it.off[0] = 0;
      while (r < CSEGS && p.next + r < c.m &&
             c.seg_off[p.next + r + 1] - base < (int64_t(1) << 32)) {
        it.off[r + 1] = (uint32_t)(c.seg_off[p.next + r + 1] - base);
        const int64_t len = c.seg_off[p.next + r + 1] - c.seg_off[p.next + r];
        if (len > longest) longest = len;
        ++r;
      }
      p.next += r;  // (r >= 1: a segment holds at most n < 2^31 entries)
      it.counter = c.counter;
      it.ring = c.ring + base;
      it.bounds = static_cast<int32_t*>(c.ws);
      it.n = c.n;
      it.tiles = (c.n + CT - 1) / CT;
      it.tile0 = blocks;
      it.m = r;
      blocks += it.tiles;
      if (r > mmax) mmax = r;
      ++tab.cnt;
      if (p.next < c.m) more = true;
      if (tab.cnt == CB) {
        const int rc = launch();
        if (rc != DPZ_OK) return rc;
      }
    }
    if (tab.cnt > 0) {
      const int rc = launch();
      if (rc != DPZ_OK) return rc;
    }
    if (!more) break;
  }
  return DPZ_OK;
}

}  // namespace
}  // namespace dpz

using namespace dpz;

extern "C" size_t dpz_counter_flush_workspace_bytes(int64_t n) {
  const int64_t tiles = (n > 0 ? n : 1) / CT + 1;
  return (size_t)CSEGS * (size_t)(tiles + 1) * sizeof(int32_t);
}

extern "C" int dpz_counter_flush(int32_t* counter, int64_t n, const int32_t* ring,
                                 const int64_t* seg_off, int m, int mode, void* ws,
                                 size_t ws_bytes, dpz_stream_t stream) {
  const dpz_counter_item c{counter, n, ring, seg_off, m, ws, ws_bytes};
  return flush_items(&c, 1, mode, static_cast<hipStream_t>(stream));
}

extern "C" int dpz_counter_flush_batch(const dpz_counter_item* items, int count, int mode,
                                       dpz_stream_t stream) {
  return flush_items(items, count, mode, static_cast<hipStream_t>(stream));
}
