// Block-floating fp32 value coding: the float leg of EliasFpzip / EliasFpzipLossy.
//
// Replaces (reference sacs-epfl/decentralizepy, src/decentralizepy/):
//   compression/EliasFpzip.py:19-51       fpzip.compress(arr, precision=0)    (lossless)
//   compression/EliasFpzipLossy.py:14-58  fpzip.compress(arr, precision=p)    (lossy, p = 16)
// fpzip is absent from this image, so the byte format is this build's own (parity with fpzip's
// bytes is unpinned); the contract kept is fpzip's: precision 0 round-trips every fp32 bit
// pattern, precision p keeps the p most significant bits of each value's bit pattern (sign,
// exponent, p - 9 mantissa bits; the rest truncated; from p = 10 on a NaN stays a NaN).
//
// Format (little-endian 32-bit words):
//   header  [0] 'DPFZ' magic  [1] n  [2] precision (32 = lossless)  [3] nblk = ceil(n / 256)
//   table   nblk + 1 words: word offset of each block from the start of the block area; the last
//           entry is the block area's length
//   block   (256 values, the last one n - 256 (nblk - 1)):
//           [0] emin | w << 8 | mb << 16   (exponent base, exponent width 0..8, mantissa bits)
//           sign plane: 1 bit a value, exponent plane: w bits (e - emin), mantissa plane: mb bits,
//           each plane a LSB-first bit stream padded to whole words (value j at bits [j*b, j*b+b)).
// Top-k values of one block share a handful of exponents (w = 3..5), so the lossless stream is
// ~12 % below raw fp32 and the 16-bit lossy stream ~62 % below; the mantissas of trained weights
// are close to random, which is where fpzip's predictive coder ends up as well.
//
// Encode: 3 launches — size (one wave per block: exponent range -> block words), a 1-workgroup
// scan (table + header), pack (one wave per block assembles its planes in LDS, then stores them
// as whole words).  Decode: 1 launch, one wave per block, sync-free (n comes from the host copy
// of the header).
#include "dpz_common.h"
#include "dpz_wire.h"

namespace dpz {

struct FzHdr {
  uint64_t words;   // block-area words
  uint64_t nbytes;  // whole stream
};

__global__ void __launch_bounds__(256) fz_size_kernel(const float* __restrict__ x, int64_t n,
                                                      int64_t nblk, int prec, int mb,
                                                      uint32_t* __restrict__ blk_words) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;
  const int lane = threadIdx.x & 63;
  uint32_t u[4], emin;
  int cnt, w;
  fz_load(x, n, b, prec, lane, u, &cnt, &emin, &w);
  if (lane == 0) blk_words[b] = fz_words(cnt, w, mb);
}

__global__ void __launch_bounds__(1024) fz_scan_kernel(int64_t n, int64_t nblk, int prec,
                                                       const uint32_t* __restrict__ blk_words,
                                                       uint32_t* __restrict__ out32,
                                                       FzHdr* hdr) {
  __shared__ uint64_t wsum[16];
  uint64_t carry = 0;
  uint32_t* table = out32 + 4;
  for (int64_t b0 = 0; b0 < nblk; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const uint64_t v = b < nblk ? blk_words[b] : 0;
    uint64_t tot;
    const uint64_t ex = block_excl_scan64(v, wsum, &tot) + carry;
    if (b < nblk) table[b] = (uint32_t)ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    table[nblk] = (uint32_t)carry;
    out32[0] = FZ_MAGIC;
    out32[1] = (uint32_t)n;
    out32[2] = (uint32_t)prec;
    out32[3] = (uint32_t)nblk;
    hdr->words = carry;
    hdr->nbytes = 4 * (4 + (uint64_t)nblk + 1 + carry);
  }
}

__global__ void __launch_bounds__(256) fz_pack_kernel(const float* __restrict__ x, int64_t n,
                                                      int64_t nblk, int prec, int mb,
                                                      uint32_t* __restrict__ out32) {
  __shared__ uint32_t stage[4][FZ_MAXW + 1];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + wid;
  if (b >= nblk) return;  // whole waves only: no block-wide barrier below
  const uint32_t* table = out32 + 4;
  fz_pack_block(x, n, b, prec, mb, lane, stage[wid], out32 + 4 + nblk + 1 + table[b]);
}

__global__ void __launch_bounds__(256) fz_decode_kernel(const uint32_t* __restrict__ in32,
                                                        int64_t nwords, int64_t n,
                                                        int64_t nblk, int prec, int mb,
                                                        float* __restrict__ out,
                                                        uint32_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;
  const int lane = threadIdx.x & 63;
  const int64_t area = nwords - (4 + nblk + 1);  // words available to the blocks
  const bool hdr = in32[0] == FZ_MAGIC && in32[1] == (uint32_t)n && in32[2] == (uint32_t)prec &&
                   in32[3] == (uint32_t)nblk;
  // malformed stream: record it, write nothing
  if ((!hdr || !fz_decode_block(in32, area, n, nblk, b, mb, lane, out)) && lane == 0)
    atomicOr(status, 1u);
}

static inline size_t fz_al256(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace dpz

using namespace dpz;

extern "C" int64_t dpz_fpz_max_bytes(int64_t n) {
  if (n < 0) return 0;
  const int64_t nblk = (n + FZ_B - 1) / FZ_B;
  return 4 * (4 + nblk + 1 + nblk * (int64_t)FZ_MAXW);
}

extern "C" size_t dpz_fpz_workspace_bytes(int64_t n) {
  const int64_t nblk = n > 0 ? (n + FZ_B - 1) / FZ_B : 1;
  return fz_al256(sizeof(FzHdr)) + fz_al256((size_t)nblk * 4);
}

extern "C" int dpz_fpz_encode(const float* x, int64_t n, int precision, uint8_t* out,
                              int64_t out_cap, int64_t* nbytes_host, void* ws, size_t ws_bytes,
                              dpz_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  int prec = 0;
  const int mb = fz_mbits(precision, &prec);
  if (mb < 0) return DPZ_ERR_UNSUPPORTED;
  if (n < 0 || n > FZ_MAXN || (n > 0 && !x) || !out || !nbytes_host) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(out) & 3u) || out_cap < dpz_fpz_max_bytes(n)) return DPZ_ERR_ARG;
  if (!ws || ws_bytes < dpz_fpz_workspace_bytes(n)) return DPZ_ERR_WORKSPACE;
  const int64_t nblk = (n + FZ_B - 1) / FZ_B;
  char* p = static_cast<char*>(ws);
  FzHdr* hdr = reinterpret_cast<FzHdr*>(p);
  uint32_t* blk_words = reinterpret_cast<uint32_t*>(p + fz_al256(sizeof(FzHdr)));
  uint32_t* out32 = reinterpret_cast<uint32_t*>(out);
  const unsigned grid = (unsigned)((nblk + 3) / 4);
  if (nblk > 0)
    DPZ_TIMED(DPZ_KT_FPZ_SIZE, st, fz_size_kernel<<<grid, 256, 0, st>>>(x, n, nblk, prec, mb, blk_words));
  DPZ_TIMED(DPZ_KT_FPZ_SCAN, st, fz_scan_kernel<<<1, 1024, 0, st>>>(n, nblk, prec, blk_words, out32, hdr));
  if (nblk > 0)
    DPZ_TIMED(DPZ_KT_FPZ_PACK, st, fz_pack_kernel<<<grid, 256, 0, st>>>(x, n, nblk, prec, mb, out32));
  FzHdr h;
  DPZ_HIP_TRY(hipMemcpyAsync(&h, hdr, sizeof(h), hipMemcpyDeviceToHost, st));
  DPZ_HIP_TRY(hipStreamSynchronize(st));
  *nbytes_host = (int64_t)h.nbytes;
  return DPZ_OK;
}

extern "C" int dpz_fpz_decode(const uint8_t* in, int64_t nbytes, int64_t n, int precision,
                              float* out, uint32_t* status, dpz_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  int prec = 0;
  const int mb = fz_mbits(precision, &prec);
  if (mb < 0) return DPZ_ERR_UNSUPPORTED;
  if (!in || n < 0 || n > FZ_MAXN || (n > 0 && !out) || !status) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(in) & 3u) || (nbytes & 3)) return DPZ_ERR_ARG;
  const int64_t nblk = (n + FZ_B - 1) / FZ_B;
  // the block area must at least hold the header, the table and one meta word a block
  if (nbytes < 4 * (4 + nblk + 1 + nblk)) return DPZ_ERR_ARG;
  if (nblk == 0) return DPZ_OK;
  const unsigned grid = (unsigned)((nblk + 3) / 4);
  DPZ_TIMED(DPZ_KT_FPZ_DECODE, st, fz_decode_kernel<<<grid, 256, 0, st>>>(
      reinterpret_cast<const uint32_t*>(in), nbytes / 4, n, nblk, prec, mb, out, status));
  return DPZ_OK;
}
