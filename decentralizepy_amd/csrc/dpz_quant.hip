// Fixed-ratio quantiser of the reference's compression/Quantization.py on the device: a statistics
// pass (max|x|, a non-finite flag and the fp32 sum of |x| in numpy's summation order), a pack pass
// (quantise + bit packing, parameters derived on the device) and the unpack kernel of the decode.
// The stream is the reference's bit for bit (include/dpz_codec.h, "Quantization").
#include "dpz_quant.h"

namespace dpz {

// One block per 8192-element chunk (dpz_quant.h quant_stats_block).
__global__ void __launch_bounds__(Q_THREADS) quant_stats_kernel(const float* __restrict__ x,
                                                                int64_t n, int vec,
                                                                uint32_t* ws) {
  __shared__ StatsLds s;
  float* sums = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + Q_WS_SUMS);
  quant_stats_block(x, n, vec, ws, sums, blockIdx.x, s);
}

__global__ void __launch_bounds__(Q_THREADS) quant_pack_kernel(const float* __restrict__ x,
                                                               int64_t n, int k, int vec,
                                                               const uint32_t* ws,
                                                               uint32_t* __restrict__ out,
                                                               int64_t cap_dwords,
                                                               int32_t* __restrict__ info) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[Q_PACK_LDS];
  const float* sums = reinterpret_cast<const float*>(reinterpret_cast<const char*>(ws) +
                                                     Q_WS_SUMS);
  quant_pack_body(x, n, k, vec, ws, sums, out, cap_dwords, info, blockIdx.x, lds);
}

// value i sits at stream bits [i*w, (i+1)*w), MSB first: out = float(double(u - 2^(w-1) + 1) *
// scale).  Four values per thread, one 16-byte store.
__global__ void __launch_bounds__(Q_THREADS) quant_unpack_kernel(const uint32_t* __restrict__ in,
                                                                 int64_t ndw, int64_t n, int w,
                                                                 double scale, int vec,
                                                                 float* __restrict__ out) {
  const int64_t n4 = (n + 3) >> 2;
  const uint32_t mask = w == 32 ? 0xFFFFFFFFu : ((1u << w) - 1u);
  const uint32_t half = (1u << (w - 1)) - 1u;
  for (int64_t g = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; g < n4;
       g += (int64_t)gridDim.x * Q_THREADS) {
    const int64_t i0 = g << 2;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t i = i0 + c;
      if (i < n) {
        const int64_t t = i * w, d = t >> 5;
        const uint64_t lo = in[d];
        const uint64_t hi = d + 1 < ndw ? in[d + 1] : 0u;
        const uint32_t fld = (uint32_t)(((hi << 32) | lo) >> (t & 31)) & mask;
        const int32_t qv = (int32_t)((__brev(fld) >> (32 - w)) - half);
        v[c] = (float)((double)qv * scale);
      }
    }
    if (vec && i0 + 3 < n) {
      *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (i0 + c < n) out[i0 + c] = v[c];
    }
  }
}

}  // namespace dpz

using namespace dpz;

extern "C" size_t dpz_quant_workspace_bytes(int64_t n) {
  if (n < 1 || n >= Q_NMAX) return 0;
  return Q_WS_SUMS + 4 * (size_t)quant_chunks(n);
}

extern "C" int64_t dpz_quant_block_elems(void) { return Q_SPAN; }

extern "C" int dpz_quant_encode(const float* x, int64_t n, int64_t k, uint8_t* body,
                                int64_t body_cap, int32_t* info, void* ws, size_t ws_bytes,
                                dpz_stream_t stream) {
  if (n < 1 || n >= Q_NMAX || k < 1 || k > ((int64_t)1 << 30)) return DPZ_ERR_ARG;
  if (!x || !body || !info || !ws || body_cap < 4) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(body) & 3u) ||
      (reinterpret_cast<uintptr_t>(ws) & 15u) || (reinterpret_cast<uintptr_t>(info) & 3u))
    return DPZ_ERR_ARG;
  if (ws_bytes < dpz_quant_workspace_bytes(n)) return DPZ_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DPZ_HIP_TRY(hipMemsetAsync(ws, 0, Q_WS_SUMS, st));
  const unsigned nchunks = (unsigned)quant_chunks(n);
  DPZ_TIMED(DPZ_KT_QUANT_STATS, st,
            quant_stats_kernel<<<nchunks, Q_THREADS, 0, st>>>(x, n, aligned16(x) ? 1 : 0,
                                                              static_cast<uint32_t*>(ws)));
  const unsigned nblocks = (unsigned)((n + Q_SPAN - 1) / Q_SPAN);
  DPZ_TIMED(DPZ_KT_QUANT_PACK, st,
            quant_pack_kernel<<<nblocks + 1, Q_THREADS, 0, st>>>(
                x, n, (int)k, aligned16(x) ? 1 : 0, static_cast<const uint32_t*>(ws),
                reinterpret_cast<uint32_t*>(body), body_cap / 4, info));
  return DPZ_OK;
}

extern "C" int dpz_quant_decode(const uint8_t* body, int64_t body_bytes, int64_t n, int w,
                                double scale, float* out, dpz_stream_t stream) {
  if (n < 1 || n >= Q_NMAX || w < 2 || w > 32) return DPZ_ERR_ARG;
  if (body_bytes < 1 || body_bytes * 8 < n * w) return DPZ_ERR_ARG;
  if (!body || !out) return DPZ_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(body) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u))
    return DPZ_ERR_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int64_t grid = (((n + 3) >> 2) + Q_THREADS - 1) / Q_THREADS;
  if (grid > 8192) grid = 8192;
  DPZ_TIMED(DPZ_KT_QUANT_UNPACK, st,
            quant_unpack_kernel<<<(unsigned)grid, Q_THREADS, 0, st>>>(
                reinterpret_cast<const uint32_t*>(body), (body_bytes + 3) / 4, n, w, scale,
                aligned16(out) ? 1 : 0, out));
  return DPZ_OK;
}
