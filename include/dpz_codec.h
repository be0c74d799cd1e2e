/*
 * dpz_codec.h — C ABI of the MI355X-native decentralizepy model-update codec (libdpzcodec.so).
 *
 * Every pointer argument is caller-owned DEVICE memory (e.g. torch.Tensor.data_ptr() of a
 * CUDA/HIP tensor) unless the comment says "host".  `stream` is a hipStream_t (NULL = default
 * stream).  Every entry point returns an int status: 0 = success, a hipError_t value for HIP
 * failures, or one of the DPZ_ERR_* codes below.  No entry point allocates device memory:
 * workspace is sized by the *_workspace_bytes() queries and passed in by the caller.
 * Codec entry points are reentrant; the only mutable global state is the opt-in per-kernel
 * timing facility (dpz_timing_*), a measurement aid.
 *
 * Each function names the reference (sacs-epfl/decentralizepy, src/decentralizepy/...) code it
 * replaces.  The reference itself has no native layer: these replace ATen-CPU / PyWavelets /
 * numpy call sites inside its Sharing and Compression plugins (see INTEGRATION.md for the
 * ctypes binding and DESIGN.md for the kernels behind each call).
 */
#ifndef DPZ_CODEC_H
#define DPZ_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dpz_stream_t; /* hipStream_t */

/* ---- status codes ------------------------------------------------------------------------ */
#define DPZ_OK 0
#define DPZ_ERR_ARG 1001         /* invalid argument (null pointer, negative size, k > n, ...) */
#define DPZ_ERR_WORKSPACE 1002   /* workspace smaller than the matching *_workspace_bytes()   */
#define DPZ_ERR_UNSUPPORTED 1003 /* size/config outside what the kernels implement            */
#define DPZ_ERR_INTERNAL 1004    /* an internal consistency check failed on the device        */

/* ---- key modes for top-k: how the selection key is formed (reference PartialModel.py:305-331)
 *   DPZ_ACC_NONE       change = x - x0              key = |change|
 *   DPZ_ACC_ACCUMULATE acc += change (written back)  key = |acc|           (:321-325)
 *   DPZ_ACC_ADD        key = |change + acc|, acc unchanged before the rewind (:326-329)
 * With x0 == NULL, change = x (x is already a change vector, e.g. W(x - x0) for JWINS).      */
#define DPZ_ACC_NONE 0
#define DPZ_ACC_ACCUMULATE 1
#define DPZ_ACC_ADD 2

/* ---- top-k flags ---- */
#define DPZ_TOPK_EXACT 0x1 /* force the exact multi-pass radix path (skip the sampled path)  */
#define DPZ_TOPK_ASYNC 0x2 /* enqueue only; the caller must call dpz_topk_complete() later   */
/* Split enqueue (implies DPZ_TOPK_ASYNC), for callers that overlap independent work with the
 * latency-bound part of the encode: STREAM enqueues the pass that reads the inputs (sample +
 * filter); a second call with TAIL and the SAME arguments, on the same stream or one ordered
 * after it, enqueues the selection tail (select, resolve, compact).  On the exact path STREAM
 * enqueues everything and TAIL nothing.                                                       */
#define DPZ_TOPK_STREAM 0x4
#define DPZ_TOPK_TAIL 0x8
/* Several codecs share the GPU (concurrent streams): up to ~2^24 elements the sampled path's
 * filter uses a smaller grid that leaves CU slots to the other streams' kernels; a lone codec
 * (the default) takes the larger, faster-alone grid.  Results are identical either way; STREAM
 * and TAIL calls of one encode must pass the same choice.                                     */
#define DPZ_TOPK_SHARED 0x10
/* val_out receives fp16 values (uint16 words, round to nearest even: torch.Tensor.half(), the
 * C5 payload's value packing) written by the encode itself — no separate packing
 * launch.  val_out then holds k * 2 bytes.  A later dpz_topk_complete re-runs a missed sampled
 * call in the same format.                                                                    */
#define DPZ_TOPK_VAL_FP16 0x20
/* Prior-round key window: the sampled path takes the filter's key window from the exact
 * threshold of the previous sampled call on this workspace — same n, k, DPZ_TOPK_SHARED choice,
 * acc_mode and x0 presence, completed without a miss — as [0.9375 T, 1.0625 T], and skips its
 * sample launch (a node's consecutive rounds: the k-th largest |change| drifts slowly).  The
 * window is validated like a sampled one; when it does not bracket the k-th key (or no such
 * previous call exists) the call misses: a blocking call / dpz_topk_complete then re-runs the
 * SAMPLED path (sample launch included) and only if that misses too the exact path; an
 * asynchronous caller sees the miss in the status word.  Ignored with DPZ_ACC_ACCUMULATE and on
 * the paths without the pipelined filter (unaligned operands).  Results are identical.       */
#define DPZ_TOPK_HINT 0x40
/* x is streamed with the default cache policy instead of non-temporal loads: for a caller that
 * reads x again right after the encode (a node's Metro-Hastings fold over its own model,
 * sharing/Sharing.py:156-190 after PartialModel.py:188-255), whose re-read may then be served
 * by the 256 MiB Infinity Cache.  Results are identical.                                       */
#define DPZ_TOPK_KEEP_X 0x80
/* dpz_topk_encode_nodes only: every node's shared_parameters_counter in bit-sliced form (as
 * dpz_topk_encode_sliced): the node table's counter word points at its planes
 * (uint32[32 * dpz_mask_words(n)]) and its last word at a selection mask
 * (uint32[dpz_mask_words(n)]); compact writes every mask word and adds the mask to the planes
 * instead of the scattered counter[idx] += 1.  DPZ_ERR_UNSUPPORTED when a node's wave segment is
 * longer than one LDS mask row (n past ~25 M at the shared grid).                           */
#define DPZ_TOPK_SLICED 0x100

/* ---- fold flags ---- */
#define DPZ_FOLD_SELF 0x1         /* add the local term w_self*local after the payloads        */
#define DPZ_FOLD_REPLACE_ONLY 0x2 /* out = local with payload[0] values replaced (no weights)  */
#define DPZ_FOLD_ZERO_BASE 0x4    /* sparse payloads are zero off their indices, not local, and
                                     the fold starts from +0.0 (reference STC.py:181-206, 336-361:
                                     T = zeros; T[idx] = params; total = zeros; total += w*T)  */
#define DPZ_FOLD_ACCUMULATE 0x10  /* out holds the running total on entry: the fold continues
                                     from it instead of starting a new one (Choco.py:433-441:
                                     s += w * T_i; s += (1 - sum w) * q)                      */
#define DPZ_FOLD_ADD_ONLY 0x8     /* n_payloads == 1: out = local + T_0 with T_0 zero-based
                                     (reference STC.py:290-303 process_received)              */
#define DPZ_FOLD_BASE_READY 0x40 /* out already holds this fold's no-hit base over local (written
                                  * by dpz_topk_encode_foldbase with the same w / w_self): only the
                                  * elements the (sparse) payloads hit are rewritten.  Only with
                                  * DPZ_FOLD_SELF, 1 <= n_payloads <= 16, no dense payload.      */
#define DPZ_FOLD_ALSO_LOCAL 0x20  /* the result is ALSO written over local, in place (the
                                     reference's load_state_dict of the averaged model while
                                     _post_step makes it init_model, Sharing.py:186-190,
                                     PartialModel.py:333-353): saves a model copy per round.
                                     Not with REPLACE_ONLY / ADD_ONLY.                       */

int dpz_abi_version(void);
/* First 16 hex digits of the SHA-256 of the sources the library was built from (csrc/ *.cpp, *.h,
 * *.hip in name order, then csrc/Makefile, then this header): the Python binding compares it
 * with the checked-out tree and refuses a stale binary.                                        */
const char* dpz_build_id(void);
const char* dpz_error_string(int code);

/* Top-k magnitude encode.
 * Replaces reference sharing/PartialModel.py:164-255 (extract_top_gradients: abs + torch.topk +
 * torch.sort; serialized_model: shared_parameters_counter[idx] += 1, rewind_accumulation(idx)
 * (models/Model.py:53-64), values pre_share_model[idx]) and sharing/JWINS/Wavelet.py:142-197
 * (apply_wavelet + the same bookkeeping on wavelet coefficients).
 * Selects the k largest keys (see DPZ_ACC_*), ties at the k-th key broken by lowest index,
 * and writes them in ascending index order:  idx_out[j] (int32), val_out[j] = vals_src[idx_out[j]].
 * Side effects: counter[idx] += 1 if counter != NULL; acc[idx] = 0 if acc != NULL and
 * acc_mode != DPZ_ACC_NONE; acc += change everywhere first when acc_mode == DPZ_ACC_ACCUMULATE.
 * n < 2^31, 0 <= k <= n.  Without DPZ_TOPK_ASYNC the call blocks until the result is final.
 * ws: device scratch of at least dpz_topk_workspace_bytes(n, k) bytes, ZERO-FILLED before its
 * first use (hipMemset once); the library keeps the small region it relies on zeroed after.   */
size_t dpz_topk_workspace_bytes(int64_t n, int64_t k);
int dpz_topk_encode(const float* x, const float* x0, float* acc, int acc_mode,
                    const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                    float* val_out, int32_t* counter, void* ws, size_t ws_bytes, int flags,
                    dpz_stream_t stream);
/* dpz_topk_encode (same arguments, flags and result) that ALSO writes the no-hit base of the
 * node's coming Metro-Hastings average over x (reference sharing/Sharing.py:156-190 with the
 * local model x, the fold of PartialModel payloads deserialized over it, PartialModel.py:257-303):
 *   base_out[j] = fl(...fl(fl(x[j]*w[0]) + fl(x[j]*w[1])) ... + fl(x[j]*w_self))
 * i.e. what dpz_decode_average(x, ..., w, w_self, DPZ_FOLD_SELF) computes at an element no
 * payload hits.  On the sampled path with 16-byte aligned operands and DPZ_ACC_NONE the filter
 * writes it as it streams x (4n bytes written, no extra read); otherwise a separate pass writes it.
 * A later dpz_decode_average(local = x, the payloads, the SAME w / w_self, DPZ_FOLD_SELF |
 * DPZ_FOLD_BASE_READY, out = base_out) then rewrites only the elements its payloads hit — the
 * decode's 8n bytes of streaming become a gather per hit element.  1 <= n_weights <= 16;
 * base_out (n floats) may not overlap any buffer of the encode (DPZ_ERR_ARG); no STREAM / TAIL
 * split.                                                                                       */
int dpz_topk_encode_foldbase(const float* x, const float* x0, float* acc, int acc_mode,
                             const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                             float* val_out, int32_t* counter, void* ws, size_t ws_bytes,
                             int flags, int n_weights, const float* w, float w_self,
                             float* base_out, dpz_stream_t stream);

/* Top-k encode (exactly dpz_topk_encode with the same arguments) TOGETHER WITH one independent
 * replace decode (exactly dpz_decode_average(r_local, r_n, 1, &r_idx, &r_val, &r_k, NULL, 0,
 * DPZ_FOLD_REPLACE_ONLY, r_out, r_ws, r_ws_bytes) — reference sharing/PartialModel.py:257-303,
 * `T[idx] = params` on a neighbour's payload).  A node's round does both (encode its own model,
 * decode a received payload); on the sampled path the decode's chunks run in blocks appended to
 * the encoder's four latency-bound selection launches, so its HBM streaming fills the CUs those
 * leave idle (a cross-stream event wait costs ~15 us on ROCm 7.2, measured, so a second stream
 * does not pay).  Otherwise the decode is enqueued first on `stream`, then the encode.
 * r_out may not overlap r_local or any buffer of the encode (DPZ_ERR_ARG).  The decode is
 * complete when the encode's stream work is (DPZ_TOPK_ASYNC applies to both); the STREAM / TAIL
 * phase flags are not accepted.  r_ws: the decode workspace (only used when not carried).
 * Decoding over the tensor being encoded (r_local == x, r_n == n, acc_mode DPZ_ACC_NONE: the
 * reference decodes a neighbour's payload over the node's own model, the one it just encoded)
 * is FUSED: the encoder's streaming filter writes r_out = x while it reads x, and only the r_k
 * entries are scattered afterwards, in blocks of the compact launch (4n fewer bytes read). */
int dpz_topk_encode_replace(const float* x, const float* x0, float* acc, int acc_mode,
                            const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                            float* val_out, int32_t* counter, void* ws, size_t ws_bytes, int flags,
                            const float* r_local, const int32_t* r_idx, const float* r_val,
                            int64_t r_k, int64_t r_n, float* r_out, void* r_ws, size_t r_ws_bytes,
                            dpz_stream_t stream);
/* Threshold selection keeping every tie (reference sharing/Choco.py:117-161:
 * cutoff = kthvalue(-|x|, k); x[|x| < -cutoff] = 0; then nonzero()): T = the k-th largest key
 * |x| (T = 0 when k == 0), selects every i with key(x[i]) >= T and x[i] != 0, in ascending
 * index order: idx_out[j], val_out[j] = x[idx_out[j]], at most cap entries.  Blocks; *count
 * (host) = the number selected; returns DPZ_ERR_ARG (with *count set) if it exceeds cap.
 * The selected threshold key stays readable on the device for dpz_mask_below_threshold.       */
int dpz_topk_threshold(const float* x, int64_t n, int64_t k, int32_t* idx_out, float* val_out,
                       int64_t cap, void* ws, size_t ws_bytes, int64_t* count,
                       dpz_stream_t stream);
/* out[i] = key(x[i]) < T ? +0.0f : x[i], T = the threshold key of the last dpz_topk_threshold on
 * this workspace (Choco's in-place sparsification of q, Choco.py:117-140).  out may alias x.   */
int dpz_mask_below_threshold(const float* x, int64_t n, const void* ws, float* out,
                             dpz_stream_t stream);
/* Elementwise fp32 helpers of the Choco update (reference Choco.py:353-447), one rounding per op:
 *   DPZ_EW_SUB   out = a - b
 *   DPZ_EW_ADD   out = a + b
 *   DPZ_EW_CHOCO out = a + c * (b - d)      (x + gamma * (s - x_hat))
 *   DPZ_EW_MHCOMBINE out = a * (c - b) + d  (the reduce-scatter gossip round's owner combine:
 *                x * (weight total - hit weights) + weighted hit values, decentralizepy_amd/gossip.py)
 * out may alias a.  c is rounded to fp32 like a torch scalar multiply.                        */
#define DPZ_EW_SUB 1
#define DPZ_EW_ADD 2
#define DPZ_EW_CHOCO 3
#define DPZ_EW_MHCOMBINE 4
int dpz_elementwise(int op, const float* a, const float* b, const float* d, float c, int64_t n,
                    float* out, dpz_stream_t stream);
/* Helpers of the sharded top-k (one tensor split over ranks, decentralizepy_amd/shard.py,
 * SURVEY §8e): out[j] = x[idx[j]] - x0[idx[j]] (x0 may be NULL); out[j] = src[pos[j]] for 32-bit
 * words (dpz_gather_u16: 16-bit words, the fp16 values of a C5 payload); dst[idx[j] - offset] +=
 * value where idx[j] - offset lies in [0, n).                                                   */
int dpz_gather_change(const float* x, const float* x0, int64_t n, const int32_t* idx, int64_t k,
                      float* out, dpz_stream_t stream);
int dpz_gather_u32(const void* src, int64_t m, const int32_t* pos, int64_t k, void* out,
                   dpz_stream_t stream);
int dpz_gather_u16(const void* src, int64_t m, const int32_t* pos, int64_t k, void* out,
                   dpz_stream_t stream);
int dpz_scatter_add_i32(int32_t* dst, int64_t n, const int32_t* idx, int64_t k, int64_t offset,
                        int32_t value, dpz_stream_t stream);
/* Completes a DPZ_TOPK_ASYNC encode issued with the SAME arguments: synchronises `stream`,
 * and if the sampled path reported a miss, re-runs the selection exactly (blocking).
 * *used_fallback (host, may be NULL) is set to 1 when that happened.                         */
int dpz_topk_complete(const float* x, const float* x0, float* acc, int acc_mode,
                      const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                      float* val_out, int32_t* counter, void* ws, size_t ws_bytes,
                      int* used_fallback, dpz_stream_t stream);

/* dpz_topk_encode with DPZ_TOPK_ASYNC (same arguments, any acc_mode) that also writes the call's
 * final status word to status_out (DEVICE int32, on `stream`, as the encode's last write): 0 =
 * the result is final; otherwise the sampled path missed, nothing was written or updated, and the
 * caller re-runs the encode with DPZ_TOPK_EXACT.  Lets a caller enqueue many encodes that share
 * one workspace (a gossip round's nodes, decentralizepy_amd/gossip_jwins.py) and read every
 * status once; replaces the same reference lines as dpz_topk_encode.  flags: DPZ_TOPK_SHARED
 * and / or DPZ_TOPK_VAL_FP16 (any other bit is DPZ_ERR_ARG).                                   */
int dpz_topk_encode_status(const float* x, const float* x0, float* acc, int acc_mode,
                           const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                           float* val_out, int32_t* counter, void* ws, size_t ws_bytes,
                           int32_t* status_out, int flags, dpz_stream_t stream);

/* ---- the encode's side effects in coalesced form (JWINS / Wavelet with accumulation) ----------
 * Selection mask: ceil(n/32) uint32 words (dpz_mask_words), bit b of word w <-> element 32w + b.
 * Sliced counter: the share counter (reference shared_parameters_counter, int32 per element,
 * sharing/PartialModel.py:143-145) as 32 bit planes of ceil(n/32) words, 4 * 32 * ceil(n/32)
 * bytes: bit b of planes[p * ceil(n/32) + w] is bit p of counter[32w + b].
 * dpz_topk_encode_sliced: the selection of dpz_topk_encode (same keys, ties, idx_out / val_out;
 * acc_mode DPZ_ACC_NONE or DPZ_ACC_ADD, acc only read) with its bookkeeping
 * (sharing/JWINS/Wavelet.py:194-197: shared_parameters_counter[idx] += 1,
 * rewind_accumulation(idx)) as: planes (may be NULL) += 1 at every selected index, and every word
 * of sel_mask written with the selected bits.  The rewind acc[idx] = 0 is NOT applied: the caller
 * folds it into the next pass that rewrites acc — dpz_dwt_sym2_rewind / dpz_dwt_haar_rewind
 * (the accumulating post-step, sharing/PartialModel.py:346-349: acc = (bit ? 0 : acc) + T(x - x0),
 * the reference's rewind-then-add) or dpz_rewind_apply.  Scattered 4-byte counter / accumulator
 * updates over 10 % of a 25 M array touch ~97 % of their 128-byte lines; this form writes
 * n/8 mask bytes and the few planes a carry reaches.  status_out (DEVICE int32, may be NULL):
 * non-NULL = asynchronous, the final status written on `stream` (nonzero: the sampled path
 * missed, nothing was written; re-run with DPZ_TOPK_EXACT); NULL = blocking, a miss re-run
 * exactly inside the call (a DPZ_TOPK_HINT call that missed first runs the sampled path once
 * more).  flags: DPZ_TOPK_EXACT, DPZ_TOPK_SHARED, DPZ_TOPK_VAL_FP16, DPZ_TOPK_HINT (the key
 * window from the previous sampled encode's exact threshold on ws, as dpz_topk_encode).
 * dpz_counter_unslice / dpz_counter_slice convert between the sliced and the int32 counter
 * (DeviceCounter materialises on read); dpz_rewind_apply: acc[i] = 0 where the bit is set.      */
int64_t dpz_mask_words(int64_t n);
int dpz_topk_encode_sliced(const float* x, const float* x0, const float* acc, int acc_mode,
                           const float* vals_src, int64_t n, int64_t k, int32_t* idx_out,
                           float* val_out, uint32_t* planes, uint32_t* sel_mask, void* ws,
                           size_t ws_bytes, int32_t* status_out, int flags, dpz_stream_t stream);
int dpz_counter_unslice(const uint32_t* planes, int64_t n, int32_t* counter, dpz_stream_t stream);
int dpz_counter_slice(const int32_t* counter, int64_t n, uint32_t* planes, dpz_stream_t stream);
int dpz_rewind_apply(float* acc, const uint32_t* sel_mask, int64_t n, dpz_stream_t stream);

/* ---- the int32 share counter applied on read (ring of sent payload indices) -----------------
 * Replaces the per-round `shared_parameters_counter[indices] += 1` of reference
 * sharing/PartialModel.py:205-207 / sharing/JWINS/Wavelet.py:194-195, whose only reader is the
 * end-of-run dump (node/DPSGDNode.py:186-194): the plugin keeps every round's payload indices (the
 * encode's idx_out, strictly ascending int32 in [0, n)) in one device ring and, before any read
 * of the counter or when the ring is full, applies them all:
 *   counter[ring[j]] += 1 for every j < seg_off[m], segment r = ring[seg_off[r], seg_off[r + 1])
 * seg_off: HOST int64[m + 1], seg_off[0] = 0, ascending; each segment strictly ascending indices
 * in [0, n) (an index outside is skipped).  mode DPZ_COUNTER_SCATTER: one atomic per entry;
 * DPZ_COUNTER_SWEEP: every tile of the counter read, incremented in LDS and written once (8n
 * coalesced bytes + 8 per entry, per 64 segments); DPZ_COUNTER_SPARSE: the sweep's tiles, but
 * only the 64-byte sectors of the counter that an entry touches are read, added to and written
 * (a sector without an entry is neither read nor written; no global atomic).  ws: device scratch
 * of dpz_counter_flush_workspace_bytes(n) bytes, used by the sweep and the sparse form.
 * DPZ_COUNTER_AUTO takes the scatter form for few entries per counter and the sparse form
 * otherwise (the more counters a call flushes, the sooner: they share the launches); the dense
 * sweep measured no faster than the sparse form and is taken only on request.  The sparse form
 * counts a launch's additions to a counter in a byte: segments must be strictly ascending.
 * dpz_counter_flush_batch: the same for `count` counters (HOST table; distinct counters, each
 * with its own ws) on one stream: the tiles of all counters that take the same tiled form run
 * in one bounds launch and one tile launch per 8 counters and 64 segments; a counter that
 * takes the scatter form keeps its own launch.  Every item is validated before the first
 * launch.                                                                                       */
#define DPZ_COUNTER_AUTO 0
#define DPZ_COUNTER_SCATTER 1
#define DPZ_COUNTER_SWEEP 2
#define DPZ_COUNTER_SPARSE 3
typedef struct dpz_counter_item {
  int32_t* counter;
  int64_t n;
  const int32_t* ring;
  const int64_t* seg_off; /* HOST int64[m + 1] */
  int m;
  void* ws;
  size_t ws_bytes;
} dpz_counter_item;
size_t dpz_counter_flush_workspace_bytes(int64_t n);
int dpz_counter_flush(int32_t* counter, int64_t n, const int32_t* ring, const int64_t* seg_off,
                      int m, int mode, void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_counter_flush_batch(const dpz_counter_item* items, int count, int mode,
                            dpz_stream_t stream);

/* Batched decode + Metro-Hastings fold over n_payloads neighbour payloads.
 * Replaces reference sharing/PartialModel.py:257-303 (T = cat(local); T[idx] = params),
 * sharing/Sharing.py:156-229 (_averaging / _averaging_server fold) and
 * sharing/JWINS/Wavelet.py:269-309, 336-366 (the same fold on wavelet coefficients).
 *   out[j] = fl( ... fl(fl(t_0[j]*w[0]) + fl(t_1[j]*w[1])) ... + fl(local[j]*w_self) )
 *   t_i[j] = vals[i][m] if idx[i][m] == j for some m, else local[j].
 * Payload i is DENSE (a full model: t_i = vals[i]) iff idx[i] == NULL and k[i] == n; otherwise
 * idx[i] holds k[i] strictly ascending indices (idx[i] may be NULL when k[i] == 0).
 * The local term is present only with DPZ_FOLD_SELF.  idx/vals/k/w are HOST arrays of length
 * n_payloads holding DEVICE pointers / sizes / fp32 weights.  out may not alias local.
 * DPZ_FOLD_REPLACE_ONLY: n_payloads == 1, out = t_0 (no multiply).
 * DPZ_FOLD_ZERO_BASE: t_i[j] = 0 where payload i has no entry (instead of local[j]) and the
 *   first term is fl(+0.0 + fl(t_0[j]*w[0])).  DPZ_FOLD_ADD_ONLY: n_payloads == 1,
 *   out[j] = fl(local[j] + T_0[j]) with T_0 zero-based (no weights).
 * ws: device scratch of at least dpz_decode_workspace_bytes(n, n_payloads) bytes.              */
size_t dpz_decode_workspace_bytes(int64_t n, int n_payloads);
int dpz_decode_average(const float* local, int64_t n, int n_payloads, const int32_t* const* idx,
                       const float* const* vals, const int64_t* k, const float* w, float w_self,
                       int flags, float* out, void* ws, size_t ws_bytes, dpz_stream_t stream);

/* Diagnostic: the kernel dpz_decode_average selects for ONE group of n_payloads <= 16 payloads,
 * computed on the host with no device call (a CPU test pins the selection thresholds).  k / w:
 * the group's sizes and weights (w may be NULL), dense[i] != 0: payload i is dense (NULL: none);
 * flags: the call's DPZ_FOLD_* flags; fresh: the group starts the total (the first group of a
 * call without DPZ_FOLD_ACCUMULATE); aligned: local, out and every dense payload are 16-byte
 * aligned.  plan_out[DPZ_FOLD_PLAN_INTS] = { engine, vec (float4 kernels), epl (walk: elements
 * per lane), dist (walk groups: 1 / 3 groups ahead), win (walk groups: 64 / 128-entry windows),
 * ept (merge: elements per thread), eqw (merge: equal weights), offsets (the tile-offsets
 * pre-pass runs first), chains (classic: the hit-chain path may run) }.                        */
#define DPZ_FOLD_ENGINE_NONE 0        /* nothing to launch                                      */
#define DPZ_FOLD_ENGINE_CLASSIC 1
#define DPZ_FOLD_ENGINE_GROUP 2       /* the 4-slot group kernel                                */
#define DPZ_FOLD_ENGINE_WALK 4        /* 1..4 payloads                                          */
#define DPZ_FOLD_ENGINE_WALK_GROUPS 5 /* 5..16 payloads                                         */
#define DPZ_FOLD_ENGINE_MERGE 8
#define DPZ_FOLD_ENGINE_REPLACE 9     /* one sparse payload replaced / added                    */
#define DPZ_FOLD_ENGINE_PATCH1 10     /* DPZ_FOLD_BASE_READY, one payload                       */
#define DPZ_FOLD_ENGINE_PATCH 11      /* DPZ_FOLD_BASE_READY, 2..16 payloads                    */
#define DPZ_FOLD_PLAN_INTS 9
int dpz_debug_fold_plan(int64_t n, int n_payloads, const int64_t* k, const int* dense,
                        const float* w, int flags, int fresh, int aligned, int* plan_out);

/* Diagnostic: how dpz_decode_average_batch / dpz_decode_average_batch_guarded fold a batch of m
 * nodes, computed on the host with no device call by the function the library itself launches
 * by.  n_payloads[m]; k / dense: the nodes' payloads flattened in node order (dense[i] != 0:
 * payload i is dense, NULL: none); aligned: every local, out and dense row is 16-byte aligned
 * (and out[j] != local[j]).  plan_out[DPZ_FOLD_BATCH_PLAN_INTS] = { path (0: node after node,
 * 1: the <= 4 sparse payloads kernel, 2: the any-degree kernel), launches (kernel launches of
 * the call), nodes of the first launch, passes (ceil(largest payload count / 16)) }.          */
#define DPZ_FOLD_BATCH_PLAN_INTS 4
int dpz_debug_fold_batch_plan(int m, int64_t n, const int* n_payloads, const int64_t* k,
                              const int* dense, int flags, int aligned, int* plan_out);

/* Replace decode of a GLOBAL payload into one rank's slice of a model sharded over ranks
 * (SURVEY §8e "one tensor, decode: no collective"; reference sharing/PartialModel.py:292-295
 * `T[idx] = params` restricted to the slice): local / out hold global elements
 * [offset, offset + n); out[i] = local[i], then out[idx[j] - offset] = vals[j] for every entry
 * inside the slice (entries outside are skipped).  idx: k strictly ascending global indices.
 * local and out 16-byte aligned, out may not alias local.                                      */
int dpz_replace_slice(const float* local, int64_t n, int64_t offset, const int32_t* idx,
                      const float* vals, int64_t k, float* out, dpz_stream_t stream);

/* Batched enqueue for a simulated gossip round (decentralizepy_amd/gossip.py): m node codecs,
 * node j on streams[j % n_streams] with workspace ws[j % n_streams].
 * dpz_topk_encode_batch == for each j: dpz_topk_encode(x[j], x0[j], NULL, DPZ_ACC_NONE, x[j], n,
 *   k, idx_out[j], val_out[j], counter[j], ws[q], ws_bytes, DPZ_TOPK_ASYNC, streams[q]), then the
 *   node's sampled-path status word is copied to status[j] (DEVICE int32[m], may be NULL) on the
 *   same stream (0 = final; otherwise re-run that node with DPZ_TOPK_EXACT).
 * dpz_decode_average_batch == for each j: dpz_decode_average(local[j], n, n_payloads[j],
 *   idx + o_j, vals + o_j, k + o_j, w + o_j, w_self[j], flags, out[j], ws[q], ws_bytes,
 *   streams[q]) with o_j = sum of n_payloads[< j] (all arrays HOST, holding device pointers).
 * Replaces the per-node loops of reference node processes (sharing/PartialModel.py:188-255,
 * sharing/Sharing.py:156-190) run side by side.                                               */
int dpz_topk_encode_batch(int m, const float* const* x, const float* const* x0, int64_t n,
                          int64_t k, int32_t* const* counter, int32_t* const* idx_out,
                          float* const* val_out, void* const* ws, size_t ws_bytes, int n_streams,
                          const dpz_stream_t* streams, int32_t* status);
/* dpz_topk_encode_batch with batch flags: DPZ_BATCH_HINT / DPZ_BATCH_HINT_ALL (the encodes'
 * prior window, as in dpz_encode_replace_batch; a miss shows in status[j] like any other).    */
int dpz_topk_encode_batch_ex(int m, const float* const* x, const float* const* x0, int64_t n,
                             int64_t k, int32_t* const* counter, int32_t* const* idx_out,
                             float* const* val_out, void* const* ws, size_t ws_bytes,
                             int n_streams, const dpz_stream_t* streams, int32_t* status,
                             int flags);
/* The encodes of m nodes of one size (n, k) — each exactly dpz_topk_encode(x, x0, NULL,
 * DPZ_ACC_NONE, x, n, k, idx_out, val_out, counter, ws, ws_bytes, DPZ_TOPK_ASYNC) with its
 * final status word also written to status_out (as dpz_topk_encode_status) — with ONE launch per
 * phase of the sampled path for all of them (sample, filter, select, compact over a grid of m x
 * the per-node grid), so the nodes' latency-bound selection tails overlap each other.
 * node_table: DEVICE array of m entries of 8 64-bit words {x, x0, counter (or 0), idx_out,
 * val_out, ws, status_out, 0}; every node its own workspace of ws_bytes >= dpz_topk_workspace_
 * bytes(n, k) bytes (zero-filled before its first use), x / x0 16-byte aligned.  flags:
 * DPZ_TOPK_HINT (every node's window from its workspace's previous encode, no sample launch; a
 * node without a usable prior misses).  Asynchronous: a nonzero status_out[j] means node j
 * wrote nothing and is re-run with DPZ_TOPK_EXACT.  DPZ_ERR_UNSUPPORTED when (n, k) is not on
 * the sampled path (n >= 2^18, 1 <= k <= n / 2).  Replaces the per-node loops of reference node
 * processes (sharing/PartialModel.py:164-255) run side by side.                               */
int dpz_topk_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, size_t ws_bytes,
                          int flags, dpz_stream_t stream);
int dpz_decode_average_batch(int m, const float* const* local, float* const* out, int64_t n,
                             const int* n_payloads, const int32_t* const* idx,
                             const float* const* vals, const int64_t* k, const float* w,
                             const float* w_self, int flags, void* const* ws, size_t ws_bytes,
                             int n_streams, const dpz_stream_t* streams);
/* dpz_decode_average_batch's one-launch fold of a gossip round on ONE stream, guarded by the
 * round's encodes.  The batch qualifies when m >= 2, 1024 <= n < 2^31 - 1024, flags are within
 * DPZ_FOLD_SELF | DPZ_FOLD_ALSO_LOCAL, every row (local, out, a dense payload's values) is
 * 16-byte aligned, out[j] != local[j], every node has at least one payload and every payload is
 * either sparse with 1 <= k <= n or dense (idx NULL, k == n); a dense payload excludes
 * DPZ_FOLD_ALSO_LOCAL (it may be another node's local row).  Nodes of 1..4 sparse payloads
 * only: one launch per 22 nodes.  Otherwise: one launch per table of nodes (a node takes one
 * slot plus one per payload of 146: 22 nodes of 4 payloads, 8 nodes of 16), a node's payloads
 * past the 16th in further launches that continue its total from out (the self term and the
 * DPZ_FOLD_ALSO_LOCAL copy with its last 16).  Each launch first reads guard[0, guard_n) (DEVICE
 * int32, e.g. dpz_topk_encode_nodes' status words) and, if any word is nonzero, writes nothing
 * (out and, with DPZ_FOLD_ALSO_LOCAL, local unchanged), so the caller checks the encodes once
 * after the round instead of between encode and fold, and re-runs the round's folds after
 * re-running a missed encode exactly.  DPZ_ERR_UNSUPPORTED (nothing enqueued) when the batch
 * does not qualify.  dpz_decode_average_batch takes the same launches (unguarded, on
 * streams[0]) for a qualifying batch, and folds any other node after node.  Replaces the
 * reference's encode -> send -> receive -> _averaging order of every node
 * (sharing/PartialModel.py:188-255, sharing/Sharing.py:156-190), run side by side.            */
int dpz_decode_average_batch_guarded(int m, const float* const* local, float* const* out,
                                     int64_t n, const int* n_payloads,
                                     const int32_t* const* idx, const float* const* vals,
                                     const int64_t* k, const float* w, const float* w_self,
                                     int flags, const int32_t* guard, int64_t guard_n,
                                     dpz_stream_t stream);

/* One codec step per node for m nodes of equal size (n, k): with DPZ_BATCH_ENCODE, node j's
 * dpz_topk_encode(x[j], x0[j], NULL, DPZ_ACC_NONE, x[j], n, k, idx_out[j], val_out[j],
 * counter[j], ws[q], ws_bytes, DPZ_TOPK_ASYNC, streams[q]); with DPZ_BATCH_DECODE, then the replace
 * decode dpz_decode_average(r_local[j], n, 1, &r_idx[j], &r_val[j], &r_k, NULL, 0,
 * DPZ_FOLD_REPLACE_ONLY, r_out[j], dws[q], dws_bytes, streams[q]); q = j % n_streams.  Arrays are
 * HOST arrays of device pointers.  A node's round (reference sharing/PartialModel.py:188-303:
 * serialized_model of its own model, deserialized_model of a received payload) with the host
 * loop in native code.  The encodes are asynchronous: a sampled-path miss is recorded in the
 * workspace's sticky status word (dpz_topk_sticky_status), never silently.                     */
#define DPZ_BATCH_ENCODE 0x1
#define DPZ_BATCH_DECODE 0x2
/* with DPZ_BATCH_ENCODE: the encodes pass DPZ_TOPK_HINT — each takes its key window from the
 * previous encode on its stream's workspace (another node of the same round or the node's own
 * previous round: the same change distribution), a miss recorded like any other.  HINT: every
 * encode but the first on each stream (fresh workspaces hold no prior); HINT_ALL: every encode
 * (the workspaces already hold one of this n, k from an earlier call).                        */
#define DPZ_BATCH_HINT 0x4
#define DPZ_BATCH_HINT_ALL 0x8
int dpz_encode_replace_batch(int m, int what, const float* const* x, const float* const* x0,
                             int64_t n, int64_t k, int32_t* const* counter,
                             int32_t* const* idx_out, float* const* val_out,
                             const float* const* r_local, const int32_t* const* r_idx,
                             const float* const* r_val, int64_t r_k, float* const* r_out,
                             void* const* ws, size_t ws_bytes, void* const* dws, size_t dws_bytes,
                             int n_streams, const dpz_stream_t* streams);
/* dpz_encode_replace_batch with the step batch pipelined where it can be.  ws_pipe: 2 * n_streams
 * further top-k workspaces of ws_bytes each (zero-filled before their first use like ws;
 * [2q], [2q + 1] belong to stream q).  Where every step of the call is a fused encode + replace
 * (both operations, r_local[j] == x[j], another node's payload) on the sampled path, the steps
 * of a stream rotate through ws[q], ws_pipe[2q], ws_pipe[2q + 1] (restarting at ws[q] on every
 * call) and a step's selection tail runs inside the next steps' filter launches: one launch per
 * step in steady state, identical results.  Any other call is enqueued as by
 * dpz_encode_replace_batch.  ws_sig: a HOST array of 3 * n_streams words, zero before the first
 * call and kept by the caller across calls ([3q] for ws[q], [3q + 1], [3q + 2] for stream q's
 * ws_pipe): the library records which encode each workspace last held, and with DPZ_BATCH_HINT
 * or DPZ_BATCH_HINT_ALL a step takes the prior window exactly where its workspace holds one of
 * the step's own kind (any other step runs its sample launch).  *pipelined (HOST, may be NULL):
 * the number of steps enqueued through the pipelined schedule (0 or m).                       */
int dpz_encode_replace_batch_ws(int m, int what, const float* const* x, const float* const* x0,
                                int64_t n, int64_t k, int32_t* const* counter,
                                int32_t* const* idx_out, float* const* val_out,
                                const float* const* r_local, const int32_t* const* r_idx,
                                const float* const* r_val, int64_t r_k, float* const* r_out,
                                void* const* ws, size_t ws_bytes, void* const* dws,
                                size_t dws_bytes, int n_streams, const dpz_stream_t* streams,
                                void* const* ws_pipe, uint32_t* ws_sig, int* pipelined);
/* OR of the final status of every sampled-path encode run on this top-k workspace since the
 * last clear (0 = every one was final; nonzero = at least one missed and, if it was ASYNC and
 * not completed by dpz_topk_complete, published unverified output).  Synchronises `stream`;
 * clear != 0 resets the word afterwards.  *out is a HOST pointer.                              */
int dpz_topk_sticky_status(void* ws, size_t ws_bytes, int clear, int32_t* out,
                           dpz_stream_t stream);

/* Multilevel sym2 DWT, mode "symmetric", fp32, pywt-1.1.1-exact summation order.
 * Replaces reference sharing/JWINS/Wavelet.py:12-32 (pywt.wavedec + coeffs_to_array).
 * coeffs layout: [cA_L, cD_L, ..., cD_1], length dpz_wavedec_len(n, level).
 *   coeffs_x    (may be NULL) = W(x)
 *   coeffs_diff (may be NULL) = W(x - x0)   (x0 must be non-NULL), or += W(x - x0) when
 *   accumulate != 0 (PartialModel._post_step acc += T(init - prev), PartialModel.py:346-349).
 * Requires every level input length >= 4.                                                      */
int64_t dpz_wavedec_len(int64_t n, int level);
int dpz_dwt_sym2(const float* x, const float* x0, int64_t n, int level, float* coeffs_x,
                 float* coeffs_diff, int accumulate, dpz_stream_t stream);

/* dpz_dwt_sym2(x, x0, n, level, NULL, acc, 1) with the deferred rewind of
 * dpz_topk_encode_sliced: acc[i] = fl((bit i of sel_mask ? +0.0 : acc[i]) + W(x - x0)[i]). */
int dpz_dwt_sym2_rewind(const float* x, const float* x0, int64_t n, int level, float* acc,
                        const uint32_t* sel_mask, dpz_stream_t stream);

/* Multilevel sym2 IDWT (pywt.array_to_coeffs + pywt.waverec), first n outputs written.
 * Replaces reference sharing/JWINS/Wavelet.py:311-316.                                        */
int dpz_idwt_sym2(const float* coeffs, int64_t n, int level, float* out, dpz_stream_t stream);

/* Tile ranges of the two transforms, for one tensor sharded over ranks (SURVEY §8e "wavelet
 * DWT/IDWT: yes, with a halo"; decentralizepy_amd/shard.py sharded_wavedec / sharded_waverec).
 * The forward tile t owns level-L outputs [t*W, (t+1)*W) (W = dpz_dwt_tile_width()) and the
 * matching 2^(L-l)*W outputs of every detail level; it reads inputs [2^L*W*t - 2(2^L - 1),
 * 2^L*W*(t+1)) of x / x0 (clipped to [0, n)); a last tile that owns a single level-L output of
 * an odd-length level-(L-1) input reads from 2^L*W*t - (3*2^L - 2): all of it lies left of
 * 2^L*W*t (n is smaller), in the slice of the rank that holds the array's tail.  The inverse
 * tile u writes outputs [u*V, (u+1)*V) (V = dpz_idwt_tile_width()).  x, x0, coeffs and out are
 * VIRTUAL bases: element i
 * of the global array is at base + i, and only the elements the tiles [tile_lo, tile_hi) touch
 * are dereferenced (a rank passes its halo'd slice buffer minus its first global index).        */
int64_t dpz_dwt_tile_width(void);
int64_t dpz_idwt_tile_width(void);
int dpz_dwt_sym2_tiles(const float* x, const float* x0, int64_t n, int level, int64_t tile_lo,
                       int64_t tile_hi, float* coeffs_x, float* coeffs_diff, int accumulate,
                       dpz_stream_t stream);
int dpz_idwt_sym2_tiles(const float* coeffs, int64_t n, int level, int64_t tile_lo,
                        int64_t tile_hi, float* out, dpz_stream_t stream);

/* ---- Haar DWT / IDWT (pywt "haar", mode "symmetric": the reference Wavelet's DEFAULT wavelet,
 * sharing/JWINS/Wavelet.py:56).  Same contracts as the sym2 entries above, levels 1..8; level
 * lengths len_l = ceil(len_{l-1} / 2), layout [cA_L, cD_L, ..., cD_1] (pywt.coeffs_to_array).
 * Bit-exact with PyWavelets 1.1.1 (csrc/dpz_haar.hip gives the summation order).              */
int64_t dpz_haar_wavedec_len(int64_t n, int level);
int dpz_dwt_haar(const float* x, const float* x0, int64_t n, int level, float* coeffs_x,
                 float* coeffs_diff, int accumulate, dpz_stream_t stream);
int dpz_idwt_haar(const float* coeffs, int64_t n, int level, float* out, dpz_stream_t stream);
/* the haar counterpart of dpz_dwt_sym2_rewind */
int dpz_dwt_haar_rewind(const float* x, const float* x0, int64_t n, int level, float* acc,
                        const uint32_t* sel_mask, dpz_stream_t stream);

/* ---- Any other pywt discrete wavelet (db1-32, sym2-20, coif1-10, bior / rbio, dmey: even filter
 * length flen <= 64), mode "symmetric", levels 1..8 with every level's input >= flen values.
 * Replaces reference sharing/JWINS/Wavelet.py:12-32 and :311-316 (pywt.wavedec / waverec with
 * the configured `wavelet`) for the wavelets the fused sym2 / haar kernels do not cover.
 * `bank` is DEVICE memory: 4*flen floats dec_lo, dec_hi, rec_lo, rec_hi — the fp32 taps pywt
 * applies to float32 data (decentralizepy_amd/wavelet_filters.json).  Level lengths
 * len_l = floor((len_{l-1} + flen - 1) / 2), layout [cA_L, cD_L, ..., cD_1].  Bit-exact with
 * PyWavelets 1.1.1 (csrc/dpz_wvgen.hip gives the summation order).  dpz_dwt_generic: W(x) into
 * coeffs_x and / or W(x - x0) into coeffs_diff (accumulate: added; sel_mask, with accumulate:
 * the deferred rewind of dpz_topk_encode_sliced, as dpz_dwt_sym2_rewind); ws of
 * dpz_wavelet_generic_workspace_bytes (levels >= 2).  Unsupported lengths: -1 / DPZ_ERR_UNSUPPORTED. */
int64_t dpz_wavedec_len_generic(int64_t n, int level, int flen);
size_t dpz_wavelet_generic_workspace_bytes(int64_t n, int level, int flen);
int dpz_dwt_generic(const float* x, const float* x0, int64_t n, int level, const float* bank,
                    int flen, float* coeffs_x, float* coeffs_diff, int accumulate,
                    const uint32_t* sel_mask, void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_idwt_generic(const float* coeffs, int64_t n, int level, const float* bank, int flen,
                     float* out, void* ws, size_t ws_bytes, dpz_stream_t stream);


/* dst[idx[j]] = value for j < k (indices outside [0, n) are ignored).
 * Replaces reference models/Model.py:53-64 (rewind_accumulation: acc[idx] = 0) where the rewind
 * is not fused into dpz_topk_encode (Wavelet with change_based_selection = False).             */
int dpz_scatter_fill(float* dst, int64_t n, const int32_t* idx, int64_t k, float value,
                     dpz_stream_t stream);

/* fp16 value packing (round-to-nearest-even, torch.half semantics) and unpacking.
 * The build's own wire codec for values (BASELINE config C5); the reference's lossy float path
 * is fpzip (compression/EliasFpzipLossy.py:14-58), which is not byte-compatible.
 * Unpacking equals numpy's half -> float widening on every one of the 65 536 patterns: a NaN
 * keeps its sign and payload (a signalling NaN is not quieted).                                */
int dpz_pack_fp16(const float* in, int64_t n, uint16_t* out, dpz_stream_t stream);
int dpz_unpack_fp16(const uint16_t* in, int64_t n, float* out, dpz_stream_t stream);

/* ---- Per-kernel timing (measurement only; not thread-safe) -----------------------------------
 * While enabled, every kernel launch records a HIP event pair on its own stream (launches into a
 * capturing stream are skipped).  dpz_timing_read waits for the pending pairs and fills the summed
 * milliseconds and launch counts per kernel id; it returns DPZ_KT_COUNT.                     */
enum {
  DPZ_KT_TOPK_SAMPLE = 0, DPZ_KT_TOPK_FILTER, DPZ_KT_TOPK_SELECT, DPZ_KT_TOPK_RESOLVE,
  DPZ_KT_TOPK_COMPACT,
  DPZ_KT_EXACT_HIST, DPZ_KT_EXACT_RESOLVE, DPZ_KT_EXACT_COUNT, DPZ_KT_EXACT_SCAN,
  DPZ_KT_EXACT_WRITE, DPZ_KT_ACCUMULATE,
  DPZ_KT_FOLD_OFFSETS, DPZ_KT_FOLD, DPZ_KT_DWT, DPZ_KT_IDWT, DPZ_KT_ELIAS_COUNT,
  DPZ_KT_ELIAS_SCAN, DPZ_KT_ELIAS_PACK, DPZ_KT_ELIAS_SPEC, DPZ_KT_ELIAS_RESOLVE,
  DPZ_KT_ELIAS_WRITE, DPZ_KT_FP16, DPZ_KT_SCATTER, DPZ_KT_FPZ_SIZE, DPZ_KT_FPZ_SCAN,
  DPZ_KT_FPZ_PACK, DPZ_KT_FPZ_DECODE, DPZ_KT_CPLX, DPZ_KT_FFT_SCALE, DPZ_KT_HAAR, DPZ_KT_LZ4,
  DPZ_KT_COUNTER, DPZ_KT_FFT, DPZ_KT_QUANT_STATS, DPZ_KT_QUANT_PACK, DPZ_KT_QUANT_UNPACK,
  DPZ_KT_COUNT
};
int dpz_timing_enable(int on);  /* also clears the accumulators */
int dpz_timing_read(double* ms_sum, int64_t* count, int max_ids);
const char* dpz_kernel_name(int id);

/* ---- Elias-gamma index coding (byte-identical to the reference wire format) ------------------
 * Replaces compression/Elias.py:20-52 (Elias.compress) and :54-97 (Elias.decompress).
 * Format: l = floor(log2(gap)) zero bits then the gap in l+1 bits, MSB-first, for every gap of the
 * sorted int32 array; 128 zero bits; np.packbits byte order; bytes [-16:-8] = int64 LE first
 * value, [-8:] = int64 LE total bit count (code bits + 128).                                   */

/* Upper bound of the encoded size for k values (all gaps 2^31-1), rounded up to 4 bytes. */
int64_t dpz_elias_max_bytes(int64_t k);
/* Device workspace for an encode of k values or a decode of an nbytes stream (the max of both). */
size_t dpz_elias_workspace_bytes(int64_t k, int64_t nbytes);
/* idx: device int32[k], strictly increasing (k >= 2; the reference raises IndexError below 2).
 * out: device buffer, 4-byte aligned, out_cap >= dpz_elias_max_bytes(k).  Writes the stream and
 * returns its length in *nbytes_host (host pointer; the call synchronises `stream`).
 * DPZ_ERR_ARG if the indices are not strictly increasing.                                      */
int dpz_elias_encode(const int32_t* idx, int64_t k, uint8_t* out, int64_t out_cap,
                     int64_t* nbytes_host, void* ws, size_t ws_bytes, dpz_stream_t stream);
/* in: device copy of the stream, 4-byte aligned, readable up to round_up(nbytes, 4) + 16 bytes.
 * nbits/first: the stream's trailer (the caller holds the bytes).  Writes first + running gap
 * sums into out64 (int64, as the reference returns) and/or out32 (either may be NULL); the value
 * count goes to *count_host (host pointer; synchronises).  DPZ_ERR_ARG on a malformed stream,
 * DPZ_ERR_WORKSPACE if the count exceeds out_cap.
 * Limit: a stream may hold at most 2^26 code bits (nbits <= 2^26 + 128: 1024 super maps of 64
 * chunks of 1024 bits).  Beyond that the call returns DPZ_ERR_UNSUPPORTED before any launch and
 * writes nothing.  dpz_elias_encode has no such limit, so it can write a stream that this
 * decoder refuses.                                                                              */
int dpz_elias_decode(const uint8_t* in, int64_t nbytes, int64_t nbits, int64_t first,
                     int64_t* out64, int32_t* out32, int64_t out_cap, int64_t* count_host,
                     void* ws, size_t ws_bytes, dpz_stream_t stream);
/* dpz_elias_decode without a host synchronisation, for a receiver that knows the value count
 * from the payload's other leg (the float header's n, or the raw values' length): decodes into
 * out64 / out32 (device, `count` entries) and ORs *status (DEVICE uint32) nonzero on `stream`
 * when the stream is malformed or holds a different number of values — the entries are then
 * unspecified (the fold kernels stay in bounds on any index values); the caller reads the status
 * word once after the round's folds.  Same workspace as dpz_elias_decode.  Replaces the same
 * reference lines (compression/Elias.py:54-97), called from PartialModel.py:156-162.          */
int dpz_elias_decode_async(const uint8_t* in, int64_t nbytes, int64_t nbits, int64_t first,
                           int64_t* out64, int32_t* out32, int64_t count, uint32_t* status,
                           void* ws, size_t ws_bytes, dpz_stream_t stream);

/* ---- Block-floating fp32 value coding (the float leg of EliasFpzip / EliasFpzipLossy) --------
 * Replaces compression/EliasFpzip.py:19-51 (fpzip.compress, precision 0) and
 * compression/EliasFpzipLossy.py:14-58 (precision p).  fpzip is absent, so the bytes are this
 * build's own format (csrc/dpz_fpz.hip): precision 0 (or >= 32) is lossless for every bit pattern;
 * 1 <= p < 32 keeps the top p bits of each value's bit pattern (the rest truncated; from p = 10 on
 * a NaN stays a NaN); p < 0 returns DPZ_ERR_UNSUPPORTED.  Stream: 16-byte header ('DPFZ', n, precision, nblk), a table of
 * nblk + 1 block offsets, then per 256 values a meta word and sign / exponent / mantissa planes. */

/* Upper bound of the stream size for n values (every block at full exponent width). */
int64_t dpz_fpz_max_bytes(int64_t n);
/* Device workspace for an encode of n values. */
size_t dpz_fpz_workspace_bytes(int64_t n);
/* x: device fp32[n] (n <= 2^30); out: device buffer, 4-byte aligned, out_cap >=
 * dpz_fpz_max_bytes(n).  Writes the stream, its length to *nbytes_host (host; synchronises).   */
int dpz_fpz_encode(const float* x, int64_t n, int precision, uint8_t* out, int64_t out_cap,
                   int64_t* nbytes_host, void* ws, size_t ws_bytes, dpz_stream_t stream);
/* in: device copy of a stream of nbytes (a multiple of 4, 4-byte aligned); n and precision from
 * its header (the caller holds the bytes).  Writes out[n]; asynchronous.  Every block is checked
 * against the header, the offset table and the buffer bounds: a malformed block is not decoded
 * and sets *status (device uint32, OR-ed) to nonzero; the caller reads it after the stream.   */
int dpz_fpz_decode(const uint8_t* in, int64_t nbytes, int64_t n, int precision, float* out,
                   uint32_t* status, dpz_stream_t stream);

/* ---- FFT sharing plugin: real FFTs and complex coefficients (decentralizepy_amd/sharing/JWINS/FFT.py)
 * Replaces sharing/JWINS/FFT.py:12-25 (torch.fft.rfft), :301 (torch.fft.irfft, 1/n on the
 * inverse), :143-156 (top-k over |complex change|, flat_fft[index]), PartialModel.py:315-329 on
 * the complex change, Model.py:53-64 (complex rewind).  Complex = interleaved fp32 (re, im), the
 * torch.complex64 layout; m = n / 2 + 1 coefficients for n reals.  The transforms are this
 * build's mixed-radix Stockham kernels (csrc/dpz_fft.hip) whenever every prime factor of the
 * complex length (n / 2 for even n, n for odd) is <= 4096; other sizes fall back to hipFFT
 * (rocFFT, plans cached per device / n / direction).  The library's device allocations are the
 * per-size twiddle tables (and rocFFT's, on the fallback); the work area is the caller's.      */
/* Work area for dpz_rfft / dpz_irfft of n reals (the max of both directions); -1 if unsupported
 * (n < 2 or n > 2^31 - 1).  Creates (and caches) the hipFFT plans of a fallback size.            */
int64_t dpz_fft_workspace_bytes(int64_t n);
/* 1 when dpz_rfft / dpz_irfft of n reals run the native kernels, 0 when they fall back to hipFFT. */
int dpz_fft_native(int64_t n);
/* Alignment: the kernels address complex data as 8-byte (re, im) pairs, and for even n the real
 * vector as n / 2 such pairs.  The complex pointer (dpz_rfft's out, dpz_irfft's coeffs) must be
 * 8-byte aligned for every n, the real pointer (x / out) for every even n that runs the native
 * kernels; otherwise DPZ_ERR_ARG is returned before anything is launched.                        */
/* out[m complex] = rfft(x[n]).  Asynchronous on stream.                                          */
int dpz_rfft(const float* x, int64_t n, float* out, void* ws, size_t ws_bytes, dpz_stream_t stream);
/* out[n] = irfft(coeffs[m complex], n) with torch's "backward" normalisation (1/n).  coeffs may be
 * OVERWRITTEN (the hipFFT fallback's C2R works in place on its input; the native passes only
 * read it).                                                                                       */
int dpz_irfft(float* coeffs, int64_t n, float* out, void* ws, size_t ws_bytes, dpz_stream_t stream);
/* key[i] = |c[i]| (fp32 sqrt(re^2 + im^2)) of the complex change after the DPZ_ACC_* step
 * (ACCUMULATE: acc += change, key = |acc|; ADD: key = |change + acc|, acc unchanged).          */
int dpz_cplx_key(const float* change, float* acc, int acc_mode, int64_t m, float* key,
                 dpz_stream_t stream);
/* out[j] = src[idx[j]] (complex); acc[idx[j]] = 0 when acc is not NULL.                          */
int dpz_cplx_gather(const float* src, int64_t m, const int32_t* idx, int64_t k, float* out,
                    float* acc, dpz_stream_t stream);
/* pair[2j] = 2 idx[j], pair[2j+1] = 2 idx[j] + 1 (8-byte aligned pair): a complex payload as a
 * float payload of the interleaved view, for dpz_decode_average.                                  */
int dpz_cplx_pair_indices(const int32_t* idx, int64_t k, int32_t* pair, dpz_stream_t stream);

/* ---- LZ4 frames (the wire format of compression/Lz4Wrapper.py:20-98, lz4.frame) -------------
 * Encoder: linked 2 KB blocks, one wave each, whose matches reach 14 KB back (B.Indep clear,
 * BD = 64 KB, content size stored, no checksums): a valid LZ4 frame any decoder reads; the bytes
 * are this build's (greedy parse over a 12-bit hash of 5 bytes; python-lz4's match finder is not
 * reproduced, so byte parity is unpinned).  Decoder: any LZ4 frame with 64 KB blocks, linked (python-lz4's
 * default, decoded by one workgroup) or independent (one workgroup per block); content and
 * block checksums are skipped, dictionary IDs rejected.                                         */
/* The built codec's geometry, for tests that place inputs at its edges: out5 = {encoder block
 * bytes, encoder history bytes, decoded bytes per block on the parallel decoder, compressed bytes
 * per block on it, its walk chunk in compressed bytes}.  Host only; DPZ_ERR_ARG on a null out5. */
int dpz_lz4_geometry(int32_t* out5);
/* Upper bound of the frame size for n input bytes. */
int64_t dpz_lz4_max_bytes(int64_t n);
/* Device workspace for an encode of n bytes (nblk = bmax = 0) or a decode of a frame of nblk
 * blocks of at most bmax bytes (n = 0); the max of what the calls ask is always enough.       */
size_t dpz_lz4_workspace_bytes(int64_t n, int64_t nblk, int64_t bmax);
/* in: device bytes[n]; out: device, out_cap >= dpz_lz4_max_bytes(n).  The frame length goes to
 * *nbytes_host (host; synchronises).                                                            */
int dpz_lz4_compress(const uint8_t* in, int64_t n, uint8_t* out, int64_t out_cap,
                     int64_t* nbytes_host, void* ws, size_t ws_bytes, dpz_stream_t stream);
/* Frame header and block walk of a HOST copy of a frame: content size (-1 if absent), block
 * count, linked flag, block max.  DPZ_ERR_ARG on a malformed frame (bad magic, version, header
 * checksum, truncated blocks).                                                                  */
int dpz_lz4_frame_info(const uint8_t* frame_host, int64_t nbytes, int64_t* content_size,
                       int64_t* nblk, int* linked, int64_t* block_max);
/* frame_dev / frame_host: the same nbytes of frame on the device and on the host (the host walks
 * the block headers).  Writes the content to out (device) and its length to *n_host (host;
 * synchronises).  DPZ_ERR_ARG on a malformed block or a content-size mismatch,
 * DPZ_ERR_WORKSPACE if the content exceeds out_cap, DPZ_ERR_UNSUPPORTED above 64 KB blocks.   */
int dpz_lz4_decompress(const uint8_t* frame_dev, const uint8_t* frame_host, int64_t nbytes,
                       uint8_t* out, int64_t out_cap, int64_t* n_host, void* ws, size_t ws_bytes,
                       dpz_stream_t stream);
/* out[j] = in[j] - in[j-1] (in[-1] = 0), int32 wrap-around: np.diff(a, prepend=0).astype(int32)
 * (Lz4Wrapper.py:35-37).  in and out must not alias.                                           */
int dpz_delta_i32(const int32_t* in, int64_t k, int32_t* out, dpz_stream_t stream);
/* Inclusive running sum of int32 values as int64 (np.cumsum, Lz4Wrapper.py:58-59) into out64
 * and / or its int32 truncation into out32 (either may be NULL).                                */
size_t dpz_running_sum_workspace_bytes(int64_t k);
int dpz_running_sum_i32(const int32_t* in, int64_t k, int64_t* out64, int32_t* out32, void* ws,
                        size_t ws_bytes, dpz_stream_t stream);

/* ---- SubSampling: the sender's Bernoulli mask rebuilt from its seed (sharing/SubSampling.py) ---
 * The reference's mask is `torch.rand(n, generator=g) <= alpha` after g.manual_seed(s): MT19937
 * (init_genrand(s & 0xffffffff)), one tempered 32-bit output per element, u = (out & 0xFFFFFF) *
 * 2^-24 as fp32, so bit j = (out_j & 0xFFFFFF) <= floor((double)(float)alpha * 2^24).  The
 * kernels reproduce that bit string in parallel by jump-ahead: chunk c of dpz_mt_chunk_elems()
 * elements starts from the state t^(c * chunk) mod phi gives (phi: MT19937's characteristic
 * polynomial; tables of jump polynomials are built on the host on first use and copied once to
 * each device that uses them, the one allocation the library makes besides the FFT twiddles).
 * So a dpz_mt_mask call that needs table rows its device does not have yet BLOCKS: it builds
 * the missing rows on the host (about 0.2 s for all that 2^24 elements need, once per process),
 * allocates on the first call per device and copies the rows with a synchronous hipMemcpy.
 * Such a call must not sit inside a stream capture: run one mask of the largest n first.
 * Above dpz_mt_coarse_chunks() chunks a coarse launch first jumps to every
 * coarse_chunks * chunk_elems boundary.  n < 2^31 elements.
 * dpz_mt_raw_host (host only, no device call): the tempered outputs [start, start + count) of
 * seed's stream into out (HOST), through the same jump tables — a jump to each enclosing chunk,
 * then stepping — so the GF(2) code can be checked without a GPU.
 * dpz_mt_mask: mask (dpz_mask_words(n) words, bit b of word w <-> element 32w + b, trailing bits
 * zero), rank_tab (dpz_mt_rank_entries(n) int32, opaque: exclusive popcounts that turn a mask
 * bit into its position among the selected elements) and *count_dev (DEVICE int64, the number
 * selected).  alpha is the fp32 the sender's Python float rounds to; alpha < 0 or NaN selects
 * nothing, alpha >= 1 everything.  ws: dpz_mt_mask_workspace_bytes(n).
 * dpz_mask_gather: vals[rank(j)] = x[j] for every selected j in index order (`concated[mask]`,
 * SubSampling.py:158) and, with counter != NULL, counter[j] += 1 (:159).
 * dpz_mask_decode_average: the Metro-Hastings fold (sharing/Sharing.py:156-190) over payloads
 * deserialised by SubSampling.deserialized_model (T = local; T[mask_i] = vals_i), in the
 * reference's fp32 order: t = w_0 v_0, t = t + w_i v_i, out = t + w_self local with
 * v_i = bit_i ? vals_i[rank_i(j)] : local[j].  mask / rank_tab / vals / w: HOST arrays of
 * n_payloads entries (1 .. 16, more is DPZ_ERR_UNSUPPORTED; device pointers inside).  flags:
 * DPZ_FOLD_SELF (without it the server form, Sharing.py:200-229: no self term) and
 * DPZ_FOLD_ACCUMULATE (out holds the running total t of earlier payloads on entry and the fold
 * continues from it: more than 16 payloads are folded 16 at a time, the self term in the last
 * call, with the same roundings as one pass); any other bit is DPZ_ERR_ARG.  vals_i must hold
 * the mask's count of values: the caller checks that before the call.  out may not overlap
 * local.
 * The three device entry points return DPZ_ERR_ARG before any device call for n < 1, null
 * pointers or n_payloads < 1.                                                                  */
int64_t dpz_mt_chunk_elems(void);
int64_t dpz_mt_coarse_chunks(void);
int dpz_mt_raw_host(uint32_t seed, int64_t start, int64_t count, uint32_t* out);
int64_t dpz_mt_rank_entries(int64_t n);
size_t dpz_mt_mask_workspace_bytes(int64_t n);
int dpz_mt_mask(uint32_t seed, float alpha, int64_t n, uint32_t* mask, int32_t* rank_tab,
                int64_t* count_dev, void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_mask_gather(const float* x, int64_t n, const uint32_t* mask, const int32_t* rank_tab,
                    float* vals, int32_t* counter, dpz_stream_t stream);
int dpz_mask_decode_average(const float* local, int64_t n, int n_payloads,
                            const uint32_t* const* mask, const int32_t* const* rank_tab,
                            const float* const* vals, const float* w, float w_self, int flags,
                            float* out, dpz_stream_t stream);

/* ---- SubSampling, a round's nodes at once (decentralizepy_amd/gossip_subsampling.py) -----------
 * The three calls above for m nodes with one launch per phase, the node in the grid's second
 * dimension: the masks of different nodes are independent and share the jump tables, and one
 * mask alone leaves most of the machine idle (n / 65536 blocks).  All three validate before any
 * device call: DPZ_ERR_ARG for m < 1, n < 1, null pointers or bad strides, DPZ_ERR_UNSUPPORTED
 * for n >= 2^31, DPZ_ERR_WORKSPACE for a short workspace.
 * dpz_mt_mask_batch: m masks of one length n; mask i from seeds[i] / alphas[i] (HOST arrays,
 * handed to the kernels by value, 64 masks per launch group; no copy, no synchronisation).  Row i
 * of mask (mask_stride words apart, a multiple of 4 and >= dpz_mask_words(n)), of rank_tab
 * (rank_stride entries apart, >= dpz_mt_rank_entries(n)) and count_dev[i] are bit for bit what
 * dpz_mt_mask(seeds[i], alphas[i], n, ...) writes.  One mask launch over chunks x m blocks, one
 * scan launch over m blocks and, above dpz_mt_coarse_chunks() chunks, one coarse launch over
 * (coarse - 1) x m blocks.  ws: dpz_mt_mask_batch_workspace_bytes(m, n).  Like dpz_mt_mask, a
 * call that needs table rows its device does not have yet BLOCKS on the host build and copy.
 * dpz_mask_gather_nodes: node_table is a DEVICE array of m entries of 8 64-bit words {x, mask,
 * rank_tab, vals, counter (or 0), count, status, 0}: count the mask's DEVICE int64 count, vals a
 * slot of `cap` values, status a DEVICE int32.  vals[rank(j)] = x[j] for every selected j with
 * rank(j) < cap, counter[j] += 1 for every selected j; nothing is written at or past vals + cap,
 * and status = (*count > cap) ? 1 : 0, so a slot that was too small is reported, never silently
 * truncated.  The float4 read of x is chosen per row from the row's alignment.
 * dpz_mask_decode_average_nodes: fold_table is a DEVICE array of m destinations of 68 64-bit
 * words: {local, out, w_self (fp32 in the low half), n_payloads} and 16 entries {mask, rank_tab,
 * vals, w (fp32 in the low half)}, the first n_payloads used; n_payloads (HOST int[m]) repeats the
 * counts so that a destination with more than 16 payloads is refused (DPZ_ERR_UNSUPPORTED, nothing
 * enqueued: the caller folds it through dpz_mask_decode_average with DPZ_FOLD_ACCUMULATE).  Each
 * element is folded exactly as by dpz_mask_decode_average; flags: DPZ_FOLD_SELF or 0.  The
 * launch first reads guard[0, guard_n) (DEVICE int32, may be NULL with guard_n = 0, e.g. the
 * gather's status words) and writes nothing if any word is nonzero.  No out may overlap any
 * local.                                                                                        */
size_t dpz_mt_mask_batch_workspace_bytes(int m, int64_t n);
int dpz_mt_mask_batch(int m, const uint32_t* seeds, const float* alphas, int64_t n, uint32_t* mask,
                      int64_t mask_stride, int32_t* rank_tab, int64_t rank_stride,
                      int64_t* count_dev, void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_mask_gather_nodes(int m, const void* node_table, int64_t n, int64_t cap,
                          dpz_stream_t stream);
int dpz_mask_decode_average_nodes(int m, const void* fold_table, const int* n_payloads, int64_t n,
                                  int flags, const int32_t* guard, int64_t guard_n,
                                  dpz_stream_t stream);

/* ---- Quantization (reference compression/Quantization.py), bit for bit ------------------------
 * Encode of n fp32 values x with float_precision k (1 <= k <= 2^30), all in fp32 with IEEE
 * divisions and ties-to-even rounding:
 *   m = max|x|,  S = the fp32 sum of |x| in numpy's order (consecutive chunks of 8192 elements,
 *   numpy's pairwise tree inside a chunk, the chunk sums added one after another),
 *   scale = (S / n) / k,  norm = m / k,  q_i = int32(rint(x_i / norm)),  qmax = |rint(m / norm)|,
 *   p = the power of two above qmax,  w = log2(p) + 1 bits per value,  u_i = q_i + p - 1.
 * Body: stream bit i*w + j holds bit w-1-j of u_i; stream bit t is bit t & 7 of byte t >> 3;
 * unused trailing bits are 0.  The wire value the Python class sends is
 * pickle((scale, uint8[padding, w, body...])) with padding = (8 - n*w % 8) % 8.
 * The reference rescales by the mean although it normalised by the max, so amplitudes do not
 * round-trip; the scale travels in the stream.
 * A statistics kernel and a pack kernel run back to back on `stream`, with no
 * host synchronisation; the pack kernel derives the parameters on the device and writes them to
 * `info`, 8 int32 words on the DEVICE:
 *   [0] status: 0 ok, 1 max|x| == 0, 2 a non-finite value, 3 m / k underflows, 4 body_cap too
 *       small for the width found (nothing is written to body for status != 0),
 *   [1] w, [2] padding, [3] scale bits, [4] norm bits, [5] max|x| bits, [6] S bits, [7] p - 1.
 * body: 4-byte aligned, body_cap bytes (a multiple of 4, at least 4 * ceil(n * w / 32); the words
 * past ceil(n*w/8) bytes are zero padding).  ws: dpz_quant_workspace_bytes(n), 16-byte aligned.
 * dpz_quant_block_elems(): the values one block of the pack kernel covers.
 * dpz_quant_decode: out[i] = float(double(u_i - 2^(w-1) + 1) * scale) for the n values of a body of
 * body_bytes bytes held in a 4-byte aligned DEVICE buffer readable up to the next multiple of 4.
 * Both return DPZ_ERR_ARG before any device call for n < 1 (or n >= 2^31), k outside [1, 2^30],
 * w outside [2, 32], a body shorter than n * w bits, null or misaligned pointers.            */
size_t dpz_quant_workspace_bytes(int64_t n);
int64_t dpz_quant_block_elems(void);
int dpz_quant_encode(const float* x, int64_t n, int64_t k, uint8_t* body, int64_t body_cap,
                     int32_t* info, void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_quant_decode(const uint8_t* body, int64_t body_bytes, int64_t n, int w, double scale,
                     float* out, dpz_stream_t stream);

/* ---- Dense folds of a round's nodes at once (decentralizepy_amd/gossip_epidemic.py) -----------
 * Full-model rounds (Epidemic Learning's PlainAverageSharing, the D-PSGD full share of class
 * Sharing): m receivers fold whole source rows in ONE launch.  fold_table is a DEVICE array of
 * 64-bit words: n_src source row pointers (fp32 rows of n elements: the flat models of the
 * round), then m receivers of 4 words {out, self (int32: the index of its own row) | w_self
 * (fp32) in the high half, start (int32) | count (int32) in the high half, 0}, then n_entries
 * list entries {src (int32) | w (fp32) in the high half}; receiver j folds the entries
 * [start_j, start_j + count_j) in that order.  A list may have any length.  host_table is the
 * HOST copy of the same words: every check below is made on it, before anything is enqueued.
 * Each element is folded exactly as by the dense-payload DPZ_FOLD_SELF form of
 * dpz_decode_average: t = fl(v_0 w_0), t = fl(t + fl(v_i w_i)) in list order,
 * out = fl(t + fl(local w_self)); a receiver with an empty list gets a bitwise copy of its own
 * row (the reference leaves such a node's model untouched, EL_Local.py:162-165).
 * mode: DPZ_DENSE_STAGED stages a column tile of every source row in LDS once and forms every
 * receiver's output from it (a tile of dpz_dense_tile_elems(n_src) elements: the largest of 1024 /
 * 512 / 256 with n_src * tile * 4 bytes <= 64 KiB, 0 when none fits: DPZ_ERR_UNSUPPORTED);
 * DPZ_DENSE_DIRECT runs a grid of tiles x receivers, each receiver streaming its sources from
 * memory; DPZ_DENSE_AUTO takes the path dpz_dense_auto_mode(n_src, sum(count_j + 1), n) names:
 * staged iff a tile fits, 2 n_src <= sum(count_j + 1) (staging at least halves the row reads) and
 * n spans at least 384 tiles (measured: below that the staged grid, tiles only, leaves the machine
 * idle and the direct path is faster).  Rows that are
 * all 16-byte aligned take 16-byte loads and stores, otherwise every access is per element.
 * DPZ_ERR_ARG: null pointers, m < 1, n < 1, n_src < 1, a mode outside 0 .. 2, an index outside
 * [0, n_src), a list outside [0, n_entries), an out row that equals or overlaps a source row or
 * another out row (receivers write while others still read: the caller double-buffers).
 * DPZ_ERR_UNSUPPORTED: n >= 2^31 or m > 65535.                                                  */
#define DPZ_DENSE_AUTO 0
#define DPZ_DENSE_STAGED 1
#define DPZ_DENSE_DIRECT 2
int64_t dpz_dense_tile_elems(int n_src);
int dpz_dense_auto_mode(int n_src, int64_t row_reads, int64_t n);
int dpz_dense_average_nodes(int m, const void* fold_table, const void* host_table,
                            int64_t n_entries, int n_src, int64_t n, int mode,
                            dpz_stream_t stream);

/* ---- A Choco-SGD round of a rank's nodes at once (decentralizepy_amd/gossip_choco.py) ----------
 * Reference sharing/Choco.py:186-207 (threshold sparsification), :359-453 (the round).  A node's
 * packed row is [count (int64), status (int32), 0 | cap x int32 idx | cap x fp32 val], 4-byte
 * aligned (the count is written and read as two 32-bit words; it is below 2^31).
 * dpz_choco_encode_nodes: `_pre_step` + `serialized_model` of m nodes of one size n.  node_table
 * is a DEVICE array of m entries of 4 64-bit words {x, x_hat, row, 0}.  Per node, exactly what
 * dpz_topk_threshold selects from d = fl(x - x_hat), which is never written to memory: T = the
 * k-th largest |d| (NaN ranks above +inf), every i with |d_i| >= T and d_i != 0 in ascending
 * index order, all ties kept, no exact zeros when T == 0; idx = i, val = d_i.  The row's count is
 * the number selected, status = (count > cap) ? 1 : 0, and nothing is written at or past idx + cap
 * or val + cap: an overflow is reported, never silently truncated.  x and x_hat are read with
 * 16-byte loads where both rows are 16-byte aligned, per element otherwise.  One memset and nine
 * launches whatever m is (the node is the grid's second dimension): three histogram passes, each
 * with a 1-block-per-node resolve, a count pass over chunks of dpz_choco_chunk_elems() elements,
 * a 1-block-per-node scan and the ordered compaction; no host synchronisation, no copy to the
 * host.  ws: dpz_choco_encode_workspace_bytes(m, n) DEVICE bytes, 4-byte aligned, any content.
 * All checks come before anything is enqueued: DPZ_ERR_ARG for m < 1, n < 1, k < 1 (the k = 0
 * "send everything" branch stays with the per-node plugin), k > n, cap < 1 or null pointers;
 * DPZ_ERR_UNSUPPORTED for n >= 2^31 or m > 65535; DPZ_ERR_WORKSPACE for a short workspace.
 * dpz_choco_fold_nodes: `_averaging` of m receivers in ONE launch, in place on each receiver's
 * x, x_hat and s rows (fp32, n elements).  fold_table is a DEVICE array of 64-bit words: m
 * receivers of 6 words {x, x_hat, s, its own packed row, w_self (fp32) | its row's cap (int32) in
 * the high half, start (int32) | count (int32) in the high half}, then n_entries list entries of
 * 2 words {packed row, w (fp32) | that row's cap (int32) in the high half}; receiver j folds the
 * entries [start_j, start_j + count_j) in that order, any count including 0.  host_table is the
 * HOST copy of the same words: every check is made on it, before anything is enqueued.  The
 * rows' counts are read from their headers on the device (clamped to the row's cap).  Per element
 * j, with t_p[j] / q_self[j] the payload's value at j or 0 where it has no entry, one fp32
 * rounding per operation:
 *   x_hat' = fl(x_hat + q_self[j]);  s' = s;  s' = fl(s' + fl(t_p[j] w_p)) in list order;
 *   s' = fl(s' + fl(q_self[j] w_self));  x' = fl(x + fl(step_size fl(s' - x_hat')))
 * which is, bit for bit, dpz_elementwise(DPZ_EW_ADD), dpz_decode_average(DPZ_FOLD_ZERO_BASE |
 * DPZ_FOLD_ACCUMULATE | DPZ_FOLD_SELF) and dpz_elementwise(DPZ_EW_CHOCO) as long as s and x_hat
 * hold no -0 (they never do when they start at +0: dpz_choco.hip), a payload's indices are
 * ascending and unique and the weights are finite.  A block owns a tile of
 * dpz_choco_tile_elems() elements of one receiver; there is no n-length temporary.  The launch
 * first reads guard[0, guard_n) (DEVICE int32, may be NULL with guard_n = 0, e.g. the gathered
 * rows' status words) and writes nothing at all if any word is nonzero.
 * DPZ_ERR_ARG: null pointers, m < 1, n < 1, a list outside [0, n_entries), a cap < 1, a
 * non-finite weight or step_size, a misaligned pointer, guard_n < 0 or guard words without a
 * guard, an x / x_hat / s row that overlaps any other row of the table (payload rows included:
 * receivers write while others read).  DPZ_ERR_UNSUPPORTED: n >= 2^31 or m > 65535.            */
int64_t dpz_choco_chunk_elems(void);
int64_t dpz_choco_tile_elems(void);
size_t dpz_choco_encode_workspace_bytes(int m, int64_t n);
int dpz_choco_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, int64_t cap,
                           void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_choco_fold_nodes(int m, const void* fold_table, const void* host_table, int64_t n_entries,
                         int64_t n, float step_size, const int32_t* guard, int64_t guard_n,
                         dpz_stream_t stream);

/* ---- Quantised full-model rounds of a rank's nodes at once (decentralizepy_amd/gossip_quant.py) -
 * Reference sharing/Sharing.py and sharing/PlainAverageSharing.py with compress = True and
 * compression_class = Quantization: every sender's model travels as its quantised stream and a
 * receiver folds the decoded streams with its own fp32 model.  A node's packed row is 4-byte
 * aligned int32 words
 *   [count = n (int64 as two words), status, 0 | the 8 info words of dpz_quant_encode | body],
 * dpz_quant_row_words(n, slot_bits) = 12 + ceil(n * slot_bits / 32) words (0 for n < 1,
 * n >= 2^31 or slot_bits outside [2, 32]); the status word repeats info[0].
 * dpz_quant_encode_nodes: dpz_quant_encode of m vectors of one length n in TWO launches whatever
 * m is, the node in the grid's second dimension.  node_table is a DEVICE array of m entries of 2
 * 64-bit words {x, packed row}.  Per node the info words and the body are bit for bit what
 * dpz_quant_encode(x, n, k, body, 4 * ceil(n * slot_bits / 32), info, ...) writes, statuses 1-4
 * included: nothing is written to the body of a row whose status is nonzero, and a field wider
 * than slot_bits is status 4, never a write past the slot.  x is read with 16-byte loads where it
 * is 16-byte aligned, per element otherwise (chosen per node on the device); a row needs 4-byte
 * alignment only.  Nothing is read back, nothing synchronises.  ws:
 * dpz_quant_encode_nodes_workspace_bytes(m, n) DEVICE bytes, 16-byte aligned (each node has its
 * own 256 max words and chunk sums).  All checks come before anything is enqueued: DPZ_ERR_ARG
 * for m < 1, n < 1, k outside [1, 2^30], slot_bits outside [2, 32], null or misaligned pointers;
 * DPZ_ERR_UNSUPPORTED for n >= 2^31 or m > 65535; DPZ_ERR_WORKSPACE for a short workspace.
 * dpz_qdense_average_nodes: dpz_dense_average_nodes with packed rows as the sources.  fold_table
 * is a DEVICE array of 64-bit words: n_src packed-row pointers, then m receivers of 4 words {out,
 * own (the receiver's fp32 model, n elements), w_self (fp32) in the low half, start (int32) |
 * count (int32) in the high half}, then n_entries list entries {src (int32) | w (fp32) in the
 * high half}; host_table is the HOST copy on which every check is made before anything is
 * enqueued.  A source's width w and scale are read from its row's header on the device (w clamped
 * to [2, 32]; different sources may differ); its value i is
 *   v = float(double(u - 2^(w-1) + 1) * double(scale)),
 * u the MSB-first w-bit field at stream bits [i w, (i+1) w), as dpz_quant_decode gives it (for
 * w <= 25 the fp32 product float(q) * scale: q is exact and the product has at most 48
 * significant bits, so both round the same exact value once; above, the fp64 product).  No read
 * goes past min(ceil(n w / 32), cap_dwords) dwords of a body; cap_dwords is what every source row
 * holds.  The fold order and the empty list are those of dpz_dense_average_nodes, fp32 denormals
 * kept.  The launch first reads guard[0, guard_n) (DEVICE int32, may be NULL with guard_n = 0,
 * e.g. the gathered rows' status words): if any word is nonzero EVERY out row becomes a bitwise
 * copy of its own row.  mode: DPZ_DENSE_AUTO / _STAGED / _DIRECT; the staged path decodes a column
 * tile of dpz_qdense_tile_elems(n_src) elements (dpz_dense_tile_elems' rule, a multiple of 32: a
 * tile starts on a dword of every body) of every source into LDS once; auto takes
 * dpz_qdense_auto_mode(n_src, sum(count_j + 1), n).  Rows out / own that are all 16-byte aligned
 * take 16-byte loads and stores.  DPZ_ERR_ARG: null or misaligned (4-byte) pointers, m < 1, n < 1,
 * n_src < 1, cap_dwords < 1 or > n, a mode outside 0 .. 2, guard_n < 0 or guard words without a
 * guard, an index outside [0, n_src), a list outside [0, n_entries), an out row that overlaps a
 * packed row, any receiver's own row or another out row.  DPZ_ERR_UNSUPPORTED: n >= 2^31,
 * m > 65535, the staged mode where no tile fits.                                                */
int64_t dpz_quant_row_words(int64_t n, int slot_bits);
size_t dpz_quant_encode_nodes_workspace_bytes(int m, int64_t n);
int dpz_quant_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, int slot_bits,
                           void* ws, size_t ws_bytes, dpz_stream_t stream);
int64_t dpz_qdense_tile_elems(int n_src);
int dpz_qdense_auto_mode(int n_src, int64_t row_reads, int64_t n);
int dpz_qdense_average_nodes(int m, const void* fold_table, const void* host_table,
                             int64_t n_entries, int n_src, int64_t n, int64_t cap_dwords, int mode,
                             const int32_t* guard, int64_t guard_n, dpz_stream_t stream);

/* ---- An STC round of a federation at once (decentralizepy_amd/gossip_stc.py) --------------------
 * Reference sharing/STC.py: sparse top-k with residual error feedback, clients and a server that
 * compresses its broadcast with a residual of its own.  Finite inputs only.  A packed row is
 * [count = k (int64 as two words), status = 0, 0 | up4(k) x int32 idx | up4(k) x fp32 val], 4-byte
 * aligned, up4(k) = k rounded up to a multiple of 4; exactly k entries are written, the words past
 * them and past the row are untouched.
 * dpz_stc_encode_nodes: the exact-k selection of m nodes of one size n.  node_table is a DEVICE
 * array of m entries of 4 64-bit words {x, prev, r, row}.  Per node, with one fp32 rounding per
 * operation, c_i = fl(fl(x_i - prev_i) + r_i); the k largest keys |c_i| (NaN ranks above +inf) are
 * selected, ties at the k-th key going to the lowest indices; idx = the selection ascending,
 * val = c[idx]; afterwards prev = x, r_i = +0 where selected and c_i elsewhere: bit for bit
 * dpz_topk_encode(x, prev, r, DPZ_ACC_ACCUMULATE, vals_src = r, DPZ_TOPK_EXACT) and a copy of x to
 * prev.  An entry with x == NULL is in server form: r already holds c, nothing is formed and prev
 * is not touched.  The first histogram pass forms c and stores it into r and x into prev; every
 * later pass reads r alone.  16-byte loads and stores where the node's rows are 16-byte aligned,
 * per element otherwise (chosen per node on the device).  One memset and nine launches whatever m
 * is: three histogram passes, each with a 1-block-per-node resolve, a count pass over chunks of
 * dpz_stc_chunk_elems() elements (key > T and key == T), a 1-block-per-node scan that allots the
 * ties in index order, and the ordered compaction.  No float atomics; the result does not depend
 * on the grid; no host synchronisation.  ws: dpz_stc_encode_workspace_bytes(m, n) DEVICE bytes,
 * 4-byte aligned, any content.  All checks come before anything is enqueued: DPZ_ERR_ARG for
 * m < 1, n < 1, k < 1, k > n, null or misaligned pointers; DPZ_ERR_UNSUPPORTED for n >= 2^31 or
 * m > 65535; DPZ_ERR_WORKSPACE for a short workspace.
 * dpz_stc_server_fold: `_averaging_server` in ONE launch, in place on r_s (fp32, n elements).
 * table is a DEVICE array of n_payloads entries of 2 64-bit words {packed row, w (fp32) in the low
 * half}; host_table is the HOST copy on which every check is made.  total starts at +0; for each
 * payload in table order total[idx[e]] = fl(total[idx[e]] + fl(val[e] w)); then
 * r_s = fl(r_s + total).  A block owns a tile of dpz_stc_tile_elems() elements and keeps its total
 * in LDS; there is no n-length temporary.  A row's count is read from its header (clamped to k);
 * indices are ascending and unique within a row; an index outside the tile or outside [0, n) is
 * skipped, never written through.  DPZ_ERR_ARG: n_payloads < 1, n < 1, k < 1, k > n, null or
 * misaligned pointers, a non-finite weight, a payload row that overlaps r_s.
 * DPZ_ERR_UNSUPPORTED: n >= 2^31.
 * dpz_stc_apply_nodes: `process_received` of m models in ONE launch, in place.  table is a DEVICE
 * array of m fp32 row pointers (n elements each, distinct rows); for each of them
 * x[idx[e]] = fl(x[idx[e]] + val[e]) over the entries of the packed row `row`.  Indices are unique:
 * no atomics.  An index outside [0, n) is skipped; an element the row does not name keeps its bits
 * (a -0 too, where the reference's dense add gives +0).  DPZ_ERR_ARG: m < 1, n < 1, k < 1, k > n,
 * null or misaligned pointers.  DPZ_ERR_UNSUPPORTED: n >= 2^31 or m > 65535.                   */
int64_t dpz_stc_chunk_elems(void);
int64_t dpz_stc_tile_elems(void);
size_t dpz_stc_encode_workspace_bytes(int m, int64_t n);
int dpz_stc_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, void* ws,
                         size_t ws_bytes, dpz_stream_t stream);
int dpz_stc_server_fold(int n_payloads, const void* table, const void* host_table, int64_t n,
                        int64_t k, float* r_s, dpz_stream_t stream);
int dpz_stc_apply_nodes(int m, const void* table, int64_t n, int64_t k, const int32_t* row,
                        dpz_stream_t stream);

/* ---- A top-k round with accumulated changes at once (decentralizepy_amd/gossip_topkacc.py) ------
 * Reference sharing/PartialModel.py with accumulation = True, both settings of
 * accumulate_averaging_changes (:305-331 `_pre_step`, :188-255 the selection, the counter and the
 * rewind, :333-353 `_post_step`).  Finite inputs only.  The packed row is STC's:
 * [count = k (int64 as two words), status = 0, 0 | up4(k) x int32 idx | up4(k) x fp32 val], 4-byte
 * aligned; exactly k entries are written, the words past them and past the row are untouched.
 * dpz_topkacc_encode_nodes: the exact-k selection of m nodes of one size n.  node_table is a DEVICE
 * array of m entries of 6 64-bit words {x, x0, acc, key, counter (or 0), row}.  Per node, with one
 * fp32 rounding per operation:
 *   mode DPZ_ACC_ACCUMULATE  acc_i = fl(acc_i + fl(x_i - x0_i)) everywhere, the key is |acc_i|; the
 *                            key row is acc itself (the entry's key word is not read);
 *   mode DPZ_ACC_ADD         the key is |fl(fl(x_i - x0_i) + acc_i)|, formed once into the scratch
 *                            row `key` (n floats, any content, overwritten); acc is not written
 *                            before the rewind.
 * The k largest keys (NaN ranks above +inf) are selected, ties at the k-th key going to the lowest
 * indices; idx = the selection ascending, val = x[idx]; counter[idx] += 1 (plain stores: an element
 * has one owner); acc[idx] = +0: bit for bit dpz_topk_encode(x, x0, acc, mode, vals_src = x, ...,
 * counter, DPZ_TOPK_EXACT) per node.  x and x0 are never written.  The first histogram pass reads
 * x, x0 and acc and stores the key row; every later pass reads the key row alone.  16-byte loads and
 * stores where the node's rows are 16-byte aligned, per element otherwise (chosen per node on the
 * device).  One memset and nine launches whatever m is: three histogram passes (10/11/10 bits),
 * each with a 1-block-per-node resolve, a count pass over chunks of dpz_topkacc_chunk_elems()
 * elements, a 1-block-per-node scan that allots the ties in index order, and the ordered
 * compaction.  No float atomics; the result does not depend on the grid; no host synchronisation.
 * ws: dpz_topkacc_encode_workspace_bytes(m, n) DEVICE bytes, 4-byte aligned, any content.  All
 * checks come before anything is enqueued: DPZ_ERR_ARG for m < 1, a null or misaligned table or
 * workspace, n outside [1, 2^31), k outside [1, n], a mode other than the two above, a short
 * workspace; DPZ_ERR_UNSUPPORTED for m > 65535.
 * dpz_topkacc_post_nodes: the accumulating `_post_step` (accumulate_averaging_changes = True) of m
 * nodes in ONE launch over the same node table, of which it reads {x, x0, acc}:
 * acc_i = fl(acc_i + fl(x_i - x0_i)), x the averaged model and x0 the model the round started
 * from; x and x0 are not written.  16-byte accesses where a node's three rows are aligned.
 * DPZ_ERR_ARG: m < 1, a null or misaligned table, n outside [1, 2^31); DPZ_ERR_UNSUPPORTED:
 * m > 65535.                                                                                   */
int64_t dpz_topkacc_chunk_elems(void);
size_t dpz_topkacc_encode_workspace_bytes(int m, int64_t n);
int dpz_topkacc_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, int mode,
                             void* ws, size_t ws_bytes, dpz_stream_t stream);
int dpz_topkacc_post_nodes(int m, const void* node_table, int64_t n, dpz_stream_t stream);

/* ---- A JWINS round of a rank's nodes at once (decentralizepy_amd/gossip_jwins_batch.py) ----------
 * dpz_dwt_sym2_nodes: dpz_dwt_sym2 of m nodes of one length n and one level (1-4) in ONE launch,
 * the node in the grid's second dimension.  table is a DEVICE array of m entries of 4 64-bit words
 * {x, x0, coeffs_x or 0, coeffs_diff or 0}; host_table is its HOST copy, on which every check is
 * made.  Per node the result is bit for bit dpz_dwt_sym2(x, x0, n, level, coeffs_x, coeffs_diff,
 * accumulate) (the tiles run on the span path at every level, which gives the bits of the level-4
 * interior path).  Every entry names the same set of outputs; with no output nothing is enqueued.
 * dpz_idwt_sym2_nodes: dpz_idwt_sym2 of m nodes in ONE launch; entries of 2 words {coeffs, out}.
 * Both, before anything is enqueued: DPZ_ERR_ARG for m < 1, n < 1, a null or misaligned table, a
 * null host table, a null required pointer (x; x0 with coeffs_diff; coeffs, out), a row that is
 * not 16-byte aligned, entries that differ in their outputs, accumulate without coeffs_diff;
 * DPZ_ERR_UNSUPPORTED for m > 65535, a level outside 1-4 or an n the level does not accept.  The
 * kernels are timed as "dwt" and "idwt".
 * dpz_jwins_encode_nodes: the selection of m nodes of one coefficient count n, each with its own
 * k.  node_table is a DEVICE array of m entries of 8 64-bit words {c, acc, vals_src, counter (or
 * 0), idx_out, val_out, k, 0}.  Per node, with one fp32 rounding per operation:
 *   1 <= k <= n  the key is |fl(c_i + acc_i)|, formed once by the first histogram pass and stored
 *                IN PLACE into the c row.  The k largest keys are selected, ties at the k-th key
 *                going to the lowest indices; idx = the selection ascending, val = vals_src[idx];
 *                counter[idx] += 1 (plain stores); acc[idx] = +0; acc is unchanged elsewhere: bit
 *                for bit dpz_topk_encode(x = c, x0 = NULL, acc, DPZ_ACC_ADD, vals_src, n, k, ...,
 *                counter, DPZ_TOPK_EXACT).  Exactly k entries are written, the words past them
 *                are untouched.
 *   k == 0       a full share: the first pass stores +0 to all of acc and, if val_out != 0,
 *                copies vals_src to val_out (n floats); c, the counter and idx_out are not
 *                touched, no other pass reads or writes the node.
 * A k above n is the caller's error (the table is on the device: the Python wrapper checks its
 * host values); the kernels then select all n and write nothing outside the node's rows of n.
 * 16-byte accesses where a node's rows are 16-byte aligned, per element otherwise.  One memset and
 * nine launches whatever m is, timed under the topk_exact_* names; no float atomics; the result
 * does not depend on the grid; no host synchronisation.  Finite inputs only.  ws:
 * dpz_jwins_encode_workspace_bytes(m, n) DEVICE bytes, 4-byte aligned, any content.  Before
 * anything is enqueued: DPZ_ERR_ARG for m < 1, a null or misaligned table or workspace, n outside
 * [1, 2^31), a short workspace; DPZ_ERR_UNSUPPORTED for m > 65535.                              */
int dpz_dwt_sym2_nodes(int m, const void* table, const void* host_table, int64_t n, int level,
                       int accumulate, dpz_stream_t stream);
int dpz_idwt_sym2_nodes(int m, const void* table, const void* host_table, int64_t n, int level,
                        dpz_stream_t stream);
int64_t dpz_jwins_chunk_elems(void);
size_t dpz_jwins_encode_workspace_bytes(int m, int64_t n);
int dpz_jwins_encode_nodes(int m, const void* node_table, int64_t n, void* ws, size_t ws_bytes,
                           dpz_stream_t stream);

/* ---- An FFT round of a rank's nodes at once (decentralizepy_amd/gossip_fft.py) -------------------
 * dpz_rfft_nodes: `jobs` forward real FFTs of one even length n >= 4 with a native plan
 * (dpz_fft_native), in one launch set of as many launches as one dpz_rfft of that n: the job is in
 * the grid's second dimension of the pass and pairing kernels.  table is a DEVICE array of `jobs`
 * entries of 4 64-bit words {x, x0 or 0, out, accumulate (0 / 1)}; host_table is its HOST copy, on
 * which every check is made.  x, x0: n reals; out: n / 2 + 1 complex.  With x0 the first pass
 * loads fl(x[i] - x0[i]) (dpz_elementwise(DPZ_EW_SUB)'s difference); with accumulate the pairing
 * pass stores out[k] = fl(out[k] + X[k]) per component (dpz_elementwise(DPZ_EW_ADD)'s sum).  Per
 * job the result is bit for bit that of the single calls.  x and x0 are only read.
 * dpz_irfft_nodes: `jobs` inverse transforms; entries of 2 words {coeffs, out}: n / 2 + 1 complex,
 * only read, and n reals; per job bit for bit dpz_irfft's result.
 * ws: dpz_fft_nodes_workspace_bytes(jobs, n) DEVICE bytes (-1 for a size the calls refuse): one
 * scratch row of n / 2 complex per job, and a second one per job where the plan has two or more
 * passes (an accumulating job cannot run its passes through its output row).
 * Both, before anything is enqueued and with nothing written: DPZ_ERR_ARG for jobs < 1, a null or
 * misaligned table, a null host table, a null x / out / coeffs, a row that is not 8-byte aligned,
 * an accumulate word above 1; DPZ_ERR_UNSUPPORTED for an odd n, n < 4, an n whose plan is not
 * native (hipFFT sizes) and jobs > 65535; DPZ_ERR_WORKSPACE for a null or short workspace.  The
 * kernels are timed as "fft".
 * dpz_cplx_encode_nodes: the exact top-k of |c| over the n complex coefficients of m nodes, one k
 * (1 <= k <= n) and one DPZ_ACC_* mode per call.  node_table is a DEVICE array of m entries of 8
 * 64-bit words {change, acc (or 0 with DPZ_ACC_NONE), vals_src, key, counter (or 0), pair_out,
 * val_out, 0}: change, acc, vals_src n complex; key n fp32 (scratch); counter n int32; pair_out
 * 2 k int32 (8-byte aligned); val_out k complex.  The first pass does dpz_cplx_key's accumulation
 * step and stores key[i] = sqrtf(re re + im im) (one rounding per operation); the k largest keys
 * are selected, ties at the k-th key going to the lowest indices; per selected i, ascending:
 * pair_out = (2 i, 2 i + 1), val_out = vals_src[i], counter[i] += 1, acc[i] = (+0, +0) when acc
 * is set: bit for bit dpz_cplx_key, the exact dpz_topk_encode of the key, dpz_cplx_gather and
 * dpz_cplx_pair_indices.  One memset and nine launches whatever m is, timed under the topk_exact_*
 * names; no float atomics; the result does not depend on the grid; no host synchronisation.
 * Finite inputs only.  ws: dpz_cplx_encode_workspace_bytes(m, n) DEVICE bytes, 4-byte aligned.
 * Before anything is enqueued: DPZ_ERR_ARG for m < 1, a null or misaligned table or workspace, n
 * outside [1, 2^30), k outside [1, n], an unknown mode, a short workspace; DPZ_ERR_UNSUPPORTED
 * for m > 65535.  The table's rows are the caller's to get right (the Python wrapper checks its
 * host copy).                                                                                    */
int64_t dpz_fft_nodes_workspace_bytes(int jobs, int64_t n);
int dpz_rfft_nodes(int jobs, const void* table, const void* host_table, int64_t n, void* ws,
                   size_t ws_bytes, dpz_stream_t stream);
int dpz_irfft_nodes(int jobs, const void* table, const void* host_table, int64_t n, void* ws,
                    size_t ws_bytes, dpz_stream_t stream);
/* ---- Chirp-z (Bluestein) real FFTs: the batched transforms at every even size -----------------
 * dpz_rfft_chirp_nodes / dpz_irfft_chirp_nodes take dpz_rfft_nodes' / dpz_irfft_nodes' tables and
 * mean the same transforms (the x0 subtraction one fp32 subtraction per element on load, the
 * accumulating store one fp32 addition per component; x, x0 and coeffs only read), for EVERY even
 * n in [4, 2^30] - sizes with a native plan included.  The complex DFT of length L = n / 2 runs as
 * a cyclic convolution of the padded length P = dpz_fft_chirp_length(n), the smallest 7-smooth
 * number >= 2 L - 1 (0 for an n the calls refuse): a = z . w (w_j = exp(-i pi j^2 / L), zero up to P), the
 * native passes of DFT_P, the product with the cached table DFT_P(b) / P of the wrapped conjugate
 * chirp (built in double on the host, rounded once), the inverse passes, then w_k and the even-n
 * pairing; the inverse runs the chain from the c2r pairing with the conjugate chirp and 1 / n.
 * The result agrees with the native kernels' to rounding, not bit for bit; a job's result does not
 * depend on `jobs` or on its position.  2 npass(P) + 3 launches whatever `jobs` is (the job in the
 * grid's second dimension), timed as "fft"; no host synchronisation.  The library allocates the
 * per-(device, n) chirp tables (L + P complex) beside the twiddles.
 * ws: dpz_fft_chirp_nodes_workspace_bytes(jobs, n) DEVICE bytes (-1 where refused): two rows of P
 * complex per job.  Before anything is enqueued, as the native batched calls: DPZ_ERR_ARG for
 * jobs < 1, a null or misaligned table, a null host table, a null x / out / coeffs, a row that is
 * not 8-byte aligned, an accumulate word above 1; DPZ_ERR_UNSUPPORTED for an odd n, n < 4,
 * n > 2^30 (before the rows are read) and jobs > 65535; DPZ_ERR_WORKSPACE for a null or short
 * workspace.                                                                                      */
int64_t dpz_fft_chirp_length(int64_t n);
int64_t dpz_fft_chirp_nodes_workspace_bytes(int jobs, int64_t n);
int dpz_rfft_chirp_nodes(int jobs, const void* table, const void* host_table, int64_t n, void* ws,
                         size_t ws_bytes, dpz_stream_t stream);
int dpz_irfft_chirp_nodes(int jobs, const void* table, const void* host_table, int64_t n, void* ws,
                          size_t ws_bytes, dpz_stream_t stream);
int64_t dpz_cplx_chunk_elems(void);
size_t dpz_cplx_encode_workspace_bytes(int m, int64_t n);
int dpz_cplx_encode_nodes(int m, const void* node_table, int64_t n, int64_t k, int acc_mode,
                          void* ws, size_t ws_bytes, dpz_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPZ_CODEC_H */
