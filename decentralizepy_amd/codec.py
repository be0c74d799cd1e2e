"""Device-tensor front end of the HIP codec (libdpzcodec.so).

Every function takes and returns torch tensors that live on a ROCm device; PyTorch is used only
for allocation, streams and tensor handles — the arithmetic runs in the hand-written HIP kernels
behind the C ABI (``include/dpz_codec.h``).  Calls are enqueued on the current torch stream.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (DPZ_ACC_ACCUMULATE, DPZ_ACC_ADD, DPZ_ACC_NONE, DPZ_EW_ADD, DPZ_EW_CHOCO,
                   DPZ_EW_SUB, DPZ_FOLD_REPLACE_ONLY,
                   DPZ_FOLD_SELF, DPZ_TOPK_ASYNC, DPZ_TOPK_EXACT, DPZ_TOPK_STREAM,
                   DPZ_TOPK_TAIL, check)

__all__ = ["DPZ_ACC_NONE", "DPZ_ACC_ACCUMULATE", "DPZ_ACC_ADD", "DPZ_EW_SUB", "DPZ_EW_ADD",
           "DPZ_EW_CHOCO", "Workspace", "topk_encode",
           "topk_threshold", "mask_below_threshold", "elementwise",
           "topk_complete", "decode_average", "replace", "wavedec_len", "wavedec", "waverec",
           "pack_fp16", "unpack_fp16", "elias_encode", "elias_decode", "elias_decode_async",
           "KernelTimer", "NodeStepBatch", "topk_sticky_status", "rfft", "irfft", "fft_native", "cplx_key",
           "cplx_gather", "cplx_pair_indices", "lz4_compress", "lz4_decompress", "lz4_frame_info", "lz4_geometry",
           "delta_i32", "running_sum_i32", "mask_words", "topk_encode_sliced", "counter_unslice",
           "counter_slice", "rewind_apply", "counter_flush", "counter_flush_batch", "mt_mask",
           "mt_rank_entries", "mask_gather", "mask_decode_average", "mt_mask_batch",
           "gather_node_table", "mask_gather_nodes", "fold_node_table",
           "mask_decode_average_nodes", "quant_encode", "quant_decode",
           "quant_block_elems", "QuantInfo", "dense_tile_elems", "dense_auto_mode", "DenseTable",
           "dense_average_nodes", "choco_chunk_elems", "choco_tile_elems", "choco_node_table",
           "choco_encode_nodes", "ChocoTable", "choco_fold_nodes", "quant_row_words",
           "quant_node_table", "quant_encode_nodes", "qdense_tile_elems", "qdense_auto_mode",
           "QDenseTable", "qdense_average_nodes", "stc_chunk_elems", "stc_tile_elems",
           "stc_row_words", "stc_node_table", "stc_encode_nodes", "StcFoldTable",
           "stc_server_fold", "stc_apply_table", "stc_apply_nodes", "topkacc_chunk_elems",
           "topkacc_row_words", "topkacc_node_table", "topkacc_encode_nodes",
           "topkacc_post_nodes", "DwtNodesTable", "IdwtNodesTable", "dwt_sym2_nodes",
           "idwt_sym2_nodes", "jwins_chunk_elems", "JwinsEncodeTable", "jwins_encode_nodes"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (got {t.device}); no CPU path exists")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


class Workspace:
    """Caller-owned device scratch for the encoder and the decoder, reused across calls.

    The top-k workspace must be zero-filled before its first use (the library keeps it so
    afterwards), hence ``torch.zeros``.
    """

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None
        self._nk = None
        self.dbuf = None
        self.ebuf = None
        self.hint_key = None  # signature of the last sampled-path encode enqueued on buf

    def get(self, n, k):
        if self.buf is not None and self._nk == (n, k):
            return self.buf
        need = int(_lib.lib().dpz_topk_workspace_bytes(int(n), int(k)))
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.zeros(max(need, 256), dtype=torch.uint8, device=self.device)
            self.hint_key = None
        self._nk = (n, k)
        return self.buf

    def get_decode(self, n, n_payloads):
        need = int(_lib.lib().dpz_decode_workspace_bytes(int(n), int(n_payloads)))
        if self.dbuf is None or self.dbuf.numel() < need:
            self.dbuf = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self.dbuf

    def get_elias(self, k, nbytes):
        need = int(_lib.lib().dpz_elias_workspace_bytes(int(k), int(nbytes)))
        if self.ebuf is None or self.ebuf.numel() < need:
            self.ebuf = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return self.ebuf


def topk_encode(x, k, x0=None, acc=None, acc_mode=DPZ_ACC_NONE, vals_src=None, counter=None,
                idx_out=None, val_out=None, workspace=None, exact=False, asynchronous=False,
                phase=None, co_replace=None, status_out=None, shared=False, fold_base=None,
                val_fp16=False, hint=False, keep_x=False):
    """Top-k magnitude encode (reference PartialModel.py:164-255 / Wavelet.py:142-197).

    Returns ``(idx int32[k], val fp32[k])`` in ascending index order.  Mutates ``acc`` and
    ``counter`` in place like the reference mutates ``model.accumulated_changes`` and
    ``model.shared_parameters_counter``.  With ``asynchronous=True`` the call only enqueues
    work; call :func:`topk_complete` with the same arguments before reading the result.
    ``phase="stream"`` / ``"tail"`` split the enqueue in two (both asynchronous; see
    DPZ_TOPK_STREAM in dpz_codec.h) so independent work can overlap the latency-bound tail.
    ``co_replace=(local, idx, vals, out)`` also performs the independent decode
    ``replace(local, idx, vals, out=out)`` of a received payload inside the encoder's
    latency-bound selection launches (dpz_topk_encode_replace); it is complete when the encode's
    stream work is.  ``status_out`` (a 1-element int32 device tensor or view): asynchronous
    encode whose final status word (0 = final, else re-run with ``exact=True``) is written there
    on the device (dpz_topk_encode_status).  ``shared``: several codecs run concurrently on the
    GPU (DPZ_TOPK_SHARED: the smaller filter grid); identical results.
    ``fold_base=(base_out, weights, w_self)``: also write the no-hit base of the coming
    Metro-Hastings fold over x with those weights into ``base_out`` (dpz_topk_encode_foldbase;
    the filter writes it as it streams x), for a later ``decode_average(x, payloads, weights,
    w_self, out=base_out, base_ready=True)``.
    ``val_fp16``: the values are written as fp16 (round to nearest even, ``torch.half``), by the
    encode itself (DPZ_TOPK_VAL_FP16: the C5 payload's value packing); ``val`` is float16[k].
    ``hint``: a node's next round — take the key window from the previous encode's exact
    threshold on this ``workspace`` when that encode had the same n, k and key source, skipping
    the sample launch (DPZ_TOPK_HINT; a window that no longer brackets the k-th key misses and a
    blocking call re-runs the sampled path).  ``keep_x``: x is read again right after (the node's
    fold over its own model): stream it with the default cache policy (DPZ_TOPK_KEEP_X).  Both
    leave the result unchanged.
    """
    _require(x, torch.float32, "x")
    _require(x0, torch.float32, "x0")
    _require(acc, torch.float32, "acc")
    _require(counter, torch.int32, "counter")
    n = x.numel()
    k = int(k)
    if vals_src is None:
        vals_src = x
    _require(vals_src, torch.float32, "vals_src")
    if idx_out is None:
        idx_out = torch.empty(k, dtype=torch.int32, device=x.device)
    vdt = torch.float16 if val_fp16 else torch.float32
    if val_out is None:
        val_out = torch.empty(k, dtype=vdt, device=x.device)
    _require(val_out, vdt, "val_out")
    if val_fp16 and (co_replace is not None or fold_base is not None):
        raise ValueError("val_fp16: a plain encode (no co_replace / fold_base)")
    wso = workspace or Workspace(x.device)
    ws = wso.get(n, k)
    flags = ((DPZ_TOPK_EXACT if exact else 0) | (DPZ_TOPK_ASYNC if asynchronous else 0)
             | (_lib.DPZ_TOPK_SHARED if shared else 0)
             | (_lib.DPZ_TOPK_VAL_FP16 if val_fp16 else 0)
             | (_lib.DPZ_TOPK_KEEP_X if keep_x else 0))
    # the device checks the prior's signature itself; this only avoids a predictable miss
    hkey = (n, k, bool(shared), int(acc_mode), x0 is not None)
    if hint and not exact and wso.hint_key == hkey:
        flags |= _lib.DPZ_TOPK_HINT
    wso.hint_key = None if exact else hkey
    if phase is not None:
        flags |= {"stream": DPZ_TOPK_STREAM, "tail": DPZ_TOPK_TAIL}[phase]
    if fold_base is not None:
        base_out, fw, fws = fold_base
        _require(base_out, torch.float32, "base_out")
        if base_out.numel() != n:
            raise ValueError("fold base: base_out must hold n values")
        if co_replace is not None or phase is not None or status_out is not None:
            raise ValueError("fold_base: a whole encode without co_replace / phase / status_out")
        nw = len(fw)
        w_arr = (ctypes.c_float * max(nw, 1))(*[float(v) for v in fw])
        rc = _lib.lib().dpz_topk_encode_foldbase(
            _ptr(x), _ptr(x0), _ptr(acc), int(acc_mode), _ptr(vals_src), n, k, _ptr(idx_out),
            _ptr(val_out), _ptr(counter), _ptr(ws), ws.numel(), flags, nw, w_arr, float(fws),
            _ptr(base_out), _stream(x.device))
        check(rc, "dpz_topk_encode_foldbase")
        return idx_out, val_out
    if status_out is not None:
        _require(status_out, torch.int32, "status_out")
        if co_replace is not None or phase is not None or exact:
            raise ValueError("status_out: a plain sampled-path encode only")
        rc = _lib.lib().dpz_topk_encode_status(_ptr(x), _ptr(x0), _ptr(acc), int(acc_mode),
                                               _ptr(vals_src), n, k, _ptr(idx_out), _ptr(val_out),
                                               _ptr(counter), _ptr(ws), ws.numel(),
                                               _ptr(status_out),
                                               (_lib.DPZ_TOPK_SHARED if shared else 0)
                                               | (_lib.DPZ_TOPK_VAL_FP16 if val_fp16 else 0),
                                               _stream(x.device))
        check(rc, "dpz_topk_encode_status")
        return idx_out, val_out
    if co_replace is None:
        rc = _lib.lib().dpz_topk_encode(_ptr(x), _ptr(x0), _ptr(acc), int(acc_mode),
                                        _ptr(vals_src), n, k, _ptr(idx_out), _ptr(val_out),
                                        _ptr(counter), _ptr(ws), ws.numel(), flags,
                                        _stream(x.device))
        check(rc, "dpz_topk_encode")
        return idx_out, val_out
    if phase is not None:
        raise ValueError("co_replace cannot be combined with a phase split")
    r_local, r_idx, r_val, r_out = co_replace
    _require(r_local, torch.float32, "co_replace local")
    _require(r_idx, torch.int32, "co_replace idx")
    _require(r_val, torch.float32, "co_replace vals")
    _require(r_out, torch.float32, "co_replace out")
    if r_idx.numel() != r_val.numel() or r_out.numel() != r_local.numel():
        raise ValueError("co_replace: idx/vals or local/out sizes differ")
    r_n = r_local.numel()
    dws = (workspace or Workspace(x.device)).get_decode(r_n, 1)
    rc = _lib.lib().dpz_topk_encode_replace(
        _ptr(x), _ptr(x0), _ptr(acc), int(acc_mode), _ptr(vals_src), n, k, _ptr(idx_out),
        _ptr(val_out), _ptr(counter), _ptr(ws), ws.numel(), flags, _ptr(r_local), _ptr(r_idx),
        _ptr(r_val), r_idx.numel(), r_n, _ptr(r_out), _ptr(dws), dws.numel(), _stream(x.device))
    check(rc, "dpz_topk_encode_replace")
    return idx_out, val_out


def mask_words(n):
    """uint32 words of a selection mask over n elements (ceil(n / 32)); held as int32 tensors."""
    return int(_lib.lib().dpz_mask_words(int(n)))


def topk_encode_sliced(x, k, sel_mask, planes=None, x0=None, acc=None, acc_mode=DPZ_ACC_NONE,
                       vals_src=None, idx_out=None, val_out=None, workspace=None, exact=False,
                       status_out=None, shared=False, val_fp16=False, hint=False):
    """The selection of :func:`topk_encode` with its bookkeeping in coalesced form
    (dpz_topk_encode_sliced; reference Wavelet.py:194-197): ``planes`` (int32[32 * mask_words(n)],
    the bit-sliced shared_parameters_counter, or None) += 1 at the selected indices, and
    ``sel_mask`` (int32[mask_words(n)]) gets the selected bits — the accumulator rewind is left
    to the caller's next accumulating pass (``wavedec(..., rewind_mask=sel_mask)``) or
    :func:`rewind_apply`.  ``acc`` (DPZ_ACC_ADD) is only read.  Blocking unless ``status_out``
    (then asynchronous: a nonzero status means re-run with ``exact=True``).  ``hint``: the key
    window from the previous encode on ``workspace`` (as :func:`topk_encode`; a blocking call
    that misses re-runs the sampled path, then the exact one)."""
    _require(x, torch.float32, "x")
    _require(x0, torch.float32, "x0")
    _require(acc, torch.float32, "acc")
    _require(sel_mask, torch.int32, "sel_mask")
    _require(planes, torch.int32, "planes")
    n = x.numel()
    k = int(k)
    nw = mask_words(n)
    if sel_mask.numel() < nw or (planes is not None and planes.numel() < 32 * nw):
        raise ValueError("sel_mask / planes too small for n")
    if vals_src is None:
        vals_src = x
    _require(vals_src, torch.float32, "vals_src")
    if idx_out is None:
        idx_out = torch.empty(k, dtype=torch.int32, device=x.device)
    vdt = torch.float16 if val_fp16 else torch.float32
    if val_out is None:
        val_out = torch.empty(k, dtype=vdt, device=x.device)
    _require(val_out, vdt, "val_out")
    _require(status_out, torch.int32, "status_out")
    wso = workspace or Workspace(x.device)
    ws = wso.get(n, k)
    flags = ((DPZ_TOPK_EXACT if exact else 0) | (_lib.DPZ_TOPK_SHARED if shared else 0)
             | (_lib.DPZ_TOPK_VAL_FP16 if val_fp16 else 0))
    # the device checks the prior's signature itself; this only avoids a predictable miss
    hkey = (n, k, bool(shared), int(acc_mode), x0 is not None)
    if hint and not exact and wso.hint_key == hkey:
        flags |= _lib.DPZ_TOPK_HINT
    wso.hint_key = None if exact else hkey
    rc = _lib.lib().dpz_topk_encode_sliced(
        _ptr(x), _ptr(x0), _ptr(acc), int(acc_mode), _ptr(vals_src), n, k, _ptr(idx_out),
        _ptr(val_out), _ptr(planes), _ptr(sel_mask), _ptr(ws), ws.numel(), _ptr(status_out),
        flags, _stream(x.device))
    check(rc, "dpz_topk_encode_sliced")
    return idx_out, val_out


def counter_unslice(planes, n, out=None):
    """int32[n] counter from its bit planes (dpz_counter_unslice)."""
    _require(planes, torch.int32, "planes")
    if out is None:
        out = torch.empty(int(n), dtype=torch.int32, device=planes.device)
    _require(out, torch.int32, "out")
    if planes.numel() < 32 * mask_words(n) or out.numel() < int(n):
        raise ValueError("counter_unslice: size mismatch")
    check(_lib.lib().dpz_counter_unslice(_ptr(planes), int(n), _ptr(out), _stream(out.device)),
          "dpz_counter_unslice")
    return out


def counter_slice(counter, planes=None):
    """Bit planes (int32[32 * mask_words(n)]) of an int32 counter (dpz_counter_slice)."""
    _require(counter, torch.int32, "counter")
    n = counter.numel()
    if planes is None:
        planes = torch.empty(32 * mask_words(n), dtype=torch.int32, device=counter.device)
    _require(planes, torch.int32, "planes")
    if planes.numel() < 32 * mask_words(n):
        raise ValueError("counter_slice: planes too small")
    check(_lib.lib().dpz_counter_slice(_ptr(counter), n, _ptr(planes), _stream(counter.device)),
          "dpz_counter_slice")
    return planes


def counter_flush(counter, ring, seg_off, mode=_lib.DPZ_COUNTER_AUTO, workspace=None):
    """``counter[ring[j]] += 1`` for every entry of the ring's segments (dpz_counter_flush):
    ``seg_off`` (host ints, seg_off[0] = 0) delimits segments of strictly ascending indices, one
    per round's payload (reference PartialModel.py:205-207, applied on read).  ``workspace``: a
    device uint8 tensor kept by the caller (grown here when too small)."""
    _require(counter, torch.int32, "counter")
    _require(ring, torch.int32, "ring")
    m = len(seg_off) - 1
    if m < 1:
        return counter
    if int(seg_off[-1]) > ring.numel():
        raise ValueError("counter_flush: segments past the ring")
    need = int(_lib.lib().dpz_counter_flush_workspace_bytes(counter.numel()))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=counter.device)
    offs = (ctypes.c_int64 * (m + 1))(*[int(v) for v in seg_off])
    check(_lib.lib().dpz_counter_flush(_ptr(counter), counter.numel(), _ptr(ring), offs, m,
                                       int(mode), _ptr(workspace), workspace.numel(),
                                       _stream(counter.device)), "dpz_counter_flush")
    return counter


def counter_flush_batch(items, mode=_lib.DPZ_COUNTER_AUTO):
    """:func:`counter_flush` of several counters on the current stream in one native call
    (dpz_counter_flush_batch): ``items`` holds ``(counter, ring, seg_off, workspace)`` per
    counter, the counters distinct and each with a workspace of its own (``None``: allocated
    here).  The counters that take a tiled form share one bounds and one tile launch."""
    tab, keep = [], []
    for counter, ring, seg_off, workspace in items:
        _require(counter, torch.int32, "counter")
        _require(ring, torch.int32, "ring")
        m = len(seg_off) - 1
        if m < 1:
            continue
        if int(seg_off[-1]) > ring.numel():
            raise ValueError("counter_flush_batch: segments past the ring")
        need = int(_lib.lib().dpz_counter_flush_workspace_bytes(counter.numel()))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(need, dtype=torch.uint8, device=counter.device)
        offs = (ctypes.c_int64 * (m + 1))(*[int(v) for v in seg_off])
        keep.append((offs, workspace))
        tab.append(_lib.CounterItem(counter.data_ptr(), counter.numel(), ring.data_ptr(), offs, m,
                                    workspace.data_ptr(), workspace.numel()))
    if not tab:
        return
    arr = (_lib.CounterItem * len(tab))(*tab)
    check(_lib.lib().dpz_counter_flush_batch(arr, len(tab), int(mode),
                                             _stream(items[0][0].device)),
          "dpz_counter_flush_batch")


def rewind_apply(acc, sel_mask):
    """acc[i] = 0 where sel_mask has bit i (the deferred rewind on its own, dpz_rewind_apply)."""
    _require(acc, torch.float32, "acc")
    _require(sel_mask, torch.int32, "sel_mask")
    if sel_mask.numel() < mask_words(acc.numel()):
        raise ValueError("rewind_apply: mask too small")
    check(_lib.lib().dpz_rewind_apply(_ptr(acc), _ptr(sel_mask), acc.numel(), _stream(acc.device)),
          "dpz_rewind_apply")
    return acc


def topk_complete(x, k, idx_out, val_out, workspace, x0=None, acc=None, acc_mode=DPZ_ACC_NONE,
                  vals_src=None, counter=None):
    """Finish an asynchronous encode; returns True if the exact fallback had to run."""
    n = x.numel()
    if vals_src is None:
        vals_src = x
    ws = workspace.get(n, k)
    fb = ctypes.c_int(0)
    rc = _lib.lib().dpz_topk_complete(_ptr(x), _ptr(x0), _ptr(acc), int(acc_mode), _ptr(vals_src),
                                      n, int(k), _ptr(idx_out), _ptr(val_out), _ptr(counter),
                                      _ptr(ws), ws.numel(), ctypes.byref(fb), _stream(x.device))
    check(rc, "dpz_topk_complete")
    return bool(fb.value)


def topk_status(workspace):
    """Status word of the last sampled encode in ``workspace`` (0 = ok, else the exact path ran or
    must run).  Synchronises with the device."""
    if workspace.buf is None:
        return 0
    return int(workspace.buf[8:12].view(torch.int32).item())


def topk_sticky_status(workspace, clear=False):
    """OR of the final status of every sampled-path encode on ``workspace`` since the last clear
    (0 = all final).  Synchronises the current stream (dpz_topk_sticky_status)."""
    if workspace.buf is None:
        return 0
    torch.cuda.synchronize(workspace.device)  # encodes may be pending on other streams
    v = ctypes.c_int32(0)
    rc = _lib.lib().dpz_topk_sticky_status(_ptr(workspace.buf), workspace.buf.numel(),
                                           1 if clear else 0, ctypes.byref(v),
                                           _stream(workspace.device))
    check(rc, "dpz_topk_sticky_status")
    return int(v.value)


class NodeStepBatch:
    """A prepared native enqueue of m node codec steps (dpz_encode_replace_batch): node j encodes
    ``nodes[j]["x"]`` (change vs ``x0``, counter update) into its payload ``idx``/``val`` and
    replace-decodes ``decode_src(j)``'s payload over its current model ``x`` into ``out`` (the
    reference's deserialized_model starts from the receiver's state_dict, PartialModel.py:278-295;
    with ``decode_src(j) != j`` the encoder's filter writes the copy of ``x``), on
    ``streams[j % len(streams)]`` with that stream's workspace.  The pointer arrays are built
    once; :meth:`run` is one ctypes call whatever m is (the host loop is native).  Where every
    step of a run is the fused step (a neighbour's payload over the model being encoded, sampled
    path), the steps of a stream are pipelined (dpz_encode_replace_batch_ws): they rotate
    through the stream's workspace and two internal ones (``pipe_workspaces``), and a step's
    selection tail rides in the next steps' filter launches; ``pipelined`` holds the number of
    steps of the last run that took that schedule.  Which encode every workspace last held is
    recorded on the host, so a step takes the prior window (DPZ_BATCH_HINT) only where its
    workspace holds one."""

    def __init__(self, nodes, n, k, streams, workspaces, decode_src=None, rings=None):
        """``rings``: one :class:`~decentralizepy_amd._device.RingCounter` per node (over its
        ``counter``): the encodes then update no counter and write their payload indices into
        the node's ring slot, as the PartialModel plugin does; the rings are flushed when full
        and by :meth:`flush_rings` (ordered on each node's stream)."""
        m = len(nodes)
        self.m, self.n, self.k = m, int(n), int(k)
        for d in nodes:
            for key in ("x", "x0", "out"):
                _require(d[key], torch.float32, key)
                if d[key].numel() != n:
                    raise ValueError(f"node tensor {key} must hold n elements")
            _require(d["idx"], torch.int32, "idx")
            _require(d["val"], torch.float32, "val")
            _require(d.get("counter"), torch.int32, "counter")
            if d["idx"].numel() != k or d["val"].numel() != k:
                raise ValueError("payload buffers must hold k entries")
        src = decode_src or (lambda j: j)
        P = ctypes.c_void_p * max(m, 1)
        self._x = P(*[d["x"].data_ptr() for d in nodes])
        self._x0 = P(*[d["x0"].data_ptr() for d in nodes])
        self._cnt = P(*[(d["counter"].data_ptr() if d.get("counter") is not None else 0)
                        for d in nodes])
        self._idx = P(*[d["idx"].data_ptr() for d in nodes])
        self._val = P(*[d["val"].data_ptr() for d in nodes])
        self._rl = P(*[d["x"].data_ptr() for d in nodes])
        self._ri = P(*[nodes[src(j)]["idx"].data_ptr() for j in range(m)])
        self._rv = P(*[nodes[src(j)]["val"].data_ptr() for j in range(m)])
        self._ro = P(*[d["out"].data_ptr() for d in nodes])
        S = len(streams)
        if len(workspaces) != S:
            raise ValueError("one workspace per stream")
        wbufs = [w.get(n, k) for w in workspaces]
        dbufs = [w.get_decode(n, 1) for w in workspaces]
        Q = ctypes.c_void_p * S
        self._ws = Q(*[b.data_ptr() for b in wbufs])
        self._dws = Q(*[b.data_ptr() for b in dbufs])
        self._ws_bytes = min(b.numel() for b in wbufs)
        self._dws_bytes = min(b.numel() for b in dbufs)
        self._streams = Q(*[s.cuda_stream for s in streams])
        self._S = S
        self.workspaces = workspaces
        # the pipelined schedule (dpz_encode_replace_batch_ws): two more workspaces per stream,
        # and the host record of which encode every workspace last held (the hint bookkeeping)
        self.pipe_workspaces = [Workspace(workspaces[0].device) for _ in range(2 * S)]
        pbufs = [w.get(n, k) for w in self.pipe_workspaces]
        self._ws_pipe = (ctypes.c_void_p * (2 * S))(*[b.data_ptr() for b in pbufs])
        self._ws_bytes = min([self._ws_bytes] + [b.numel() for b in pbufs])
        self._ws_sig = (ctypes.c_uint32 * (3 * S))()
        self.pipelined = 0  # steps of the last run that took the pipelined schedule
        self._keep = (nodes, wbufs, dbufs, streams, pbufs)
        self._rings = rings
        if rings is not None:
            if len(rings) != m:
                raise ValueError("one ring per node")
            self._src = [src(j) for j in range(m)]
            self._tstreams = list(streams)
            self._cnt = P(*([0] * m))  # no counter update in the encodes
            # the last committed payload of every node (its own buffer until the first encode)
            self._last = [d["idx"].data_ptr() for d in nodes]

    def _ring_slot(self, j):
        """Node j's next ring slot; a full ring is flushed first, on node j's stream."""
        r = self._rings[j]
        if r.ring is None or r.segs[-1] + self.k > r.ring.numel() or len(r.segs) > r.MAX_SEGS:
            with torch.cuda.stream(self._tstreams[j % self._S]):
                return r.slot(self.k)
        return r.slot(self.k)

    def flush_rings(self):
        """Every node's deferred counter updates into its counter, on its stream: the nodes of a
        stream in one batched flush."""
        if self._rings is None:
            return
        from ._device import RingCounter
        for s in range(self._S):  # one native call per stream (dpz_counter_flush_batch)
            mine = [r for r in self._rings[s::self._S] if r.pending_rounds()]
            if mine:
                with torch.cuda.stream(self._tstreams[s]):
                    RingCounter.flush_many(mine)

    def run(self, what=_lib.DPZ_BATCH_ENCODE | _lib.DPZ_BATCH_DECODE, m=None):
        """``what`` with DPZ_BATCH_HINT: the encodes take the prior window (DPZ_TOPK_HINT) —
        after this batch's first encoding run every encode, the first on each stream too."""
        m = self.m if m is None else int(m)
        if what & _lib.DPZ_BATCH_HINT and what & _lib.DPZ_BATCH_ENCODE:
            if getattr(self, "_primed", False):
                what = (what & ~_lib.DPZ_BATCH_HINT) | _lib.DPZ_BATCH_HINT_ALL
            self._primed = True
        idx, ri = self._idx, self._ri
        enc = bool(what & _lib.DPZ_BATCH_ENCODE)
        if self._rings is not None:
            P = ctypes.c_void_p * max(self.m, 1)
            new = [self._ring_slot(j).data_ptr() if enc else self._last[j] for j in range(m)]
            idx = P(*(new + [0] * (self.m - m)))
            # a payload encoded earlier in this run (src < j, same stream) is the new slot
            ri = P(*([(new[q] if (enc and q < j) else self._last[q])
                      for j, q in ((j, self._src[j]) for j in range(m))] + [0] * (self.m - m)))
        piped = ctypes.c_int(0)
        rc = _lib.lib().dpz_encode_replace_batch_ws(
            m, int(what), self._x, self._x0, self.n, self.k, self._cnt, idx, self._val,
            self._rl, ri, self._rv, self.k, self._ro, self._ws, self._ws_bytes, self._dws,
            self._dws_bytes, self._S, self._streams, self._ws_pipe, self._ws_sig,
            ctypes.byref(piped))
        check(rc, "dpz_encode_replace_batch_ws")
        self.pipelined = int(piped.value)
        if self._rings is not None and enc:
            for j in range(m):
                self._rings[j].commit(self.k)
                self._last[j] = new[j]

    def last_idx(self, j):
        """Node j's payload indices as this batch encoded them last: its ``idx`` buffer, or with
        ``rings`` the ring slot they were written into (a flush leaves the slot's content)."""
        nodes = self._keep[0]
        ring = self._rings[j].ring if self._rings is not None else None
        if ring is None or self._last[j] == nodes[j]["idx"].data_ptr():
            return nodes[j]["idx"]
        off = (self._last[j] - ring.data_ptr()) // ring.element_size()
        return ring[off:off + self.k]

    def sticky_status(self, clear=False):
        """OR of every encode's final status on these workspaces since the last clear."""
        v = 0
        for w in list(self.workspaces) + self.pipe_workspaces:
            v |= topk_sticky_status(w, clear)
        return v


def decode_average(local, payloads, weights=None, w_self=None, out=None, replace_only=False,
                   workspace=None, zero_base=False, add_only=False, accumulate=False,
                   also_local=False, base_ready=False):
    """Batched replace + Metro-Hastings fold (reference Sharing.py:156-229, PartialModel.py:257-303).

    payloads : list of ``(idx int32 device tensor or None, vals fp32 device tensor)``
    weights  : per-payload weights (Python floats, rounded to fp32 like torch does)
    w_self   : weight of the local term, or None for no self term (server variant)
    zero_base: sparse payloads are zero off their indices (STC's ``T = zeros; T[idx] = params``)
               and the fold starts from +0.0 (DPZ_FOLD_ZERO_BASE)
    add_only : one payload, ``out = local + T`` with T zero-based (DPZ_FOLD_ADD_ONLY)
    accumulate: ``out`` holds a running total the fold continues (DPZ_FOLD_ACCUMULATE)
    also_local: the result is also written over ``local`` in place (DPZ_FOLD_ALSO_LOCAL)
    base_ready: ``out`` already holds this fold's no-hit base over ``local`` (written by
               ``topk_encode(..., fold_base=(out, weights, w_self))``): only the elements the
               payloads hit are rewritten (DPZ_FOLD_BASE_READY)
    """
    _require(local, torch.float32, "local")
    n = local.numel()
    if out is None:
        out = torch.empty_like(local)
    _require(out, torch.float32, "out")
    npay = len(payloads)
    idx_arr = (ctypes.c_void_p * max(npay, 1))()
    val_arr = (ctypes.c_void_p * max(npay, 1))()
    k_arr = (ctypes.c_int64 * max(npay, 1))()
    w_arr = (ctypes.c_float * max(npay, 1))()
    for i, (idx, vals) in enumerate(payloads):
        _require(idx, torch.int32, "idx")
        _require(vals, torch.float32, "vals")
        if idx is not None and idx.numel() != vals.numel():
            raise ValueError("payload idx and vals differ in length")
        if idx is None and vals.numel() != n:
            raise ValueError("a dense payload (idx=None) must hold n values")
        idx_arr[i] = idx.data_ptr() if idx is not None else None
        val_arr[i] = vals.data_ptr()
        k_arr[i] = vals.numel()
        w_arr[i] = float(weights[i]) if weights is not None else 1.0
    flags = ((DPZ_FOLD_SELF if w_self is not None else 0)
             | (DPZ_FOLD_REPLACE_ONLY if replace_only else 0)
             | (_lib.DPZ_FOLD_ZERO_BASE if zero_base else 0)
             | (_lib.DPZ_FOLD_ADD_ONLY if add_only else 0)
             | (_lib.DPZ_FOLD_ACCUMULATE if accumulate else 0)
             | (_lib.DPZ_FOLD_ALSO_LOCAL if also_local else 0)
             | (_lib.DPZ_FOLD_BASE_READY if base_ready else 0))
    ws = (workspace or Workspace(local.device)).get_decode(n, npay)
    rc = _lib.lib().dpz_decode_average(_ptr(local), n, npay, idx_arr, val_arr, k_arr, w_arr,
                                       float(w_self) if w_self is not None else 0.0, flags,
                                       _ptr(out), _ptr(ws), ws.numel(), _stream(local.device))
    check(rc, "dpz_decode_average")
    return out


def topk_threshold(x, k, workspace=None, cap=None):
    """Choco's threshold selection (reference sharing/Choco.py:117-161): every element with
    ``|x| >= T`` (T = the k-th largest |x|, all ties kept; 0 when k == 0) that is nonzero, in
    ascending index order.  Returns ``(idx int32[c], vals fp32[c])`` (blocks for the count)."""
    _require(x, torch.float32, "x")
    n = x.numel()
    cap = n if cap is None else int(cap)
    idx = torch.empty(max(cap, 1), dtype=torch.int32, device=x.device)
    val = torch.empty(max(cap, 1), dtype=torch.float32, device=x.device)
    ws = (workspace or Workspace(x.device)).get(n, int(k))
    cnt = ctypes.c_int64(0)
    rc = _lib.lib().dpz_topk_threshold(_ptr(x), n, int(k), _ptr(idx), _ptr(val), cap, _ptr(ws),
                                       ws.numel(), ctypes.byref(cnt), _stream(x.device))
    check(rc, "dpz_topk_threshold")
    c = int(cnt.value)
    return idx[:c], val[:c]


def mask_below_threshold(x, workspace, out=None):
    """``x[|x| < T] = 0`` with T of the last :func:`topk_threshold` on ``workspace``."""
    _require(x, torch.float32, "x")
    out = x if out is None else out
    rc = _lib.lib().dpz_mask_below_threshold(_ptr(x), x.numel(), _ptr(workspace.buf), _ptr(out),
                                             _stream(x.device))
    check(rc, "dpz_mask_below_threshold")
    return out


def elementwise(op, a, b, d=None, c=0.0, out=None):
    """fp32 elementwise helpers of the Choco update (DPZ_EW_SUB / ADD / CHOCO)."""
    for t, nm in ((a, "a"), (b, "b"), (d, "d")):
        _require(t, torch.float32, nm)
    if out is None:
        out = torch.empty_like(a)
    rc = _lib.lib().dpz_elementwise(int(op), _ptr(a), _ptr(b), _ptr(d), float(c), a.numel(),
                                    _ptr(out), _stream(a.device))
    check(rc, "dpz_elementwise")
    return out


def replace(local, idx, vals, out=None, workspace=None):
    """``T = local.clone(); T[idx] = vals`` (reference PartialModel.py:292-295)."""
    return decode_average(local, [(idx, vals)], out=out, replace_only=True, workspace=workspace)


WAVELETS = ("sym2", "haar")  # the fused kernels (dpz_dwt.hip, dpz_haar.hip)
_BANKS = None
_BANK_DEV = {}


def _bank_table():
    """pywt's fp32 filter banks (decentralizepy_amd/wavelet_filters.json, generated from
    PyWavelets 1.1.1 by tools/gen_wavelet_filters.py)."""
    global _BANKS
    if _BANKS is None:
        import json
        import os
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)),
                               "wavelet_filters.json")) as f:
            _BANKS = json.load(f)["wavelets"]
    return _BANKS


def wavelet_names():
    """Every wavelet the device kernels implement: sym2 / haar (fused kernels) and every other
    pywt discrete wavelet with an even filter length <= 64 (dpz_dwt_generic)."""
    return sorted(set(WAVELETS) | set(_bank_table()))


def filter_len(wavelet):
    _check_wavelet(wavelet)
    return {"sym2": 4, "haar": 2}.get(wavelet) or len(_bank_table()[wavelet][0])


def _check_wavelet(wavelet):
    if wavelet not in WAVELETS and wavelet not in _bank_table():
        raise NotImplementedError(
            f"wavelet '{wavelet}': the device kernels implement sym2, haar and the pywt discrete "
            f"wavelets with filter length <= 64 ({len(_bank_table())} names, wavelet_names())")


def _fused(wavelet, level):
    """sym2 to level 4 and haar to level 8 run the fused kernels; every other (wavelet, level)
    the generic-filter path."""
    return (wavelet == "sym2" and int(level) <= 4) or (wavelet == "haar" and int(level) <= 8)


def _bank(wavelet, device):
    """The filter bank in device memory: dec_lo, dec_hi, rec_lo, rec_hi (4F fp32)."""
    key = (wavelet, str(device))
    t = _BANK_DEV.get(key)
    if t is None:
        b = np.concatenate([np.array(v, dtype=np.uint32) for v in _bank_table()[wavelet]])
        t = torch.from_numpy(b.view(np.float32).copy()).to(device)
        _BANK_DEV[key] = t
    return t


def _generic_ws(n, level, wavelet, device):
    nb = int(_lib.lib().dpz_wavelet_generic_workspace_bytes(int(n), int(level),
                                                            filter_len(wavelet)))
    return torch.empty(max(1, (nb + 3) // 4), dtype=torch.float32, device=device), nb


def wavedec_len(n, level=4, wavelet="sym2"):
    _check_wavelet(wavelet)
    if _fused(wavelet, level):
        fn = _lib.lib().dpz_wavedec_len if wavelet == "sym2" else _lib.lib().dpz_haar_wavedec_len
        m = int(fn(int(n), int(level)))
    else:
        m = int(_lib.lib().dpz_wavedec_len_generic(int(n), int(level), filter_len(wavelet)))
    if m < 0:
        # a level whose input is shorter than the filter (pywt's multi-reflection branch) or a
        # level past the kernels' 8: not implemented on the device (Wavelet's documented error)
        raise NotImplementedError(f"{wavelet} level-{level} wavedec unsupported for n={n}")
    return m


def wavedec(x, level=4, x0=None, want_x=True, coeffs_x=None, coeffs_diff=None, accumulate=False,
            wavelet="sym2", rewind_mask=None):
    """Multilevel DWT (mode "symmetric"; ``wavelet`` "sym2" / "haar" on the fused kernels, any
    other name of :func:`wavelet_names` on dpz_dwt_generic) as one ``coeffs_to_array`` vector
    (reference Wavelet.py:12-32).

    Returns ``(W(x) or None, W(x - x0) or None)``; with ``accumulate=True`` adds W(x - x0) into
    ``coeffs_diff`` instead of overwriting it.  ``rewind_mask`` (with ``accumulate``, no W(x)): the
    selection mask of :func:`topk_encode_sliced` — the deferred rewind is applied first,
    ``acc = (selected ? 0 : acc) + W(x - x0)`` (dpz_dwt_sym2_rewind / dpz_dwt_haar_rewind).
    """
    if rewind_mask is not None:
        if not accumulate or want_x or coeffs_diff is None or x0 is None:
            raise ValueError("rewind_mask: an accumulating W(x - x0) pass into coeffs_diff only")
        _require(x, torch.float32, "x")
        _require(x0, torch.float32, "x0")
        _require(coeffs_diff, torch.float32, "coeffs_diff")
        _require(rewind_mask, torch.int32, "rewind_mask")
        n = x.numel()
        m = wavedec_len(n, level, wavelet)
        if coeffs_diff.numel() != m or x0.numel() != n or rewind_mask.numel() < mask_words(m):
            raise ValueError("rewind_mask: size mismatch")
        if not _fused(wavelet, level):
            ws, nb = _generic_ws(n, level, wavelet, x.device)
            rc = _lib.lib().dpz_dwt_generic(
                _ptr(x), _ptr(x0), n, int(level), _ptr(_bank(wavelet, x.device)),
                filter_len(wavelet), None, _ptr(coeffs_diff), 1, _ptr(rewind_mask), _ptr(ws), nb,
                _stream(x.device))
            check(rc, f"dpz_dwt_generic({wavelet})")
            return None, coeffs_diff
        fn = (_lib.lib().dpz_dwt_sym2_rewind if wavelet == "sym2"
              else _lib.lib().dpz_dwt_haar_rewind)
        rc = fn(_ptr(x), _ptr(x0), n, int(level), _ptr(coeffs_diff), _ptr(rewind_mask),
                _stream(x.device))
        check(rc, f"dpz_dwt_{wavelet}_rewind")
        return None, coeffs_diff
    _require(x, torch.float32, "x")
    _require(x0, torch.float32, "x0")
    n = x.numel()
    m = wavedec_len(n, level, wavelet)
    if want_x and coeffs_x is None:
        coeffs_x = torch.empty(m, dtype=torch.float32, device=x.device)
    if x0 is not None and coeffs_diff is None:
        if accumulate:
            raise ValueError("accumulate needs coeffs_diff")
        coeffs_diff = torch.empty(m, dtype=torch.float32, device=x.device)
    for t, nm in ((coeffs_x if want_x else None, "coeffs_x"),
                  (coeffs_diff if x0 is not None else None, "coeffs_diff")):
        _require(t, torch.float32, nm)
        if t is not None and t.numel() != m:
            raise ValueError(f"{nm} must hold wavedec_len(n, level) = {m} values")
    if x0 is not None and x0.numel() != n:
        raise ValueError("x0 must match x")
    if not _fused(wavelet, level):
        ws, nb = _generic_ws(n, level, wavelet, x.device)
        rc = _lib.lib().dpz_dwt_generic(
            _ptr(x), _ptr(x0), n, int(level), _ptr(_bank(wavelet, x.device)), filter_len(wavelet),
            _ptr(coeffs_x if want_x else None), _ptr(coeffs_diff if x0 is not None else None),
            1 if accumulate else 0, None, _ptr(ws), nb, _stream(x.device))
        check(rc, f"dpz_dwt_generic({wavelet})")
    else:
        fn = _lib.lib().dpz_dwt_sym2 if wavelet == "sym2" else _lib.lib().dpz_dwt_haar
        rc = fn(_ptr(x), _ptr(x0), n, int(level), _ptr(coeffs_x if want_x else None),
                _ptr(coeffs_diff if x0 is not None else None), 1 if accumulate else 0,
                _stream(x.device))
        check(rc, f"dpz_dwt_{wavelet}")
    return (coeffs_x if want_x else None), (coeffs_diff if x0 is not None else None)


def waverec(coeffs, n, level=4, out=None, wavelet="sym2"):
    """Multilevel IDWT (any wavelet of :func:`wavelet_names`), first n outputs (reference
    Wavelet.py:311-316)."""
    _require(coeffs, torch.float32, "coeffs")
    if coeffs.numel() != wavedec_len(n, level, wavelet):
        raise ValueError("coeffs must hold wavedec_len(n, level) values")
    if out is None:
        out = torch.empty(int(n), dtype=torch.float32, device=coeffs.device)
    _require(out, torch.float32, "out")
    if out.numel() < int(n):
        raise ValueError("out must hold n values")
    if not _fused(wavelet, level):
        ws, nb = _generic_ws(n, level, wavelet, coeffs.device)
        rc = _lib.lib().dpz_idwt_generic(_ptr(coeffs), int(n), int(level),
                                         _ptr(_bank(wavelet, coeffs.device)), filter_len(wavelet),
                                         _ptr(out), _ptr(ws), nb, _stream(coeffs.device))
        check(rc, f"dpz_idwt_generic({wavelet})")
        return out
    fn = _lib.lib().dpz_idwt_sym2 if wavelet == "sym2" else _lib.lib().dpz_idwt_haar
    rc = fn(_ptr(coeffs), int(n), int(level), _ptr(out), _stream(coeffs.device))
    check(rc, f"dpz_idwt_{wavelet}")
    return out


def scatter_fill(dst, idx, value):
    """``dst[idx] = value`` (reference models/Model.py:53-64 rewind_accumulation)."""
    _require(dst, torch.float32, "dst")
    _require(idx, torch.int32, "idx")
    rc = _lib.lib().dpz_scatter_fill(_ptr(dst), dst.numel(), _ptr(idx), idx.numel(), float(value),
                                     _stream(dst.device))
    check(rc, "dpz_scatter_fill")
    return dst


def pack_fp16(x, out=None):
    _require(x, torch.float32, "x")
    if out is None:
        out = torch.empty(x.numel(), dtype=torch.float16, device=x.device)
    rc = _lib.lib().dpz_pack_fp16(_ptr(x), x.numel(), _ptr(out), _stream(x.device))
    check(rc, "dpz_pack_fp16")
    return out


def unpack_fp16(h, out=None):
    _require(h, torch.float16, "h")
    if out is None:
        out = torch.empty(h.numel(), dtype=torch.float32, device=h.device)
    rc = _lib.lib().dpz_unpack_fp16(_ptr(h), h.numel(), _ptr(out), _stream(h.device))
    check(rc, "dpz_unpack_fp16")
    return out


def elias_encode(idx, out=None, workspace=None):
    """Elias-gamma stream of a strictly increasing device int32 index array (k >= 2).

    Returns a device uint8 view of exactly the reference's byte count (compression/Elias.py:20-52).
    """
    _require(idx, torch.int32, "idx")
    k = idx.numel()
    if k < 2:
        raise IndexError("Elias coding needs at least two indices (reference Elias.py:38-46)")
    cap = int(_lib.lib().dpz_elias_max_bytes(k))
    if out is None or out.numel() < cap:
        out = torch.empty(cap, dtype=torch.uint8, device=idx.device)
    workspace = workspace or Workspace(idx.device)
    ws = workspace.get_elias(k, 0)
    nbytes = ctypes.c_int64(0)
    rc = _lib.lib().dpz_elias_encode(_ptr(idx), k, _ptr(out), out.numel(), ctypes.byref(nbytes),
                                     _ptr(ws), ws.numel(), _stream(idx.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("Elias coding needs strictly increasing indices")
    check(rc, "dpz_elias_encode")
    return out[:nbytes.value]


def elias_decode(buf, nbytes, nbits, first, count, dtype=torch.int64, workspace=None):
    """Values of an Elias-gamma stream held on the device (compression/Elias.py:54-97).

    ``buf`` is a device uint8 tensor with at least round_up(nbytes, 4) + 16 bytes; ``nbits`` and
    ``first`` come from the stream's trailer; ``count`` bounds the output (the stream encodes at
    most (nbits - 128) + 1 values).

    A stream may hold at most 2^26 code bits (``nbits <= 2**26 + 128``).  A longer one raises
    CodecError ("unsupported size or configuration") before anything is launched, here and in
    ``elias_decode_async``.  ``elias_encode`` has no such limit, so it can write a stream that
    these decoders refuse.
    """
    _require(buf, torch.uint8, "buf")
    if buf.numel() < ((nbytes + 3) // 4) * 4 + 16:
        raise ValueError("buf must be padded to round_up(nbytes, 4) + 16 bytes")
    out = torch.empty(max(count, 1), dtype=dtype, device=buf.device)
    workspace = workspace or Workspace(buf.device)
    ws = workspace.get_elias(2, nbytes)
    n = ctypes.c_int64(0)
    o64 = out if dtype == torch.int64 else None
    o32 = out if dtype == torch.int32 else None
    if o64 is None and o32 is None:
        raise ValueError("dtype must be torch.int64 or torch.int32")
    rc = _lib.lib().dpz_elias_decode(_ptr(buf), nbytes, nbits, first, _ptr(o64), _ptr(o32),
                                     out.numel(), ctypes.byref(n), _ptr(ws), ws.numel(),
                                     _stream(buf.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed Elias stream")
    check(rc, "dpz_elias_decode")
    return out[:n.value]


def elias_decode_async(buf, nbytes, nbits, first, count, status, dtype=torch.int32,
                       workspace=None):
    """``elias_decode`` with no host synchronisation: the caller knows the value count (the
    payload's other leg) and passes a device int32 status word, OR-ed nonzero on the stream when
    the stream is malformed or holds a different count (the values are then unspecified).  Read
    the status once, after the round's folds (PartialModel.decompress_data's device path)."""
    _require(buf, torch.uint8, "buf")
    _require(status, torch.int32, "status")
    if buf.numel() < ((nbytes + 3) // 4) * 4 + 16:
        raise ValueError("buf must be padded to round_up(nbytes, 4) + 16 bytes")
    if count < 1:
        raise ValueError("count must be >= 1")
    if dtype not in (torch.int64, torch.int32):
        raise ValueError("dtype must be torch.int64 or torch.int32")
    out = torch.empty(count, dtype=dtype, device=buf.device)
    workspace = workspace or Workspace(buf.device)
    ws = workspace.get_elias(2, nbytes)
    o64 = out if dtype == torch.int64 else None
    o32 = out if dtype == torch.int32 else None
    rc = _lib.lib().dpz_elias_decode_async(_ptr(buf), nbytes, nbits, first, _ptr(o64), _ptr(o32),
                                           count, _ptr(status), _ptr(ws), ws.numel(),
                                           _stream(buf.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed Elias stream")
    check(rc, "dpz_elias_decode_async")
    return out


def fpz_encode(x, precision=0, out=None, workspace=None):
    """Block-floating stream of a device fp32 vector (csrc/dpz_fpz.hip; the float leg of
    compression/EliasFpzip.py:19-51 at precision 0 and EliasFpzipLossy.py:14-58 at precision p).
    Returns a device uint8 view of exactly the stream's bytes.

    ``precision`` 0 or >= 32 is lossless; 1..31 keeps the top ``precision`` bits of every bit
    pattern (1..9: sign and leading exponent bits only, no mantissa); a negative precision raises
    ValueError."""
    _require(x, torch.float32, "x")
    n = x.numel()
    cap = int(_lib.lib().dpz_fpz_max_bytes(n))
    if out is None or out.numel() < cap:
        out = torch.empty(cap, dtype=torch.uint8, device=x.device)
    need = int(_lib.lib().dpz_fpz_workspace_bytes(n))
    workspace = workspace or Workspace(x.device)
    if workspace.ebuf is None or workspace.ebuf.numel() < need:
        workspace.ebuf = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
    ws = workspace.ebuf
    nbytes = ctypes.c_int64(0)
    rc = _lib.lib().dpz_fpz_encode(_ptr(x), n, int(precision), _ptr(out), out.numel(),
                                   ctypes.byref(nbytes), _ptr(ws), ws.numel(), _stream(x.device))
    if rc == _lib.DPZ_ERR_UNSUPPORTED:
        raise ValueError("float precision must be >= 0 (0 or >= 32: lossless)")
    check(rc, "dpz_fpz_encode")
    return out[:nbytes.value]


def fpz_decode(buf, n, precision, out=None, check_status=True, status=None):
    """Values of a block-floating stream held on the device (a uint8 tensor of the whole stream,
    4-byte aligned); ``n`` and ``precision`` come from its header (any precision >= 0, as
    ``fpz_encode`` takes; a negative one raises ValueError).  With ``check_status`` the
    call synchronises and raises ValueError on a malformed stream; a caller's ``status`` (device
    int32 word) is OR-ed instead, with no synchronisation."""
    _require(buf, torch.uint8, "buf")
    if out is None:
        out = torch.empty(max(n, 1), dtype=torch.float32, device=buf.device)
    _require(out, torch.float32, "out")
    if out.numel() < n:
        raise ValueError("out holds fewer than n values")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=buf.device)
    else:
        _require(status, torch.int32, "status")
        check_status = False
    rc = _lib.lib().dpz_fpz_decode(_ptr(buf), buf.numel(), n, int(precision), _ptr(out),
                                   _ptr(status), _stream(buf.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed float stream")
    if rc == _lib.DPZ_ERR_UNSUPPORTED:
        raise ValueError("float precision must be >= 0 (0 or >= 32: lossless)")
    check(rc, "dpz_fpz_decode")
    if check_status and int(status.item()) != 0:
        raise ValueError("malformed float stream")
    return out[:n]


def _fft_ws(n, workspace, device):
    need = int(_lib.lib().dpz_fft_workspace_bytes(int(n)))
    if need < 0:
        raise ValueError(f"real FFT of n={n} unsupported (2 <= n < 2**31)")
    workspace = workspace or Workspace(device)
    buf = getattr(workspace, "fbuf", None)
    if buf is None or buf.numel() < max(need, 256):
        buf = workspace.fbuf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return buf


def _chirp_ws(n, workspace, device):
    workspace = workspace or Workspace(device)
    buf = workspace.cbuf = fft_chirp_nodes_workspace(1, n, device, getattr(workspace, "cbuf", None))
    return buf


def rfft(x, out=None, workspace=None, chirp=False):
    """``torch.fft.rfft(x)`` of a device fp32 vector (reference sharing/JWINS/FFT.py:12-25):
    the native mixed-radix kernels, or hipFFT for a size with a prime factor above 4096
    (``fft_native(n)``); returns complex64[n // 2 + 1].  ``chirp=True`` (even n >= 4) runs the
    vector as a one-job table through ``rfft_chirp_nodes`` instead."""
    _require(x, torch.float32, "x")
    n = x.numel()
    if out is None:
        out = torch.empty(n // 2 + 1, dtype=torch.complex64, device=x.device)
    _require(out, torch.complex64, "out")
    if out.numel() != n // 2 + 1:
        raise ValueError("out must hold n // 2 + 1 complex values")
    if chirp:
        rfft_chirp_nodes(FftNodesTable([x], None, [out], False, x.device), n,
                         _chirp_ws(n, workspace, x.device))
        return out
    ws = _fft_ws(n, workspace, x.device)
    rc = _lib.lib().dpz_rfft(_ptr(x), n, _ptr(out), _ptr(ws), ws.numel(), _stream(x.device))
    check(rc, "dpz_rfft")
    return out


def fft_native(n):
    """True when rfft / irfft of n reals run this build's kernels (else hipFFT)."""
    return bool(_lib.lib().dpz_fft_native(int(n)))


def irfft(coeffs, n, out=None, workspace=None, chirp=False):
    """``torch.fft.irfft(coeffs, n)`` (1/n normalisation; reference sharing/JWINS/FFT.py:301).
    ``coeffs`` (complex64[n // 2 + 1]) is overwritten.  ``chirp=True`` (even n >= 4) runs a
    one-job table through ``irfft_chirp_nodes`` instead, which only reads ``coeffs``."""
    _require(coeffs, torch.complex64, "coeffs")
    n = int(n)
    if coeffs.numel() != n // 2 + 1:
        raise ValueError("coeffs must hold n // 2 + 1 complex values")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=coeffs.device)
    _require(out, torch.float32, "out")
    if chirp:
        irfft_chirp_nodes(IfftNodesTable([coeffs], [out], coeffs.device), n,
                          _chirp_ws(n, workspace, coeffs.device))
        return out
    ws = _fft_ws(n, workspace, coeffs.device)
    rc = _lib.lib().dpz_irfft(_ptr(coeffs), n, _ptr(out), _ptr(ws), ws.numel(),
                              _stream(coeffs.device))
    check(rc, "dpz_irfft")
    return out


def cplx_key(change, acc=None, acc_mode=DPZ_ACC_NONE, out=None):
    """fp32 |change| of a complex64 change vector after the DPZ_ACC_* accumulation step
    (reference PartialModel.py:315-329 + FFT.py:143-149)."""
    _require(change, torch.complex64, "change")
    _require(acc, torch.complex64, "acc")
    m = change.numel()
    if acc is not None and acc.numel() != m:
        raise ValueError("acc must match the change length")
    if out is None:
        out = torch.empty(m, dtype=torch.float32, device=change.device)
    _require(out, torch.float32, "out")
    rc = _lib.lib().dpz_cplx_key(_ptr(change), _ptr(acc), int(acc_mode), m, _ptr(out),
                                 _stream(change.device))
    check(rc, "dpz_cplx_key")
    return out


def cplx_gather(src, idx, acc=None, out=None):
    """``src[idx]`` of a complex64 vector; zeroes ``acc[idx]`` when given (Model.py:53-64)."""
    _require(src, torch.complex64, "src")
    _require(idx, torch.int32, "idx")
    _require(acc, torch.complex64, "acc")
    if out is None:
        out = torch.empty(idx.numel(), dtype=torch.complex64, device=src.device)
    _require(out, torch.complex64, "out")
    rc = _lib.lib().dpz_cplx_gather(_ptr(src), src.numel(), _ptr(idx), idx.numel(), _ptr(out),
                                    _ptr(acc), _stream(src.device))
    check(rc, "dpz_cplx_gather")
    return out


def cplx_pair_indices(idx, out=None):
    """int32[2k] ``(2 i, 2 i + 1)`` per index: a complex payload as a payload of the float view."""
    _require(idx, torch.int32, "idx")
    k = idx.numel()
    if out is None:
        out = torch.empty(2 * k, dtype=torch.int32, device=idx.device)
    _require(out, torch.int32, "out")
    rc = _lib.lib().dpz_cplx_pair_indices(_ptr(idx), k, _ptr(out), _stream(idx.device))
    check(rc, "dpz_cplx_pair_indices")
    return out


def _lz4_ws(workspace, device, need):
    workspace = workspace or Workspace(device)
    buf = getattr(workspace, "lbuf", None)
    if buf is None or buf.numel() < max(need, 256):
        buf = workspace.lbuf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return buf


def lz4_compress(data, out=None, workspace=None):
    """LZ4 frame of a device byte tensor (csrc/dpz_lz4.hip: linked 2 KB blocks, one wave each,
    whose matches reach 14 KB back into the input; ``lz4_geometry()`` has the built figures);
    returns a device uint8 view of exactly the frame (reference Lz4Wrapper.py:20-98)."""
    _require(data, torch.uint8, "data")
    n = data.numel()
    cap = int(_lib.lib().dpz_lz4_max_bytes(n))
    if out is None or out.numel() < cap:
        out = torch.empty(cap, dtype=torch.uint8, device=data.device)
    ws = _lz4_ws(workspace, data.device, int(_lib.lib().dpz_lz4_workspace_bytes(n, 0, 0)))
    nbytes = ctypes.c_int64(0)
    rc = _lib.lib().dpz_lz4_compress(_ptr(data), n, _ptr(out), out.numel(), ctypes.byref(nbytes),
                                     _ptr(ws), ws.numel(), _stream(data.device))
    check(rc, "dpz_lz4_compress")
    return out[:nbytes.value]


def lz4_geometry():
    """The built LZ4 codec's geometry (host only, no GPU): ``blk`` encoder block bytes, ``win``
    encoder history bytes, ``par_max`` / ``par_cmax`` decoded / compressed bytes of a block the
    parallel decoder takes, ``chunk`` its walk chunk in compressed bytes."""
    g = (ctypes.c_int32 * 5)()
    check(_lib.lib().dpz_lz4_geometry(g), "dpz_lz4_geometry")
    return dict(zip(("blk", "win", "par_max", "par_cmax", "chunk"), (int(v) for v in g)))


def lz4_frame_info(frame):
    """(content_size or -1, blocks, linked, block_max) of a host frame (bytes-like)."""
    b = bytes(frame)
    cs, nb, ln, bm = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    rc = _lib.lib().dpz_lz4_frame_info(b, len(b), ctypes.byref(cs), ctypes.byref(nb),
                                       ctypes.byref(ln), ctypes.byref(bm))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed LZ4 frame")
    check(rc, "dpz_lz4_frame_info")
    return int(cs.value), int(nb.value), bool(ln.value), int(bm.value)


def lz4_decompress(frame, device, out=None, workspace=None, max_size=None):
    """Content of an LZ4 frame (host bytes-like) decoded on ``device``; returns a device uint8
    tensor.  Linked frames (python-lz4's default) and independent frames with blocks of at most
    64 KB are supported.  The frame comes from a peer, so its header is untrusted: a stored
    content size is checked against what the blocks can hold (each decodes to at most bmax
    bytes) and against ``max_size`` BEFORE anything is allocated.  Block / content xxh32
    checksums, when the frame carries them, are skipped, not verified (the transport —
    ZeroMQ over TCP — already guarantees integrity; every decoder read and write is
    bounds-checked, so a corrupt frame cannot fault or overrun)."""
    b = frame if isinstance(frame, bytes) else bytes(frame)
    cs, nb, linked, bmax = lz4_frame_info(b)
    bound = nb * bmax
    if cs > bound or (max_size is not None and cs > int(max_size)):
        raise ValueError(f"malformed LZ4 frame: content size {cs} exceeds what its {nb} "
                         f"blocks can hold ({bound} bytes) or max_size")
    if bmax > 65536 and nb > 0:  # what dpz_lz4_decompress answers, before anything is allocated
        check(_lib.DPZ_ERR_UNSUPPORTED, "dpz_lz4_decompress")
    # without a stored content size the blocks bound it
    size = cs if cs >= 0 else (min(bound, int(max_size)) if max_size is not None else bound)
    if out is None or out.numel() < size:
        out = torch.empty(max(size, 1), dtype=torch.uint8, device=device)
    _require(out, torch.uint8, "out")
    # the frame goes up through a pinned buffer kept with the workspace (the call synchronizes
    # its stream before returning, so the buffer is free again when the next call starts)
    wsp = workspace or Workspace(out.device)
    pin = getattr(wsp, "lz4_pin", None)
    if pin is None or pin.numel() < max(len(b), 1):
        pin = wsp.lz4_pin = torch.empty(max(len(b), 4096), dtype=torch.uint8, pin_memory=True)
    if b:
        pin.numpy()[:len(b)] = np.frombuffer(b, dtype=np.uint8)
    # and into a device buffer kept with it (no allocation per call)
    dbuf = getattr(wsp, "lz4_dev", None)
    if dbuf is None or dbuf.numel() < max(len(b), 1) or dbuf.device != out.device:
        dbuf = wsp.lz4_dev = torch.empty(max(len(b), 4096), dtype=torch.uint8, device=out.device)
    dframe = dbuf[:max(len(b), 1)]
    dframe.copy_(pin[:max(len(b), 1)], non_blocking=True)
    workspace = wsp
    need = int(_lib.lib().dpz_lz4_workspace_bytes(0, nb, 0 if linked else bmax))
    ws = _lz4_ws(workspace, out.device, need)
    n = ctypes.c_int64(0)
    rc = _lib.lib().dpz_lz4_decompress(_ptr(dframe), b, len(b), _ptr(out), out.numel(),
                                       ctypes.byref(n), _ptr(ws), ws.numel(), _stream(out.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed LZ4 frame")
    check(rc, "dpz_lz4_decompress")
    return out[:n.value]


def delta_i32(idx, out=None):
    """``np.diff(idx, prepend=0).astype(np.int32)`` of a device int32 vector."""
    _require(idx, torch.int32, "idx")
    if out is None:  # (not empty_like: an empty idx may carry a zero stride, which no view takes)
        out = torch.empty(idx.shape, dtype=torch.int32, device=idx.device)
    rc = _lib.lib().dpz_delta_i32(_ptr(idx), idx.numel(), _ptr(out), _stream(idx.device))
    check(rc, "dpz_delta_i32")
    return out


def running_sum_i32(d, dtype=torch.int64, workspace=None):
    """``np.cumsum`` of a device int32 vector as int64 (or truncated to int32)."""
    _require(d, torch.int32, "d")
    k = d.numel()
    out = torch.empty(max(k, 1), dtype=dtype, device=d.device)
    ws = _lz4_ws(workspace, d.device, int(_lib.lib().dpz_running_sum_workspace_bytes(k)))
    rc = _lib.lib().dpz_running_sum_i32(_ptr(d), k, _ptr(out if dtype == torch.int64 else None),
                                        _ptr(out if dtype == torch.int32 else None), _ptr(ws),
                                        ws.numel(), _stream(d.device))
    check(rc, "dpz_running_sum_i32")
    return out[:k]


def mt_rank_entries(n):
    """int32 entries of the rank table that goes with a mask over n elements (opaque)."""
    return int(_lib.lib().dpz_mt_rank_entries(int(n)))


def _mt_ws(workspace, device, need):
    workspace = workspace or Workspace(device)
    buf = getattr(workspace, "mbuf", None)
    if buf is None or buf.numel() < max(need, 256):
        buf = workspace.mbuf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return buf


def mt_mask(seed, alpha, n, device, mask=None, rank_tab=None, count=None, workspace=None):
    """SubSampling's Bernoulli mask (reference sharing/SubSampling.py:148-157, 265-294):
    ``torch.rand(n, generator=g) <= alpha`` after ``g.manual_seed(seed)``, bit for bit, from a
    jump-ahead MT19937 on the device (the generator is seeded with ``seed & 0xffffffff`` and
    ``alpha`` compared as the fp32 torch rounds it to).  Returns ``(mask int32[mask_words(n)],
    rank_tab int32[mt_rank_entries(n)], count int64[1])``, all on the device; nothing blocks."""
    n = int(n)
    device = torch.device(device)
    if mask is None:
        mask = torch.empty(mask_words(n), dtype=torch.int32, device=device)
    if rank_tab is None:
        rank_tab = torch.empty(mt_rank_entries(n), dtype=torch.int32, device=device)
    if count is None:
        count = torch.empty(1, dtype=torch.int64, device=device)
    _require(mask, torch.int32, "mask")
    _require(rank_tab, torch.int32, "rank_tab")
    _require(count, torch.int64, "count")
    if mask.numel() < mask_words(n) or rank_tab.numel() < mt_rank_entries(n):
        raise ValueError("mask / rank_tab too small for n")
    ws = _mt_ws(workspace, device, int(_lib.lib().dpz_mt_mask_workspace_bytes(n)))
    with torch.cuda.device(device):  # the jump tables are kept per device
        rc = _lib.lib().dpz_mt_mask(int(seed) & 0xffffffff, float(np.float32(alpha)), n,
                                    _ptr(mask), _ptr(rank_tab), _ptr(count), _ptr(ws),
                                    ws.numel(), _stream(device))
    check(rc, "dpz_mt_mask")
    return mask, rank_tab, count


def mask_gather(x, mask, rank_tab, vals, counter=None, count=None):
    """``vals[:count] = x[mask]`` in index order and, with ``counter`` (int32[n]),
    ``counter[mask] += 1`` (reference SubSampling.py:158-159).  ``vals`` is caller-owned and
    holds at least the mask's count of values: a caller that has read the count passes it as
    ``count`` (a Python int) and a shorter ``vals`` is refused here, before the launch."""
    _require(x, torch.float32, "x")
    _require(mask, torch.int32, "mask")
    _require(rank_tab, torch.int32, "rank_tab")
    _require(vals, torch.float32, "vals")
    _require(counter, torch.int32, "counter")
    n = x.numel()
    if mask.numel() < mask_words(n) or rank_tab.numel() < mt_rank_entries(n):
        raise ValueError("mask / rank_tab too small for x")
    if counter is not None and counter.numel() != n:
        raise ValueError("counter and x differ in length")
    if count is not None and vals.numel() < int(count):
        raise ValueError(f"vals holds {vals.numel()} values for a mask of {int(count)} elements")
    # an empty selection writes nothing, but the ABI wants a pointer
    rc = _lib.lib().dpz_mask_gather(_ptr(x), n, _ptr(mask), _ptr(rank_tab),
                                    _ptr(vals if vals.numel() else x), _ptr(counter),
                                    _stream(x.device))
    check(rc, "dpz_mask_gather")
    return vals


MASK_FOLD_MAX = 16  # payloads per dpz_mask_decode_average launch


def mask_decode_average(local, payloads, weights, w_self=None, out=None, counts=None):
    """Metro-Hastings fold over SubSampling payloads (reference Sharing.py:156-229 over
    SubSampling.deserialized_model), bit-exact in the reference's fp32 order.

    payloads : list of ``(mask, rank_tab, vals)`` device tensors; ``vals`` must hold exactly the
               mask's count of values
    weights  : per-payload weights (Python floats, rounded to fp32 like torch does)
    w_self   : weight of the local term, or None for the server form (no self term)
    counts   : the masks' counts as Python ints, when the caller has read them: a payload whose
               ``vals`` differs in length raises ValueError before anything is launched (without
               it the caller answers for the lengths: the kernel indexes vals by mask rank)

    More than 16 payloads are folded 16 at a time, each launch continuing the running total of
    the one before it (DPZ_FOLD_ACCUMULATE) and the last adding the self term: the same
    roundings in the same order as one pass.
    """
    _require(local, torch.float32, "local")
    n = local.numel()
    if out is None:
        out = torch.empty_like(local)
    _require(out, torch.float32, "out")
    if out.numel() != n or out.data_ptr() == local.data_ptr():
        raise ValueError("out must hold n values and not be local")
    npay = len(payloads)
    if npay < 1:
        raise ValueError("no payloads")
    if counts is not None:
        for i, ((_, _, vals), c) in enumerate(zip(payloads, counts)):
            if vals.numel() != int(c):
                raise ValueError(f"payload {i}: {vals.numel()} params for a mask of {int(c)} "
                                 "elements")
    for i, (mask, rank_tab, vals) in enumerate(payloads):
        _require(mask, torch.int32, "mask")
        _require(rank_tab, torch.int32, "rank_tab")
        _require(vals, torch.float32, "vals")
        if mask.numel() < mask_words(n) or rank_tab.numel() < mt_rank_entries(n):
            raise ValueError("mask / rank_tab too small for local")
    for lo in range(0, npay, MASK_FOLD_MAX):
        part = payloads[lo:lo + MASK_FOLD_MAX]
        last = lo + MASK_FOLD_MAX >= npay
        m_arr = (ctypes.c_void_p * len(part))()
        r_arr = (ctypes.c_void_p * len(part))()
        v_arr = (ctypes.c_void_p * len(part))()
        w_arr = (ctypes.c_float * len(part))()
        for i, (mask, rank_tab, vals) in enumerate(part):
            if vals.numel() == 0:  # an empty selection: never read, but the ABI wants a pointer
                vals = local
            m_arr[i], r_arr[i], v_arr[i] = mask.data_ptr(), rank_tab.data_ptr(), vals.data_ptr()
            w_arr[i] = float(weights[lo + i])
        flags = ((DPZ_FOLD_SELF if last and w_self is not None else 0)
                 | (_lib.DPZ_FOLD_ACCUMULATE if lo else 0))
        rc = _lib.lib().dpz_mask_decode_average(
            _ptr(local), n, len(part), m_arr, r_arr, v_arr, w_arr,
            float(w_self) if w_self is not None else 0.0, flags, _ptr(out),
            _stream(local.device))
        check(rc, "dpz_mask_decode_average")
    return out


def mt_mask_batch(seeds, alphas, n, device, mask=None, rank_tab=None, count=None,
                  workspace=None):
    """``mt_mask`` for ``len(seeds)`` masks of one length with one launch per phase
    (dpz_mt_mask_batch): row i of the returned ``(mask int32[m, >= mask_words(n)], rank_tab
    int32[m, >= mt_rank_entries(n)], count int64[m])`` is bit for bit ``mt_mask(seeds[i],
    alphas[i], n)``.  Caller-owned outputs are 2-D with contiguous rows; a mask row stride is a
    multiple of 4 words.  Nothing blocks (but the first call on a device, as ``mt_mask``)."""
    n, m = int(n), len(seeds)
    if m < 1 or len(alphas) != m:
        raise ValueError("seeds and alphas must hold one entry per mask, at least one")
    device = torch.device(device)
    if mask is None:
        mask = torch.empty(m, -(-mask_words(n) // 4) * 4, dtype=torch.int32, device=device)
    if rank_tab is None:
        rank_tab = torch.empty(m, mt_rank_entries(n), dtype=torch.int32, device=device)
    if count is None:
        count = torch.empty(m, dtype=torch.int64, device=device)
    for t, dtype, name, need in ((mask, torch.int32, "mask", mask_words(n)),
                                 (rank_tab, torch.int32, "rank_tab", mt_rank_entries(n))):
        if not t.is_cuda or t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{name} must be a 2-D {dtype} device tensor with contiguous rows")
        if t.shape[0] < m or t.shape[1] < need or (m > 1 and t.stride(0) < need):
            raise ValueError(f"{name} too small for {m} masks of {n} elements")
    _require(count, torch.int64, "count")
    if count.numel() < m:
        raise ValueError("count must hold one word per mask")
    L = _lib.lib()
    ws = _mt_ws(workspace, device, int(L.dpz_mt_mask_batch_workspace_bytes(m, n)))
    s_arr = (ctypes.c_uint32 * m)(*[int(s) & 0xffffffff for s in seeds])
    a_arr = (ctypes.c_float * m)(*[float(np.float32(a)) for a in alphas])
    with torch.cuda.device(device):  # the jump tables are kept per device
        rc = L.dpz_mt_mask_batch(m, s_arr, a_arr, n, _ptr(mask), mask.stride(0), _ptr(rank_tab),
                                 rank_tab.stride(0), _ptr(count), _ptr(ws), ws.numel(),
                                 _stream(device))
    check(rc, "dpz_mt_mask_batch")
    return mask, rank_tab, count


def _row_ptrs(rows, m):
    """Device addresses of m rows: the rows of a 2-D tensor or the words of a 1-D one (computed
    from its stride, no views), or a list's tensors (None: a zero word)."""
    if rows is None:
        return [0] * m
    if isinstance(rows, torch.Tensor):
        step = rows.stride(0) * rows.element_size()
        return [rows.data_ptr() + j * step for j in range(m)]
    return [0 if t is None else t.data_ptr() for t in rows]


def _f32_bits(v):
    """The fp32 bits of a Python number, rounded as torch rounds a scalar."""
    return int(np.float32(v).view(np.uint32))


def _i32_bits(v):
    return int(np.int32(v).view(np.uint32))


def _ptr_table(cols, m, device):
    """A DEVICE node table: ``cols`` (tensors with a row per node, lists of per-node tensors, or
    None for a zero column) as the row pointers of an (m, len(cols)) int64 table."""
    tab = np.array([_row_ptrs(c, m) for c in cols], dtype=np.uint64).T.copy()
    return torch.from_numpy(tab.view(np.int64)).to(device)


def gather_node_table(x, mask, rank_tab, vals, count, status, counter=None):
    """The DEVICE node table of ``mask_gather_nodes``: 8 64-bit words per node {x, mask, rank_tab,
    vals, counter or 0, count, status, 0}.  Every argument is a 2-D tensor (one row per node) or
    a list of per-node tensors; ``count`` (int64) and ``status`` (int32) are 1-D (any stride), one
    word per node."""
    dev = (x if isinstance(x, torch.Tensor) else x[0]).device
    return _ptr_table((x, mask, rank_tab, vals, counter, count, status, None), len(x), dev)


def mask_gather_nodes(table, n, cap):
    """``mask_gather`` of every node of ``table`` (``gather_node_table``) in one launch, each into
    its slot of ``cap`` values: a node whose mask selects more leaves its slot filled up to
    ``cap``, nothing past it, and its status word nonzero (zero otherwise)."""
    _require(table, torch.int64, "table")
    rc = _lib.lib().dpz_mask_gather_nodes(table.shape[0], _ptr(table), int(n), int(cap),
                                          _stream(table.device))
    check(rc, "dpz_mask_gather_nodes")


def fold_node_table(dests, device):
    """The DEVICE fold table of ``mask_decode_average_nodes`` and the host copy of its payload
    counts.  ``dests``: per destination ``(local, out, w_self or None, [(mask, rank_tab, vals,
    w), ...])`` with 1..16 payloads; 68 64-bit words each: {local, out, w_self, n_payloads}, then
    {mask, rank_tab, vals, w} per payload (weights as fp32 bits in the low half of their word)."""
    tab = np.zeros((max(1, len(dests)), 4 + 4 * MASK_FOLD_MAX), dtype=np.uint64)
    counts = (ctypes.c_int * max(1, len(dests)))()
    for j, (local, out, w_self, pays) in enumerate(dests):
        counts[j] = len(pays)
        tab[j, :4] = (local.data_ptr(), out.data_ptr(), _f32_bits(w_self or 0.0), len(pays))
        for p, (mask, rank_tab, vals, w) in enumerate(pays[:MASK_FOLD_MAX]):
            if vals.numel() == 0:  # an empty selection: never read, but kept a valid address
                vals = local
            tab[j, 4 + 4 * p:8 + 4 * p] = (mask.data_ptr(), rank_tab.data_ptr(), vals.data_ptr(),
                                           _f32_bits(w))
    return torch.from_numpy(tab.view(np.int64)).to(device), counts


def mask_decode_average_nodes(table, counts, n, self_term=True, guard=None):
    """``mask_decode_average`` of every destination of ``table`` (``fold_node_table``) in one
    launch.  ``guard`` (int32 device words, e.g. the gathers' status words): nothing is written
    if any is nonzero.  Returns False, with nothing enqueued, when a destination has more than
    16 payloads (the caller folds that round through ``mask_decode_average``)."""
    _require(table, torch.int64, "table")
    _require(guard, torch.int32, "guard")
    rc = _lib.lib().dpz_mask_decode_average_nodes(
        len(counts), _ptr(table), counts, int(n), DPZ_FOLD_SELF if self_term else 0, _ptr(guard),
        guard.numel() if guard is not None else 0, _stream(table.device))
    if rc == _lib.DPZ_ERR_UNSUPPORTED and max(counts) > MASK_FOLD_MAX:
        return False
    check(rc, "dpz_mask_decode_average_nodes")
    return True


def dense_tile_elems(n_src):
    """The column tile of the staged dense fold for ``n_src`` source rows: the largest of 1024 /
    512 / 256 elements whose rows fit 64 KiB of LDS; 0 when none does (only the direct path)."""
    return int(_lib.lib().dpz_dense_tile_elems(int(n_src)))


def dense_auto_mode(n_src, row_reads, n):
    """The path DPZ_DENSE_AUTO takes for ``n_src`` sources, ``row_reads`` = sum(count + 1) over
    the receivers and rows of n elements: DPZ_DENSE_STAGED or DPZ_DENSE_DIRECT."""
    return int(_lib.lib().dpz_dense_auto_mode(int(n_src), int(row_reads), int(n)))


class _WordTable:
    """A fold table of 64-bit words: ``host``, the copy the library validates (kept alive here),
    and ``dev``, the DEVICE words."""

    def _words(self, n_words):
        self.host = np.zeros(max(1, n_words), dtype=np.uint64)
        return self.host, self.host.view(np.uint32)  # little endian: [2 i] the low half of word i

    def _upload(self, device):
        self.dev = torch.from_numpy(self.host.view(np.int64)).to(device)


class DenseTable(_WordTable):
    """The fold table of ``dense_average_nodes`` (a ``_WordTable``), with the counts the call
    repeats."""

    def __init__(self, srcs, recvs, device):
        """srcs: the source rows (a 2-D tensor or a list of 1-D tensors); recvs: per receiver
        ``(out row, index of its own row, w_self, [(source index, weight), ...])`` in fold
        order.  Weights are Python floats, rounded to fp32 here as torch rounds a scalar."""
        src_ptrs = _row_ptrs(srcs, srcs.shape[0] if isinstance(srcs, torch.Tensor) else len(srcs))
        self.n_src, self.m = len(src_ptrs), len(recvs)
        self.n_entries = sum(len(r[3]) for r in recvs)
        self.reads = self.n_entries + self.m  # row reads of the direct path
        words, halves = self._words(self.n_src + 4 * self.m + self.n_entries)
        words[:self.n_src] = src_ptrs
        ent = self.n_src + 4 * self.m
        start = 0
        for j, (out, own, w_self, pairs) in enumerate(recvs):
            b = self.n_src + 4 * j
            words[b] = out.data_ptr()
            halves[2 * b + 2:2 * b + 6] = (_i32_bits(own), _f32_bits(w_self), start, len(pairs))
            for src, w in pairs:
                halves[2 * (ent + start):2 * (ent + start) + 2] = (_i32_bits(src), _f32_bits(w))
                start += 1
        self._upload(device)


def dense_average_nodes(table, n, mode=_lib.DPZ_DENSE_AUTO, check_rc=True):
    """Every receiver's dense fold of ``table`` (a ``DenseTable``) in one launch: out = the
    weighted sum of its list's source rows in list order plus ``w_self`` times its own row, in
    the fp32 order of the dense ``decode_average``; an empty list copies the own row.  mode:
    DPZ_DENSE_AUTO / _STAGED / _DIRECT.  Returns the library's code (raises unless it is DPZ_OK
    when ``check_rc``)."""
    _require(table.dev, torch.int64, "table")
    rc = _lib.lib().dpz_dense_average_nodes(
        table.m, _ptr(table.dev), ctypes.c_void_p(table.host.ctypes.data), table.n_entries,
        table.n_src, int(n), int(mode), _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_dense_average_nodes")
    return rc


def choco_chunk_elems():
    """Elements one block of ``choco_encode_nodes``' count and compaction passes covers."""
    return int(_lib.lib().dpz_choco_chunk_elems())


def choco_tile_elems():
    """Elements of one receiver a block of ``choco_fold_nodes`` owns."""
    return int(_lib.lib().dpz_choco_tile_elems())


def choco_node_table(x, x_hat, rows):
    """The DEVICE node table of ``choco_encode_nodes``: 4 64-bit words per node {x, x_hat, packed
    row, 0}.  Each argument is a 2-D tensor (one row per node) or a list of per-node tensors."""
    dev = (x if isinstance(x, torch.Tensor) else x[0]).device
    return _ptr_table((x, x_hat, rows, None), len(x), dev)


def _encode_nodes(name, table, m, n, args, workspace):
    """``dpz_<name>_encode_nodes`` on the m nodes of the device ``table``: size the workspace, grow
    it where it is too small, call with ``args`` between n and the workspace, check; returns the
    workspace."""
    lib = _lib.lib()
    need = int(getattr(lib, f"dpz_{name}_encode_workspace_bytes")(m, n))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=table.device)
    rc = getattr(lib, f"dpz_{name}_encode_nodes")(m, _ptr(table), n, *args, _ptr(workspace),
                                                   workspace.numel(), _stream(table.device))
    check(rc, f"dpz_{name}_encode_nodes")
    return workspace


def choco_encode_nodes(table, n, k, cap, workspace=None):
    """Choco's ``_pre_step`` + ``serialized_model`` of every node of ``table``
    (``choco_node_table``): per node the threshold selection of ``topk_threshold(x - x_hat, k)``
    into its packed row ``[count (int64), status, 0 | cap idx | cap vals]``, status 1 and nothing
    written past ``cap`` when more are selected.  One launch set for all nodes, nothing read back.
    ``workspace``: a uint8 device tensor kept by the caller (allocated here when None); returned."""
    _require(table, torch.int64, "table")
    return _encode_nodes("choco", table, table.shape[0], int(n), (int(k), int(cap)), workspace)


class ChocoTable(_WordTable):
    """The fold table of ``choco_fold_nodes`` (a ``_WordTable``), with the counts the call
    repeats."""

    def __init__(self, recvs, device):
        """recvs: per receiver ``(x, x_hat, s, own packed row, own cap, w_self, [(packed row,
        cap, weight), ...])``, the list in fold order.  Rows are tensors or device addresses;
        weights are Python floats, rounded to fp32 here as torch rounds a scalar."""
        def ptr(t):
            return t.data_ptr() if isinstance(t, torch.Tensor) else int(t)

        self.m = len(recvs)
        self.n_entries = sum(len(r[6]) for r in recvs)
        words, halves = self._words(6 * self.m + 2 * self.n_entries)
        ent, start = 6 * self.m, 0
        for j, (x, x_hat, s, row, cap, w_self, pays) in enumerate(recvs):
            b = 6 * j
            words[b:b + 4] = (ptr(x), ptr(x_hat), ptr(s), ptr(row))
            halves[2 * b + 8:2 * b + 12] = (_f32_bits(w_self), _i32_bits(cap), start, len(pays))
            for prow, pcap, w in pays:
                e = ent + 2 * start
                words[e] = ptr(prow)
                halves[2 * e + 2:2 * e + 4] = (_f32_bits(w), _i32_bits(pcap))
                start += 1
        self._upload(device)


def choco_fold_nodes(table, n, step_size, guard=None, check_rc=True):
    """Choco's ``_averaging`` of every receiver of ``table`` (a ``ChocoTable``) in one launch, in
    place: ``x_hat += q_self``; ``s += w_p T_p`` in list order, ``+= w_self q_self``;
    ``x += step_size (s - x_hat)``, each operation rounded to fp32 on its own.  ``guard`` (int32
    device words, e.g. the rows' status words): nothing is written if any is nonzero.  Returns
    the library's code (raises unless it is DPZ_OK when ``check_rc``)."""
    _require(table.dev, torch.int64, "table")
    _require(guard, torch.int32, "guard")
    rc = _lib.lib().dpz_choco_fold_nodes(
        table.m, _ptr(table.dev), ctypes.c_void_p(table.host.ctypes.data), table.n_entries,
        int(n), float(step_size), _ptr(guard), guard.numel() if guard is not None else 0,
        _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_choco_fold_nodes")
    return rc


def stc_chunk_elems():
    """Elements one block of ``stc_encode_nodes``' count and compaction passes covers."""
    return int(_lib.lib().dpz_stc_chunk_elems())


def stc_tile_elems():
    """Elements of the server's residual a block of ``stc_server_fold`` owns."""
    return int(_lib.lib().dpz_stc_tile_elems())


def stc_row_words(k):
    """int32 words of an STC packed row ``[count = k (int64), 0, 0 | up4(k) idx | up4(k) vals]``."""
    return 4 + 2 * (-(-int(k) // 4) * 4)


def stc_node_table(x, prev, r, rows):
    """The DEVICE node table of ``stc_encode_nodes``: 4 64-bit words per node {x, prev, r, packed
    row}.  Each argument is a 2-D tensor (one row per node) or a list of per-node tensors.  ``x``
    and ``prev`` None, or None for a node in their lists: the server form (``r`` already holds
    the change vector)."""
    dev = (r if isinstance(r, torch.Tensor) else r[0]).device
    m = len(r)

    def ptrs(col):
        if col is None or isinstance(col, torch.Tensor):
            return _row_ptrs(col, m)
        return [0 if t is None else t.data_ptr() for t in col]

    tab = np.array([ptrs(c) for c in (x, prev, r, rows)], dtype=np.uint64).T.copy()
    return torch.from_numpy(tab.view(np.int64)).to(dev)


def stc_encode_nodes(table, n, k, workspace=None):
    """STC's ``get_data_to_send`` of every node of ``table`` (``stc_node_table``): per node
    ``c = (x - prev) + r``, the exact top-k of ``|c|`` (ties to the lowest indices) into its packed
    row, ``prev = x`` and ``r = c`` with +0 at the sent entries; a node in server form selects from
    ``r`` as it is.  One launch set for all nodes, nothing read back.  ``workspace``: a uint8
    device tensor kept by the caller (allocated here when None); returned."""
    _require(table, torch.int64, "table")
    return _encode_nodes("stc", table, table.shape[0], int(n), (int(k),), workspace)


class StcFoldTable(_WordTable):
    """The table of ``stc_server_fold`` (a ``_WordTable``): 2 words per payload {packed row,
    weight}, in fold order."""

    def __init__(self, pays, device):
        """pays: ``[(packed row, weight), ...]`` in fold order.  Rows are tensors or device
        addresses; weights are Python floats, rounded to fp32 here as torch rounds a scalar."""
        self.n_payloads = len(pays)
        words, halves = self._words(2 * self.n_payloads)
        for p, (row, w) in enumerate(pays):
            words[2 * p] = row.data_ptr() if isinstance(row, torch.Tensor) else int(row)
            halves[4 * p + 2] = _f32_bits(w)
        self._upload(device)


def stc_server_fold(table, n, k, r_s, check_rc=True):
    """STC's ``_averaging_server`` over the payloads of ``table`` (a ``StcFoldTable``) in one
    launch, in place: ``total = 0; total[idx_p] += vals_p w_p`` in table order, then
    ``r_s += total``, each operation rounded to fp32 on its own.  Returns the library's code
    (raises unless it is DPZ_OK when ``check_rc``)."""
    _require(table.dev, torch.int64, "table")
    _require(r_s, torch.float32, "r_s")
    rc = _lib.lib().dpz_stc_server_fold(
        table.n_payloads, _ptr(table.dev), ctypes.c_void_p(table.host.ctypes.data), int(n),
        int(k), _ptr(r_s), _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_stc_server_fold")
    return rc


def stc_apply_table(xs):
    """The DEVICE table of ``stc_apply_nodes``: one row pointer per target model (a 2-D tensor or
    a list of per-model tensors)."""
    dev = (xs if isinstance(xs, torch.Tensor) else xs[0]).device
    return _ptr_table((xs,), len(xs), dev).reshape(-1)


def stc_apply_nodes(table, n, k, row):
    """STC's ``process_received`` of every model of ``table`` (``stc_apply_table``) in one launch,
    in place: ``x[idx] += vals`` over the packed broadcast ``row``; the elements the row does not
    name keep their bits."""
    _require(table, torch.int64, "table")
    _require(row, torch.int32, "row")
    rc = _lib.lib().dpz_stc_apply_nodes(table.numel(), _ptr(table), int(n), int(k), _ptr(row),
                                        _stream(table.device))
    check(rc, "dpz_stc_apply_nodes")


def topkacc_chunk_elems():
    """Elements one block of ``topkacc_encode_nodes``' count and compaction passes covers."""
    return int(_lib.lib().dpz_topkacc_chunk_elems())


def topkacc_row_words(k):
    """int32 words of a packed row ``[count = k (int64), 0, 0 | up4(k) idx | up4(k) vals]``."""
    return 4 + 2 * (-(-int(k) // 4) * 4)


def topkacc_node_table(x, x0, acc, rows, key=None, counter=None):
    """The DEVICE node table of ``topkacc_encode_nodes`` and ``topkacc_post_nodes``: 6 64-bit
    words per node {x, x0, acc, key, counter or 0, packed row}.  Each argument is a 2-D tensor (one
    row per node) or a list of per-node tensors.  ``key``: the scratch rows of DPZ_ACC_ADD (not
    read with DPZ_ACC_ACCUMULATE, whose key row is ``acc``); ``rows`` may be None for a table that
    only ``topkacc_post_nodes`` reads."""
    dev = (x if isinstance(x, torch.Tensor) else x[0]).device
    return _ptr_table((x, x0, acc, key, counter, rows), len(x), dev)


def topkacc_encode_nodes(table, n, k, mode, workspace=None):
    """PartialModel's ``_pre_step`` + ``serialized_model`` with accumulation of every node of
    ``table`` (``topkacc_node_table``).  mode DPZ_ACC_ACCUMULATE: ``acc += x - x0`` everywhere, the
    key is ``|acc|``; DPZ_ACC_ADD: the key is ``|(x - x0) + acc|``, formed into the table's key
    rows, ``acc`` unchanged before the rewind.  Per node the exact top-k of the key (ties to the
    lowest indices) into its packed row with ``vals = x[idx]``, ``counter[idx] += 1`` and
    ``acc[idx] = +0``.  One launch set for all nodes, nothing read back.  ``workspace``: a uint8
    device tensor kept by the caller (allocated here when None); returned."""
    _require(table, torch.int64, "table")
    return _encode_nodes("topkacc", table, table.shape[0], int(n), (int(k), int(mode)), workspace)


def topkacc_post_nodes(table, n):
    """PartialModel's accumulating ``_post_step`` of every node of ``table``
    (``topkacc_node_table``) in one launch: ``acc += x - x0``, x the averaged model and x0 the model
    the round started from."""
    _require(table, torch.int64, "table")
    rc = _lib.lib().dpz_topkacc_post_nodes(table.shape[0], _ptr(table), int(n),
                                           _stream(table.device))
    check(rc, "dpz_topkacc_post_nodes")


class DwtNodesTable(_WordTable):
    """The table of ``dwt_sym2_nodes`` (a ``_WordTable``): 4 words per node {x, x0, coeffs_x or 0,
    coeffs_diff or 0}.  Each argument is a 2-D tensor (one row per node), a list of per-node
    tensors, or None (a zero column)."""

    def __init__(self, x, x0, coeffs_x, coeffs_diff, device):
        self.m = m = len(x)
        words, _ = self._words(4 * m)
        words[:4 * m] = np.array([_row_ptrs(c, m) for c in (x, x0, coeffs_x, coeffs_diff)],
                                 dtype=np.uint64).T.reshape(-1)
        self._upload(device)


class IdwtNodesTable(_WordTable):
    """The table of ``idwt_sym2_nodes`` (a ``_WordTable``): 2 words per node {coeffs, out}."""

    def __init__(self, coeffs, out, device):
        self.m = m = len(coeffs)
        words, _ = self._words(2 * m)
        words[:2 * m] = np.array([_row_ptrs(c, m) for c in (coeffs, out)],
                                 dtype=np.uint64).T.reshape(-1)
        self._upload(device)


def dwt_sym2_nodes(table, n, level=4, accumulate=False, check_rc=True):
    """``wavedec`` (sym2) of every node of ``table`` (a ``DwtNodesTable``) in ONE launch: per node
    bit for bit ``dpz_dwt_sym2(x, x0, n, level, coeffs_x, coeffs_diff, accumulate)``.  Every row is
    16-byte aligned and every node names the same outputs.  Returns the library's code (raises
    unless it is DPZ_OK when ``check_rc``)."""
    _require(table.dev, torch.int64, "table")
    rc = _lib.lib().dpz_dwt_sym2_nodes(table.m, _ptr(table.dev),
                                       ctypes.c_void_p(table.host.ctypes.data), int(n), int(level),
                                       1 if accumulate else 0, _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_dwt_sym2_nodes")
    return rc


def idwt_sym2_nodes(table, n, level=4, check_rc=True):
    """``waverec`` (sym2) of every node of ``table`` (an ``IdwtNodesTable``) in ONE launch: per
    node bit for bit ``dpz_idwt_sym2(coeffs, n, level, out)``."""
    _require(table.dev, torch.int64, "table")
    rc = _lib.lib().dpz_idwt_sym2_nodes(table.m, _ptr(table.dev),
                                        ctypes.c_void_p(table.host.ctypes.data), int(n),
                                        int(level), _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_idwt_sym2_nodes")
    return rc


def jwins_chunk_elems():
    """Elements one block of ``jwins_encode_nodes``' count and compaction passes covers."""
    return int(_lib.lib().dpz_jwins_chunk_elems())


class JwinsEncodeTable:
    """The node table of ``jwins_encode_nodes``: 8 words per node {c, acc, vals_src, counter or 0,
    idx_out, val_out, k, 0}.  The first four columns are set once (2-D tensors with a row per
    node, or lists of per-node tensors; ``counter`` may be None); ``set(j, k, idx_out, val_out)``
    fills a round's words of node j on the host (addresses or tensors; 0 / None for none), and
    ``upload()`` enqueues the copy to the DEVICE words without waiting for it: the host words go
    through a pinned staging block of their own per upload, which the allocator hands out again
    only after the copy has run."""

    def __init__(self, c, acc, vals_src, counter, device):
        self.m = m = len(c)
        self.host = np.zeros((max(1, m), 8), dtype=np.uint64)
        for col, rows in enumerate((c, acc, vals_src, counter)):
            self.host[:m, col] = _row_ptrs(rows, m)
        self.dev = torch.zeros(max(1, m), 8, dtype=torch.int64, device=device)

    @staticmethod
    def _addr(t):
        if t is None:
            return 0
        return t.data_ptr() if isinstance(t, torch.Tensor) else int(t)

    def set(self, j, k, idx_out, val_out):
        self.host[j, 4:] = (self._addr(idx_out), self._addr(val_out), int(k), 0)

    def upload(self):
        src = torch.from_numpy(self.host.view(np.int64))
        if self.dev.is_cuda:
            src = src.pin_memory()
        self.dev.copy_(src, non_blocking=True)
        return self


def jwins_encode_nodes(table, n, workspace=None):
    """JWINS's ``serialized_model`` of every node of ``table`` (an uploaded ``JwinsEncodeTable``),
    each with its own k, in one launch set.  A node with 1 <= k <= n: the key ``|c + acc|`` is
    formed in place into its ``c`` row, the exact top-k of it (ties to the lowest indices) goes
    to ``idx_out`` ascending with ``val_out = vals_src[idx]``, ``counter[idx] += 1``,
    ``acc[idx] = +0``.  A node with k = 0 shares fully: ``acc = +0`` everywhere and, with a
    ``val_out``, ``val_out[:n] = vals_src``.  Nothing is read back.  ``workspace``: a uint8 device
    tensor kept by the caller (allocated here when None); returned."""
    _require(table.dev, torch.int64, "table")
    m, n = table.m, int(n)
    ks = table.host[:m, 6]
    if m and int(ks.max()) > n:
        raise ValueError(f"a node's k = {int(ks.max())} exceeds n = {n}")
    part = ks > 0
    if (table.host[:m, :3] == 0).any() or (table.host[:m, 4:6][part] == 0).any():
        raise ValueError("a node table with a null row: c, acc and vals_src of every node, "
                         "idx_out and val_out of every node with k >= 1")
    return _encode_nodes("jwins", table.dev, m, n, (), workspace)


class FftNodesTable(_WordTable):
    """The table of ``rfft_nodes`` (a ``_WordTable``): 4 words per job {x, x0 or 0, out,
    accumulate}.  A job is a transform: ``x`` / ``x0`` (fp32, n) and ``out`` (complex64,
    n // 2 + 1) are 2-D tensors (one row per job), lists of per-job tensors, or None for ``x0``
    (a zero column); ``accumulate`` is one flag for every job or a list of flags."""

    def __init__(self, x, x0, out, accumulate, device):
        self.m = m = len(x)
        words, _ = self._words(4 * m)
        flags = [int(bool(accumulate))] * m if isinstance(accumulate, (bool, int)) \
            else [int(bool(a)) for a in accumulate]
        words[:4 * m] = np.array([_row_ptrs(x, m), _row_ptrs(x0, m), _row_ptrs(out, m), flags],
                                 dtype=np.uint64).T.reshape(-1)
        self._upload(device)


class IfftNodesTable(_WordTable):
    """The table of ``irfft_nodes`` (a ``_WordTable``): 2 words per job {coeffs, out}."""

    def __init__(self, coeffs, out, device):
        self.m = m = len(coeffs)
        words, _ = self._words(2 * m)
        words[:2 * m] = np.array([_row_ptrs(c, m) for c in (coeffs, out)],
                                 dtype=np.uint64).T.reshape(-1)
        self._upload(device)


def fft_nodes_workspace(jobs, n, device, workspace=None):
    """A uint8 device tensor of ``dpz_fft_nodes_workspace_bytes(jobs, n)`` bytes (``workspace``
    itself when it is large enough); ValueError for a size the batched transforms refuse."""
    need = int(_lib.lib().dpz_fft_nodes_workspace_bytes(int(jobs), int(n)))
    if need < 0:
        raise ValueError(f"batched real FFTs of n={n}: an even n >= 4 with a native plan "
                         "(fft_native) and jobs >= 1")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    return workspace


def _fft_nodes(name, table, n, workspace, check_rc):
    _require(table.dev, torch.int64, "table")
    if workspace is None:
        need = int(_lib.lib().dpz_fft_nodes_workspace_bytes(table.m, int(n)))
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=table.dev.device)
    rc = getattr(_lib.lib(), name)(table.m, _ptr(table.dev),
                                   ctypes.c_void_p(table.host.ctypes.data), int(n),
                                   _ptr(workspace), workspace.numel(),
                                   _stream(table.dev.device))
    if check_rc:
        check(rc, name)
    return rc


def rfft_nodes(table, n, workspace=None, check_rc=True):
    """``rfft`` of every job of ``table`` (an ``FftNodesTable``) in ONE launch set, as many
    launches as one ``rfft`` of that n: per job bit for bit ``rfft(x)``, ``rfft(x - x0)`` (the
    difference as ``elementwise(SUB)`` rounds it) where the job has an ``x0``, and ``out +=`` that
    (as ``elementwise(ADD)`` rounds it) where it accumulates.  Even n >= 4 with a native plan.
    ``workspace``: ``fft_nodes_workspace``'s tensor (allocated here when None).  Returns the
    library's code (raises unless it is DPZ_OK when ``check_rc``)."""
    return _fft_nodes("dpz_rfft_nodes", table, n, workspace, check_rc)


def irfft_nodes(table, n, workspace=None, check_rc=True):
    """``irfft`` of every job of ``table`` (an ``IfftNodesTable``) in ONE launch set: per job bit
    for bit ``irfft(coeffs, n)``; the coefficients are only read."""
    return _fft_nodes("dpz_irfft_nodes", table, n, workspace, check_rc)


def fft_chirp_length(n):
    """The padded length P of the chirp-z transforms of n reals (the smallest 7-smooth number
    >= n - 1); 0 for an n they refuse (odd, below 4, above 2**30)."""
    return int(_lib.lib().dpz_fft_chirp_length(int(n)))


def fft_chirp_nodes_workspace(jobs, n, device, workspace=None):
    """A uint8 device tensor of ``dpz_fft_chirp_nodes_workspace_bytes(jobs, n)`` bytes
    (``workspace`` itself when it is large enough); ValueError for a size the chirp-z transforms
    refuse."""
    need = int(_lib.lib().dpz_fft_chirp_nodes_workspace_bytes(int(jobs), int(n)))
    if need < 0:
        raise ValueError(f"batched chirp-z real FFTs of n={n}: an even n in [4, 2**30] and "
                         "jobs >= 1")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    return workspace


def _fft_chirp_nodes(name, table, n, workspace, check_rc):
    _require(table.dev, torch.int64, "table")
    if workspace is None:
        need = int(_lib.lib().dpz_fft_chirp_nodes_workspace_bytes(table.m, int(n)))
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=table.dev.device)
    rc = getattr(_lib.lib(), name)(table.m, _ptr(table.dev),
                                   ctypes.c_void_p(table.host.ctypes.data), int(n),
                                   _ptr(workspace), workspace.numel(),
                                   _stream(table.dev.device))
    if check_rc:
        check(rc, name)
    return rc


def rfft_chirp_nodes(table, n, workspace=None, check_rc=True):
    """``rfft_nodes``' transforms of ``table`` (an ``FftNodesTable``) by the chirp-z algorithm:
    every even n in [4, 2**30], one launch set whatever the job count.  The results agree with
    ``rfft_nodes``' to rounding (not bit for bit); the x0 subtraction and the accumulating store
    round as ``elementwise(SUB)`` / ``elementwise(ADD)`` do.  ``workspace``:
    ``fft_chirp_nodes_workspace``'s tensor (allocated here when None)."""
    return _fft_chirp_nodes("dpz_rfft_chirp_nodes", table, n, workspace, check_rc)


def irfft_chirp_nodes(table, n, workspace=None, check_rc=True):
    """``irfft_nodes``' transforms of ``table`` (an ``IfftNodesTable``) by the chirp-z algorithm;
    the coefficients are only read."""
    return _fft_chirp_nodes("dpz_irfft_chirp_nodes", table, n, workspace, check_rc)


def cplx_chunk_elems():
    """Coefficients one block of ``cplx_encode_nodes``' count and compaction passes covers."""
    return int(_lib.lib().dpz_cplx_chunk_elems())


class CplxEncodeTable(_WordTable):
    """The node table of ``cplx_encode_nodes`` (a ``_WordTable``): 8 words per node {change, acc
    or 0, vals_src, key, counter or 0, pair_out, val_out, 0}.  Each argument is a 2-D tensor (one
    row per node) or a list of per-node tensors; ``acc`` and ``counter`` may be None."""

    def __init__(self, change, acc, vals_src, key, counter, pair_out, val_out, device):
        self.m = m = len(change)
        words, _ = self._words(8 * m)
        cols = (change, acc, vals_src, key, counter, pair_out, val_out, None)
        words[:8 * m] = np.array([_row_ptrs(c, m) for c in cols], dtype=np.uint64).T.reshape(-1)
        self._upload(device)


def cplx_encode_nodes(table, n, k, acc_mode=DPZ_ACC_NONE, workspace=None):
    """The FFT plugin's partial share of every node of ``table`` (a ``CplxEncodeTable``) in one
    launch set: the accumulation step of ``cplx_key`` on the n complex coefficients, the exact
    top-k of the fp32 key (ties to the lowest indices), and per selected coefficient i,
    ascending: ``pair_out = (2 i, 2 i + 1)``, ``val_out = vals_src[i]``, ``counter[i] += 1``,
    ``acc[i] = 0`` where the node has an accumulator.  Nothing is read back.  ``workspace``: a
    uint8 device tensor kept by the caller (allocated here when None); returned."""
    m, n, k = table.m, int(n), int(k)
    if not 1 <= k <= n:
        raise ValueError(f"k = {k} outside [1, n = {n}]")
    rows = table.host[:8 * m].reshape(m, 8)
    if (rows[:, [0, 2, 3, 5, 6]] == 0).any() or (acc_mode != DPZ_ACC_NONE
                                                 and (rows[:, 1] == 0).any()):
        raise ValueError("a node table with a null row: change, vals_src, key, pair_out and "
                         "val_out of every node, acc with an accumulating mode")
    if (rows[:, [0, 1, 2, 5, 6]] & 7).any() or (rows[:, [3, 4]] & 3).any():
        raise ValueError("a misaligned row: complex rows and pair_out on 8 bytes, key and "
                         "counter on 4")
    _require(table.dev, torch.int64, "table")
    return _encode_nodes("cplx", table.dev, m, n, (k, int(acc_mode)), workspace)


class QuantInfo:
    """The info record of a ``quant_encode``: what the pack kernel derived on the device."""

    __slots__ = ("status", "w", "padding", "scale", "norm", "max_abs", "abs_sum", "offset")

    def __init__(self, words):
        f = np.asarray(words, dtype=np.int32).view(np.float32)
        self.status, self.w, self.padding = int(words[0]), int(words[1]), int(words[2])
        self.scale, self.norm, self.max_abs, self.abs_sum = f[3], f[4], f[5], f[6]
        self.offset = int(np.asarray(words, dtype=np.int32).view(np.uint32)[7])


def quant_block_elems():
    """Values one block of the quantiser's pack kernel covers (the tests' edge sizes)."""
    return int(_lib.lib().dpz_quant_block_elems())


def _quant_ws(workspace, device, need):
    workspace = workspace or Workspace(device)
    buf = getattr(workspace, "qbuf", None)
    if buf is None or buf.numel() < max(need, 256):
        buf = workspace.qbuf = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return buf


def quant_encode(x, k, workspace=None):
    """The reference quantiser (compression/Quantization.py:28-91) of a device fp32 vector with
    ``float_precision`` k: ``(body, info)``, the packed stream body as a device uint8 tensor
    (4-byte aligned, exactly ceil(n * w / 8) bytes) and a :class:`QuantInfo`.  The statistics and
    the pack kernels run back to back; the one synchronisation is the read of the info record,
    which the caller's copy of the body needs anyway.  The body is allocated for the widest
    field k can give.  ValueError for an empty, all-zero or non-finite input and for k outside
    [1, 2^30]; TypeError for a k that is no int."""
    _require(x, torch.float32, "x")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"float_precision must be an int, got {type(k).__name__}")
    k = int(k)
    if not 1 <= k <= 2 ** 30:
        raise ValueError("float_precision must be in [1, 2^30]")
    x = x.reshape(-1)
    n = x.numel()
    if n < 1:
        raise ValueError("cannot quantise an empty array")
    ws = _quant_ws(workspace, x.device, int(_lib.lib().dpz_quant_workspace_bytes(n)))
    info_dev = torch.empty(8, dtype=torch.int32, device=x.device)
    # norm = fl(max / k) keeps max / norm within a few ulp of k: two bits above k's length,
    # except where norm is subnormal (status 4: once more with the full 32 bits)
    for w_cap in (min(32, k.bit_length() + 2), 32):
        cap = 4 * ((n * w_cap + 31) // 32)
        body = torch.empty(cap, dtype=torch.uint8, device=x.device)
        rc = _lib.lib().dpz_quant_encode(_ptr(x), n, k, _ptr(body), cap, _ptr(info_dev),
                                         _ptr(ws), ws.numel(), _stream(x.device))
        check(rc, "dpz_quant_encode")
        info = QuantInfo(info_dev.cpu().numpy())
        if info.status != 4:
            break
    if info.status == 1:
        raise ValueError("cannot quantise an all-zero array")
    if info.status == 2:
        raise ValueError("cannot quantise a non-finite array")
    if info.status != 0:
        raise ValueError("cannot quantise: max|x| / float_precision underflows")
    return body[:(n * info.w + 7) // 8], info


def quant_decode(body, n, w, scale, out=None):
    """Values of a quantised stream body held on the device (a uint8 tensor, 4-byte aligned,
    readable up to the next multiple of 4 bytes): ``float32(float64(u - 2^(w-1) + 1) * scale)``
    (compression/Quantization.py:93-132).  ``n``, ``w`` and ``scale`` come from the stream's
    header; nothing synchronises."""
    _require(body, torch.uint8, "body")
    n, w = int(n), int(w)
    if n < 1 or not 2 <= w <= 32 or 8 * body.numel() < n * w:
        raise ValueError("malformed quantised stream")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=body.device)
    _require(out, torch.float32, "out")
    if out.numel() < n:
        raise ValueError("out holds fewer than n values")
    nbytes = (n * w + 7) // 8
    store = body.untyped_storage()
    if body.storage_offset() + ((nbytes + 3) // 4) * 4 > store.nbytes():
        raise ValueError("body must be readable up to the next multiple of 4 bytes")
    rc = _lib.lib().dpz_quant_decode(_ptr(body), nbytes, n, w, float(scale), _ptr(out),
                                     _stream(body.device))
    if rc == _lib.DPZ_ERR_ARG:
        raise ValueError("malformed quantised stream")
    check(rc, "dpz_quant_decode")
    return out[:n]


QROW_INFO = 4   # int32 words of a packed quantised row in front of its info record
QROW_BODY = 12  # ... and in front of its body


def quant_row_words(n, slot_bits):
    """int32 words of a packed quantised row ``[count (int64), status, 0 | 8 info words | body]``
    whose body holds n fields of ``slot_bits`` bits."""
    words = int(_lib.lib().dpz_quant_row_words(int(n), int(slot_bits)))
    if not words:
        raise ValueError("n must lie in [1, 2^31) and slot_bits in [2, 32]")
    return words


def quant_node_table(x, rows):
    """The DEVICE node table of ``quant_encode_nodes``: 2 64-bit words per node {x, packed row}.
    Each argument is a 2-D tensor (one row per node) or a list of per-node tensors."""
    dev = (x if isinstance(x, torch.Tensor) else x[0]).device
    return _ptr_table((x, rows), len(x), dev)


def quant_encode_nodes(table, n, k, slot_bits, workspace=None):
    """``quant_encode`` of every node of ``table`` (``quant_node_table``) with float_precision k
    in two launches whatever the node count, each into its packed row: the info record and the
    body bit for bit the single call's, the row's status word = the info record's (1 all zero, 2
    non-finite, 3 underflow, 4 a field wider than ``slot_bits``; the body of such a row is not
    written).  Nothing is read back.  ``workspace``: a uint8 device tensor kept by the caller
    (allocated here when None); returned."""
    _require(table, torch.int64, "table")
    m = table.shape[0]
    need = int(_lib.lib().dpz_quant_encode_nodes_workspace_bytes(m, int(n)))
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=table.device)
    rc = _lib.lib().dpz_quant_encode_nodes(m, _ptr(table), int(n), int(k), int(slot_bits),
                                           _ptr(workspace), workspace.numel(),
                                           _stream(table.device))
    check(rc, "dpz_quant_encode_nodes")
    return workspace


def qdense_tile_elems(n_src):
    """The column tile of the staged quantised fold for ``n_src`` packed rows (0: direct only)."""
    return int(_lib.lib().dpz_qdense_tile_elems(int(n_src)))


def qdense_auto_mode(n_src, row_reads, n):
    """The path DPZ_DENSE_AUTO takes in ``qdense_average_nodes``."""
    return int(_lib.lib().dpz_qdense_auto_mode(int(n_src), int(row_reads), int(n)))


class QDenseTable(_WordTable):
    """The fold table of ``qdense_average_nodes`` (a ``_WordTable``), with the counts the call
    repeats."""

    def __init__(self, srcs, recvs, device):
        """srcs: the packed rows (a 2-D int32 tensor or a list of 1-D tensors); recvs: per
        receiver ``(out row, own fp32 row, w_self, [(source index, weight), ...])`` in fold
        order.  Weights are Python floats, rounded to fp32 here as torch rounds a scalar."""
        src_ptrs = _row_ptrs(srcs, srcs.shape[0] if isinstance(srcs, torch.Tensor) else len(srcs))
        self.n_src, self.m = len(src_ptrs), len(recvs)
        self.n_entries = sum(len(r[3]) for r in recvs)
        words, halves = self._words(self.n_src + 4 * self.m + self.n_entries)
        words[:self.n_src] = src_ptrs
        ent = self.n_src + 4 * self.m
        start = 0
        for j, (out, own, w_self, pairs) in enumerate(recvs):
            b = self.n_src + 4 * j
            words[b], words[b + 1] = out.data_ptr(), own.data_ptr()
            halves[2 * b + 4] = _f32_bits(w_self)
            halves[2 * b + 6:2 * b + 8] = (start, len(pairs))
            for src, w in pairs:
                halves[2 * (ent + start):2 * (ent + start) + 2] = (_i32_bits(src), _f32_bits(w))
                start += 1
        self._upload(device)


def qdense_average_nodes(table, n, cap_dwords, mode=_lib.DPZ_DENSE_AUTO, guard=None,
                         check_rc=True):
    """Every receiver's fold of ``table`` (a ``QDenseTable``) in one launch: the dense fold of
    ``dense_average_nodes`` over sources that are packed quantised rows, each decoded with the
    width and scale of its own header as ``quant_decode`` decodes it; every row holds
    ``cap_dwords`` body dwords.  ``guard`` (int32 device words, e.g. the rows' status words): if
    any is nonzero every out row becomes a bitwise copy of its own row.  Returns the library's
    code (raises unless it is DPZ_OK when ``check_rc``)."""
    _require(table.dev, torch.int64, "table")
    _require(guard, torch.int32, "guard")
    rc = _lib.lib().dpz_qdense_average_nodes(
        table.m, _ptr(table.dev), ctypes.c_void_p(table.host.ctypes.data), table.n_entries,
        table.n_src, int(n), int(cap_dwords), int(mode), _ptr(guard),
        guard.numel() if guard is not None else 0, _stream(table.dev.device))
    if check_rc:
        check(rc, "dpz_qdense_average_nodes")
    return rc


class KernelTimer:
    """Per-kernel device time measured by the library with HIP event pairs on each launch's own
    stream (``dpz_timing_*``).  Launches into a capturing stream are not timed.

    >>> with KernelTimer() as t:
    ...     topk_encode(...)
    >>> t.result  # {"topk_filter": (ms_total, launches), ...}
    """

    N_MAX = 64

    def __enter__(self):
        _lib.lib().dpz_timing_enable(1)
        self.result = {}
        return self

    def __exit__(self, *exc):
        self.result = self.read()
        _lib.lib().dpz_timing_enable(0)
        return False

    @classmethod
    def read(cls):
        ms = (ctypes.c_double * cls.N_MAX)()
        cnt = (ctypes.c_int64 * cls.N_MAX)()
        nk = _lib.lib().dpz_timing_read(ms, cnt, cls.N_MAX)
        out = {}
        for i in range(min(nk, cls.N_MAX)):
            if cnt[i]:
                out[_lib.lib().dpz_kernel_name(i).decode()] = (ms[i], int(cnt[i]))
        return out
