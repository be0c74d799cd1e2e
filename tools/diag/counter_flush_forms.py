"""Diagnostic: the time of every form of the ring flush (dpz_counter_flush: scatter, dense sweep,
sparse sectors) by HIP events around back-to-back flushes, at n = 2^24 and 11,000,000 with
k = n / 100, for 1..64 rounds in the ring, on (a) independent random rounds and (b) identical
rounds (what a benchmark that re-encodes unchanged tensors produces); and at k = n / 10 on
independent rounds (up to 6.4 entries per counter: where the dense sweep is due).  The flushes
rotate over COUNTERS counters with a ring each, so that neither sits in the 256 MiB Infinity
Cache.  Also times 2 and COUNTERS counters flushed by one dpz_counter_flush_batch call in every
form, and by single calls (us is then the time for all of them).

One JSON line per measurement on stdout and in --out (default profiles/counter_flush_forms.jsonl).
``--also name=mode`` times a further mode number of an experimental build."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from decentralizepy_amd import _lib  # noqa: E402

COUNTERS = 8
SIZES = (2 ** 24, 11_000_000)
# (n / k, rounds in the ring, inputs)
CASES = ((100, (1, 2, 3, 4, 8, 16, 33, 64), ("independent", "identical")),
         (10, (4, 16, 64), ("independent",)))
BATCHES = (2, COUNTERS)
FLUSHES = 16  # back-to-back flushes per timed loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "counter_flush_forms.jsonl"))
    ap.add_argument("--also", action="append", default=[])
    args = ap.parse_args()
    forms = {"scatter": _lib.DPZ_COUNTER_SCATTER, "sweep": _lib.DPZ_COUNTER_SWEEP,
             "sparse": _lib.DPZ_COUNTER_SPARSE, "auto": _lib.DPZ_COUNTER_AUTO}
    for a in args.also:
        name, mode = a.split("=")
        forms[name] = int(mode)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.lib()
    st = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(st.cuda_stream)
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def timed(call):
        """Median and min over 3 loops of FLUSHES calls, in us per call."""
        call(0)
        torch.cuda.synchronize()
        res = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for i in range(FLUSHES):
                call(i)
            e1.record(st)
            e1.synchronize()
            res.append(e0.elapsed_time(e1) * 1e3 / FLUSHES)
        res.sort()
        return round(res[1], 2), round(res[0], 2)

    for n, (div, rounds, inputs) in ((n, c) for n in SIZES for c in CASES):
        k = n // div
        g = torch.Generator(device=dev).manual_seed(n % 1000 + div)
        counters = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(COUNTERS)]
        need = int(L.dpz_counter_flush_workspace_bytes(n))
        wss = [torch.empty(need, dtype=torch.uint8, device=dev) for _ in range(COUNTERS)]
        rnd = torch.stack([torch.randperm(n, device=dev, generator=g)[:k].sort().values
                           .to(torch.int32) for _ in range(max(rounds))])
        rings = {"independent": [rnd.clone().view(-1) for _ in range(COUNTERS)],
                 "identical": [rnd[:1].repeat(max(rounds), 1).view(-1) for _ in range(COUNTERS)]}
        for inp in inputs:
            rr = rings[inp]
            for r in rounds:
                offs = (ctypes.c_int64 * (r + 1))(*[i * k for i in range(r + 1)])
                for name, mode in forms.items():
                    def one(i, mode=mode):
                        c = i % COUNTERS
                        rc = L.dpz_counter_flush(counters[c].data_ptr(), n, rr[c].data_ptr(), offs,
                                                 r, mode, wss[c].data_ptr(), need, sp)
                        assert rc == 0, rc
                    med, best = timed(one)
                    emit(dict(n=n, k=k, rounds=r, input=inp, form=name, us=med, us_min=best))
                # a region's end: B counters flushed once each, by single calls and by one batch
                for B in BATCHES:
                    def item(c):
                        return _lib.CounterItem(counters[c].data_ptr(), n, rr[c].data_ptr(), offs,
                                                r, wss[c].data_ptr(), need)
                    # (the counters of consecutive calls differ: i * B .. i * B + B - 1)
                    tabs = [(_lib.CounterItem * B)(*[item((i * B + c) % COUNTERS)
                                                     for c in range(B)])
                            for i in range(COUNTERS // B)]

                    def singles(i):
                        for c in range(B):
                            c = (i * B + c) % COUNTERS
                            L.dpz_counter_flush(counters[c].data_ptr(), n, rr[c].data_ptr(), offs,
                                                r, _lib.DPZ_COUNTER_AUTO, wss[c].data_ptr(), need,
                                                sp)

                    med, best = timed(singles)
                    emit(dict(n=n, k=k, rounds=r, input=inp, form="auto_x%d_single_calls" % B,
                              us=med, us_min=best))
                    for name, mode in forms.items():
                        def batch(i, mode=mode):
                            rc = L.dpz_counter_flush_batch(tabs[i % len(tabs)], B, mode, sp)
                            assert rc == 0, rc
                        med, best = timed(batch)
                        emit(dict(n=n, k=k, rounds=r, input=inp,
                                  form="%s_x%d_one_batch" % (name, B), us=med, us_min=best))
        del counters, wss, rings, rnd
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
