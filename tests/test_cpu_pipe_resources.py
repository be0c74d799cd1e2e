"""Compiler-reported resources of the merged step kernel (pipe_step_kernel, dpz_topk_sampled.hip).
Its filter, select and compact parts overlay one LDS arena, so the kernel needs no more LDS than
its largest part and its registers allow at least 5 blocks per CU; as three sets of function-local
arrays the parts' LDS added up to 38.8 KB and the kernel was LDS-bound at 4.  Reads the remarks
of -Rpass-analysis=kernel-resource-usage only: no GPU, nothing is run."""
import os
import re
import shlex
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "decentralizepy_amd", "csrc")
SRC = "dpz_topk_sampled.hip"
# Itanium-mangled prefixes of the stand-alone kernels whose parts the merged kernel runs, with
# their LDS bytes per block before the parts' LDS became structs (never to grow)
FILTER = "_ZN3dpz26sampled_filter_pipe_kernelILi1ELi1ELi4ELi4ELb1EEE"   # <1, 1, 4, 4, true>
SELECT = "_ZN3dpz21sampled_select_kernelILb1EEE"                        # <true>
COMPACT = "_ZN3dpz22sampled_compact_kernelILb1ELb0ELi2ELb0EEE"          # <true, false, 2, false>
LDS_BEFORE = {FILTER: 16480, SELECT: 12404, COMPACT: 9968}
PIPE = "_ZN3dpz16pipe_step_kernelI"


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of one device-only compile with the Makefile's
    own command line."""
    dry = subprocess.run(["make", "-C", CSRC, "-n", "-B", "dpz_topk_sampled.o"],
                         capture_output=True, text=True, check=True).stdout
    line = next(ln for ln in dry.splitlines() if "-c -o dpz_topk_sampled.o" in ln)
    cmd = shlex.split(line)
    obj = str(tmp_path_factory.mktemp("pipe_resources") / "dpz_topk_sampled.o")
    cmd[cmd.index("-o") + 1] = obj
    cmd += ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = blk.split()[0]
        out[name] = {m.group(1).strip(): int(m.group(2))
                     for m in re.finditer(r"remark: +([A-Za-z][^:\n]*): (\d+) \[-Rpass", blk)}
    return out


def _one(remarks, prefix):
    hits = [v for k, v in remarks.items() if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, len(hits))
    return hits[0]


def test_standalone_kernels_lds_did_not_grow(remarks):
    for prefix, before in LDS_BEFORE.items():
        lds = _one(remarks, prefix)["LDS Size [bytes/block]"]
        print(prefix, "LDS", lds, "before", before)
        assert lds <= before


def test_merged_kernel_overlays_its_parts(remarks):
    largest = max(_one(remarks, p)["LDS Size [bytes/block]"] for p in LDS_BEFORE)
    pipes = {k: v for k, v in remarks.items() if k.startswith(PIPE)}
    assert len(pipes) >= 2  # a launch with a filter part, and the drain
    for name, v in pipes.items():
        print(name[:48], v)
        assert v["ScratchSize [bytes/lane]"] == 0
        assert v["VGPRs Spill"] == 0
        assert v["Occupancy [waves/SIMD]"] >= 5
        assert v["LDS Size [bytes/block]"] <= largest + 64
