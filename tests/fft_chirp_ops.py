"""The numpy side of the chirp-z real FFTs (dpz_rfft_chirp_nodes / dpz_irfft_chirp_nodes) - TEST
INFRASTRUCTURE ONLY: the padded length's rule restated, the fixed-seed inputs with their float64
references, ``emu_rfft`` / ``emu_irfft``, an fp32 restatement of the algorithm on the CPU (a
float64 chirp rounded to complex64, torch's CPU complex64 fft / ifft of the padded length, a Bhat
rounded from float64, the even-n pairing in complex64), and the loader of the recorded reference
run of a size without a native plan (tests/golden/make_golden_fft_round_chirp.py).

Accuracy.  E(y) = ||y - ref||_2 / ||ref||_2 against numpy's float64 transform of the same fp32
input; E_ref is that figure for torch's CPU fp32 transform at n, E_emu for the restatement.  The
bound is E <= 4 max(E_ref, E_emu, eps): 4 is the project's factor for two fp32 O(log n) algorithms
whose twiddles are products of two rounded table entries; nothing is summed directly, so there is
no D term."""
import functools
import json
import os

import numpy as np
import torch

from tests import fft_round_ops

EPS = float(np.finfo(np.float32).eps)
c64, c128 = np.complex64, np.complex128
# even n in 4..200: L = 2 and 3 (P = 3, 5), P = 2 L - 1 exactly (n = 4, 6, 8, 10, 16, 22, ...),
# P one above it (n = 12, 14, 18, 20, ...), gaps up to 4 (n = 66: P = 70), one-pass P throughout
SWEEP = list(range(4, 201, 2))
FORCED = [1030, 4100, 8186]                # native sizes forced through the chirp path
NO_PLAN = [8198, 16_396, 24_594, 89_834]   # 2 * 4,099, 4 * 4,099, 6 * 4,099, 2 * 44,917 (LeNet)
SIZES = SWEEP + FORCED + NO_PLAN
STRUCTURED = [8198, 89_834]
FLAT_C = 0.75


def chirp_length(n):
    """The rule of dpz_fft_chirp_length restated: the smallest 7-smooth number >= n - 1 for an
    even n in [4, 2^30], else 0."""
    if n < 4 or n % 2 or n > 1 << 30:
        return 0
    p = n - 1
    while True:
        q = p
        for f in (2, 3, 5, 7):
            while q % f == 0:
                q //= f
        if q == 1:
            return p
        p += 1


def is_prime(q):
    return q >= 2 and all(q % f for f in range(2, int(q ** 0.5) + 1))


def rel(y, ref):
    y, ref = np.asarray(y), np.asarray(ref)
    wide = c128 if np.iscomplexobj(ref) else np.float64
    return float(np.linalg.norm(y.astype(wide) - ref) / np.linalg.norm(ref))


def bound(*errs):
    return 4 * max(max(errs), EPS)


def _ro(a):
    a.setflags(write=False)
    return a


# ---- the fp32 restatement -------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def tables(n, P):
    """(w, Bhat, W_n) in complex64: w_j = exp(-i pi (j^2 mod 2 L) / L), Bhat = DFT_P of the
    conjugate chirp wrapped to length P (float64, rounded once), W_n^k for k <= L."""
    L = n // 2
    j = np.arange(L, dtype=np.int64)
    w = np.exp(-1j * np.pi * ((j * j) % (2 * L)) / L)
    b = np.zeros(P, c128)
    b[:L] = w.conj()
    b[P - L + 1:] = w.conj()[1:][::-1]
    k = np.arange(L + 1, dtype=np.int64)
    return (_ro(w.astype(c64)), _ro(np.fft.fft(b).astype(c64)),
            _ro(np.exp(-2j * np.pi * k / n).astype(c64)))


def _conv(a, bhat, P, L):
    """The cyclic convolution with the chirp through torch's CPU complex64 transforms."""
    pad = np.zeros(P, c64)
    pad[:L] = a
    spec = torch.fft.fft(torch.from_numpy(pad)).numpy() * bhat
    return torch.fft.ifft(torch.from_numpy(spec.astype(c64))).numpy()[:L]


def emu_rfft(x, P):
    x = np.asarray(x, np.float32)
    n, L = x.size, x.size // 2
    w, bhat, wn = tables(n, P)
    z = (x[0::2] + 1j * x[1::2]).astype(c64)
    Z = (_conv((z * w).astype(c64), bhat, P, L) * w).astype(c64)
    Zk = np.concatenate([Z, Z[:1]])
    Zm = Zk[::-1].conj()
    return (c64(0.5) * ((Zk + Zm) - c64(1j) * wn * (Zk - Zm))).astype(c64)


def emu_irfft(spec, n, P):
    X = np.array(spec, c64)
    L = n // 2
    w, bhat, wn = tables(n, P)
    X[0], X[L] = X[0].real, X[L].real
    Xm = X[::-1].conj()
    Z = ((X + Xm) + c64(1j) * wn.conj() * (X - Xm)).astype(c64)[:L]
    y = _conv((Z * w.conj()).astype(c64), bhat.conj(), P, L)
    z = ((y * w.conj()).astype(c64) * np.float32(1.0 / n)).astype(c64)
    out = np.empty(n, np.float32)
    out[0::2], out[1::2] = z.real, z.imag
    return out


# ---- inputs with their references, computed once per size and read-only -----------------------------
@functools.lru_cache(maxsize=None)
def random_case(n):
    """tests/test_gpu_fft_conformance.random_case's recipe (seed 7000 + n) with the restatement's
    errors beside the reference transform's."""
    g = torch.Generator().manual_seed(7000 + n)
    x = torch.randn(n, generator=g)
    m = n // 2 + 1
    spec = torch.complex(torch.randn(m, generator=g), torch.randn(m, generator=g))
    x64 = x.numpy().astype(np.float64)
    fwd = np.fft.rfft(x64)
    inv = np.fft.irfft(spec.numpy().astype(c128), n)
    t_fwd = torch.fft.rfft(x)
    P = chirp_length(n)
    e_fwd = emu_rfft(x.numpy(), P)
    return {
        "x": _ro(x.numpy().copy()), "x64": _ro(x64), "fwd": _ro(fwd),
        "spec": _ro(spec.numpy().copy()), "inv": _ro(inv),
        "ref": {"fwd": rel(t_fwd.numpy(), fwd),
                "inv": rel(torch.fft.irfft(spec, n).numpy(), inv),
                "rt": rel(torch.fft.irfft(t_fwd, n).numpy(), x64)},
        "emu": {"fwd": rel(e_fwd, fwd), "inv": rel(emu_irfft(spec.numpy(), n, P), inv),
                "rt": rel(emu_irfft(e_fwd, n, P), x64)},
    }


def structured(n):
    """(name, x fp32) of the unit impulses at j in {0, 1, n/3, n/2, n - 1} and the tones
    cos(2 pi f j / n + 0.3), f in {1, n/3, n/2}."""
    j = np.arange(n, dtype=np.int64)
    for at in sorted({0, 1, n // 3, n // 2, n - 1}):
        x = np.zeros(n, np.float32)
        x[at] = 1.0
        yield f"impulse{at}", x
    for f in sorted({1, n // 3, n // 2}):
        yield f"tone{f}", np.cos(2 * np.pi * ((f * j) % n) / n + 0.3).astype(np.float32)


def flat_errors(got, ref):
    """(error of the DC bin, max-abs error of the other bins)."""
    err = np.abs(np.asarray(got).astype(c128) - ref)
    return float(err[0]), float(err[1:].max())


# ---- the recorded reference run -------------------------------------------------------------------
def load_run():
    """(meta, arrays) of ``chirp4``, ``acc_enc`` rebuilt as fft_round_ops.load_runs does."""
    with open(os.path.join(fft_round_ops.GOLDEN, "fft_round_chirp.json")) as f:
        (m,) = json.load(f)["runs"]
    arr = dict(np.load(os.path.join(fft_round_ops.GOLDEN, f"fft_round_{m['name']}.npz"),
                       allow_pickle=False))
    for r in range(m["rounds"]):
        base = arr[f"r{r - 1}_acc_avg"] if r else np.zeros_like(arr["r0_acc_avg"])
        arr[f"r{r}_acc_enc"] = fft_round_ops.patched(base, arr.pop(f"r{r}_acc_enc_at"),
                                                     arr.pop(f"r{r}_acc_enc_val"))
    return m, arr
