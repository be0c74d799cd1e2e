"""GPU: the native real FFTs (csrc/dpz_fft.hip, dpz_rfft / dpz_irfft) held to the accuracy of the
reference's own fp32 transform (torch's CPU pocketfft) at small sizes that reach every planner
branch, element-wise on structured inputs, and to the contract include/dpz_codec.h states.

Accuracy.  E(y) = ||y - ref||_2 / ||ref||_2 against a float64 numpy transform of the same fp32
input; E_ref is the same figure for torch's CPU fp32 transform, computed here.  The bound is
    E <= 4 * max(E_ref, eps) + D,      D = 2 * eps * sqrt(q_max)
with q_max the largest prime factor >= 17 of the complex length (n / 2 for even n, n for odd;
D = 0 without one).  4: both are fp32 O(log n) algorithms, and the native twiddle is the fp32
product of two rounded table entries where pocketfft uses one.  D: such a prime is summed
directly in fp32 (ft_sub_any); a recursive sum of q terms has an expected rms error of about
0.7 eps sqrt(q) and a worst case of q eps, so D is about 3x the expectation.

Impulses.  Every output of the transform of a unit impulse is one root of unity: a chain of at
most one twiddle multiply per sub-pass, per pass and for the even-n pairing, each costing at most
about 4 eps, the additions adding (near) zeros: max-abs error <= 4 eps (ceil(log2 n) + 2).  The
inverse of a unit spectrum is c / n * cos(2 pi j k / n) (c = 1 at DC / Nyquist, else 2); the same
bound is applied to the error relative to that amplitude c / n (taken absolutely it would be n / 2
times looser than the forward one).

Constant and alternating vectors of amplitude c: the peak bin (DC / Nyquist, n * c) within the
random-input bound of n * c, every other bin within
    (4 * max(E_ref, r / ||x||_2, eps) + D) * ||x||_2,
r being the largest other-bin error of torch's CPU transform of the same vector.  Without r this
is the random-input bound times ||x||_2, which assumes the rounding error spreads evenly over the
bins as it does for random input.  For a constant column every butterfly of a radix 5 / 7 / 11 /
13 stage leaves the same residue (the rounded cosines do not sum to -1/2 exactly), so the error
is coherent and lands in a few bins: pocketfft itself exceeds the even-spread figure 24x at
n = 449,878, 13x at 60,060, 5.7x at 393,216 (the native kernels 36x, 8x and 0: radix 2 / 4 / 8 and
3 butterflies of equal inputs give exact zeros).  The term therefore tracks the reference's own
other-bin error in the same 4x form and equals the even-spread one wherever the reference meets
it.  An odd n has no Nyquist bin: the alternating vector's spectrum 2 c / (1 + W_n^k) is then
broadband with entries of order n * c, so there every bin is held to the random-input bound times
||ref||_2.

Measured on an MI355X: DESIGN.md section 3.7 (the table of E, E_ref and the impulse errors).  A
plain fp32 sum in ft_sub_any missed the tone bound at the sizes with the prime 2053 (f = n // 2,
a constant complex column: E = 108-127 eps against 97-100 allowed); the sum is compensated now.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)

SWEEP = list(range(2, 67))
# n: (plan of the complex length as passes R[sub-radices], native)
TARGETED = {
    272: ("136[17,8]", True), 442: ("221[17,13]", True), 510: ("255[17,5,3]", True),
    289: ("17, 17", True), 514: ("257", True), 771: ("257, 3", True),
    131_584: ("257, 256[8,8,4]", True), 4106: ("2053", True), 6159: ("2053, 3", True),
    65_696: ("2053, 16[8,2]", True), 4093: ("4093", True), 8186: ("4093", True),
    4099: ("hipFFT", False), 8198: ("hipFFT", False),
    1000: ("250[5,5,5,2], 2", True), 1024: ("256[8,8,4], 2", True),
    65_536: ("256[8,8,4], 128[8,8,2]", True), 393_216: ("192[3,8,8], 256[8,8,4], 4", True),
    39_366: ("243[3^5], 81[3^4]", True), 31_250: ("125[5,5,5], 125[5,5,5]", True),
    33_614: ("49[7,7], 49[7,7], 7", True), 449_878: ("169[13,13], 121[11,11], 11", True),
    60_060: ("143[13,11], 210[7,5,3,2]", True), 2187: ("243[3^5], 9[3,3]", True),
    3125: ("125[5,5,5], 25[5,5]", True), 15_015: ("143[13,11], 105[7,5,3]", True),
}
SIZES = SWEEP + list(TARGETED)
# contract tests: even native, odd native, hipFFT
CONTRACT = [30, 1000, 8186, 60_060, 33, 289, 6159, 15_015, 4099, 8198]
KNOB_SIZES = [510, 1000, 8186, 33_614, 60_060]


def native(n):
    return TARGETED.get(n, ("", True))[1]


def q_max(n):
    """The largest prime factor >= 17 of the complex length (0 if none)."""
    m, q, f = (n // 2 if n % 2 == 0 else n), 0, 2
    while f * f <= m:
        while m % f == 0:
            q, m = f, m // f
        f += 1
    q = max(q, m) if m > 1 else q
    return q if q >= 17 else 0


def bound(e_ref, n):
    return 4 * max(e_ref, EPS) + 2 * EPS * math.sqrt(q_max(n))


def impulse_bound(n):
    return 4 * EPS * (math.ceil(math.log2(n)) + 2)


def rel(y, ref):
    y, ref = np.asarray(y), np.asarray(ref)
    wide = np.complex128 if np.iscomplexobj(ref) else np.float64
    return float(np.linalg.norm(y.astype(wide) - ref) / np.linalg.norm(ref))


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_case(n):
    """Fixed-seed inputs of size n with their float64 references and the reference transform's
    own errors (computed once per size, read-only)."""
    g = torch.Generator().manual_seed(7000 + n)
    x = torch.randn(n, generator=g)
    m = n // 2 + 1
    spec = torch.complex(torch.randn(m, generator=g), torch.randn(m, generator=g))
    x64 = x.numpy().astype(np.float64)
    fwd = np.fft.rfft(x64)
    inv = np.fft.irfft(spec.numpy().astype(np.complex128), n)
    t_fwd = torch.fft.rfft(x)
    return {
        "x": _ro(x.numpy().copy()), "x64": _ro(x64), "fwd": _ro(fwd),
        "spec": _ro(spec.numpy().copy()), "inv": _ro(inv),
        "e_fwd": rel(t_fwd.numpy(), fwd),
        "e_inv": rel(torch.fft.irfft(spec, n).numpy(), inv),
        "e_rt": rel(torch.fft.irfft(t_fwd, n).numpy(), x64),
    }


def dev_rfft(a, dev, **kw):
    from decentralizepy_amd import codec
    return codec.rfft(torch.tensor(a).to(dev), **kw).cpu().numpy()


def dev_irfft(a, n, dev, **kw):
    from decentralizepy_amd import codec
    return codec.irfft(torch.tensor(a).to(dev), n, **kw).cpu().numpy()


def random_errors(n, dev):
    """(E, E_ref) of rfft, irfft and the round trip on the random case of size n."""
    c = random_case(n)
    f = dev_rfft(c["x"], dev)
    return {"fwd": (rel(f, c["fwd"]), c["e_fwd"]),
            "inv": (rel(dev_irfft(c["spec"], n, dev), c["inv"]), c["e_inv"]),
            "rt": (rel(dev_irfft(f, n, dev), c["x64"]), c["e_rt"])}


def tones(n):
    j = np.arange(n, dtype=np.int64)
    for f in sorted({1, n // 3, n // 2}):
        yield f, np.cos(2 * np.pi * ((f * j) % n) / n + 0.3).astype(np.float32)


def tone_errors(n, dev):
    out = {}
    for f, x in tones(n):
        ref = np.fft.rfft(x.astype(np.float64))
        out[f] = (rel(dev_rfft(x, dev), ref), rel(torch.fft.rfft(torch.from_numpy(x)).numpy(), ref))
    return out


def impulse_errors(n, dev):
    """max-abs error of rfft(delta_j) against W_n^{jk}, per j."""
    k = np.arange(n // 2 + 1, dtype=np.int64)
    out = {}
    for j in sorted({0, 1, n // 3, n // 2, n - 1}):
        x = np.zeros(n, np.float32)
        x[j] = 1.0
        want = np.exp(-2j * np.pi * ((j * k) % n) / n)
        out[j] = float(np.abs(dev_rfft(x, dev).astype(np.complex128) - want).max())
    return out


def inverse_impulse_errors(n, dev):
    """max-abs error of irfft(unit spectrum at bin k), relative to its amplitude c / n, per k."""
    j = np.arange(n, dtype=np.int64)
    out = {}
    for k in sorted({0, 1, n // 4, n // 2}):
        spec = np.zeros(n // 2 + 1, np.complex64)
        spec[k] = 1.0
        amp = (1.0 if k == 0 or 2 * k == n else 2.0) / n
        want = amp * np.cos(2 * np.pi * ((j * k) % n) / n)
        out[k] = float(np.abs(dev_irfft(spec, n, dev).astype(np.float64) - want).max() / amp)
    return out


FLAT_C = 0.75  # n * c is exact in fp32 up to the largest n


def flat_vectors(n):
    """(name, x, float64 spectrum, peak bin) of the constant and the alternating-sign vector; the
    peak bin holds n * c and every other bin 0 (None for odd-n alternating: no Nyquist bin)."""
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    for name, x64 in (("constant", np.full(n, FLAT_C)), ("alternating", FLAT_C * sign)):
        if name == "alternating" and n % 2 == 1:
            yield name, x64, np.fft.rfft(x64), None
            continue
        ref = np.zeros(n // 2 + 1, np.complex128)
        peak = 0 if name == "constant" else n // 2
        ref[peak] = n * FLAT_C
        yield name, x64, ref, peak


def flat_errors(got, ref, peak):
    """(error of the peak bin, max-abs error of the other bins)."""
    err = np.abs(got - ref)
    if peak is None:
        return 0.0, float(err.max())
    rest = np.ones(err.shape, bool)
    rest[peak] = False
    return float(err[peak]), float(err[rest].max()) if rest.any() else 0.0


@pytest.mark.parametrize("n", SIZES)
def test_native_flag(dev, n):
    from decentralizepy_amd import _lib
    assert _lib.lib().dpz_fft_native(n) == int(native(n))


@pytest.mark.parametrize("n", SIZES)
def test_random_accuracy(dev, n):
    """rfft, irfft of an arbitrary spectrum and the round trip: E <= 4 max(E_ref, eps) + D."""
    errs = random_errors(n, dev)
    print({k: (e / EPS, r / EPS, bound(r, n) / EPS) for k, (e, r) in errs.items()})
    for what, (e, e_ref) in errs.items():
        assert e <= bound(e_ref, n), (what, n, e / EPS, e_ref / EPS)


@pytest.mark.parametrize("n", SIZES)
def test_tone_accuracy(dev, n):
    """cos(2 pi f j / n + 0.3), f in {1, n // 3, n // 2}: the same bound."""
    errs = tone_errors(n, dev)
    print({f: (e / EPS, r / EPS, bound(r, n) / EPS) for f, (e, r) in errs.items()})
    for f, (e, e_ref) in errs.items():
        assert e <= bound(e_ref, n), (f, n, e / EPS, e_ref / EPS)


@pytest.mark.parametrize("n", SIZES)
def test_impulses(dev, n):
    errs = impulse_errors(n, dev)
    print({j: e / EPS for j, e in errs.items()}, impulse_bound(n) / EPS)
    for j, e in errs.items():
        assert e <= impulse_bound(n), (j, n, e / EPS)


@pytest.mark.parametrize("n", SIZES)
def test_inverse_impulses(dev, n):
    errs = inverse_impulse_errors(n, dev)
    print({k: e / EPS for k, e in errs.items()}, impulse_bound(n) / EPS)
    for k, e in errs.items():
        assert e <= impulse_bound(n), (k, n, e / EPS)


@pytest.mark.parametrize("n", SIZES)
def test_constant_and_alternating(dev, n):
    e_rand = random_case(n)["e_fwd"]
    for name, x64, ref, peak in flat_vectors(n):
        x32 = x64.astype(np.float32)
        got = dev_rfft(x32, dev).astype(np.complex128)
        e_peak, e_rest = flat_errors(got, ref, peak)
        if peak is None:
            b = bound(e_rand, n) * np.linalg.norm(ref)
            print(name, n, e_rest / b)
            assert e_rest <= b, (name, n, e_rest, b)
            continue
        nx = np.linalg.norm(x64)
        tor = torch.fft.rfft(torch.from_numpy(x32)).numpy().astype(np.complex128)
        r_rest = flat_errors(tor, ref, peak)[1]
        b_peak, b_rest = bound(e_rand, n) * n * FLAT_C, bound(max(e_rand, r_rest / nx), n) * nx
        print(name, n, e_peak / b_peak, e_rest / b_rest, "reference's other bins",
              r_rest / (bound(e_rand, n) * nx))
        assert e_peak <= b_peak, (name, n, e_peak, b_peak)
        assert e_rest <= b_rest, (name, n, e_rest, b_rest)


# ---- contract ------------------------------------------------------------------------------------

def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("n", CONTRACT)
def test_guards_and_inputs_untouched(dev, n):
    """out as a view inside a sentinel-filled tensor: nothing before it or past its n / 2 + 1
    (rfft) / n (irfft) elements is written, the result equals a plain call's, x is not written,
    and coeffs is not written by the native irfft.  Odd native sizes take the real vectors at an
    odd float offset (only even n reads them as pairs)."""
    from decentralizepy_amd import codec
    c = random_case(n)
    m = n // 2 + 1
    g = 65 if (native(n) and n % 2) else 64
    xbase = torch.full((g + n + g,), -77.0, device=dev)
    x = xbase[g:g + n]
    x.copy_(torch.tensor(c["x"]))
    xb0 = _bits(xbase)
    plain = _bits(codec.rfft(x.clone()))
    sent = complex(1234.5, -6789.25)
    obase = torch.full((64 + m + 64,), sent, dtype=torch.complex64, device=dev)
    codec.rfft(x, out=obase[64:64 + m])
    ob = _bits(obase)
    want = np.array([sent], np.complex64).view(np.uint64)[0]
    assert (ob[:64] == want).all() and (ob[64 + m:] == want).all()
    np.testing.assert_array_equal(ob[64:64 + m], plain)
    np.testing.assert_array_equal(_bits(xbase), xb0)

    spec = torch.tensor(c["spec"]).to(dev)
    sb0 = _bits(spec)
    plain = _bits(codec.irfft(spec.clone(), n))
    rbase = torch.full((g + n + g,), -4321.5, device=dev)
    codec.irfft(spec, n, out=rbase[g:g + n])
    rb = _bits(rbase)
    want = np.array([-4321.5], np.float32).view(np.uint32)[0]
    assert (rb[:g] == want).all() and (rb[g + n:] == want).all()
    np.testing.assert_array_equal(rb[g:g + n], plain)
    if native(n):
        np.testing.assert_array_equal(_bits(spec), sb0)


@pytest.mark.parametrize("n", CONTRACT)
def test_nan_prefilled_out_and_work_area(dev, n):
    """out and the caller's work area may hold anything on entry."""
    from decentralizepy_amd import codec
    c = random_case(n)
    x = torch.tensor(c["x"]).to(dev)
    ws = codec.Workspace(dev)
    codec.rfft(x, workspace=ws)  # allocates ws.fbuf
    res = []
    for fill in (0, 255):  # 0xFF bytes: NaN as fp32
        ws.fbuf.fill_(fill)
        v = math.nan if fill else 0.0
        out = torch.full((n // 2 + 1,), complex(v, v), dtype=torch.complex64, device=dev)
        f = _bits(codec.rfft(x, out=out, workspace=ws))
        ws.fbuf.fill_(fill)
        spec = torch.tensor(c["spec"]).to(dev)
        back = torch.full((n,), v, device=dev)
        res.append((f, _bits(codec.irfft(spec, n, out=back, workspace=ws))))
    np.testing.assert_array_equal(res[1][0], res[0][0])
    np.testing.assert_array_equal(res[1][1], res[0][1])
    assert not np.isnan(res[1][1].view(np.float32)).any()


@pytest.mark.parametrize("n1,n2", [(1000, 289), (60_060, 15_015), (8186, 6159), (30, 33),
                                   (8198, 4099)])
def test_repeatable_through_one_workspace(dev, n1, n2):
    """n1, n2, n1 (even, odd, even) through one Workspace: the third result is the first's, bit
    for bit (twiddle cache, work-area reuse), and so is an immediate repeat."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)

    def both(n):
        c = random_case(n)
        f = _bits(codec.rfft(torch.tensor(c["x"]).to(dev), workspace=ws))
        b = _bits(codec.irfft(torch.tensor(c["spec"]).to(dev), n, workspace=ws))
        return f, b

    first, again = both(n1), both(n1)
    both(n2)
    third = both(n1)
    for a, b in ((first, again), (first, third)):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


# ---- diagnostic-build switches -------------------------------------------------------------------

@pytest.mark.parametrize("n", KNOB_SIZES)
def test_knob_pair_fused_bit_equal(dev, diag_lib, monkeypatch, n):
    """The inverse's pairing inside the first pass's loads (default) against the separate pairing
    pass (which overwrites coeffs): the same arithmetic."""
    c = random_case(n)
    monkeypatch.setenv("DPZ_FFT_PAIR_FUSED", "1")
    b1 = dev_irfft(c["spec"], n, dev)
    monkeypatch.setenv("DPZ_FFT_PAIR_FUSED", "0")
    b0 = dev_irfft(c["spec"], n, dev)
    np.testing.assert_array_equal(b0.view(np.uint32), b1.view(np.uint32))


@pytest.mark.parametrize("n", KNOB_SIZES)
def test_knob_bmax_bit_equal(dev, diag_lib, monkeypatch, n):
    """Columns per block do not change a column's arithmetic."""
    c = random_case(n)
    monkeypatch.setenv("DPZ_FFT_BMAX", "16")
    f16, b16 = dev_rfft(c["x"], dev), dev_irfft(c["spec"], n, dev)
    for bmax in (1, 2, 4, 8):
        monkeypatch.setenv("DPZ_FFT_BMAX", str(bmax))
        np.testing.assert_array_equal(dev_rfft(c["x"], dev).view(np.uint64), f16.view(np.uint64))
        np.testing.assert_array_equal(dev_irfft(c["spec"], n, dev).view(np.uint32),
                                      b16.view(np.uint32))


@pytest.mark.parametrize("pack", [4, 16, 64])
@pytest.mark.parametrize("n", KNOB_SIZES)
def test_knob_pack_accuracy(dev, diag_lib, monkeypatch, n, pack):
    """Many shallow passes (packing bound 4 / 16 / 64): the accuracy bound of the default plan."""
    monkeypatch.setenv("DPZ_FFT_PACK", str(pack))
    errs = random_errors(n, dev)
    print({k: (e / EPS, r / EPS) for k, (e, r) in errs.items()})
    for what, (e, e_ref) in errs.items():
        assert e <= bound(e_ref, n), (what, n, pack, e / EPS, e_ref / EPS)


@pytest.mark.parametrize("n", KNOB_SIZES)
def test_knob_lib_accuracy(dev, diag_lib, monkeypatch, n):
    """hipFFT (DPZ_FFT_LIB=1) and the native kernels against the same float64 reference within the
    same bound."""
    from decentralizepy_amd import codec
    for lib in ("1", "0"):
        monkeypatch.setenv("DPZ_FFT_LIB", lib)
        assert codec.fft_native(n) == (lib == "0")
        errs = random_errors(n, dev)
        print(lib, {k: (e / EPS, r / EPS) for k, (e, r) in errs.items()})
        for what, (e, e_ref) in errs.items():
            assert e <= bound(e_ref, n), (what, n, lib, e / EPS, e_ref / EPS)


# ---- alignment -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 289, 4099])
def test_misaligned_pointers_are_refused(dev, n):
    """A pointer the kernels would read as (re, im) pairs that is not 8-byte aligned: DPZ_ERR_ARG
    before any launch (only the return code is tested; out keeps its fill)."""
    import ctypes

    from decentralizepy_amd import _lib, codec
    lib = _lib.lib()
    m = n // 2 + 1
    x = torch.ones(n + 2, device=dev)
    cx = torch.ones(2 * m + 2, device=dev)
    ws = torch.empty(max(int(lib.dpz_fft_workspace_bytes(n)), 256), dtype=torch.uint8, device=dev)
    st = codec._stream(dev)

    def call(fn, a, a_off, b, b_off):
        return fn(ctypes.c_void_p(a.data_ptr() + a_off), n, ctypes.c_void_p(b.data_ptr() + b_off),
                  codec._ptr(ws), ws.numel(), st)

    assert call(lib.dpz_rfft, x, 0, cx, 4) == _lib.DPZ_ERR_ARG      # complex out
    assert call(lib.dpz_irfft, cx, 4, x, 0) == _lib.DPZ_ERR_ARG     # complex coeffs
    if native(n) and n % 2 == 0:                                     # the reals as n / 2 pairs
        assert call(lib.dpz_rfft, x, 4, cx, 0) == _lib.DPZ_ERR_ARG
        assert call(lib.dpz_irfft, cx, 0, x, 4) == _lib.DPZ_ERR_ARG
    torch.cuda.synchronize(dev)
    assert bool((x == 1).all()) and bool((cx == 1).all())
