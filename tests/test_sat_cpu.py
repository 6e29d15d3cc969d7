"""K18 saturation, no GPU: the CPU statement (tests/sat_ref/ref_sat.c) against the library's tap design and against its float64 numpy
restatement; what the node is for, measured on the statement: the linear region, and the aliasing of a driven tone against the oversampling
factor; the closed forms: the odd map, M = 1's direct formula, the hard curve's bound, where a non-finite sample reaches; nae_sat_design
against its restatement and every rejection; the header; the node's JSON and the eleven registration calls (tests/sat_ref/host_sat_node.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import node_harness
import sat_ref

INVALID, UNSUPPORTED = sat_ref.INVALID, sat_ref.UNSUPPORTED
SOFT, HARD = sat_ref.SOFT, sat_ref.HARD


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sat_ref.build(str(tmp_path_factory.mktemp("ref_sat")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("sat_ref/host_sat_node.cpp", str(tmp_path_factory.mktemp("host_sat")))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def noise(n, ch, seed=0, amp=1.0):
    return (amp * np.random.default_rng(1000 * n + seed).uniform(-1, 1, (n, ch))).astype(np.float32)


def rel_rms(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.sqrt(np.mean((got - want) ** 2) / np.mean(want ** 2)))


def db(v):
    return 20.0 * np.log10(v)


@pytest.mark.parametrize("m", (2, 4, 8))
def test_taps_are_the_librarys_design(ref, nae, m):
    """hd = nae_fir_design(0, 2 M, -, 1.0, 32 M + 1) bit for bit, in the statement and in nae_sat_taps; the prototype's response in float64:
    flat within 0.001 dB to 20 kHz at 48 kHz, -6.02 dB at the base Nyquist, at most -80.8 dB from 28 kHz on"""
    n = 32 * m + 1
    design = nae.Context.fir_design("lowpass", 2 * m, 0.0, 1.0, n)
    stated = sat_ref.taps(ref, m)
    assert stated.size == n and same_bits(stated, design)
    assert same_bits(nae.Context.sat_taps(m), design)
    assert same_bits(stated, stated[::-1]), "linear phase"
    h = stated.astype(np.float64)
    f = np.arange(0, 24000 * m + 1, 50.0)                                  # hertz, at the rate 48 kHz x M
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(n)) / (48000.0 * m)) @ h)
    # the specification's figures, to the digits it gives them in (0.0010010 dB at M = 4 is "0.001 dB")
    ripple, nyq, stop = np.max(np.abs(db(H[f <= 20000]))), db(H[f == 24000][0]), np.max(db(H[f >= 28000]))
    print(f"prototype, M = {m}: ripple to 20 kHz {ripple:.7f} dB, at 24 kHz {nyq:.4f} dB, from 28 kHz on {stop:.2f} dB")
    assert ripple < 0.0015 and abs(nyq + 6.02) < 0.005 and stop < -80.75


def test_no_taps_at_one_and_the_latency(ref, nae):
    assert nae.Context.sat_taps(1).size == 0 and sat_ref.taps(ref, 1).size == 0 and nae.Context.sat_taps(3).size == 0
    lib = nae.load_library()
    assert lib.nae_sat_taps(2, None) == 0
    for m, d in ((1, 0), (2, 32), (4, 32), (8, 32), (0, -1), (3, -1), (16, -1), (-2, -1)):
        assert nae.Context.sat_latency(m) == d == ref.ref_sat_latency(m), m


def test_statement_against_restatement(ref):
    """f32 chains against float64 convolutions: relative RMS at most 1e-4, the project's bar for results continuous in their inputs"""
    worst = 0.0
    for m in sat_ref.FACTORS:
        hd = sat_ref.taps(ref, m)
        for curve, drive, bias, wet, dry in ((SOFT, 4.0, 0.0, 1.0, 0.0), (SOFT, 15.8, 0.3, 0.5, 0.5), (HARD, 4.0, 0.0, 1.0, 0.0), (HARD, 2.0, 0.3, 0.7, 0.3)):
            p = sat_ref.params(m, curve, drive, bias, wet, dry)
            x = noise(6000, 2, seed=m, amp=0.5)
            e = rel_rms(sat_ref.run(ref, p, x), sat_ref.run_np(p, x, hd))
            print(f"statement against restatement, M = {m}, curve {curve}, drive {drive}, bias {bias}: relative RMS {e:.3g}")
            worst = max(worst, e)
    assert worst <= 1e-4, worst


@pytest.mark.parametrize("m", (2, 4, 8))
def test_linear_region(ref, m):
    """drive 0 dB, soft, a 3 kHz sine of amplitude 1e-3 at 48 kHz: y[n + 32] against x[n] within 1e-5 relative RMS"""
    n = 16384
    x = (1e-3 * np.sin(2 * np.pi * 3000.0 * np.arange(n) / 48000.0)).astype(np.float32).reshape(-1, 1)
    y = sat_ref.run(ref, sat_ref.params(m, SOFT, 1.0, 0.0, 1.0, 0.0), x)
    e = rel_rms(y[32 + 64:, 0], x[64:n - 32, 0])
    print(f"linear region, M = {m}: relative RMS {e:.3g}")
    assert e <= 1e-5, e


def alias_db(ref, m, curve):
    """A: the RMS of the non-harmonic bins up to 20 kHz over the fundamental's bin, in dB: x = 0.5 sin(2 pi 3413 n / 32768) (4999.5 Hz at
    48 kHz), drive 24 dB, bias 0, the first 4096 outputs dropped, a 32768-point FFT"""
    N, k0 = 32768, 3413
    n = np.arange(4096 + N)
    x = (0.5 * np.sin(2 * np.pi * k0 * n / N)).astype(np.float32).reshape(-1, 1)
    p = sat_ref.design(24.0, 0.0, curve, m)
    y = sat_ref.run(ref, p, x)[4096:, 0].astype(np.float64)
    mag = np.abs(np.fft.rfft(y))
    top = int(np.floor(20000.0 / 48000.0 * N))
    # the harmonics of k0 folded at the base rate land on multiples of k0 mod N (mirrored): all of them, aliased or not, are on those bins; what
    # the node is measured by is the ALIASED ones, which land off the harmonic series h k0 <= top
    harmonic = {h * k0 for h in range(1, top // k0 + 1)}
    other = np.array([k for k in range(1, top + 1) if k not in harmonic])
    return float(db(np.sqrt(np.mean(mag[other] ** 2)) / mag[k0]))


def test_aliasing_falls_with_the_oversampling(ref):
    """the reason the node exists: A(4) <= A(1) - 40 dB and A(8) <= A(4) - 20 dB on the soft curve; the hard curve's falls with each doubling"""
    soft = {m: alias_db(ref, m, SOFT) for m in sat_ref.FACTORS}
    hard = {m: alias_db(ref, m, HARD) for m in sat_ref.FACTORS}
    print("aliasing, soft:", {m: round(v, 1) for m, v in soft.items()}, "hard:", {m: round(v, 1) for m, v in hard.items()})
    assert soft[4] <= soft[1] - 40.0, soft
    assert soft[8] <= soft[4] - 20.0, soft
    assert hard[1] > hard[2] > hard[4] > hard[8], hard


def test_the_map_is_odd_at_bias_zero(ref):
    """b = 0: f is odd and f(0) = 0, products and fused chains are odd in their signal operand, so negating x negates y bit for bit"""
    x = noise(5000, 2, seed=3)
    for m in sat_ref.FACTORS:
        for curve in (SOFT, HARD):
            p = sat_ref.params(m, curve, 7.5, 0.0, 0.8, 0.4)
            y, yn = sat_ref.run(ref, p, x), sat_ref.run(ref, p, -x)
            nz = y != 0                                            # a zero sum keeps its sign: (+0) + (+0) and (-0) + (-0) negate, x - x does not
            assert np.array_equal(yn, -y) and same_bits(yn[nz], -y[nz]), (m, curve)


def test_one_is_the_direct_formula(ref):
    """M = 1: y = (dry x) + (wet (f(fma(g, x, b)) - f(b))), every step rounded to f32; the fma through float64, where g x is exact"""
    f32, f64 = np.float32, np.float64
    x = noise(4000, 2, seed=5)
    for curve in (SOFT, HARD):
        g, b, wet, dry = f32(5.25), f32(0.2), f32(0.7), f32(0.35)
        t = (x.astype(f64) * f64(g) + f64(b)).astype(f32)          # the product is exact in float64 (a double rounding of the sum needs a tie in 29 bits: not met on this signal)
        if curve == SOFT:
            c = np.clip(t, f32(-3), f32(3))
            q = c * c
            f = (c * (f32(27) + q)) / (f32(27) + (f32(9) * q))
        else:
            f = np.clip(t, f32(-1), f32(1))
        fb = f32(ref.ref_sat_curve(curve, float(b)))
        want = (dry * x) + (wet * (f - fb))
        got = sat_ref.run(ref, sat_ref.params(1, curve, float(g), float(b), float(wet), float(dry)), x)
        assert same_bits(got, want.astype(f32)), curve


def test_hard_curve_is_bounded(ref):
    """|v| <= 1 + |f(b)|, so |y| <= wet (1 + |f(b)|) sum|hd| + dry max|x| (a few f32 roundings over: 1e-5 relative)"""
    x = noise(6000, 2, seed=9, amp=4.0)
    for m in (2, 4, 8):
        hd = sat_ref.taps(ref, m).astype(np.float64)
        for bias in (0.0, 0.6):
            wet, dry = 0.9, 0.5
            y = sat_ref.run(ref, sat_ref.params(m, HARD, 50.0, bias, wet, dry), x)
            bound = wet * (1.0 + min(bias, 1.0)) * np.sum(np.abs(hd)) + dry * float(np.max(np.abs(x)))
            assert float(np.max(np.abs(y))) <= bound * (1 + 1e-5), (m, bias)


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_a_non_finite_sample_stays_in_its_reach(ref, bad):
    """a non-finite x[n] reaches y[n ... n + 64] of its own channel: everything else has the clean run's bits"""
    x = noise(3000, 2, seed=11)
    at = 1500
    for m in sat_ref.FACTORS:
        for curve in (SOFT, HARD):
            p = sat_ref.params(m, curve, 3.0, 0.1, 0.8, 0.4)
            clean = sat_ref.run(ref, p, x)
            dirty_x = x.copy()
            dirty_x[at, 1] = bad
            dirty = sat_ref.run(ref, p, dirty_x)
            reach = 64 if m > 1 else 0
            assert same_bits(dirty[:, 0], clean[:, 0]), "the other channel"
            assert same_bits(dirty[:at, 1], clean[:at, 1]) and same_bits(dirty[at + reach + 1:, 1], clean[at + reach + 1:, 1]), (m, curve)
            assert not np.isfinite(dirty[at + (32 if m > 1 else 0), 1]), "the dry path carries it at the latency (dry is not 0)"


def test_design_against_its_restatement(ref, nae):
    lib = nae.load_library()
    cases = [(12.0, 0.0, SOFT, 4, 0.0, 1.0), (0.0, 0.0, SOFT, 1, -24.0, 0.0), (48.0, 1.0, HARD, 8, 24.0, 1.0), (6.02, 0.3, HARD, 2, -3.5, 0.35),
             (24.0, 0.5, SOFT, 2, 3.0, 0.5)]
    for args in cases:
        out, stated = nae.SatParams(), sat_ref.Params()
        assert lib.nae_sat_design(*args, C.byref(out)) == 0 and ref.ref_sat_design(*args, C.byref(stated)) == 0, args
        want = sat_ref.design(*args)
        assert sat_ref.as_tuple(stated) == sat_ref.as_tuple(want) == (out.oversample, out.curve, out.drive, out.bias, out.wet, out.dry), args
    d = nae.Context.sat_design()
    assert (d.oversample, d.curve, d.bias, d.wet, d.dry) == (4, SOFT, 0.0, 1.0, 0.0) and d.drive == np.float32(10.0 ** 0.6)
    assert nae.Context.sat_design(curve="hard", mix=0.25, output_db=6.0).dry == 0.75


def test_design_rejections(ref, nae):
    lib = nae.load_library()
    good = [12.0, 0.0, SOFT, 4, 0.0, 1.0]
    nan, inf = float("nan"), float("inf")
    out, stated = nae.SatParams(), sat_ref.Params()
    assert lib.nae_sat_design(*good, C.byref(out)) == 0 and lib.nae_sat_design(*good, None) == INVALID and ref.ref_sat_design(*good, None) == INVALID
    for i, values in ((0, (-0.001, 48.001, nan, inf, -inf)), (1, (-0.001, 1.001, nan, inf)), (2, (2, -1)), (4, (-24.001, 24.001, nan, -inf)),
                      (5, (-0.001, 1.001, nan, inf))):
        for v in values:
            args = good[:i] + [v] + good[i + 1:]
            assert lib.nae_sat_design(*args, C.byref(out)) == INVALID, args
            assert ref.ref_sat_design(*args, C.byref(stated)) == INVALID and sat_ref.design(*args) == INVALID, args
    for m in (0, 3, 5, 6, 16, -4):
        args = good[:3] + [m] + good[4:]
        assert lib.nae_sat_design(*args, C.byref(out)) == UNSUPPORTED and ref.ref_sat_design(*args, C.byref(stated)) == UNSUPPORTED, m
        assert sat_ref.design(*args) == UNSUPPORTED
    assert lib.nae_sat_design(12.0, 0.0, 7, 3, 0.0, 1.0, C.byref(out)) == INVALID, "an unknown curve is asked before the oversampling factor"


def test_statement_rejects_what_the_library_rejects(ref):
    """the parameter rules (tests/test_gpu_sat.py asks the library's entries the same questions)"""
    def check(ch=2, **kw):
        args = dict(oversample=8, curve=HARD, drive=250.0, bias=-3.0, wet=-2.0, dry=1e6)
        args.update(kw)
        return ref.ref_sat_check(C.byref(sat_ref.params(**args)), ch)

    assert check() == 0 and check(ch=1) == 0 and check(curve=SOFT, oversample=1) == 0
    assert ref.ref_sat_check(None, 2) == INVALID and check(ch=0) == INVALID and check(ch=3) == INVALID
    for key in ("drive", "bias", "wet", "dry"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert check(**{key: v}) == INVALID, (key, v)
    assert check(curve=2) == INVALID and check(curve=-1) == INVALID
    for m in (0, 3, 16, -1):
        assert check(oversample=m) == UNSUPPORTED, m
    assert check(oversample=3, curve=5) == INVALID
    x = np.zeros((8, 2), np.float32)
    assert ref.ref_sat_run(C.byref(sat_ref.params(oversample=3)), x.ctypes.data, 8, 2, x.ctypes.data) == UNSUPPORTED


def test_record_and_constants_agree_with_the_header(nae):
    """the binding's record has the statement's layout and the header's fields, the NAE_SAT_* constants stand in include/nae_dsp_spec.h, the
    sat_tile row in the header's key list, the ABI version stays 3"""
    spec = open(os.path.join(sat_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    for name, value in (("HALF", "16"), ("MAX_OS", "8"), ("SOFT", "0"), ("HARD", "1")):
        assert re.search(rf"#define\s+NAE_SAT_{name}\s+{value}\s*$", spec, re.M), name
    assert (nae.SAT_HALF, nae.SAT_MAX_OS, nae.SAT_CURVES) == (sat_ref.HALF, sat_ref.MAX_OS, ("soft", "hard"))
    assert C.sizeof(nae.SatParams) == C.sizeof(sat_ref.Params) == 24
    for name in ("oversample", "curve", "drive", "bias", "wet", "dry"):
        assert getattr(nae.SatParams, name).offset == getattr(sat_ref.Params, name).offset, name
    header = open(os.path.join(sat_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_sat_params \{(.*?)\} nae_sat_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|int)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("int", "oversample"), ("int", "curve"), ("float", "drive"), ("float", "bias"), ("float", "wet,dry")]
    assert re.search(r"^ \*   sat_tile\s", header, re.M) and "#define NAE_ABI_VERSION 3" in header
    assert all("nae_sat_" + s in nae.EXPORTED_SYMBOLS for s in ("latency", "taps", "design", "block_f32", "create", "put", "put_host", "flush", "available",
                                                                 "receive", "receive_host", "destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.SatParams.make(4, 0, 4.0)
    h = C.c_void_p()
    assert lib.nae_sat_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_sat_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_sat_put(None, None, 0) == INVALID and lib.nae_sat_put_host(None, None, 0) == INVALID
    assert lib.nae_sat_flush(None) == INVALID and lib.nae_sat_available(None) == 0
    got = C.c_size_t()
    assert lib.nae_sat_receive(None, None, 0, C.byref(got)) == INVALID and lib.nae_sat_receive_host(None, None, 0, C.byref(got)) == INVALID
    assert lib.nae_sat_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: the six keys round-trip, the defaults are not written back, a wrong type or value is the error
    "Wrong field: <key>" with that key"""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST SAT OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the ten existing calls give 16 entries without audio_saturation, register_saturation_processors() adds exactly it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST SAT OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [16, 17]
    assert "audio_saturation" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_saturation"])
