"""K11 biquad cascade, no GPU: the CPU statement (tests/eq_ref/ref_eq.c) — the tiled form the GPU computes — against the plain sequential double
recurrence, and at steady state both against the same recurrence in long double; its carry tables against exact rational arithmetic; the library's host-side design nae_eq_design against its float64 restatement and against the magnitudes it promises; the
rejections; the equalizer node's JSON and the four registration calls (tests/eq_ref/host_eq_node.cpp)."""
import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import eq_ref
import node_harness
from conftest import rel_rms

# The tiled statement in double, in front of the final rounding.  Measured here over the cases below:
# - in_len = 3 C + 7 against the sequential double recurrence, noise and a two-tone: 3.3e-14 ... 3.9e-14 with one section, 6.1e-13 ... 1.6e-12
#   with four, 5.8e-12 ... 5.8e-11 with the 16-section cascades (the worst is noise through S16).  The same recurrence in f32 is 1.8e-5 ... 1.1e-2
#   away.
# - in_len = 300 C + 7 against the same recurrence in long double ("truth"), noise, the two-tone and 20 Hz + 40 Hz: 3.3e-14 ... 9.7e-14 with one
#   section, 2.8e-12 ... 3.0e-11 with four, 4.7e-11 ... 2.0e-10 with the 16-section cascades (the worst, 1.98e-10, is the two-tone through S16).
#   The sequential double recurrence itself is 3.4e-14 ... 7.7e-14, 3.2e-12 ... 5.4e-12 and 6.9e-12 ... 3.0e-10 away from truth (its worst,
#   3.02e-10, in the same case), so on noise and the two-tone the tiled form is as near to truth as the reference form; on 20 Hz + 40 Hz it is
#   1.3 ... 18 times farther.  After the rounding 0 ... 2306 of the 307 207 f32 samples differ from the rounded truth; of the sequential
#   recurrence's, 0 ... 2965.
# With tables made in double (until the tables moved to double-double) the steady state was 3.8e-9 ... 1.2e-8 through the 16-section cascades and
# four sections on 20 Hz + 40 Hz, and up to 75 850 f32 samples differed: test_statement_at_steady_state and
# test_tables_against_exact_arithmetic fail on them.
# The bound is by rule 30 times the worst case over all of these, the margin the long convolution's bound has over its own, and never above the
# 3e-9 it was first set to: 30 x 1.98e-10 = 5.9e-9, so it stays 3e-9, 15 times the worst case.
RMS_BOUND = 3e-9
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return eq_ref.build(str(tmp_path_factory.mktemp("ref_eq")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("eq_ref/host_eq_node.cpp", str(tmp_path_factory.mktemp("host_eq")))


def _signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return {"noise": rng.uniform(-1, 1, n).astype(np.float32),
            "two-tone": (0.6 * np.sin(2 * np.pi * 0.0371 * t) + 0.3 * np.sin(2 * np.pi * 0.213 * t + 1.0)).astype(np.float32)}


CASCADES = {"S1": lambda: eq_ref.cascade(1), "S4": lambda: eq_ref.cascade(4), "S16": lambda: eq_ref.cascade(16), "hard": eq_ref.hard_cascade}


@pytest.mark.parametrize("name", CASCADES)
def test_statement_against_sequential_recurrence(ref, name):
    coef = CASCADES[name]()
    n = 3 * eq_ref.CHUNK + 7
    for sig, x in _signals(n, 1).items():
        seq = eq_ref.sequential(ref, coef, x)
        err = rel_rms(eq_ref.run_f64(ref, coef, x), seq)
        y = eq_ref.run(ref, coef, x)
        differ = int(np.sum(y != seq.astype(np.float32)))
        f32 = rel_rms(eq_ref.sequential_f32(ref, coef, x), seq)
        print(f"{name} ({len(coef)} sections) {sig}: rel RMS {err:.3g} in double; {differ} of {n} f32 samples differ; the f32 recurrence {f32:.3g}")
        assert err <= RMS_BOUND, (name, sig, err)
        assert np.array_equal(y, eq_ref.run_f64(ref, coef, x).astype(np.float32)), "rounded once, behind the last section"
        assert rel_rms(y, seq) <= 1e-7, "and the f32 result is the sequential one to f32's own rounding"


def _steady_signals(n):
    t = np.arange(n)
    low = 0.5 * np.sin(2 * np.pi * 20 * t / 48000) + 0.3 * np.sin(2 * np.pi * 40 * t / 48000)
    return {**_signals(n, 1), "20 + 40 Hz": low.astype(np.float32)}


@pytest.mark.parametrize("name", CASCADES)
def test_statement_at_steady_state(ref, name):
    """300 chunks, far longer than the memory of the 20 - 60 Hz bells, which the last signal excites: the tiled statement and the sequential
    double recurrence, each against the same recurrence in long double ("truth"), in front of the final rounding.  The carry tables decide
    this: an error of theirs is the same in every chunk and adds up over the filter's memory."""
    assert eq_ref.ldbl_mant_dig(ref) >= 64, "truth needs an extended long double"
    coef = CASCADES[name]()
    n = 300 * eq_ref.CHUNK + 7
    for sig, x in _steady_signals(n).items():
        truth = eq_ref.sequential_ld(ref, coef, x)
        err = rel_rms(eq_ref.run_f64(ref, coef, x), truth)
        seq = rel_rms(eq_ref.sequential(ref, coef, x), truth)
        y = eq_ref.run(ref, coef, x)
        r32 = truth.astype(np.float32)
        differ, differ_seq = int(np.sum(y != r32)), int(np.sum(eq_ref.sequential(ref, coef, x).astype(np.float32) != r32))
        print(f"{name} ({len(coef)} sections) {sig}: rel RMS to truth {err:.3g} tiled, {seq:.3g} sequential, ratio {err / seq:.3g}; "
              f"{differ} (tiled) and {differ_seq} (sequential) of {n} f32 samples differ from the rounded truth")
        assert err <= RMS_BOUND, (name, sig, err)
        assert seq <= RMS_BOUND, "the bar is one the reference form meets on this input"
        assert rel_rms(y, truth) <= 1e-7, "and the f32 result is the truth to f32's own rounding"


def _exact_tables(a1, a2):
    """the 56 table entries of one section as exact rationals: the zero-input recurrence and the five squarings in fractions.Fraction"""
    a1, a2 = Fraction(float(a1)), Fraction(float(a2))
    cols, m = [], [None] * 4
    for col in range(2):
        z1, z2, out = Fraction(1 - col), Fraction(col), []
        for _ in range(eq_ref.LANE):
            y = z1
            z1, z2 = -a1 * y + z2, -a2 * y
            out.append(y)
        cols += out
        m[col], m[2 + col] = z1, z2
    phis = []
    for _ in range(6):
        phis += m
        m = [m[0] * m[0] + m[1] * m[2], m[0] * m[1] + m[1] * m[3], m[2] * m[0] + m[3] * m[2], m[2] * m[1] + m[3] * m[3]]
    return cols + phis


def _ulp(v):
    """the spacing of the doubles at the exact rational |v| > 0"""
    v = abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    return Fraction(2) ** (max(e, -1022) - 52)


TABLE_SECTIONS = {**{f"hard at {sr}": (lambda sr=sr: eq_ref.hard_cascade(sr)) for sr in (44100, 48000, 96000)},
                  "edges": lambda: np.stack([eq_ref.design("peak", 192000, 0.5, 24, 40), eq_ref.design("lowshelf", 48000, 1.0, -24, 0.1),
                                             eq_ref.design("highpass", 8000, 3999, 0, 40), eq_ref.design("notch", 48000, 23999, 0, 0.1)])}


@pytest.mark.parametrize("name", TABLE_SECTIONS)
def test_tables_against_exact_arithmetic(ref, name):
    """p, q and Phi_0 ... Phi_5 of the statement against exact rational arithmetic: every entry within 1 ulp of double, an exact zero 0.0,
    p[0] = 1.  Phi of a pole pair close to z = 1 is nearly defective and each squaring magnifies a rounding by about 1 / w0: tables made in
    double were up to 1.6e6 ulp off here, in long double 2500; in double-double the worst is 0.5 ulp, the final rounding"""
    worst, smallest = 0.0, 1.0
    for sec in TABLE_SECTIONS[name]():
        got, want = eq_ref.tables(ref, sec[3], sec[4]), _exact_tables(sec[3], sec[4])
        assert len(want) == got.size == 56 and got[0] == 1.0 and np.all(np.isfinite(got))
        largest = max(abs(w) for w in want)
        for i, (g, w) in enumerate(zip(got, want)):
            if w == 0:
                assert g == 0.0, (sec, i, g)
                continue
            ulps = float(abs(Fraction(float(g)) - w) / _ulp(w))
            worst, smallest = max(worst, ulps), min(smallest, float(abs(w) / largest))
            assert ulps <= 1.0, (sec, i, g, float(w), ulps)
    print(f"{name}: worst {worst:.4g} ulp; the smallest entry is {smallest:.3g} of its section's largest")


def test_statement_is_the_sequential_recurrence_inside_the_first_lane(ref):
    """no carry and a zero correction: the first 16 samples are the sequential recurrence's, rounded"""
    coef = eq_ref.cascade(4)
    x = _signals(40, 2)["noise"]
    assert np.array_equal(eq_ref.run(ref, coef, x)[:eq_ref.LANE], eq_ref.sequential(ref, coef, x).astype(np.float32)[:eq_ref.LANE])


def test_statement_channels_and_limits(ref):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (1500, 2)).astype(np.float32)
    coef = eq_ref.cascade(3)
    y = eq_ref.run(ref, coef, x.reshape(-1), ch=2).reshape(-1, 2)
    for c in range(2):
        assert np.array_equal(y[:, c], eq_ref.run(ref, coef, np.ascontiguousarray(x[:, c])))
    many = np.tile(eq_ref.cascade(1), (17, 1))
    assert ref.ref_eq_check(many.ctypes.data, 16) == 0 and ref.ref_eq_check(many.ctypes.data, 17) == -1 and ref.ref_eq_check(many.ctypes.data, 0) == -1


@pytest.mark.parametrize("sample_rate", (44100, 48000))
@pytest.mark.parametrize("kind", eq_ref.KINDS)
def test_design_against_float64_restatement(nae, ref, kind, sample_rate):
    """bound: 1 ulp of double per coefficient; measured 0 ulp in every case (the same libm behind both)"""
    worst = 0
    for freq, gain_db, q in ((20.0, 12.0, 10.0), (1000.0, 6.0, 1.0), (15000.0, -24.0, 0.1), (50.0, 0.0, 40.0), (sample_rate / 2 - 1.0, 24.0, 0.7071),
                             (0.5, 3.0, 2.0), (4321.0, -0.5, 0.707)):
        got = nae.Context.eq_design(kind, sample_rate, freq, gain_db, q)
        want = eq_ref.design(kind, sample_rate, freq, gain_db, q)
        stated = np.zeros(5)
        assert ref.ref_eq_design(eq_ref.KINDS.index(kind), sample_rate, freq, gain_db, q, stated.ctypes.data) == 0
        ulps = int(np.abs(got.view(np.int64) - want.view(np.int64)).max())
        worst = max(worst, ulps)
        assert ulps <= 1, (kind, sample_rate, freq, gain_db, q, got, want)
        assert np.array_equal(got, stated), "the statement's design is the library's"
        assert eq_ref.stable(got)
    print(f"{kind} at {sample_rate}: worst {worst} ulp")


@pytest.mark.parametrize("sample_rate", (44100, 48000))
def test_magnitude_from_the_coefficients(nae, sample_rate):
    des, mag = nae.Context.eq_design, lambda c, f: eq_ref.magnitude_db(c, f, sample_rate)
    peak = des("peak", sample_rate, 1000.0, 6.0, 1.0)
    assert abs(mag(peak, 1000.0) - 6.0) <= 0.01 and abs(mag(peak, 50.0)) <= 0.1 and abs(mag(peak, 15000.0)) <= 0.1
    low = des("lowshelf", sample_rate, 200.0, 9.0, 0.7071)
    assert abs(mag(low, 1.0) - 9.0) <= 0.01 and abs(mag(low, 20000.0)) <= 0.01, "a low shelf reaches its gain towards 0 Hz"
    high = des("highshelf", sample_rate, 4000.0, -7.5, 0.7071)
    assert abs(mag(high, sample_rate / 2 - 1.0) + 7.5) <= 0.01 and abs(mag(high, 10.0)) <= 0.01, "a high shelf reaches its gain towards Nyquist"
    lp, hp = des("lowpass", sample_rate, 2000.0, 0.0, 0.7071), des("highpass", sample_rate, 2000.0, 0.0, 0.7071)
    assert abs(mag(lp, 2000.0) + 3.01) <= 0.05 and abs(mag(hp, 2000.0) + 3.01) <= 0.05
    assert abs(mag(lp, 10.0)) <= 0.01 and mag(lp, 20000.0) < -38.0 and abs(mag(hp, 20000.0)) <= 0.05 and mag(hp, 20.0) < -75.0
    assert np.array_equal(lp, des("lowpass", sample_rate, 2000.0, 17.0, 0.7071)), "gain_db is ignored by the low-pass"
    notch = des("notch", sample_rate, 1000.0, 0.0, 4.0)
    assert mag(notch, 1000.0) < -60.0 and abs(mag(notch, 100.0)) <= 0.1 and abs(mag(notch, 8000.0)) <= 0.1


def test_design_rejections(nae):
    lib = nae.load_library()
    out = np.zeros(5)
    des = lambda kind, sr, f, g, q, p=out.ctypes.data: lib.nae_eq_design(kind, sr, f, g, q, p)
    assert des(0, 48000, 1000.0, 6.0, 1.0) == 0
    assert des(-1, 48000, 1000.0, 6.0, 1.0) == INVALID and des(6, 48000, 1000.0, 6.0, 1.0) == INVALID
    assert des(0, 0, 1000.0, 6.0, 1.0) == INVALID and des(0, -48000, 1000.0, 6.0, 1.0) == INVALID
    for f in (0.0, -1.0, 24000.0, 30000.0, float("nan"), float("inf")):
        assert des(0, 48000, f, 6.0, 1.0) == INVALID, f
    assert des(0, 48000, 23999.0, 6.0, 1.0) == 0 and des(0, 44100, 22050.0, 6.0, 1.0) == INVALID
    for q in (0.0, 0.099, 40.001, -1.0, float("nan"), float("inf")):
        assert des(0, 48000, 1000.0, 6.0, q) == INVALID, q
    assert des(0, 48000, 1000.0, 6.0, 0.1) == 0 and des(0, 48000, 1000.0, 6.0, 40.0) == 0
    for g in (24.001, -24.001, float("nan"), float("inf"), -float("inf")):
        assert des(0, 48000, 1000.0, g, 1.0) == INVALID, g
        assert des(3, 48000, 1000.0, g, 1.0) == INVALID, "out of range even where the kind ignores it"
    assert des(0, 48000, 1000.0, 24.0, 1.0) == 0 and des(0, 48000, 1000.0, -24.0, 1.0) == 0
    assert des(0, 48000, 1000.0, 6.0, 1.0, None) == INVALID
    with pytest.raises(nae.NaeError):
        nae.Context.eq_design("peak", 48000, 30000.0, 0.0, 1.0)


def test_unstable_and_non_finite_sections_are_rejected(ref):
    """the statement's rule, restated in eq_ref.stable; tests/test_gpu_eq.py asks the same of the library's entries, which need a context"""
    for sec in eq_ref.BAD_SECTIONS:
        c = np.array(sec, np.float64)
        assert ref.ref_eq_check(c.ctypes.data, 1) == -1 and not eq_ref.stable(c), sec
        both = np.concatenate([eq_ref.cascade(1)[0], c])
        assert ref.ref_eq_check(both.ctypes.data, 2) == -1, "a bad section behind a good one"
    for sec in eq_ref.GOOD_SECTIONS:
        c = np.array(sec, np.float64)
        assert ref.ref_eq_check(c.ctypes.data, 1) == 0 and eq_ref.stable(c), sec


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    coef = eq_ref.cascade(1)
    h = C.c_void_p()
    assert lib.nae_eq_block_f32(None, coef.ctypes.data, 1, None, 0, 1, 0, None) == INVALID
    assert lib.nae_eq_create(None, coef.ctypes.data, 1, 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_eq_put(None, None, 0) == INVALID and lib.nae_eq_flush(None) == INVALID and lib.nae_eq_available(None) == 0
    assert lib.nae_eq_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>"; json_mini's arrays"""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the three existing calls give 9 entries without audio_eq, register_equalizer_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [9, 10]
    assert "audio_eq" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_eq"])
