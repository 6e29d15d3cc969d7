"""K17 modulated delay, no GPU: the CPU statement (tests/mod_ref/ref_mod.c) against its numpy restatement; the closed forms, bit for bit: a
pure delay, two equal voices, channel 1 alone, an impulse's repeats; the LFO's two forms; the interpolation's accuracy on a vibrato against
its derived bound; stability at the largest feedback as a condition; nae_mod_design against its restatement and every rejection of the design
and of the parameter rules; the header; the node's JSON and the ten registration calls (tests/mod_ref/host_mod_node.cpp)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mod_ref
import node_harness

INVALID, UNSUPPORTED = -1, -2
SINE, TRIANGLE = mod_ref.SINE, mod_ref.TRIANGLE


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mod_ref.build(str(tmp_path_factory.mktemp("ref_mod")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("mod_ref/host_mod_node.cpp", str(tmp_path_factory.mktemp("host_mod")))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def noise(n, ch, seed=0):
    return np.random.default_rng(1000 * n + seed).uniform(-1, 1, (n, ch)).astype(np.float32)


def test_statement_against_restatement(ref):
    """every step one float64 operation, the line np.float32: the C statement's bits.  Without feedback the restatement computes every
    sample at once; with it, sample after sample (at most 5000)"""
    cases = ((20000, 2, dict(delay=300, depth=96, rate_inc=mod_ref.hz(5), phase_ch=1 << 30, voice_phase=mod_ref.spread_voices(3), wet=0.5)),
             (20000, 1, dict(delay=2969.5, depth=100.5, rate_inc=mod_ref.hz(20), phase0=12345, voice_phase=mod_ref.spread_voices(4), shape=TRIANGLE, wet=0.7, dry=0.3)),
             (5000, 2, dict(delay=7.5, depth=5.5, feedback=0.9, rate_inc=mod_ref.hz(20), phase_ch=1 << 31, voice_phase=mod_ref.spread_voices(4), shape=TRIANGLE)),
             (5000, 1, dict(delay=20.25, depth=3.0, feedback=-0.9, rate_inc=mod_ref.hz(3), phase0=77, wet=0.7, dry=0.3)),
             (4000, 2, dict(delay=69.9, depth=4.0, feedback=0.9, rate_inc=0, phase0=1 << 29, phase_ch=1 << 30, voice_phase=(0, 1 << 31))))
    for n, ch, kw in cases:
        p = mod_ref.params(**kw)
        x = noise(n, ch)
        assert same_bits(mod_ref.run_np(p, x), mod_ref.run(ref, p, x)), kw


@pytest.mark.parametrize("D", (2, 3, 64, 1024, 3070))
def test_pure_delay(ref, D):
    """depth = 0, an integer delay, g = 0, dry = 0, wet = 1 and one voice: f = 0 makes the coefficients (-0, 1, 0, -0), and y is x delayed by
    D (values: a product with a zero coefficient may be a zero of either sign)"""
    n = 2 * D + 3000
    x = noise(n, 2)
    for shape in (SINE, TRIANGLE):
        y = mod_ref.run(ref, mod_ref.params(float(D), 0.0, 0.0, 1.0, 0.0, mod_ref.hz(5), phase_ch=1 << 30, shape=shape), x)
        assert np.array_equal(y, np.concatenate([np.zeros((D, 2), np.float32), x[:n - D]])), (D, shape)


def test_two_equal_voices_are_one(ref):
    """two voices with equal voice_phase: (t + t) 0.5 is exact, so the bits are one voice's, with and without feedback"""
    x = noise(6000, 2)
    for g in (0.0, 0.9, -0.9):
        for shape in (SINE, TRIANGLE):
            kw = dict(delay=40.3, depth=11.1, feedback=g, wet=0.6, dry=0.8, rate_inc=mod_ref.hz(7), phase_ch=1 << 30, shape=shape)
            one = mod_ref.run(ref, mod_ref.params(voice_phase=(999,), **kw), x)
            two = mod_ref.run(ref, mod_ref.params(voice_phase=(999, 999), **kw), x)
            four = mod_ref.run(ref, mod_ref.params(voice_phase=(999,) * 4, **kw), x)
            assert same_bits(one, two) and same_bits(one, four), (g, shape)


def test_channel_one_alone(ref):
    """channel 1 of a stereo run is a mono run of that channel with phase0 + phase_ch; channel 0 is a mono run as it stands: the channels do
    not interact, and mono reads no phase_ch"""
    x = noise(6000, 2)
    for g in (0.0, 0.9):
        kw = dict(delay=33.0, depth=20.5, feedback=g, wet=0.5, dry=1.0, rate_inc=mod_ref.hz(2.5), voice_phase=mod_ref.spread_voices(3))
        phase0, phase_ch = 0xf0000000, 0x30000000                     # their sum wraps
        y = mod_ref.run(ref, mod_ref.params(phase0=phase0, phase_ch=phase_ch, **kw), x)
        left = mod_ref.run(ref, mod_ref.params(phase0=phase0, phase_ch=phase_ch, **kw), np.ascontiguousarray(x[:, :1]))
        right = mod_ref.run(ref, mod_ref.params(phase0=phase0 + phase_ch, phase_ch=0, **kw), np.ascontiguousarray(x[:, 1:]))
        assert same_bits(y[:, 0], left[:, 0]) and same_bits(y[:, 1], right[:, 0]), g
        assert not same_bits(y[:, 1], mod_ref.run(ref, mod_ref.params(phase0=phase0, **kw), np.ascontiguousarray(x[:, 1:]))[:, 0]), "the spread is heard"


def phases_65536():
    return (np.arange(65536, dtype=np.uint64) << np.uint64(16)).astype(np.uint32)


def test_lfo_sine_form(ref):
    """the corrected parabola: within 1.1e-3 of sin(pi t) over 65 536 phases (measured here: 1.0903e-3), exact at t = 0, +-1/2 and -1,
    |l| <= 1 everywhere; the statement and the restatement agree bit for bit"""
    phi = phases_65536()
    t = phi.view(np.int32).astype(np.float64) * 2.0 ** -31
    l = np.array([ref.ref_mod_lfo(SINE, int(v)) for v in phi])
    assert np.array_equal(l, mod_ref.lfo_np(SINE, phi))
    err = float(np.max(np.abs(l - np.sin(np.pi * t))))
    print(f"sine form: max |l - sin(pi t)| = {err:.6g} over {len(phi)} phases")
    assert err <= 1.1e-3
    assert np.max(np.abs(l)) <= 1.0
    for phase, want in ((0, 0.0), (1 << 30, 1.0), (3 << 30, -1.0), (1 << 31, 0.0)):
        assert ref.ref_mod_lfo(SINE, phase) == want, (phase, want)
    # around the extremes, phase by phase: the bound |l| <= 1 holds where the parabola peaks
    for centre in (1 << 30, 3 << 30):
        near = np.arange(centre - 4096, centre + 4097, dtype=np.uint64).astype(np.uint32)
        assert np.max(np.abs(mod_ref.lfo_np(SINE, near))) <= 1.0


def test_lfo_triangle_form(ref):
    """2 |t| - 1, exact: against integers, l 2^30 = |phi as int32| - 2^30"""
    phi = np.concatenate([phases_65536(), np.array([1, 0x7fffffff, 0x80000000, 0x80000001, 0xffffffff], np.uint32)])
    l = np.array([ref.ref_mod_lfo(TRIANGLE, int(v)) for v in phi])
    assert np.array_equal(l, mod_ref.lfo_np(TRIANGLE, phi))
    want = np.abs(phi.view(np.int32).astype(np.int64)) - (1 << 30)
    assert np.array_equal(l * 2.0 ** 30, want.astype(np.float64))
    assert ref.ref_mod_lfo(TRIANGLE, 0) == -1.0 and ref.ref_mod_lfo(TRIANGLE, 1 << 30) == 0.0 and ref.ref_mod_lfo(TRIANGLE, 1 << 31) == 1.0


@pytest.mark.parametrize("g", (0.9, -0.9, 0.3))
def test_impulse_repeats(ref, g):
    """depth = 0 and an impulse: dry delta[n] plus wet times the repeats at n = k D; repeat k is g^(k - 1) accumulated by the line's own f32
    roundings, trip by trip, so the first repeat has amplitude wet"""
    D, wet, dry = 37, 0.35, 0.8
    n = 12 * D + 10
    x = np.zeros((n, 1), np.float32)
    x[0] = 1.0
    y = mod_ref.run(ref, mod_ref.params(float(D), 0.0, g, wet, dry, mod_ref.hz(3)), x)[:, 0]
    want = np.zeros(n, np.float32)
    want[0] = np.float32(np.float64(dry))
    amp = np.float32(1.0)                                   # w[0] = (float)(1 + g 0)
    for k in range(1, 13):
        want[k * D] = np.float32(np.float64(wet) * np.float64(amp))
        amp = np.float32(np.float64(g) * np.float64(amp))   # w[k D] = (float)(0 + g w[(k - 1) D])
    assert np.array_equal(y, want)
    assert y[D] == np.float32(wet), "the first repeat has amplitude wet"


def test_vibrato_accuracy(ref):
    """a unit sine at 1 kHz and 48 kHz through delay 240, depth 96, 5 Hz, dry 0, wet 1: after the first 400 samples the output is within
    9/384 w^4 + 3 2^-24 of sin(w (n - d(n))): the cubic Lagrange remainder |f (f^2 - 1)(f - 2)| / 24 <= (9/16) / 24 times the fourth
    derivative w^4, plus three f32 roundings of values up to 1 (the input, and the output's own; the third is slack).  A derived bound, not a
    tuned one: 7.06e-6.  Measured here: 6.87e-6"""
    n = np.arange(48000)
    w = 2.0 * np.pi * 1000.0 / 48000.0
    x = np.sin(w * n).astype(np.float32).reshape(-1, 1)
    p = mod_ref.params(240.0, 96.0, 0.0, 1.0, 0.0, mod_ref.hz(5))
    y = mod_ref.run(ref, p, x)[:, 0]
    phi = ((n.astype(np.uint64) * np.uint64(p.rate_inc)) & np.uint64(mod_ref.M32)).astype(np.uint32)
    d = 240.0 + 96.0 * mod_ref.lfo_np(SINE, phi)
    err = float(np.max(np.abs(y - np.sin(w * (n - d)))[400:]))
    bound = 9.0 / 384.0 * w ** 4 + 3.0 * 2.0 ** -24
    print(f"vibrato: max error {err:.4g}, bound {bound:.4g}")
    assert err <= bound


@pytest.mark.parametrize("voices", (1, 4))
@pytest.mark.parametrize("g", (0.95, -0.95))
def test_stability_is_a_condition(ref, g, voices):
    """unit noise of 20 000 samples at |g| = 0.95, delay 8, depth 5.5: every output finite and under 100 (measured here: under 6.3; a loop
    that diverges grows without bound).  The interpolator's gain exceeds 1 nowhere near enough to carry 0.95 over 1"""
    x = np.random.default_rng(5).uniform(-1, 1, (20000, 1)).astype(np.float32)
    for shape in (SINE, TRIANGLE):
        y = mod_ref.run(ref, mod_ref.params(8.0, 5.5, g, 1.0, 1.0, mod_ref.hz(0.8), voice_phase=mod_ref.spread_voices(voices), shape=shape), x)
        peak = float(np.max(np.abs(y)))
        print(f"g {g} voices {voices} shape {shape}: max |y| {peak:.4g}")
        assert np.all(np.isfinite(y)) and peak < 100.0


DESIGNS = ((48000, 0.8, 12.0, 3.0, 0.0, 3, 0.5, SINE, 0.5, 1.0), (48000, 0.25, 3.0, 2.0, 0.7, 1, 0.5, SINE, 0.7, 1.0),
           (48000, 5.0, 5.0, 2.0, 0.0, 1, 0.0, SINE, 1.0, 0.0), (44100, 20.0, 0.1, 0.0, -0.95, 4, 1.0, TRIANGLE, -2.0, 3.5),
           (96000, 0.0, 20.0, 11.0, 0.95, 2, 0.25, TRIANGLE, 0.0, 0.0), (8000, 13.7, 200.0, 183.75, 0.3, 3, 0.999, SINE, 1.0, 1.0),
           (48000, 1.0, 2.0 / 48.0, 0.0, 0.0, 1, 0.0, SINE, 1.0, 1.0))


def test_design_against_the_restatement(nae, ref):
    lib = nae.load_library()
    for args in DESIGNS:
        got, stated = nae.ModParams(), mod_ref.Params()
        want = mod_ref.design(*args)
        assert want is not None, args
        assert lib.nae_mod_design(*args, C.byref(got)) == 0 and ref.ref_mod_design(*args, C.byref(stated)) == 0, args
        assert mod_ref.as_tuple(got) == mod_ref.as_tuple(want) == mod_ref.as_tuple(stated), args
        assert ref.ref_mod_check(C.byref(stated), 2) == 0
    p = mod_ref.design(48000)
    assert (p.delay, p.depth, p.n_voices, p.phase0, p.phase_ch) == (576.0, 144.0, 3, 0, 1 << 30), "the defaults are a chorus: 12 ms +- 3 ms, three voices"
    assert tuple(p.voice_phase) == (0, 0x55555555, 0xaaaaaaaa, 0) and p.rate_inc == round(0.8 / 48000 * 2 ** 32)
    assert mod_ref.design(48000, spread=1.0).phase_ch == 1 << 31, "a spread of 1: half a turn"
    assert mod_ref.design(48000, rate_hz=0.0).rate_inc == 0, "a rate of 0: a fixed comb"
    assert tuple(mod_ref.design(48000, voices=4).voice_phase) == (0, 1 << 30, 1 << 31, 3 << 30)
    assert nae.Context.mod_design(48000, shape="triangle").shape == TRIANGLE and mod_ref.as_tuple(nae.Context.mod_design(48000)) == mod_ref.as_tuple(p)


def test_design_rejections(nae, ref):
    """NAE_ERR_INVALID outside the ranges, by the library, the statement and the restatement alike"""
    lib = nae.load_library()
    good = [48000, 0.8, 12.0, 3.0, 0.0, 3, 0.5, SINE, 0.5, 1.0]
    nan, inf = float("nan"), float("inf")
    bad = []
    for i, values in ((0, (0, -48000)), (1, (-0.1, 20.001, nan, inf)), (2, (3.04, 0.0, -1.0, 61.0, 1e300, nan, inf)), (3, (-0.001, 11.97, 52.0, nan, inf)),
                      (4, (0.951, -0.951, 5.0, nan, inf)), (5, (0, 5, -1)), (6, (-0.01, 1.01, nan, inf)), (7, (2, -1)), (8, (nan, inf)), (9, (nan, -inf))):
        for v in values:
            bad.append(good[:i] + [v] + good[i + 1:])
    out, stated = nae.ModParams(), mod_ref.Params()
    assert lib.nae_mod_design(*good, C.byref(out)) == 0 and lib.nae_mod_design(*good, None) == INVALID
    for args in bad:
        assert lib.nae_mod_design(*args, C.byref(out)) == INVALID, args
        assert ref.ref_mod_design(*args, C.byref(stated)) == INVALID, args
        assert mod_ref.design(*args) is None, args
    # the limits themselves: 2 and 3070 samples at 48 kHz and 8 kHz
    for args in ([8000, 20.0, 0.25, 0.0, 0.95, 4, 1.0, TRIANGLE, 0.0, 0.0], [8000, 0.0, 200.0, 183.75, -0.95, 1, 0.0, SINE, 1.0, 1.0]):
        assert lib.nae_mod_design(*args, C.byref(out)) == 0 and mod_ref.design(*args) is not None, args
    assert (out.delay - out.depth, out.delay + out.depth) == (130.0, 3070.0)


def test_statement_rejects_what_the_library_rejects(ref):
    """the parameter rules (tests/test_gpu_mod.py asks the library's entries the same questions)"""
    def check(ch=2, **kw):
        args = dict(delay=1536.0, depth=1534.0, feedback=0.95, wet=-3.0, dry=1e6, voice_phase=(1, 2, 3, 4), shape=TRIANGLE)
        args.update(kw)
        return ref.ref_mod_check(C.byref(mod_ref.params(**args)), ch)

    assert check() == 0 and check(ch=1) == 0 and check(feedback=-0.95) == 0 and check(depth=0.0) == 0 and check(shape=SINE) == 0
    assert ref.ref_mod_check(None, 2) == INVALID and check(ch=0) == INVALID and check(ch=3) == INVALID
    for key in ("delay", "depth", "feedback", "wet", "dry"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert check(**{key: v}) == INVALID, (key, v)
    assert check(feedback=0.9501) == INVALID and check(feedback=-1.0) == INVALID
    assert check(depth=-1e-9) == INVALID and check(delay=100.0, depth=-1.0) == INVALID
    assert check(n_voices=0) == INVALID and check(n_voices=-3) == INVALID and check(n_voices=5) == UNSUPPORTED
    assert check(shape=2) == INVALID and check(shape=-1) == INVALID
    assert check(n_voices=5, shape=7) == INVALID, "an unknown shape is asked before the voices' limit"
    for delay, depth in ((1536.0, 1534.5), (1.99, 0.0), (2.0, 1e-9), (3070.5, 0.0), (3000.0, 70.5), (0.0, 0.0), (-5.0, 0.0), (1e9, 0.0)):
        assert check(delay=delay, depth=depth) == UNSUPPORTED, (delay, depth)
    for delay, depth in ((2.0, 0.0), (3070.0, 0.0), (1536.0, 1534.0), (3000.0, 70.0)):
        assert check(delay=delay, depth=depth) == 0, (delay, depth)
    # a run with rejected parameters computes nothing
    x = np.zeros((8, 2), np.float32)
    assert ref.ref_mod_run(C.byref(mod_ref.params(1.0, 0.0)), x.ctypes.data, 8, 2, x.ctypes.data, None) == -1


def test_record_and_limits_agree_with_the_header(nae):
    """the binding's record has the statement's layout and the size the header's fields give, the NAE_MOD_* constants stand in
    include/nae_dsp_spec.h, the mod_sub row in the header's key list"""
    spec = open(os.path.join(mod_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    for name, value in (("MIN_DELAY", r"2\.0"), ("MAX_DELAY", r"3070\.0"), ("MAX_VOICES", "4"), ("MAX_FEEDBACK", r"0\.95"), ("SINE", "0"), ("TRIANGLE", "1")):
        assert re.search(rf"#define\s+NAE_MOD_{name}\s+{value}\s*$", spec, re.M), name
    assert (nae.MOD_MIN_DELAY, nae.MOD_MAX_DELAY, nae.MOD_MAX_VOICES, nae.MOD_MAX_FEEDBACK) == \
        (mod_ref.MIN_DELAY, mod_ref.MAX_DELAY, mod_ref.MAX_VOICES, mod_ref.MAX_FEEDBACK) == (2.0, 3070.0, 4, 0.95)
    assert nae.MOD_SHAPES == ("sine", "triangle")
    assert C.sizeof(nae.ModParams) == C.sizeof(mod_ref.Params) == 80, "five doubles, nine 32-bit words, padded to the doubles' alignment"
    for name in ("delay", "depth", "feedback", "wet", "dry", "rate_inc", "phase0", "phase_ch", "n_voices", "voice_phase", "shape"):
        assert getattr(nae.ModParams, name).offset == getattr(mod_ref.Params, name).offset, name
    header = open(os.path.join(mod_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_mod_params \{(.*?)\} nae_mod_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(double|uint32_t|int)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("double", "delay"), ("double", "depth"), ("double", "feedback"), ("double", "wet,dry"),
                                                            ("uint32_t", "rate_inc"), ("uint32_t", "phase0"), ("uint32_t", "phase_ch"), ("int", "n_voices"),
                                                            ("uint32_t", "voice_phase[NAE_MOD_MAX_VOICES]"), ("int", "shape")]
    with pytest.raises(nae.NaeError):
        nae.ModParams.make(10.0, 1.0, voice_phase=(0,) * 5)
    assert re.search(r"^ \*   mod_sub\s", header, re.M) and "#define NAE_ABI_VERSION 3" in header
    assert all(s in nae.EXPORTED_SYMBOLS for s in ("nae_mod_design", "nae_mod_block_f32", "nae_mod_create", "nae_mod_put", "nae_mod_put_host",
                                                   "nae_mod_flush", "nae_mod_available", "nae_mod_receive", "nae_mod_receive_host", "nae_mod_destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.ModParams.make(20.0, 5.0, 0.5)
    h = C.c_void_p()
    assert lib.nae_mod_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_mod_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_mod_put(None, None, 0) == INVALID and lib.nae_mod_put_host(None, None, 0) == INVALID
    assert lib.nae_mod_flush(None) == INVALID and lib.nae_mod_available(None) == 0
    got = C.c_size_t()
    assert lib.nae_mod_receive(None, None, 0, C.byref(got)) == INVALID and lib.nae_mod_receive_host(None, None, 0, C.byref(got)) == INVALID
    assert lib.nae_mod_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: the nine keys round-trip, the defaults are not written back, a wrong type or value is the error
    "Wrong field: <key>" with that key"""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MOD OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the nine existing calls give 15 entries without audio_modulation, register_modulation_processors() adds it: two pins, one audio input"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MOD OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [15, 16]
    assert "audio_modulation" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_modulation"])
