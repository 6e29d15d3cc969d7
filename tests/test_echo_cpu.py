"""K16 echo, no GPU: the CPU statement (tests/echo_ref/ref_echo.c) — the tiled form against the plain sequential one; the closed forms, bit for
bit: a pure delay, an impulse's repeats, ping-pong's silent repeats and its channel symmetry; the identity that ties the statement's loop
filter to the equalizer's statement; the numpy restatement; nae_echo_design against its restatement and every rejection of the design and
of the parameter rules; the node's JSON and the nine registration calls (tests/echo_ref/host_echo_node.cpp)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import echo_ref
import eq_ref
import node_harness
from conftest import rel_rms

# The tiled statement against the sequential one, both rounded to f32 (the line is f32 in both, so they are compared as the GPU's results
# are), over the cases of test_statement_against_sequential_form: g = +-0.9, 0 / 2 / 4 sections, D = 1024 / 1500 / 4097, both `cross`
# settings, in_len = 5 (D + 1024) + 7, stereo.  Measured here (relative RMS; f32 samples that differ, of 2 in_len):
#   noise:        no section 0 and 0 samples in every case (the two forms are the same operations); 2 sections at most 1.7e-10, at most 1
#                 sample of 25254; 4 sections at most 1.8e-10, at most 1 sample of 20494
#   click train:  no section 0 and 0 samples; 2 sections at most 2.2e-10, at most 41 samples of 51224; 4 sections at most 1.9e-10, at most
#                 400 samples of 20494 (D = 1024, g = -0.9, no cross; every other case at most 57)
# The bound is the criterion tests/test_eq_cpu.py applies to f32 results against the sequential recurrence: 1e-7.  A sample that differs
# does so by one f32 rounding of a value whose two double forms straddle a rounding boundary; the line carries it round the loop, where
# |g| < 1 and a filter of gain at most 1 shrink it (the click train's quiet stretches are where such last-place differences show).
RMS_BOUND = 1e-7
INVALID, UNSUPPORTED = -1, -2
FILTERS = echo_ref.loop_filters()
DELAYS = (1024, 1500, 4097)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return echo_ref.build(str(tmp_path_factory.mktemp("ref_echo")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("echo_ref/host_echo_node.cpp", str(tmp_path_factory.mktemp("host_echo")))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def signals(n):
    """noise, and a click train whose period shares no factor with the chunk or the delays"""
    rng = np.random.default_rng(n)
    clicks = np.zeros((n, 2), np.float32)
    clicks[::997, 0] = 0.9
    clicks[331::1409, 1] = -0.8
    return {"noise": rng.uniform(-1, 1, (n, 2)).astype(np.float32), "clicks": clicks}


@pytest.mark.parametrize("D", DELAYS)
@pytest.mark.parametrize("sections", (0, 2, 4))
def test_statement_against_sequential_form(ref, sections, D):
    n = 5 * (D + 1024) + 7
    worst = {}
    for sig, x in signals(n).items():
        for g in (0.9, -0.9):
            for cross in (0, 1):
                p = echo_ref.params(D, g, cross, 0.7, 0.9, FILTERS[sections])
                tiled, seq = echo_ref.run(ref, p, x), echo_ref.sequential(ref, p, x)
                err, differ = rel_rms(tiled, seq), int(np.sum(tiled != seq))
                print(f"D {D} sections {sections} {sig} g {g} cross {cross}: rel RMS {err:.3g}, {differ} of {tiled.size} f32 samples differ")
                worst[sig] = (max(worst.get(sig, (0.0, 0))[0], err), max(worst.get(sig, (0.0, 0))[1], differ))
                assert err <= RMS_BOUND, (sig, g, cross, err)
                if sections == 0:
                    assert same_bits(tiled, seq), "with no section the two forms are the same operations"
    print(f"D {D} sections {sections}: worst (rel RMS, differing samples) {worst}, bound {RMS_BOUND}")


def test_numpy_restatement_is_the_sequential_form(ref):
    """every step one float64 operation, the line np.float32: the C statement's bits"""
    x = signals(2 * 1024 + 500)["noise"]
    for ch, delay, cross, sections in ((2, (1024, 1100), 1, 2), (2, (1030, 1024), 0, 1), (1, 1024, 0, 4), (1, 1500, 1, 0)):
        p = echo_ref.params(delay, -0.8, cross, 0.6, 0.5, FILTERS[sections])
        xs = np.ascontiguousarray(x[:, :ch])
        assert same_bits(echo_ref.sequential_np(p, xs), echo_ref.sequential(ref, p, xs)), (ch, delay, cross, sections)


@pytest.mark.parametrize("D", DELAYS)
def test_pure_delay(ref, D):
    """g = 0, dry = 0, wet = 1, no section: y is x delayed by D (values: 0 x + f may be a zero of either sign)"""
    n = 3 * D + 77
    x = signals(n)["noise"]
    for ch, delay, cross in ((1, D, 0), (2, (D, D + 13), 0), (2, (D + 5, D), 1)):
        xs = np.ascontiguousarray(x[:, :ch])
        y = echo_ref.run(ref, echo_ref.params(delay, 0.0, cross, 1.0, 0.0), xs)
        for c in range(ch):
            d = delay if ch == 1 else delay[c]
            s = 1 - c if cross else c
            want = np.concatenate([np.zeros(d, np.float32), xs[:n - d, s]])
            assert np.array_equal(y[:, c], want), (ch, delay, cross, c)


@pytest.mark.parametrize("g", (0.9, -0.9, 0.3))
def test_impulse_repeats(ref, g):
    """an impulse, no section: dry delta[n] plus wet times the repeats at n = k D; repeat k is g^(k - 1) accumulated by the line's own f32
    roundings, trip by trip, so the first repeat has amplitude wet"""
    D, wet, dry = 1500, 0.35, 0.8
    n = 6 * D + 10
    x = np.zeros((n, 1), np.float32)
    x[0] = 1.0
    y = echo_ref.run(ref, echo_ref.params(D, g, 0, wet, dry), x)[:, 0]
    want = np.zeros(n, np.float32)
    want[0] = np.float32(np.float64(dry))
    amp = np.float32(1.0)                                   # w[0] = (float)(1 + g 0)
    for k in range(1, 7):
        want[k * D] = np.float32(np.float64(wet) * np.float64(amp))
        amp = np.float32(np.float64(g) * np.float64(amp))   # w[k D] = (float)(0 + g w[(k - 1) D])
    assert np.array_equal(y, want)
    assert y[D] == np.float32(wet), "the first repeat has amplitude wet"


def test_ping_pong_alternates(ref):
    """cross, input on the left only, D_L = D_R: repeats 1, 3, 5 are exactly zero on the left, repeats 2, 4 exactly zero on the right — and
    the others are there"""
    D = 1024
    n = 6 * D + 10
    x = np.zeros((n, 2), np.float32)
    x[0, 0] = 1.0
    y = echo_ref.run(ref, echo_ref.params(D, 0.8, 1, 1.0, 1.0), x)
    for k in range(1, 6):
        quiet, loud = (0, 1) if k % 2 else (1, 0)
        assert np.all(y[k * D:(k + 1) * D, quiet] == 0.0), k
        assert y[k * D, loud] != 0.0 and np.all(y[k * D + 1:(k + 1) * D, loud] == 0.0), k


def test_ping_pong_channel_symmetry(ref):
    """swapping the input channels and the delays under cross swaps the output channels, bit for bit"""
    x = signals(4 * 2600 + 9)["noise"]
    for sections in (0, 4):
        y = echo_ref.run(ref, echo_ref.params((1024, 1500), -0.9, 1, 0.6, 0.7, FILTERS[sections]), x)
        swapped = echo_ref.run(ref, echo_ref.params((1500, 1024), -0.9, 1, 0.6, 0.7, FILTERS[sections]), np.ascontiguousarray(x[:, ::-1]))
        assert same_bits(swapped, np.ascontiguousarray(y[:, ::-1])), sections


@pytest.mark.parametrize("sections", (1, 2, 4))
def test_loop_filter_is_the_equalizer(ref, sections):
    """g = 0, dry = 0, wet = 1 and a delay of whole chunks: y[D:] is the equalizer's statement of x, bit for bit — the chunk grid of the
    delayed signal is the grid of x, and the state in front of it is zero"""
    D = 2 * echo_ref.CHUNK
    x = signals(3 * D + 333)["noise"]
    y = echo_ref.run(ref, echo_ref.params(D, 0.0, 0, 1.0, 0.0, FILTERS[sections]), x)
    want = eq_ref.run(ref, FILTERS[sections], x.reshape(-1), ch=2).reshape(x.shape)
    assert np.array_equal(y[D:], want[:len(x) - D]) and np.all(y[:D] == 0.0)


def test_line_is_what_comes_round(ref):
    """the line the statement hands out is x + g f in f32, and y - dry x is wet / g of its loop part (no section, powers of two: exact)"""
    x = signals(4000)["noise"]
    y, w = echo_ref.run(ref, echo_ref.params(1024, 0.5, 0, 0.25, 0.0), x, want_line=True)
    assert np.array_equal(w[:1024], x[:1024])
    assert np.array_equal(y[1024:], (0.25 * w[:-1024].astype(np.float64)).astype(np.float32))


DESIGNS = ((48000, 0.35, 0.35, 0.4, 0.0, 0.0, 0.35, 1.0, 0), (44100, 0.0233, 0.5, -0.99, 5000.0, 0.0, 1.0, 0.0, 1), (48000, 0.25, 0.375, 0.99, 0.0, 120.0, 0.5, 0.5, 1),
           (96000, 1024 / 96000, (1 << 20) / 96000, 0.0, 20000.0, 20.0, 0.0, 1.0, 0), (8000, 0.128, 131.072, 0.7, 3999.0, 3999.0, 2.5, -1.0, 0),
           (48000, 1023.5 / 48000, 0.1, 0.5, 0.0, 0.0, 1.0, 1.0, 0))


def test_design_against_the_restatement(nae, ref):
    lib = nae.load_library()
    for args in DESIGNS:
        got, stated = nae.EchoParams(), echo_ref.Params()
        want = echo_ref.design(*args)
        assert want is not None, args
        assert lib.nae_echo_design(*args, C.byref(got)) == 0 and ref.ref_echo_design(*args, C.byref(stated)) == 0, args
        assert echo_ref.as_tuple(got) == echo_ref.as_tuple(want) == echo_ref.as_tuple(stated), args
        assert ref.ref_echo_check(C.byref(stated), 2) == 0 and eq_ref.stable(echo_ref.coef_of(want))
    p = echo_ref.design(48000, 0.35, 0.2, 0.4, 4000.0, 100.0)
    assert (p.delay[0], p.delay[1], p.n_sections) == (16800, 9600, 2)
    assert np.array_equal(echo_ref.coef_of(p), np.stack([eq_ref.design("lowpass", 48000, 4000.0, 0.0, math.sqrt(0.5)),
                                                         eq_ref.design("highpass", 48000, 100.0, 0.0, math.sqrt(0.5))]))
    # Butterworth sections: no gain above 1 anywhere, so the designed loop with |g| < 1 is stable
    for f in np.geomspace(1.0, 23999.0, 400):
        assert eq_ref.magnitude_db(echo_ref.coef_of(p), f, 48000) <= 1e-9


def test_design_rejections(nae, ref):
    """NAE_ERR_INVALID outside the ranges, by the library, the statement and the restatement alike"""
    lib = nae.load_library()
    good = [48000, 0.35, 0.35, 0.4, 4000.0, 100.0, 0.35, 1.0, 0]
    nan, inf = float("nan"), float("inf")
    bad = []
    for i, values in ((0, (0, -48000)), (1, (1023.4 / 48000, 0.0, -0.1, ((1 << 20) + 0.6) / 48000, 1e300, nan, inf)),
                      (2, (1023.4 / 48000, ((1 << 20) + 0.6) / 48000, nan)), (3, (0.991, -0.991, 5.0, nan, inf)), (4, (-1.0, 24000.0, 30000.0, nan, inf)),
                      (5, (-1.0, 24000.0, nan, -inf)), (6, (nan, inf)), (7, (nan, -inf)), (8, (2, -1))):
        for v in values:
            bad.append(good[:i] + [v] + good[i + 1:])
    out, stated = nae.EchoParams(), echo_ref.Params()
    assert lib.nae_echo_design(*good, C.byref(out)) == 0 and lib.nae_echo_design(*good, None) == INVALID
    for args in bad:
        assert lib.nae_echo_design(*args, C.byref(out)) == INVALID, args
        assert ref.ref_echo_design(*args, C.byref(stated)) == INVALID, args
        assert echo_ref.design(*args) is None, args
    # the limits themselves
    for args in ([48000, 1024 / 48000, (1 << 20) / 48000, 0.99, 23999.0, 23999.0, 0.0, 0.0, 1], [8000, 0.128, 0.128, -0.99, 0.0, 0.0, 1.0, 1.0, 0]):
        assert lib.nae_echo_design(*args, C.byref(out)) == 0 and echo_ref.design(*args) is not None, args


def test_statement_rejects_what_the_library_rejects(ref):
    """the parameter rules (tests/test_gpu_echo.py asks the library's entries the same questions)"""
    def check(ch=2, **kw):
        args = dict(delay=(1024, 1 << 20), feedback=0.99, cross=1, wet=-3.0, dry=1e6, coef=FILTERS[4])
        args.update(kw)
        return ref.ref_echo_check(C.byref(echo_ref.params(**args)), ch)

    assert check() == 0 and check(ch=1) == 0 and check(coef=()) == 0 and check(feedback=-0.99) == 0
    assert ref.ref_echo_check(None, 2) == INVALID and check(ch=0) == INVALID and check(ch=3) == INVALID
    for key in ("feedback", "wet", "dry"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert check(**{key: v}) == INVALID, (key, v)
    assert check(feedback=0.9901) == INVALID and check(feedback=-1.0) == INVALID
    assert check(cross=2) == INVALID and check(cross=-1) == INVALID
    assert check(n_sections=-1) == INVALID and check(coef=np.repeat(FILTERS[1], 5, 0), n_sections=5) == UNSUPPORTED
    for d in (1023, 0, -1024, (1 << 20) + 1):
        assert check(delay=(d, 2048)) == UNSUPPORTED and check(delay=(2048, d)) == UNSUPPORTED, d
        assert check(ch=1, delay=(2048, d)) == 0, "mono reads delay[0] alone"
    for section in eq_ref.BAD_SECTIONS:
        assert check(coef=np.array([FILTERS[1][0], section], np.float64)) == INVALID, section
    for section in eq_ref.GOOD_SECTIONS:
        assert check(coef=np.array([FILTERS[1][0], section], np.float64)) == 0, section
    # a run with rejected parameters computes nothing
    x = np.zeros((8, 2), np.float32)
    assert ref.ref_echo_run(C.byref(echo_ref.params(1000)), x.ctypes.data, 8, 2, x.ctypes.data, 1, None) == -1


def test_record_and_limits_agree_with_the_header(nae):
    """the binding's record has the statement's layout, and the four NAE_ECHO_* constants stand in include/nae_dsp_spec.h"""
    spec = open(os.path.join(echo_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_ECHO_MIN_DELAY\s+NAE_EQ_CHUNK\b", spec) and re.search(r"#define\s+NAE_ECHO_MAX_DELAY\s+\(1 << 20\)", spec)
    assert re.search(r"#define\s+NAE_ECHO_MAX_SECTIONS\s+4\b", spec) and re.search(r"#define\s+NAE_ECHO_MAX_FEEDBACK\s+0\.99\b", spec)
    assert (nae.ECHO_MIN_DELAY, nae.ECHO_MAX_DELAY, nae.ECHO_MAX_SECTIONS, nae.ECHO_MAX_FEEDBACK) == \
        (echo_ref.MIN_DELAY, echo_ref.MAX_DELAY, echo_ref.MAX_SECTIONS, echo_ref.MAX_FEEDBACK) == (1024, 1 << 20, 4, 0.99)
    assert C.sizeof(nae.EchoParams) == C.sizeof(echo_ref.Params)
    for name in ("delay", "feedback", "cross", "wet", "dry", "n_sections", "coef"):
        assert getattr(nae.EchoParams, name).offset == getattr(echo_ref.Params, name).offset, name
    with pytest.raises(nae.NaeError):
        nae.EchoParams.make(1024, 0.5, coef=np.zeros((5, 5)))
    header = open(os.path.join(echo_ref.ROOT, "include", "nae_gpu.h")).read()
    assert re.search(r"^ \*   echo_group\s", header, re.M) and "#define NAE_ABI_VERSION 3" in header
    assert all(s in nae.EXPORTED_SYMBOLS for s in ("nae_echo_design", "nae_echo_block_f32", "nae_echo_create", "nae_echo_put", "nae_echo_put_host",
                                                   "nae_echo_flush", "nae_echo_available", "nae_echo_receive", "nae_echo_receive_host", "nae_echo_destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.EchoParams.make(2048, 0.5, coef=FILTERS[1])
    h = C.c_void_p()
    assert lib.nae_echo_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_echo_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_echo_put(None, None, 0) == INVALID and lib.nae_echo_put_host(None, None, 0) == INVALID
    assert lib.nae_echo_flush(None) == INVALID and lib.nae_echo_available(None) == 0
    got = C.c_size_t()
    assert lib.nae_echo_receive(None, None, 0, C.byref(got)) == INVALID and lib.nae_echo_receive_host(None, None, 0, C.byref(got)) == INVALID
    assert lib.nae_echo_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: the eight keys round-trip, the defaults are not written back, a wrong type or value is the error
    "Wrong field: <key>" with that key"""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST ECHO OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the eight existing calls give 14 entries without audio_echo, register_echo_processors() adds it: two pins, one audio input"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST ECHO OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [14, 15]
    assert "audio_echo" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_echo"])
