"""K12 dynamics, no GPU: the CPU statement (tests/dyn_ref/ref_dyn.c) — the tiled form the GPU computes — against the plain sequential double
recurrence; dyn_log2 and dyn_exp2 against libm; the library's host-side design nae_dyn_design against its float64 restatement; what the
sequential form promises analytically; the rejections; the dynamics node's JSON and the five registration calls
(tests/dyn_ref/host_dyn_node.cpp)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import dyn_ref
import node_harness
from conftest import rel_rms

# The tiled statement against the sequential recurrence, both in double, in front of the final rounding, over the cases below: 0 ... 2.6e-14
# (the worst: the burst train, slowest attack and release, look-ahead 1024, linked; DESIGN.md §3, "K12 dynamics").  The bound is 30 times the
# worst case, the margin the long convolution's and the equalizer's bounds have over theirs.  It was measured at 3 chunks and is kept there:
# at 300 chunks (test_statement_at_steady_state) the slow pair reaches 1.2e-13 ... 1.6e-13, which it must hold too.
RMS_BOUND = 30 * 2.6e-14
INVALID, UNSUPPORTED = -1, -2
FUNCTION_BOUND = 2.0 ** -40


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dyn_ref.build(str(tmp_path_factory.mktemp("ref_dyn")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dyn_ref/host_dyn_node.cpp", str(tmp_path_factory.mktemp("host_dyn")))


@pytest.mark.parametrize("speed", ("fast", "slow"))
@pytest.mark.parametrize("la", (0, 17, 1024))
def test_statement_against_sequential_recurrence(ref, la, speed):
    n = 3 * dyn_ref.CHUNK + 7
    worst = 0.0
    for sig, x in dyn_ref.signals(n).items():
        for link in (0, 1):
            p = dyn_ref.params(lookahead=la, link=link, **(dyn_ref.FAST if speed == "fast" else dyn_ref.SLOW))
            seq = dyn_ref.sequential(ref, p, x)
            tiled = dyn_ref.run_f64(ref, p, x)
            err = rel_rms(tiled, seq)
            y = dyn_ref.run(ref, p, x)
            print(f"{speed} la {la} link {link} {sig}: rel RMS {err:.3g} in double; {int(np.sum(y != seq.astype(np.float32)))} of {y.size} f32 samples differ")
            worst = max(worst, err)
            assert err <= RMS_BOUND, (sig, link, err)
            assert np.array_equal(y, tiled.astype(np.float32)), "rounded once, at the end"
            assert np.any(np.abs(seq) < 0.99 * np.abs(x)), "the case compresses, however slowly"
    print(f"worst {worst:.3g}, bound {RMS_BOUND:.3g}")


@pytest.mark.parametrize("la", (0, 1024))
def test_statement_at_steady_state(ref, la):
    """300 chunks with the slowest attack and release, whose memory is hundreds of chunks long: the error of the tiled form grows with
    the length (2.7e-15 at 3 chunks with these parameters) and must stay under the bound measured at 3 chunks.  Measured here: 1.2e-13 ...
    1.3e-13 without look-ahead, 1.3e-13 ... 1.6e-13 with 1024 samples of it"""
    n = 300 * dyn_ref.CHUNK + 7
    p = dyn_ref.params(lookahead=la, link=1, **dyn_ref.SLOW)
    for sig, x in dyn_ref.signals(n).items():
        seq = dyn_ref.sequential(ref, p, x)
        tiled = dyn_ref.run_f64(ref, p, x)
        err = rel_rms(tiled, seq)
        y = dyn_ref.run(ref, p, x)
        print(f"slow la {la} link 1 {sig}: rel RMS {err:.3g} in double (bound {RMS_BOUND:.3g}); {int(np.sum(y != seq.astype(np.float32)))} of {y.size} f32 samples differ")
        assert err <= RMS_BOUND, (sig, err)
        assert np.array_equal(y, tiled.astype(np.float32)), "rounded once, at the end"
        assert np.any(np.abs(seq) < 0.99 * np.abs(x)), "the case compresses, however slowly"


def test_statement_is_the_sequential_recurrence_inside_the_first_lane(ref):
    p = dyn_ref.params(lookahead=5, **dyn_ref.SLOW)
    x = dyn_ref.signals(40)["noise"]
    assert np.array_equal(dyn_ref.run_f64(ref, p, x)[:dyn_ref.LANE], dyn_ref.sequential(ref, p, x)[:dyn_ref.LANE])


def test_link_and_channels(ref):
    """unlinked stereo is two mono runs; linked stereo is one gain on both channels, from the larger magnitude"""
    x = dyn_ref.signals(1500)["bursts"]
    x[:, 1] *= 0.25
    p = dyn_ref.params(lookahead=9, link=0)
    y = dyn_ref.run(ref, p, x)
    for c in range(2):
        assert np.array_equal(y[:, c], dyn_ref.run(ref, p, np.ascontiguousarray(x[:, c:c + 1]))[:, 0])
    p.link = 1
    seq, yl = dyn_ref.sequential(ref, p, x, with_yl=True)
    assert yl.shape == (1500, 1)
    loud = np.max(np.abs(x), axis=1, keepdims=True).astype(np.float32)
    assert np.array_equal(yl, dyn_ref.sequential(ref, p, loud, with_yl=True)[1])


def test_log2_against_libm(ref):
    """absolute error at most 2^-40 over the finite non-zero f32 values: a dense sweep, every power of two, the extremes"""
    rng = np.random.default_rng(0)
    tiny, big = np.float32(1e-45), np.finfo(np.float32).max
    a = np.concatenate([np.exp(rng.uniform(math.log(1e-45), math.log(3.4e38), 2_000_000)).astype(np.float32).astype(np.float64),
                        np.linspace(0.5, 2.0, 400_001).astype(np.float32).astype(np.float64),
                        2.0 ** np.arange(-149, 128), np.nextafter(2.0 ** np.arange(-148, 128), 0).astype(np.float32).astype(np.float64),
                        np.array([tiny, big, np.finfo(np.float32).tiny, np.sqrt(2.0), np.sqrt(0.5)], np.float64)])
    a = a[a > 0]
    err = np.abs(dyn_ref.log2_v(ref, a) - np.log2(a))
    print(f"dyn_log2: worst absolute error {err.max():.3g} at {a[err.argmax()]:.9g} (bound {FUNCTION_BOUND:.3g})")
    assert err.max() <= FUNCTION_BOUND
    assert np.array_equal(dyn_ref.log2_v(ref, 2.0 ** np.arange(-149, 128)), np.arange(-149.0, 128.0)), "a power of two is exact"


def test_exp2_against_libm(ref):
    """relative error at most 2^-40 on [-200 / K, 48 / K]: a dense sweep, the integers, the half-integers next to the split"""
    lo, hi = -200.0 / dyn_ref.K, 48.0 / dyn_ref.K
    t = np.concatenate([np.linspace(lo, hi, 2_000_001), np.arange(-33.0, 8.0), np.nextafter(np.arange(-33.0, 8.0) + 0.5, 0),
                        np.arange(-33.0, 7.0) + 0.5, [lo, hi]])
    err = np.abs(dyn_ref.exp2_v(ref, t) / np.exp2(t) - 1.0)
    print(f"dyn_exp2: worst relative error {err.max():.3g} at {t[err.argmax()]:.9g} (bound {FUNCTION_BOUND:.3g})")
    assert err.max() <= FUNCTION_BOUND
    assert np.array_equal(dyn_ref.exp2_v(ref, np.arange(-33.0, 8.0)), 2.0 ** np.arange(-33.0, 8.0)), "an integer is exact"


DESIGNS = ((48000, -18.0, 4.0, 6.0, 0.005, 0.1, 0.0, 0.0, 1), (44100, -60.0, 1.0, 0.0, 0.0, 0.001, 0.02, -24.0, 0),
           (48000, 0.0, math.inf, 24.0, 0.5, 5.0, 1024 / 48000, 24.0, 1), (96000, -1.0, 100.0, 0.5, 1e-4, 0.25, 0.01, 3.5, 0),
           (8000, -30.0, 2.0, 12.0, 0.03, 1.0, 0.128, -6.0, 1), (44100, -12.0, 1.5, 3.0, 0.0101, 0.3337, 0.0115, 1.0, 1))


@pytest.mark.parametrize("args", DESIGNS)
def test_design_against_float64_restatement(nae, ref, args):
    """bound: 1 ulp of double per real parameter (the same libm exp behind both), the integers equal"""
    got = nae.Context.dyn_design(*args)
    want = dyn_ref.design(*args)
    stated = dyn_ref.Params()
    assert ref.ref_dyn_design(*args, C.byref(stated)) == 0
    g, w = np.array(dyn_ref.as_tuple(got)[:6]), np.array(dyn_ref.as_tuple(want)[:6])
    ulps = int(np.abs(g.view(np.int64) - w.view(np.int64)).max())
    print(f"{args}: worst {ulps} ulp; slope {got.slope}, alphas {got.alpha_attack} {got.alpha_release}, lookahead {got.lookahead}")
    assert ulps <= 1 and (got.lookahead, got.link) == (want.lookahead, want.link)
    assert dyn_ref.as_tuple(got) == dyn_ref.as_tuple(stated), "the statement's design is the library's"
    assert ref.ref_dyn_check(C.byref(stated)) == 0


@pytest.mark.parametrize("ratio", (2.0, 4.0, math.inf))
def test_constant_input_reaches_the_static_curve(ref, ratio):
    """a constant amplitude A: in steady state yl = r(A), the gain 10^((makeup - r(A)) / 20), below, inside and above the knee"""
    slope = 1.0 if math.isinf(ratio) else 1.0 - 1.0 / ratio
    p = dyn_ref.params(threshold_db=-20.0, slope=slope, knee_db=8.0, alpha_attack=dyn_ref.alpha(0.0005), alpha_release=dyn_ref.alpha(0.001),
                       makeup_db=2.5, lookahead=3)
    for level_db in (-40.0, -24.5, -22.0, -20.0, -17.0, -15.5, -6.0, 0.0):
        A = np.float32(10.0 ** (level_db / 20.0))
        x = np.full((6000, 1), A, np.float32)
        y = dyn_ref.sequential(ref, p, x)
        want = 10.0 ** ((p.makeup_db - dyn_ref.demand_db(p, 20.0 * math.log10(float(A)))) / 20.0)
        assert abs(y[-1, 0] / float(A) / want - 1.0) <= 1e-9, (ratio, level_db, y[-1, 0] / float(A), want)


def test_step_up_follows_the_attack_exactly(ref):
    """from silence to a constant level with release 0: yl[n] = r (1 - alpha_attack^(n + 1)), to the rounding of the recurrence"""
    aa = dyn_ref.alpha(0.002)
    p = dyn_ref.params(threshold_db=-30.0, slope=0.75, knee_db=0.0, alpha_attack=aa, alpha_release=0.0)
    x = np.full((2000, 1), 0.5, np.float32)
    _, yl = dyn_ref.sequential(ref, p, x, with_yl=True)
    r = dyn_ref.demand_db(p, 20.0 * math.log10(0.5))
    want = r * (1.0 - aa ** np.arange(1, 2001))
    assert np.max(np.abs(yl[:, 0] - want)) <= 1e-12 * r


@pytest.mark.parametrize("la", (0, 5, 300))
def test_a_lone_click_is_seen_exactly_lookahead_samples_ahead(ref, la):
    i = 1500
    x = np.full((2500, 1), 0.01, np.float32)      # -40 dB: under the threshold, no reduction
    x[i] = 0.9
    p = dyn_ref.params(threshold_db=-18.0, slope=1.0, knee_db=0.0, makeup_db=4.0, lookahead=la, **dyn_ref.FAST)
    y, yl = dyn_ref.sequential(ref, p, x, with_yl=True)
    g = 10.0 ** (4.0 / 20.0)
    assert np.all(yl[:i - la] == 0.0) and np.all(yl[i - la:i + 1] > 0.0), "the reduction starts exactly at i - la"
    assert np.max(np.abs(y[:i - la, 0] / (0.01 * g) - 1.0)) <= 1e-7, "before it the output is x times the makeup gain (x is 0.01 in f32)"
    assert abs(y[i, 0]) <= 10.0 ** ((-18.0 + 4.0) / 20.0) * (1 + 1e-12)


@pytest.mark.parametrize("la", (0, 64, 1024))
def test_brick_wall(ref, la):
    """slope 1, knee 0, no attack smoothing: no output above 10^((threshold + makeup) / 20) but by the final rounding, on noise 12 dB over it"""
    rng = np.random.default_rng(la)
    x = (rng.uniform(-1, 1, (3 * dyn_ref.CHUNK + 7, 2)) * 10.0 ** ((-18.0 + 12.0) / 20.0) * math.sqrt(3.0)).astype(np.float32)
    for link in (0, 1):
        for makeup in (0.0, 5.0):
            p = dyn_ref.params(threshold_db=-18.0, slope=1.0, knee_db=0.0, alpha_attack=0.0, alpha_release=dyn_ref.alpha(0.05), makeup_db=makeup,
                               lookahead=la, link=link)
            ceiling = 10.0 ** ((-18.0 + makeup) / 20.0)
            assert np.max(np.abs(dyn_ref.sequential(ref, p, x))) <= ceiling * (1 + 1e-12)
            y = dyn_ref.run(ref, p, x)
            assert np.max(np.abs(y)) <= ceiling * (1 + 2.0 ** -23) and np.max(np.abs(y)) > 0.9 * ceiling


def test_design_rejections(nae):
    lib = nae.load_library()
    out = nae.DynParams()
    good = dict(sample_rate=48000, threshold_db=-18.0, ratio=4.0, knee_db=6.0, attack_s=0.005, release_s=0.1, lookahead_s=0.0, makeup_db=0.0, link=1)

    def des(p=C.byref(out), **kw):
        a = dict(good, **kw)
        return lib.nae_dyn_design(a["sample_rate"], a["threshold_db"], a["ratio"], a["knee_db"], a["attack_s"], a["release_s"], a["lookahead_s"],
                                  a["makeup_db"], a["link"], p)

    nan, inf = float("nan"), float("inf")
    assert des() == 0 and des(ratio=inf) == 0 and out.slope == 1.0 and des(ratio=1.0) == 0 and out.slope == 0.0
    assert des(attack_s=0.0) == 0 and out.alpha_attack == 0.0
    bad = {"sample_rate": (0, -48000), "threshold_db": (-60.001, 0.001, nan, inf), "ratio": (0.999, 0.0, -2.0, nan, -inf),
           "knee_db": (-0.001, 24.001, nan, inf), "attack_s": (-0.001, 0.501, nan, inf), "release_s": (0.0, 0.0009, 5.001, nan, inf),
           "makeup_db": (-24.001, 24.001, nan, -inf), "lookahead_s": (-0.001, nan, inf), "link": (2, -1)}
    for key, values in bad.items():
        for v in values:
            assert des(**{key: v}) == INVALID, (key, v)
    for key, values in {"threshold_db": (-60.0, 0.0), "knee_db": (0.0, 24.0), "attack_s": (0.0, 0.5), "release_s": (0.001, 5.0),
                        "makeup_db": (-24.0, 24.0), "link": (0, 1)}.items():
        for v in values:
            assert des(**{key: v}) == 0, (key, v)
    assert des(lookahead_s=1024 / 48000) == 0 and out.lookahead == 1024
    assert des(lookahead_s=1025 / 48000) == UNSUPPORTED and des(lookahead_s=0.02, sample_rate=96000) == UNSUPPORTED and des(lookahead_s=1e6) == UNSUPPORTED
    assert des(p=None) == INVALID
    with pytest.raises(nae.NaeError):
        nae.Context.dyn_design(48000, threshold_db=1.0)


def test_statement_rejects_what_the_library_rejects(ref):
    assert ref.ref_dyn_check(C.byref(dyn_ref.params())) == 0 and ref.ref_dyn_check(C.byref(dyn_ref.params(lookahead=1024))) == 0
    assert ref.ref_dyn_check(C.byref(dyn_ref.params(lookahead=1025))) == UNSUPPORTED
    for kw in (dict(threshold_db=0.5), dict(slope=1.5), dict(knee_db=-1.0), dict(alpha_attack=1.0), dict(alpha_release=float("nan")),
               dict(makeup_db=30.0), dict(lookahead=-1), dict(link=2)):
        assert ref.ref_dyn_check(C.byref(dyn_ref.params(**kw))) == INVALID, kw


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.DynParams(*dyn_ref.as_tuple(dyn_ref.params()))
    h = C.c_void_p()
    assert lib.nae_dyn_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_dyn_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_dyn_put(None, None, 0) == INVALID and lib.nae_dyn_flush(None) == INVALID and lib.nae_dyn_available(None) == 0
    assert lib.nae_dyn_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYN OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the four existing calls give 10 entries without audio_dynamics, register_dynamics_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYN OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [10, 11]
    assert "audio_dynamics" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_dynamics"])
