"""K19 gate, no GPU: the CPU statement (tests/gate_ref/ref_gate.c) — the tiled form the GPU computes — against the plain sequential form (the
window searched sample by sample, the plain recurrence) and against a float64 numpy restatement; what the specification promises (wire, brick,
hold and look-ahead to the sample, the non-finite rule); the library's host-side design nae_gate_design against its float64 restatement; the
rejections; the header; the gate node's JSON and the twelve registration calls (tests/gate_ref/host_gate_node.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gate_ref
import node_harness
from conftest import rel_rms

# The tiled statement against the sequential form, both in double, over the cases of test_statement_against_sequential_form at 3 * 1024 + 7
# and at 300 * 1024 + 7 samples.  Every integer decision (the hysteresis state, the open gate) is equal.  Measured, relative RMS:
#   the output in front of its final rounding:  0 ... 2.5e-13 at 3 chunks, 0 ... 1.36e-11 at 300 chunks
#   the smoothed depth y:                       0 ... 3.6e-14 at 3 chunks, 0 ... 2.56e-12 at 300 chunks
# the worst each time the burst train in gate mode with the slowest attack and release, whose memory is hundreds of chunks long; with the
# fastest pair both stay under 2e-17 and 2.3e-15.  After the rounding at most 89 of 614414 f32 samples differ (none at 3 chunks).  The bounds
# are 30 times the worst case, the margin the long convolution's, the equalizer's and the dynamics' bounds have over theirs.
RMS_BOUND = 30 * 1.36e-11
DEPTH_RMS_BOUND = 30 * 2.56e-12
INVALID, UNSUPPORTED = -1, -2
LENGTHS = (3 * gate_ref.CHUNK + 7, 300 * gate_ref.CHUNK + 7)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gate_ref.build(str(tmp_path_factory.mktemp("ref_gate")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("gate_ref/host_gate_node.cpp", str(tmp_path_factory.mktemp("host_gate")))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("speed", ("fast", "slow"))
def test_statement_against_sequential_form(ref, speed, n):
    worst = worst_depth = 0.0
    most_differ = 0
    for sig, x in gate_ref.signals(n).items():
        for expand in (0, 1):
            for link in (0, 1):
                for la, hold in ((0, 0), (17, 100), (1024, 5000)):
                    p = gate_ref.params(lookahead=la, hold=hold, expand=expand, link=link, **(gate_ref.FAST if speed == "fast" else gate_ref.SLOW))
                    tiled, seq = gate_ref.full(ref, p, x, 1), gate_ref.full(ref, p, x, 0)
                    assert np.array_equal(tiled["s"], seq["s"]) and np.array_equal(tiled["open"], seq["open"]), "every integer decision, exactly"
                    err, err_depth = rel_rms(tiled["yd"], seq["yd"]), rel_rms(tiled["sm"], seq["sm"])
                    differ = int(np.sum(tiled["y"] != seq["y"]))
                    print(f"{speed} n {n} {MODE[expand]} link {link} la {la} hold {hold} {sig}: rel RMS {err:.3g} out, {err_depth:.3g} depth, in double; "
                          f"{differ} of {tiled['y'].size} f32 samples differ")
                    worst, worst_depth, most_differ = max(worst, err), max(worst_depth, err_depth), max(most_differ, differ)
                    assert err <= RMS_BOUND and err_depth <= DEPTH_RMS_BOUND, (sig, expand, link, la, hold, err, err_depth)
                    assert np.array_equal(tiled["y"], tiled["yd"].astype(np.float32)), "rounded once, at the end"
                    assert np.array_equal(tiled["y"], gate_ref.run(ref, p, x))
                    if la + hold < 200 and (sig != "decay" or n > 9000):   # the tone's first decay takes 6000 samples
                        assert 0.02 < seq["open"].mean() < 0.98, "the case opens and closes"
    print(f"worst {worst:.3g} (bound {RMS_BOUND:.3g}), depth {worst_depth:.3g} (bound {DEPTH_RMS_BOUND:.3g}); at most {most_differ} f32 samples differ")


MODE = ("gate", "expander")


def test_statement_is_the_sequential_form_inside_the_first_lane(ref):
    p = gate_ref.params(lookahead=5, hold=3, expand=1, **gate_ref.SLOW)
    x = gate_ref.signals(40)["noise"]
    assert np.array_equal(gate_ref.full(ref, p, x, 1)["yd"][:gate_ref.LANE], gate_ref.full(ref, p, x, 0)["yd"][:gate_ref.LANE])


@pytest.mark.parametrize("expand", (0, 1))
@pytest.mark.parametrize("link", (0, 1))
def test_statement_against_numpy_restatement(ref, expand, link):
    """the restatement shares no code with the C: every decision equal; the output to the functions' 2^-40 and the recurrences' rounding"""
    n = 2 * gate_ref.CHUNK + 7
    for sig, x in gate_ref.signals(n).items():
        p = gate_ref.params(lookahead=23, hold=150, expand=expand, link=link, slope=2.0, alpha_attack=gate_ref.alpha(0.001), alpha_release=gate_ref.alpha(0.02))
        seq, re_ = gate_ref.full(ref, p, x, 0), gate_ref.restate(p, x)
        assert np.array_equal(seq["open"], re_["open"]), sig
        err = rel_rms(seq["yd"], re_["yd"])
        print(f"{MODE[expand]} link {link} {sig}: rel RMS {err:.3g} against the numpy restatement")
        assert err <= 2.0 ** -36, (sig, err)


def test_link_and_channels(ref):
    """unlinked stereo is two mono runs; linked stereo is one decision on both channels, from the larger magnitude"""
    x = gate_ref.signals(1500)["bursts"]
    x[:, 1] *= 0.25
    p = gate_ref.params(lookahead=9, hold=40, link=0, expand=1)
    y = gate_ref.run(ref, p, x)
    for c in range(2):
        assert np.array_equal(y[:, c], gate_ref.run(ref, p, np.ascontiguousarray(x[:, c:c + 1]))[:, 0])
    p.link = 1
    both = gate_ref.full(ref, p, x, 1)
    assert both["sm"].shape == (1500, 1)
    loud = np.max(np.abs(x), axis=1, keepdims=True).astype(np.float32)
    assert np.array_equal(both["sm"], gate_ref.full(ref, p, loud, 1)["sm"])


@pytest.mark.parametrize("form", (0, 1))
def test_wire(ref, form):
    """alpha_attack = 0 and every magnitude at or above open_lin: the output is the input, bit for bit"""
    rng = np.random.default_rng(3)
    n = 2 * gate_ref.CHUNK + 7
    x = (rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(0.1, 1.0, (n, 2))).astype(np.float32)
    x[5] = 0.1                                             # exactly open_lin
    for expand in (0, 1):
        for link in (0, 1):
            p = gate_ref.params(open_lin=0.1, close_lin=0.05, alpha_attack=0.0, alpha_release=gate_ref.alpha(0.1), expand=expand, link=link, hold=3, lookahead=7)
            assert np.array_equal(gate_ref.full(ref, p, x, form)["y"].view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("form", (0, 1))
def test_brick(ref, form):
    """both alphas 0, no hold, no look-ahead, one threshold, gate mode: a sample under open_lin is x times one constant, every other is x"""
    rng = np.random.default_rng(4)
    n = 2 * gate_ref.CHUNK + 7
    x = rng.uniform(-1, 1, (n, 1)).astype(np.float32)
    x[7], x[8], x[9] = 0.25, np.nextafter(np.float32(0.25), np.float32(0)), 0.125
    p = gate_ref.params(open_lin=0.25, close_lin=0.25, range_db=37.0, alpha_attack=0.0, alpha_release=0.0)
    out = gate_ref.full(ref, p, x, form)
    below = np.abs(x) < np.float32(0.25)
    assert below[8] and not below[7] and 0.1 < below.mean() < 0.9
    g = out["yd"][9, 0] / 0.125                            # exact: a power of two
    assert abs(g / 10.0 ** (-37.0 / 20.0) - 1.0) <= 2.0 ** -40, "the one constant dyn_exp2(-range_db KINV)"
    assert np.array_equal(out["yd"][below], x[below].astype(np.float64) * g)
    assert np.array_equal(out["y"][below], (x[below].astype(np.float64) * g).astype(np.float32))
    assert np.array_equal(out["y"][~below].view(np.uint32), x[~below].view(np.uint32))


@pytest.mark.parametrize("hold", (0, 1, 15, 16, 17, 1024, 5000))
def test_hold_to_the_sample(ref, hold):
    """the gate stays open for exactly `hold` samples behind the last s = 1"""
    n, i = 7 * gate_ref.CHUNK, 1030
    x = np.full((n, 1), 0.001, np.float32)
    x[i - 3:i + 1] = 0.5
    p = gate_ref.params(open_lin=0.1, close_lin=0.05, hold=hold, **gate_ref.FAST)
    for form in (0, 1):
        o = gate_ref.full(ref, p, x, form)["open"][:, 0]
        want = np.zeros(n, np.uint8)
        want[i - 3:i + hold + 1] = 1
        assert np.array_equal(o, want), (hold, form)


@pytest.mark.parametrize("la", (0, 1, 15, 16, 17, 1023, 1024))
def test_lookahead_to_the_sample(ref, la):
    """the gate opens exactly `lookahead` samples before the first s = 1, and the output before it is untouched by the click"""
    n, i = 4 * gate_ref.CHUNK, 2 * gate_ref.CHUNK
    x = np.full((n, 1), 0.001, np.float32)
    x[i] = 0.5
    p = gate_ref.params(open_lin=0.1, close_lin=0.05, lookahead=la, hold=2, **gate_ref.FAST)
    quiet = x.copy()
    quiet[i] = 0.001
    for form in (0, 1):
        out = gate_ref.full(ref, p, x, form)
        want = np.zeros(n, np.uint8)
        want[i - la:i + 3] = 1
        assert np.array_equal(out["open"][:, 0], want), (la, form)
        assert np.array_equal(out["y"][:i - la], gate_ref.full(ref, p, quiet, form)["y"][:i - la])
        assert out["y"][i, 0] == x[i, 0], "attack 0: the click itself passes"


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("expand", (0, 1))
def test_non_finite_sample(ref, expand, bad):
    """a non-finite sample i leaves every output sample before i - lookahead as it was; a NaN keeps the hysteresis state"""
    n, i, la = 3 * gate_ref.CHUNK + 7, 2000, 37
    x = gate_ref.signals(n)["noise"]
    p = gate_ref.params(lookahead=la, hold=50, expand=expand, link=1, **gate_ref.SLOW)
    clean = gate_ref.full(ref, p, x, 1)
    dirty_x = x.copy()
    dirty_x[i, 0] = bad
    dirty = gate_ref.full(ref, p, dirty_x, 1)
    assert np.array_equal(dirty["y"][:i - la].view(np.uint32), clean["y"][:i - la].view(np.uint32))
    assert np.all(np.isfinite(dirty["sm"])), "the depth stays finite"
    if np.isnan(bad):
        assert dirty["s"][i, 0] == dirty["s"][i - 1, 0]
    else:
        assert dirty["s"][i, 0] == 1


DESIGNS = ((48000, "gate", -40.0, 3.0, 60.0, 2.0, 0.001, 0.05, 0.1, 0.0, 1), (44100, "expander", -90.0, 24.0, 120.0, 100.0, 0.0, 0.0, 0.001, 0.02, 0),
           (48000, "expander", 0.0, 0.0, 0.0, 1.0, 0.5, 10.0, 5.0, 1024 / 48000, 1), (96000, "gate", -1.0, 0.5, 33.3, 7.5, 1e-4, 0.0123, 0.25, 0.01, 0),
           (8000, "expander", -30.0, 12.0, 80.0, 2.0, 0.03, 1.0, 1.0, 0.128, 1), (44100, "gate", -12.0, 1.5, 20.0, 1.5, 0.0101, 0.3337, 0.3337, 0.0115, 1))


@pytest.mark.parametrize("args", DESIGNS)
def test_design_against_float64_restatement(nae, ref, args):
    """bound: 1 ulp of double per real parameter and 1 ulp of f32 per threshold (the same libm behind both), the integers equal"""
    got = nae.Context.gate_design(*args)
    want = gate_ref.design(*args)
    stated = gate_ref.Params()
    assert ref.ref_gate_design(args[0], gate_ref.MODES.index(args[1]), *args[2:], C.byref(stated)) == 0
    g, w = np.array(gate_ref.as_tuple(got)[2:7]), np.array(gate_ref.as_tuple(want)[2:7])
    ulps = int(np.abs(g.view(np.int64) - w.view(np.int64)).max())
    gf, wf = np.array(gate_ref.as_tuple(got)[:2], np.float32), np.array(gate_ref.as_tuple(want)[:2], np.float32)
    ulps_f = int(np.abs(gf.view(np.int32) - wf.view(np.int32)).max())
    print(f"{args}: worst {ulps} ulp of double, {ulps_f} ulp of f32; thresholds {got.open_lin} {got.close_lin}, slope {got.slope}, alphas {got.alpha_attack} "
          f"{got.alpha_release}, hold {got.hold}, lookahead {got.lookahead}")
    assert ulps <= 1 and ulps_f <= 1 and gate_ref.as_tuple(got)[7:] == gate_ref.as_tuple(want)[7:]
    assert gate_ref.as_tuple(got) == gate_ref.as_tuple(stated), "the statement's design is the library's"
    assert ref.ref_gate_check(C.byref(stated)) == 0
    assert C.sizeof(nae.GateParams) == C.sizeof(gate_ref.Params) == 64


def test_design_rejections(nae):
    lib = nae.load_library()
    out = nae.GateParams()
    good = dict(sample_rate=48000, mode=0, threshold_db=-40.0, hysteresis_db=3.0, range_db=60.0, ratio=2.0, attack_s=0.001, hold_s=0.05, release_s=0.1,
                lookahead_s=0.0, link=1)

    def des(p=C.byref(out), **kw):
        a = dict(good, **kw)
        return lib.nae_gate_design(a["sample_rate"], a["mode"], a["threshold_db"], a["hysteresis_db"], a["range_db"], a["ratio"], a["attack_s"], a["hold_s"],
                                   a["release_s"], a["lookahead_s"], a["link"], p)

    nan, inf = float("nan"), float("inf")
    assert des() == 0 and out.expand == 0 and out.slope == 1.0 and out.hold == 2400 and des(mode=1) == 0 and out.expand == 1
    assert des(attack_s=0.0) == 0 and out.alpha_attack == 0.0
    assert des(hysteresis_db=0.0) == 0 and out.open_lin == out.close_lin
    bad = {"sample_rate": (0, -48000), "mode": (2, -1), "threshold_db": (-90.001, 0.001, nan, inf), "hysteresis_db": (-0.001, 24.001, nan, inf),
           "range_db": (-0.001, 120.001, nan, inf), "ratio": (0.999, 100.001, 0.0, nan, inf), "attack_s": (-0.001, 0.501, nan, inf),
           "hold_s": (-0.001, 10.001, nan, inf), "release_s": (0.0, 0.0009, 5.001, nan, inf), "lookahead_s": (-0.001, nan, inf), "link": (2, -1)}
    for key, values in bad.items():
        for v in values:
            assert des(**{key: v}) == INVALID, (key, v)
    for key, values in {"threshold_db": (-90.0, 0.0), "hysteresis_db": (0.0, 24.0), "range_db": (0.0, 120.0), "ratio": (1.0, 100.0), "attack_s": (0.0, 0.5),
                        "hold_s": (0.0, 10.0), "release_s": (0.001, 5.0), "link": (0, 1), "mode": (0, 1)}.items():
        for v in values:
            assert des(**{key: v}) == 0, (key, v)
    assert des(lookahead_s=1024 / 48000) == 0 and out.lookahead == 1024
    assert des(lookahead_s=1025 / 48000) == UNSUPPORTED and des(lookahead_s=0.02, sample_rate=96000) == UNSUPPORTED and des(lookahead_s=1e6) == UNSUPPORTED
    assert des(hold_s=10.0, sample_rate=209715) == 0 and out.hold == 2097150
    assert des(hold_s=10.0, sample_rate=209716) == UNSUPPORTED and des(hold_s=10.0, sample_rate=1 << 30) == UNSUPPORTED
    assert des(p=None) == INVALID
    with pytest.raises(nae.NaeError):
        nae.Context.gate_design(48000, threshold_db=1.0)


BAD_PARAMS = (dict(open_lin=0.1, close_lin=0.2), dict(open_lin=0.1, close_lin=0.0), dict(open_lin=0.1, close_lin=-0.05), dict(open_lin=float("inf"), close_lin=0.1),
              dict(open_lin=float("nan"), close_lin=0.1), dict(open_lin=0.1, close_lin=float("nan")), dict(threshold_db=0.5), dict(threshold_db=-90.5),
              dict(threshold_db=float("nan")), dict(slope=-0.1), dict(slope=99.5), dict(slope=float("inf")), dict(range_db=-1.0), dict(range_db=120.5),
              dict(range_db=float("nan")), dict(alpha_attack=1.0), dict(alpha_attack=-0.1), dict(alpha_release=1.0), dict(alpha_release=float("nan")),
              dict(hold=-1), dict(lookahead=-1), dict(expand=2), dict(expand=-1), dict(link=2), dict(link=-1))
TOO_FAR = (dict(lookahead=1025), dict(hold=gate_ref.MAX_HOLD + 1))


def test_statement_rejects_what_the_library_rejects(ref):
    assert ref.ref_gate_check(C.byref(gate_ref.params())) == 0
    assert ref.ref_gate_check(C.byref(gate_ref.params(lookahead=1024, hold=gate_ref.MAX_HOLD, open_lin=0.1, close_lin=0.1))) == 0
    for kw in TOO_FAR:
        assert ref.ref_gate_check(C.byref(gate_ref.params(**kw))) == UNSUPPORTED, kw
    for kw in BAD_PARAMS:
        assert ref.ref_gate_check(C.byref(gate_ref.params(**kw))) == INVALID, kw


def test_header_and_binding(nae):
    """the constants beside K12's, the record's layout, the additions list, the ABI version stays 3"""
    spec = open(os.path.join(gate_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_GATE_MAX_HOLD\s+\(1 << 21\)\s*$", spec, re.M)
    assert nae.GATE_MAX_HOLD == gate_ref.MAX_HOLD == 1 << 21 and nae.GATE_MODES == gate_ref.MODES
    assert C.sizeof(nae.GateParams) == C.sizeof(gate_ref.Params) == 64
    for name, _ in gate_ref.Params._fields_:
        assert getattr(nae.GateParams, name).offset == getattr(gate_ref.Params, name).offset, name
    header = open(os.path.join(gate_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_gate_params \{(.*?)\} nae_gate_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|double|int)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("float", "open_lin,close_lin"), ("double", "threshold_db"), ("double", "slope"), ("double", "range_db"),
                                                            ("double", "alpha_attack,alpha_release"), ("int", "hold"), ("int", "lookahead"), ("int", "expand"),
                                                            ("int", "link")]
    additions = re.search(r"Later additions within 3(.*?)\*/", header, re.S).group(1)
    assert "nae_gate_design, nae_gate_block_f32 and the nae_gate handle" in additions and "K19" in additions
    assert "#define NAE_ABI_VERSION 3" in header and nae.load_library().nae_abi_version() == 3
    assert all("nae_gate_" + s in nae.EXPORTED_SYMBOLS for s in ("design", "block_f32", "create", "put", "put_host", "flush", "available", "receive",
                                                                  "receive_host", "destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.GateParams(*gate_ref.as_tuple(gate_ref.params()))
    h = C.c_void_p()
    assert lib.nae_gate_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_gate_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_gate_put(None, None, 0) == INVALID and lib.nae_gate_put_host(None, None, 0) == INVALID
    assert lib.nae_gate_flush(None) == INVALID and lib.nae_gate_available(None) == 0
    assert lib.nae_gate_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST GATE OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the eleven existing calls keep their counts and give 17 entries without audio_gate, register_gate_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST GATE OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [17, 18]
    assert "audio_gate" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_gate"])
