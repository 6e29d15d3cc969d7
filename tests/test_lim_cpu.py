"""K22 limiter without a GPU: the CPU statement (tests/lim_ref/ref_lim.c) in its tiled and its sequential form and against the float64 numpy
restatement (tests/lim_ref.py), the properties DESIGN.md §3 "K22 limiter" states (the sample ceiling, s >= r, W as integers, no ramp at the
start, the non-finite rule, the limit cases), the true peak of the output by the restatement of K14's meter, the design, the header, the
node's JSON and the fifteen registration calls (tests/lim_ref/host_lim_node.cpp).  The measured figures stand beside their asserts."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_ref
import lim_ref
import node_harness

INVALID, UNSUPPORTED = -1, -2
LOOKAHEADS = (0, 1, 15, 16, 17, 1018)
# tiled against sequential.  The release's output y1 in its two forms: worst relative RMS measured 1.19e-13 over the cases below (5.57e-14
# over 300 chunks); in front of the final rounding the two forms measured EQUAL on every case of 3 chunks and 2.17e-12 apart over 300 chunks
# (1022 of 614414 samples differ, the worst by 9.4e-11): q = ceil(y1 2^24) takes the difference out except where y1 2^24 lies within its
# error of an integer.  The bounds are K12's margin of 30 on the worst figure measured.  Where the forms do differ, q differs by 1 and sits in
# the windows of la + 1 samples: s differs by at most 2^-24 dB (by 2^-24 / 73 dB at la = 72: the 9.4e-11) and the gain by at most
# 2^-24 ln(10) / 20 = 6.9e-9 relative: that holds every single sample.
Y1_RMS_BOUND = 30 * 1.19e-13
RMS_BOUND = 30 * 2.17e-12
SAMPLE_BOUND = 2.0 ** -24 * math.log(10.0) / 20.0
# statement against the float64 restatement: worst output distance measured 2.17e-7 (true_peak = 1: the restatement's taps are not rounded to
# f32; 7.77e-15 with true_peak = 0), the bound is K12's margin of 4
F64_BOUND = 4 * 2.17e-7
F64_BOUND_SAMPLE_PEAK = 4 * 7.77e-15
TP_TOLERANCE_DB = 0.2          # EBU Tech 3341's meter tolerance, the bound K14's own test uses


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lim_ref.build(str(tmp_path_factory.mktemp("lim_ref")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("lim_ref/host_lim_node.cpp", str(tmp_path_factory.mktemp("host_lim")))


@pytest.fixture(scope="module")
def cases(ref):
    """every signal at every look-ahead, detector, link and release: (name, params, x, tiled, sequential), computed once"""
    out = []
    for name, x in lim_ref.signals().items():
        for la, tp, link, ar in itertools.product(LOOKAHEADS, (0, 1), (0, 1), (lim_ref.FAST, lim_ref.SLOW)):
            p = lim_ref.params(lookahead=la, true_peak=tp, link=link, alpha_release=ar)
            out.append((name, p, x, lim_ref.full(ref, p, x, True), lim_ref.full(ref, p, x, False)))
    return out


def sample_distance(a, b):
    """the largest relative distance of one sample, and how many samples differ"""
    d = np.abs(a - b)
    return float(np.max(d / np.maximum(np.abs(b), 1e-300))) if np.any(d) else 0.0, int(np.count_nonzero(d))


def rel_rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2))) if np.any(b) else float(np.max(np.abs(a - b)))


def test_sample_ceiling_and_integer_sums(cases):
    """on every case: no output sample above 10^(ceiling / 20) (1 + 2^-22); s >= r exactly; W of the prefix sums equals the brute-force sum as
    integers; the statement's f32 output is its double output rounded once"""
    worst = 0.0
    for name, p, x, t, s in cases:
        top = 10.0 ** (p.ceiling_db / 20.0) * lim_ref.CEILING_SLACK
        worst = max(worst, float(np.max(np.abs(t["y"].astype(np.float64)))) / 10.0 ** (p.ceiling_db / 20.0))
        assert np.all(np.abs(t["y"].astype(np.float64)) <= top), (name, lim_ref.as_tuple(p))
        assert np.all(t["s"] >= t["r"]) and np.all(s["s"] >= s["r"]), (name, lim_ref.as_tuple(p))
        assert np.array_equal(t["w"], s["w"]), (name, lim_ref.as_tuple(p))
        assert np.array_equal(t["y"], t["yd"].astype(np.float32))
    print(f"largest |y| over the ceiling: {worst:.9f}")   # measured 0.999999967: s lies on or above r, and the rounding to f32 did not lift a sample over the ceiling
    assert worst > 0.999, "the cases are driven into the ceiling"


def test_statement_against_sequential_form(cases):
    worst_y1 = worst = worst_one = 0.0
    differing = 0
    for name, p, x, t, s in cases:
        worst_y1 = max(worst_y1, rel_rms(t["y1"], s["y1"]))
        worst = max(worst, rel_rms(t["yd"], s["yd"]))
        one, count = sample_distance(t["yd"], s["yd"])
        worst_one, differing = max(worst_one, one), differing + count
    print(f"tiled against sequential: y1 {worst_y1:.3g}, in front of the final rounding {worst:.3g}, "
          f"one sample {worst_one:.3g}, {differing} samples differ")   # 1.19e-13, 0, 0, 0
    assert worst_y1 <= Y1_RMS_BOUND and worst <= RMS_BOUND and worst_one <= SAMPLE_BOUND


def test_statement_against_numpy_restatement(cases):
    worst = {0: 0.0, 1: 0.0}
    for name, p, x, t, s in cases:
        f = lim_ref.restate(p, x)
        assert np.allclose(f["r"], t["r"], rtol=0, atol=1e-5), name
        worst[p.true_peak] = max(worst[p.true_peak], float(np.max(np.abs(t["yd"] - f["yd"]))))
    print(f"statement against float64: true_peak 1 {worst[1]:.3g}, true_peak 0 {worst[0]:.3g}")   # 2.17e-7, 7.77e-15
    assert worst[1] <= F64_BOUND and worst[0] <= F64_BOUND_SAMPLE_PEAK


def test_steady_state(ref):
    """300 chunks at the 5 s release: the release's memory spans hundreds of chunks and the running total of q passes 2^45; the tiled form
    stays at the sequential one, the ceiling holds and s >= r"""
    n = 300 * lim_ref.CHUNK + 7
    rng = np.random.default_rng(300)
    x = (rng.uniform(-1, 1, (n, 2)) * (0.3 + 0.7 * (np.arange(n) % 40000 < 9000))[:, None]).astype(np.float32)
    p = lim_ref.params(lookahead=72, alpha_release=lim_ref.SLOW)
    t, s = lim_ref.full(ref, p, x, True), lim_ref.full(ref, p, x, False)
    one, count = sample_distance(t["yd"], s["yd"])
    print(f"300 chunks: y1 {rel_rms(t['y1'], s['y1']):.3g}, in front of the final rounding {rel_rms(t['yd'], s['yd']):.3g}, "
          f"one sample {one:.3g}, {count} of {t['yd'].size} samples differ")   # 5.57e-14, 2.17e-12, 9.4e-11, 1022
    assert rel_rms(t["y1"], s["y1"]) <= Y1_RMS_BOUND and rel_rms(t["yd"], s["yd"]) <= RMS_BOUND and one <= SAMPLE_BOUND
    assert np.all(t["s"] >= t["r"]) and np.all(np.abs(t["yd"]) <= 10.0 ** (p.ceiling_db / 20.0) * lim_ref.CEILING_SLACK)
    assert float(np.cumsum(np.ceil(t["y1"][:, 0] * lim_ref.Q_SCALE))[-1]) > 2.0 ** 45


def test_start_of_a_stream_has_no_ramp(ref):
    """q[n] = q[0] below 0: the window at sample 0 holds la + 1 times q[0], so s[0] = q[0] / 2^24 >= r[0] and a steady signal has its steady
    gain from the first sample on"""
    n = 2 * lim_ref.CHUNK
    x = np.full((n, 1), 0.9, np.float32) * np.where(np.arange(n) % 2, -1, 1)[:, None].astype(np.float32)
    for la in LOOKAHEADS:
        for tp in (0, 1):
            p = lim_ref.params(lookahead=la, true_peak=tp, link=0, gain_db=6.0, alpha_release=lim_ref.alpha(0.1))
            t = lim_ref.full(ref, p, x, True)
            assert t["s"][0, 0] == math.ceil(t["y1"][0, 0] * lim_ref.Q_SCALE) / lim_ref.Q_SCALE and t["w"][0, 0] == (la + 1) * math.ceil(t["y1"][0, 0] * lim_ref.Q_SCALE)
            if not tp:
                # a square wave's sample level is steady: the gain is too, from sample 0 on
                assert np.ptp(t["s"][:, 0]) == 0.0 and np.ptp(np.abs(t["y"])) == 0.0, la


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_sample(ref, bad):
    """a non-finite sample i leaves every output before i - la - D bit-identical to the clean run, in both forms; the statement returns 0"""
    x = lim_ref.signals()["noise"]
    i = 2 * lim_ref.CHUNK + 5
    dirty = x.copy()
    dirty[i, 0] = bad
    for la, tp, link in itertools.product((0, 17, 1018), (0, 1), (0, 1)):
        p = lim_ref.params(lookahead=la, true_peak=tp, link=link)
        stop = i - la - lim_ref.reach(p)
        for tiled in (True, False):
            a, b = lim_ref.full(ref, p, x, tiled)["y"], lim_ref.full(ref, p, dirty, tiled)["y"]
            assert np.array_equal(a[:stop].view(np.uint32), b[:stop].view(np.uint32)), (la, tp, link, tiled)
            if not link:
                assert np.array_equal(a[:, 1].view(np.uint32), b[:, 1].view(np.uint32)), "the other channel's detector is its own"
        clean_r, dirty_r = lim_ref.full(ref, p, x, True)["r"], lim_ref.full(ref, p, dirty, True)["r"]
        assert np.array_equal(clean_r[:i - lim_ref.reach(p)], dirty_r[:i - lim_ref.reach(p)]) and (la == 0 or not np.array_equal(clean_r, dirty_r))


def test_brick_wall_is_k12s_limiter(ref, tmp_path):
    """la = 0, true_peak = 0, gain_db = 0: K12 in limiter mode with attack 0 at the same release, but for the rounding of y1 up to the 2^-24 dB
    grid: the outputs lie within 2^-24 ln(10) / 20 of K12's, relatively, and never above them"""
    K12 = dyn_ref.build(str(tmp_path))
    x = lim_ref.signals()["bursts"]
    for ar in (lim_ref.FAST, lim_ref.SLOW):
        p = lim_ref.params(lookahead=0, true_peak=0, gain_db=0.0, ceiling_db=-6.0, alpha_release=ar)
        d = dyn_ref.params(threshold_db=-6.0, slope=1.0, knee_db=0.0, alpha_attack=0.0, alpha_release=ar, makeup_db=0.0, lookahead=0, link=1)
        a, b = lim_ref.full(ref, p, x, True)["yd"], dyn_ref.run_f64(K12, d, x)
        assert np.all(np.abs(a) <= np.abs(b)) and np.all(np.abs(a - b) <= SAMPLE_BOUND * 1.01 * np.abs(b))


def test_clipper_by_gain(ref):
    """alpha_release = 0 and la = 0: memoryless.  A sample whose level lies above the ceiling comes out at the ceiling, every other one comes
    out bit for bit (gain_db = 0: dyn_exp2(0) is 1)"""
    x = lim_ref.signals()["noise"][:, :1].copy()
    p = lim_ref.params(lookahead=0, true_peak=0, gain_db=0.0, ceiling_db=-6.0, alpha_release=0.0, link=0)
    t = lim_ref.full(ref, p, x, True)
    c = 10.0 ** (-6.0 / 20.0)
    over = t["r"][:, 0] > 0
    assert 0.3 < over.mean() < 0.7
    assert np.array_equal(t["y"][~over].view(np.uint32), x[~over].view(np.uint32))
    assert np.all(np.abs(t["yd"][over]) <= c * lim_ref.CEILING_SLACK) and np.all(np.abs(t["yd"][over]) >= c * (1.0 - 1e-7))
    assert np.array_equal(t["s"][:, 0] * lim_ref.Q_SCALE, np.ceil(t["r"][:, 0] * lim_ref.Q_SCALE)), "s is r on the 2^-24 dB grid"


def test_true_peak_of_the_output(cases):
    """by the restatement of K14's meter.  On the fs/4 sine the true-peak detector's output reads lower than the sample-peak detector's; for
    la >= 16 every signal reads at most ceiling + 0.2 dB; for la < 16 the overshoot is printed and written down, not capped.
    Measured with the statement, linked and unlinked, both releases: at most 0.032 dB over the ceiling at la = 16, 0.029 dB at la = 17 and
    0.0001 dB at la = 1018; 0.54 dB at la = 0, 0.32 dB at la = 1, 0.034 dB at la = 15.  The sample-peak detector leaves the fs/4 sine at
    +2.34 dBTP, the true-peak detector at -1.00 ... -0.96 dBTP."""
    over = {la: -100.0 for la in LOOKAHEADS}
    fs4 = {0: [], 1: []}
    for name, p, x, t, s in cases:
        tp = lim_ref.true_peak_db(t["y"])
        if name == "fs4":
            fs4[p.true_peak].append(tp)
        if p.true_peak:
            over[p.lookahead] = max(over[p.lookahead], tp - p.ceiling_db)
    print("true peak over the ceiling in dB by look-ahead:", {la: round(v, 4) for la, v in over.items()})
    print(f"fs/4 sine: sample-peak detector {min(fs4[0]):.2f} ... {max(fs4[0]):.2f} dBTP, true-peak detector {min(fs4[1]):.2f} ... {max(fs4[1]):.2f} dBTP")
    assert max(fs4[1]) < min(fs4[0]) and min(fs4[0]) > 2.0 and max(fs4[1]) <= -1.0 + TP_TOLERANCE_DB
    for la in LOOKAHEADS:
        if la >= 16:
            assert over[la] <= TP_TOLERANCE_DB, (la, over[la])


DESIGNS = ((48000, -1.0, 0.0, 0.1, 0.0015, 1, 1), (44100, -20.0, 24.0, 0.001, 0.02, 0, 0), (96000, 0.0, -24.0, 5.0, 0.0, 1, 0),
           (8000, -0.3, 6.0, 0.25, 0.12725, 0, 1), (192000, -3.0, 3.0, 1.0, 0.0053, 1, 1))


@pytest.mark.parametrize("args", DESIGNS)
def test_design_against_float64_restatement(nae, ref, args):
    """the library's design, the statement's and the float64 restatement: the integers equal, alpha within 1 ulp"""
    want = lim_ref.design(*args)
    lib_p = nae.LimParams()
    assert nae.load_library().nae_lim_design(*args, C.byref(lib_p)) == 0
    c_p = lim_ref.Params()
    assert ref.ref_lim_design(*args, C.byref(c_p)) == 0
    for got in (lib_p, c_p):
        assert (got.lookahead, got.true_peak, got.link, got.ceiling_db, got.gain_db) == (want.lookahead, want.true_peak, want.link, want.ceiling_db, want.gain_db)
        assert abs(got.alpha_release - want.alpha_release) <= np.spacing(want.alpha_release)
    assert nae.Context.lim_design(args[0], args[1], args[2], args[3], args[4], bool(args[5]), bool(args[6])).lookahead == want.lookahead


def test_design_rejections(nae, ref):
    lib = nae.load_library()
    out = nae.LimParams()
    c_out = lim_ref.Params()
    good = dict(sample_rate=48000, ceiling_db=-1.0, gain_db=0.0, release_s=0.1, lookahead_s=0.0015, true_peak=1, link=1)

    def des(p=True, **kw):
        a = dict(good, **kw)
        args = (a["sample_rate"], a["ceiling_db"], a["gain_db"], a["release_s"], a["lookahead_s"], a["true_peak"], a["link"])
        rc = lib.nae_lim_design(*args, C.byref(out) if p else None)
        assert ref.ref_lim_design(*args, C.byref(c_out) if p else None) == rc, "the statement's design refuses what the library's does"
        return rc

    nan, inf = float("nan"), float("inf")
    assert des() == 0 and out.lookahead == 72 and out.true_peak == 1 and out.link == 1
    bad = {"sample_rate": (0, -48000), "ceiling_db": (-20.001, 0.001, nan, inf), "gain_db": (-24.001, 24.001, nan, inf),
           "release_s": (0.0, 0.0009, 5.001, nan, inf), "lookahead_s": (-0.001, nan, inf), "true_peak": (2, -1), "link": (2, -1)}
    for key, values in bad.items():
        for v in values:
            assert des(**{key: v}) == INVALID, (key, v)
    for key, values in {"ceiling_db": (-20.0, 0.0), "gain_db": (-24.0, 24.0), "release_s": (0.001, 5.0), "true_peak": (0, 1), "link": (0, 1)}.items():
        for v in values:
            assert des(**{key: v}) == 0, (key, v)
    assert des(lookahead_s=1018 / 48000) == 0 and out.lookahead == 1018 == nae.LIM_MAX_LOOKAHEAD
    assert des(lookahead_s=1019 / 48000) == UNSUPPORTED and des(lookahead_s=0.02, sample_rate=96000) == UNSUPPORTED and des(lookahead_s=1e6) == UNSUPPORTED
    assert des(p=False) == INVALID
    with pytest.raises(nae.NaeError):
        nae.Context.lim_design(48000, ceiling_db=1.0)


BAD_PARAMS = (dict(ceiling_db=0.5), dict(ceiling_db=-20.5), dict(ceiling_db=float("nan")), dict(gain_db=24.5), dict(gain_db=-24.5), dict(gain_db=float("inf")),
              dict(alpha_release=1.0), dict(alpha_release=-0.1), dict(alpha_release=float("nan")), dict(lookahead=-1), dict(true_peak=2), dict(true_peak=-1),
              dict(link=2), dict(link=-1))


def test_statement_rejects_what_the_library_rejects(ref):
    assert ref.ref_lim_check(C.byref(lim_ref.params())) == 0
    assert ref.ref_lim_check(C.byref(lim_ref.params(lookahead=1018, ceiling_db=0.0, gain_db=-24.0, alpha_release=0.0))) == 0
    assert ref.ref_lim_check(C.byref(lim_ref.params(lookahead=1019))) == UNSUPPORTED
    for kw in BAD_PARAMS:
        assert ref.ref_lim_check(C.byref(lim_ref.params(**kw))) == INVALID, kw


def test_header_and_binding(nae):
    """the constants beside K12's, the record's layout, the additions list, the ABI version stays 3"""
    spec = open(os.path.join(lim_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_LIM_MAX_LOOKAHEAD\s+\(NAE_DYN_CHUNK - NAE_LIM_TP_REACH\)\s*$", spec, re.M)
    assert re.search(r"#define\s+NAE_LIM_TP_REACH\s+6\s*$", spec, re.M) and re.search(r"#define\s+NAE_LIM_Q_SCALE\s+16777216\.0\s*$", spec, re.M)
    assert nae.LIM_MAX_LOOKAHEAD == lim_ref.MAX_LOOKAHEAD == lim_ref.CHUNK - lim_ref.REACH and nae.LIM_TP_REACH == lim_ref.REACH
    assert C.sizeof(nae.LimParams) == C.sizeof(lim_ref.Params) == 40
    for name, _ in lim_ref.Params._fields_:
        assert getattr(nae.LimParams, name).offset == getattr(lim_ref.Params, name).offset, name
    header = open(os.path.join(lim_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_lim_params \{(.*?)\} nae_lim_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(float|double|int)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("double", "ceiling_db"), ("double", "gain_db"), ("double", "alpha_release"), ("int", "lookahead"),
                                                            ("int", "true_peak"), ("int", "link")]
    additions = re.search(r"Later additions within 3(.*?)\*/", header, re.S).group(1)
    assert "nae_lim_design, nae_lim_block_f32 and the nae_lim handle" in additions and "K22" in additions
    assert "#define NAE_ABI_VERSION 3" in header and nae.load_library().nae_abi_version() == 3
    assert all("nae_lim_" + s in nae.EXPORTED_SYMBOLS for s in ("design", "block_f32", "create", "put", "put_host", "flush", "available", "receive",
                                                                 "receive_host", "destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.LimParams(*lim_ref.as_tuple(lim_ref.params()))
    h = C.c_void_p()
    assert lib.nae_lim_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_lim_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_lim_put(None, None, 0) == INVALID and lib.nae_lim_put_host(None, None, 0) == INVALID
    assert lib.nae_lim_flush(None) == INVALID and lib.nae_lim_available(None) == 0
    assert lib.nae_lim_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST LIM OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the fourteen existing calls keep their counts and give 20 entries without audio_limiter, register_limiter_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST LIM OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [20, 21]
    assert "audio_limiter" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_limiter"])
