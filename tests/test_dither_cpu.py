"""K23 dither without a GPU: the CPU statement (tests/dither_ref/ref_dither.c) against restatements that share no code with it (the random
source in numpy uint64, the quantiser as a Python loop in float64), the random source's moments and correlations, what the specification
("K23 dither") says dither and shaping do, the cuts, the clamp rule, the non-finite rule, the design and the parameter rules,
the header, the node's JSON and the sixteen registration calls (tests/dither_ref/host_dither_node.cpp).

Every statistical bound is the estimator's own standard error for the N used, times FACTOR; the derivations stand at the asserts, the
figures measured at the fixed seeds beside them (and in profiles/r37_dither.md)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dither_ref
import node_harness

INVALID = -1
N = 1 << 18
FACTOR = 5.0          # standard errors allowed to an estimate of mean, variance, correlation or projection: 5.7e-7 two-sided per assert
WELCH_SEG = 1024      # 511 half-overlapping segments of N: the Welch estimate's relative standard error is 1 / sqrt(511) = 0.044
WELCH_FACTOR = 3.0    # times that: 13 % per band of 32 bins (a band's mean over 32 bins moves less than one bin does: room)
BANDS = 16
RATE = 48000


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dither_ref.build(str(tmp_path_factory.mktemp("dither_ref")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dither_ref/host_dither_node.cpp", str(tmp_path_factory.mktemp("host_dither")))


def lsb(y, bits):
    return y.astype(np.float64) * 2.0 ** (bits - 1)


# ---------------------------------------------------------------------------------------------- random source
def test_random_source_restated_in_numpy(ref):
    """key, r1 and r2 of the statement equal the numpy uint64 restatement bit for bit: at the start, across 2^32 and at 2^40"""
    for seed, s, c in ((1, 0, 0), (1, 0, 1), (1, 5, 0), (0, 0, 0), (2 ** 64 - 1, 2 ** 40, 1), (987654321, 3, 1)):
        key = int(dither_ref.key64(seed, s, c))
        assert key == ref.ref_dither_key(seed, s, c), (seed, s, c)
        for n0 in (0, 2 ** 32 - 3, 2 ** 32 + 5, 2 ** 40, 2 ** 64 - 4):
            n = (np.arange(8, dtype=np.uint64) + np.uint64(n0))
            r1, r2 = dither_ref.r12(key, n)
            for i, ni in enumerate(n):
                a, b = C.c_double(), C.c_double()
                ref.ref_dither_r12(key, int(ni), C.byref(a), C.byref(b))
                assert (a.value, b.value) == (r1[i], r2[i]), (seed, s, c, int(ni))
                assert -0.5 <= a.value < 0.5 and -0.5 <= b.value < 0.5 and a.value * 2.0 ** 32 == int(a.value * 2.0 ** 32)
    key = int(dither_ref.key64(1, 0, 0))
    for kind in dither_ref.KINDS:
        for n0 in (0, 1, 2 ** 32 + 5, 2 ** 40):
            d = dither_ref.dither(kind, key, n0, 16)
            assert [ref.ref_dither_d(key, n0 + i, dither_ref.KINDS.index(kind)) for i in range(16)] == list(d), (kind, n0)


def test_moments_of_the_random_source():
    """over N = 2^18 samples: means 0; variances 1/12 (r1), 1/6 (triangular), 1/6 (highpass).  Standard errors: the mean's is sqrt(var / N);
    the variance's is sqrt((m4 - var^2) / N) with m4 = 1/80 for the uniform and 1/15 for the sum of two, so 1/180 and 7/180 under the root;
    the highpass dither is 1-dependent: cov(d[n]^2, d[n+1]^2) = 1/30 - 1/36 = 1/180, so (7 + 2) / 180 = 1/20 under the root, and its sum
    telescopes to r1[N - 1], so its mean lies within 0.5 / N."""
    key = dither_ref.key64(1, 0, 0)
    r1, r2 = dither_ref.r12(key, np.arange(N, dtype=np.uint64))
    tri, hp = dither_ref.dither("triangular", key, 0, N), dither_ref.dither("highpass", key, 0, N)
    worst = 0.0
    for name, v, var, under in (("r1", r1, 1 / 12, 1 / 180), ("r2", r2, 1 / 12, 1 / 180), ("triangular", tri, 1 / 6, 7 / 180), ("highpass", hp, 1 / 6, 1 / 20)):
        se_mean, se_var = math.sqrt(var / N), math.sqrt(under / N)
        m, s2 = float(np.mean(v)), float(np.mean(v * v))
        worst = max(worst, abs(m) / se_mean if name != "highpass" else 0.0, abs(s2 - var) / se_var)
        assert abs(m) <= (FACTOR * se_mean if name != "highpass" else 0.5 / N), (name, m)
        assert abs(s2 - var) <= FACTOR * se_var, (name, s2, var)
    print(f"worst moment: {worst:.2f} standard errors")          # measured: profiles/r37_dither.md
    assert np.max(np.abs(tri)) < 1.0 and np.max(np.abs(hp)) < 1.0 and np.max(np.abs(tri)) > 0.99, "the triangular PDF spans +-1 LSB"


def test_channels_streams_and_seeds_are_decorrelated():
    """the correlation coefficient of two independent sequences of N samples has standard error 1 / sqrt(N): the two halves of one hash, two
    channels, two streams, two seeds, neighbouring seeds and streams, for r1 and for the triangular dither"""
    def corr(a, b):
        return float(np.sum(a * b) / math.sqrt(np.sum(a * a) * np.sum(b * b)))
    n = np.arange(N, dtype=np.uint64)
    base = dither_ref.key64(1, 0, 0)
    r1, r2 = dither_ref.r12(base, n)
    worst = abs(corr(r1, r2))
    assert worst <= FACTOR / math.sqrt(N), "the two halves of one hash"
    for what, key in (("channel", dither_ref.key64(1, 0, 1)), ("stream", dither_ref.key64(1, 1, 0)), ("seed", dither_ref.key64(2, 0, 0)),
                      ("stream and channel swapped", dither_ref.key64(1, 1, 1)), ("far stream", dither_ref.key64(1, 1023, 0)), ("seed 0", dither_ref.key64(0, 0, 0))):
        for kind in ("rectangular", "triangular", "highpass"):
            c = corr(dither_ref.dither(kind, base, 0, N), dither_ref.dither(kind, key, 0, N))
            worst = max(worst, abs(c))
            assert abs(c) <= FACTOR / math.sqrt(N), (what, kind, c)
        # and at a lag: a key that only shifted the counter would show here
        for lag in (1, 2, 64):
            c = corr(r1[lag:], dither_ref.r12(key, n)[0][:-lag])
            assert abs(c) <= FACTOR / math.sqrt(N - lag), (what, lag, c)
    print(f"worst correlation: {worst * math.sqrt(N):.2f} standard errors")


def band_means(v):
    return np.array([np.mean(b) for b in np.array_split(v[1:], BANDS)])          # bin 0 (DC) aside: 512 bins in 16 bands of 32


def test_highpass_dither_is_blue():
    """the highpass dither's PSD follows 2 (1 - cos w) / 12 in 16 bands, within the Welch estimate's standard error times WELCH_FACTOR"""
    d = dither_ref.dither("highpass", dither_ref.key64(3, 0, 0), 0, N)
    w, psd, segments = dither_ref.welch(d, WELCH_SEG)
    got, want = band_means(psd), band_means(2.0 * (1.0 - np.cos(w)) / 12.0)
    rel = np.abs(got / want - 1.0)
    print(f"highpass PSD, worst band: {rel.max():.4f} of {WELCH_FACTOR / math.sqrt(segments):.4f}")
    assert segments == 511 and np.all(rel <= WELCH_FACTOR / math.sqrt(segments)), rel


# ---------------------------------------------------------------------------------------------- rounding alone
@pytest.mark.parametrize("bits", (8, 16, 24))
def test_rounding_alone(ref, bits):
    """no dither, no taps: y S == clip(rint(x S)) exactly, ties (to even) included; +-1 and the floats just beyond clamp to S - 1 and -S"""
    S = 2.0 ** (bits - 1)
    rng = np.random.default_rng(bits)
    ties = (np.arange(-40, 40) + 0.5) / S                                         # exact in f32: at most 24 significant bits
    edge = np.array([1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2)), 1.5, -1.5, 3e38, -3e38,
                     (S - 1) / S, (S - 0.5) / S, (-S + 0.5) / S, 0.0, -0.0])
    x = np.concatenate([ties, edge, rng.uniform(-1.1, 1.1, 4000), rng.uniform(-4, 4, 4000) / S]).astype(np.float32)[:, None]
    assert np.array_equal(x[:80, 0].astype(np.float64) * S, np.arange(-40, 40) + 0.5), "the ties are ties"
    y = dither_ref.run(ref, dither_ref.params(bits, "none"), x)
    want = np.clip(np.rint(x.astype(np.float64) * S), -S, S - 1)
    assert np.array_equal(lsb(y, bits), want)
    assert lsb(y, bits)[80, 0] == S - 1 and lsb(y, bits)[81, 0] == -S and lsb(y, bits)[82, 0] == S - 1 and lsb(y, bits)[83, 0] == -S
    assert np.array_equal(want[:80, 0] % 2, np.zeros(80)), "ties go to the even neighbour"


def test_every_mode_stays_on_the_grid_and_in_range(ref):
    x = np.random.default_rng(8).uniform(-1.3, 1.3, (3000, 2)).astype(np.float32)
    for bits in (8, 16, 24):
        S = 2.0 ** (bits - 1)
        for kind in dither_ref.KINDS:
            for taps in ("none", "first", "second", "lipshitz", dither_ref.drawn_taps()):
                v = lsb(dither_ref.run(ref, dither_ref.params(bits, kind, taps), x), bits)
                assert np.array_equal(v, np.rint(v)) and v.min() >= -S and v.max() <= S - 1, (bits, kind, taps)
                assert v.min() == -S and v.max() == S - 1, "the input clips both ways"


# ---------------------------------------------------------------------------------------------- what dither is for
def test_a_sine_under_half_an_lsb(ref):
    """1 kHz at 0.4 LSB of 16 bits.  Without dither the output is identically zero.  With triangular dither y S = s + e, e of mean 0 and variance
    1/4 and uncorrelated with s = x S: the projection gain sum(y S s) / sum(s s) is 1 with standard error sqrt(1/4 / sum(s s))"""
    S = 2.0 ** 15
    x = (0.4 / S * np.sin(2 * np.pi * 1000.0 * np.arange(N) / RATE)).astype(np.float32)[:, None]
    s = x[:, 0].astype(np.float64) * S
    assert not np.any(dither_ref.run(ref, dither_ref.params(16, "none"), x)), "plain rounding loses the sine"
    v = lsb(dither_ref.run(ref, dither_ref.params(16, "triangular"), x), 16)[:, 0]
    gain, se = float(np.sum(v * s) / np.sum(s * s)), 0.5 / math.sqrt(float(np.sum(s * s)))
    print(f"projection gain {gain:.5f}, {abs(gain - 1) / se:.2f} standard errors of {se:.5f}")
    assert abs(gain - 1.0) <= FACTOR * se, (gain, se)


def test_no_noise_modulation(ref):
    """DC at f = 0, 0.1, 0.25, 0.5, 0.7 LSB.  Triangular: error mean 0 (standard error sqrt(1/4 / N)) and variance 1/4 at every offset; |e| <= 1.5,
    so var(e^2) <= E e^4 <= 2.25 E e^2 and the variance's standard error is at most 0.75 / sqrt(N).  Rectangular: e is -f with probability 1 - f and
    1 - f with probability f: mean 0, variance f (1 - f), 0 at f = 0 and 1/4 at f = 0.5; |e| <= 1 gives a standard error of at most 0.5 / sqrt(N)"""
    S = 2.0 ** 15
    worst = 0.0
    rect = {}
    for f in (0.0, 0.1, 0.25, 0.5, 0.7):
        x = np.full((N, 1), f / S, np.float32)
        t = float(x[0, 0]) * S                                                    # the offset the f32 input really has
        for kind, var, se_var in (("triangular", 0.25, 0.75 / math.sqrt(N)), ("rectangular", t * (1 - t), 0.5 / math.sqrt(N))):
            e = lsb(dither_ref.run(ref, dither_ref.params(16, kind, seed=11), x), 16)[:, 0] - t
            m, s2 = float(np.mean(e)), float(np.mean(e * e))
            worst = max(worst, abs(m) / math.sqrt(var / N) if var else 0.0, abs(s2 - var) / se_var)
            assert abs(m) <= FACTOR * math.sqrt(max(var, 1e-300) / N), (kind, f, m)
            assert abs(s2 - var) <= FACTOR * se_var, (kind, f, s2, var)
            if kind == "rectangular":
                rect[f] = s2
    print(f"worst DC moment: {worst:.2f} standard errors")
    assert rect[0.0] == 0.0 and rect[0.5] > 0.24, "rectangular dither's noise follows the signal; triangular dither's does not"


# ---------------------------------------------------------------------------------------------- shaping
@pytest.mark.parametrize("taps", ("none", "first", "second", "lipshitz", "drawn"))
def test_shaped_error_spectrum(ref, taps):
    """noise at -20 dBFS, triangular dither, 16 bits: the Welch PSD of (y - x) S in 16 bands equals 1/4 |NTF|^2 and the total power equals
    1/4 (1 + sum c^2), both within the Welch estimate's relative standard error 1 / sqrt(segments) times WELCH_FACTOR"""
    c = dither_ref.drawn_taps() if taps == "drawn" else dither_ref.PRESETS[taps]
    S = 2.0 ** 15
    x = np.random.default_rng(20).uniform(-0.1, 0.1, (N, 1)).astype(np.float32)
    y, e = dither_ref.run(ref, dither_ref.params(16, "triangular", c, seed=5), x, errors=True)
    err = (y.astype(np.float64) - x.astype(np.float64))[:, 0] * S
    w, psd, segments = dither_ref.welch(err, WELCH_SEG)
    tol = WELCH_FACTOR / math.sqrt(segments)
    got, want = band_means(psd), band_means(0.25 * dither_ref.ntf2(c, w))
    rel = np.abs(got / want - 1.0)
    total, total_want = float(np.mean(err * err)), 0.25 * (1.0 + sum(v * v for v in c))
    print(f"{taps}: worst band {rel.max():.4f}, total {abs(total / total_want - 1):.4f}, of {tol:.4f}")
    assert np.all(rel <= tol), (taps, rel)
    assert abs(total / total_want - 1.0) <= tol, (taps, total, total_want)
    # y - x = (e * ntf) / S, sample by sample: the filter on the exported errors, in float64
    shaped = e[:, 0].copy()
    for k, ck in enumerate(c):
        shaped[k + 1:] -= ck * e[:-(k + 1), 0]
    assert np.max(np.abs(shaped - err)) < 1e-6, "the output error is the error through the NTF"
    if taps == "lipshitz":
        assert abs(math.sqrt(dither_ref.ntf2(c, 0.0)) - 0.148) < 1e-3 and abs(math.sqrt(dither_ref.ntf2(c, np.pi)) - 9.36) < 5e-3


# ---------------------------------------------------------------------------------------------- the statement itself
@pytest.mark.parametrize("kind", dither_ref.KINDS)
def test_statement_against_float64_loop(ref, kind):
    """a plain Python loop over 4096 samples with the same operations gives the statement's bits, outputs and errors, at K = 0, 1, 5, 12; the
    fused step is exact in Python (rationals, rounded once), so the equality is of bits and no distance is needed"""
    x = np.random.default_rng(31).uniform(-1.05, 1.05, (4096, 1)).astype(np.float32)
    for taps in ((), dither_ref.PRESETS["first"], dither_ref.PRESETS["lipshitz"], dither_ref.drawn_taps()):
        p = dither_ref.params(16 if len(taps) != 5 else 24, kind, taps, seed=9)
        y, e = dither_ref.run(ref, p, x, stream=2, errors=True)
        y2, e2 = dither_ref.restate(p, x, stream=2)
        assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(e, e2), (kind, len(taps))


def test_cuts(ref):
    """the statement in pieces with carried state equals the whole run, bit for bit"""
    x = np.random.default_rng(41).uniform(-1, 1, (12000, 2)).astype(np.float32)
    for kind, taps in (("highpass", "lipshitz"), ("triangular", dither_ref.drawn_taps()), ("rectangular", "none"), ("highpass", "none")):
        p = dither_ref.params(16, kind, taps, seed=3)
        whole = dither_ref.run(ref, p, x, stream=4)
        for cuts in ((1,), (7,), (1000,), (1024,), (5000,), (1, 7, 1000, 1024, 5000)):
            n = 2000 if cuts == (1,) else len(x)
            assert np.array_equal(dither_ref.in_pieces(ref, p, x[:n], cuts, stream=4).view(np.uint32), whole[:n].view(np.uint32)), (kind, cuts)


def test_error_is_taken_before_the_clamp(ref):
    """a full-scale square wave through lipshitz: |e| = |rint(u + d) - u| <= 1/2 + |d| <= 1.5 LSB whether or not the sample clips; the error
    taken behind the clamp (planted in the statement) winds the shaper up past that"""
    n = np.arange(20000)
    for amp in (1.0, 1.2):
        x = (amp * np.where((n // 50) % 2 == 0, 1.0, -1.0)).astype(np.float32)[:, None]
        p = dither_ref.params(16, "triangular", "lipshitz")
        y, e = dither_ref.run(ref, p, x, errors=True)
        assert np.max(np.abs(e)) <= 1.5, np.max(np.abs(e))
        assert np.array_equal(np.unique(lsb(y, 16)), [-32768.0, 32767.0]) or amp == 1.0
        _, planted = dither_ref.run(ref, p, x, errors=True, after_clamp=True)
        assert np.max(np.abs(planted)) > 1.5, "the planted mistake shows"


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_sample_counts_as_zero(ref, bad):
    """the rule: a sample that is not finite counts as x = 0: the output stays on the grid, the error state stays finite, and the run equals
    the run on the input with a zero in its place, bit for bit"""
    x = np.random.default_rng(51).uniform(-1, 1, (500, 2)).astype(np.float32)
    dirty, zeroed = x.copy(), x.copy()
    dirty[100, 0], zeroed[100, 0] = bad, 0.0
    for kind in dither_ref.KINDS:
        for taps in ("none", "lipshitz"):
            p = dither_ref.params(16, kind, taps)
            y, e = dither_ref.run(ref, p, dirty, errors=True)
            y0, e0 = dither_ref.run(ref, p, zeroed, errors=True)
            assert np.all(np.isfinite(y)) and np.all(np.isfinite(e)) and np.array_equal(y.view(np.uint32), y0.view(np.uint32)) and np.array_equal(e, e0)


# ---------------------------------------------------------------------------------------------- design, rules, header
def test_design(nae, ref):
    """the library's presets, the statement's and the table of the specification; the rejections of both"""
    lib = nae.load_library()
    for bits in (8, 16, 24):
        for kind in range(4):
            for shaping, name in enumerate(dither_ref.SHAPINGS):
                a, b = nae.DitherParams(), dither_ref.Params()
                assert lib.nae_dither_design(bits, kind, shaping, 77, C.byref(a)) == 0 and ref.ref_dither_design(bits, kind, shaping, 77, C.byref(b)) == 0
                assert bytes(a) == bytes(b) and dither_ref.taps_of(b) == dither_ref.PRESETS[name] and (b.bits, b.kind, b.seed) == (bits, kind, 77)
                assert ref.ref_dither_check(C.byref(b), 2) == 0
    out, c_out = nae.DitherParams(), dither_ref.Params()
    for args in ((7, 2, 0, 1), (25, 2, 0, 1), (16, -1, 0, 1), (16, 4, 0, 1), (16, 2, -1, 1), (16, 2, 4, 1)):
        assert lib.nae_dither_design(*args, C.byref(out)) == INVALID and ref.ref_dither_design(*args, C.byref(c_out)) == INVALID, args
    assert lib.nae_dither_design(16, 2, 0, 1, None) == INVALID and ref.ref_dither_design(16, 2, 0, 1, None) == INVALID
    assert lib.nae_dither_design(16, 2, 3, 2 ** 64 - 1, C.byref(out)) == 0 and out.seed == 2 ** 64 - 1
    p = nae.dither_design(24, "highpass", "lipshitz", seed=5)
    assert (p.bits, p.kind, p.n_taps, p.seed) == (24, 3, 5, 5) and nae.Context.dither_design().kind == 2
    for kw in (dict(bits=7), dict(kind="blue"), dict(shaping="third")):
        with pytest.raises(nae.NaeError):
            nae.dither_design(**kw)


def test_parameter_rules(ref):
    """the table of NAE_ERR_INVALID cases, through the statement's twin of nae_dither_check (the library's needs a context; the GPU test runs
    the same table through the block call and the create)"""
    ok = dither_ref.params(16, "triangular", "lipshitz")
    assert ref.ref_dither_check(C.byref(ok), 1) == 0 and ref.ref_dither_check(C.byref(ok), 2) == 0
    assert ref.ref_dither_check(None, 1) == INVALID and ref.ref_dither_check(C.byref(ok), 0) == INVALID and ref.ref_dither_check(C.byref(ok), 3) == INVALID
    for good in dither_ref.BOUNDARY_PARAMS:
        assert ref.ref_dither_check(C.byref(dither_ref.params(**good)), 2) == 0, good
    for bad in dither_ref.BAD_PARAMS:
        assert ref.ref_dither_check(C.byref(dither_ref.bad_params(bad)), 2) == INVALID, bad


def test_header_and_binding(nae):
    """the constants, the record's layout, the additions list, the debug key; the ABI version stays 3"""
    spec = open(os.path.join(dither_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    for name, value in (("MIN_BITS", "8"), ("MAX_BITS", "24"), ("MAX_TAPS", "12"), ("MAX_TAP_SUM", r"64\.0"), ("NONE", "0"), ("RECTANGULAR", "1"),
                        ("TRIANGULAR", "2"), ("HIGHPASS", "3"), ("SHAPE_NONE", "0"), ("SHAPE_FIRST", "1"), ("SHAPE_SECOND", "2"), ("SHAPE_LIPSHITZ", "3")):
        assert re.search(rf"#define\s+NAE_DITHER_{name}\s+{value}\s*$", spec, re.M), name
    assert (nae.DITHER_MIN_BITS, nae.DITHER_MAX_BITS, nae.DITHER_MAX_TAPS) == (dither_ref.MIN_BITS, dither_ref.MAX_BITS, dither_ref.MAX_TAPS)
    assert nae.DITHER_KINDS == dither_ref.KINDS and nae.DITHER_SHAPINGS == dither_ref.SHAPINGS
    assert C.sizeof(nae.DitherParams) == C.sizeof(dither_ref.Params) == 120
    for name, _ in dither_ref.Params._fields_:
        assert getattr(nae.DitherParams, name).offset == getattr(dither_ref.Params, name).offset, name
    header = open(os.path.join(dither_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_dither_params \{(.*?)\} nae_dither_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(unsigned long long|double|int)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("int", "bits"), ("int", "kind"), ("int", "n_taps"), ("double", "taps[12]"), ("unsigned long long", "seed")]
    additions = re.search(r"Later additions within 3(.*?)\*/", header, re.S).group(1)
    assert "nae_dither_design, nae_dither_block_f32 and the" in additions and "K23" in additions and "dither_roles" in header
    assert "#define NAE_ABI_VERSION 3" in header and nae.load_library().nae_abi_version() == 3
    assert all("nae_dither_" + s in nae.EXPORTED_SYMBOLS for s in ("design", "block_f32", "create", "put", "put_host", "flush", "available", "receive",
                                                                    "receive_host", "destroy"))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.dither_design()
    h = C.c_void_p()
    assert lib.nae_dither_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_dither_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_dither_put(None, None, 0) == INVALID and lib.nae_dither_put_host(None, None, 0) == INVALID
    assert lib.nae_dither_flush(None) == INVALID and lib.nae_dither_available(None) == 0
    assert lib.nae_dither_destroy(None) == 0


# ---------------------------------------------------------------------------------------------- the node
def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type, value or array length is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DITHER OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the fifteen existing calls keep their counts and give 21 entries without audio_dither, register_dither_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DITHER OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [21, 22]
    assert "audio_dither" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_dither"])


# ---------------------------------------------------------------------------------------------- the timing tool
def test_timing_tool_steps():
    """tools/dither_time.py as tests/test_time_tools_cpu.py holds the other tools: --help needs no device, and 'Steps: ...' in its docstring is
    what its driver runs, every step starting the tool in its child mode"""
    import importlib.util
    import sys
    tools = os.path.join(dither_ref.ROOT, "tools")
    env = dict(os.environ, NAE_GPU_LIB="/nonexistent/libnae_gpu.so", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(tools, "dither_time.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and all(flag in r.stdout for flag in ("--runs", "--warmup", "--quick", "--limit", "--shape")), r.stderr
    sys.path.insert(0, tools)
    try:
        spec = importlib.util.spec_from_file_location("dither_time", os.path.join(tools, "dither_time.py"))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        import nodetime
    finally:
        sys.path.remove(tools)
    full, quick = re.search(r"^Steps: (.+) \(--quick: (.+)\)\.", tool.__doc__, re.M).groups()
    for text, steps in ((full, tool.steps(False)), (quick, tool.steps(True))):
        assert [label for label, _ in steps] == text.split(", ")
        for label, tail in steps:
            assert tail == ["--shape", label] and label in nodetime.SHAPES
    assert len(tool.DRAWN) == 12 and abs(sum(abs(c) for c in tool.DRAWN) - 3.0) < 1e-12
