"""K20 multiband compressor, no GPU: the CPU statement (tests/mb_ref/ref_mb.c) against the composition of the equalizer's and the dynamics'
statements and a float64 sum; the library's host-side design nae_mb_design against its float64 restatement; what the specification promises
(bypass is the wire compressor, a solo is the band's own chain, the bands of a designed tree add to the all-pass cascade); K11's tiled form
against the plain recurrence in front of the bands' roundings; the rejections; the header; the multiband node's JSON and the thirteen
registration calls (tests/mb_ref/host_mb_node.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dyn_ref
import eq_ref
import mb_ref
import node_harness
from conftest import rel_rms

# K11's tiled form against the plain sequential recurrence on every band's path, both in double in front of the band's rounding, over the six
# designed trees of mb_ref.FLAT_CASES, unit noise and noise at -40 dB, at 3 * 1024 + 7 and at 300 * 1024 + 7 samples.  Measured, relative RMS per
# band: at most 3.53e-11 at 3 chunks and 3.06e-10 at 300 chunks, both in the bands of the 192 kHz tree with crossovers at 20 and 25 Hz, whose
# sections' poles lie 6.5e-4 from the unit circle; the trees at ordinary crossovers stay under 1e-12.  The bound is 30 times the worst case, the
# margin the long convolution's, the equalizer's, the dynamics' and the gate's bounds have over theirs.
SPLIT_RMS_BOUND = 30 * 3.06e-10
INVALID, UNSUPPORTED = -1, -2
CH = mb_ref.CHUNK


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return mb_ref.build(str(tmp_path_factory.mktemp("ref_mb")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("mb_ref/host_mb_node.cpp", str(tmp_path_factory.mktemp("host_mb")))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def wander(seed, n, ch, period=1500, level_db=-18.0):
    """noise whose level wanders +-14 dB around level_db, another phase per channel"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    ph = rng.uniform(0, 2 * np.pi, (1, ch))
    return (rng.uniform(-1, 1, (n, ch)) * 10.0 ** ((level_db + 14.0 * np.sin(2 * np.pi * t / period + ph)) / 20.0)).astype(np.float32)


def composition(ref, p, x):
    """eq_ref.run on every path's sections, dyn_ref.run on every band, the float64 sum in band order: what the specification says, from the two
    statements' own bindings"""
    n, ch = x.shape
    acc = None
    for b in range(p.n_bands):
        xb = eq_ref.run(ref, mb_ref.path_coef(p, b), x.reshape(-1), ch=ch).reshape(n, ch)
        yb = xb if p.bypass_mask >> b & 1 else dyn_ref.run(ref, p.band[b], xb)
        if not p.mute_mask >> b & 1:
            acc = yb.astype(np.float64) if acc is None else acc + yb.astype(np.float64)
    return np.zeros((n, ch), np.float32) if acc is None else acc.astype(np.float32)


@pytest.mark.parametrize("n_bands", (2, 3, 4))
@pytest.mark.parametrize("link", (0, 1))
def test_statement_is_the_composition_of_the_two_statements(ref, n_bands, link):
    for ch in (1, 2):
        for n in (1, 17, CH, 3 * CH + 7):
            x = wander(n_bands + n, n, ch)
            for la, mute, bypass in ((0, 0, 0), (17, 1, 2), (1024, 0, 1 << (n_bands - 1)), (300, (1 << n_bands) - 1, 0)):
                p = mb_ref.case(n_bands, la, link, mute, bypass)
                got, want = mb_ref.run(ref, p, x), composition(ref, p, x)
                assert np.array_equal(bits(got), bits(want)), (n_bands, link, ch, n, la, mute, bypass)
                if mute == (1 << n_bands) - 1:
                    assert not np.any(bits(got)), "every band muted: +0.0"
    xb = mb_ref.bands(ref, mb_ref.case(n_bands, 0, link), wander(1, 2 * CH + 7, 2))
    for b in range(n_bands):
        for c in range(b):
            assert not np.array_equal(xb[b], xb[c]), "the bands differ"


@pytest.mark.parametrize("rate,crossovers", mb_ref.FLAT_CASES)
def test_design_against_float64_restatement(nae, ref, rate, crossovers):
    """nae_mb_design's sections within 1 ulp of the restatement, slot by slot; the statement's design is the library's; every section stable
    under K11's rule; the band records and the masks are passed through"""
    n_bands = len(crossovers) + 1
    bands = [nae.Context.dyn_design(rate, -30.0 + b, 2.0 + b, 3.0 * b, 0.001 * (b + 1), 0.05 * (b + 1), 0.002, 1.0 * b, False) for b in range(n_bands)]
    got = nae.Context.mb_design(rate, crossovers, bands, 1, 2)
    want = mb_ref.design64(rate, crossovers)
    g = np.array([[got.coef[s][i] for i in range(5)] for s in range(got.n_sections)], np.float64)
    ulps = int(np.abs(g.view(np.int64) - want.view(np.int64)).max())
    print(f"{rate} Hz {crossovers}: {got.n_sections} sections, worst {ulps} ulp of double against the float64 restatement")
    assert (got.n_bands, got.n_sections) == (n_bands, mb_ref.SECTIONS[n_bands]) and want.shape == g.shape
    assert ulps <= 1
    assert eq_ref.stable(g) and eq_ref.stable(want)
    assert (got.mute_mask, got.bypass_mask) == (1, 2)
    for b in range(n_bands):
        assert dyn_ref.as_tuple(got.band[b]) == dyn_ref.as_tuple(bands[b])
    stated = mb_ref.design(ref, rate, crossovers, [dyn_ref.Params(*dyn_ref.as_tuple(b)) for b in bands], 1, 2)
    assert stated is not None and bytes(stated) == bytes(got), "the statement's design is the library's"
    assert ref.ref_mb_check(C.byref(stated), 2) == 0
    for kind, i in set(mb_ref.SLOTS[n_bands]):
        slots = [s for s, slot in enumerate(mb_ref.SLOTS[n_bands]) if slot == (kind, i)]
        assert all(np.array_equal(g[s], g[slots[0]]) for s in slots), "the two halves of a Linkwitz-Riley filter are one section twice"
    assert C.sizeof(nae.MbParams) == C.sizeof(mb_ref.Params)


def test_design_rejections(nae):
    lib = nae.load_library()
    out = nae.MbParams()
    bands = (nae.DynParams * 4)(*[nae.Context.dyn_design(48000) for _ in range(4)])

    def des(rate=48000, n_bands=3, xs=(120.0, 2500.0, 9000.0), bands_p=C.addressof(bands), mute=0, bypass=0, p=C.byref(out)):
        a = np.ascontiguousarray(xs, np.float64)
        return lib.nae_mb_design(rate, n_bands, a.ctypes.data if xs is not None else None, bands_p, mute, bypass, p)

    nan, inf = float("nan"), float("inf")
    assert des() == 0 and (out.n_bands, out.n_sections) == (3, 9) and des(n_bands=2) == 0 and out.n_sections == 4 and des(n_bands=4) == 0 and out.n_sections == 14
    assert des(n_bands=1) == INVALID and des(n_bands=5) == INVALID and des(n_bands=0) == INVALID
    assert des(rate=0) == INVALID and des(rate=-48000) == INVALID
    assert des(xs=None) == INVALID and des(bands_p=None) == INVALID and des(p=None) == INVALID
    for xs in ((2500.0, 120.0), (120.0, 120.0), (0.0, 120.0), (-5.0, 120.0), (120.0, 24000.0), (120.0, 30000.0), (nan, 120.0), (120.0, inf)):
        assert des(xs=xs) == INVALID, xs
    assert des(xs=(120.0, 23999.0)) == 0
    assert des(mute=8) == INVALID and des(bypass=8) == INVALID and des(mute=7, bypass=7) == 0 and des(n_bands=4, mute=8) == 0
    bad = (nae.DynParams * 4)(*bands)
    bad[2].lookahead = 5
    assert des(bands_p=C.addressof(bad)) == INVALID and des(n_bands=2, bands_p=C.addressof(bad)) == 0, "unequal look-ahead, in a band that counts"
    bad[2].lookahead, bad[1].link = 0, 0
    assert des(bands_p=C.addressof(bad)) == INVALID, "unequal link"
    bad[1].link, bad[0].slope = 1, 1.5
    assert des(bands_p=C.addressof(bad)) == INVALID, "a band record nae_dyn_check refuses"
    with pytest.raises(nae.NaeError):
        nae.Context.mb_design(48000, (2500.0, 120.0), list(bands)[:3])
    with pytest.raises(nae.NaeError):
        nae.Context.mb_design(48000, (120.0,), list(bands)[:3])


@pytest.mark.parametrize("n_bands", (2, 3, 4))
def test_bypass_is_the_wire_compressor_and_a_solo_is_the_bands_chain(ref, n_bands):
    x = wander(5, 2 * CH + 7, 2)
    base = mb_ref.case(n_bands, 17, 1)
    wire = dyn_ref.params(slope=0.0, makeup_db=0.0, lookahead=17, link=1)
    for b in range(n_bands):
        bands = mb_ref.bands_of(base)
        bands[b] = wire
        assert np.array_equal(bits(mb_ref.run(ref, mb_ref.with_masks(base, bypass_mask=1 << b), x)), bits(mb_ref.run(ref, mb_ref.with_masks(base, bands=bands), x))), b
        solo = ((1 << n_bands) - 1) & ~(1 << b)
        xb = eq_ref.run(ref, mb_ref.path_coef(base, b), x.reshape(-1), ch=2).reshape(x.shape)
        assert np.array_equal(bits(mb_ref.run(ref, mb_ref.with_masks(base, mute_mask=solo), x)), bits(dyn_ref.run(ref, base.band[b], xb))), b
        assert np.array_equal(bits(mb_ref.run(ref, mb_ref.with_masks(base, mute_mask=solo, bypass_mask=1 << b), x)), bits(xb)), b
        assert np.array_equal(bits(mb_ref.bands(ref, base, x)[b]), bits(xb))


@pytest.mark.parametrize("rate,crossovers", mb_ref.FLAT_CASES)
def test_flat_sum(ref, rate, crossovers):
    """Every band bypassed: the output is the float64 all-pass cascade AP(f1) ... AP(f_(B-1)) of the input within (B + 1) 2^-24 P + 1e-9: B band
    roundings and one final rounding, each at most half an f32 step of a value no larger than P, the largest magnitude among the float64 band
    signals and their sum, which the restatement computes from the input alone.  Measured: 0.96e-7 ... 1.24e-7 against bounds of 2.5e-7 ... 5.9e-7.
    The magnitude of the sum of the bands' transfer functions is within 8.6e-10 of 1 from 10 Hz to Nyquist (1.6e-12 at the ordinary crossovers)"""
    n_bands = len(crossovers) + 1
    x = np.random.default_rng(0).uniform(-1, 1, 3 * CH + 7).astype(np.float32)
    coef = mb_ref.design64(rate, crossovers)
    assert eq_ref.stable(coef)
    p = mb_ref.params(coef, mb_ref.band_set(n_bands), 0, (1 << n_bands) - 1)
    y = mb_ref.run(ref, p, x[:, None])[:, 0].astype(np.float64)
    w = mb_ref.bands64(coef, n_bands, x)
    want = mb_ref.biquads64(np.stack([mb_ref.allpass(rate, f) for f in crossovers]), x)
    P = max(float(np.abs(w).max()), float(np.abs(w.sum(0)).max()))
    bound = (n_bands + 1) * 2.0 ** -24 * P + 1e-9
    err = float(np.abs(y - want).max())
    flat = float(np.abs(mb_ref.magnitude_of_sum(coef, n_bands, np.geomspace(10.0, rate / 2.0, 4000), rate) - 1.0).max())
    print(f"{rate} Hz {crossovers}: |y - allpass(x)| {err:.3g} (bound {bound:.3g}, P {P:.4g}); the float64 bands' sum off by {np.abs(w.sum(0) - want).max():.3g}; "
          f"| |sum H_b| - 1 | {flat:.3g}")
    assert err <= bound
    assert flat <= 1e-8, "the designed tree's bands add to an all-pass"


@pytest.mark.parametrize("n", (3 * CH + 7, 300 * CH + 7))
def test_tiled_split_against_the_sequential_form(ref, n):
    worst = 0.0
    for rate, crossovers in mb_ref.FLAT_CASES:
        n_bands = len(crossovers) + 1
        p = mb_ref.params(mb_ref.design64(rate, crossovers), mb_ref.band_set(n_bands))
        for seed, scale in ((1, 1.0), (2, 0.01)):
            x = (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)
            tiled, seq = mb_ref.split_f64(ref, p, x, True), mb_ref.split_f64(ref, p, x, False)
            errs = [rel_rms(tiled[b], seq[b]) for b in range(n_bands)]
            print(f"n {n} {rate} Hz {crossovers} scale {scale}: rel RMS per band " + " ".join(f"{e:.3g}" for e in errs))
            worst = max(worst, max(errs))
            assert max(errs) <= SPLIT_RMS_BOUND, (rate, crossovers, scale, errs)
            assert np.array_equal(bits(mb_ref.bands(ref, p, x[:, None])[:, :, 0]), bits(tiled.astype(np.float32))), "a band is the tiled path rounded once"
    print(f"n {n}: worst {worst:.3g} (bound {SPLIT_RMS_BOUND:.3g})")


def test_statement_rejects_what_the_library_rejects(ref):
    good = mb_ref.case(3)
    coef, bands = mb_ref.coef_of(good), mb_ref.bands_of(good)

    def check(p, ch=2):
        return ref.ref_mb_check(C.byref(p) if p is not None else None, ch)

    assert check(good) == 0 and check(good, 1) == 0 and check(mb_ref.case(2)) == 0 and check(mb_ref.case(4, 1024, 0, 15, 15)) == 0
    assert check(None) == INVALID, "a null pointer"
    assert check(good, 0) == INVALID and check(good, 3) == INVALID, "ch not 1 or 2"
    assert check(mb_ref.params(coef, bands, n_bands=1)) == INVALID and check(mb_ref.params(coef, bands, n_bands=-2)) == INVALID, "B < 2"
    assert check(mb_ref.params(coef, bands, n_bands=5)) == UNSUPPORTED, "B > 4"
    for n_sections in (0, 4, 8, 10, 14):
        assert check(mb_ref.params(coef, bands, n_sections=n_sections)) == INVALID, "n_sections not the tree's count"
    assert check(mb_ref.params(mb_ref.coef_of(mb_ref.case(2)), bands, n_sections=4)) == INVALID
    for s in (0, 4, 8):
        for bad in eq_ref.BAD_SECTIONS:
            c = coef.copy()
            c[s] = bad
            assert check(mb_ref.params(c, bands)) == INVALID, ("a non-finite or not strictly stable section", s, bad)
    c = coef.copy()
    c[8] = eq_ref.GOOD_SECTIONS[-1]
    assert check(mb_ref.params(c, bands)) == 0, "any checked section in a slot"
    for b in range(3):
        for field, v in (("threshold_db", 0.5), ("threshold_db", float("nan")), ("slope", -0.1), ("knee_db", 24.5), ("alpha_attack", 1.0), ("alpha_release", -0.1),
                         ("makeup_db", 24.5), ("lookahead", -1), ("link", 2)):
            bb = [dyn_ref.Params(*dyn_ref.as_tuple(x)) for x in bands]
            setattr(bb[b], field, v)
            assert check(mb_ref.params(coef, bb)) == INVALID, ("a band failing the dynamics' check", b, field, v)
    for b in (1, 2):
        bb = [dyn_ref.Params(*dyn_ref.as_tuple(x)) for x in bands]
        bb[b].lookahead = 7
        assert check(mb_ref.params(coef, bb)) == INVALID, "unequal look-ahead"
        bb[b].lookahead, bb[b].link = 0, 0
        assert check(mb_ref.params(coef, bb)) == INVALID, "unequal link"
    for mask in (8, 16, 1 << 31):
        assert check(mb_ref.params(coef, bands, mute_mask=mask)) == INVALID and check(mb_ref.params(coef, bands, bypass_mask=mask)) == INVALID, "mask bits at or above B"
    assert check(mb_ref.case(3, 1025)) == UNSUPPORTED, "a look-ahead above 1024"
    assert check(mb_ref.case(3, 1024)) == 0


def test_header_and_binding(nae, ref):
    """the constants, the record's layout, the paths of the tree, the additions list, the debug keys, the ABI version stays 3"""
    spec = open(os.path.join(mb_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_MB_MAX_BANDS\s+4\s*$", spec, re.M) and re.search(r"#define\s+NAE_MB_MAX_SECTIONS\s+14\s*$", spec, re.M)
    assert (nae.MB_MAX_BANDS, nae.MB_MAX_SECTIONS) == (mb_ref.MAX_BANDS, mb_ref.MAX_SECTIONS) == (4, 14)
    assert C.sizeof(nae.MbParams) == C.sizeof(mb_ref.Params) == 8 + 14 * 40 + 4 * 56 + 8
    for name, _ in mb_ref.Params._fields_:
        assert getattr(nae.MbParams, name).offset == getattr(mb_ref.Params, name).offset, name
    header = open(os.path.join(mb_ref.ROOT, "include", "nae_gpu.h")).read()
    record = re.search(r"typedef struct nae_mb_params \{(.*?)\} nae_mb_params;", header, re.S).group(1)
    fields = re.findall(r"^\s*(unsigned|double|int|nae_dyn_params)\s+([^;]+);", record, re.M)
    assert [(t, n.replace(" ", "")) for t, n in fields] == [("int", "n_bands"), ("int", "n_sections"), ("double", "coef[NAE_MB_MAX_SECTIONS][5]"),
                                                            ("nae_dyn_params", "band[NAE_MB_MAX_BANDS]"), ("unsigned", "mute_mask,bypass_mask")]
    additions = re.search(r"Later additions within 3(.*?)\*/", header, re.S).group(1)
    assert "nae_mb_design, nae_mb_block_f32 and the nae_mb handle" in additions and "K20" in additions
    assert re.search(r"^ \*   mb_group\s", header, re.M) and re.search(r"^ \*   mb_slab\s", header, re.M)
    assert "#define NAE_ABI_VERSION 3" in header and nae.load_library().nae_abi_version() == 3
    assert all("nae_mb_" + s in nae.EXPORTED_SYMBOLS for s in ("design", "block_f32", "create", "put", "put_host", "flush", "available", "receive",
                                                                "receive_host", "destroy"))
    # every slot stands on a path, and the statement's tree is the one the tests compose
    for n_bands, paths in mb_ref.PATHS.items():
        assert sorted(set(s for path in paths for s in path)) == list(range(mb_ref.SECTIONS[n_bands])) == list(range(len(mb_ref.SLOTS[n_bands])))
        for b, path in enumerate(paths):
            slots = (C.c_int * 5)()
            assert tuple(slots[:ref.ref_mb_path(n_bands, b, slots)]) == path, (n_bands, b)


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = mb_ref.lib_params(nae, mb_ref.case(3))
    h = C.c_void_p()
    assert lib.nae_mb_block_f32(None, C.byref(p), None, 0, 1, 0, None) == INVALID
    assert lib.nae_mb_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_mb_put(None, None, 0) == INVALID and lib.nae_mb_put_host(None, None, 0) == INVALID
    assert lib.nae_mb_flush(None) == INVALID and lib.nae_mb_available(None) == 0
    assert lib.nae_mb_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type, value or array length is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MB OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the twelve existing calls keep their counts and give 18 entries without audio_multiband, register_multiband_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MB OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [18, 19]
    assert "audio_multiband" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_multiband"])
