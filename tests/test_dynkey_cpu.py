"""K15 keyed dynamics, no GPU: the CPU statement (tests/dynkey_ref/ref_dynkey.c) — the three identities that tie it to the statements of the
dynamics processor and of the equalizer, bit for bit; the tiled form against the plain sequential recurrences; what a side-chain is for, a
ducker and a de-esser, against the static curve; the statement's and the library's rejections without a context; the side-chain node's
JSON and the eight registration calls (tests/dynkey_ref/host_dynkey_node.cpp)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import dyn_ref
import dynkey_ref
import eq_ref
import node_harness
from conftest import rel_rms

# The tiled statement against the sequential recurrences, both in double, in front of the final rounding, over the cases of
# test_statement_against_sequential_recurrence, measured here by section count: 0 ... 3.1e-15 with no section, 0 ... 2.6e-15 with one,
# 0 ... 5.0e-11 with the four slow ones (one cell: fast, look-ahead 0; every other at most 3.9e-15).  The last is not K12's figure (2.6e-14):
# the tiled and the sequential filter differ in the last places of w, so now and then m = (float)|w| falls on the other side of a rounding
# boundary, one f32 ulp of the level, and the gain follows it.  Each bound is 30 times its section count's worst case, the margin
# tests/test_dyn_cpu.py gives K12.
RMS_BOUND = {0: 30 * 3.1e-15, 1: 30 * 2.6e-15, 4: 30 * 5.0e-11}
INVALID, UNSUPPORTED = -1, -2
FILTERS = dynkey_ref.key_filters()
N = 3 * dyn_ref.CHUNK + 7


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dynkey_ref.build(str(tmp_path_factory.mktemp("ref_dynkey")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dynkey_ref/host_dynkey_node.cpp", str(tmp_path_factory.mktemp("host_dynkey")))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("la", (0, 17, 1024))
def test_no_section_is_the_dynamics_processor(ref, la):
    """an internal key with no section, and an external key equal to the signal, are K12's statement bit for bit"""
    for sig, x in dyn_ref.signals(N).items():
        for ch in (1, 2):
            for link in (0, 1):
                xs = np.ascontiguousarray(x[:, :ch])
                dp = dyn_ref.params(lookahead=la, link=link, **dyn_ref.SLOW)
                want = dyn_ref.run(ref, dp, xs)
                assert same_bits(dynkey_ref.run(ref, dynkey_ref.params(dp, 0), xs), want), (sig, ch, link, "internal")
                assert same_bits(dynkey_ref.run(ref, dynkey_ref.params(dp, ch), xs, xs), want), (sig, ch, link, "self")


@pytest.mark.parametrize("sections", (1, 4))
def test_filtered_key_is_the_equalizer_in_front_of_the_key(ref, sections):
    """a key filtered by n sections gives the bits of the call with no section keyed by the equalizer's f32 output: (float)|w| = |(float)w|"""
    rng = np.random.default_rng(sections)
    x = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    for sig, key in dyn_ref.signals(N).items():
        for ch, key_ch, link in ((1, 1, 0), (2, 1, 1), (2, 2, 1), (2, 2, 0), (2, 1, 0)):
            xs, ks = np.ascontiguousarray(x[:, :ch]), np.ascontiguousarray(key[:, :key_ch])
            dp = dyn_ref.params(lookahead=17, link=link)
            got = dynkey_ref.run(ref, dynkey_ref.params(dp, key_ch, FILTERS[sections]), xs, ks)
            filtered = dynkey_ref.eq_f32(ref, FILTERS[sections], ks)
            assert same_bits(got, dynkey_ref.run(ref, dynkey_ref.params(dp, key_ch), xs, filtered)), (sig, ch, key_ch, link)
            assert same_bits(dynkey_ref.magnitude(ref, dynkey_ref.params(dp, key_ch, FILTERS[sections]), xs, ks), np.abs(filtered))
        # the internal key: the signal through the equalizer keys itself
        dp = dyn_ref.params(lookahead=17, link=1)
        got = dynkey_ref.run(ref, dynkey_ref.params(dp, 0, FILTERS[sections]), key)
        assert same_bits(got, dynkey_ref.run(ref, dynkey_ref.params(dp, 2), key, dynkey_ref.eq_f32(ref, FILTERS[sections], key))), sig


def test_detectors_follow_the_link_and_the_key_channels(ref):
    """linked: one detector on the larger m; unlinked: detector c on key channel c, or on channel 0 of a mono key"""
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (1500, 2)).astype(np.float32)
    key = dyn_ref.signals(1500)["bursts"]
    key[:, 1] *= 0.25
    dp = dyn_ref.params(lookahead=9, link=0)
    y = dynkey_ref.run(ref, dynkey_ref.params(dp, 2, FILTERS[1]), x, key)
    for c in range(2):
        one = dynkey_ref.run(ref, dynkey_ref.params(dp, 1, FILTERS[1]), np.ascontiguousarray(x[:, c:c + 1]), np.ascontiguousarray(key[:, c:c + 1]))
        assert same_bits(y[:, c], one[:, 0]), c
    mono = dynkey_ref.run(ref, dynkey_ref.params(dp, 1), x, np.ascontiguousarray(key[:, :1]))
    assert same_bits(mono, dynkey_ref.run(ref, dynkey_ref.params(dp, 2), x, np.repeat(key[:, :1], 2, 1)))
    dp.link = 1
    larger = np.max(np.abs(key), axis=1, keepdims=True).astype(np.float32)
    assert same_bits(dynkey_ref.run(ref, dynkey_ref.params(dp, 2), x, key), dynkey_ref.run(ref, dynkey_ref.params(dp, 1), x, larger))


@pytest.mark.parametrize("speed", ("fast", "slow"))
@pytest.mark.parametrize("la", (0, 17, 1024))
def test_statement_against_sequential_recurrence(ref, la, speed):
    x = np.random.default_rng(3).uniform(-1, 1, (N, 2)).astype(np.float32)
    worst = {}
    for sections in (0, 1, 4):
        for sig, key in dyn_ref.signals(N).items():
            for link in (0, 1):
                for key_ch in (0, 1, 2):
                    p = dynkey_ref.params(dyn_ref.params(lookahead=la, link=link, **(dyn_ref.FAST if speed == "fast" else dyn_ref.SLOW)), key_ch,
                                          FILTERS[sections])
                    xs, ks = (key, None) if key_ch == 0 else (x, np.ascontiguousarray(key[:, :key_ch]))
                    seq, tiled = dynkey_ref.sequential(ref, p, xs, ks), dynkey_ref.run_f64(ref, p, xs, ks)
                    err = rel_rms(tiled, seq)
                    worst[sections] = max(worst.get(sections, 0.0), err)
                    assert err <= RMS_BOUND[sections], (sections, sig, link, key_ch, err)
                    assert np.array_equal(dynkey_ref.run(ref, p, xs, ks), tiled.astype(np.float32)), "rounded once, at the end"
    print(f"{speed} la {la}: worst rel RMS in double by section count {worst}, bounds {RMS_BOUND}")


def test_ducking(ref):
    """the key is a burst train, the signal a steady tone: inside the bursts the tone falls by the static curve's demand of the key's level
    (the tolerance of test_dyn_cpu.py's test_constant_input_reaches_the_static_curve: 1e-9 of the gain), outside them, after the release, it
    is untouched"""
    n, period, on = 24000, 6000, 3000
    t = np.arange(n)
    tone = (0.4 * np.sin(2 * np.pi * 440.0 * t / 48000.0)).astype(np.float32)[:, None]
    for level_db, ratio in ((-6.0, 4.0), (-15.5, 2.0), (-1.0, math.inf)):
        A = np.float32(10.0 ** (level_db / 20.0))
        key = (np.where(t % period < on, A, 0.0) * np.where(t % 2, -1.0, 1.0)).astype(np.float32)[:, None]   # a voice at a constant level
        dp = dyn_ref.params(threshold_db=-20.0, slope=1.0 if math.isinf(ratio) else 1.0 - 1.0 / ratio, knee_db=8.0,
                            alpha_attack=dyn_ref.alpha(0.0005), alpha_release=dyn_ref.alpha(0.001), makeup_db=0.0, lookahead=3)
        y = dynkey_ref.sequential(ref, dynkey_ref.params(dp, 1), tone, key)
        want = 10.0 ** (-dyn_ref.demand_db(dp, 20.0 * math.log10(float(A))) / 20.0)
        assert want < 0.8, "the case ducks"
        loud = np.abs(tone[:, 0]) > 0.05
        gain = y[loud, 0] / tone[loud, 0].astype(np.float64)
        pos = t[loud] % period
        inside, outside = (pos >= 1000) & (pos < on - 3), (pos >= on + 1500) & (pos < period - 3)   # the look-ahead sees the next burst 3 early
        assert inside.sum() > 1000 and outside.sum() > 1000
        assert np.max(np.abs(gain[inside] / want - 1.0)) <= 1e-9, (level_db, ratio)
        assert np.max(np.abs(gain[outside] - 1.0)) <= 1e-9, (level_db, ratio)
        # and the tiled form, rounded: the tone itself outside the bursts
        y32 = dynkey_ref.run(ref, dynkey_ref.params(dp, 1), tone, key)
        quiet = (t % period >= on + 1500) & (t % period < period - 3)
        assert np.array_equal(y32[quiet], tone[quiet])


def test_de_esser(ref):
    """a 200 Hz tone with gated 8 kHz bursts keys itself through a band-pass around 8 kHz: the reduction happens during the bursts only;
    without the filter the tone holds the compressor down throughout.  The design has no band-pass kind (nae_eq_design: peak, shelves,
    low-pass, high-pass, notch), so the band is two of the key filter's four sections, a high-pass at 6 kHz and a low-pass at 10 kHz"""
    n, period, on = 24000, 6000, 2000
    t = np.arange(n)
    ess = np.where(t % period < on, 0.3, 0.0) * np.sin(2 * np.pi * 8000.0 * t / 48000.0)
    x = (0.5 * np.sin(2 * np.pi * 200.0 * t / 48000.0) + ess).astype(np.float32)[:, None]
    band = np.stack([eq_ref.design("highpass", 48000, 6000.0, 0.0, 0.7071), eq_ref.design("lowpass", 48000, 10000.0, 0.0, 0.7071)])
    assert eq_ref.magnitude_db(band, 8000.0, 48000) > -4.0 and eq_ref.magnitude_db(band, 200.0, 48000) < -50.0
    dp = dyn_ref.params(threshold_db=-30.0, slope=0.75, knee_db=6.0, alpha_attack=dyn_ref.alpha(0.0005), alpha_release=dyn_ref.alpha(0.001),
                        makeup_db=0.0, lookahead=0)
    loud = np.abs(x[:, 0]) > 0.05
    pos = t[loud] % period

    def gain(p):
        return dynkey_ref.sequential(ref, p, x)[loud, 0] / x[loud, 0].astype(np.float64)

    g = gain(dynkey_ref.params(dp, 0, band))
    during, between = (pos >= 300) & (pos < on), pos >= on + 1500
    assert np.max(g[during]) < 0.6, "the bursts are turned down"
    assert np.max(np.abs(g[between] - 1.0)) <= 1e-9, "the tone alone is left as it is"
    assert np.max(gain(dynkey_ref.params(dp, 0))[between]) < 0.6, "without the key filter the tone itself is compressed"


def test_statement_rejects_what_the_library_rejects(ref):
    hp = FILTERS[1]

    def check(p, ch=2):
        return ref.ref_dynkey_check(C.byref(p), ch)

    assert check(dynkey_ref.params(dyn_ref.params(), 0)) == 0 and check(dynkey_ref.params(dyn_ref.params(), 2, FILTERS[4])) == 0
    assert check(dynkey_ref.params(dyn_ref.params(), 1, hp), 1) == 0
    assert check(dynkey_ref.params(dyn_ref.params(lookahead=1025), 1, hp)) == UNSUPPORTED
    assert check(dynkey_ref.params(dyn_ref.params(slope=1.5), 1, hp)) == INVALID
    assert check(dynkey_ref.params(dyn_ref.params(), 2, hp), 1) == INVALID and check(dynkey_ref.params(dyn_ref.params(), 3, hp)) == INVALID
    assert check(dynkey_ref.params(dyn_ref.params(), -1, hp)) == INVALID
    assert check(dynkey_ref.params(dyn_ref.params(), 1, hp, n_sections=-1)) == INVALID
    assert check(dynkey_ref.params(dyn_ref.params(), 1, np.repeat(hp, 4, 0), n_sections=5)) == UNSUPPORTED
    for section in eq_ref.BAD_SECTIONS:
        assert check(dynkey_ref.params(dyn_ref.params(), 1, np.array([hp[0], section], np.float64))) == INVALID, section
    for section in eq_ref.GOOD_SECTIONS:
        assert check(dynkey_ref.params(dyn_ref.params(), 1, np.array([hp[0], section], np.float64))) == 0, section


def test_record_and_limits_agree_with_the_header(nae):
    """the binding's record has the statement's layout, and NAE_DYNKEY_MAX_SECTIONS is 4 in include/nae_dsp_spec.h"""
    import os
    import re
    spec = open(os.path.join(dynkey_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_DYNKEY_MAX_SECTIONS\s+4\b", spec) and nae.DYNKEY_MAX_SECTIONS == dynkey_ref.MAX_SECTIONS == 4
    assert C.sizeof(nae.DynKeyParams) == C.sizeof(dynkey_ref.Params)
    for name in ("dyn", "key_ch", "n_sections", "coef"):
        assert getattr(nae.DynKeyParams, name).offset == getattr(dynkey_ref.Params, name).offset, name
    with pytest.raises(nae.NaeError):
        nae.DynKeyParams.make(nae.DynParams(), 1, np.zeros((5, 5)))


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.DynKeyParams.make(nae.DynParams(*dyn_ref.as_tuple(dyn_ref.params())), 1, FILTERS[1])
    h = C.c_void_p()
    assert lib.nae_dynkey_block_f32(None, C.byref(p), None, None, 0, 1, 0, None) == INVALID
    assert lib.nae_dynkey_create(None, C.byref(p), 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_dynkey_put(None, None, 0) == INVALID and lib.nae_dynkey_put_host(None, None, 0) == INVALID
    assert lib.nae_dynkey_flush(None) == INVALID and lib.nae_dynkey_available(None) == 0
    got = C.c_size_t()
    assert lib.nae_dynkey_receive(None, None, 0, C.byref(got)) == INVALID and lib.nae_dynkey_receive_host(None, None, 0, C.byref(got)) == INVALID
    assert lib.nae_dynkey_destroy(None) == 0


def test_host_node_json_keys(host):
    """the node's JSON: audio_dynamics' nine keys and "key_filter" of 0 ... 4 bands round-trip, the defaults are not written back, a wrong
    type or value is the error "Wrong field: <key>" with that key"""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYNKEY OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the seven existing calls give 13 entries without audio_sidechain, register_sidechain_processors() adds it: three pins, two audio inputs"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYNKEY OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [13, 14]
    assert "audio_sidechain" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_sidechain"])
