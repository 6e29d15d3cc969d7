"""K7 at vocoder frame sizes 512 ... 4096, no GPU: the CPU statement (tests/pv_ref/ref_pv.c) pinned to the oracle at N = 1024 and to
the float64 numpy restatement (tests/pv_sizes_numpy.py) at the other sizes, the plan of every size through the library, what a size changes
on clicks and on close low partials, and the C ABI's declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_ref
import pv_sizes_numpy
from conftest import rel_rms
from pv_gpu import tone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5), (0.5, 2.0)]   # those of tests/test_gpu_pv_lock.py
SYMBOLS = ("nae_stretch_plan_make_n", "nae_stretch_block_n_f32", "nae_debug_pv_tile_phase_n", "nae_stretch_create_n")
UNSUPPORTED = -2   # NAE_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", PAIRS)
def test_restatement_at_1024_is_the_oracle(ref, rate, pitch, ch):
    """N = 1024: samples and every frame's Qs equal orc.stretch / orc.pv_synth_phase bit for bit, on noise and on tones"""
    L = 20000
    m = tone(L)
    for x in (orc.fill_uniform(L * ch, 3), np.stack([m, 0.5 * m], 1).reshape(-1) if ch == 2 else m):
        a, b = pv_ref.stretch(ref, x, ch, rate, pitch, 1024), orc.stretch(x, ch, rate, pitch)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(pv_ref.synth_phase(ref, x, ch, rate, pitch, 1024), orc.pv_synth_phase(x, ch, rate, pitch))


@pytest.mark.parametrize("n_fft", [512, 2048, 4096])
@pytest.mark.parametrize("rate,pitch", [(0.5, 2.0), (0.8, 2.0), (0.3, 2.0)])
def test_restatement_matches_the_numpy_specification(ref, n_fft, rate, pitch):
    """512 / 2048 / 4096 on a two-tone signal, vocoder alone and with the transposer after (rho < 1) and before it (rho > 1): within 1e-5
    relative RMS of the float64 restatement (measured 2.4e-7 - 3.6e-7 at tempo 1/2).  The tempo is 1/2 for a reason: at a tempo of 1 or more a
    Hann main-lobe bin 1-2 bins away from a partial advances by about half a turn or more per analysis hop, so float32 against float64
    rounding decides its phase wrap, and the two restatements differ by 1e-3 at every size, 1024 included."""
    x = tone(24000)
    got = pv_ref.stretch(ref, x, 1, rate, pitch, n_fft)
    want = pv_sizes_numpy.stretch(x, 1, rate, pitch, n_fft)
    assert got.size == want.size
    assert rel_rms(got, want) <= 1e-5, rel_rms(got, want)


def lib_plan(nae, rate, pitch, n_fft, L):
    pl = nae.StretchPlan()
    rc = nae.load_library().nae_stretch_plan_make_n(rate, pitch, n_fft, L, C.byref(pl))
    return rc, pl


FIELDS = ("pv_on", "rs_on", "tempo_eff", "rate_eff", "ha_q24", "d0", "step_q32", "out_len", "mid_len", "frames", "rs_first")


@pytest.mark.parametrize("rate,pitch", PAIRS + [(1.3, 1 / 1.1), (1.0, 1.0), (2.0, 1.0)])
def test_plan_of_every_size(nae, ref, rate, pitch):
    """_n at 1024 is nae_stretch_plan_make field for field; at every size the frame count and the hop follow N (the restatement's plan,
    which is the oracle's with H = N/4), and the size-independent fields do not move"""
    L = 48000
    base = nae.StretchPlan()
    assert nae.load_library().nae_stretch_plan_make(rate, pitch, L, C.byref(base)) == 0
    for n_fft in (512, 1024, 2048, 4096):
        rc, pl = lib_plan(nae, rate, pitch, n_fft, L)
        assert rc == 0
        rc2, want = pv_ref.plan(ref, rate, pitch, n_fft, L)
        assert rc2 == 0
        for f in FIELDS:
            assert getattr(pl, f) == getattr(want, f), (n_fft, f)
        assert list(pl.r_q24) == list(want.r_q24)
        H = n_fft // 4
        pv_out = pl.out_len if pl.rs_first else pl.mid_len
        assert pl.frames == ((pv_out + n_fft // 2 + H - 1) // H + 1 if pl.pv_on else 0)
        for f in ("pv_on", "rs_on", "out_len", "mid_len", "rs_first", "step_q32"):
            assert getattr(pl, f) == getattr(base, f), (n_fft, f)
        if n_fft == 1024:
            for f in FIELDS:
                assert getattr(pl, f) == getattr(base, f), f
            assert list(pl.r_q24) == list(base.r_q24)


def test_plan_ratio_at_the_tempo_limits(nae):
    """R = round(2^24 H / d) ~ 2^24 / tempo depends on the tempo only: a positive int32 at every size and at both tempo limits (1/64 and 16,
    NAE_TEMPO_MIN / NAE_TEMPO_MAX; tests/test_stretch_range_cpu.py checks one step outside them)"""
    import struct
    for tempo, rate in [(t, 1.0 / t) for t in (0.25, 0.2500001, 3.999, 4.0)] + [(1 / 64, 1 / 64), (16.0, 16.0)]:
        for n_fft in (512, 1024, 2048, 4096):
            rc, pl = lib_plan(nae, rate, 1.0 / tempo, n_fft, 10000)
            assert rc == 0, (tempo, n_fft, rc)
            assert pl.pv_on
            for r in pl.r_q24:
                assert 0 < r <= 2 ** 30 and struct.unpack("i", struct.pack("I", r))[0] > 0
            assert abs(pl.r_q24[0] / 2 ** 24 * tempo - 1) < 0.01


@pytest.mark.parametrize("n_fft", [256, 8192, 1000, 0, -1024])
def test_plan_refuses_other_sizes(nae, n_fft):
    rc, _ = lib_plan(nae, 1.0, 1.2, n_fft, 1000)
    assert rc == UNSUPPORTED


def click_width(ref, n_fft):
    """median RMS width (samples) of the energy of each output click; a click every 9600 samples, velocity 1.5 with keep_pitch"""
    L = 96000
    x = np.zeros(L, np.float32)
    pos = np.arange(4800, L - 4800, 9600)
    x[pos] = 1.0
    y = pv_ref.stretch(ref, x, 1, 1.5, 1 / 1.5, n_fft).astype(np.float64)
    widths = []
    for p in pos:
        c = int(round(p / 1.5))
        e = y[c - 3000:c + 3000] ** 2
        t = np.arange(e.size)
        m = (e * t).sum() / e.sum()
        widths.append(np.sqrt((e * (t - m) ** 2).sum() / e.sum()))
    return float(np.median(widths))


def test_clicks_spread_with_the_frame(ref):
    """a click train at velocity 1.5 (keep_pitch): the energy of each output click spreads over a width that grows with N — measured
    75 / 208 / 327 / 709 samples RMS at 512 / 1024 / 2048 / 4096.  Drums want the short frame."""
    w = [click_width(ref, n) for n in (512, 1024, 2048, 4096)]
    assert all(a < b for a, b in zip(w, w[1:])), w
    assert w[0] < 0.5 * w[1] and w[3] > 2 * w[1], w


def two_tone_gains(ref, n_fft):
    L, f1, f2, p = 96000, 110.0, 140.0, 2 ** (3 / 12)
    n = np.arange(L)
    x = (0.3 * np.sin(2 * np.pi * f1 * n / 48000) + 0.3 * np.sin(2 * np.pi * f2 * n / 48000)).astype(np.float32)
    y = pv_ref.stretch(ref, x, 1, 1.0, p, n_fft).astype(np.float64)
    seg = y[y.size // 4: 3 * y.size // 4]
    t = np.arange(seg.size)
    g = []
    for f in (f1 * p, f2 * p):
        w = 2 * np.pi * f * t / 48000
        g.append(2 * np.hypot((seg * np.cos(w)).mean(), (seg * np.sin(w)).mean()) / 0.3)
    return g


def test_close_low_partials_keep_their_amplitude_with_a_long_frame(ref):
    """110 Hz + 140 Hz (30 Hz apart, 0.3 each) shifted +3 semitones: each output partial's amplitude relative to the input's, measured
    0.86 / 0.53 at 1024 (the two share 47 Hz bins and beat) and 0.98 / 0.98 at 4096"""
    g1024, g4096 = two_tone_gains(ref, 1024), two_tone_gains(ref, 4096)
    e1024, e4096 = max(abs(g - 1) for g in g1024), max(abs(g - 1) for g in g4096)
    assert e4096 < 0.05 and e1024 > 0.3, (g1024, g4096)


def test_abi_declares_the_sizes(nae):
    h = open(os.path.join(ROOT, "include", "nae_gpu.h")).read()
    lib = nae.load_library()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", h), s
        assert s in nae.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert re.search(r"#define\s+NAE_ABI_VERSION\s+3\b", h)


def test_host_node_fft_size_key(tmp_path):
    """Velocity_modifier / Pitch_modifier: "fft_size" round-trips, is absent by default and at 1024; a value outside 512 / 1024 / 2048 / 4096
    and a size other than 1024 with "phase_lock": true are "Wrong field: fft_size" """
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "json", "fft_size"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST PV NODE OK json fft_size" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
