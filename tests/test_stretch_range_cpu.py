"""K7 over the whole supported parameter range, no GPU: the plan of every frame size at the tempo limits (1/64, 16), the transposer limits
(rho = 1/16, 16), one step outside each and on both sides of the 1e-6 snap to 1; and the CPU statement tests/pv_ref/ref_pv.c
against the float64 specification tests/pv_sizes_numpy.py at every size, at extreme tempos and at the transposer ratios where the GPU
changes kernels (tests/test_gpu_stretch_range.py)."""
import math

import numpy as np
import pytest

import orc
import pv_ref
import pv_sizes_numpy
from conftest import rel_rms
from pv_gpu import tone
from pv_ref import SIZES
from test_pv_sizes_cpu import FIELDS, lib_plan

UNSUPPORTED = -2   # NAE_ERR_UNSUPPORTED
TEMPO_MIN, TEMPO_MAX, RHO_MIN, RHO_MAX = 1 / 64, 16.0, 1 / 16, 16.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def below(v):
    return math.nextafter(v, 0.0)


def above(v):
    return math.nextafter(v, math.inf)


def inside_cases():
    """(rate, pitch) at each limit: tempo = 1/pitch, rho = rate * pitch"""
    out = []
    for tempo in (TEMPO_MIN, TEMPO_MAX):
        out += [(tempo, 1 / tempo), (RHO_MIN * tempo, 1 / tempo), (RHO_MAX * tempo, 1 / tempo)]
    out += [(RHO_MIN, 1.0), (RHO_MAX, 1.0)]
    return out


def outside_cases():
    """one double-precision step outside each limit, through the same double arithmetic as the plan (tempo = 1 / pitch, rho = rate * pitch)"""
    out = []
    p_lo, p_hi = above(1 / TEMPO_MIN), below(1 / TEMPO_MAX)     # 1/pitch: just below 1/64, just above 16
    assert 1.0 / p_lo < TEMPO_MIN and 1.0 / p_hi > TEMPO_MAX
    out += [(1.0 / p_lo, p_lo), (1.0 / p_hi, p_hi)]
    for r in (below(RHO_MIN), above(RHO_MAX)):
        assert not (RHO_MIN <= r * 1.0 <= RHO_MAX)
        out.append((r, 1.0))
    for tempo in (TEMPO_MIN, 1.0, TEMPO_MAX):                   # the transposer's limits, with and without the vocoder
        pitch = 1 / tempo
        for rate in (below(RHO_MIN / pitch), above(RHO_MAX / pitch)):
            while RHO_MIN <= rate * pitch <= RHO_MAX:           # one more step where the product rounds back onto the limit
                rate = below(rate) if rate < 1 else above(rate)
            out.append((rate, pitch))
    return out


@pytest.mark.parametrize("n_fft", SIZES)
def test_plan_at_the_limits(nae, ref, n_fft):
    """inside: accepted, every field the restatement's (and at 1024 the oracle's), 0 < R <= 2^30; outside by one step: NAE_ERR_UNSUPPORTED"""
    L = 10000
    for rate, pitch in inside_cases():
        rc, pl = lib_plan(nae, rate, pitch, n_fft, L)
        assert rc == 0, (rate, pitch)
        rc2, want = pv_ref.plan(ref, rate, pitch, n_fft, L)
        assert rc2 == 0
        for f in FIELDS:
            assert getattr(pl, f) == getattr(want, f), (rate, pitch, f)
        assert list(pl.r_q24) == list(want.r_q24)
        if n_fft == 1024:
            rc3, o = orc.plan(rate, pitch, L)
            assert rc3 == 0
            for f in FIELDS:
                assert getattr(pl, f) == getattr(o, f), (rate, pitch, f)
        if pl.pv_on:
            assert all(0 < r <= 2 ** 30 for r in pl.r_q24), list(pl.r_q24)
            if abs(pl.tempo_eff - TEMPO_MIN) < 1e-12:
                assert pl.r_q24[0] == 2 ** 30 and pl.d0 == n_fft // 4 // 64     # the edge of the positive-int32 claim, at every size
    for rate, pitch in outside_cases():
        rc, _ = lib_plan(nae, rate, pitch, n_fft, L)
        assert rc == UNSUPPORTED, (rate, pitch, rc)
        assert pv_ref.plan(ref, rate, pitch, n_fft, L)[0] == UNSUPPORTED
        if n_fft == 1024:
            assert orc.plan(rate, pitch, L)[0] == UNSUPPORTED


@pytest.mark.parametrize("n_fft", SIZES)
def test_plan_snaps_to_one_within_1e6(nae, ref, n_fft):
    """a tempo or a ratio within 1e-6 of 1 is 1 (that stage is off); just outside the snap it runs"""
    for eps, on in ((0.9e-6, False), (-0.9e-6, False), (1.1e-6, True), (-1.1e-6, True)):
        rc, pl = lib_plan(nae, 1 + eps, 1 / (1 + eps), n_fft, 10000)          # tempo 1 + eps, rho ~ 1
        assert rc == 0 and bool(pl.pv_on) == on and not pl.rs_on, eps
        assert (pl.tempo_eff == 1.0) == (not on)
        rc, pl = lib_plan(nae, 1 + eps, 1.0, n_fft, 10000)                     # rho 1 + eps, tempo 1
        assert rc == 0 and bool(pl.rs_on) == on and not pl.pv_on, eps
        assert (pl.rate_eff == 1.0) == (not on)
        rc2, want = pv_ref.plan(ref, 1 + eps, 1.0, n_fft, 10000)
        assert rc2 == 0 and want.rs_on == pl.rs_on and want.out_len == pl.out_len


# (tempo, rho): the vocoder alone, the transposer alone (rho past the GPU's tile switches and the direct kernel), and both on both stage
# orders (rho > 1: transposer first)
VOCODER = [(t, 1.0) for t in (1 / 64, 0.1, 0.3, 0.75, 0.9)]
TRANSPOSER = [(1.0, r) for r in (1 / 16, 0.26, 3.9, 8.0078125, 8.01, 16.0)]
BOTH = [(1 / 64, 16.0), (0.3, 3.9), (0.1, 8.01), (0.75, 1 / 16), (0.9, 0.26), (1 / 64, 0.26)]


@pytest.mark.parametrize("tempo,rho", VOCODER + TRANSPOSER + BOTH)
@pytest.mark.parametrize("n_fft", SIZES)
def test_restatement_matches_the_specification_over_the_range(ref, n_fft, tempo, rho):
    """ref_pv.c against pv_sizes_numpy.py, ~12000 output frames, noise mono and stereo, and the two-tone signal where the vocoder is off
    or the tempo is 1/64.  Within 1e-5 relative RMS (measured at most 2.7e-6 for tempos 0.1 - 0.9 and 8.8e-8 for the transposer alone), except
    at tempo 1/64: there R = H / d = 64, and every analysis phase's float32 rounding reaches the synthesis phase 64 times larger (the increments
    telescope to R times the last frame's error), measured 1.3e-5 - 4.0e-5 at every size, so the bar there is 1e-4.
    Tempo >= 1 is left out for the reason written in test_pv_sizes_cpu.test_restatement_matches_the_numpy_specification: a Hann main-lobe bin
    1-2 bins from a partial advances by about half a turn per analysis hop, and float32 against float64 rounding decides its wrap.  The two-tone
    signal meets the same wrap decisions at tempos below 1 whenever R is not an integer (a wrong wrap then costs a fraction of a turn):
    measured 6e-4 - 9e-3 at tempo 0.3 - 0.75, so tones run only where the wrap cannot matter (R = 64, or no vocoder)."""
    pitch = 1 / tempo
    rate = rho / pitch
    n = max(64, int(12000 * tempo * rho))
    tol = 1e-4 if tempo == 1 / 64 else 1e-5
    signals = [("noise", 1, orc.fill_uniform(n, 5)), ("noise", 2, orc.fill_uniform(2 * n, 6))]
    if tempo in (1.0, 1 / 64):
        m = tone(n)
        signals += [("tone", 1, m), ("tone", 2, np.stack([m, 0.5 * m], 1).reshape(-1))]
    for kind, ch, x in signals:
        got = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft)
        want = pv_sizes_numpy.stretch(x, ch, rate, pitch, n_fft)
        assert got.size == want.size and got.size > 0
        e = rel_rms(got, want)
        print(f"N={n_fft} tempo {tempo:.4f} rho {rho:.4f} {kind} ch{ch}: {e:.3g}")
        assert e <= tol, (kind, ch, e)
