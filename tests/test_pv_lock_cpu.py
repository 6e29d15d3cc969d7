"""K7 with identity phase locking, no GPU: the CPU statement (tests/pv_ref/ref_pv.c) pinned to the oracle with lock = 0, the amplitude
a locked steady tone keeps, the peak and region rules on hand-built spectra, the host nodes' "phase_lock" key, and the C ABI's declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def tone(L, f_bin, amp=0.5):
    return (amp * np.sin(2 * np.pi * f_bin / 1024 * np.arange(L))).astype(np.float32)


@pytest.mark.parametrize("rate,pitch", [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12)), (1.5, 1 / 1.5), (0.6, 1 / 0.6), (0.5, 2.0),
                                        (1.3, 1.0 / 1.1)])
def test_unlocked_restatement_is_the_oracle(ref, rate, pitch):
    """lock = 0: samples and phases equal orc.stretch / orc.pv_synth_phase bit for bit, on noise and on a tone (+3 semitones and
    1.3 / (1/1.1) run the transposer first)"""
    L, ch = 20000, 2
    noise = orc.fill_uniform(L * ch, 3)
    m = tone(L, 23.5)
    for x in (noise, np.stack([m, 0.5 * m], 1).reshape(-1)):
        a, b = pv_ref.stretch(ref, x, ch, rate, pitch, lock=False), orc.stretch(x, ch, rate, pitch)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(pv_ref.synth_phase(ref, x, ch, rate, pitch, lock=False), orc.pv_synth_phase(x, ch, rate, pitch))


def mid_rms(y):
    y = np.asarray(y, np.float64).reshape(-1, 2)
    n = y.shape[0]
    return float(np.sqrt(np.mean(y[n // 4: 3 * n // 4] ** 2)))


@pytest.mark.parametrize("f_bin", [23.5, 40.25])
@pytest.mark.parametrize("rate,pitch", [(0.6, 1 / 0.6), (1.5, 1 / 1.5), (1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12))])
def test_locked_tone_keeps_its_amplitude(ref, f_bin, rate, pitch):
    """a steady off-centre sine, 0.5 amplitude, stereo: locked, the RMS of the steady middle is within 1 % of the input's (measured:
    within 0.01 %); unlocked, the same input loses more (measured 2-16 %)"""
    m = tone(96000, f_bin)
    x = np.stack([m, m], 1).reshape(-1)
    r_in = float(np.sqrt(np.mean(m.astype(np.float64) ** 2)))
    locked = mid_rms(pv_ref.stretch(ref, x, 2, rate, pitch, lock=True)) / r_in
    unlocked = mid_rms(pv_ref.stretch(ref, x, 2, rate, pitch, lock=False)) / r_in
    assert abs(locked - 1) <= 0.01, locked
    assert abs(unlocked - 1) > abs(locked - 1) and unlocked < 0.99, (unlocked, locked)


def spectrum(**points):
    P = np.zeros(513, np.float32)
    for k, v in points.items():
        P[int(k[1:])] = v
    return P


def test_peak_rules(ref):
    P = spectrum(k10=1.0, k11=1.0, k100=2.0, k101=1.0, k102=3.0, k512=5.0, k0=4.0)
    pk = pv_ref.peaks(ref, P)
    assert pk[10] and not pk[11], "a two-bin plateau yields its lower bin"
    assert not pk[100] and pk[102], "P[k] >= P[k+2] is required"
    assert pk[0] and pk[512], "neighbours outside 0..512 count as satisfied"
    assert pk.sum() == 4
    P2 = P.copy()
    P2[50], P2[51] = NAN, 1.0
    pk2 = pv_ref.peaks(ref, P2)
    assert not pk2[50] and not pk2[51], "a NaN is never a peak and blocks its neighbours"
    P3 = spectrum(k60=1.0, k61=NAN)
    assert not pv_ref.peaks(ref, P3)[60]
    assert not pv_ref.peaks(ref, np.zeros(513, np.float32)).any(), "P[k] > 0 is required"


def test_region_rules(ref):
    sg = pv_ref.regions(ref, spectrum(k10=1.0, k20=1.0))
    assert (sg[:16] == 10).all() and sg[15] == 10, "a tie goes to the lower peak"
    assert (sg[16:] == 20).all()
    sg = pv_ref.regions(ref, spectrum(k10=1.0, k21=1.0))
    assert sg[15] == 10 and sg[16] == 21
    assert (pv_ref.regions(ref, np.zeros(513, np.float32)) == np.arange(513)).all(), "silence: unlocked"
    P = np.full(513, NAN, np.float32)
    assert (pv_ref.regions(ref, P) == np.arange(513)).all(), "a non-finite frame has no peak"
    sg = pv_ref.regions(ref, spectrum(k300=1.0))
    assert (sg == 300).all(), "one peak takes every bin"


def test_host_node_phase_lock_key(tmp_path):
    """Velocity_modifier / Pitch_modifier: "phase_lock" round-trips, is absent by default, and a non-bool is "Wrong field: phase_lock" """
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "json", "phase_lock"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST PV NODE OK json phase_lock" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_abi_declares_phase_lock(nae):
    h = open(os.path.join(ROOT, "include", "nae_gpu.h")).read()
    assert re.search(r"#define\s+NAE_STRETCH_PHASE_LOCK\s+1u", h)
    lib = nae.load_library()
    for s in ("nae_stretch_block_ex_f32", "nae_stretch_create_ex", "nae_debug_pv_tile_phase_ex"):
        assert re.search(r"\b" + s + r"\s*\(", h), s
        assert s in nae.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert nae.STRETCH_PHASE_LOCK == 1
    assert re.search(r"#define\s+NAE_ABI_VERSION\s+3\b", h)
