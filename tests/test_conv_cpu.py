"""K10 long convolution, no GPU: the CPU statement (tests/conv_ref/ref_conv.c) against a float64 convolution at every frame size and against the
FIR filter's statement where one partition suffices; the library's host-side entries nae_conv_design_reverb, nae_conv_reverb_taps and
nae_conv_pick_n_fft against their restatements (tests/conv_ref.py); the reverb node's JSON keys and the three registration calls
(tests/conv_ref/host_conv_node.cpp)."""
import subprocess

import numpy as np
import pytest

import conv_ref
import node_harness
from conftest import rel_rms

# the statement against float64: the bound the project uses for its float64 pins (K9 measured 1.3e-7 ... 3.4e-7 against it).  Measured here
# 1.3e-7 ... 3.0e-7, 64 partitions included ("K10 long convolution"): the bound leaves a factor of 33, more than the four asked for
RMS_BOUND = 1e-5


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return conv_ref.build(str(tmp_path_factory.mktemp("ref_conv")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("conv_ref/host_conv_node.cpp", str(tmp_path_factory.mktemp("host_conv")))


def _signals(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return {"noise": rng.uniform(-1, 1, n).astype(np.float32),
            "two-tone": (0.6 * np.sin(2 * np.pi * 0.0371 * t) + 0.3 * np.sin(2 * np.pi * 0.213 * t + 1.0)).astype(np.float32)}


CASES = [(n, L) for n in conv_ref.SIZES for L in (1, n // 2, n // 2 + 1, 3 * (n // 2) + 5)] + [(512, 64 * 256 - 3)]


@pytest.mark.parametrize("n_fft,L", CASES)
def test_statement_against_float64_convolution(ref, n_fft, L):
    B = n_fft // 2
    P = conv_ref.parts(L, n_fft)
    in_len = (P + 3) * B + 7
    taps = np.random.default_rng(100 + n_fft + L).uniform(-1, 1, L).astype(np.float32)
    for name, x in _signals(in_len, n_fft + L).items():
        err = rel_rms(conv_ref.run(ref, taps, n_fft, x), conv_ref.direct(taps, x))
        print(f"n_fft {n_fft} L {L} P {P} {name}: rel RMS {err:.3g}")
        assert err <= RMS_BOUND, (n_fft, L, name, err)


@pytest.mark.parametrize("n_fft", conv_ref.SIZES)
def test_one_partition_is_the_fir_statement(ref, n_fft):
    B = n_fft // 2
    rng = np.random.default_rng(n_fft)
    x = rng.uniform(-1, 1, 4 * B + 7).astype(np.float32)
    for L in (1, 2, B - 1, B):
        taps = rng.uniform(-1, 1, L).astype(np.float32)
        assert np.array_equal(conv_ref.run(ref, taps, n_fft, x).view(np.uint32), conv_ref.fir_run(ref, taps, n_fft, x).view(np.uint32)), L


def test_statement_channels_take_their_own_taps_and_limits_are_rejected(ref):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (1500, 2)).astype(np.float32)
    taps = rng.uniform(-1, 1, (2, 600)).astype(np.float32)
    y = conv_ref.run(ref, taps, 512, x.reshape(-1), ch=2).reshape(-1, 2)
    for c in range(2):
        assert np.array_equal(y[:, c], conv_ref.run(ref, taps[c], 512, np.ascontiguousarray(x[:, c])))
    one = np.zeros(8, np.float32)
    big = np.zeros(262145, np.float32)
    run = lambda L, n: ref.ref_conv_run(big.ctypes.data, L, n, one.ctypes.data, 8, 1, one.ctypes.data)
    assert run(0, 512) == -1 and run(262145, 4096) == -1 and run(512 * 256 + 1, 512) == -1 and run(3, 300) == -1
    assert run(512 * 256, 512) == 0 and run(262144, 4096) == 0


def test_pick_n_fft(nae, ref):
    lib = nae.load_library()
    for L in (-1, 0, 1, 2, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 72000, 262144, 262145, 1 << 30):
        want = conv_ref.pick_n_fft(L)
        assert lib.nae_conv_pick_n_fft(L) == want == ref.ref_conv_pick_n_fft(L), L
        assert nae.Context.conv_pick_n_fft(L) == want
    assert conv_ref.pick_n_fft(4096) == 512 and conv_ref.pick_n_fft(4097) == 1024 and conv_ref.pick_n_fft(32769) == 4096
    assert conv_ref.pick_n_fft(262144) == 4096 and conv_ref.pick_n_fft(262145) == 0


def _ulp_diff(a, b):
    """distance in f32 steps between same-signed neighbours (and 0 against -0 counts 0)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("sample_rate,rt60,predelay,dry,wet,seed", ((48000, 1.5, 0.02, 1.0, 0.3, 1), (44100, 0.1, 0.0, 0.0, 1.0, 2),
                                                                      (8000, 5.0, 0.2, 0.5, 0.7, 1 << 40), (22050, 0.73, 0.0131, 1.0, 0.0, 7)))
def test_design_against_float64_restatement(nae, ref, sample_rate, rt60, predelay, dry, wet, seed):
    n = nae.Context.conv_reverb_taps(sample_rate, rt60, predelay)
    d = int(np.floor(predelay * sample_rate + 0.5))
    assert n == ref.ref_conv_reverb_taps(sample_rate, rt60, predelay) == d + int(np.ceil(rt60 * sample_rate))
    got = nae.Context.conv_design_reverb(sample_rate, rt60, predelay, dry, wet, seed)
    want = conv_ref.design_reverb(ref, sample_rate, rt60, predelay, dry, wet, seed)
    assert got.shape == want.shape == (n,)
    assert _ulp_diff(got, want.astype(np.float32)).max() <= 1
    wet_part = got.astype(np.float64).copy()
    wet_part[0] -= dry if d > 0 else 0.0
    if d > 0:
        assert got[0] == np.float32(dry) and not got[1:d].any(), "silent before the pre-delay"
        assert abs(np.sum(wet_part[d:] ** 2) - wet * wet) <= 1e-6
    else:
        assert abs(np.sum((want - np.eye(1, n)[0] * dry) ** 2) - wet * wet) <= 1e-6


def test_designed_decay_reaches_minus_60_db_at_rt60(nae):
    """Schroeder integration of the wet part: the backward energy integral, relative to the whole, is -60 dB +- 1 dB at rt60 behind the pre-delay"""
    sr, rt60, pre = 48000, 0.8, 0.01
    n = nae.Context.conv_reverb_taps(sr, 2 * rt60, pre)            # a response twice as long, so that the integral at rt60 has its tail
    h = nae.Context.conv_design_reverb(sr, rt60, pre, 0.0, 1.0, 5, n).astype(np.float64)
    d = round(pre * sr)
    edc = np.cumsum((h[d:] ** 2)[::-1])[::-1]
    db = 10 * np.log10(edc[int(rt60 * sr)] / edc[0])
    print(f"Schroeder decay at rt60: {db:.2f} dB")
    assert abs(db + 60.0) <= 1.0, db
    # the level of the response itself: the rms of 10 ms around rt60 against 10 ms at the start
    w = sr // 100
    lvl = 10 * np.log10(np.mean(h[d + int(rt60 * sr) - w // 2:][:w] ** 2) / np.mean(h[d:d + w] ** 2))
    assert abs(lvl + 60.0) <= 2.0, lvl


def test_design_seeds_differ_and_repeat(nae):
    a = nae.Context.conv_design_reverb(48000, 0.3, 0.0, 0.0, 1.0, 1)
    b = nae.Context.conv_design_reverb(48000, 0.3, 0.0, 0.0, 1.0, 2)
    assert np.array_equal(a, nae.Context.conv_design_reverb(48000, 0.3, 0.0, 0.0, 1.0, 1))
    assert abs(np.dot(a.astype(np.float64), b.astype(np.float64))) < 0.05, "unit-energy responses of two seeds are decorrelated"


def test_design_rejections(nae):
    lib = nae.load_library()
    INVALID = -1
    out = np.zeros(48000, np.float32)
    des = lambda sr, rt, pre, dry, wet, n, p=out.ctypes.data: lib.nae_conv_design_reverb(sr, rt, pre, dry, wet, 1, n, p)
    assert des(48000, 0.5, 0.01, 1.0, 0.3, 24480) == 0
    assert des(0, 0.5, 0.01, 1.0, 0.3, 1000) == INVALID and des(-1, 0.5, 0.01, 1.0, 0.3, 1000) == INVALID
    for rt in (0.0, -1.0, 10.5, float("nan"), float("inf")):
        assert des(48000, rt, 0.01, 1.0, 0.3, 1000) == INVALID, rt
        assert lib.nae_conv_reverb_taps(48000, rt, 0.01) == INVALID, rt
    for pre in (-0.001, 1.001, float("nan")):
        assert des(48000, 0.5, pre, 1.0, 0.3, 1000) == INVALID, pre
        assert lib.nae_conv_reverb_taps(48000, 0.5, pre) == INVALID, pre
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert des(48000, 0.5, 0.01, bad, 0.3, 1000) == INVALID and des(48000, 0.5, 0.01, 1.0, bad, 1000) == INVALID
    assert des(48000, 0.5, 0.01, 1.0, 0.3, 480) == INVALID, "n_taps < d + 1"
    assert des(48000, 0.5, 0.01, 1.0, 0.3, 481) == 0
    assert des(48000, 0.5, 0.01, 1.0, 0.3, 1000, None) == INVALID
    assert lib.nae_conv_reverb_taps(0, 0.5, 0.01) == INVALID
    assert lib.nae_conv_reverb_taps(48000, 10.0, 1.0) == 48000 + 480000
    with pytest.raises(nae.NaeError):
        nae.Context.conv_design_reverb(48000, 0.0, 0.0, 1.0, 0.3, 1, 100)


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>" """
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST CONV OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """register_all_processors() gives 7 entries, register_extension_processors() 8 without audio_reverb, register_effect_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST CONV OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    # the registry on both sides of register_effect_processors(); the sizes behind the two calls in front of it (7, 8) are the harness's CHECKs
    assert [len(l) for l in lines] == [8, 9]
    assert "audio_reverb" not in lines[0] and "audio_filter" in lines[0]
    assert sorted(lines[1]) == sorted(lines[0] + ["audio_reverb"])
