"""K8 spectrum at every size (n_fft = 256 ... 4096, any hop), no GPU: the CPU restatement of the canonical FFT
(tests/spec_sizes/ref_spectrum.c) against the oracle at 1024 / 256 and against numpy float64 at every size; the library's
frames_ex; the host node's "fft_size" / "hop" JSON keys (tests/spec_sizes/host_spectrum.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import node_harness
import orc
from conftest import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "spec_sizes")
SIZES = (256, 512, 1024, 2048, 4096)
# relative RMS against float64 rfft of the same windowed f32 frames: measured 0.8e-7 ... 1.2e-7 (the bound leaves room)
RMS_BOUND = {256: 4e-7, 512: 4e-7, 1024: 4e-7, 2048: 5e-7, 4096: 5e-7}


def _build_ref(out_dir):
    so = os.path.join(out_dir, "libref_spectrum.so")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                        os.path.join(HERE, "ref_spectrum.c"), "-o", so, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ref_frames.restype = C.c_size_t
    L.ref_frames.argtypes = [C.c_size_t, C.c_int, C.c_int]
    L.ref_spectrum_f32.restype = C.c_int
    L.ref_spectrum_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return _build_ref(str(tmp_path_factory.mktemp("ref_spectrum")))


def ref_spectrum(L, x, ch, n_fft, hop):
    """x: interleaved [T*ch] f32 -> [frames, ch, n_fft/2 + 1]"""
    x = np.ascontiguousarray(x, np.float32)
    T = x.size // ch
    F = L.ref_frames(T, n_fft, hop)
    out = np.empty((F, ch, n_fft // 2 + 1), np.float32)
    if F:
        assert L.ref_spectrum_f32(x.ctypes.data, T, ch, n_fft, hop, out.ctypes.data) == 0
    return out


def f64_spectrum(x, ch, n_fft, hop):
    x = np.asarray(x, np.float32).reshape(-1, ch)
    n = np.arange(n_fft)
    w = (0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)).astype(np.float32)
    F = (x.shape[0] - n_fft) // hop + 1
    out = np.empty((F, ch, n_fft // 2 + 1))
    for f in range(F):
        for c in range(ch):
            xw = (x[f * hop:f * hop + n_fft, c] * w).astype(np.float64)   # the f32 window product, as specified
            out[f, c] = np.abs(np.fft.rfft(xw))
    return out


def test_restatement_at_1024_is_the_oracle(ref, golden):
    g = golden["spectrum"]
    for name in ("tone", "noise", "impulse"):
        x = g[name + "_in"]
        assert np.array_equal(ref_spectrum(ref, x, 1, 1024, 256).view(np.uint32), orc.spectrum(x, 1).view(np.uint32)), name
    rng = np.random.default_rng(3)
    for ch in (1, 2):
        x = rng.uniform(-1, 1, 5000 * ch).astype(np.float32)
        assert np.array_equal(ref_spectrum(ref, x, ch, 1024, 256).view(np.uint32), orc.spectrum(x, ch).view(np.uint32)), ch


@pytest.mark.parametrize("n_fft", SIZES)
def test_restatement_against_float64(ref, n_fft):
    rng = np.random.default_rng(n_fft)
    hop = n_fft // 4
    T = 3 * n_fft + 5
    noise = rng.uniform(-1, 1, 2 * T).astype(np.float32)
    t = np.arange(T)
    sine = np.stack([np.sin(2 * np.pi * 0.0371 * t), 0.25 * np.sin(2 * np.pi * 0.213 * t + 1.0)], 1).reshape(-1).astype(np.float32)
    for x in (noise, sine):
        got = ref_spectrum(ref, x, 2, n_fft, hop)
        want = f64_spectrum(x, 2, n_fft, hop)
        assert got.shape == want.shape
        err = rel_rms(got, want)
        print(f"n_fft {n_fft}: rel RMS {err:.2e}")
        assert err <= RMS_BOUND[n_fft], err


def test_restatement_peak_bin_of_a_sine(ref):
    for n_fft in SIZES:
        k0 = n_fft // 8
        x = np.sin(2 * np.pi * k0 / n_fft * np.arange(2 * n_fft)).astype(np.float32)
        s = ref_spectrum(ref, x, 1, n_fft, n_fft)
        assert s.shape == (2, 1, n_fft // 2 + 1)
        assert int(np.argmax(s[0, 0])) == k0
        assert abs(s[0, 0, k0] - n_fft / 4) < 1e-3 * n_fft   # Hann's coherent gain 1/2 of the n_fft/2 amplitude


def test_frames_ex(nae):
    lib = nae.load_library()
    fx = lib.nae_spectrum_frames_ex
    for n in SIZES:
        for hop in (1, 7, n // 4, n // 2, n):
            for T in (0, n - 1, n, n + hop - 1, n + hop, 10 * n + 3):
                want = 0 if T < n else (T - n) // hop + 1
                assert fx(T, n, hop) == want, (T, n, hop)
    assert lib.nae_spectrum_frames_ex(5000, 1024, 256) == lib.nae_spectrum_frames(5000)
    for n, hop in ((128, 32), (8192, 2048), (1000, 250), (0, 1), (-1024, 256), (1024, 0), (1024, -1), (1024, 1025), (256, 257)):
        assert fx(100000, n, hop) == 0, (n, hop)


def test_ref_frames_match_the_library(ref, nae):
    lib = nae.load_library()
    for n in SIZES:
        for hop in (1, 3, n // 4, n):
            for T in (n - 1, n, 4 * n + 17):
                assert ref.ref_frames(T, n, hop) == lib.nae_spectrum_frames_ex(T, n, hop)


def test_host_node_json_keys(tmp_path):
    """the host node's JSON: round trip, nothing written at the defaults, bad size / hop rejected with "Wrong field: ..." """
    exe = node_harness.build("spec_sizes/host_spectrum.cpp", str(tmp_path))
    r = subprocess.run([exe, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST SPECTRUM OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
