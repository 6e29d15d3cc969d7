"""K13 spectral gate, no GPU: the CPU statement (tests/denoise_ref/ref_denoise.c) — what the GPU computes bit for bit — as the STFT identity,
under exact scaling, against its float64 numpy restatement (tests/denoise_ref.py), and on a tone in noise; the profile against float64; the
design's formulas and ranges; the header's entries; the noise reduction node's JSON and the six registration calls
(tests/denoise_ref/host_denoise_node.cpp).  The measured figures stand with their tests and in DESIGN.md §3, "K13 spectral gate"."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref
import node_harness
from conftest import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
# Identity (floor_gain = 1): the relative RMS of the statement's output against its input, measured here on `noisy(n_fft)`:
IDENTITY = {512: 9.73e-8, 1024: 1.00e-7, 2048: 1.07e-7, 4096: 1.11e-7}
# The float64 restatement's output against the statement's, the statement's mask given, both smoothing widths below: the larger of the two
AGAINST_F64 = {512: 1.07e-7, 1024: 1.05e-7, 2048: 1.12e-7, 4096: 1.15e-7}
# A 1 kHz tone of amplitude 0.5 in -40 dB white noise at 48 kHz, N = 512, the defaults, the profile from the noise-only lead-in: the
# noise-only part drops by 10.98 dB and the tone stands 0.003 dB above 0.5 (amplitude 0.5002)
NOISE_DROP_DB, TONE_DB = 10.98, 0.003


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return denoise_ref.build(str(tmp_path_factory.mktemp("ref_denoise")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("denoise_ref/host_denoise_node.cpp", str(tmp_path_factory.mktemp("host_denoise")))


def noisy(n_fft):
    """x[6 N + 5, 2]: noise whose level wanders +-14 dB around 1 with a period of three frames, and a profile tilted by -6 dB per channel"""
    rng = np.random.default_rng(n_fft)
    return denoise_ref.wander(rng, 1, 6 * n_fft + 5, 2, period=3.0 * n_fft)[0], denoise_ref.flat_profile(n_fft, 2, tilt_db=-6.0)


@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_floor_gain_one_is_the_identity(ref, n_fft):
    """every gain is 1 (c = C) or 1 + 0 (c / C): the output is the input but for the roundings of two FFTs, two windows and the gain.
    Bound: four times the measured figure"""
    x, profile = noisy(n_fft)
    y, d, _ = denoise_ref.run(ref, denoise_ref.params(n_fft, 2, 2, 1.0, 1.0), profile, x, detail=True)
    err = rel_rms(y, x)
    print(f"identity, n_fft {n_fft}: relative RMS {err:.3e}; open {denoise_ref.open_share(d):.3f}")
    assert 0.2 <= denoise_ref.open_share(d) <= 0.8, "both branches of the gain are taken"
    assert err <= 4 * IDENTITY[n_fft]


@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_a_closed_gate_scales_exactly(ref, n_fft):
    """thr_scale so large that every decision is closed, floor_gain 0.25: G = 0.25 + 0.75 * 0 in every bin, a power of two, so the output
    bits are 0.25 times the identity run's (the inputs stand far above the subnormals)"""
    x, profile = noisy(n_fft)
    identity = denoise_ref.run(ref, denoise_ref.params(n_fft, 2, 2, 1.0, 1.0), profile, x)
    y, d, c = denoise_ref.run(ref, denoise_ref.params(n_fft, 2, 2, 1e30, 0.25), profile, x, detail=True)
    assert not d.any() and not c.any()
    assert np.min(np.abs(identity[identity != 0])) > 1e-20
    assert np.array_equal(y.view(np.uint32), (np.float32(0.25) * identity).view(np.uint32))


@pytest.mark.parametrize("tn,fn", ((2, 2), (8, 4)))
@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_statement_against_float64(ref, n_fft, tn, fn):
    """the statement's mask is the float64 restatement's wherever |p / threshold - 1| > 1e-5, and at most 0.1 % of the decisions lie inside
    that band; the counts are the restatement's; with the statement's mask given the restatement's output agrees to four times the measured
    relative RMS"""
    x, profile = noisy(n_fft)
    p = denoise_ref.params(n_fft, tn, fn, 1.0, 0.25)
    y, d, c = denoise_ref.run(ref, p, profile, x, detail=True)
    inside = total = 0
    worst = 0.0
    for ch in range(2):
        _, ratio, d64 = denoise_ref.run64(p, profile[ch], x[:, ch])
        band = ~(np.abs(ratio - 1.0) > 1e-5)
        inside += int(band.sum())
        total += band.size
        assert np.array_equal(d[ch].astype(bool)[~band], d64[~band])
        assert np.array_equal(denoise_ref.counts64(d[ch], tn, fn), c[ch])
        y64, _, _ = denoise_ref.run64(p, profile[ch], x[:, ch], mask=d[ch])
        worst = max(worst, rel_rms(y[:, ch], y64))
    print(f"against float64, n_fft {n_fft}, Tn {tn}, Fn {fn}: {inside} of {total} decisions inside the band; output relative RMS {worst:.3e}; "
          f"open {denoise_ref.open_share(d):.3f}")
    assert 0.2 <= denoise_ref.open_share(d) <= 0.8
    assert inside <= total // 1000
    assert worst <= 4 * AGAINST_F64[n_fft]
    full = (tn + 1) ** 2 * (fn + 1) ** 2
    assert 0 <= c.min() and c.max() <= full and len(np.unique(c)) > full // 4, "the counts spread over their range"
    if (tn, fn) == (2, 2):
        assert (c == full).any() and (c == 0).any(), "fully open and fully closed bins: both branches of the gain"


def test_mask_given_is_the_mask_used(ref):
    """the statement run on its own mask gives its own bits"""
    x, profile = noisy(512)
    p = denoise_ref.params(512, 2, 2, 1.0, 0.25)
    y, d, c = denoise_ref.run(ref, p, profile, x, detail=True)
    y2, d2, c2 = denoise_ref.run(ref, p, profile, x, detail=True, mask=d)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(d, d2) and np.array_equal(c, c2)


def test_tone_in_noise(nae, ref):
    """N = 512, the node's defaults (12 dB, 6 dB, Tn = Fn = 2), the profile learned from the noise-only lead-in: the noise-only part drops
    and the tone keeps its amplitude, each asserted with 1 dB of margin around the figure measured here"""
    rng = np.random.default_rng(512)
    n, lead, tail, n_fft = 48000, 12000, 36000, 512
    t = np.arange(n)
    w = 2 * np.pi * 1000.0 / 48000
    tone = np.where((t >= lead) & (t < tail), 0.5 * np.sin(w * t), 0.0)
    x = (rng.standard_normal(n) * 0.01 + tone).astype(np.float32)[:, None]
    profile = denoise_ref.profile(ref, n_fft, x[:lead - n_fft])
    q = nae.Context.denoise_design(12.0, 6.0, n_fft, 2, 2)
    y = denoise_ref.run(ref, denoise_ref.params(n_fft, 2, 2, q.thr_scale, q.floor_gain), profile, x)[:, 0].astype(np.float64)
    a, b = 2 * n_fft, lead - 2 * n_fft
    drop = -10 * math.log10(np.mean(y[a:b] ** 2) / np.mean(x[a:b, 0].astype(np.float64) ** 2))
    seg = slice(lead + 4 * n_fft, tail - 4 * n_fft)
    amp = 2 * math.hypot(np.mean(y[seg] * np.sin(w * t[seg])), np.mean(y[seg] * np.cos(w * t[seg])))
    tone_db = 20 * math.log10(amp / 0.5)
    print(f"tone in noise: the noise-only part drops by {drop:.2f} dB; the tone stands at {amp:.4f} ({tone_db:+.3f} dB)")
    assert drop >= NOISE_DROP_DB - 1.0
    assert abs(tone_db - TONE_DB) <= 1.0


@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_profile_against_float64(ref, n_fft):
    """bound: p = |X|^2 moves by 2 |X| |dX|, and the FFT's rounding |dX| stays under (log2 N + 2) 2^-24 of the largest bin magnitude, so a
    bin's power is off by at most 2 (log2 N + 2) 2^-24 of the largest power, under 2e-6 of it at every size; the double sum and the one
    division add nothing to that.  Measured: 0.9e-7 ... 3.2e-7 of the largest power"""
    rng = np.random.default_rng(3 * n_fft)
    for length in (n_fft, n_fft + n_fft // 4 - 1, 9 * n_fft + 3):
        x = denoise_ref.wander(rng, 1, length, 2, period=3.0 * n_fft)[0]
        got = denoise_ref.profile(ref, n_fft, x)
        h, frames = n_fft // 4, (length - n_fft) // (n_fft // 4) + 1
        for ch in range(2):
            seg = np.stack([x[f * h:f * h + n_fft, ch].astype(np.float64) for f in range(frames)]) * denoise_ref.hann64(n_fft)
            X = np.fft.rfft(seg, axis=1)
            want = np.mean(X.real ** 2 + X.imag ** 2, axis=0)
            err = float(np.max(np.abs(got[ch] - want)) / np.max(want))
            print(f"profile, n_fft {n_fft}, {length} samples, channel {ch}: {err:.3e} of the largest power")
            assert err <= 2 * (math.log2(n_fft) + 2) * 2.0 ** -24
    assert denoise_ref.profile(ref, n_fft, np.zeros((n_fft - 1, 1), np.float32)) is None, "no whole frame: rejected"


def test_design(nae, ref):
    """thr_scale = (float)10^(sensitivity / 10), floor_gain = (float)10^(-reduction / 20): the statement's bits (the same libm pow), and
    float64 numpy's value to one f32 rounding"""
    for red, sens, n_fft, tn, fn in ((12.0, 6.0, 2048, 2, 2), (0.0, -6.0, 512, 0, 0), (48.0, 24.0, 4096, 8, 4), (23.5, 9.25, 1024, 4, 3)):
        p = nae.Context.denoise_design(red, sens, n_fft, tn, fn)
        assert (p.n_fft, p.time_smooth, p.freq_smooth) == (n_fft, tn, fn)
        assert (p.thr_scale, p.floor_gain) == denoise_ref.design(ref, red, sens)
        assert abs(p.thr_scale - 10.0 ** (sens / 10.0)) <= 2.0 ** -23 * 10.0 ** (sens / 10.0)
        assert abs(p.floor_gain - 10.0 ** (-red / 20.0)) <= 2.0 ** -23 * 10.0 ** (-red / 20.0)
    p = nae.Context.denoise_design()
    assert (p.n_fft, p.time_smooth, p.freq_smooth) == (2048, 2, 2) and p.floor_gain == np.float32(10.0 ** -0.6) and p.thr_scale == np.float32(10.0 ** 0.6)
    assert nae.Context.denoise_design(0.0, 0.0).floor_gain == 1.0 and nae.Context.denoise_design(0.0, 0.0).thr_scale == 1.0


def test_design_rejections(nae):
    lib = nae.load_library()
    out = nae.DenoiseParams()
    good = dict(reduction_db=12.0, sensitivity_db=6.0, n_fft=2048, time_smooth=2, freq_smooth=2)

    def design(**kw):
        a = dict(good, **kw)
        return lib.nae_denoise_design(a["reduction_db"], a["sensitivity_db"], a["n_fft"], a["time_smooth"], a["freq_smooth"], C.byref(out))

    assert design() == 0
    for kw in (dict(reduction_db=-0.5), dict(reduction_db=48.5), dict(reduction_db=float("nan")), dict(sensitivity_db=-6.5),
               dict(sensitivity_db=24.5), dict(sensitivity_db=float("inf")), dict(time_smooth=-1), dict(time_smooth=9), dict(freq_smooth=-1),
               dict(freq_smooth=5)):
        assert design(**kw) == INVALID, kw
    for n_fft in (0, 256, 1000, 8192):
        assert design(n_fft=n_fft) == UNSUPPORTED
    assert lib.nae_denoise_design(12.0, 6.0, 2048, 2, 2, None) == INVALID
    assert design(reduction_db=0.0) == 0 and design(reduction_db=48.0) == 0 and design(sensitivity_db=-6.0) == 0 and design(sensitivity_db=24.0) == 0
    assert design(time_smooth=8, freq_smooth=4) == 0 and design(time_smooth=0, freq_smooth=0) == 0


def test_statement_rejects_what_the_library_rejects(ref):
    x = np.zeros((8, 1), np.float32)
    prof = np.ones(257, np.float32)

    def run(n_fft=512, tn=2, fn=2):
        return ref.ref_denoise_run(n_fft, tn, fn, 1.0, 0.5, prof.ctypes.data, x.ctypes.data, 8, 1, x.ctypes.data, None, None, None)

    assert run() == 0
    assert run(n_fft=256) == -1 and run(tn=9) == -1 and run(tn=-1) == -1 and run(fn=5) == -1 and run(fn=-1) == -1


def test_entries_without_a_context_are_invalid(nae):
    lib = nae.load_library()
    p = nae.DenoiseParams(*denoise_ref.as_tuple(denoise_ref.params()))
    h = C.c_void_p()
    assert lib.nae_denoise_block_f32(None, C.byref(p), None, 1, None, 0, 1, 0, None) == INVALID
    assert lib.nae_denoise_profile_f32(None, 512, None, 512, 1, None) == INVALID
    assert lib.nae_denoise_create(None, C.byref(p), None, 1, 2, C.byref(h)) == INVALID and not h.value
    assert lib.nae_denoise_put(None, None, 0) == INVALID and lib.nae_denoise_flush(None) == INVALID and lib.nae_denoise_available(None) == 0
    assert lib.nae_denoise_destroy(None) == 0


def test_header_lists_the_entries():
    """the additions stand under "Later additions within 3", the version stays 3, the debug key and the limits are documented"""
    header = open(os.path.join(ROOT, "include", "nae_gpu.h")).read()
    later = header[header.index("Later additions within 3"):header.index("#define NAE_ABI_VERSION")]
    for name in ("nae_denoise_design", "nae_denoise_profile_f32", "nae_denoise_block_f32", "nae_denoise handle", "nae_denoise_params", "K13"):
        assert name in later, name
    assert re.search(r"#define\s+NAE_ABI_VERSION\s+3\b", header)
    assert re.search(r"^ \*   dn_tile\s", header, re.M)
    spec = open(os.path.join(ROOT, "include", "nae_dsp_spec.h")).read()
    assert re.search(r"#define\s+NAE_DENOISE_MAX_TIME\s+8\b", spec) and re.search(r"#define\s+NAE_DENOISE_MAX_FREQ\s+4\b", spec)
    assert (denoise_ref.MAX_TIME, denoise_ref.MAX_FREQ) == (8, 4)


def test_host_node_json_keys(host):
    """the node's JSON: every key round-trips, the defaults are not written back, a wrong type or value is "Wrong field: <key>\""""
    r = subprocess.run([host, "json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DENOISE OK json" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_registration(host):
    """the five existing calls give 11 entries without audio_denoise, register_restoration_processors() adds it"""
    r = subprocess.run([host, "registry"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DENOISE OK registry" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    lines = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith("REGISTRY ")]
    assert [len(l) for l in lines] == [11, 12]
    assert "audio_denoise" not in lines[0] and sorted(lines[1]) == sorted(lines[0] + ["audio_denoise"])
