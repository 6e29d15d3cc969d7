"""Formant preservation over its whole range, no GPU: the CPU statement tests/pv_ref/ref_pv.c pinned to the float64 numpy
statement (tests/pv_sizes_numpy.py) at every frame size, at the lifters where the kernels change behaviour (1, 2, odd, N/4 - 1, N/4) and
at the tempo and transposer limits; the default lifter at every sample rate up to 192 kHz; and the two signals that make the gain cap and the
spectral floor bind, shown to do so, which tests/test_gpu_pv_formant_range.py runs on the GPU."""
import numpy as np
import pytest

import orc
import pv_ref
import pv_sizes_numpy
from conftest import rel_rms
from golden import pv_numpy

SIZES = pv_ref.SIZES
FLOOR, CAP = 2.0 ** -40, 16.0          # the spectral floor of step 1 and NAE_FORMANT_MAX_GAIN
RHO_DIRECT = 4101 / 512                # from here on the transposer runs resample_kernel (tests/test_gpu_stretch_range.py)

# (tempo, rho): a pure pitch shift (tempo 1/rho) at rho = 1/16 ... 16, then tempo 1/64 and tempo 16 at two ratios each
PIN_CASES = [(1 / r, r) for r in (1 / 16, 1 / 2, 2.0, RHO_DIRECT, 16.0)] + [(1 / 64, RHO_DIRECT), (1 / 64, 16.0), (16.0, 1 / 2), (16.0, 2.0)]


def lifters(n_fft):
    return (1, 2, 63, n_fft // 4 - 1, n_fft // 4)


def pin_bar(tempo, rho):
    """1e-5, except where the formant gain attenuates the output while the vocoder's own float32 error stays.  At rho = 16 the gain of bin k
    reads the envelope at 16 k, in the transposer's stopband: the output's RMS falls to 0.26 of the unflagged one, the absolute error does not
    (N = 1024: 6.9e-6 relative unflagged, 1.9e-5 with the lifter), so the relative error grows by about 1/0.26 (measured up to 2.2e-5).  At
    tempo 1/64 the R = 64 phase rounding of the range tests (bar 1e-4 there, tests/test_stretch_range_cpu.py) meets the same attenuation:
    measured up to 6.4e-5."""
    if tempo < 1 / 32:
        return 1e-4
    if rho > 12:
        return 5e-5
    return 1e-5


def pin_length(tempo, rho, n_fft):
    """at least 12000 input samples, and enough for about 12 vocoder output hops (tempo 16 shrinks the vocoder's output 16 times)"""
    return max(12000, int(np.ceil(12 * (n_fft // 4) * tempo * max(rho, 1.0))))


def numpy_statement_all_lifters(x, tempo, rho, n_fft, qs):
    """pv_sizes_numpy.stretch for mono x at every lifter in qs, sharing the transposer when it runs first"""
    pl = pv_sizes_numpy.plan(rho * tempo, 1 / tempo, x.size, n_fft)
    assert pl["pv_on"] and pl["rs_on"]
    g = float(np.float32(pl["rho"]))
    x = x.astype(np.float64)
    if pl["rs_first"]:
        v = pv_numpy.transposer(x, pl, pl["mid"])
        return {q: pv_sizes_numpy.vocoder(v, pl, pl["out_len"], q, g) for q in qs}
    return {q: pv_numpy.transposer(pv_sizes_numpy.vocoder(x, pl, pl["mid"], q, g), pl, pl["out_len"]) for q in qs}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


@pytest.mark.parametrize("tempo,rho", PIN_CASES)
@pytest.mark.parametrize("n_fft", SIZES)
def test_statement_pinned_over_the_range(ref, n_fft, tempo, rho):
    """white noise (the reason: tests/test_pv_formant_cpu.py::test_statement_matches_the_numpy_specification), lifters 1, 2, 63, N/4 - 1 and
    N/4: within pin_bar of the float64 statement.  The numpy statement is the one helped by the shared transposer, nothing else"""
    L = pin_length(tempo, rho, n_fft)
    x = orc.fill_uniform(L, 3)
    want = numpy_statement_all_lifters(x, tempo, rho, n_fft, lifters(n_fft))
    bar = pin_bar(tempo, rho)
    for q in lifters(n_fft):
        got = pv_ref.stretch(ref, x, 1, rho * tempo, 1 / tempo, n_fft, lifter=q)
        assert got.size == want[q].size > 0, q
        e = rel_rms(got, want[q])
        print(f"N={n_fft} tempo {tempo:.4g} rho {rho:.4g} q={q}: {e:.3g}")
        assert e <= bar, (q, e)


# sample rate -> sample_rate // 700 ("Formant preservation"), before the clamp to [1, N/4]
RATES = {1000: 1, 8000: 11, 11025: 15, 22050: 31, 44100: 63, 48000: 68, 88200: 126, 96000: 137, 176400: 252, 192000: 274}


@pytest.mark.parametrize("n_fft", SIZES)
def test_default_lifter_at_every_rate(nae, n_fft):
    """nae_stretch_formant_lifter, nae.formant_lifter and pv_ref.default_lifter agree, and the clamp to N/4 applies exactly where
    sample_rate // 700 exceeds it: 96000, 176400 and 192000 Hz at N = 512 (128), 192000 Hz at N = 1024 (256); q = 1 at 1000 Hz and below"""
    lib = nae.load_library()
    for sr, raw in RATES.items():
        want = min(raw, n_fft // 4)
        got = (lib.nae_stretch_formant_lifter(sr, n_fft), nae.formant_lifter(sr, n_fft), pv_ref.default_lifter(sr, n_fft))
        assert got == (want,) * 3, (sr, got, want)
    clamped = {sr for sr, raw in RATES.items() if raw > n_fft // 4}
    assert clamped == {512: {96000, 176400, 192000}, 1024: {192000}, 2048: set(), 4096: set()}[n_fft]
    for sr in clamped:
        assert nae.formant_lifter(sr, n_fft) == n_fft // 4
    for sr in (1, 300, 699, 1000, 1399):
        assert nae.formant_lifter(sr, n_fft) == 1 == pv_ref.default_lifter(sr, n_fft), sr
    assert nae.formant_lifter(1400, n_fft) == 2


# ------------------------------------------------------------------------------------------------ signals where the clamps bind
def lowpassed(L, seed, level=1.0, fc=0.03, order=3):
    """white noise through |H(f)| = 1 / (1 + (f / fc)^order), fc in cycles per sample (1.44 kHz at 48 kHz): 18 dB per octave above fc, 55 dB
    down at Nyquist.  A steeper stopband would sink below the float32 transforms' rounding noise (see test_statement_pinned_where_the_clamps_bind)"""
    x = orc.fill_uniform(L, seed).astype(np.float64)
    X = np.fft.rfft(x)
    f = np.arange(X.size) / L
    return (level * np.fft.irfft(X / (1 + (f / fc) ** order), L)).astype(np.float32)


def cap_signal(L, seed=5):
    """shifted down by rho = 1/4, bin k of the synthesis reads the envelope at k / 4, two octaves down the slope, 36 dB above its own: G = 16 there"""
    return lowpassed(L, seed)


def floor_signal(L, seed=5):
    """the cap signal at 2^-36: its stopband bins fall below 2^-40, so step 1 clamps them"""
    return lowpassed(L, seed, 2.0 ** -36)


def analysis_gains(x, n_fft, q, rho):
    """(G, |X|) of the float64 statement over Hann frames of x every N/2 samples: what the vocoder's analysis sees when it runs first"""
    x = np.asarray(x, np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    g = float(np.float32(rho))
    Gs, As = [], []
    for s in range(0, x.size - n_fft + 1, n_fft // 2):
        X = np.fft.rfft(x[s:s + n_fft] * w)
        Gs.append(pv_sizes_numpy.gain(X, n_fft, q, g))
        As.append(np.abs(X))
    return np.array(Gs), np.array(As)


def cap_share(x, n_fft, q, rho):
    """the share of the synthesis energy sum |G X|^2 over (frame, bin) pairs whose gain is capped at 16"""
    G, A = analysis_gains(x, n_fft, q, rho)
    e = (G * A) ** 2
    return float(e[G >= CAP].sum() / e.sum())


def floor_share(x, n_fft, q=1, rho=0.5):
    """the share of (frame, bin) pairs where max(|X|, 2^-40) is the floor"""
    _, A = analysis_gains(x, n_fft, q, rho)
    return float(np.mean(A < FLOOR))


@pytest.mark.parametrize("n_fft", SIZES)
def test_cap_signal_binds_the_cap(n_fft):
    """measured: 12.6 - 13.0 % of the synthesis energy at G = 16 with the default lifter, rho = 1/4; white noise: none"""
    q = min(68, n_fft // 4)
    assert cap_share(cap_signal(24000), n_fft, q, 0.25) >= 0.05
    assert cap_share(orc.fill_uniform(24000, 5), n_fft, q, 0.25) < 1e-3


@pytest.mark.parametrize("n_fft", SIZES)
def test_floor_signal_binds_the_floor(n_fft):
    """measured: 60 - 72 % of the bins below 2^-40; the same signal at full scale: none"""
    assert floor_share(floor_signal(24000), n_fft) >= 0.5
    assert floor_share(cap_signal(24000), n_fft) == 0.0


@pytest.mark.parametrize("n_fft", SIZES)
@pytest.mark.parametrize("kind,rho", [("cap", 0.25), ("cap", 0.5), ("floor", 0.5), ("floor", 2.0)])
def test_statement_pinned_where_the_clamps_bind(ref, n_fft, kind, rho):
    """the cap and floor signals, a pure pitch shift, default 48 kHz lifter: within 1e-5 of the float64 statement (measured 1.4e-6 -
    3.8e-6).  A 30 dB per octave stopband instead (80 - 90 dB down in the vocoder's input, where the float32 transforms' rounding noise enters
    the log spectrum) measured 3.8e-6 - 6.1e-4 for the same reason white noise is the range pin's signal"""
    L = 12000
    x = (cap_signal if kind == "cap" else floor_signal)(L)
    q = pv_ref.default_lifter(48000, n_fft)
    got = pv_ref.stretch(ref, x, 1, 1.0, rho, n_fft, lifter=q)
    want = pv_sizes_numpy.stretch(x, 1, 1.0, rho, n_fft, q)
    assert got.size == want.size
    e = rel_rms(got, want)
    print(f"N={n_fft} {kind} rho {rho}: {e:.3g}")
    assert e <= 1e-5, e
