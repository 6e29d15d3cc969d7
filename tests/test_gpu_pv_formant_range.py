"""Formant preservation on the GPU over its whole range, against the CPU statement tests/pv_ref/ref_pv.c: the lifters where the
kernels' cepstral indexing changes (1, 2, odd, N/4 - 1 and N/4, where pva_formant's two packed ranges meet; odd lifters on the locked
kernel's (n, n + 1) pairs), the high-rate default lifters, the tempo and transposer limits, both sides of the snap to rho = 1, signal levels
where the spectral floor and the gain cap bind, non-finite samples, and envelopes that change every frame.

Bars: samples within 1e-4 relative RMS (per channel where a channel is quiet); tilings, the streaming handle and batch positions give the same
bits; prof_report names the formant kernel that ran (and resample_kernel from rho = 4101/512 on), so no case is vacuous."""
import ctypes as C

import numpy as np
import pytest

import orc
import pv_ref
from conftest import rel_rms
from pv_gpu import block, profiled, same_bits, stream
from test_pv_formant_range_cpu import RHO_DIRECT, cap_signal, floor_signal

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
CONFIGS = [(512, False), (1024, False), (2048, False), (4096, False), (1024, True)]      # (N, phase lock)
ORDERS = [(1.0, 2.0), (0.25, 2.0)]          # rho = 2: transposer first; rho = 1/2: vocoder first


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


@pytest.fixture(scope="module")
def tile_ctxs(nae):
    out = {}
    for tile in (1000000, 16, 1):
        out[tile] = nae.Context(0)
        out[tile].debug_set("pv_tile", tile)
    yield out
    for c in out.values():
        c.close()


def run(c, nae, x, ch, rate, pitch, n_fft, lifter, lock=False, n_streams=1):
    """x: [n_streams][L][ch] flattened -> (interleaved output [n_streams][out_len * ch], kernels launched)"""
    return profiled(c, block, c, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=lifter, n_streams=n_streams)


def formant_kernel(lock):
    return "pvlock_synth_formant_kernel" if lock else "pv_any_synth_formant_kernel"


def assert_formant_ran(launched, lock):
    plain = "pvlock_synth_kernel" if lock else "pv_any_synth_kernel"
    assert formant_kernel(lock) in launched and plain not in launched, launched


def check(c, nae, ref, x, ch, rate, pitch, n_fft, q, lock, label, per_channel=False):
    """the formant kernel ran; finite; within TOL of the statement (each channel on its own if per_channel); returns (output, worst error)"""
    got, launched = run(c, nae, x, ch, rate, pitch, n_fft, q, lock)
    assert_formant_ran(launched, lock)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock=lock, lifter=q)
    assert got.size == want.size > 0 and np.isfinite(got).all(), label
    if per_channel:
        e = max(rel_rms(got[k::ch], want[k::ch]) for k in range(ch))
    else:
        e = rel_rms(got, want)
    print(f"{label}: {e:.3g}")
    assert e <= TOL, (label, e)
    return got, e


# ------------------------------------------------------------------------------------------------ lifters
@pytest.mark.parametrize("n_fft", SIZES)
def test_lifters_unlocked(ctx, nae, ref, n_fft):
    """q = 1, 2, 63, 68, N/4 - 1 and N/4 (pva_formant's c[n < q] and c[N - j] meet in its M-float array at N/4), both stage orders, mono
    and stereo"""
    L = 12000
    for q in sorted({1, 2, 63, 68, n_fft // 4 - 1, n_fft // 4}):
        for rate, pitch in ORDERS:
            for ch in (1, 2):
                x = orc.fill_uniform(L * ch, 50 + q + ch)
                check(ctx, nae, ref, x, ch, rate, pitch, n_fft, q, False, f"N={n_fft} q={q} {rate}/{pitch} ch{ch}")


def test_lifters_locked(ctx, nae, ref):
    """odd lifters split lock_formant_apply's (n, n + 1) cepstrum pairs: q = 1, 63, 68, 255, 256"""
    L = 12000
    for q in (1, 63, 68, 255, 256):
        for rate, pitch in ORDERS:
            for ch in (1, 2):
                x = orc.fill_uniform(L * ch, 60 + q + ch)
                check(ctx, nae, ref, x, ch, rate, pitch, 1024, q, True, f"locked q={q} {rate}/{pitch} ch{ch}")


@pytest.mark.parametrize("sample_rate", [96000, 192000])
@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_high_rate_default_lifters(ctx, nae, ref, n_fft, lock, sample_rate):
    """the default lifter at 96 and 192 kHz (N/4 at 512, and at 1024 for 192 kHz, where the locked kernel reaches it): the block call within
    the bar of the statement, the streaming handle with that lifter equal to it bit for bit.  The handle keeps the reference's 8 - 48 kHz
    envelope (NAE_ERR_UNSUPPORTED at these rates), lifted with sample_rate 0"""
    q = nae.formant_lifter(sample_rate, n_fft)
    assert q == min(sample_rate // 700, n_fft // 4)
    L, ch, rate, pitch = 20000, 2, 1.0, float(np.float32(2 ** (-5 / 12)))
    x = (0.5 * orc.fill_uniform(L * ch, 81)).astype(np.float32)
    blk, _ = check(ctx, nae, ref, x, ch, rate, pitch, n_fft, q, lock, f"{sample_rate} Hz N={n_fft} lock={lock} q={q}")
    rng = np.random.default_rng(sample_rate + n_fft + lock)
    h = C.c_void_p()
    assert ctx.lib.nae_stretch_create_formant(ctx.h, sample_rate, ch, rate, pitch, 1 if lock else 0, n_fft, q, C.byref(h)) == -2
    y = stream(ctx, x, ch, rate, pitch, [int(v) for v in rng.integers(1, 6000, 12)], "formant", n_fft, flags=int(lock), lifter=q,
               sample_rate=0, repeat_last=True)
    assert same_bits(y, blk)


# ------------------------------------------------------------------------------------------------ the range
# (tempo, rho) at the limits of tests/test_pv_formant_range_cpu.py's grid
RANGE = [(16.0, 1 / 16), (1 / 16, 16.0), (1 / RHO_DIRECT, RHO_DIRECT), (1 / 64, 16.0), (1 / 64, RHO_DIRECT), (16.0, 1 / 2), (16.0, 2.0)]


@pytest.mark.parametrize("tempo,rho", RANGE)
@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_range_limits(ctx, tile_ctxs, nae, ref, n_fft, lock, tempo, rho):
    """odd lifter 63, stereo noise long enough for 40 vocoder output hops: within the bar of the statement; 1- and 16-frame tiles give the
    one-tile bits; the streaming handle (1-sample puts, then seeded random cuts) gives the block call's bits"""
    rate, pitch = float(np.float32(rho * tempo)), float(np.float32(1 / tempo))
    q, ch = 63, 2
    L = max(12000, int(np.ceil(40 * (n_fft // 4) * tempo * max(rho, 1.0))))
    x = (0.5 * orc.fill_uniform(L * ch, 91)).astype(np.float32)
    got, launched = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock)
    assert_formant_ran(launched, lock)
    assert ("resample_kernel" in launched) == (rate * pitch >= RHO_DIRECT), (rate * pitch, launched)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock=lock, lifter=q)
    assert got.size == want.size > 0 and np.isfinite(got).all()
    e = rel_rms(got, want)
    print(f"N={n_fft} lock={lock} tempo {tempo:.4g} rho {rho:.4g}: {e:.3g}")
    assert e <= TOL, e
    for tile in (1000000, 16, 1):
        t, _ = run(tile_ctxs[tile], nae, x, ch, rate, pitch, n_fft, q, lock)
        assert same_bits(t, got), tile
    rng = np.random.default_rng(n_fft + int(lock))
    puts = [1] * min(L // 4, 1500) + [int(v) for v in rng.integers(1, max(2, L // 6), 30)]
    assert same_bits(stream(ctx, x, ch, rate, pitch, puts, "formant", n_fft, flags=int(lock), lifter=q, repeat_last=True), got)


# ------------------------------------------------------------------------------------------------ near rho = 1
# rho = 1 +- 2e-6 with the lifter against the unflagged call, relative RMS.  Below 1 the gain moves by |rho - 1| k dLs/dk: measured 1.9e-5 -
# 4.6e-5.  Above 1 the Nyquist bin reads the envelope at M rho > M, so its gain is 0: the output loses that bin, measured
# 9.0e-3 (N = 4096) - 2.7e-2 (N = 512), about 0.6 / sqrt(M)
NEAR_ONE = {-1: 1e-4, 1: 4e-2}


@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_near_rho_one(ctx, nae, ref, n_fft, lock):
    """tempo 1/2.  Inside the 1e-6 snap (rho = 1 +- 5e-7) the transposer is off, so formant preservation is: the lifter-0 bits.  Just outside
    (1 +- 2e-6) the formant kernel runs, within the bar of the statement and within NEAR_ONE of the unflagged call, but not equal to it"""
    L, ch, q = 16000, 2, pv_ref.default_lifter(48000, n_fft)
    x = (0.5 * orc.fill_uniform(L * ch, 17)).astype(np.float32)
    pitch = 2.0
    for d in (-5e-7, 5e-7):
        rate = (1 + d) / pitch
        pl = ctx.stretch_plan(rate, pitch, L, n_fft)
        assert pl.pv_on and not pl.rs_on
        a, launched = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock)
        assert formant_kernel(lock) not in launched, launched
        b, _ = run(ctx, nae, x, ch, rate, pitch, n_fft, 0, lock)
        assert same_bits(a, b), d
    for d in (-2e-6, 2e-6):
        rate = (1 + d) / pitch
        pl = ctx.stretch_plan(rate, pitch, L, n_fft)
        assert pl.pv_on and pl.rs_on
        got, _ = check(ctx, nae, ref, x, ch, rate, pitch, n_fft, q, lock, f"N={n_fft} lock={lock} rho 1{d:+g}")
        off, _ = run(ctx, nae, x, ch, rate, pitch, n_fft, 0, lock)
        e = rel_rms(got, off)
        print(f"  vs unflagged: {e:.3g}")
        assert 0 < e <= NEAR_ONE[int(np.sign(d))], e


# ------------------------------------------------------------------------------------------------ levels and spectra
@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_levels(ctx, nae, ref, n_fft, lock):
    """silence: exact zeros.  A silent channel beside a loud one: the silent one exactly zero, the loud one within the bar.  Noise at 2^-36,
    per channel.  Noise scaled by 2^20 and 2^-20: within the bar of the statement, and of the unscaled output scaled"""
    L, ch = 12000, 2
    q = pv_ref.default_lifter(48000, n_fft)
    noise = (0.5 * orc.fill_uniform(L * ch, 23)).astype(np.float32)
    for rate, pitch in ORDERS:
        tag = f"N={n_fft} lock={lock} {rate}/{pitch}"
        z, launched = run(ctx, nae, np.zeros(L * ch, np.float32), ch, rate, pitch, n_fft, q, lock)
        assert_formant_ran(launched, lock)
        assert z.size > 0 and np.all(z == 0), tag                       # +0.0 or -0.0
        one = noise.reshape(L, ch).copy()
        one[:, 1] = 0.0
        got, _ = check(ctx, nae, ref, one.reshape(-1), ch, rate, pitch, n_fft, q, lock, tag + " silent ch1", per_channel=True)
        assert np.all(got[1::2] == 0), tag
        check(ctx, nae, ref, (noise * np.float32(2.0 ** -36)).astype(np.float32), ch, rate, pitch, n_fft, q, lock, tag + " 2^-36",
              per_channel=True)
        base, _ = run(ctx, nae, noise, ch, rate, pitch, n_fft, q, lock)
        for s in (20, -20):
            got, _ = check(ctx, nae, ref, (noise * np.float32(2.0 ** s)).astype(np.float32), ch, rate, pitch, n_fft, q, lock,
                           tag + f" 2^{s}", per_channel=True)
            e = rel_rms(got.astype(np.float64) * 2.0 ** -s, base)
            print(f"  vs the unscaled output: {e:.3g}")
            assert e <= TOL, (s, e)


@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_cap_and_floor_signals(ctx, nae, ref, n_fft, lock):
    """the signals of tests/test_pv_formant_range_cpu.py: the cap signal shifted down by rho = 1/4 and 1/2 (G = 16 on 13 % of the energy at
    1/4), the floor signal (2^-36, 60 - 72 % of the bins on the floor) shifted down and up, stereo with the second channel at half level"""
    L, ch = 12000, 2
    q = pv_ref.default_lifter(48000, n_fft)
    for kind, rho in (("cap", 0.25), ("cap", 0.5), ("floor", 0.5), ("floor", 2.0)):
        m = (cap_signal if kind == "cap" else floor_signal)(L)
        x = np.stack([m, np.float32(0.5) * m], 1).reshape(-1).astype(np.float32)
        check(ctx, nae, ref, x, ch, 1.0, rho, n_fft, q, lock, f"N={n_fft} lock={lock} {kind} rho {rho}", per_channel=True)


# ------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_non_finite_sample_is_confined(ctx, nae, ref, n_fft, lock, bad):
    """one NaN or +Inf sample in channel 0 with the lifter on: the non-finite span is the unflagged call's to +-16 samples (the transposer's
    reach), channel 1 stays finite, and the rest of the output is within the bar of the statement"""
    L, ch, rate, pitch = 40000, 2, 1.0, 2 ** (3 / 12)
    q = pv_ref.default_lifter(48000, n_fft)
    x = (0.5 * orc.fill_uniform(L * ch, 43)).reshape(L, ch).copy()
    x[20001, 0] = bad
    x = x.reshape(-1)
    got, launched = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock)
    assert_formant_ran(launched, lock)
    off, _ = run(ctx, nae, x, ch, rate, pitch, n_fft, 0, lock)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock=lock, lifter=q)
    got, off, want = got.reshape(-1, ch), off.reshape(-1, ch), want.reshape(-1, ch)
    assert got.shape == want.shape == off.shape
    bad_got, bad_off = ~np.isfinite(got), ~np.isfinite(off)
    assert not bad_got[:, 1].any() and not bad_off[:, 1].any(), "the clean channel stays finite"
    assert bad_got[:, 0].any() and bad_off[:, 0].any()
    lo, hi = np.flatnonzero(bad_off[:, 0])[[0, -1]]
    glo, ghi = np.flatnonzero(bad_got[:, 0])[[0, -1]]
    assert abs(int(lo) - int(glo)) <= 16 and abs(int(hi) - int(ghi)) <= 16, (lo, hi, glo, ghi)
    ok = np.ones(got.shape[0], bool)
    ok[min(lo, glo) - 16: max(hi, ghi) + 17] = False
    assert np.isfinite(want[ok]).all()
    e0, e1 = rel_rms(got[ok, 0], want[ok, 0]), rel_rms(got[:, 1], want[:, 1])
    print(f"N={n_fft} lock={lock} {bad}: span {glo}-{ghi} (unflagged {lo}-{hi}), rest {e0:.3g}, clean channel {e1:.3g}")
    assert e0 <= TOL and e1 <= TOL, (e0, e1)


# ------------------------------------------------------------------------------------------------ changing envelopes
def changing(L, seg, seed):
    """segments of seg samples cycling through loud noise, silence, a 1.5 kHz tone and noise at 2^-36: no two neighbouring frames share an
    envelope"""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    kinds = [0.5 * rng.uniform(-1, 1, L), np.zeros(L), 0.4 * np.sin(2 * np.pi * 1500 / 48000 * n), 2.0 ** -36 * rng.uniform(-1, 1, L)]
    y = np.empty(L)
    for s in range(0, L, seg):
        y[s:s + seg] = kinds[(s // seg) % 4][s:s + seg]
    return y.astype(np.float32)


@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_changing_envelope(ctx, nae, ref, n_fft, lock):
    """a new level and spectrum every 1.3 analysis hops, both stage orders, stereo (channel 1 offset by half a segment): within the bar"""
    L, ch = 24000, 2
    q = pv_ref.default_lifter(48000, n_fft)
    seg = int(1.3 * n_fft / 4)
    for rate, pitch in ORDERS + [(1.0, 2 ** (-5 / 12))]:
        a = changing(L, seg, 5)
        b = np.roll(changing(L, seg, 6), seg // 2)
        x = np.stack([a, b], 1).reshape(-1)
        check(ctx, nae, ref, x, ch, rate, pitch, n_fft, q, lock, f"N={n_fft} lock={lock} {rate:.4f}/{pitch:.4f}", per_channel=True)


def batch_kinds(n, L, ch, seed):
    """n streams of [L][ch]: loud, silent, floor-level, NaN-carrying, tonal and changing streams side by side"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, L, ch), np.float32)
    for s in range(n):
        k = s % 6
        if k == 0:
            v = 0.5 * rng.uniform(-1, 1, (L, ch))
        elif k == 1:
            v = np.zeros((L, ch))
        elif k == 2:
            v = 2.0 ** -36 * rng.uniform(-1, 1, (L, ch))
        elif k == 3:
            v = 0.5 * rng.uniform(-1, 1, (L, ch))
            v[int(rng.integers(L)), 0] = np.nan
        elif k == 4:
            v = 0.4 * np.sin(2 * np.pi * (300 + 200 * s) / 48000 * np.arange(L))[:, None] * np.ones(ch)
        else:
            v = np.stack([changing(L, 333, 100 + s + c) for c in range(ch)], 1)
        out[s] = v
    return out.reshape(-1)


@pytest.mark.parametrize("n_fft,lock", CONFIGS)
def test_mixed_batch_each_equals_its_lone_run(ctx, nae, n_fft, lock):
    """24 streams of the six kinds of batch_kinds: each equals its own lone run bit for bit (NaN payloads included), so no envelope leaks
    between streams, waves or frames"""
    n, L, ch, rate, pitch = 24, 9000, 2, 1.0, 2 ** (4 / 12)
    q = pv_ref.default_lifter(48000, n_fft)
    x = batch_kinds(n, L, ch, 31)
    got, launched = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock, n_streams=n)
    assert_formant_ran(launched, lock)
    got = got.reshape(n, -1)
    for s in range(n):
        one, _ = run(ctx, nae, x.reshape(n, -1)[s].copy(), ch, rate, pitch, n_fft, q, lock)
        assert same_bits(one, got[s]), s
    assert np.all(got[1] == 0) and not np.isfinite(got[3]).all() and np.isfinite(got[0]).all()
