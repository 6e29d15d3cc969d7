"""K7 on the GPU over the whole supported range: the transposer's kernel regimes up to rho = 16 (the tiled kernel's 768 / 512-frame tiles,
its 4-stream groups, the direct kernel past the staging limit), the vocoder at tempos 1/64 ... 16 at every frame size (locked at 1024),
inputs around one frame long, the size-generic tile policy on both sides of its switch, and the streaming handle at the extremes.

References: orc.stretch / orc.pv_synth_phase at 1024, tests/pv_ref/ref_pv.c at the other sizes and locked.
Bars: integer phases bit-exact, samples within 1e-4 relative RMS; prof_report names the kernel that ran, so no case is vacuous."""
import ctypes as C

import numpy as np
import pytest

import orc
import pv_ref
from conftest import rel_rms
from pv_gpu import block, profiled, same_bits, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
RESIDENT3 = {512: 16, 1024: 8, 2048: 6, 4096: 3}     # PvAny<N>::kResident3 (kernels_pv_any.hip)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


@pytest.fixture(scope="module")
def ctxs(nae):
    """the library's transposer, the direct kernel (rs_direct) and one stream per workgroup (rs_single)"""
    out = {}
    for key in ("default", "rs_direct", "rs_single"):
        c = nae.Context(0)
        if key != "default":
            c.debug_set(key, 1)
        out[key] = c
    yield out
    for c in out.values():
        c.close()


def want_ref(ref, x, ch, rate, pitch, n_fft, lock=False):
    if n_fft == 1024 and not lock:
        return orc.stretch(x, ch, rate, pitch)
    return pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock)


def run(c, nae, x, ch, rate, pitch, n_fft=1024, n_streams=1, lock=False, planar_in=False, planar_out=False):
    """x: [n_streams][L][ch] flattened; returns [n_streams][out_len * ch] interleaved, the kernels launched and the plan"""
    out, launched = profiled(c, block, c, nae, x, ch, rate, pitch, n_fft, lock=lock, n_streams=n_streams, planar_in=planar_in,
                             planar_out=planar_out)
    return out.reshape(n_streams, -1), launched, c.stretch_plan(rate, pitch, x.size // (ch * n_streams), n_fft)


# ------------------------------------------------------------------------------------------------ B.1 transposer regimes
# (rho, kernel).  768-frame tiles while floor(768 rho) + 28 <= 1536 (rho <= 1508/768), else 512-frame tiles; 4-stream stereo groups while the
# staging row floor(512 rho) + 28 rounded up to 4 is <= 1536 (rho < 1509/512); the tiled kernel while floor(512 rho) + 28 <= kRsMaxSpan = 4128
# (rho < 4101/512), else the direct kernel
RHO = [(1 / 16, "resample_tile_kernel"), (0.26, "resample_tile_kernel"), (1508 / 768, "resample_tile_kernel"),
       (1509 / 768, "resample_tile_kernel"), (1508 / 512, "resample_tile_kernel"), (1509 / 512, "resample_tile_kernel"),
       (4.5, "resample_tile_kernel"), (4100 / 512, "resample_tile_kernel"), (4101 / 512, "resample_kernel"), (12.0, "resample_kernel"),
       (16.0, "resample_kernel")]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rho,kernel", RHO)
def test_transposer_regimes(ctxs, nae, rho, kernel, ch):
    """the transposer alone (pitch 1): the kernel the span rule names, within 1e-4 of orc.stretch for streams 0 and last of 1, 3 and 4 + 1
    streams, planar and interleaved; the direct kernel and one stream per workgroup give the default launch's bits"""
    L = max(64, int(6000 * rho))
    for n_streams in (1, 3, 5):
        x = (0.5 * orc.fill_uniform(n_streams * L * ch, 61 + n_streams)).astype(np.float32)
        for planar_in, planar_out in ((False, False), (True, True), (False, True)):
            got, launched, pl = run(ctxs["default"], nae, x, ch, rho, 1.0, n_streams=n_streams, planar_in=planar_in, planar_out=planar_out)
            assert pl.rs_on and not pl.pv_on
            assert kernel in launched and ({"resample_tile_kernel", "resample_kernel"} - {kernel}).isdisjoint(launched), launched
            for s in sorted({0, n_streams - 1}):
                want = orc.stretch(x.reshape(n_streams, -1)[s], ch, rho, 1.0)
                e = rel_rms(got[s], want)
                assert got[s].size == want.size and e <= TOL, (n_streams, s, e)
            for key in ("rs_direct", "rs_single"):
                alt, launched2, _ = run(ctxs[key], nae, x, ch, rho, 1.0, n_streams=n_streams, planar_in=planar_in, planar_out=planar_out)
                assert ("resample_kernel" in launched2) == (key == "rs_direct" or kernel == "resample_kernel"), (key, launched2)
                assert same_bits(alt, got), (key, n_streams, planar_in, planar_out)


# ------------------------------------------------------------------------------------------------ B.2 vocoder at the tempo limits
TEMPOS = [1 / 64, 1 / 63, 0.26, 3.9, 8.0, 16.0]
RHOS = [1.0, 0.5, 3.0, 12.0]          # no transposer; after the vocoder; before it; before it, direct kernel


def case_signal(tempo, rho, n_fft, seed):
    """noise with ~max(12000, 20 H) vocoder output frames (>= 2 tiles of 16 frames at every N; the vocoder runs first and makes 1/rho times
    the output when rho < 1); stereo where the input stays short"""
    out = int(max(12000, 20 * n_fft // 4) / min(rho, 1.0))
    L = max(64, int(out * tempo * rho))
    ch = 2 if L <= 200000 else 1
    return (0.5 * orc.fill_uniform(L * ch, seed)).astype(np.float32), ch


@pytest.fixture(scope="module")
def tile_ctxs(nae):
    out = {}
    for tile in (16, 1):
        out[tile] = nae.Context(0)
        out[tile].debug_set("pv_tile", tile)
    yield out
    for c in out.values():
        c.close()


def check_tile_phases(c, nae, x, ch, rate, pitch, n_fft, want_qs, tile, lock=False):
    L = x.size // ch
    d_x = c.array(x)
    got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, 1, phase_lock=lock, n_fft=n_fft)
    d_x.free()
    assert t == tile and got.shape[2] >= 2
    bins = n_fft // 2 + 1
    for j in range(got.shape[2]):
        for c2 in range(ch):
            want = want_qs[j * tile - 1, c2] if j > 0 else np.zeros(bins, np.int32)
            assert np.array_equal(got[0, c2, j], want), (tile, j, c2, int(np.count_nonzero(got[0, c2, j] != want)))


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("tempo", TEMPOS)
@pytest.mark.parametrize("n_fft", SIZES)
def test_vocoder_at_the_tempo_limits(ctx, tile_ctxs, nae, ref, n_fft, tempo, rho):
    """tile phases with 16- and 1-frame tiles bit-exact; samples within 1e-4 of the restatement; the size's vocoder kernels ran"""
    pitch = 1 / tempo
    rate = rho / pitch
    x, ch = case_signal(tempo, rho, n_fft, 71)
    pl = ctx.stretch_plan(rate, pitch, x.size // ch, n_fft)
    assert pl.pv_on and bool(pl.rs_on) == (rho != 1.0)
    qs = orc.pv_synth_phase(x, ch, rate, pitch) if n_fft == 1024 else pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft)
    for tile in (16, 1):
        check_tile_phases(tile_ctxs[tile], nae, x, ch, rate, pitch, n_fft, qs, tile)
    got, launched, _ = run(ctx, nae, x, ch, rate, pitch, n_fft)
    want = want_ref(ref, x, ch, rate, pitch, n_fft)
    assert got[0].size == want.size and np.isfinite(got).all()
    e = rel_rms(got[0], want)
    print(f"N={n_fft} tempo {tempo:.4f} rho {rho:.4f} ch{ch}: {e:.3g}")
    assert e <= TOL, e
    assert ("pv_any_synth_kernel" in launched) == (n_fft != 1024), launched
    if rho == 12.0:
        assert "resample_kernel" in launched, launched


@pytest.mark.parametrize("rho", RHOS)
@pytest.mark.parametrize("tempo", TEMPOS)
def test_locked_vocoder_at_the_tempo_limits(ctx, tile_ctxs, nae, ref, tempo, rho):
    pitch = 1 / tempo
    rate = rho / pitch
    x, ch = case_signal(tempo, rho, 1024, 73)
    qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, lock=True)
    for tile in (16, 1):
        check_tile_phases(tile_ctxs[tile], nae, x, ch, rate, pitch, 1024, qs, tile, lock=True)
    got, launched, _ = run(ctx, nae, x, ch, rate, pitch, 1024, lock=True)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, lock=True)
    assert got[0].size == want.size and np.isfinite(got).all()
    e = rel_rms(got[0], want)
    print(f"locked tempo {tempo:.4f} rho {rho:.4f} ch{ch}: {e:.3g}")
    assert e <= TOL, e
    assert any(k.startswith("pvlock") for k in launched), launched


# ------------------------------------------------------------------------------------------------ B.3 edge lengths
@pytest.mark.parametrize("rate,pitch", [(0.7, 1 / 0.7), (1.6, 1 / 1.6), (1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12))])
@pytest.mark.parametrize("n_fft,lock", [(512, False), (2048, False), (4096, False), (1024, True)])
def test_edge_lengths(ctx, nae, ref, n_fft, lock, rate, pitch):
    """inputs of 0, 1, H - 1, H, N/2 - 1, N/2, N - 1, N, N + 1, N + H + 1 frames, tempo below and above 1 (and both stage orders): the plan's
    length, finite, within 1e-4 of the restatement (or a near-silent reference, the rule of test_k7_edge_lengths)"""
    N, H, ch = n_fft, n_fft // 4, 2
    for L in (0, 1, H - 1, H, N // 2 - 1, N // 2, N - 1, N, N + 1, N + H + 1):
        x = orc.fill_uniform(max(L, 1) * ch, 49 + L)[: L * ch]
        pl = ctx.stretch_plan(rate, pitch, L, n_fft)
        if L == 0:
            assert pl.out_len == 0
            d = ctx.empty(16)
            ctx.stretch_block(rate, pitch, nae.Sig.interleaved(d.ptr, 0, ch), 0, ch, 1, nae.Sig.interleaved(d.ptr, 0, ch), phase_lock=lock,
                              n_fft=n_fft)
            d.free()
            continue
        got, _, _ = run(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock)
        want = want_ref(ref, x, ch, rate, pitch, n_fft, lock)
        assert got[0].size == pl.out_len * ch == want.size, L
        assert np.isfinite(got).all(), L
        assert rel_rms(got[0], want) <= TOL or np.sqrt(np.mean(want.astype(np.float64) ** 2)) < 1e-6, (L, rel_rms(got[0], want))


# ------------------------------------------------------------------------------------------------ B.4 tile policy
def cu_count():
    hip = C.CDLL("libamdhip64.so.7")                    # already loaded by libnae_gpu.so
    v = C.c_int()
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0       # hipDeviceAttributeMultiprocessorCount
    return v.value


@pytest.mark.parametrize("n_fft", SIZES)
def test_tile_policy_threshold(nae, ref, n_fft):
    """nae_pick_tile at kResident3: below kResident3 * n_cu stream-channels a stream is cut into 2 tiles (pass 1 runs), from there on it is one tile
    (no pass 1).  Mono batches just below, at and above the switch, long enough for 65 frames (two 64-frame tiles): streams 0, middle and
    last equal their lone runs bit for bit, the first and last the restatement (at 1024 through the size-generic kernels, pv_any)"""
    n_cu = cu_count()
    assert n_cu > 0
    thr = RESIDENT3[n_fft] * n_cu
    tempo = 0.25
    H = n_fft // 4
    out = 64 * H + H                                   # frames = (out + N/2 + H - 1) / H + 1 >= 67
    L = int(out * tempo) + 1
    seen = {}
    with nae.Context(0) as c:
        if n_fft == 1024:
            c.debug_set("pv_any", 1)
        pl = c.stretch_plan(tempo, 1 / tempo, L, n_fft)
        assert (pl.frames + 63) // 64 >= 2
        for n_sc in (thr - 1, thr, thr + 1):
            d_x, d_o = c.empty(n_sc * L), c.empty(n_sc * pl.out_len)
            c.fill_uniform(d_x.ptr, L, L, n_sc, 0, 3)
            c.prof_reset(); c.prof_enable(True)
            c.stretch_block(tempo, 1 / tempo, nae.Sig.interleaved(d_x.ptr, L, 1), L, 1, n_sc, nae.Sig.interleaved(d_o.ptr, pl.out_len, 1),
                            n_fft=n_fft)
            c.sync()
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert "pv_any_synth_kernel" in launched, launched
            seen[n_sc] = "pv_any_phase_kernel" in launched
            picks = (0, n_sc // 2, n_sc - 1)
            rows = {}
            for s in picks:
                buf = np.empty(pl.out_len, np.float32)
                c._ck(c.lib.nae_memcpy_d2h(c.h, buf.ctypes.data, d_o.at(s * pl.out_len), buf.nbytes))
                rows[s] = buf
            c.sync()
            d_x.free(); d_o.free()
            for s in picks:
                xs = orc.fill_uniform(L, orc.stream_seed(s, 3))
                lone, _, _ = run(c, nae, xs, 1, tempo, 1 / tempo, n_fft)
                assert same_bits(rows[s], lone[0]), (n_sc, s)
                if s != n_sc // 2:
                    assert rel_rms(rows[s], want_ref(ref, xs, 1, tempo, 1 / tempo, n_fft)) <= TOL, (n_sc, s)
    assert seen == {thr - 1: True, thr: False, thr + 1: False}, seen


# ------------------------------------------------------------------------------------------------ B.5 streaming handle at the extremes
EXTREMES = [(1 / 64, 1.0), (16.0, 1.0), (1.0, 16.0)]     # (tempo, rho)


@pytest.mark.parametrize("tempo,rho", EXTREMES)
@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (2048, False), (4096, False), (1024, True)])
def test_stream_handle_at_the_extremes(ctx, nae, n_fft, lock, tempo, rho):
    """1-frame puts for a stretch, then seeded random cuts, then flush: the block call's bits"""
    rate, pitch = float(np.float32(rho * tempo)), float(np.float32(1 / tempo))
    ch = 2
    out_frames = 24 * n_fft
    L = int(out_frames * tempo * rho)
    x = (0.5 * orc.fill_uniform(L * ch, 7)).astype(np.float32)
    blk, _, pl = run(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock)
    assert pl.out_len > 0
    rng = np.random.default_rng(n_fft + int(lock))
    ones = min(L // 4, 1500)
    puts = [1] * ones + [int(v) for v in rng.integers(1, max(2, L // 6), 30)]
    y = stream(ctx, x, ch, rate, pitch, puts, "ex" if n_fft == 1024 else "n", n_fft, flags=int(lock), repeat_last=True)
    assert y.size == blk[0].size
    assert same_bits(y, blk[0])
