"""Transient preservation (NAE_STRETCH_TRANSIENTS; DESIGN.md §3, "Transient preservation") on the GPU, against the CPU statement
tests/pv_ref/ref_pv.c.

Every test runs at every size unlocked and at 1024 locked (NAE_STRETCH_PHASE_LOCK | NAE_STRETCH_TRANSIENTS, the reset maps).
Bars: the integer synthesis phases are bit-exact at every size and tiling (the segmented scan, the chunked scan from 256 tiles on, onsets on a
tile's first, second and last frame); the samples are within 1e-4 relative RMS of the statement, with and without the formant lifter; every
tiling and the streaming handle give the block call's bits; a signal without onsets gives the unflagged call's bits; the error codes and the
host graph.  Unlinked, the two channels of a stream and the streams of a batch decide on their own: on the scene of pv_gpu.py, whose channels
and streams have their onsets at different frames, every channel's phases are the statement's of that channel alone, and every stream of a
batch gives its lone run's bits — also where one workgroup holds waves of different streams.  And the range: tempo 1/64 ... 16 with the
transposer off, behind and in front, on inputs whose onsets fall in one channel only (tests/test_pv_transient_cpu.py checks that they do)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_ref
from conftest import rel_rms
from pv_gpu import RANGE_RHOS, RANGE_TEMPOS, placed_clicks, profiled, range_case, same_bits, scene, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
TR = 4                                                     # NAE_STRETCH_TRANSIENTS
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12)), (1.5, 1 / 1.5)]   # transposer first, after, none
ROUTES = [pytest.param(512, False, id="512"), pytest.param(1024, False, id="1024"), pytest.param(1024, True, id="1024-locked"),
          pytest.param(2048, False, id="2048"), pytest.param(4096, False, id="4096")]
# the most waves a workgroup of the transient kernels holds: PvAny<N, false, true>::kWaves1 of pass 1 (pv_any.h; pass 3 has 8, 8, 5, 2), and
# kWaves = 8 of the locked kernels (stft_common.h)
WG_WAVES = {(512, False): 8, (1024, False): 8, (1024, True): 8, (2048, False): 7, (4096, False): 3}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def attacks(L, ch, seed=3, n_hits=None):
    """quiet noise with clicks and short decaying noise bursts at seeded, irregular places (the second channel at 0.7 of the first's hits)"""
    rng = np.random.default_rng(seed)
    x = 0.01 * rng.standard_normal((L, ch))
    n_hits = n_hits or max(4, L // 6000)
    for p in np.sort(rng.choice(np.arange(2000, L - 3000), n_hits, replace=False)):
        if rng.random() < 0.5:
            x[p] += 0.9
        else:
            x[p:p + 2400] += (0.6 * np.exp(-np.arange(2400) / 300.0) * rng.standard_normal(2400))[:, None]
    if ch == 2:
        x[:, 1] *= 0.7
    return np.ascontiguousarray(x, np.float32).reshape(-1)


def steady(L, ch):
    """the 110 + 140 Hz two-tone with a 20 ms fade-out: no onset at any size and setting (tests/test_pv_transient_cpu.py)"""
    t = np.arange(L) / 48000
    m = 0.3 * np.sin(2 * np.pi * 110 * t) + 0.3 * np.sin(2 * np.pi * 140 * t)
    m[-960:] *= 0.5 + 0.5 * np.cos(np.pi * np.arange(960) / 960)
    return np.ascontiguousarray(np.stack([m, 0.5 * m], 1).reshape(-1) if ch == 2 else m, np.float32)


def block(c, nae, x, ch, rate, pitch, n_fft, transients=True, lifter=0, lock=False, n_streams=1):
    L = x.size // (ch * n_streams)
    pl = c.stretch_plan(rate, pitch, L, n_fft)
    d_x, d_o = c.array(x), c.empty(max(1, n_streams * pl.out_len * ch))
    c.stretch_block(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch),
                    n_fft=n_fft, formant=lifter, transients=transients, phase_lock=lock)
    out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    return out


def tile_phases(c, nae, x, ch, rate, pitch, n_fft, transients=True, lock=False, n_streams=1):
    L = x.size // (ch * n_streams)
    d_x = c.array(x)
    got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, n_streams, phase_lock=lock, n_fft=n_fft,
                                   transients=transients)
    d_x.free()
    return got, t


def check_tiles(got, tile, qs, ch, s=0):
    """stream s of got [streams, ch, tiles, bins] against the statement's phases qs [frames, ch, bins] of that stream"""
    bins = qs.shape[2]
    assert got.shape[2] == (qs.shape[0] + tile - 1) // tile, (got.shape, qs.shape, tile)
    for j in range(got.shape[2]):
        for c2 in range(ch):
            want = qs[j * tile - 1, c2] if j > 0 else np.zeros(bins, np.int32)
            assert np.array_equal(got[s, c2, j], want), (tile, s, j, c2, int(np.count_nonzero(got[s, c2, j] != want)))


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", PAIRS)
@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_integer_phases_bit_exact(nae, ref, n_fft, lock, rate, pitch, ch):
    """Qs in front of every tile equals the statement's phase of the frame before it, bit for bit, with tiles of 1, 2, 3, 16 and 64 frames;
    onsets fall on a 16-frame tile's first, second and last frame"""
    L = 60000 * n_fft // 1024
    for i, x in enumerate((attacks(L, ch), placed_clicks(nae, L, ch, rate, pitch, n_fft))):
        qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock, transients=True)
        # the resets change the attacks' phases (a lone click in silence may already get its analysis phases without one: a flat spectrum
        # has no peak, so the locked frame runs unlocked)
        assert i == 1 or not np.array_equal(qs, pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock))
        for tile in (1, 2, 3, 16, 64):
            with nae.Context(0) as c:
                c.debug_set("pv_tile", tile)
                got, t = tile_phases(c, nae, x, ch, rate, pitch, n_fft, lock=lock)
            assert t == tile
            check_tiles(got, tile, qs, ch)
    on = np.nonzero(pv_ref.onsets(ref, x, ch, rate, pitch, n_fft).any(1))[0]
    assert {0, 1, 15} <= set(on % 16), sorted(set(on % 16))


@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_chunked_scan_phases(nae, ref, n_fft, lock):
    """a lone stereo stream of more than 256 16-frame tiles (pv_scan_chunked_kernel, segmented; locked: pvlock_scan_kernel in 16 chunks) with
    onsets in several of its 16 chunks"""
    ch, rate, pitch, tile = 2, 1.5, 1 / 1.5, 16
    L = int(16 * 270 * (n_fft // 4) * 1.5)
    x = attacks(L, ch, seed=11, n_hits=60)
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    n_tiles = (pl.frames + tile - 1) // tile
    assert n_tiles >= 256
    on = np.nonzero(pv_ref.onsets(ref, x, ch, rate, pitch, n_fft).any(1))[0]
    per = (n_tiles + 15) // 16
    assert len(set(on // tile // per)) >= 8, on
    qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock, transients=True)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", tile)
        (got, t), launched = profiled(c, tile_phases, c, nae, x, ch, rate, pitch, n_fft, lock=lock)
    want = ({"pvlock_map_transient_kernel", "pvlock_scan_transient_kernel"} if lock
            else {"pv_any_phase_transient_kernel", "pv_any_scan_chunked_transient_kernel"})
    assert want <= launched, launched
    check_tiles(got, tile, qs, ch)


@pytest.mark.parametrize("lifter", [0, "default"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", PAIRS)
@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_samples_vs_statement(ctx, nae, ref, n_fft, lock, rate, pitch, ch, lifter):
    """within 1e-4 relative RMS of the flagged CPU statement, with and without the formant lifter (it applies with the transposer on)"""
    L = 40000
    x = attacks(L, ch, seed=5)
    q = pv_ref.default_lifter(48000, n_fft) if lifter == "default" else 0
    got, launched = profiled(ctx, block, ctx, nae, x, ch, rate, pitch, n_fft, True, q, lock)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lock, lifter=q, transients=True)
    assert got.size == want.size and np.isfinite(got).all()
    e = rel_rms(got, want)
    print(f"N={n_fft} lock={lock} rel RMS {rate:.4f}/{pitch:.4f} ch{ch} q{q}: {e:.3g}")
    assert e <= TOL, e
    synth = "pvlock_synth" if lock else "pv_any_synth"
    assert any(k.startswith(synth) and k.endswith("transient_kernel") for k in launched), launched
    assert not any(k.startswith("pv_pipe") or k.startswith("pv_flow") or k == "pv_phase_kernel" for k in launched), launched


@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_every_tiling_gives_the_same_bits(nae, n_fft, lock):
    """one tile, 1-, 2-, 3-, 16- and 64-frame tiles and the library's choice give the same samples bit for bit"""
    ch, rate, pitch = 2, 1.0, 2 ** (-7 / 12)
    L = 80000 * n_fft // 1024
    x = attacks(L, ch, seed=13)
    outs = {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("1", {"pv_tile": 1}), ("2", {"pv_tile": 2}), ("3", {"pv_tile": 3}),
                       ("16", {"pv_tile": 16}), ("64", {"pv_tile": 64}), ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            outs[key] = block(c, nae, x, ch, rate, pitch, n_fft, lock=lock)
    for key in outs:
        assert same_bits(outs[key], outs["one tile"]), key


def onset_cuts(ref, nae, x, ch, rate, pitch, n_fft):
    """put sizes whose running totals make an onset frame available exactly, one sample early and one sample late"""
    L = x.size // ch
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    on = np.nonzero(pv_ref.onsets(ref, x, ch, rate, pitch, n_fft).any(1))[0]
    ends = []
    for i, f in enumerate(on[1:12]):
        end = (((int(f) - 1) * pl.ha_q24 + (1 << 23)) >> 24) - n_fft // 2 + n_fft
        ends.append(end + (0, -1, 1)[i % 3])
    ends = sorted({e for e in ends if 0 < e < L}) + [L]
    return [b - a for a, b in zip([0] + ends[:-1], ends) if b > a]


@pytest.mark.parametrize("entry", ["n", "formant"])
@pytest.mark.parametrize("rate,pitch", [(1.0, float(np.float32(2 ** (-7 / 12)))), (1.5, float(np.float32(1 / 1.5))),
                                        (1.0, float(np.float32(2 ** (3 / 12))))])
@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_stream_handle_equals_block(ctx, nae, ref, n_fft, lock, rate, pitch, entry):
    """puts cut at, one sample before and one after the input that completes onset frames, 1152-frame puts and seeded random cuts, flush
    included, equal the block call bit for bit (the _formant entry with its default lifter)"""
    L, ch = 120000, 2
    x = attacks(L, ch, seed=17)
    q = pv_ref.default_lifter(48000, n_fft) if entry == "formant" else 0
    blk = block(ctx, nae, x, ch, rate, pitch, n_fft, lifter=q, lock=lock)
    assert not same_bits(blk, block(ctx, nae, x, ch, rate, pitch, n_fft, transients=False, lifter=q, lock=lock))
    rng = np.random.default_rng(n_fft)
    cuts = onset_cuts(ref, nae, x, ch, rate, pitch, n_fft)
    for puts in (cuts, [1152], [int(v) for v in rng.integers(1, 30000, 40)]):
        y = stream(ctx, x, ch, rate, pitch, puts, entry, n_fft, flags=TR | (1 if lock else 0), lifter=q)
        assert y.size == blk.size
        assert same_bits(y, blk), puts[:4]


@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_without_onsets_the_flag_changes_nothing(nae, ref, n_fft, lock):
    """a signal without onsets: the flagged call's phases and samples are the unflagged call's bit for bit (at unlocked 1024 against the
    unflagged call on the size-generic kernels, debug key pv_any = 1, which the flagged call runs; locked against the locked call)"""
    ch, rate, pitch = 2, 1.0, 2 ** (3 / 12)
    x = steady(60000, ch)
    assert not pv_ref.onsets(ref, x, ch, rate, pitch, n_fft).any()
    res = {}
    for tr in (False, True):
        with nae.Context(0) as c:
            c.debug_set("pv_tile", 16)
            if n_fft == 1024 and not tr and not lock:
                c.debug_set("pv_any", 1)
            res[tr] = (tile_phases(c, nae, x, ch, rate, pitch, n_fft, transients=tr, lock=lock)[0],
                       block(c, nae, x, ch, rate, pitch, n_fft, transients=tr, lock=lock))
    assert np.array_equal(res[False][0], res[True][0])
    assert same_bits(res[False][1], res[True][1])


def test_error_codes(ctx, nae):
    """_n / _formant accept 4 at every size and 4 | 1 (the lock) at 1024; 4 | 1 at another size is NAE_ERR_UNSUPPORTED; 2 and 4 | 2 are
    NAE_ERR_INVALID; the _ex entries reject 4 with NAE_ERR_INVALID"""
    lib = ctx.lib
    L, ch = 4096, 2
    d_x, d_o = ctx.empty(L * ch), ctx.empty(2 * L * ch)
    src, dst = nae.Sig.interleaved(d_x.ptr, L, ch), nae.Sig.interleaved(d_o.ptr, 2 * L, ch)
    h = C.c_void_p()
    nt, tf = C.c_size_t(), C.c_size_t()
    buf = np.zeros(64 * 2049 * ch, np.int32)

    def all5(flags, n_fft):
        rc = [lib.nae_stretch_block_n_f32(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, C.byref(dst)),
              lib.nae_stretch_create_n(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, C.byref(h))]
        if rc[1] == 0:
            assert lib.nae_stretch_destroy(h) == 0
        rc.append(lib.nae_debug_pv_tile_phase_n(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size,
                                                C.byref(nt), C.byref(tf)))
        rc.append(lib.nae_stretch_block_formant_f32(ctx.h, 1.0, 1.2, flags, n_fft, 8, C.byref(src), L, ch, 1, C.byref(dst)))
        rc.append(lib.nae_stretch_create_formant(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, 8, C.byref(h)))
        if rc[4] == 0:
            assert lib.nae_stretch_destroy(h) == 0
        return tuple(rc)

    for n_fft in SIZES:
        assert all5(TR, n_fft) == (0,) * 5, n_fft
        assert all5(TR | 1, n_fft) == ((0,) * 5 if n_fft == 1024 else (-2,) * 5), n_fft   # else NAE_ERR_UNSUPPORTED
        assert all5(2, n_fft) == (-1,) * 5, n_fft                          # NAE_ERR_INVALID
        assert all5(TR | 2, n_fft) == (-1,) * 5, n_fft
    assert lib.nae_stretch_block_ex_f32(ctx.h, 1.0, 1.2, TR, C.byref(src), L, ch, 1, C.byref(dst)) == -1
    assert lib.nae_stretch_create_ex(ctx.h, 48000, ch, 1.0, 1.2, TR, C.byref(h)) == -1
    assert lib.nae_debug_pv_tile_phase_ex(ctx.h, 1.0, 1.2, TR, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size, C.byref(nt), C.byref(tf)) == -1
    d_x.free(); d_o.free()


def test_flag_without_vocoder_is_a_no_op(ctx, nae):
    """rate 2, pitch 1 (the transposer alone) and rate 1, pitch 1 (a wire): the flagged call is the unflagged one bit for bit"""
    x = orc.fill_uniform(30000 * 2, 23)
    for rate, pitch in ((2.0, 1.0), (1.0, 1.0)):
        assert same_bits(block(ctx, nae, x, 2, rate, pitch, 2048), block(ctx, nae, x, 2, rate, pitch, 2048, transients=False))


def test_host_graph_pitch_node_transients(tmp_path):
    """source -> Pitch_modifier {"pitch": 3, "fft_size": 2048, "transients": true} -> sink through the fiber runner equals the flagged block
    call bit for bit and differs from the unflagged one; the same with {"pitch": 3, "phase_lock": true, "transients": true} at 1024"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    for mode in (["gpu", "transients"], ["gpu", "transients", "lock"]):
        r = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "HOST PV NODE OK " + " ".join(mode) in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def one_sided(on):
    """the frames with an onset in the left channel only, and in the right only, of verdicts [frames, 2]"""
    return np.nonzero(on[:, 0] & ~on[:, 1])[0], np.nonzero(on[:, 1] & ~on[:, 0])[0]


@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_channels_decide_on_their_own(nae, ref, n_fft, lock):
    """a stereo stream whose channels have onsets at different frames (asserted on the statement): both channels' phases are bit-exact at tiles
    of 1, 3, 16 and 64 frames, each channel's are the statement's of that channel run as mono, and the GPU's mono run of a channel gives
    the stereo run's phases of it.  A wave that took the other channel's high(f - 1), P_{f-1} or reset mark would fail here and nowhere
    else: in every other unlinked stereo input of this file the channels decide alike."""
    L = 30000 * n_fft // 1024
    x = scene(L, seed=30)
    for rate, pitch in PAIRS:
        left, right = one_sided(pv_ref.onsets(ref, x, 2, rate, pitch, n_fft))
        assert left.size and right.size, (rate, left, right)
        qs = pv_ref.synth_phase(ref, x, 2, rate, pitch, n_fft, lock, transients=True)
        monos = [np.ascontiguousarray(x[c2::2]) for c2 in range(2)]
        for c2 in range(2):
            assert np.array_equal(qs[:, c2], pv_ref.synth_phase(ref, monos[c2], 1, rate, pitch, n_fft, lock, transients=True)[:, 0]), c2
        for tile in (1, 3, 16, 64):
            with nae.Context(0) as c:
                c.debug_set("pv_tile", tile)
                got, t = tile_phases(c, nae, x, 2, rate, pitch, n_fft, lock=lock)
                alone = [tile_phases(c, nae, m, 1, rate, pitch, n_fft, lock=lock)[0] for m in monos] if tile == 16 else None
            assert t == tile
            check_tiles(got, tile, qs, 2)
            if alone:
                assert np.array_equal(alone[0][0, 0], got[0, 0]) and np.array_equal(alone[1][0, 0], got[0, 1]), (rate, tile)


def batch_of(n, L, ch):
    """n different streams of the scene (mono: its left channel), [n][L * ch]"""
    xs = [scene(L, seed=30 + i) for i in range(n)]
    return xs if ch == 2 else [np.ascontiguousarray(x[0::2]) for x in xs]


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_batch_streams_equal_their_lone_runs(ctx, nae, ref, n_fft, lock, ch):
    """a batch of five different streams, unlinked: every stream's output is its lone run's bit for bit, and the batch's integer phases
    (debug_pv_tile_phase with n_streams = 5) are every stream's statement; then at 16-frame tiles a batch of one stream more than a
    workgroup has waves, its records so many that workgroups hold waves of two streams: the same two bars.  No two streams have the same
    onsets (asserted), so a wave that read P_{f-1}, high(f - 1) or a record's reset mark of the neighbouring stream would show."""
    rate, pitch = 1.0, 2 ** (-7 / 12)

    def check(c, n, L, tile):
        xs = batch_of(n, L, ch)
        sets = [frozenset(map(tuple, np.argwhere(pv_ref.onsets(ref, x, ch, rate, pitch, n_fft)))) for x in xs]
        assert len(set(sets)) == n and all(sets)
        got = block(c, nae, np.concatenate(xs), ch, rate, pitch, n_fft, lock=lock, n_streams=n).reshape(n, -1)
        phases, t = tile_phases(c, nae, np.concatenate(xs), ch, rate, pitch, n_fft, lock=lock, n_streams=n)
        assert t == tile and phases.shape[0] == n
        for i, x in enumerate(xs):
            assert same_bits(np.ascontiguousarray(got[i]), block(c, nae, x, ch, rate, pitch, n_fft, lock=lock)), (n, tile, i)
            check_tiles(phases, tile, pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock, transients=True), ch, s=i)

    check(ctx, 5, 30000 * n_fft // 1024, 64)
    # five 16-frame tiles: 5 or 10 records a stream (wave w of a launch works on record w), no multiple of the 8, 7 or 3 waves of WG_WAVES
    L = 27000 * n_fft // 1024
    waves = WG_WAVES[n_fft, lock]
    records = (nae.Context.stretch_plan(rate, pitch, L, n_fft).frames + 15) // 16 * ch
    assert records in (5, 10) and records % waves, "a workgroup ends inside a stream"
    with nae.Context(0) as c:
        c.debug_set("pv_tile", 16)
        check(c, waves + 1, L, 16)


@pytest.mark.parametrize("tempo", RANGE_TEMPOS, ids=["0.26", "3.9", "8", "16", "1-64"])
@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_transients_over_the_tempo_range(ctx, nae, ref, n_fft, lock, tempo):
    """tempo 0.26, 3.9, 8, 16 and 1/64, each with the transposer off, behind the vocoder (0.5) and in front of it (3), on the stereo inputs
    of pv_gpu.range_case: placed clicks above tempo 1/2, hard bursts at 0.26, and at 1/64 clicks of height 4096 in digital silence.  (At
    1/64 the analysis hop is N/256 samples: nothing within full scale fired in the statement, these clicks do, so the rows test the resets
    like the others and not only that the flag changes nothing.)  In every row the statement has onsets in the left channel only and in the
    right only (tests/test_pv_transient_cpu.py::test_range_rows_fire_in_one_channel_only).  Bars: the integer phases bit-exact at tiles of 16
    frames and of 1, the samples within 1e-4 relative RMS of the flagged statement, the transient kernels ran, and at 3 the transposer ran
    first."""
    for rho in RANGE_RHOS:
        x, L, rate, pitch = range_case(nae, n_fft, tempo, rho)
        left, right = one_sided(pv_ref.onsets(ref, x, 2, rate, pitch, n_fft))
        assert left.size and right.size, (rho, left, right)
        qs = pv_ref.synth_phase(ref, x, 2, rate, pitch, n_fft, lock, transients=True)
        for tile in (16, 1):
            with nae.Context(0) as c:
                c.debug_set("pv_tile", tile)
                got, t = tile_phases(c, nae, x, 2, rate, pitch, n_fft, lock=lock)
            assert t == tile
            check_tiles(got, tile, qs, 2)
        got, launched = profiled(ctx, block, ctx, nae, x, 2, rate, pitch, n_fft, lock=lock)
        want = pv_ref.stretch(ref, x, 2, rate, pitch, n_fft, lock, transients=True)
        assert got.size == want.size and np.isfinite(got).all()
        e = rel_rms(got, want)
        print(f"N={n_fft} lock={lock} tempo {tempo:.4g} rho {rho}: L {L} frames {qs.shape[0]} rel RMS {e:.3g}")
        assert e <= TOL, (rho, e)
        kinds = ("pvlock_map", "pvlock_synth") if lock else ("pv_any_phase", "pv_any_synth")
        for kind in kinds:
            assert any(k.startswith(kind) and k.endswith("transient_kernel") for k in launched), (kind, launched)
        pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
        assert pl.rs_first == (rho > 1) and pl.rs_on == (rho != 1), (rho, pl.rs_first, pl.rs_on)
        assert any(k.startswith("resample") for k in launched) == (rho != 1), launched


@pytest.mark.parametrize("n_fft,lock", ROUTES)
def test_phase_in_front_of_a_single_tile_is_zero(nae, n_fft, lock):
    """a stream of one tile has no record for pass 1 to write (pass 3 starts it from zero by itself), so debug_pv_tile_phase must say zero
    whatever an earlier call left in the phase workspace: after a batch's block call at 16-frame tiles it gave that call's records
    (tests/tools/fuzz_pv_options.py found it)"""
    L, rate, pitch = 30000 * n_fft // 1024, 1.0, 2 ** (-7 / 12)
    xs = batch_of(3, L, 2)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", 16)
        block(c, nae, np.concatenate(xs), 2, rate, pitch, n_fft, lock=lock, n_streams=3)
        c.debug_set("pv_tile", 1000000)
        got, t = tile_phases(c, nae, np.concatenate(xs), 2, rate, pitch, n_fft, lock=lock, n_streams=3)
    assert got.shape[:3] == (3, 2, 1) and not got.any()
