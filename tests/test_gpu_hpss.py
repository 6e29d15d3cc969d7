"""K21 separation on the GPU, bit for bit against the CPU statement (tests/hpss_ref/ref_hpss.c): every frame size, both masks, mono and
stereo, one and three streams, the spans at their edges, the lengths around the hop, a strided view, every tiling, the library's own tile pick
over 300 blocks, the key ring wrapped twice at every size, the streaming handle in ragged puts, in a long stream with deferred receives, in
pieces and into device memory, two handles on one context and on two, batches of more items than each size holds resident waves and than the
chip holds waves at all, a non-finite sample, powers on the subnormal grid, digital silence, the error codes, the host node
(tests/hpss_ref/host_hpss_node.cpp) and a seeded run of tests/tools/fuzz_hpss.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hpss_ref
import node_harness
from block_gpu import bits, each_stream, mismatch, statement
from hpss_gpu import gpu_hpss, hpss_stream, lib_params
from test_hpss_cpu import BAD, quiet, reach

pytestmark = pytest.mark.gpu

N0, H0 = 512, 128
SPANS = ((0, 0), (1, 8), (8, 1), (8, 8))
INVALID, UNSUPPORTED, STATE = -1, -2, -5
RESIDENT = {512: 8, 1024: 5, 2048: 3, 4096: 1}    # Hp<N>::kResident of kernels_hpss.hip: the waves a CU holds
MIN_TILE, N_CU = 64, 256                           # NAE_HPSS_MIN_TILE; the MI355X's compute units


@pytest.fixture(scope="module")
def ref():
    return statement(hpss_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("hpss_ref/host_hpss_node.cpp", str(tmp_path_factory.mktemp("host_hpss_gpu")))


def wander(rng, n_streams, n, ch, n_fft=N0):
    """noise whose level wanders +-14 dB around 1 with a period of three frames, another phase per stream and channel: neither median wins everywhere"""
    return hpss_ref.wander(rng, n_streams, n, ch, period=3.0 * n_fft)


@pytest.mark.parametrize("mask", ("soft", "hard"))
@pytest.mark.parametrize("n_fft", hpss_ref.SIZES)
def test_block_call(nae, ctx, ref, n_fft, mask):
    """one sample, the hop's edge, five blocks and a rest — the shortest that put the zero frames, the drain and a ragged last block in play —
    at every pair of spans; mono is the unit-stride kernel, interleaved stereo the strided one"""
    H = n_fft // 4
    rng = np.random.default_rng(n_fft + (mask == "hard"))
    harmonic = total = 0
    for tn, fn in SPANS:
        p = hpss_ref.params(n_fft, tn, fn, int(mask == "hard"), 0.9, 0.125)
        for in_len in (1, H - 1, H, H + 1, 5 * H + 7):
            for ch, n_streams in ((1, 1), (2, 3), (1, 3), (2, 1)):
                x = wander(rng, n_streams, in_len, ch, n_fft)
                want = hpss_ref.run_streams(ref, p, x)
                got = gpu_hpss(nae, ctx, p, x)
                assert np.array_equal(bits(got), bits(want)), (tn, fn, in_len, ch, n_streams, mismatch(got, want))
        _, _, hq, pq, _ = hpss_ref.run(ref, p, x[0], detail=True)
        harmonic += int((hq >= pq).sum())
        total += hq.size
    assert 0 < harmonic < total, f"each median wins somewhere: Hq >= Pq at {harmonic} of {total} bins"


@pytest.mark.parametrize("n_fft", (512, 2048))
def test_strided_views(nae, ctx, ref, n_fft):
    """planar to interleaved and back with channel padding, a gap between the streams and an odd offset: the kUnit = false instantiation"""
    rng = np.random.default_rng(5 + n_fft)
    p = hpss_ref.params(n_fft, 3, 5, 0, 1.0, 0.0)
    x = wander(rng, 3, 5 * (n_fft // 4) + 7, 2, n_fft)
    want = hpss_ref.run_streams(ref, p, x)
    for sl, dl in (("p", "i"), ("i", "p"), ("i", "i"), ("p", "p")):
        got = gpu_hpss(nae, ctx, p, x, sl, dl, gap=3 if sl == "p" else 0, chan_pad=5, offset=1)
        assert np.array_equal(bits(got), bits(want)), (sl, dl, mismatch(got, want))


@pytest.mark.parametrize("tn,fn,mask", ((8, 8, 0), (2, 3, 1), (0, 4, 0)))
def test_every_tiling_gives_the_same_bits(nae, ctx, ref, tn, fn, mask):
    """11 blocks cut into tiles of 1, 2 and 3 blocks and by the library's pick: the key front starts cold Tn frames early at every tile boundary"""
    rng = np.random.default_rng(11 + tn)
    p = hpss_ref.params(N0, tn, fn, mask, 1.0, 0.0)
    x = wander(rng, 2, 11 * H0 - 5, 2)
    want = hpss_ref.run_streams(ref, p, x)
    try:
        for tile in (1, 2, 3, 0):
            ctx.debug_set("hpss_tile", tile)
            got = gpu_hpss(nae, ctx, p, x)
            assert np.array_equal(bits(got), bits(want)), (tile, mismatch(got, want))
    finally:
        ctx.debug_set("hpss_tile", 0)


@pytest.mark.parametrize("n_fft,tn", ((512, 8), (512, 0), (1024, 2)))
def test_handle_equals_the_block_call(nae, ctx, ref, n_fft, tn):
    """ragged puts — one sample, the hop less and plus one — from host and device memory, then the flush: the block call's bits; `available`
    after every put is floor((total - (Tn + 3) H) / H) H, never below zero (hpss_stream asserts it); a put after the flush is NAE_ERR_STATE
    (block_gpu.flushed asserts it)"""
    H = n_fft // 4
    rng = np.random.default_rng(n_fft + tn)
    p = hpss_ref.params(n_fft, tn, 4, 0, 1.0, 0.25)
    x = wander(rng, 1, 14 * H + 9, 2, n_fft)
    want = hpss_ref.run_streams(ref, p, x)[0]
    block = gpu_hpss(nae, ctx, p, x)[0]
    assert np.array_equal(bits(block), bits(want))
    for puts, device in (((1, H - 1, H + 1, 1, 3 * H + 5, 7), False), ((H + 1, 1, H - 1), True), ((H,), (True, False)), ((15 * H,), False)):
        got = hpss_stream(nae, ctx, p, x[0], puts, device)
        assert got.shape == block.shape and np.array_equal(bits(got), bits(block)), (puts, device)


def both_medians_win(ref, p, x, streams):
    """on the statement's detail, before the device is touched: over the streams named, Hq >= Pq at some bins and not at others"""
    harmonic = total = 0
    for i in streams:
        _, _, hq, pq, _ = hpss_ref.run(ref, p, x[i], detail=True)
        harmonic += int((hq >= pq).sum())
        total += hq.size
    assert 0 < harmonic < total, f"each median wins somewhere: Hq >= Pq at {harmonic} of {total} bins"


@pytest.mark.parametrize("n_fft,n_streams,tn", ((512, 1100, 8), (512, 1100, 2), (1024, 650, 2), (2048, 390, 2), (4096, 130, 2)))
def test_batch_beyond_the_resident_waves(nae, ctx, ref, n_fft, n_streams, tn):
    """1100 stereo streams of three blocks at N = 512: 2200 waves, more than the 256 CUs hold at 8 each, so the launch list has a second round;
    650, 390 and 130 at N = 1024, 2048 and 4096: 1300, 780 and 260 waves against the 1280, 768 and 256 that 5, 3 and 1 per CU make, in
    workgroups of 5, 3 and 1 waves (the item of a wave is blockIdx.x * kWaves + its index); every stream is compared.  Three blocks are six
    frames: with Tn = 8 eleven of a window's seventeen keys are the zeros outside the signal, Hq is 0 at every bin and with g_p = 0 the
    output is zero — the first case, kept as it was, compares the launch and nothing of the mask.  The others run Tn = 2, where the windows
    of the inner frames lie inside the signal and each median wins somewhere"""
    H = n_fft // 4
    assert 2 * n_streams > 256 * RESIDENT[n_fft]
    rng = np.random.default_rng(2 * n_streams)
    p = hpss_ref.params(n_fft, tn, 8, 0, 1.0, 0.0)
    x = wander(rng, n_streams, 2 * H + 3, 2, n_fft)
    if tn < 3:
        both_medians_win(ref, p, x, (0, 1, n_streams - 1))
    want = each_stream(lambda i: hpss_ref.run(ref, p, x[i]), len(x))
    assert np.any(want) == (tn < 3)
    got = gpu_hpss(nae, ctx, p, x)
    assert not mismatch(got, want), mismatch(got, want)


def test_batch_overfills_the_chip(nae, ctx, ref):
    """4099 stereo streams (a prime) of three blocks at N = 512, hard mask, Tn = 2: 8198 waves, more than 256 CUs x 32.  Stream s carries
    signal s mod 61 of 61 seeded signals (61 divides no count of waves per workgroup, CU or chip); the statement runs on each of the 61 and
    every stream is compared"""
    base = wander(np.random.default_rng(4099), 61, 2 * H0 + 3, 2)
    p = hpss_ref.params(N0, 2, 8, 1, 1.0, 0.0)
    both_medians_win(ref, p, base, (0, 1, 60))
    want61 = each_stream(lambda i: hpss_ref.run(ref, p, base[i]), 61)
    pick = np.arange(4099) % 61
    message = mismatch(gpu_hpss(nae, ctx, p, base[pick]), want61[pick])
    assert not message, message


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig, out_sig = nae.Sig(d.ptr, 0, 1, 1), nae.Sig(d.at(32), 0, 1, 1)
    good = hpss_ref.params()

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(out_sig), n=16, streams=1):
        return lib.nae_hpss_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    def create(p, ch=2, out=True):
        h = C.c_void_p()
        rc = lib.nae_hpss_create(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, ch, C.byref(h) if out else None)
        assert rc == 0 or not h.value
        if h.value:
            lib.nae_hpss_destroy(h)
        return rc

    def message():
        return lib.nae_last_error(ctx.h).decode()

    assert block(good) == 0 and create(good) == 0
    assert block(None) == INVALID and "null pointer" in message()
    assert block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID and "channel count" in message()
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    top = float(np.float32(10.0 ** (12.0 / 20.0)))
    for field, values in (("time_span", (-1, 9)), ("freq_span", (-1, 9)), ("hard", (-1, 2)), ("gain_h", (-0.5, np.nextafter(np.float32(top), np.float32(9)), np.nan, np.inf)),
                          ("gain_p", (-0.5, 4.0, np.nan, np.inf))):
        for v in values:
            p = hpss_ref.params()
            setattr(p, field, v)
            assert block(p) == INVALID and field in message(), (field, v, message())
            assert block(p, n=0) == INVALID, "checked before the empty call returns"
            assert create(p) == INVALID, (field, v)
    for n_fft in (0, 256, 1000, 8192):
        assert block(hpss_ref.params(n_fft)) == UNSUPPORTED and "n_fft" in message() and create(hpss_ref.params(n_fft)) == UNSUPPORTED, n_fft
    assert block(hpss_ref.params(gain_h=0.0, gain_p=top, time_span=0, freq_span=8, hard=1)) == 0
    assert create(None) == INVALID and create(good, ch=3) == INVALID and create(good, out=False) == INVALID
    h = nae.Hpss(ctx, lib_params(nae, good), 1)
    h.put_host(np.zeros(5, np.float32))
    h.flush()
    assert h._fn("put_host")(h.h, np.zeros(1, np.float32).ctypes.data, 1) == STATE, "put after flush: NAE_ERR_STATE"
    assert h.available() == 5
    h.close()
    assert lib.nae_debug_set(ctx.h, b"hpss_tile", 5) == 0 and lib.nae_debug_set(ctx.h, b"hpss_tile", 0) == 0
    assert lib.nae_debug_set(ctx.h, b"hpss_tile", -1) == INVALID and lib.nae_debug_set(ctx.h, b"hpss_tiles", 1) == INVALID
    ctx.sync()
    d.free()


def test_host_node_graph(host):
    """source -> audio_separation -> sink with 1152-sample frames: the source's frames, sizes and pts; the block call's samples"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST HPSS OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------- tiles and the ring
def library_tile(n_fft, blocks, n_sc):
    """nae_pick_tile with max_tiles_down, in Python: as many tiles as one round of resident waves takes, at most floor(blocks / MIN_TILE), at
    least one -> (tiles, blocks per tile)"""
    n_tiles = max(1, min(-(-RESIDENT[n_fft] * N_CU // n_sc), blocks // MIN_TILE))
    tile = -(-blocks // n_tiles)
    return -(-blocks // tile), tile


@pytest.mark.parametrize("n_fft", (512, 4096))
def test_library_tile_pick(nae, ctx, ref, n_fft):
    """one stereo stream of 300 blocks less nine samples with hpss_tile = 0: the library's own pick cuts it into 4 tiles of 75 blocks, so three
    tiles start cold in the middle of the signal and every one wraps the ring four times.  The call is one launch of hpss_kernel (read from the
    context's profile as tests/test_gpu_launch_names.py does); the profile counts launches, not items, so the tile count itself is asserted by
    nae_pick_tile's arithmetic restated in Python, and NAE_HPSS_MIN_TILE is read from the header"""
    H = n_fft // 4
    spec = open(os.path.join(hpss_ref.ROOT, "include", "nae_dsp_spec.h")).read()
    assert any(line.split()[:3] == ["#define", "NAE_HPSS_MIN_TILE", str(MIN_TILE)] for line in spec.splitlines())
    x = wander(np.random.default_rng(300 + n_fft), 1, 300 * H - 9, 2, n_fft)
    assert library_tile(n_fft, 300, 2) == (4, 75)
    p = hpss_ref.params(n_fft, 8, 8, 0, 1.0, 0.0)
    both_medians_win(ref, p, x, (0,))
    want = hpss_ref.run_streams(ref, p, x)
    ctx.debug_set("hpss_tile", 0)
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        got = gpu_hpss(nae, ctx, p, x)
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    launches = {name: int(count) for name, (_, count) in ctx.prof_report().items()}
    assert launches == {"hpss_kernel": 1}, launches
    assert not mismatch(got, want), mismatch(got, want)


@pytest.mark.parametrize("tn", (8, 3))
@pytest.mark.parametrize("n_fft", hpss_ref.SIZES)
def test_ring_wraps_at_every_size(nae, ctx, ref, n_fft, tn):
    """two stereo streams of 41 blocks, planar to interleaved with channel padding.  With the library's tile (41 blocks are one tile) a wave
    synthesises 44 frames in a row: the ring's head comes back to slot 0 twice at Tn = 8 (17 slots) and six times at Tn = 3 (7 slots, the
    other ten rows padding).  With tiles of 20 blocks a tile border falls mid-ring and the next tile starts cold.  Both give the statement's bits"""
    H = n_fft // 4
    x = wander(np.random.default_rng(41 * n_fft + tn), 2, 40 * H + 7, 2, n_fft)
    p = hpss_ref.params(n_fft, tn, 8, 0, 1.0, 0.0)
    assert library_tile(n_fft, 41, 4) == (1, 41)
    both_medians_win(ref, p, x, (0, 1))
    want = hpss_ref.run_streams(ref, p, x)
    try:
        for tile in (0, 20):
            ctx.debug_set("hpss_tile", tile)
            got = gpu_hpss(nae, ctx, p, x, "p", "i", chan_pad=3)
            assert not mismatch(got, want), (tile, mismatch(got, want))
    finally:
        ctx.debug_set("hpss_tile", 0)


# ---------------------------------------------------------------------------------------------------- the handle
@pytest.fixture(scope="module")
def long_stream(nae, ctx, ref):
    """x[100 000, 2] (three times what a handle's FIFOs start with) at N = 512, Tn = 8: the block call's result, the statement's bits"""
    p = hpss_ref.params(N0, 8, 8, 0, 1.0, 0.0)
    x = wander(np.random.default_rng(100000), 1, 100000, 2)
    both_medians_win(ref, p, x, (0,))
    block = gpu_hpss(nae, ctx, p, x)[0]
    assert np.array_equal(bits(block), bits(hpss_ref.run_streams(ref, p, x)[0]))
    puts = tuple(int(k) for k in np.random.default_rng(9000).integers(1, 9001, 64))
    return p, x[0], block, puts


@pytest.mark.parametrize("drive", ("received after every put", "received after the flush"))
def test_handle_long_stream(nae, ctx, long_stream, drive):
    """100 000 frames through a handle in 64 seeded random puts of 1 ... 9000 frames (the last repeated), from the device and the host in
    turn, give the block call's bits: the input FIFO, which keeps Tn + 3 = 11 blocks, moves its live rest to the front again and again; with
    nothing received before the flush the output FIFO grows while all of it is live"""
    p, x, block, puts = long_stream
    got = hpss_stream(nae, ctx, p, x, puts, device=(True, False), defer=drive == "received after the flush")
    assert got.shape == block.shape and np.array_equal(bits(got), bits(block)), int(np.sum(bits(got) != bits(block)))


def test_handle_pieces_and_device_receive(nae, ctx, ref):
    """N = 1024, 14 blocks and a rest: received in pieces of 100 frames into host memory, and in pieces of 100 frames into device memory"""
    n_fft, H = 1024, 256
    p = hpss_ref.params(n_fft, 2, 4, 0, 1.0, 0.25)
    x = wander(np.random.default_rng(1409), 1, 14 * H + 9, 2, n_fft)
    both_medians_win(ref, p, x, (0,))
    want = hpss_ref.run_streams(ref, p, x)[0]
    got = hpss_stream(nae, ctx, p, x[0], (3 * H + 5, 1, 777), (False, True), piece=100)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), "pieces into host memory"
    d_out = ctx.array(np.zeros(100 * 2, np.float32))
    try:
        got = hpss_stream(nae, ctx, p, x[0], (len(x[0]),), True, d_out=d_out, piece=100)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), "pieces into device memory"
        got = hpss_stream(nae, ctx, p, x[0], (777,), (True, False), d_out=d_out, piece=100, defer=True)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), "deferred, in pieces into device memory"
    finally:
        d_out.free()


def test_two_handles_on_one_context_and_on_two(nae, ctx, ref):
    """two handles of different frame size, spans and mask fed in turn, on one context and on two: each gives its own statement's bits"""
    ps = [hpss_ref.params(512, 8, 8, 0, 1.0, 0.0), hpss_ref.params(2048, 1, 3, 1, 0.25, 1.0)]
    xs = [wander(np.random.default_rng(21 + k), 1, 9000 + 100 * k, 2, ps[k].n_fft)[0] for k in range(2)]
    want = [hpss_ref.run(ref, ps[k], xs[k]) for k in range(2)]
    other = nae.Context(0)
    try:
        for ctxs in ((ctx, ctx), (ctx, other)):
            hs = [nae.Hpss(ctxs[k], lib_params(nae, ps[k]), 2) for k in range(2)]
            parts = [[], []]
            try:
                for pos in range(0, max(len(x) for x in xs), 777):
                    for k in range(2):
                        if pos < len(xs[k]):
                            hs[k].put_host(xs[k][pos:pos + 777].reshape(-1))
                        if hs[k].available():
                            parts[k].append(hs[k].receive_host())
                for k in range(2):
                    hs[k].flush()
                    parts[k].append(hs[k].receive_host())
            finally:
                for h in hs:
                    h.close()
            for k in range(2):
                got = np.concatenate(parts[k]).reshape(-1, 2)
                assert got.shape == want[k].shape and np.array_equal(bits(got), bits(want[k])), (k, ctxs[1] is other)
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------- non-finite, subnormal, silence
NON_FINITE = [(N0, tn, mask, bad) for tn in (0, 1, 8) for mask in ("soft", "hard") for bad in BAD] + [(4096, 8, "soft", np.nan)]


@pytest.mark.parametrize("n_fft,tn,mask,bad", NON_FINITE)
def test_non_finite_sample_stays_local(nae, ctx, ref, n_fft, tn, mask, bad):
    """the contract of include/nae_gpu.h for a non-finite sample i, b = floor(i / H): outside [(b - Tn - 3) H, (b + Tn + 4) H) the stream-channel
    has the clean run's bits, and so have the other channel and the other stream everywhere; inside, wherever the statement run on the same
    input is finite the GPU has its bits, and wherever it is not (exactly [(b - 3) H, (b + 4) H), asserted here and in tests/test_hpss_cpu.py)
    the GPU is not finite either — NaN payloads are never compared; the call returns NAE_OK and the guard words stand (gpu_hpss checks both).
    Tiles of 5 blocks start in front of, inside and behind the reach"""
    H = n_fft // 4
    i = 20 * H + 5
    (lo, hi), (nlo, nhi) = reach(n_fft, tn, i)
    p = hpss_ref.params(n_fft, tn, 8, int(mask == "hard"), 1.0, 0.0)
    x = wander(np.random.default_rng(9), 2, 40 * H + 40, 2, n_fft)
    dirty_x = x.copy()
    dirty_x[0, i, 1] = bad
    assert 0 < lo and hi < x.shape[1]
    want = hpss_ref.run(ref, p, dirty_x[0])
    wild = ~np.isfinite(want[:, 1])
    assert np.array_equal(np.flatnonzero(wild), np.arange(nlo, nhi)) and np.all(np.isfinite(want[:, 0]))
    try:
        ctx.debug_set("hpss_tile", 5)
        clean = gpu_hpss(nae, ctx, p, x, "p", "p", chan_pad=3)
        got = gpu_hpss(nae, ctx, p, dirty_x, "p", "p", chan_pad=3)
    finally:
        ctx.debug_set("hpss_tile", 0)
    assert np.array_equal(bits(clean[0]), bits(hpss_ref.run(ref, p, x[0]))), "the clean run is the statement's"
    assert np.array_equal(bits(got[0, :lo]), bits(clean[0, :lo])), "samples in front of the sample's reach changed"
    assert np.array_equal(bits(got[0, hi:]), bits(clean[0, hi:])), "samples behind the sample's reach changed"
    assert np.array_equal(bits(got[0, :, 0]), bits(clean[0, :, 0])), "the other channel changed"
    assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"
    assert np.array_equal(bits(got[0, ~wild, 1]), bits(want[~wild, 1])), "where the statement is finite: its bits"
    assert not np.any(np.isfinite(got[0, wild, 1])), "where the statement is not finite the GPU is not finite either"


@pytest.mark.parametrize("mask", ("soft", "hard"))
@pytest.mark.parametrize("n_fft", hpss_ref.SIZES)
def test_subnormal_powers(nae, ctx, ref, n_fft, mask):
    """wandering noise around 1e-20, one mono and one stereo stream, spans 8: the samples are normal f32, the powers of the bins are subnormal,
    and a key is the upper half of the power's bits — a multiply, an add or a load that flushed subnormals to zero would change decisions, not
    roundings.  Bit for bit against the statement; tests/test_hpss_cpu.py::test_subnormal_powers asserts on the statement that the keys of
    this very signal lie on the subnormal grid.  Not compared with the float64 restatement: the band of hpss_ref.near_boundary is relative to
    the power and means nothing where the keys' cells are a fixed 2^-133 wide"""
    p = hpss_ref.params(n_fft, 8, 8, int(mask == "hard"), 1.0, 0.0)
    for ch in (1, 2):
        x = quiet(n_fft, ch)
        want = hpss_ref.run_streams(ref, p, x)
        assert np.any(want)
        got = gpu_hpss(nae, ctx, p, x)
        assert not mismatch(got, want), (ch, mismatch(got, want))


@pytest.mark.parametrize("mask", ("soft", "hard"))
def test_silence_and_bursts(nae, ctx, ref, mask):
    """all-zero input gives all-zero output (s == 0: the soft mask is 0.5, the hard one 1, the spectrum zero); one hop block of noise in every
    twelve with exact zeros between, at N = 512 and N = 2048: on the statement's detail some frames have Hq = Pq = 0 at every bin and others
    have not, and the GPU has the statement's bits"""
    hard = int(mask == "hard")
    z = np.zeros((2, 5 * H0 + 7, 2), np.float32)
    for p in (hpss_ref.params(N0, 8, 8, hard, 1.0, 0.0), hpss_ref.params(N0, 0, 3, hard, 0.5, 2.0)):
        assert not np.any(gpu_hpss(nae, ctx, p, z)), "silence in, silence out"
    for n_fft in (512, 2048):
        H = n_fft // 4
        p = hpss_ref.params(n_fft, 8, 8, hard, 1.0, 0.25)
        x = hpss_ref.bursts(np.random.default_rng(12 + n_fft), 40 * H + 9, 2, n_fft, on=1, period=12)[None]
        want, _, hq, pq, _ = hpss_ref.run(ref, p, x[0], detail=True)
        silent = np.all((hq == 0) & (pq == 0), axis=2)
        assert silent.any() and not silent.all(), "frames of nothing but zeros, and others"
        got = gpu_hpss(nae, ctx, p, x)
        assert not mismatch(got, want[None]), (n_fft, mismatch(got, want[None]))


def test_fuzz_hpss_seeded(nae, ctx):
    """a seeded run of tests/tools/fuzz_hpss.py: sizes, spans, masks, levels, lengths, tiles, views and put patterns; tests/test_hpss_cpu.py
    pins the edges the seed reaches"""
    sys.path.insert(0, os.path.join(hpss_ref.ROOT, "tests", "tools"))
    import fuzz_hpss
    assert fuzz_hpss.main(cases=fuzz_hpss.SEEDED[0], seed=fuzz_hpss.SEEDED[1], ctx=ctx, nae=nae) == fuzz_hpss.SEEDED[0]
