"""K9 FIR filter on the GPU: nae_fir_block_f32 bit for bit against the CPU statement (tests/fir_ref/ref_fir.c) at the smallest shapes that reach
every edge, every tiling, a NaN's reach, the streaming handle, the error codes, and the host node (tests/fir_ref/host_fir_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fir_ref
import node_harness
from block_gpu import CONFIGS, bits, noise, statement
from fir_gpu import MIN_TILE, WAVES, fir_stream, gpu_fir, pick_tile, ref_fir, ref_fir_flushed

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ref():
    return statement(fir_ref)


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_block_bits_equal_the_statement(nae, ctx, ref, n_fft):
    """every L and in_len edge at this size, the view / channel / stream configurations taken in turn so that each is met with several edges"""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft)
    k = 0
    for L in (1, 2, B, B + 1):
        taps = rng.uniform(-1, 1, L).astype(np.float32)
        for in_len in (1, B - 1, B, B + 1, 3 * B + 7):
            ch, n_streams, sl, dl, shared = CONFIGS[k % len(CONFIGS)]
            k += 1
            x = noise(rng, n_streams, in_len, ch, shared)
            got = gpu_fir(nae, ctx, taps, n_fft, x, sl, dl, shared)
            want = ref_fir(ref, taps, n_fft, x)
            assert np.array_equal(bits(got), bits(want)), (n_fft, L, in_len, ch, n_streams, sl, dl, shared)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"ch{c[0]}-s{c[1]}-{c[2]}{c[3]}{'-shared' if c[4] else ''}")
def test_block_bits_in_every_view(nae, ctx, ref, cfg):
    """mono / stereo, 1 / 3 streams, interleaved and planar views on both sides, a shared source: more than one block and a partial one"""
    ch, n_streams, sl, dl, shared = cfg
    n_fft, B = 512, 256
    rng = np.random.default_rng(77)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = noise(rng, n_streams, 3 * B + 7, ch, shared)
    got = gpu_fir(nae, ctx, taps, n_fft, x, sl, dl, shared)
    assert np.array_equal(bits(got), bits(ref_fir(ref, taps, n_fft, x)))


def test_pick_equals_explicit_size(nae, ctx):
    rng = np.random.default_rng(9)
    x = noise(rng, 2, 2500, 2)
    for L, n_fft in ((1, 512), (257, 512), (258, 1024), (513, 1024), (514, 2048), (1026, 4096), (2049, 4096)):
        taps = rng.uniform(-1, 1, L).astype(np.float32)
        assert nae.Context.fir_pick_n_fft(L) == n_fft
        assert np.array_equal(bits(gpu_fir(nae, ctx, taps, 0, x)), bits(gpu_fir(nae, ctx, taps, n_fft, x))), L


@pytest.mark.parametrize("n_fft", (512, 4096))
def test_every_tiling_gives_the_same_bits(nae, ctx, ref, n_fft):
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 1)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = noise(rng, 2, 7 * B + 5, 2)
    own = gpu_fir(nae, ctx, taps, n_fft, x)
    assert np.array_equal(bits(own), bits(ref_fir(ref, taps, n_fft, x)))
    try:
        for tile in (1, 2, 3):
            ctx.debug_set("fir_tile", tile)
            assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x)), bits(own)), tile
            assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x, "p", "p")), bits(own)), tile
    finally:
        ctx.debug_set("fir_tile", 0)


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_automatic_tiles(nae, ctx, ref, n_fft):
    """fir_tile = 0 on signals long enough for nae_pick_fir_tile to cut them: block counts on both sides of one, two and several tiles, the last
    tile ending in a partial block, 1 and 6 stream-channels.  At 256 CUs the rule's first term (a round of resident waves) is at least 128 tiles
    here, so blocks / MIN_TILE alone decides, as it does for any CU count from 16 on."""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 2)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    ctx.debug_set("fir_tile", 0)
    for blocks in (8, 9, 16, 17, 41, 67):
        for ch, n_streams in ((1, 1), (2, 3)):
            tile, n_tiles = pick_tile(n_fft, blocks, ch * n_streams)
            assert tile >= MIN_TILE and (n_tiles > 1) == (blocks >= 16), (blocks, tile, n_tiles)
            x = noise(rng, n_streams, blocks * B - 5, ch)
            got = gpu_fir(nae, ctx, taps, n_fft, x)
            assert np.array_equal(bits(got), bits(ref_fir(ref, taps, n_fft, x))), (blocks, ch, n_streams, tile, n_tiles)
    assert pick_tile(n_fft, 41, 1) == (9, 5) and pick_tile(n_fft, 67, 6) == (9, 8)


@pytest.mark.parametrize("layout", ("i", "p"))
@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_a_full_and_a_partial_workgroup(nae, ctx, ref, n_fft, layout):
    """5 stereo streams are 10 one-tile items against 8, 8, 7 and 3 waves per workgroup: a full workgroup and a partly filled last one at every
    size; NaN between the source's streams"""
    B = n_fft // 2
    assert 10 > WAVES[n_fft] and 10 % WAVES[n_fft]
    rng = np.random.default_rng(n_fft + 3)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = noise(rng, 5, 2 * B + 3, 2)
    ctx.debug_set("fir_tile", 0)
    got = gpu_fir(nae, ctx, taps, n_fft, x, layout, layout, gap=37)
    assert np.array_equal(bits(got), bits(ref_fir(ref, taps, n_fft, x)))


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_forced_tiles_over_several_workgroups(nae, ctx, ref, n_fft):
    """7 blocks of 5 stereo streams in tiles of 1, 2, 3 and 100 blocks (more than there are): 70, 40, 30 and 10 items, so tiles of one
    stream-channel lie in different workgroups and the last workgroup is partly filled"""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 4)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = noise(rng, 5, 7 * B - 5, 2)
    want = bits(ref_fir(ref, taps, n_fft, x))
    try:
        for tile in (1, 2, 3, 100):
            ctx.debug_set("fir_tile", tile)
            assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x, gap=37)), want), tile
            assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x, "p", "p", gap=37)), want), tile
    finally:
        ctx.debug_set("fir_tile", 0)


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_unit_stride_at_odd_addresses(nae, ctx, ref, n_fft):
    """the 8-byte accesses of the unit-stride kernel at 4-byte alignment, loads and stores: mono and planar stereo with both bases one float
    past an allocation's start and an odd channel stride, so that channels 0 and 1 and streams 0 and 1 start at addresses of both parities"""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 5)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    n = 3 * B + 7
    assert n % 2 == 1, "n and n + PAD are the planar channel strides"
    for ch, layout in ((1, "i"), (1, "p"), (2, "p")):
        x = noise(rng, 2, n, ch)
        got = gpu_fir(nae, ctx, taps, n_fft, x, layout, layout, gap=1, offset=1)
        assert np.array_equal(bits(got), bits(ref_fir(ref, taps, n_fft, x))), (ch, layout)


def test_nan_reaches_only_the_blocks_that_read_it(nae, ctx):
    n_fft, B = 512, 256
    rng = np.random.default_rng(11)
    taps = rng.uniform(-1, 1, 65).astype(np.float32)
    x = noise(rng, 2, 5 * B + 3, 2)
    clean = gpu_fir(nae, ctx, taps, n_fft, x)
    p = 2 * B + 10                       # read by blocks 2 (its new half) and 3 (its carried half)
    x[1, p, 0] = np.nan
    got = gpu_fir(nae, ctx, taps, n_fft, x)
    hit = np.zeros(x.shape, bool)
    hit[1, 2 * B:4 * B, 0] = True
    assert np.all(np.isnan(got[hit])), "every sample of the two blocks is NaN"
    assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), "no other output word changes"
    try:
        ctx.debug_set("fir_tile", 1)     # the block after the NaN starts a tile: it reads the sample through the tile head
        assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x)), bits(got))
    finally:
        ctx.debug_set("fir_tile", 0)


@pytest.fixture(scope="module")
def handle_case(nae, ctx, ref):
    """N = 1024, L = 513, 5000 stereo frames: the block call's bits and the statement on the zero-extended input, computed once"""
    rng = np.random.default_rng(21)
    L, in_len = 513, 5000
    taps = rng.uniform(-1, 1, L).astype(np.float32)
    x = noise(rng, 1, in_len, 2)
    block = gpu_fir(nae, ctx, taps, 1024, x)[0]
    ext = np.concatenate([x, np.zeros((1, L - 1, 2), np.float32)], 1)
    tail = ref_fir(ref, taps, 1024, ext)[0]
    block.setflags(write=False)
    tail.setflags(write=False)
    return taps, x[0], block, tail


@pytest.mark.parametrize("chunk", (1, 7, 512, 1152))
def test_handle_equals_the_block_call_for_any_chunking(nae, ctx, handle_case, chunk):
    taps, x, block, tail = handle_case
    in_len, L = x.shape[0], taps.size
    h = nae.Fir(ctx, taps, 2, 1024)
    try:
        parts = []
        for pos in range(0, in_len, chunk):
            h.put_host(x[pos:pos + chunk].reshape(-1))
            if h.available() >= 2000:
                parts.append(h.receive_host())
        assert sum(p.size for p in parts) // 2 + h.available() == in_len // 512 * 512, "whole blocks come out as they fill"
        h.flush()
        h.flush()                                          # a second flush changes nothing
        parts.append(h.receive_host())
        assert h.available() == 0
        got = np.concatenate(parts).reshape(-1, 2)
        assert got.shape[0] == in_len + L - 1
        assert np.array_equal(bits(got[:in_len]), bits(block)), "the first in_len frames are the block call's"
        assert np.array_equal(bits(got), bits(tail)), "and the tail is the statement on the zero-extended input"
        assert ctx.lib.nae_fir_put_host(h.h, x.ctypes.data, 1) == -5, "put after flush: NAE_ERR_STATE, as the other handles"
    finally:
        h.close()


def test_handle_device_put_and_mono(nae, ctx, ref):
    rng = np.random.default_rng(31)
    taps = rng.uniform(-1, 1, 2).astype(np.float32)
    x = rng.uniform(-1, 1, 700).astype(np.float32)
    d_x = ctx.array(x)
    h = nae.Fir(ctx, taps, 1)                              # the pick: 512
    try:
        h.put(d_x.ptr, 300)
        h.put(d_x.at(300), 400)
        h.flush()
        got = h.receive_host()
        want = fir_ref.run(ref, taps, 512, np.concatenate([x, np.zeros(1, np.float32)]))
        assert np.array_equal(bits(got), bits(want))
    finally:
        h.close()
        d_x.free()


@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_handle_launch_past_block_0_in_several_tiles(nae, ctx, ref, n_fft, ch):
    """3 blocks and 11 frames, then 9 blocks in one put: the second launch computes blocks 3 ... 11 in tiles of 2, and every tile head reads
    the half block in front of it through the FIFO's absolutely indexed view (mono: the unit-stride kernel); then the flushed tail"""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 6 + ch)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = noise(rng, 1, 12 * B + 11, ch)[0]
    try:
        ctx.debug_set("fir_tile", 2)
        got = fir_stream(nae, ctx, taps, n_fft, x, (3 * B + 11, 9 * B))
    finally:
        ctx.debug_set("fir_tile", 0)
    assert np.array_equal(bits(got), bits(ref_fir_flushed(ref, taps, n_fft, x)))


def test_the_context_keeps_the_right_taps(nae, ctx, ref):
    """the block call's cache of the last taps and their spectrum: every call of each sequence equals the statement for ITS taps and size"""
    rng = np.random.default_rng(41)
    x = noise(rng, 2, 3 * 256 + 7, 2)
    a = rng.uniform(-1, 1, 200).astype(np.float32)
    b = rng.uniform(-1, 1, 200).astype(np.float32)

    def check(taps, n_fft, what):
        want = ref_fir(ref, taps, n_fft, x)
        assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x)), bits(want)), what

    # shorter taps after longer ones at the same size: padded taps left behind by A would show
    check(a, 512, "A")
    check(a[:3], 512, "A's first 3 taps after A")
    # the same taps at another size and back
    check(a, 512, "A at 512")
    check(a, 1024, "A at 1024")
    check(a, 512, "A at 512 again")
    check(a, 512, "A at 512, a cache hit")
    # same length, other taps
    check(b, 512, "B after A")
    # the caller rewrites its array in place: the library compares values, not the pointer
    t = a.copy()
    check(t, 512, "t = A")
    t[:] = b[::-1]
    check(t, 512, "t rewritten in place")
    t[117] = np.float32(0.5)
    check(t, 512, "one tap of t changed")
    # a handle created between two block calls computes its own spectrum with the same routine and leaves the context's alone
    check(a, 1024, "A at 1024 before the handle")
    h = nae.Fir(ctx, b, 2, 1024)
    check(a, 1024, "A at 1024 after the handle was created")
    got = fir_stream(nae, ctx, b, 1024, x[0], (700, 75), handle=h)
    assert np.array_equal(bits(got), bits(ref_fir_flushed(ref, b, 1024, x[0]))), "the handle's output, with B"
    check(a, 1024, "A at 1024 after the handle ran")


FLT_MIN = np.float32(1.17549435e-38)


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_subnormal_input(nae, ctx, ref, n_fft):
    """every step an IEEE operation: nothing on the way flushes a subnormal to zero.  The input is subnormal throughout, and so is part of the
    statement's output (asserted: a condition on the input)"""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 7)
    taps = rng.uniform(-1, 1, 5).astype(np.float32)
    x = rng.uniform(-1e-38, 1e-38, (2, 2 * B + 3, 2)).astype(np.float32)
    want = ref_fir(ref, taps, n_fft, x)
    sub = (np.abs(want) < FLT_MIN) & (want != 0)
    assert sub.sum() > want.size // 4 and np.any(np.abs(want) >= FLT_MIN), "subnormal and normal output words"
    assert np.array_equal(bits(gpu_fir(nae, ctx, taps, n_fft, x)), bits(want))


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_overflow(nae, ctx, ref, n_fft):
    """samples near FLT_MAX in blocks 1 and 3 (sums of them overflow on the way) and one Inf in block 5: the non-finite output words are the
    statement's, every other word is equal bit for bit.  NaN payload and sign are not compared."""
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 8)
    taps = rng.uniform(-1, 1, 2).astype(np.float32)
    x = noise(rng, 1, 8 * B + 3, 2)
    x[0, B + 5, 0] = 3e38
    x[0, 3 * B + 9, 0] = 3e38
    x[0, 3 * B + 10, 0] = -3e38
    x[0, 3 * B + 40, 1] = 3e38
    x[0, 3 * B + 41, 1] = 3e38
    x[0, 5 * B + 1, 1] = np.inf
    x[0, 7 * B + 2, 0] = 2.4e39 / B                      # the last FFT's sums pass FLT_MAX on the way to a few output words only
    want = ref_fir(ref, taps, n_fft, x)
    bad = ~np.isfinite(want)
    assert np.all(bad[0, B:3 * B, 0]) and np.all(bad[0, 3 * B:5 * B]) and np.all(bad[0, 5 * B:7 * B, 1]), "the whole of these blocks"
    assert 0 < bad[0, 7 * B:8 * B, 0].sum() < 8, "a few words of this one"
    assert not bad[0, :B].any() and not bad[0, B:3 * B, 1].any() and not bad[0, 5 * B:7 * B, 0].any() and not bad[0, 7 * B:, 1].any()
    got = gpu_fir(nae, ctx, taps, n_fft, x)
    assert np.array_equal(~np.isfinite(got), bad), "the same words are non-finite"
    assert np.array_equal(bits(got)[~bad], bits(want)[~bad])


def test_error_codes(nae, ctx):
    lib = ctx.lib
    INVALID, UNSUPPORTED = -1, -2
    taps = np.ones(2050, np.float32)
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 2)
    tp, s = taps.ctypes.data, C.byref(sig)
    blk = lambda c, t, L, n, src, in_len, ch, ns, dst: lib.nae_fir_block_f32(c, t, L, n, src, in_len, ch, ns, dst)
    try:
        assert blk(None, tp, 3, 0, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, None, 3, 0, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, tp, 3, 0, None, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, tp, 3, 0, s, 8, 2, 1, None) == INVALID
        assert blk(ctx.h, tp, 0, 0, s, 8, 2, 1, s) == INVALID and blk(ctx.h, tp, -4, 512, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, tp, 3, 0, s, 8, 3, 1, s) == INVALID and blk(ctx.h, tp, 3, 0, s, 8, 0, 1, s) == INVALID
        for n_fft in (256, 1000, 8192, -512, 1):
            assert blk(ctx.h, tp, 3, n_fft, s, 8, 2, 1, s) == UNSUPPORTED, n_fft
        assert blk(ctx.h, tp, 258, 512, s, 8, 2, 1, s) == UNSUPPORTED and blk(ctx.h, tp, 2050, 4096, s, 8, 2, 1, s) == UNSUPPORTED
        assert blk(ctx.h, tp, 2050, 0, s, 8, 2, 1, s) == UNSUPPORTED
        assert blk(ctx.h, tp, 3, 0, s, 0, 2, 1, s) == 0 and blk(ctx.h, tp, 3, 0, s, 8, 2, 0, s) == 0
        assert np.all(d.download() == 0), "in_len = 0 and n_streams = 0 launch nothing"
        assert blk(ctx.h, tp, 257, 512, s, 8, 2, 1, s) == 0 and blk(ctx.h, tp, 2049, 4096, s, 8, 2, 1, s) == 0
        h = C.c_void_p()
        mk = lambda c, t, L, n, ch, out: lib.nae_fir_create(c, t, L, n, ch, out)
        assert mk(None, tp, 3, 0, 2, C.byref(h)) == INVALID and mk(ctx.h, None, 3, 0, 2, C.byref(h)) == INVALID
        assert mk(ctx.h, tp, 3, 0, 2, None) == INVALID
        assert mk(ctx.h, tp, 0, 0, 2, C.byref(h)) == INVALID and mk(ctx.h, tp, 3, 0, 3, C.byref(h)) == INVALID
        assert mk(ctx.h, tp, 3, 1000, 2, C.byref(h)) == UNSUPPORTED and mk(ctx.h, tp, 514, 1024, 2, C.byref(h)) == UNSUPPORTED
        assert not h.value
        assert mk(ctx.h, tp, 3, 0, 2, C.byref(h)) == 0 and h.value
        got = C.c_size_t(7)
        assert lib.nae_fir_put(None, d.ptr, 1) == INVALID and lib.nae_fir_put(h, None, 1) == INVALID and lib.nae_fir_put(h, None, 0) == 0
        assert lib.nae_fir_flush(None) == INVALID and lib.nae_fir_available(None) == 0
        assert lib.nae_fir_receive(h, d.ptr, 4, None) == INVALID and lib.nae_fir_receive(h, None, 4, C.byref(got)) == INVALID
        assert lib.nae_fir_receive(h, d.ptr, 4, C.byref(got)) == 0 and got.value == 0
        assert lib.nae_fir_destroy(h) == 0 and lib.nae_fir_destroy(None) == 0
        # the debug key: accepted, range-checked, and an unknown key is still an error
        assert lib.nae_debug_set(ctx.h, b"fir_tile", 5) == 0 and lib.nae_debug_set(ctx.h, b"fir_tile", 0) == 0
        assert lib.nae_debug_set(ctx.h, b"fir_tile", -1) == INVALID
        assert lib.nae_debug_set(ctx.h, b"fir_tiles", 1) == INVALID
    finally:
        lib.nae_debug_set(ctx.h, b"fir_tile", 0)
        d.free()


def test_host_node_graph(tmp_path):
    """source -> audio_filter -> sink: the frames and samples the source sent, its pts, sample n = y[n + 256] of the block call, the flushed
    tail past the input's end"""
    exe = node_harness.build("fir_ref/host_fir_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST FIR OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
