"""K10 long convolution on the GPU: nae_conv_block_f32 and the nae_conv handle bit for bit against the CPU statement
(tests/conv_ref/ref_conv.c) at the smallest shapes that reach every mechanism: blocks in front of and behind the P-th, per-channel taps, every
view, every accumulate tile, slabs of one and two blocks and a wrapped ring, the limits, a NaN's reach, the handle, the context's cache and the
error codes, and the host node (tests/conv_ref/host_conv_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import conv_ref
import node_harness
from block_gpu import CONFIGS, bits, noise, statement
from conv_gpu import conv_stream, gpu_conv
from fir_gpu import gpu_fir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return statement(conv_ref)


def _taps(rng, L, taps_ch=1):
    return rng.uniform(-1, 1, L if taps_ch == 1 else (taps_ch, L)).astype(np.float32)


def _check(nae, ctx, ref, taps, n_fft, x, *a, **kw):
    got = gpu_conv(nae, ctx, taps, n_fft, x, *a, **kw)
    want = conv_ref.run_streams(ref, taps, n_fft, x)
    assert np.array_equal(bits(got), bits(want)), (n_fft, taps.shape, x.shape, a, kw)
    return got


@pytest.mark.parametrize("L", (1, 256, 257, 773))
def test_block_bits_in_every_view(nae, ctx, ref, L):
    """N = 512, P = 1, 1, 2, 4; 8 blocks, the last partial: blocks with b < P and with b >= P; every view, one set of taps and one per channel"""
    rng = np.random.default_rng(L)
    in_len = 7 * 256 + 3
    for ch, n_streams, sl, dl, shared in CONFIGS:
        x = noise(rng, n_streams, in_len, ch, shared)
        for taps_ch in sorted({1, ch}):
            _check(nae, ctx, ref, _taps(rng, L, taps_ch), 512, x, sl, dl, shared, gap=5, chan_pad=3 if "p" in (sl, dl) else 0)


@pytest.mark.parametrize("n_fft", conv_ref.SIZES)
def test_every_size_at_three_partitions(nae, ctx, ref, n_fft):
    B = n_fft // 2
    rng = np.random.default_rng(n_fft)
    _check(nae, ctx, ref, _taps(rng, 2 * B + 5, 2), n_fft, noise(rng, 2, 6 * B + 9, 2))


@pytest.mark.parametrize("n_fft", conv_ref.SIZES)
def test_one_partition_equals_the_fir_filter(nae, ctx, n_fft):
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 1)
    x = noise(rng, 2, 3 * B + 7, 2)
    for L in (1, B):
        taps = _taps(rng, L)
        assert np.array_equal(bits(gpu_conv(nae, ctx, taps, n_fft, x)), bits(gpu_fir(nae, ctx, taps, n_fft, x))), L


@pytest.mark.parametrize("n_fft,P", ((512, 6), (4096, 3)))
def test_every_tile_gives_the_same_bits(nae, ctx, ref, n_fft, P):
    """conv_tile 1, 2, 3 (shorter than the register tile at 512), 100 (one wave walks several register groups and a partial one) and automatic"""
    B = n_fft // 2
    rng = np.random.default_rng(5)
    taps, x = _taps(rng, (P - 1) * B + 9, 2), noise(rng, 1, 10 * B + 5, 2)
    try:
        for tile in (1, 2, 3, 100, 0):
            ctx.debug_set("conv_tile", tile)
            _check(nae, ctx, ref, taps, n_fft, x)
    finally:
        ctx.debug_set("conv_tile", 0)


def test_every_ring_gives_the_same_bits(nae, ctx, ref):
    """P = 4: conv_ring P (slabs of 1 block), P + 1 (2 blocks) and 2 P + 3 (slabs of 8: the 13 blocks wrap the ring of 11 slots); a ring below P is
    raised to P"""
    rng = np.random.default_rng(6)
    taps, x = _taps(rng, 773, 2), noise(rng, 2, 12 * 256 + 50, 2)
    try:
        for ring in (4, 5, 11, 1):
            ctx.debug_set("conv_ring", ring)
            _check(nae, ctx, ref, taps, 512, x)
    finally:
        ctx.debug_set("conv_ring", 0)


def test_several_workgroups_and_a_partial_one(nae, ctx, ref):
    """N = 512: 9 stream-channels x 9 blocks are 27 accumulate waves (7 per workgroup: 3 whole, one of 6) and 9 spectrum waves (8 per workgroup)"""
    rng = np.random.default_rng(7)
    _check(nae, ctx, ref, _taps(rng, 600), 512, noise(rng, 9, 9 * 256 - 11, 1), "p", "p")


@pytest.mark.parametrize("n_fft,L,blocks", ((512, 512 * 256, 520), (4096, 262144, 130)))
def test_the_limits(nae, ctx, ref, n_fft, L, blocks):
    """NAE_CONV_MAX_PARTS partitions at 512 and NAE_CONV_MAX_TAPS taps at 4096 (P = 128), with blocks behind the P-th; one mono stream"""
    B = n_fft // 2
    rng = np.random.default_rng(8)
    taps = (_taps(rng, L) * np.float32(0.05))
    _check(nae, ctx, ref, taps, n_fft, noise(rng, 1, blocks * B - 3, 1))


def test_a_nan_reaches_p_plus_one_blocks(nae, ctx, ref):
    """N = 512, P = 3, a NaN at sample i of block 4: blocks 4 ... 7 may change, the block holding it is non-finite, every other keeps its bits"""
    B, P = 256, 3
    rng = np.random.default_rng(9)
    taps, x = _taps(rng, 2 * B + 40), noise(rng, 1, 12 * B, 1)
    clean = gpu_conv(nae, ctx, taps, 512, x)
    i = 4 * B + 17
    x[0, i, 0] = np.nan
    got = gpu_conv(nae, ctx, taps, 512, x)
    # against the statement: the same words are non-finite and every other word has its bits (the sign and payload of a NaN are the machine's: an
    # x86 NaN from an invalid operation is negative, the GPU's positive; tests/test_gpu_fir.py compares a NaN's reach the same way)
    want = conv_ref.run_streams(ref, taps, 512, x)
    bad = ~np.isfinite(want)
    assert np.array_equal(~np.isfinite(got), bad), "the same words are non-finite"
    assert np.array_equal(bits(got)[~bad], bits(want)[~bad])
    b = i // B
    assert np.array_equal(bits(got[0, :b * B]), bits(clean[0, :b * B]))
    assert np.array_equal(bits(got[0, (b + P + 1) * B:]), bits(clean[0, (b + P + 1) * B:]))
    assert not np.isfinite(got[0, b * B:(b + 1) * B]).any()


@pytest.mark.parametrize("device", (False, True))
def test_handle_equals_the_block_call(nae, ctx, ref, device):
    """P = 4 at 512 with per-channel taps: puts of 1, B - 1, B, B + 1 and 5 B + 3 frames, then 5 B + 3 again; with conv_ring = 6 (slabs of 3
    blocks) the ring wraps between puts.  in_len + L - 1 frames come out: the statement on the zero-extended input, whose first in_len frames
    are the block call's"""
    B, L = 256, 773
    rng = np.random.default_rng(10)
    taps, x = _taps(rng, L, 2), noise(rng, 1, 14 * B + 31, 2)[0]
    ext = np.concatenate([x, np.zeros((L - 1, 2), np.float32)])
    want = conv_ref.run_streams(ref, taps, 512, ext[None])[0]
    block = gpu_conv(nae, ctx, taps, 512, x[None])[0]
    assert np.array_equal(bits(block), bits(want[:len(x)]))
    try:
        for ring in (0, 6):
            ctx.debug_set("conv_ring", ring)
            got = conv_stream(nae, ctx, taps, 512, x, (1, B - 1, B, B + 1, 5 * B + 3), device)
            assert got.shape == (len(x) + L - 1, 2)
            assert np.array_equal(bits(got), bits(want)), ring
    finally:
        ctx.debug_set("conv_ring", 0)


def test_context_cache(nae, ctx, ref):
    """the context keeps H of the last call: the same taps twice, changed taps, changed taps_ch, changed N, and a FIR call in between (the two
    caches are separate)"""
    rng = np.random.default_rng(11)
    x = noise(rng, 1, 5 * 256 + 9, 2)
    a, b = _taps(rng, 600), _taps(rng, 600)
    fir_taps = _taps(rng, 100)
    fir_want = gpu_fir(nae, ctx, fir_taps, 512, x)
    _check(nae, ctx, ref, a, 512, x)
    _check(nae, ctx, ref, a, 512, x)
    _check(nae, ctx, ref, b, 512, x)
    assert np.array_equal(bits(gpu_fir(nae, ctx, fir_taps, 512, x)), bits(fir_want))
    _check(nae, ctx, ref, b, 512, x)
    _check(nae, ctx, ref, np.stack([b, b]), 512, x)
    _check(nae, ctx, ref, np.stack([b, a]), 512, x)
    _check(nae, ctx, ref, np.stack([b, a]), 1024, x)
    _check(nae, ctx, ref, b, 1024, x)
    assert np.array_equal(bits(gpu_fir(nae, ctx, fir_taps, 512, x)), bits(fir_want))


def test_error_codes(nae, ctx):
    lib = ctx.lib
    INVALID, UNSUPPORTED = -1, -2
    taps = np.zeros(3 * 262145, np.float32)
    d = ctx.array(np.zeros(96, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 2)
    sig3 = nae.Sig(d.ptr, 32, 1, 3)
    tp, s = taps.ctypes.data, C.byref(sig)
    blk = lib.nae_conv_block_f32
    h = C.c_void_p()
    try:
        assert blk(None, tp, 3, 1, 0, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, None, 3, 1, 0, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, tp, 3, 1, 0, None, 8, 2, 1, s) == INVALID and blk(ctx.h, tp, 3, 1, 0, s, 8, 2, 1, None) == INVALID
        assert blk(ctx.h, tp, 0, 1, 0, s, 8, 2, 1, s) == INVALID
        assert blk(ctx.h, tp, 3, 3, 0, s, 8, 2, 1, s) == INVALID, "taps_ch = 3"
        assert blk(ctx.h, tp, 3, 2, 0, s, 8, 1, 1, s) == INVALID, "taps_ch = 2 on a mono signal"
        assert blk(ctx.h, tp, 3, 1, 0, C.byref(sig3), 8, 3, 1, C.byref(sig3)) == INVALID, "ch = 3"
        assert blk(ctx.h, tp, 3, 1, 300, s, 8, 2, 1, s) == UNSUPPORTED
        assert blk(ctx.h, tp, 262145, 1, 0, s, 8, 2, 1, s) == UNSUPPORTED, "more than NAE_CONV_MAX_TAPS taps"
        assert blk(ctx.h, tp, 512 * 256 + 1, 1, 512, s, 8, 2, 1, s) == UNSUPPORTED, "P = 513 at 512"
        assert blk(ctx.h, tp, 262144, 1, 512, s, 8, 2, 1, s) == UNSUPPORTED, "P = 1024 at 512 with L within the tap limit"
        assert blk(ctx.h, tp, 262144, 1, 1024, s, 0, 2, 1, s) == 0 and blk(ctx.h, tp, 512 * 256, 1, 512, s, 8, 2, 0, s) == 0, "zero lengths"
        assert blk(ctx.h, tp, 3, 2, 0, s, 8, 2, 1, s) == 0
        for L, want in ((0, 0), (1, 512), (4096, 512), (4097, 1024), (32768, 4096), (32769, 4096), (262144, 4096), (262145, 0)):
            assert lib.nae_conv_pick_n_fft(L) == want, L
        mk = lib.nae_conv_create
        assert mk(None, tp, 3, 1, 0, 2, C.byref(h)) == INVALID and mk(ctx.h, None, 3, 1, 0, 2, C.byref(h)) == INVALID
        assert mk(ctx.h, tp, 3, 1, 0, 2, None) == INVALID
        assert mk(ctx.h, tp, 3, 3, 0, 2, C.byref(h)) == INVALID and mk(ctx.h, tp, 3, 1, 0, 3, C.byref(h)) == INVALID
        assert mk(ctx.h, tp, 262145, 1, 0, 2, C.byref(h)) == UNSUPPORTED and mk(ctx.h, tp, 262144, 1, 512, 2, C.byref(h)) == UNSUPPORTED
        assert not h.value
        assert mk(ctx.h, tp, 3, 2, 0, 2, C.byref(h)) == 0 and h.value
        got = C.c_size_t(7)
        assert lib.nae_conv_put(None, d.ptr, 1) == INVALID and lib.nae_conv_put(h, None, 1) == INVALID and lib.nae_conv_put(h, None, 0) == 0
        assert lib.nae_conv_flush(None) == INVALID and lib.nae_conv_available(None) == 0
        assert lib.nae_conv_receive(h, d.ptr, 4, None) == INVALID and lib.nae_conv_receive(h, None, 4, C.byref(got)) == INVALID
        assert lib.nae_conv_receive(h, d.ptr, 4, C.byref(got)) == 0 and got.value == 0
        assert lib.nae_conv_destroy(h) == 0 and lib.nae_conv_destroy(None) == 0
        for key in (b"conv_tile", b"conv_ring"):
            assert lib.nae_debug_set(ctx.h, key, 5) == 0 and lib.nae_debug_set(ctx.h, key, 0) == 0 and lib.nae_debug_set(ctx.h, key, -1) == INVALID
    finally:
        d.free()


def test_host_node_graph(tmp_path):
    """source -> audio_reverb -> sink: the frames and samples the source sent, its pts, and the block call's samples with the designed taps of
    seed + c on channel c"""
    exe = node_harness.build("conv_ref/host_conv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST CONV OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
