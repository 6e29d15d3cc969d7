"""K9 FIR filter on the GPU: nae_fir_block_f32 bit for bit against the CPU statement (tests/fir_ref/ref_fir.c) at the smallest shapes that reach
every edge, every tiling, a NaN's reach, the streaming handle, the error codes, and the host node (tests/fir_ref/host_fir_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fir_ref
import node_harness

pytestmark = pytest.mark.gpu

PAD = 8        # frames behind every destination signal that must stay untouched
SENTINEL = np.float32(-12345.0)
# (channels, streams, source layout, destination layout, shared source): interleaved and planar views on both sides, stream_stride = 0
CONFIGS = ((1, 1, "i", "i", False), (2, 1, "i", "i", False), (1, 3, "p", "p", False), (2, 3, "p", "p", False),
           (2, 3, "i", "p", False), (2, 1, "p", "i", False), (2, 3, "i", "i", True), (1, 3, "p", "p", True))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return fir_ref.build(str(tmp_path_factory.mktemp("ref_fir_gpu")))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_fir(nae, ctx, taps, n_fft, x, src_layout="i", dst_layout="i", shared=False):
    """x[streams, n, ch] -> y[streams, n, ch] through nae_fir_block_f32; the frames behind each destination signal are checked untouched"""
    n_streams, n, ch = x.shape
    xs = x[:1] if shared else x
    src_host = xs if src_layout == "i" else xs.transpose(0, 2, 1)
    d_x = ctx.array(np.ascontiguousarray(src_host, np.float32).reshape(-1))
    ss = 0 if shared else n * ch
    src = nae.Sig(d_x.ptr, ss, 1, ch) if src_layout == "i" else nae.Sig(d_x.ptr, ss, n, 1)
    m = n + PAD
    d_y = ctx.array(np.full(n_streams * m * ch, SENTINEL, np.float32))
    dst = nae.Sig(d_y.ptr, m * ch, 1, ch) if dst_layout == "i" else nae.Sig(d_y.ptr, m * ch, m, 1)
    ctx.fir_block(taps, src, n, ch, n_streams, dst, n_fft)
    out = d_y.download()
    d_x.free()
    d_y.free()
    out = out.reshape(n_streams, m, ch) if dst_layout == "i" else out.reshape(n_streams, ch, m).transpose(0, 2, 1)
    assert np.all(out[:, n:, :] == SENTINEL), "wrote behind in_len"
    return np.ascontiguousarray(out[:, :n, :])


def ref_fir(ref, taps, n_fft, x):
    """the statement on x[streams, n, ch]"""
    return np.stack([fir_ref.run(ref, taps, n_fft, s.reshape(-1), ch=x.shape[2]).reshape(s.shape) for s in x])


def _noise(rng, n_streams, n, ch, shared=False):
    x = rng.uniform(-1, 1, (n_streams, n, ch)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


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
            x = _noise(rng, n_streams, in_len, ch, shared)
            got = gpu_fir(nae, ctx, taps, n_fft, x, sl, dl, shared)
            want = ref_fir(ref, taps, n_fft, x)
            assert np.array_equal(_bits(got), _bits(want)), (n_fft, L, in_len, ch, n_streams, sl, dl, shared)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"ch{c[0]}-s{c[1]}-{c[2]}{c[3]}{'-shared' if c[4] else ''}")
def test_block_bits_in_every_view(nae, ctx, ref, cfg):
    """mono / stereo, 1 / 3 streams, interleaved and planar views on both sides, a shared source: more than one block and a partial one"""
    ch, n_streams, sl, dl, shared = cfg
    n_fft, B = 512, 256
    rng = np.random.default_rng(77)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = _noise(rng, n_streams, 3 * B + 7, ch, shared)
    got = gpu_fir(nae, ctx, taps, n_fft, x, sl, dl, shared)
    assert np.array_equal(_bits(got), _bits(ref_fir(ref, taps, n_fft, x)))


def test_pick_equals_explicit_size(nae, ctx):
    rng = np.random.default_rng(9)
    x = _noise(rng, 2, 2500, 2)
    for L, n_fft in ((1, 512), (257, 512), (258, 1024), (513, 1024), (514, 2048), (1026, 4096), (2049, 4096)):
        taps = rng.uniform(-1, 1, L).astype(np.float32)
        assert nae.Context.fir_pick_n_fft(L) == n_fft
        assert np.array_equal(_bits(gpu_fir(nae, ctx, taps, 0, x)), _bits(gpu_fir(nae, ctx, taps, n_fft, x))), L


@pytest.mark.parametrize("n_fft", (512, 4096))
def test_every_tiling_gives_the_same_bits(nae, ctx, ref, n_fft):
    B = n_fft // 2
    rng = np.random.default_rng(n_fft + 1)
    taps = rng.uniform(-1, 1, B + 1).astype(np.float32)
    x = _noise(rng, 2, 7 * B + 5, 2)
    own = gpu_fir(nae, ctx, taps, n_fft, x)
    assert np.array_equal(_bits(own), _bits(ref_fir(ref, taps, n_fft, x)))
    try:
        for tile in (1, 2, 3):
            ctx.debug_set("fir_tile", tile)
            assert np.array_equal(_bits(gpu_fir(nae, ctx, taps, n_fft, x)), _bits(own)), tile
            assert np.array_equal(_bits(gpu_fir(nae, ctx, taps, n_fft, x, "p", "p")), _bits(own)), tile
    finally:
        ctx.debug_set("fir_tile", 0)


def test_nan_reaches_only_the_blocks_that_read_it(nae, ctx):
    n_fft, B = 512, 256
    rng = np.random.default_rng(11)
    taps = rng.uniform(-1, 1, 65).astype(np.float32)
    x = _noise(rng, 2, 5 * B + 3, 2)
    clean = gpu_fir(nae, ctx, taps, n_fft, x)
    p = 2 * B + 10                       # read by blocks 2 (its new half) and 3 (its carried half)
    x[1, p, 0] = np.nan
    got = gpu_fir(nae, ctx, taps, n_fft, x)
    hit = np.zeros(x.shape, bool)
    hit[1, 2 * B:4 * B, 0] = True
    assert np.all(np.isnan(got[hit])), "every sample of the two blocks is NaN"
    assert np.array_equal(_bits(got)[~hit], _bits(clean)[~hit]), "no other output word changes"
    try:
        ctx.debug_set("fir_tile", 1)     # the block after the NaN starts a tile: it reads the sample through the tile head
        assert np.array_equal(_bits(gpu_fir(nae, ctx, taps, n_fft, x)), _bits(got))
    finally:
        ctx.debug_set("fir_tile", 0)


@pytest.fixture(scope="module")
def handle_case(nae, ctx, ref):
    """N = 1024, L = 513, 5000 stereo frames: the block call's bits and the statement on the zero-extended input, computed once"""
    rng = np.random.default_rng(21)
    L, in_len = 513, 5000
    taps = rng.uniform(-1, 1, L).astype(np.float32)
    x = _noise(rng, 1, in_len, 2)
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
        assert np.array_equal(_bits(got[:in_len]), _bits(block)), "the first in_len frames are the block call's"
        assert np.array_equal(_bits(got), _bits(tail)), "and the tail is the statement on the zero-extended input"
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
        assert np.array_equal(_bits(got), _bits(want))
    finally:
        h.close()
        d_x.free()


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
