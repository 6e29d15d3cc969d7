"""K21 separation on the GPU, bit for bit against the CPU statement (tests/hpss_ref/ref_hpss.c): every frame size, both masks, mono and
stereo, one and three streams, the spans at their edges, the lengths around the hop, a strided view, every tiling, the streaming handle in ragged
puts, a batch of more items than the chip holds resident waves, the error codes, and the host node (tests/hpss_ref/host_hpss_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hpss_ref
import node_harness
from block_gpu import bits, each_stream, mismatch, statement
from hpss_gpu import gpu_hpss, hpss_stream, lib_params

pytestmark = pytest.mark.gpu

N0, H0 = 512, 128
SPANS = ((0, 0), (1, 8), (8, 1), (8, 8))
INVALID, UNSUPPORTED, STATE = -1, -2, -5


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


def test_batch_beyond_the_resident_waves(nae, ctx, ref):
    """1100 stereo streams of three blocks at N = 512: 2200 waves, more than the 256 CUs hold at 8 each, so the launch list has a second round;
    every stream is compared"""
    rng = np.random.default_rng(2200)
    p = hpss_ref.params(N0, 8, 8, 0, 1.0, 0.0)
    x = wander(rng, 1100, 2 * H0 + 3, 2)
    want = each_stream(lambda i: hpss_ref.run(ref, p, x[i]), len(x))
    got = gpu_hpss(nae, ctx, p, x)
    assert not mismatch(got, want), mismatch(got, want)


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
