"""K18 saturation on the GPU, bit for bit against the CPU statement (tests/sat_ref/ref_sat.c): every length around the halo, the piece and the
chunk at every oversampling factor, curve and bias, mono and stereo, in every view and at 1, 3 and 130 streams; every tiling; the streaming
handle under every put pattern and over 400 000 frames; two batches that fill and overfill the chip; a non-finite sample's reach; two contexts
interleaved; the error codes; the host node (tests/sat_ref/host_sat_node.cpp); a seeded run of tests/tools/fuzz_sat.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import node_harness
import sat_ref
from block_gpu import CONFIGS, bits, mismatch, noise, statement
from sat_gpu import gpu_sat, lib_params, sat_stream

pytestmark = pytest.mark.gpu

CH = sat_ref.CHUNK
INVALID, UNSUPPORTED = sat_ref.INVALID, sat_ref.UNSUPPORTED
SOFT, HARD = sat_ref.SOFT, sat_ref.HARD
LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 5)


@pytest.fixture(scope="module")
def ref():
    return statement(sat_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("sat_ref/host_sat_node.cpp", str(tmp_path_factory.mktemp("host_sat_gpu")))


def same(got, want):
    return np.array_equal(bits(got), bits(want))


def stated(ref, p, x, shared=False):
    """the statement on x[streams, n, ch]; a shared source is computed once"""
    if shared:
        return np.repeat(sat_ref.run(ref, p, x[0])[None], x.shape[0], axis=0)
    return sat_ref.run_streams(ref, p, x)


@pytest.mark.parametrize("curve", (SOFT, HARD))
@pytest.mark.parametrize("m", sat_ref.FACTORS)
def test_lengths_views_and_streams(nae, ctx, ref, m, curve):
    """every length at bias 0 and 0.3; the view (mono and stereo, interleaved and planar on either side, stream_stride 0, NaN outside the
    source's signals, guard words behind the destination's) and the stream count (1, 3, 130) change from call to call, so that every length
    meets several of each over the eight cases.  The drive of 18 dB on noise of +-1 puts a third of the samples on the curve's flat part"""
    rng = np.random.default_rng(100 * m + curve)
    turn = 3 * sat_ref.FACTORS.index(m) + curve
    for j, bias in enumerate((0.0, 0.3)):
        for i, in_len in enumerate(LENGTHS):
            k = i + 3 * j + turn
            ch, _, sl, dl, shared = CONFIGS[k % len(CONFIGS)]
            n_streams = (1, 3, 130)[(k // 2) % 3]
            p = sat_ref.params(m, curve, 7.94, bias, 0.8, 0.4)
            x = noise(rng, n_streams, in_len, ch, shared)
            got = gpu_sat(nae, ctx, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0)
            message = mismatch(got, stated(ref, p, x, shared))
            assert not message, (in_len, bias, ch, n_streams, sl, dl, shared, message)


@pytest.mark.parametrize("curve", (SOFT, HARD))
@pytest.mark.parametrize("m", sat_ref.FACTORS)
def test_short_lengths_in_every_view_and_stream_count(nae, ctx, ref, m, curve):
    """the lengths around the halo, 1, 63, 64 and 65, crossed with every view of block_gpu.CONFIGS (mono and stereo, interleaved and planar on
    either side, stream_stride 0) and with 1, 3 and 130 streams; the bias, 0 or 0.3, alternates with the length and the view"""
    rng = np.random.default_rng(500 + 10 * m + curve)
    for i, in_len in enumerate((1, 63, 64, 65)):
        for k, (ch, _, sl, dl, shared) in enumerate(CONFIGS):
            p = sat_ref.params(m, curve, 7.94, (0.0, 0.3)[(i + k) % 2], 0.8, 0.4)
            for n_streams in (1, 3, 130):
                x = noise(rng, n_streams, in_len, ch, shared)
                got = gpu_sat(nae, ctx, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0)
                message = mismatch(got, stated(ref, p, x, shared))
                assert not message, (in_len, p.bias, ch, n_streams, sl, dl, shared, message)


def test_unaligned_bases(nae, ctx, ref):
    """bases that are 4-byte aligned and no more, at every factor (M = 1 leaves its 16-byte path)"""
    rng = np.random.default_rng(7)
    x = noise(rng, 2, 2 * CH + 77, 2)
    for m in sat_ref.FACTORS:
        p = sat_ref.params(m, SOFT, 4.0, 0.1, 1.0, 0.5)
        want = stated(ref, p, x)
        for layout in ("i", "p"):
            assert same(gpu_sat(nae, ctx, p, x, layout, layout, offset=3, chan_pad=2 if layout == "p" else 0), want), (m, layout)


@pytest.mark.parametrize("m", (2, 4, 8))
def test_every_tiling_gives_the_same_bits(nae, ctx, ref, m):
    """sat_tile 1, 2, 3 and 0 at 3 * 1024 + 5 samples: four chunks, so one, two, three and four chunks a wave, and a halo across every
    tile edge; one stream (the pick cuts it to one chunk a wave) and 130 (the pick leaves them whole)"""
    rng = np.random.default_rng(20 + m)
    p = sat_ref.params(m, SOFT, 7.94, 0.3, 0.8, 0.4)
    x1, x130 = noise(rng, 1, 3 * CH + 5, 2), noise(rng, 130, 3 * CH + 5, 1)
    want1, want130 = stated(ref, p, x1), stated(ref, p, x130)
    try:
        for tile in (1, 2, 3, 0, 7):
            ctx.debug_set("sat_tile", tile)
            assert same(gpu_sat(nae, ctx, p, x1), want1), tile
            message = mismatch(gpu_sat(nae, ctx, p, x130, "p", "p"), want130)
            assert not message, (tile, message)
    finally:
        ctx.debug_set("sat_tile", 0)
    lib = ctx.lib
    assert lib.nae_debug_set(ctx.h, b"sat_tile", -1) == INVALID and lib.nae_debug_set(ctx.h, b"sat_tiles", 1) == INVALID


@pytest.fixture(scope="module")
def streamed(ref):
    """per factor: parameters, x[3 * 1024 + 600, 2] and what a handle delivers: the statement on x extended by the latency's zeros"""
    out = {}
    for m in sat_ref.FACTORS:
        p = sat_ref.params(m, (SOFT, HARD)[m // 2 % 2], 7.94, 0.2, 0.8, 0.4)
        x = noise(np.random.default_rng(60 + m), 1, 3 * CH + 600, 2)[0]
        out[m] = (p, x, sat_ref.run_tail(ref, p, x))
    return out


@pytest.mark.parametrize("put", (7, 1024, 1025, "random", "everything"))
@pytest.mark.parametrize("m", sat_ref.FACTORS)
def test_handle_equals_the_block_call_on_the_extended_input(nae, ctx, streamed, m, put):
    """any cut of the input into puts, from host and device memory in turn, gives in_len + D frames: the block call's on the input extended by D
    zeros (the statement's bits, and the block call's once)"""
    p, x, want = streamed[m]
    puts = {"random": tuple(int(k) for k in np.random.default_rng(5 + m).integers(1, 2500, 16)), "everything": (len(x),)}.get(put, (put,))
    got = sat_stream(nae, ctx, p, x, puts, device=(False, True))
    assert got.shape == want.shape and same(got, want)
    if put == "everything":
        ext = np.concatenate([x, np.zeros((sat_ref.latency(m), 2), np.float32)])[None]
        assert same(gpu_sat(nae, ctx, p, ext)[0], want)


@pytest.mark.parametrize("m", (1, 4))
def test_handle_one_frame_puts(nae, ctx, ref, m):
    """puts of one frame, 1024 + 200 of them, mono: the partial chunk and the tail are released by the flush alone"""
    p = sat_ref.params(m, SOFT, 7.94, 0.0, 1.0, 0.0)
    x = noise(np.random.default_rng(70 + m), 1, CH + 200, 1)[0]
    assert same(sat_stream(nae, ctx, p, x, (1,), device=(False, True)), sat_ref.run_tail(ref, p, x))


def test_handle_deferred_receives_and_pieces(nae, ctx, streamed):
    """nothing received before the flush, mixed put sizes; and one put of everything received device to device in pieces of 1000 frames"""
    p, x, want = streamed[8]
    assert same(sat_stream(nae, ctx, p, x, (1, 1023, 1025, 7, 2500), device=(True, False), defer=True), want)
    d_out = ctx.array(np.zeros(1000 * 2, np.float32))
    got = sat_stream(nae, ctx, p, x, (len(x),), device=True, d_out=d_out, piece=1000)
    d_out.free()
    assert same(got, want)


def test_handle_long_stream(nae, ctx, ref):
    """400 000 mono frames at M = 2 through one handle in seeded random puts of 1 ... 9000 frames from the device and the host in turn: the
    input FIFO fills, compacts and grows while it keeps a chunk for the halo; every frame against the statement"""
    p = sat_ref.params(2, SOFT, 7.94, 0.1, 0.9, 0.3)
    x = noise(np.random.default_rng(80), 1, 400000, 1)[0]
    puts = tuple(int(k) for k in np.random.default_rng(81).integers(1, 9001, 128))
    got = sat_stream(nae, ctx, p, x, puts, device=(True, False))
    want = sat_ref.run_tail(ref, p, x)
    assert got.shape == want.shape == (400032, 1) and same(got, want)


@pytest.mark.parametrize("m,n_streams,n", ((4, 1024, 2500), (2, 4099, 1500)))
def test_batches(nae, ctx, ref, m, n_streams, n):
    """1024 stereo streams x 2500 frames at M = 4 fill the chip; 4099 x 1500 at M = 2 are 8198 waves, more than it holds, and a prime number of
    streams.  Stream s carries signal s mod 17 of 17 seeded signals at levels spread over 40 dB; the statement runs 17 times and every stream
    is compared"""
    rng = np.random.default_rng(90 + m)
    base = rng.uniform(-1, 1, (17, n, 2)).astype(np.float32) * (10.0 ** (-np.arange(17) * 2.5 / 20.0)).astype(np.float32)[:, None, None]
    p = sat_ref.params(m, SOFT, 15.85, 0.2, 0.8, 0.4)
    want17 = sat_ref.run_streams(ref, p, base)
    pick = np.arange(n_streams) % 17
    message = mismatch(gpu_sat(nae, ctx, p, base[pick]), want17[pick])
    assert not message, message


@pytest.mark.parametrize("bad", (np.nan, np.inf))
def test_a_non_finite_sample_stays_in_its_reach(nae, ctx, ref, bad):
    """x[n] non-finite in one stream-channel, across a tile edge: y[n ... n + 64] of that stream-channel may change, and nothing else; NaN at
    the statement's positions (sign and payload differ between the CPU and the GPU), the statement's bits elsewhere"""
    at = CH - 20
    x = noise(np.random.default_rng(100), 3, 2 * CH + 100, 2)
    dirty_x = x.copy()
    dirty_x[1, at, 0] = bad
    try:
        ctx.debug_set("sat_tile", 1)
        for m in sat_ref.FACTORS:
            p = sat_ref.params(m, (SOFT, HARD)[m // 2 % 2], 3.0, 0.1, 0.8, 0.4)
            clean, got = gpu_sat(nae, ctx, p, x), gpu_sat(nae, ctx, p, dirty_x)
            reach = 64 if m > 1 else 0
            assert same(got[0], clean[0]) and same(got[2], clean[2]) and same(got[1, :, 1], clean[1, :, 1]), "another stream-channel changed"
            assert same(got[1, :at, 0], clean[1, :at, 0]) and same(got[1, at + reach + 1:, 0], clean[1, at + reach + 1:, 0]), m
            want = sat_ref.run(ref, p, dirty_x[1])
            nan_g, nan_w = np.isnan(got[1]), np.isnan(want)
            assert np.array_equal(nan_g, nan_w) and np.array_equal(bits(got[1])[~nan_g], bits(want)[~nan_w]), m
    finally:
        ctx.debug_set("sat_tile", 0)


def test_two_contexts_interleaved(nae, ref):
    """two contexts of one thread, calls in turn with a different factor each time and no wait between them: every context keeps its own
    device taps, of every factor it has run"""
    n = 2 * CH + 9
    x = noise(np.random.default_rng(110), 2, n, 2)
    a, b = nae.Context(0), nae.Context(0)
    try:
        order = [(a, 2), (b, 8), (a, 4), (b, 2), (a, 8), (b, 4), (a, 2), (b, 1), (a, 1), (b, 8)]
        d_x = {c: c.array(x.reshape(-1)) for c in (a, b)}
        outs = []
        for c, m in order:
            d_y = c.array(np.zeros(x.size, np.float32))
            p = sat_ref.params(m, SOFT, 7.94, 0.1, 0.8, 0.4)
            c.sat_block(lib_params(nae, p), nae.Sig.interleaved(d_x[c].ptr, n, 2), n, 2, 2, nae.Sig.interleaved(d_y.ptr, n, 2))
            outs.append((p, d_y))
        for p, d_y in outs:
            assert same(d_y.download().reshape(2, n, 2), stated(ref, p, x)), p.oversample
            d_y.free()
        for d in d_x.values():
            d.free()
    finally:
        a.close()
        b.close()


def test_errors(nae, ctx, ref):
    """the entries answer as the statement's check does (tests/test_sat_cpu.py walks it); dst on src's base is refused; a rejected or empty
    call stores nothing"""
    lib = ctx.lib
    d = ctx.array(np.zeros(128, np.float32))
    src, dst = nae.Sig(d.ptr, 32, 1, 1), nae.Sig(d.at(64), 32, 1, 1)

    def block(p, ch=1, n=16, streams=1, s=C.byref(src), t=C.byref(dst)):
        return lib.nae_sat_block_f32(ctx.h, C.byref(p), s, n, ch, streams, t)

    def create(p, ch=1):
        h = C.c_void_p()
        rc = lib.nae_sat_create(ctx.h, C.byref(p), ch, C.byref(h))
        assert bool(h.value) == (rc == 0)
        if not rc:
            lib.nae_sat_destroy(h)
        return rc

    def both(ch=1, **kw):
        args = dict(oversample=8, curve=HARD, drive=250.0, bias=-3.0, wet=-2.0, dry=1e6)
        args.update(kw)
        sp = sat_ref.params(**args)
        p = lib_params(nae, sp)
        rc = block(p, ch, n=0)
        assert rc == create(p, ch) == ref.ref_sat_check(C.byref(sp), ch), (ch, kw)
        if rc:
            assert block(p, ch) == rc, (ch, kw)
        return rc

    good = lib_params(nae, sat_ref.params(4, SOFT, 4.0))
    assert both() == 0 and both(ch=2) == 0 and both(oversample=1, curve=SOFT) == 0
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    assert both(ch=0) == INVALID and both(ch=3) == INVALID
    for key in ("drive", "bias", "wet", "dry"):
        assert both(**{key: float("nan")}) == INVALID and both(**{key: float("inf")}) == INVALID, key
    assert both(curve=2) == INVALID and both(curve=-1) == INVALID
    for m in (0, 3, 16, -1):
        assert both(oversample=m) == UNSUPPORTED, m
    assert block(good, s=None) == INVALID and block(good, t=None) == INVALID
    assert lib.nae_sat_block_f32(ctx.h, None, C.byref(src), 16, 1, 1, C.byref(dst)) == INVALID
    assert block(good, t=C.byref(src)) == INVALID, "in place is refused"
    assert block(lib_params(nae, sat_ref.params(1)), t=C.byref(src)) == INVALID, "at every factor"
    h = C.c_void_p()
    assert lib.nae_sat_create(ctx.h, None, 1, C.byref(h)) == INVALID and lib.nae_sat_create(ctx.h, C.byref(good), 1, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download(), np.zeros(128, np.float32)), "no rejected or empty call stored a sample"
    d.free()


def test_host_node_graph(host):
    """source -> audio_saturation -> sink with 1152-sample frames, stereo and mono, at 1, 2, 4 and 8: the source's frames, sizes and pts; the
    samples of the statement (tests/sat_ref/ref_sat.c, compiled into the harness) on the extended input, shifted by the latency, and the
    block call's are the same"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST SAT OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_fuzz_sat_seeded(nae, ctx):
    """a seeded run of tests/tools/fuzz_sat.py: parameters over their whole range, lengths, views, tilings and put patterns"""
    sys.path.insert(0, os.path.join(sat_ref.ROOT, "tests", "tools"))
    import fuzz_sat
    assert fuzz_sat.main(cases=fuzz_sat.SEEDED[0], seed=fuzz_sat.SEEDED[1], ctx=ctx, nae=nae) == fuzz_sat.SEEDED[0]
