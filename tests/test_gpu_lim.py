"""K22 limiter on the GPU, bit for bit against the CPU statement (tests/lim_ref/ref_lim.c): the five signals of tests/lim_ref.py at every
look-ahead around the lane and the limit, both detectors, linked and unlinked, both ends of the release, every view, the streaming handle in
every put pattern, two contexts, a launch of 300 chunks, a batch of more waves than the chip holds, non-finite input, the error codes, the
host node (tests/lim_ref/host_lim_node.cpp) and a seeded run of tests/tools/fuzz_lim.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lim_ref
import node_harness
from block_gpu import CONFIGS, bits, each_stream, mismatch, statement
from lim_gpu import gpu_lim, lib_params, lim_stream

pytestmark = pytest.mark.gpu

T, CH = lim_ref.LANE, lim_ref.CHUNK
LOOKAHEADS = (0, 1, 15, 16, 17, 1018)
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ref():
    return statement(lim_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("lim_ref/host_lim_node.cpp", str(tmp_path_factory.mktemp("host_lim_gpu")))


def same(nae, ctx, ref, p, x, *views, **kw):
    got, want = gpu_lim(nae, ctx, p, x, *views, **kw), lim_ref.run_streams(ref, p, x)
    return mismatch(got, want)


@pytest.mark.parametrize("la", LOOKAHEADS)
def test_small_batch(nae, ctx, ref, la):
    """the five signals of 3 C + 7 samples as 3 stereo streams (two of them rolled and scaled) and one mono stream: both detectors, linked
    and unlinked, release 1 ms and 5 s, the full cross"""
    for name, x in lim_ref.signals().items():
        x3 = np.stack([x, np.roll(x, 301, axis=0) * np.float32(0.5), x[::-1] * np.float32(1.7)])
        mono = x[None, :, :1].copy()
        for tp in (0, 1):
            for ar in (lim_ref.FAST, lim_ref.SLOW):
                for link in (0, 1):
                    message = same(nae, ctx, ref, lim_ref.params(lookahead=la, true_peak=tp, link=link, alpha_release=ar), x3)
                    assert not message, (name, la, tp, link, ar, message)
                message = same(nae, ctx, ref, lim_ref.params(lookahead=la, true_peak=tp, link=1, alpha_release=ar), mono)
                assert not message, (name, la, tp, "mono", ar, message)


@pytest.mark.parametrize("tp", (0, 1))
def test_lengths(nae, ctx, ref, tp):
    """the lane edge and the chunk edge in the length: a signal that ends within the detector's reach of a chunk border has a level past it"""
    rng = np.random.default_rng(40 + tp)
    for in_len in (1, 5, 6, 7, T, T + 1, CH - 7, CH - 6, CH - 1, CH, CH + 1, CH + 6, 2 * CH):
        for la in (0, 5, 17, 1018):
            p = lim_ref.params(lookahead=la, true_peak=tp, link=in_len % 2)
            message = same(nae, ctx, ref, p, rng.uniform(-1, 1, (2, in_len, 2)).astype(np.float32))
            assert not message, (in_len, la, message)


@pytest.mark.parametrize("tp", (0, 1))
def test_views(nae, ctx, ref, tp):
    """interleaved and planar on either side, stream_stride 0, odd offsets, gaps; the guard words around the destination stand and nothing
    outside a source signal is read (view_call fills it with NaN)"""
    rng = np.random.default_rng(10 + tp)
    in_len = CH + 3 * T + 5
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        for link in (0, 1):
            p = lim_ref.params(lookahead=(0, 17, 200)[i % 3], true_peak=tp, link=link, alpha_release=(lim_ref.FAST, lim_ref.SLOW)[i % 2])
            x = rng.uniform(-1, 1, (n_streams, in_len, ch)).astype(np.float32)
            if shared:
                x[:] = x[0]
            message = same(nae, ctx, ref, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
            assert not message, (ch, n_streams, sl, dl, shared, link, message)


def test_in_place(nae, ctx, ref):
    """dst->base == src->base is allowed: a chunk's samples are read for the last time before they are stored"""
    x = np.random.default_rng(5).uniform(-1, 1, (3, 2 * CH + 9, 2)).astype(np.float32)
    for link, la, tp in ((1, 0, 1), (0, 300, 1), (1, 1018, 0)):
        p = lim_ref.params(lookahead=la, link=link, true_peak=tp)
        d = ctx.array(x.reshape(-1))
        sig = nae.Sig(d.ptr, x.shape[1] * 2, 1, 2)
        ctx.lim_block(lib_params(nae, p), sig, x.shape[1], 2, 3, sig)
        got = d.download().reshape(x.shape)
        d.free()
        message = mismatch(got, lim_ref.run_streams(ref, p, x))
        assert not message, (link, la, message)


@pytest.mark.parametrize("la", (0, 17, 1018))
@pytest.mark.parametrize("put", (1, 1023, 1024, 1025, "ragged"))
def test_handle_equals_the_block_call(nae, ctx, ref, put, la):
    """any cut of the input into puts gives the block call's bits; `available` follows floor((put - la - D) / 1024) chunks after every put
    and the flush releases the rest; a put after the flush is NAE_ERR_STATE (lim_stream asserts all three)"""
    # single frames: just past the first chunk with its look-ahead and reach, so a chunk comes out before the flush and the carries, the
    # running total and the prefix sums in device memory are crossed by one-frame puts
    in_len = CH + la + lim_ref.REACH + 37 if put == 1 else 3 * CH + 7
    ch, link = (1, 0) if put in (1023, 1024) else (2, 1 if put != 1025 else 0)
    puts = tuple(int(k) for k in np.random.default_rng(la).integers(1, 1500, 16)) if put == "ragged" else (put,)
    x = lim_ref.signals(in_len, seed=la + 2)["noise" if put != 1025 else "peaks"][None, :, :ch].copy()
    for tp in (0, 1):
        p = lim_ref.params(lookahead=la, true_peak=tp, link=link, alpha_release=lim_ref.alpha(0.05))
        block = gpu_lim(nae, ctx, p, x)[0]
        assert np.array_equal(bits(block), bits(lim_ref.run(ref, p, x[0])))
        for device in (False, True):
            got = lim_stream(nae, ctx, p, x[0], puts, device=device)
            assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block)), (device, tp)


def test_two_handles_on_one_context_and_on_two(nae, ctx, ref):
    """two handles fed in turn, on one context and on two: each gives its own block call's bits"""
    x = np.random.default_rng(21).uniform(-1, 1, (2, 3 * CH + 100, 2)).astype(np.float32)
    ps = [lim_ref.params(lookahead=33, link=1, true_peak=1), lim_ref.params(lookahead=500, link=0, true_peak=0, alpha_release=lim_ref.SLOW)]
    want = [lim_ref.run(ref, ps[k], x[k]) for k in range(2)]
    other = nae.Context(0)
    try:
        for ctxs in ((ctx, ctx), (ctx, other)):
            hs = [nae.Limiter(ctxs[k], lib_params(nae, ps[k]), 2) for k in range(2)]
            parts = [[], []]
            try:
                for pos in range(0, x.shape[1], 777):
                    for k in range(2):
                        hs[k].put_host(x[k, pos:pos + 777].reshape(-1))
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


def test_large_batch(nae, ctx, ref):
    """4099 unlinked stereo streams of 2 chunks are 8198 waves, more than the chip holds, and a prime number of streams.  Stream s carries
    signal s mod 17 of 17 seeded signals; the statement runs on each and every stream is compared"""
    base = np.random.default_rng(90).uniform(-1, 1, (17, 2 * CH, 2)).astype(np.float32)
    p = lim_ref.params(lookahead=72, link=0, true_peak=1, alpha_release=lim_ref.alpha(0.05))
    want17 = each_stream(lambda i: lim_ref.run(ref, p, base[i]), 17)
    pick = np.arange(4099) % 17
    message = mismatch(gpu_lim(nae, ctx, p, base[pick]), want17[pick])
    assert not message, message


def test_long_launch(nae, ctx, ref):
    """one stereo stream of 300 C + 7 samples at the slowest release: one wave walks 301 chunks, the release it carries from chunk to chunk
    has a memory of hundreds of them, and the running total of q grows past 2^45"""
    p = lim_ref.params(lookahead=72, link=1, true_peak=1, alpha_release=lim_ref.SLOW)
    n = 300 * CH + 7
    x = (np.random.default_rng(300).uniform(-1, 1, (1, n, 2)) * (0.3 + 0.7 * (np.arange(n) % 40000 < 9000))[None, :, None]).astype(np.float32)
    message = same(nae, ctx, ref, p, x, "p", "i", chan_pad=3)
    assert not message, message


@pytest.mark.parametrize("la", (0, 17, 1018))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_does_not_reach_back(nae, ctx, bad, la):
    """a non-finite sample at i = 2 C + 5: every output before i - la - D has the clean run's bits, the other stream is untouched, the call
    returns NAE_OK and the sentinels around the destination stand (view_call checks them)"""
    i = 2 * CH + 5
    x = np.random.default_rng(9).uniform(-1, 1, (2, 3 * CH + 40, 2)).astype(np.float32)
    dirty_x = x.copy()
    dirty_x[0, i, 0] = bad
    for tp in (0, 1):
        p = lim_ref.params(lookahead=la, link=1, true_peak=tp)
        clean = gpu_lim(nae, ctx, p, x, "p", "p", chan_pad=3)
        got = gpu_lim(nae, ctx, p, dirty_x, "p", "p", chan_pad=3)
        stop = i - la - lim_ref.reach(p)
        assert np.array_equal(bits(got[:, :stop]), bits(clean[:, :stop])), "samples before i - la - D changed"
        assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = lim_ref.params(gain_db=0.0)

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1):
        return lib.nae_lim_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    assert block(good) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    h = C.c_void_p()
    for field, values in (("ceiling_db", (-20.5, 0.5, np.nan)), ("gain_db", (-24.5, 24.5, np.inf)), ("alpha_release", (-0.1, 1.0, np.nan)),
                          ("lookahead", (-1,)), ("true_peak", (2, -1)), ("link", (2, -1))):
        for v in values:
            p = lim_ref.params()
            setattr(p, field, v)
            assert block(p) == INVALID, (field, v)
            assert block(p, n=0) == INVALID, "checked before the empty call returns"
            assert lib.nae_lim_create(ctx.h, C.byref(lib_params(nae, p)), 2, C.byref(h)) == INVALID and not h.value, (field, v)
    far = lim_ref.params(lookahead=1019)
    assert block(far) == UNSUPPORTED and lib.nae_lim_create(ctx.h, C.byref(lib_params(nae, far)), 2, C.byref(h)) == UNSUPPORTED and not h.value
    assert block(lim_ref.params(lookahead=1018, gain_db=0.0)) == 0
    assert lib.nae_lim_create(ctx.h, None, 2, C.byref(h)) == INVALID
    assert lib.nae_lim_create(ctx.h, C.byref(lib_params(nae, good)), 3, C.byref(h)) == INVALID
    assert lib.nae_lim_create(ctx.h, C.byref(lib_params(nae, good)), 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host):
    """source -> audio_limiter -> sink with 1152-sample frames: the source's frames, sizes and pts; the statement's samples with the designed
    parameters, and the block call's"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST LIM OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_fuzz_lim_seeded(nae, ctx):
    """a seeded run of tests/tools/fuzz_lim.py: parameters at their edges, lengths, views, put patterns and peaks at drawn positions"""
    sys.path.insert(0, os.path.join(lim_ref.ROOT, "tests", "tools"))
    import fuzz_lim
    assert fuzz_lim.main(cases=fuzz_lim.SEEDED[0], seed=fuzz_lim.SEEDED[1], ctx=ctx, nae=nae) == fuzz_lim.SEEDED[0]
