"""K17 modulated delay on the GPU, bit for bit against the CPU statement (tests/mod_ref/ref_mod.c): every length around the run, the chunk and
the ring's wrap at every run length the sub-block rule gives, with and without feedback, one and four voices, both shapes, mono and stereo
with and without spread; every forced run length; every view and in place; the streaming handle under every put pattern and over 400 000
frames; a batch that overfills the chip; a NaN that stays in its stream-channel; two contexts from two threads; the error codes; and the host
node (tests/mod_ref/host_mod_node.cpp)."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import mod_ref
import node_harness
from block_gpu import CONFIGS, bits, each_stream, mismatch, noise, statement
from mod_gpu import gpu_mod, lib_params, mod_stream

pytestmark = pytest.mark.gpu

CH = mod_ref.CHUNK
INVALID, UNSUPPORTED = -1, -2
SINE, TRIANGLE = mod_ref.SINE, mod_ref.TRIANGLE
FAST = (1 << 32) // 997        # an LFO period of 997 samples: every signal of a chunk or more sweeps the whole delay range, at no grid's pace
LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 3 * 4096 + 7)
# (delay, depth) and the run length L its feedback loop allows: min(64, floor(delay - depth) - 1)
SWEEPS = (((7.5, 5.5), 1), ((20.25, 3.0), 16), ((69.9, 4.0), 64), ((300.0, 96.0), 64), ((2969.5, 100.5), 64))


@pytest.fixture(scope="module")
def ref():
    return statement(mod_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("mod_ref/host_mod_node.cpp", str(tmp_path_factory.mktemp("host_mod_gpu")))


def same(got, want):
    return np.array_equal(bits(got), bits(want))


def test_sweeps_name_their_run_lengths():
    for (delay, depth), L in SWEEPS:
        assert mod_ref.sub_block(mod_ref.params(delay, depth, 0.9)) == L and mod_ref.sub_block(mod_ref.params(delay, depth, 0.0)) == 64
    assert mod_ref.params(2969.5, 100.5).delay + 100.5 == mod_ref.MAX_DELAY, "the reach to the ring's limit"


@pytest.mark.parametrize("g", (0.0, 0.9, -0.9))
@pytest.mark.parametrize("sweep", SWEEPS, ids=lambda s: f"{s[0][0]}-{s[0][1]}")
def test_lengths_and_delays(nae, ctx, ref, sweep, g):
    """2 streams of distinct content at every length, so every length occurs at every run length (1, 16 and 64; 64 again without feedback);
    voices, shape and layout change from length to length and from case to case, so that each (delay, depth, g) meets one and four voices,
    both shapes, mono and stereo with spread 0 and 0.5.  3 * 4096 + 7 wraps the ring three times"""
    (delay, depth), _ = sweep
    turn = SWEEPS.index(sweep) + (0, 1, 2)[(0.0, 0.9, -0.9).index(g)]
    rng = np.random.default_rng(int(delay * 100) + int(g * 10) + 50)
    for i, in_len in enumerate(LENGTHS):
        k = i + turn
        voices, shape = (1, 4)[k % 2], (SINE, TRIANGLE)[(k // 2) % 2]
        ch, phase_ch = ((1, 0), (2, 0), (2, 1 << 30))[k % 3]
        p = mod_ref.params(delay, depth, g, 0.6, 0.8, FAST, 0x9e3779b9, phase_ch, mod_ref.spread_voices(voices), shape)
        x = noise(rng, 2, in_len, ch)
        got = gpu_mod(nae, ctx, p, x)
        want = mod_ref.run_streams(ref, p, x)
        assert same(got, want), (in_len, voices, shape, ch, phase_ch, int(np.sum(bits(got) != bits(want))))


def test_sub_block_independence(nae, ctx, ref):
    """mod_sub = 1, 7, 16, 33 and 64 at (300, 96), g = 0.9, four voices: the default's bits, which are the statement's; a cap above the rule's
    run length is cut down to it (L = 16 under mod_sub = 33)"""
    rng = np.random.default_rng(20)
    p = mod_ref.params(300.0, 96.0, 0.9, 0.6, 0.8, FAST, 5, 1 << 30, mod_ref.spread_voices(4))
    short = mod_ref.params(20.25, 3.0, -0.9, 0.6, 0.8, FAST, 5, 1 << 30, mod_ref.spread_voices(2), TRIANGLE)
    x = noise(rng, 2, 4097 + 1024 + 33, 2)
    want, want_short = mod_ref.run_streams(ref, p, x), mod_ref.run_streams(ref, short, x)
    try:
        for sub in (0, 1, 7, 16, 33, 64):
            ctx.debug_set("mod_sub", sub)
            assert same(gpu_mod(nae, ctx, p, x), want), sub
            assert same(gpu_mod(nae, ctx, short, x), want_short), sub
    finally:
        ctx.debug_set("mod_sub", 0)
    lib = ctx.lib
    assert lib.nae_debug_set(ctx.h, b"mod_sub", -1) == INVALID and lib.nae_debug_set(ctx.h, b"mod_sub", 65) == INVALID
    assert lib.nae_debug_set(ctx.h, b"mod_subs", 1) == INVALID


def test_views(nae, ctx, ref):
    """mono and stereo, interleaved and planar on either side, stream_stride 0, guard words behind every destination signal and NaN outside
    the source's signals; a base that is 4-byte aligned and no more; in place"""
    rng = np.random.default_rng(30)
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        p = mod_ref.params(300.0, 96.0, (0.8, 0.0)[i % 2], 0.5, 0.7, FAST, 7, 1 << 30, mod_ref.spread_voices(3), (SINE, TRIANGLE)[i // 2 % 2])
        x = noise(rng, n_streams, 2 * CH + 77, ch, shared)
        got = gpu_mod(nae, ctx, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0)
        assert same(got, mod_ref.run_streams(ref, p, x)), (ch, n_streams, sl, dl, shared)
    p = mod_ref.params(20.25, 3.0, 0.8, 0.5, 0.7, FAST, 7, 1 << 30, mod_ref.spread_voices(2))
    x = noise(rng, 2, 3 * CH + 9, 2)
    want = mod_ref.run_streams(ref, p, x)
    for layout in ("i", "p"):
        assert same(gpu_mod(nae, ctx, p, x, layout, layout, offset=3, chan_pad=2 if layout == "p" else 0), want), layout
    # in place: the destination is the source, interleaved and planar; a wave has read a chunk before it stores it
    n = x.shape[1]
    lp = lib_params(nae, p)
    for layout in ("i", "p"):
        host = x.reshape(2, -1) if layout == "i" else np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(2, -1)
        d = ctx.array(host.reshape(-1))
        sig = nae.Sig.interleaved(d.ptr, n, 2) if layout == "i" else nae.Sig.planar(d.ptr, n, 2)
        ctx.mod_block(lp, sig, n, 2, 2, sig)
        out = d.download()
        d.free()
        got = out.reshape(2, n, 2) if layout == "i" else out.reshape(2, 2, n).transpose(0, 2, 1)
        assert same(got, want), ("in place", layout)


@pytest.fixture(scope="module")
def streamed(nae, ctx, ref):
    """x[3 * 4096 + 7, 2] through a flanger at L = 16 with two voices and spread: the block call's result, the statement's bits"""
    p = mod_ref.params(24.0, 7.0, 0.9, 0.6, 0.8, FAST, 3, 1 << 30, mod_ref.spread_voices(2))
    x = noise(np.random.default_rng(60), 1, 3 * 4096 + 7, 2)
    block = gpu_mod(nae, ctx, p, x)[0]
    assert same(block, mod_ref.run_streams(ref, p, x)[0])
    return p, x[0], block


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("put", (1023, 1025, 4096 + 7, "everything"))
def test_handle_equals_the_block_call(nae, ctx, streamed, put, device):
    """any cut of the input into puts, from host or device memory, gives the block call's bits: phases and runs are absolute"""
    p, x, block = streamed
    got = mod_stream(nae, ctx, p, x, (len(x) if put == "everything" else put,), device=device)
    assert got.shape == block.shape and same(got, block)


@pytest.mark.parametrize("ch", (1, 2))
def test_handle_one_frame_puts(nae, ctx, ref, ch):
    """puts of one frame: 2 * 1024 + 600 of them at the deepest reach (the third chunk's taps read what the first launch kept), host and
    device in turn; the partial chunk is released by the flush alone"""
    p = mod_ref.params(2000.0, 1070.0, -0.9, 0.7, 0.7, FAST, 9, 1 << 31, mod_ref.spread_voices(4), TRIANGLE)
    x = noise(np.random.default_rng(70 + ch), 1, 2 * 1024 + 600, ch)
    got = mod_stream(nae, ctx, p, x[0], (1,), device=(False, True))
    assert same(got, mod_ref.run_streams(ref, p, x)[0])


def test_handle_deferred_receives_and_pieces(nae, ctx, streamed):
    """nothing received before the flush, mixed put sizes; and one put of everything received device to device in pieces of 1000 frames"""
    p, x, block = streamed
    assert same(mod_stream(nae, ctx, p, x, (1, 1023, 1025, 4096 + 7, 2500), device=(True, False), defer=True), block)
    d_out = ctx.array(np.zeros(1000 * 2, np.float32))
    got = mod_stream(nae, ctx, p, x, (len(x),), device=True, d_out=d_out, piece=1000)
    d_out.free()
    assert same(got, block)


def test_handle_long_stream(nae, ctx, ref):
    """400 000 frames through one handle at g = 0.9, in seeded random puts of 1 ... 9000 frames from the device and the host in turn: the input
    FIFO fills, compacts and grows, the line crosses some ninety launches, and the LFO at 997 samples a turn wraps 2^32 four hundred times.
    Against the block call on sampled windows and the last 5000 frames; the block call is the statement's there"""
    p = mod_ref.params(144.0, 48.0, 0.9, 0.7, 1.0, FAST, 11, 1 << 30)
    n = 400000
    x = noise(np.random.default_rng(80), 1, n, 2)
    block = gpu_mod(nae, ctx, p, x)[0]
    puts = tuple(int(k) for k in np.random.default_rng(81).integers(1, 9001, 128))
    got = mod_stream(nae, ctx, p, x[0], puts, device=(True, False))
    assert got.shape == block.shape
    want = mod_ref.run(ref, p, x[0])
    windows = [(int(s), int(s) + 3000) for s in np.random.default_rng(82).integers(0, n - 3000, 12)] + [(0, 5000), (n - 5000, n)]
    for a, b in windows:
        assert same(got[a:b], block[a:b]), ("the handle against the block call", a, b)
        assert same(block[a:b], want[a:b]), ("the block call against the statement", a, b)


def test_batch_overfills_the_chip(nae, ctx, ref):
    """4099 stereo streams x 2049 samples in one call: 8198 waves, more than the chip holds at once, so the launch runs in several rounds; every
    stream is compared"""
    n_streams, n = 4099, 2049
    p = mod_ref.params(24.0, 7.0, 0.9, 0.6, 0.8, FAST, 1, 1 << 30, mod_ref.spread_voices(2))
    x = np.random.default_rng(90).uniform(-1, 1, (n_streams, n, 2)).astype(np.float32)
    want = each_stream(lambda s: mod_ref.run(ref, p, x[s]), n_streams)
    assert not np.array_equal(want[0], want[1]) and np.all(np.isfinite(want))
    message = mismatch(gpu_mod(nae, ctx, p, x), want)
    assert not message, message


def test_nan_stays_in_its_stream_channel(nae, ctx, ref):
    """a NaN at one sample of one stream-channel: that stream-channel is the statement's — NaN at the same positions (its sign and payload
    differ between the CPU and the GPU), equal bits elsewhere; no sample in front of it changes; its sibling channel and the other streams
    have the clean run's bits"""
    p = mod_ref.params(24.0, 7.0, 0.9, 0.6, 0.8, FAST, 1, 1 << 30, mod_ref.spread_voices(2))
    i = CH + 5
    x = noise(np.random.default_rng(100), 3, 3 * CH + 100, 2)
    clean = gpu_mod(nae, ctx, p, x)
    dirty_x = x.copy()
    dirty_x[1, i, 0] = np.nan
    got = gpu_mod(nae, ctx, p, dirty_x)
    assert same(got[0], clean[0]) and same(got[2], clean[2]), "another stream changed"
    assert same(got[1, :, 1], clean[1, :, 1]), "the sibling channel changed"
    assert same(got[1, :i], clean[1, :i]), "samples before the NaN changed"
    want = mod_ref.run_streams(ref, p, dirty_x)[1]
    nan_g, nan_w = np.isnan(got[1]), np.isnan(want)
    assert np.array_equal(nan_g, nan_w) and nan_g[i, 0] and nan_g.sum() > 2
    assert np.array_equal(bits(got[1])[~nan_g], bits(want)[~nan_w])


def test_two_contexts_from_two_threads(nae, ref):
    """each thread creates, drives and destroys a context of its own, with its own parameters, at once"""
    x = noise(np.random.default_rng(110), 3, 3 * 1024 + 3, 2)
    ps = [mod_ref.params(300.0, 96.0, 0.9, 0.6, 0.8, FAST, 1, 1 << 30, mod_ref.spread_voices(4)),
          mod_ref.params(20.25, 3.0, -0.8, 1.0, 0.5, FAST, 2, 0, mod_ref.spread_voices(1), TRIANGLE)]
    out, errors = {}, []

    def worker(k):
        try:
            c = nae.Context(0)
            try:
                for _ in range(3):
                    out[k] = gpu_mod(nae, c, ps[k], x)
                    out[k + 2] = mod_stream(nae, c, ps[k], x[0], (777,))
            finally:
                c.close()
        except Exception as e:                                         # noqa: BLE001 — reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    for k in range(2):
        want = mod_ref.run_streams(ref, ps[k], x)
        assert same(out[k], want) and same(out[k + 2], want[0]), k


def test_errors(nae, ctx, ref):
    """the entries answer as the statement's check does (tests/test_mod_cpu.py walks it); a rejected call stores nothing"""
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)

    def block(p, ch=1, n=16, streams=1, src=C.byref(sig), dst=C.byref(sig)):
        return lib.nae_mod_block_f32(ctx.h, C.byref(p), src, n, ch, streams, dst)

    def create(p, ch=1):
        """the create entry's code; a failure hands no handle out"""
        h = C.c_void_p()
        rc = lib.nae_mod_create(ctx.h, C.byref(p), ch, C.byref(h))
        assert bool(h.value) == (rc == 0)
        if not rc:
            lib.nae_mod_destroy(h)
        return rc

    def both(ch=1, **kw):
        args = dict(delay=1536.0, depth=1534.0, feedback=0.95, wet=-3.0, dry=1e6, voice_phase=(1, 2, 3, 4), shape=TRIANGLE)
        args.update(kw)
        sp = mod_ref.params(**args)
        p = lib_params(nae, sp)
        rc = block(p, ch, n=0)
        assert rc == create(p, ch) == ref.ref_mod_check(C.byref(sp), ch), (ch, kw)
        if rc:
            assert block(p, ch) == rc, (ch, kw)
        return rc

    good = lib_params(nae, mod_ref.params(20.0, 5.0, 0.5))
    assert both() == 0 and both(ch=2) == 0 and both(feedback=-0.95) == 0 and both(depth=0.0) == 0
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    assert both(ch=0) == INVALID and both(ch=3) == INVALID
    for key in ("delay", "depth", "feedback", "wet", "dry"):
        assert both(**{key: float("nan")}) == INVALID and both(**{key: float("inf")}) == INVALID, key
    assert both(feedback=0.9501) == INVALID and both(feedback=-1.0) == INVALID
    assert both(depth=-1e-9) == INVALID
    assert both(n_voices=0) == INVALID and both(n_voices=-3) == INVALID and both(n_voices=5) == UNSUPPORTED
    assert both(shape=2) == INVALID and both(shape=-1) == INVALID
    for delay, depth in ((1536.0, 1534.5), (1.99, 0.0), (3070.5, 0.0), (3000.0, 70.5), (0.0, 0.0)):
        assert both(delay=delay, depth=depth) == UNSUPPORTED, (delay, depth)
    for delay, depth in ((2.0, 0.0), (3070.0, 0.0), (3000.0, 70.0)):
        assert both(delay=delay, depth=depth) == 0, (delay, depth)
    assert block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert lib.nae_mod_block_f32(ctx.h, None, C.byref(sig), 16, 1, 1, C.byref(sig)) == INVALID
    h = C.c_void_p()
    assert lib.nae_mod_create(ctx.h, None, 1, C.byref(h)) == INVALID and lib.nae_mod_create(ctx.h, C.byref(good), 1, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download(), np.zeros(64, np.float32)), "no rejected or empty call stored a sample"
    d.free()


def test_host_node_graph(host):
    """source -> audio_modulation -> sink with 1152-sample frames: the default chorus in stereo and mono, the flanger on the triangle and the
    vibrato: the source's frames, sizes and pts; the block call's samples with the designed parameters"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MOD OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_first_frame_errors(host):
    """a delay range outside 2 ... 3070 samples at the stream's sample rate is a Runtime_error on the first frame (the node opens its context
    first, so the mode needs a device)"""
    r = subprocess.run([host, "range"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MOD OK range" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
