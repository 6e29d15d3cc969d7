"""K16 echo on the GPU, bit for bit against the CPU statement (tests/echo_ref/ref_echo.c): every length around the chunk, the delay and the
ring's wrap at delays on and off the chunk grid, equal and unequal per channel, with and without ping-pong and loop filter; the longest
delay; every view; identities through the public entries alone; the streaming handle under every put pattern; launch groups; a NaN that
stays in its stream; two contexts from two threads; the error codes; and the host node (tests/echo_ref/host_echo_node.cpp)."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import echo_ref
import node_harness
from block_gpu import CONFIGS, bits, noise, statement
from echo_gpu import echo_stream, gpu_echo, lib_params
from eq_gpu import gpu_eq

pytestmark = pytest.mark.gpu

CH = echo_ref.CHUNK
INVALID, UNSUPPORTED = -1, -2
FILTERS = echo_ref.loop_filters()
DELAYS = (1024, 1025, 1500, 4097)


@pytest.fixture(scope="module")
def ref():
    return statement(echo_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("echo_ref/host_echo_node.cpp", str(tmp_path_factory.mktemp("host_echo_gpu")))


def same(got, want):
    return np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("sections", (0, 1, 4))
@pytest.mark.parametrize("D", DELAYS)
def test_lengths_delays_and_channels(nae, ctx, ref, D, sections):
    """2 streams of distinct content; mono, stereo with equal and with unequal delays (either channel the longer), each stereo shape with and
    without cross.  D = 1024 with cross reads in every chunk what the sibling wave stored one iteration before; 3 R + 7 wraps the ring three
    times, at a sample inside a chunk whenever D is off the grid"""
    rng = np.random.default_rng(10 * D + sections)
    for ch, delay, cross in ((1, D, 0), (2, (D, D), 0), (2, (D, D), 1), (2, (D, D + 37), 1), (2, (D + 1100, D), 0), (2, (D + 1100, D), 1)):
        p = echo_ref.params(delay, -0.9 if cross else 0.9, cross, 0.6, 0.8, FILTERS[sections])
        R = echo_ref.ring(p, ch)
        for in_len in (1, 1023, 1024, 1025, D, D + 1, 2 * D + 1, 3 * R + 7):
            x = noise(rng, 2, in_len, ch)
            got = gpu_echo(nae, ctx, p, x)
            want = echo_ref.run_streams(ref, p, x)
            assert same(got, want), (ch, delay, cross, in_len, int(np.sum(bits(got) != bits(want))))


def test_longest_delay(nae, ctx, ref):
    """one mono stream at NAE_ECHO_MAX_DELAY with in_len = D + 1025: the ring's largest size, and the first repeat's first 1025 samples"""
    D = echo_ref.MAX_DELAY
    p = echo_ref.params(D, 0.7, 0, 0.5, 0.9, FILTERS[1])
    x = noise(np.random.default_rng(20), 1, D + 1025, 1)
    got = gpu_echo(nae, ctx, p, x)
    assert same(got, echo_ref.run_streams(ref, p, x))
    assert not same(got[0, D:], (0.9 * x[0, D:].astype(np.float64)).astype(np.float32)), "the repeat is there"


def test_views(nae, ctx, ref):
    """mono and stereo, interleaved and planar on either side, stream_stride 0, guard words behind every destination signal and NaN outside
    the source's signals"""
    rng = np.random.default_rng(30)
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        p = echo_ref.params((1500, 1030), 0.8, i % 2, 0.5, 0.7, FILTERS[2])
        in_len = 2 * echo_ref.ring(p, ch) + 7
        x = noise(rng, n_streams, in_len, ch, shared)
        got = gpu_echo(nae, ctx, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0)
        assert same(got, echo_ref.run_streams(ref, p, x)), (ch, n_streams, sl, dl, shared)
    # a base that is 4-byte aligned and no more, on both sides
    p = echo_ref.params(1025, 0.8, 1, 0.5, 0.7, FILTERS[1])
    x = noise(rng, 2, 3 * CH + 9, 2)
    for layout in ("i", "p"):
        assert same(gpu_echo(nae, ctx, p, x, layout, layout, offset=3, chan_pad=2 if layout == "p" else 0), echo_ref.run_streams(ref, p, x)), layout


@pytest.mark.parametrize("sections", (1, 4))
def test_first_repeat_is_the_equalizer(nae, ctx, sections):
    """through public entries only: D = 2048, dry = 0, wet = 1, any g and n sections: y[D : 2 D] is nae_eq_block_f32(x)[0 : D] — the first
    repeat has been round the loop once, through the filter, and the delayed signal's chunk grid is the input's"""
    D = 2048
    x = noise(np.random.default_rng(40 + sections), 2, 2 * D, 2)
    filtered = gpu_eq(nae, ctx, FILTERS[sections], x)
    for g, cross in ((0.9, 0), (-0.5, 0), (0.0, 0)):
        y = gpu_echo(nae, ctx, echo_ref.params(D, g, cross, 1.0, 0.0, FILTERS[sections]), x)
        assert np.array_equal(y[:, D:], filtered[:, :D]), (g, cross)
        assert np.all(y[:, :D] == 0.0)
    y = gpu_echo(nae, ctx, echo_ref.params(D, 0.9, 1, 1.0, 0.0, FILTERS[sections]), x)
    assert np.array_equal(y[:, D:], filtered[:, :D, ::-1]), "cross: the other channel's"


def test_no_loop_is_a_delay(nae, ctx):
    """through public entries only: no section and g = 0: y is the input delayed (values: 0 x + f may be a zero of either sign)"""
    x = noise(np.random.default_rng(50), 2, 3 * 1500 + 11, 2)
    for delay, cross in (((1500, 1024), 0), ((1024, 1500), 1)):
        y = gpu_echo(nae, ctx, echo_ref.params(delay, 0.0, cross, 1.0, 0.0), x)
        for c in range(2):
            s = 1 - c if cross else c
            assert np.all(y[:, :delay[c], c] == 0.0) and np.array_equal(y[:, delay[c]:, c], x[:, :x.shape[1] - delay[c], s]), (delay, cross, c)


@pytest.fixture(scope="module")
def streamed(nae, ctx, ref):
    """x[3 R + 7, 2] through ping-pong at delays 1024 and 1500 with two sections: the block call's result, the statement's bits"""
    p = echo_ref.params((1024, 1500), 0.9, 1, 0.6, 0.8, FILTERS[2])
    x = noise(np.random.default_rng(60), 1, 3 * echo_ref.ring(p, 2) + 7, 2)
    block = gpu_echo(nae, ctx, p, x)[0]
    assert same(block, echo_ref.run_streams(ref, p, x)[0])
    return p, x[0], block


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("put", (1023, 1025, 4096 + 7, "everything"))
def test_handle_equals_the_block_call(nae, ctx, streamed, put, device):
    """any cut of the input into puts, from host or device memory, gives the block call's bits: the chunks are absolute"""
    p, x, block = streamed
    got = echo_stream(nae, ctx, p, x, (len(x) if put == "everything" else put,), device=device)
    assert got.shape == block.shape and same(got, block)


@pytest.mark.parametrize("ch", (1, 2))
def test_handle_one_frame_puts(nae, ctx, ref, ch):
    """puts of one frame: 2 D + 600 of them at D = 1024 (three launches, a partial chunk released by the flush alone), host and device in turn"""
    p = echo_ref.params(1024, -0.9, 1, 0.7, 0.7, FILTERS[1])
    x = noise(np.random.default_rng(70 + ch), 1, 2 * 1024 + 600, ch)
    got = echo_stream(nae, ctx, p, x[0], (1,), device=(False, True))
    assert same(got, echo_ref.run_streams(ref, p, x)[0])


def test_handle_deferred_receives_and_pieces(nae, ctx, streamed):
    """nothing received before the flush, mixed put sizes; and one put of everything received device to device in pieces of 1000 frames"""
    p, x, block = streamed
    assert same(echo_stream(nae, ctx, p, x, (1, 1023, 1025, 4096 + 7, 2500), device=(True, False), defer=True), block)
    d_out = ctx.array(np.zeros(1000 * 2, np.float32))
    got = echo_stream(nae, ctx, p, x, (len(x),), device=True, d_out=d_out, piece=1000)
    d_out.free()
    assert same(got, block)


def test_launch_groups(nae, ctx, ref):
    """echo_group = 1 and 2 on 3 streams (one launch per group, every group on the workspace's first rings) equal the default"""
    p = echo_ref.params((1500, 1024), 0.9, 1, 0.6, 0.8, FILTERS[4])
    x = noise(np.random.default_rng(80), 3, 2 * echo_ref.ring(p, 2) + 7, 2)
    want = echo_ref.run_streams(ref, p, x)
    try:
        for group in (0, 1, 2):
            ctx.debug_set("echo_group", group)
            assert same(gpu_echo(nae, ctx, p, x), want), group
            assert same(gpu_echo(nae, ctx, p, x, "p", "i", chan_pad=3), want), group
    finally:
        ctx.debug_set("echo_group", 0)
    lib = ctx.lib
    assert lib.nae_debug_set(ctx.h, b"echo_group", -1) == INVALID and lib.nae_debug_set(ctx.h, b"echo_groups", 1) == INVALID


@pytest.mark.parametrize("cross", (0, 1))
def test_nan_stays_in_its_stream(nae, ctx, ref, cross):
    """a NaN at one sample of one stream: that stream is the statement's — NaN at the same positions (its sign and payload differ between the
    CPU and the GPU), equal bits elsewhere; no sample in front of it changes; the other streams have the clean run's bits"""
    p = echo_ref.params((1024, 1500), 0.9, cross, 0.6, 0.8, FILTERS[1])
    i = CH + 5
    x = noise(np.random.default_rng(90), 3, 4 * echo_ref.ring(p, 2), 2)
    clean = gpu_echo(nae, ctx, p, x)
    dirty_x = x.copy()
    dirty_x[1, i, 0] = np.nan
    got = gpu_echo(nae, ctx, p, dirty_x)
    assert same(got[0], clean[0]) and same(got[2], clean[2]), "another stream changed"
    assert same(got[1, :i], clean[1, :i]), "samples before the NaN changed"
    want = echo_ref.run_streams(ref, p, dirty_x)[1]
    nan_g, nan_w = np.isnan(got[1]), np.isnan(want)
    assert np.array_equal(nan_g, nan_w) and nan_g[i, 0] and nan_g.sum() > 2
    assert np.array_equal(bits(got[1])[~nan_g], bits(want)[~nan_w])
    if not cross:
        assert same(got[1, :, 1], clean[1, :, 1]), "without cross the other channel does not hear it"


def test_two_contexts_from_two_threads(nae, ref):
    """each thread creates, drives and destroys a context of its own, with its own parameters, at once"""
    x = noise(np.random.default_rng(100), 3, 3 * 3072 + 3, 2)
    ps = [echo_ref.params((1024, 1500), 0.9, 1, 0.6, 0.8, FILTERS[4]), echo_ref.params((2000, 1024), -0.8, 0, 1.0, 0.5, FILTERS[1])]
    out, errors = {}, []

    def worker(k):
        try:
            c = nae.Context(0)
            try:
                for _ in range(3):
                    out[k] = gpu_echo(nae, c, ps[k], x)
                    out[k + 2] = echo_stream(nae, c, ps[k], x[0], (777,))
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
        want = echo_ref.run_streams(ref, ps[k], x)
        assert same(out[k], want) and same(out[k + 2], want[0]), k


def test_errors(nae, ctx, ref):
    """the entries answer as the statement's check does (tests/test_echo_cpu.py walks it); a rejected call stores nothing"""
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)

    def block(p, ch=1, n=16, streams=1, src=C.byref(sig), dst=C.byref(sig)):
        return lib.nae_echo_block_f32(ctx.h, C.byref(p), src, n, ch, streams, dst)

    def create(p, ch=1):
        """the create entry's code; a failure hands no handle out"""
        h = C.c_void_p()
        rc = lib.nae_echo_create(ctx.h, C.byref(p), ch, C.byref(h))
        assert bool(h.value) == (rc == 0)
        if not rc:
            lib.nae_echo_destroy(h)
        return rc

    def both(ch=1, **kw):
        args = dict(delay=(1024, 1 << 20), feedback=0.99, cross=1, wet=-3.0, dry=1e6, coef=FILTERS[4])
        args.update(kw)
        sp = echo_ref.params(**args)
        p = lib_params(nae, sp)
        p.n_sections = sp.n_sections
        rc = block(p, ch)
        assert rc == create(p, ch) == block(p, ch, n=0) == ref.ref_echo_check(C.byref(sp), ch), (ch, kw)
        return rc

    good = lib_params(nae, echo_ref.params(1024, 0.5))
    assert both() == 0 and both(coef=()) == 0 and both(ch=2, delay=(1 << 20, 1024)) == 0
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    assert both(ch=0) == INVALID and both(ch=3) == INVALID
    for key in ("feedback", "wet", "dry"):
        assert both(**{key: float("nan")}) == INVALID and both(**{key: float("inf")}) == INVALID, key
    assert both(feedback=0.9901) == INVALID and both(feedback=-1.0) == INVALID and both(feedback=-0.99) == 0
    assert both(cross=2) == INVALID and both(cross=-1) == INVALID
    assert both(n_sections=-1) == INVALID and both(coef=np.repeat(FILTERS[1], 5, 0), n_sections=5) == UNSUPPORTED
    for bad in (1023, 0, -5, (1 << 20) + 1):
        assert both(delay=(bad, 2048)) == UNSUPPORTED and both(ch=2, delay=(2048, bad)) == UNSUPPORTED, bad
        assert both(ch=1, delay=(2048, bad)) == 0, "mono reads delay[0] alone"
    for section in ((1, 0, 0, 0, 1.0), (1, 0, 0, 1.5, 0.5), (float("nan"), 0, 0, 0, 0), (1, 0, 0, float("inf"), 0)):
        assert both(coef=np.array([FILTERS[1][0], section])) == INVALID, section
    assert block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert lib.nae_echo_block_f32(ctx.h, None, C.byref(sig), 16, 1, 1, C.byref(sig)) == INVALID
    h = C.c_void_p()
    assert lib.nae_echo_create(ctx.h, None, 1, C.byref(h)) == INVALID and lib.nae_echo_create(ctx.h, C.byref(good), 1, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[32:], np.zeros(32, np.float32)), "nothing behind the one stream's 16 frames of at most two channels"
    d.free()


def test_host_node_graph(host):
    """source -> audio_echo -> sink with 1152-sample frames, stereo ping-pong with two delays and both loop filters, stereo and mono at the
    defaults: the source's frames, sizes and pts; the block call's samples with the designed parameters"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST ECHO OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("mode", ("short", "nyquist"))
def test_host_node_first_frame_errors(host, mode):
    """a delay under 1024 or above 1048576 samples at the stream's sample rate, and a corner at or above Nyquist, are Runtime_errors on the
    first frame (the node opens its context first, so the modes need a device)"""
    r = subprocess.run([host, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"HOST ECHO OK {mode}" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
