"""K11 biquad cascade on the GPU, bit for bit against the CPU statement (tests/eq_ref/ref_eq.c): every length around the lane and the chunk,
short and long cascades, every view, a launch of many workgroups, a launch of 300 chunks, the context's table cache under its three users
(nae_eq_block_f32, nae_echo_block_f32, nae_dynkey_block_f32), the streaming handle in short and in long streams, non-finite and subnormal
input, the error codes, and the host node (tests/eq_ref/host_eq_node.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import dyn_ref
import dynkey_ref
import echo_ref
import eq_ref
import node_harness
from block_gpu import CONFIGS, bits, noise, statement
from dynkey_gpu import lib_params as dynkey_params
from echo_gpu import lib_params as echo_params
from eq_gpu import eq_stream, gpu_eq

pytestmark = pytest.mark.gpu

T, CH = eq_ref.LANE, eq_ref.CHUNK
LENGTHS = (1, T - 1, T, CH - 1, CH, CH + 1, 3 * CH + 7)
INVALID, UNSUPPORTED, STATE = -1, -2, -5


@pytest.fixture(scope="module")
def ref():
    return statement(eq_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("eq_ref/host_eq_node.cpp", str(tmp_path_factory.mktemp("host_eq_gpu")))


@pytest.mark.parametrize("n_sections", (1, 2, 16))
@pytest.mark.parametrize("in_len", LENGTHS)
def test_lengths_cascades_and_views(nae, ctx, ref, in_len, n_sections):
    """mono and stereo, interleaved and planar on either side, stream_stride 0, 3 streams of distinct content"""
    coef = eq_ref.cascade(n_sections)
    rng = np.random.default_rng(1000 * n_sections + in_len)
    for ch, n_streams, sl, dl, shared in CONFIGS:
        x = noise(rng, n_streams, in_len, ch, shared)
        want = eq_ref.run_streams(ref, coef, x)
        got = gpu_eq(nae, ctx, coef, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0)
        assert np.array_equal(bits(got), bits(want)), (ch, n_streams, sl, dl, shared, int(np.sum(bits(got) != bits(want))))


@pytest.mark.parametrize("in_len", (T - 1, CH + 1, 3 * CH + 7))
def test_odd_base_address(nae, ctx, ref, in_len):
    """a base that is 4-byte aligned and no more, on both sides"""
    coef = eq_ref.cascade(2)
    rng = np.random.default_rng(in_len)
    for ch, layout in ((1, "i"), (2, "i"), (2, "p")):
        x = noise(rng, 3, in_len, ch)
        for offset in (1, 3):
            got = gpu_eq(nae, ctx, coef, x, layout, layout, offset=offset, chan_pad=2 if layout == "p" else 0)
            assert np.array_equal(bits(got), bits(eq_ref.run_streams(ref, coef, x))), (ch, layout, offset)


def test_hard_cascade(nae, ctx, ref):
    """16 sections, four of them 20 Hz / Q 10 / +12 dB bells: the carry over three chunk borders in its worst conditioning"""
    coef = eq_ref.hard_cascade()
    x = noise(np.random.default_rng(5), 2, 3 * CH + 7, 2)
    assert np.array_equal(bits(gpu_eq(nae, ctx, coef, x)), bits(eq_ref.run_streams(ref, coef, x)))


def test_larger_launch(nae, ctx, ref):
    """40 stereo streams x (2 C + 5): 80 waves, each a workgroup of its own"""
    coef = eq_ref.cascade(4)
    x = noise(np.random.default_rng(40), 40, 2 * CH + 5, 2)
    want = eq_ref.run_streams(ref, coef, x)
    assert np.array_equal(bits(gpu_eq(nae, ctx, coef, x)), bits(want))
    assert np.array_equal(bits(gpu_eq(nae, ctx, coef, x, "p", "i", chan_pad=1)), bits(want))


def low_two_tone(n):
    """20 Hz + 40 Hz at 48 kHz: what the hard cascade's bells, whose memory is tens of chunks long, respond to"""
    t = np.arange(n)
    return (0.5 * np.sin(2 * np.pi * 20 * t / 48000) + 0.3 * np.sin(2 * np.pi * 40 * t / 48000)).astype(np.float32)


@pytest.mark.parametrize("name", ("hard", "S16"))
def test_long_launch(nae, ctx, ref, name):
    """two stereo streams of 300 C + 7 samples, planar in and interleaved out: one wave per stream-channel walks 301 chunks, far into the
    steady state of the 20 - 60 Hz bells, where an error of the library's carry tables (made on the host, as the statement's, in
    double-double) has added up over the filter's memory; channel 1 carries the low two-tone on top of the noise"""
    coef = eq_ref.hard_cascade() if name == "hard" else eq_ref.cascade(16)
    in_len = 300 * CH + 7
    x = noise(np.random.default_rng(300), 2, in_len, 2)
    x[:, :, 1] += low_two_tone(in_len)
    got = gpu_eq(nae, ctx, coef, x, "p", "i", chan_pad=3)
    want = eq_ref.run_streams(ref, coef, x)
    assert np.array_equal(bits(got), bits(want)), int(np.sum(bits(got) != bits(want)))


def test_the_context_keeps_its_tables_and_takes_new_ones(nae, ctx, ref):
    x = noise(np.random.default_rng(6), 1, CH + 9, 2)
    a, b = eq_ref.cascade(3), eq_ref.cascade(5)[2:]
    for coef in (a, a, b, a):
        assert np.array_equal(bits(gpu_eq(nae, ctx, coef, x)), bits(eq_ref.run_streams(ref, coef, x)))


def cache_steps():
    """(entry, coefficients, what the step is there for): nae_eq_cached_block keeps one constant block per context, keyed by the last
    coefficients, and the equalizer, the echo (its loop filter) and the keyed dynamics (its key filter) all go through it"""
    a, b, other = eq_ref.cascade(4), eq_ref.cascade(6)[4:], eq_ref.cascade(9)[6:]
    return (("eq", a, "A"), ("echo", a, "A from another entry: a hit"), ("eq", a[:2], "A's first two: the bytes are a prefix, only the count differs"),
            ("dynkey", b, "B after A[:2]: a miss on the same count"), ("echo", None, "an echo without sections: it does not ask the cache"),
            ("dynkey", b, "B behind the echo without sections: a hit"), ("handle", other, "a handle with other coefficients: its upload waits for the stream"),
            ("echo", b, "B behind the handle: the handle's tables are its own"), ("eq", a, "A after B: a miss on another count"),
            ("dynkey", a[:2], "A then A[:2] from another entry"), ("echo", a[:2], "a hit"), ("eq", a, "the first set again"))


def cache_walk(nae, contexts, orders, x, key):
    """orders[k][i] is issued on contexts[k], step by step across the contexts, with no sync between the calls (the outputs are downloaded
    behind the last one) -> [k][i] the outputs of the block calls, None for a handle's step"""
    n_streams, n, ch = x.shape
    dev = []
    for c, order in zip(contexts, orders):
        dev.append((c.array(x.reshape(-1)), c.array(key.reshape(-1)), [None if entry == "handle" else c.empty(x.size) for entry, _, _ in order]))
    handles = []
    try:
        for i in range(len(orders[0])):
            for c, order, (d_x, d_key, d_ys) in zip(contexts, orders, dev):
                entry, coef, _ = order[i]
                if entry == "handle":
                    handles.append(nae.Eq(c, coef, ch))
                    continue
                src, ksig, dst = (nae.Sig.interleaved(d.ptr, n, ch) for d in (d_x, d_key, d_ys[i]))
                if entry == "eq":
                    c.eq_block(coef, src, n, ch, n_streams, dst)
                elif entry == "echo":
                    c.echo_block(echo_params(nae, cache_echo(coef)), src, n, ch, n_streams, dst)
                else:
                    c.dynkey_block(dynkey_params(nae, cache_dynkey(coef)), src, ksig, n, ch, n_streams, dst)
        return [[None if d is None else d.download().reshape(x.shape) for d in d_ys] for _, _, d_ys in dev]
    finally:
        for h in handles:
            h.close()
        for d_x, d_key, d_ys in dev:
            for d in [d_x, d_key] + [d for d in d_ys if d is not None]:
                d.free()


def cache_echo(coef):
    return echo_ref.params((1024, 1500), 0.5, 1, 0.6, 0.8, () if coef is None else coef)


def cache_dynkey(coef):
    return dynkey_ref.params(dyn_ref.params(lookahead=17, link=1, alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05)), 2, coef)


def test_the_table_cache_under_its_three_users(nae, ctx):
    """every call of the walk equals the statement for ITS coefficients: on one context, then on that context and a second one whose walk is
    three steps ahead, call by call, so that each context must keep its own tables (tests/test_gpu_multi_ctx.py does this for the FIR filter)"""
    rng = np.random.default_rng(61)
    x = noise(rng, 2, 2 * 3072 + 7, 2)
    key = noise(rng, 2, 2 * 3072 + 7, 2)
    steps = cache_steps()
    refs = {"eq": statement(eq_ref), "echo": statement(echo_ref), "dynkey": statement(dynkey_ref)}

    def want(entry, coef):
        if entry == "eq":
            return eq_ref.run_streams(refs["eq"], coef, x)
        if entry == "echo":
            return echo_ref.run_streams(refs["echo"], cache_echo(coef), x)
        return dynkey_ref.run_streams(refs["dynkey"], cache_dynkey(coef), x, key)

    wants = {what: want(entry, coef) for entry, coef, what in steps if entry != "handle"}
    distinct = {bits(w).tobytes() for w in wants.values()}
    assert len(distinct) == len({(e, None if c is None else c.tobytes()) for e, c, _ in steps if e != "handle"}), "other coefficients, other bits"

    def check(got, order, label):
        for i, (entry, coef, what) in enumerate(order):
            if entry != "handle":
                w = wants[what]
                assert np.array_equal(bits(got[i]), bits(w)), (label, i, entry, what, int(np.sum(bits(got[i]) != bits(w))))

    check(cache_walk(nae, [ctx], [steps], x, key)[0], steps, "one context")
    second = nae.Context(0)
    try:
        ahead = steps[3:] + steps[:3]
        got = cache_walk(nae, [ctx, second], [steps, ahead], x, key)
        check(got[0], steps, "first of two contexts")
        check(got[1], ahead, "second of two contexts")
    finally:
        second.close()


@pytest.mark.parametrize("ch", (1, 2))
@pytest.mark.parametrize("put", (1, 7, 1023, 1025, 2500))
def test_handle_equals_the_block_call(nae, ctx, ref, put, ch):
    """any cut of the input into puts gives the same bits"""
    in_len = 600 if put == 1 else 3 * CH + 7       # one-frame puts: a partial chunk, released by the flush alone
    coef = eq_ref.cascade(16 if put == 1025 else 3)
    x = noise(np.random.default_rng(put), 1, in_len, ch)
    block = gpu_eq(nae, ctx, coef, x)[0]
    assert np.array_equal(bits(block), bits(eq_ref.run_streams(ref, coef, x)[0]))
    got = eq_stream(nae, ctx, coef, x[0], (put,), device=put == 1023)
    assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block))


def test_handle_mixed_puts(nae, ctx, ref):
    coef = eq_ref.cascade(2)
    x = noise(np.random.default_rng(77), 1, 2 * CH + 300, 2)
    want = eq_ref.run_streams(ref, coef, x)[0]
    for puts, device in (((1, 7, 1023, 1025, 2500), False), ((1025, 1, 1022, 7), True), ((CH,), False), ((5 * CH,), True)):
        assert np.array_equal(bits(eq_stream(nae, ctx, coef, x[0], puts, device)), bits(want)), puts


@pytest.fixture(scope="module")
def long_stream(nae, ctx, ref):
    """x[100 000, 2] (three times what a handle's FIFOs start with) through the hard cascade: the block call's result, the statement's bits"""
    coef = eq_ref.hard_cascade()
    x = noise(np.random.default_rng(100000), 1, 100000, 2)
    x[0, :, 1] += low_two_tone(100000)
    block = gpu_eq(nae, ctx, coef, x)[0]
    assert np.array_equal(bits(block), bits(eq_ref.run_streams(ref, coef, x)[0]))
    puts = tuple(int(k) for k in np.random.default_rng(9000).integers(1, 9001, 64))
    return coef, x[0], block, puts


@pytest.mark.parametrize("drive", ("received after every put", "received after the flush", "one put, received in pieces"))
def test_handle_long_stream(nae, ctx, long_stream, drive):
    """100 000 frames through a handle give the block call's bits.  Seeded random puts of 1 ... 9000 frames, from the device and the host in
    turn: the input FIFO runs out of room again and again and moves its live rest to the front in place, and the carry of every section
    crosses some twenty launches; the same with nothing received before the flush: the output FIFO grows twice while all of it is live; one
    put of everything, received device to device in pieces of 4096 frames"""
    coef, x, block, puts = long_stream
    if drive == "one put, received in pieces":
        d_out = ctx.array(np.zeros(4096 * 2, np.float32))
        got = eq_stream(nae, ctx, coef, x, (len(x),), device=True, d_out=d_out, piece=4096)
        d_out.free()
    else:
        got = eq_stream(nae, ctx, coef, x, puts, device=(True, False), defer=drive == "received after the flush")
    assert got.shape == block.shape and np.array_equal(bits(got), bits(block)), int(np.sum(bits(got) != bits(block)))


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_does_not_reach_back(nae, ctx, ref, bad):
    """a non-finite sample at C + 5: every sample before it has the clean run's bits; from it on the statement's, a NaN for a NaN (its sign
    and payload differ between the CPU and the GPU)"""
    i = CH + 5
    coef = eq_ref.cascade(16)
    x = noise(np.random.default_rng(9), 2, 2 * CH + 40, 2)
    clean = gpu_eq(nae, ctx, coef, x)
    dirty_x = x.copy()
    dirty_x[0, i, 1] = bad
    got = gpu_eq(nae, ctx, coef, dirty_x)
    assert np.array_equal(bits(got[:, :i]), bits(clean[:, :i])), "samples before the non-finite one changed"
    assert np.array_equal(bits(got[1]), bits(clean[1])) and np.array_equal(bits(got[0, :, 0]), bits(clean[0, :, 0])), "another stream or channel changed"
    want = eq_ref.run_streams(ref, coef, dirty_x)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w) and not np.isfinite(got[0, i, 1])
    assert np.array_equal(bits(got)[~nan_g], bits(want)[~nan_w])


def test_subnormal_input_is_not_flushed(nae, ctx, ref):
    """f32 subnormals in, a gain near 1: subnormals out, as the statement's"""
    coef = np.stack([eq_ref.design("peak", 48000, 1000.0, 0.5, 1.0), eq_ref.design("highshelf", 48000, 8000.0, -0.5, 0.7071)])
    rng = np.random.default_rng(11)
    x = (rng.integers(-(1 << 22), 1 << 22, (2, CH + 70, 2)).astype(np.int32) & np.int32(-0x7f800001)).view(np.float32)
    x = np.ascontiguousarray(x)
    assert np.all(np.abs(x) < np.finfo(np.float32).tiny) and np.count_nonzero(x) > x.size // 2
    want = eq_ref.run_streams(ref, coef, x)
    assert np.count_nonzero(want) > want.size // 2 and np.all(np.abs(want) < 4 * np.finfo(np.float32).tiny), "the statement keeps subnormals"
    assert np.array_equal(bits(gpu_eq(nae, ctx, coef, x)), bits(want))


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = eq_ref.cascade(2)
    block = lambda coef, S, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1: lib.nae_eq_block_f32(ctx.h, coef, S, src, n, ch, streams, dst)
    assert block(good.ctypes.data, 2) == 0
    assert block(None, 2) == INVALID and block(good.ctypes.data, 2, src=None) == INVALID and block(good.ctypes.data, 2, dst=None) == INVALID
    assert block(good.ctypes.data, 0) == INVALID and block(good.ctypes.data, -1) == INVALID
    assert block(good.ctypes.data, 2, ch=0) == INVALID and block(good.ctypes.data, 2, ch=3) == INVALID
    many = np.tile(good[0], (17, 1))
    assert block(many.ctypes.data, 16) == 0 and block(many.ctypes.data, 17) == UNSUPPORTED
    assert block(good.ctypes.data, 2, n=0) == 0 and block(good.ctypes.data, 2, streams=0) == 0, "nothing to do: NAE_OK"
    h = C.c_void_p()
    for sec in eq_ref.BAD_SECTIONS:
        c = np.concatenate([good[0], np.array(sec, np.float64)])
        assert block(c.ctypes.data, 2) == INVALID, sec
        assert block(c.ctypes.data, 2, n=0) == INVALID, "checked before the empty call returns"
        assert lib.nae_eq_create(ctx.h, c.ctypes.data, 2, 2, C.byref(h)) == INVALID and not h.value, sec
    for sec in eq_ref.GOOD_SECTIONS:
        c = np.array(sec, np.float64)
        assert block(c.ctypes.data, 1) == 0, sec
    assert lib.nae_eq_create(ctx.h, None, 1, 2, C.byref(h)) == INVALID
    assert lib.nae_eq_create(ctx.h, good.ctypes.data, 0, 2, C.byref(h)) == INVALID
    assert lib.nae_eq_create(ctx.h, good.ctypes.data, 2, 3, C.byref(h)) == INVALID
    assert lib.nae_eq_create(ctx.h, many.ctypes.data, 17, 2, C.byref(h)) == UNSUPPORTED and not h.value
    assert lib.nae_eq_create(ctx.h, good.ctypes.data, 2, 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host):
    """source -> audio_eq -> sink with 1152-sample frames: the source's frames, sizes and pts; the block call's samples with the designed
    coefficients"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_wire(host):
    """an absent and an empty "bands" deliver the input's bits"""
    r = subprocess.run([host, "wire"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK wire" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_wire_passes_s16_as_it_came(host):
    """without bands a packed S16 stream of 2500 samples in frames of 1000 arrives as S16 frames of 1000 / 1000 / 500 with the source's pts and
    words (no kernel runs; the node still opens its context first, so the mode needs a device)"""
    r = subprocess.run([host, "wire_s16"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK wire_s16" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_band_at_nyquist(host):
    """a band at half the stream's sample rate is a Runtime_error on the first frame"""
    r = subprocess.run([host, "nyquist"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST EQ OK nyquist" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
