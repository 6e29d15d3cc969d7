"""K12 dynamics on the GPU, bit for bit against the CPU statement (tests/dyn_ref/ref_dyn.c): every length around the lane, the wave and the chunk
at every look-ahead, every view, linked and unlinked detectors, hard and soft knee, limiter and compressor, a launch of 300 chunks, the
streaming handle in short and in long streams, non-finite, subnormal and zero input, two contexts from two threads, the error codes, and the host node (tests/dyn_ref/host_dyn_node.cpp)."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import dyn_ref
import node_harness
from block_gpu import CONFIGS, bits, statement
from dyn_gpu import dyn_stream, gpu_dyn, lib_params

pytestmark = pytest.mark.gpu

T, CH = dyn_ref.LANE, dyn_ref.CHUNK
LOOKAHEADS = (0, 1, 15, 16, 17, 63, 64, 1023, 1024)
INVALID, UNSUPPORTED, STATE = -1, -2, -5
MID = dict(alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05))


@pytest.fixture(scope="module")
def ref():
    return statement(dyn_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dyn_ref/host_dyn_node.cpp", str(tmp_path_factory.mktemp("host_dyn_gpu")))


def loud(rng, n_streams, n, ch, shared=False):
    """noise whose level wanders from far under to far over the -18 dB threshold, another phase per stream and channel"""
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * 10.0 ** ((-18.0 + 14.0 * np.sin(2 * np.pi * t / 411.0 + ph)) / 20.0)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


@pytest.mark.parametrize("la", LOOKAHEADS)
def test_lengths_and_lookaheads(nae, ctx, ref, la):
    """the lane edge, the wave edge, the chunk edge, a look-ahead that reaches into the zero padding and across one full chunk"""
    rng = np.random.default_rng(100 + la)
    for in_len in (1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH - 1 + la, 3 * CH + 7):
        for link, ch in ((1, 2), (0, 1)):
            p = dyn_ref.params(lookahead=la, link=link, **MID)
            x = loud(rng, 2, in_len, ch)
            want = dyn_ref.run_streams(ref, p, x)
            got = gpu_dyn(nae, ctx, p, x)
            assert np.array_equal(bits(got), bits(want)), (in_len, la, link, ch, int(np.sum(bits(got) != bits(want))))


VARIANTS = {"soft-compressor": dict(knee_db=6.0, slope=0.75, **MID), "hard-limiter": dict(knee_db=0.0, slope=1.0, **MID),
            "no-attack": dict(knee_db=3.0, slope=0.5, alpha_attack=0.0, alpha_release=dyn_ref.alpha(0.05)),
            "brick-wall": dict(knee_db=0.0, slope=1.0, makeup_db=3.0, **dyn_ref.FAST), "slow": dict(knee_db=12.0, slope=0.9, **dyn_ref.SLOW)}


@pytest.mark.parametrize("variant", VARIANTS)
def test_views_and_parameters(nae, ctx, ref, variant):
    """mono, stereo linked and unlinked; interleaved and planar on either side, stream_stride 0, odd offsets, gaps; 3 streams of distinct content"""
    rng = np.random.default_rng(len(variant))
    in_len = CH + 3 * T + 5
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        for link in (0, 1):
            p = dyn_ref.params(lookahead=(0, 17, 200)[i % 3], link=link, **VARIANTS[variant])
            x = loud(rng, n_streams, in_len, ch, shared)
            want = dyn_ref.run_streams(ref, p, x)
            got = gpu_dyn(nae, ctx, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
            assert np.array_equal(bits(got), bits(want)), (ch, n_streams, sl, dl, shared, link, int(np.sum(bits(got) != bits(want))))
            if link and ch == 2:
                assert not np.array_equal(bits(want), bits(dyn_ref.run_streams(ref, dyn_ref.params(lookahead=p.lookahead, link=0, **VARIANTS[variant]), x))), \
                    "the link changes the result: the case tests it"


def test_larger_launch(nae, ctx, ref):
    """40 stereo streams x (2 C + 5): 40 linked waves, 80 unlinked ones, each a workgroup of its own"""
    x = loud(np.random.default_rng(40), 40, 2 * CH + 5, 2)
    for link in (1, 0):
        p = dyn_ref.params(lookahead=96, link=link, **MID)
        assert np.array_equal(bits(gpu_dyn(nae, ctx, p, x, "p", "i", chan_pad=1)), bits(dyn_ref.run_streams(ref, p, x)))


@pytest.mark.parametrize("link", (1, 0))
def test_long_launch(nae, ctx, ref, link):
    """two stereo streams of 300 C + 7 samples, planar in and interleaved out, the slowest attack and release and the longest look-ahead: one
    wave per detector walks 301 chunks, and the smoothed level it carries from chunk to chunk has a memory of hundreds of them"""
    p = dyn_ref.params(lookahead=1024, link=link, **dyn_ref.SLOW)
    x = loud(np.random.default_rng(300 + link), 2, 300 * CH + 7, 2)
    got = gpu_dyn(nae, ctx, p, x, "p", "i", chan_pad=3)
    want = dyn_ref.run_streams(ref, p, x)
    assert np.array_equal(bits(got), bits(want)), int(np.sum(bits(got) != bits(want)))


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("put", (1, 7, 1000, 1024, 1025, 5000))
def test_handle_equals_the_block_call(nae, ctx, ref, put, la):
    """any cut of the input into puts gives the same bits; `available` follows floor((put - la) / 1024) chunks after every put"""
    # one-frame and seven-frame puts: short signals; 5000-frame puts: two of them and a rest, so a launch of several chunks is continued
    # from the carries it left
    in_len = {1: 700, 7: 1500, 5000: 2 * 5000 + CH + 300}.get(put, 3 * CH + 7)
    ch, link = (1, 0) if put in (7, 1024) else (2, 1 if put != 1000 else 0)
    p = dyn_ref.params(lookahead=la, link=link, **MID)
    x = loud(np.random.default_rng(put + la), 1, in_len, ch)
    block = gpu_dyn(nae, ctx, p, x)[0]
    assert np.array_equal(bits(block), bits(dyn_ref.run_streams(ref, p, x)[0]))
    for device in (False, True):
        got = dyn_stream(nae, ctx, p, x[0], (put,), device=device)
        assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block)), device


def test_handle_mixed_puts(nae, ctx, ref):
    p = dyn_ref.params(lookahead=300, link=1, **MID)
    x = loud(np.random.default_rng(77), 1, 4 * CH + 300, 2)
    want = dyn_ref.run_streams(ref, p, x)[0]
    for puts, device in (((1, 7, 1023, 1025, 2500), False), ((1025, 1, 1022, 7), True), ((CH,), False), ((5 * CH,), True), ((2 * CH + 40, 3, CH), True)):
        assert np.array_equal(bits(dyn_stream(nae, ctx, p, x[0], puts, device)), bits(want)), puts


@pytest.fixture(scope="module")
def long_stream(nae, ctx, ref):
    """x[100 000, 2] (three times what a handle's FIFOs start with), the slowest attack and release, look-ahead 1024, linked: the block
    call's result, the statement's bits"""
    p = dyn_ref.params(lookahead=1024, link=1, **dyn_ref.SLOW)
    x = loud(np.random.default_rng(100000), 1, 100000, 2)
    block = gpu_dyn(nae, ctx, p, x)[0]
    assert np.array_equal(bits(block), bits(dyn_ref.run_streams(ref, p, x)[0]))
    puts = tuple(int(k) for k in np.random.default_rng(9000).integers(1, 9001, 64))
    return p, x[0], block, puts


@pytest.mark.parametrize("drive", ("received after every put", "received after the flush", "one put, received in pieces"))
def test_handle_long_stream(nae, ctx, long_stream, drive):
    """100 000 frames through a handle give the block call's bits, and `available` follows floor((put - 1024) / 1024) chunks after every
    put (dyn_stream asserts it).  Seeded random puts of 1 ... 9000 frames, from the device and the host in turn: the input FIFO, which
    keeps the look-ahead, runs out of room again and again and moves its live rest to the front in place, and the carries cross some twenty
    launches; the same with nothing received before the flush: the output FIFO grows twice while all of it is live; one put of
    everything, received device to device in pieces of 4096 frames"""
    p, x, block, puts = long_stream
    if drive == "one put, received in pieces":
        d_out = ctx.array(np.zeros(4096 * 2, np.float32))
        got = dyn_stream(nae, ctx, p, x, (len(x),), device=True, d_out=d_out, piece=4096)
        d_out.free()
    else:
        got = dyn_stream(nae, ctx, p, x, puts, device=(True, False), defer=drive == "received after the flush")
    assert got.shape == block.shape and np.array_equal(bits(got), bits(block)), int(np.sum(bits(got) != bits(block)))


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_does_not_reach_back(nae, ctx, bad, la):
    """a non-finite sample at 2 C + 5: every sample before it by more than the look-ahead has the clean run's bits, the other stream is
    untouched, the call returns NAE_OK and the sentinels around the destination stand (gpu_dyn checks them)"""
    i = 2 * CH + 5
    p = dyn_ref.params(lookahead=la, link=1, **MID)
    x = loud(np.random.default_rng(9), 2, 3 * CH + 40, 2)
    clean = gpu_dyn(nae, ctx, p, x, "p", "p", chan_pad=3)
    dirty_x = x.copy()
    dirty_x[0, i, 1] = bad
    got = gpu_dyn(nae, ctx, p, dirty_x, "p", "p", chan_pad=3)
    assert np.array_equal(bits(got[:, :i - la]), bits(clean[:, :i - la])), "samples before i - la changed"
    assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"


def test_zero_and_subnormal_input(nae, ctx, ref):
    """zeros in: zeros out; f32 subnormals in: the statement's bits, subnormals, and no NaN (a zero stands at -1000 dB, far under the knee)"""
    p = dyn_ref.params(lookahead=40, link=1, makeup_db=6.0, **MID)
    z = np.zeros((2, CH + 70, 2), np.float32)
    assert not np.any(gpu_dyn(nae, ctx, p, z))
    rng = np.random.default_rng(11)
    x = (rng.integers(-(1 << 22), 1 << 22, (2, CH + 70, 2)).astype(np.int32) & np.int32(-0x7f800001)).view(np.float32)
    x = np.ascontiguousarray(x)
    x[:, ::5] = 0.0
    assert np.all(np.abs(x) < np.finfo(np.float32).tiny) and np.count_nonzero(x) > x.size // 2
    want = dyn_ref.run_streams(ref, p, x)
    got = gpu_dyn(nae, ctx, p, x)
    assert not np.any(np.isnan(got)) and np.array_equal(bits(got), bits(want))
    assert np.count_nonzero(want) == np.count_nonzero(x) and np.all(np.abs(want) < 4 * np.finfo(np.float32).tiny), "the statement keeps subnormals"


def test_two_contexts_from_two_threads(nae, ref):
    """each thread creates, drives and destroys a context of its own, with its own parameters, at once"""
    x = loud(np.random.default_rng(61), 3, 2 * CH + 3, 2)
    ps = [dyn_ref.params(lookahead=33, link=1, **MID), dyn_ref.params(lookahead=500, link=0, knee_db=0.0, slope=1.0, **dyn_ref.FAST)]
    out, errors = {}, []

    def worker(k):
        try:
            c = nae.Context(0)
            try:
                for _ in range(3):
                    out[k] = gpu_dyn(nae, c, ps[k], x)
                    out[k + 2] = dyn_stream(nae, c, ps[k], x[0], (777,))
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
        want = dyn_ref.run_streams(ref, ps[k], x)
        assert np.array_equal(bits(out[k]), bits(want)) and np.array_equal(bits(out[k + 2]), bits(want[0])), k


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = dyn_ref.params()

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1):
        return lib.nae_dyn_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    assert block(good) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    h = C.c_void_p()
    for field, values in (("threshold_db", (-60.5, 0.5, np.nan)), ("slope", (-0.1, 1.1, np.inf)), ("knee_db", (-1.0, 24.5, np.nan)),
                          ("alpha_attack", (-0.1, 1.0, np.nan)), ("alpha_release", (-0.1, 1.0, np.inf)), ("makeup_db", (-24.5, 24.5, np.nan)),
                          ("lookahead", (-1,)), ("link", (2, -1))):
        for v in values:
            p = dyn_ref.params()
            setattr(p, field, v)
            assert block(p) == INVALID, (field, v)
            assert block(p, n=0) == INVALID, "checked before the empty call returns"
            assert lib.nae_dyn_create(ctx.h, C.byref(lib_params(nae, p)), 2, C.byref(h)) == INVALID and not h.value, (field, v)
    far = dyn_ref.params(lookahead=1025)
    assert block(far) == UNSUPPORTED and lib.nae_dyn_create(ctx.h, C.byref(lib_params(nae, far)), 2, C.byref(h)) == UNSUPPORTED and not h.value
    assert block(dyn_ref.params(lookahead=1024)) == 0
    assert lib.nae_dyn_create(ctx.h, None, 2, C.byref(h)) == INVALID
    assert lib.nae_dyn_create(ctx.h, C.byref(lib_params(nae, good)), 3, C.byref(h)) == INVALID
    assert lib.nae_dyn_create(ctx.h, C.byref(lib_params(nae, good)), 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host):
    """source -> audio_dynamics -> sink with 1152-sample frames: the source's frames, sizes and pts; the block call's samples with the
    designed parameters"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYN OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_lookahead_too_long(host):
    """a look-ahead of more than 1024 samples at the stream's rate is a Runtime_error on the first frame"""
    r = subprocess.run([host, "lookahead"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYN OK lookahead" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
