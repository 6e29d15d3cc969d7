"""K13 spectral gate on the GPU, bit for bit against the CPU statement (tests/denoise_ref/ref_denoise.c): every length around the hop and the
frame at every smoothing width, every frame size, every tiling, every view, one profile for all channels and one per channel, a launch of many
streams and a launch of many blocks, the profile kernel, the streaming handle in short and in long streams, a non-finite sample, zero input, two
contexts from two threads, the error codes, and the host node (tests/denoise_ref/host_denoise_node.cpp).  Every parametrised case asserts on the
statement's own mask that between 20 % and 80 % of its decisions are open: otherwise the smoothing is not exercised."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import denoise_ref
import node_harness
from block_gpu import CONFIGS, bits, statement
from denoise_gpu import denoise_stream, gpu_denoise, gpu_profile, lib_params

pytestmark = pytest.mark.gpu

N0, H0 = 512, 128
WIDTHS = ((0, 0), (1, 1), (2, 2), (8, 4))
INVALID, UNSUPPORTED, STATE = -1, -2, -5


@pytest.fixture(scope="module")
def ref():
    return statement(denoise_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("denoise_ref/host_denoise_node.cpp", str(tmp_path_factory.mktemp("host_denoise_gpu")))


def wander(rng, n_streams, n, ch, n_fft=N0, shared=False):
    """noise whose level wanders +-14 dB around 1 with a period of three frames, another phase per stream and channel"""
    return denoise_ref.wander(rng, n_streams, n, ch, period=3.0 * n_fft, shared=shared)


class Share:
    """the open decisions of a case's statement runs, counted over all of them"""

    def __init__(self):
        self.open, self.all = 0, 0

    def want(self, ref, p, profile, x):
        out = []
        for s in x:
            y, d, _ = denoise_ref.run(ref, p, profile, s, detail=True)
            self.open += int(d.sum())
            self.all += d.size
            out.append(y)
        return np.stack(out)

    def check(self):
        assert 0.2 <= self.open / self.all <= 0.8, f"between a fifth and four fifths of the decisions are open: {self.open / self.all:.3f}"


@pytest.mark.parametrize("tn,fn", WIDTHS)
def test_lengths_and_smoothing_widths(nae, ctx, ref, tn, fn):
    """one sample, the hop's edge, the frame's edge, five blocks and a rest; mono against a flat profile, stereo against a tilted one per channel"""
    rng = np.random.default_rng(100 + 10 * tn + fn)
    share = Share()
    for in_len in (1, H0 - 1, H0, H0 + 1, N0, N0 + 1, 5 * H0 + 7):
        for ch, tilt in ((1, 0.0), (2, -6.0)):
            p = denoise_ref.params(N0, tn, fn, 0.25, 0.25)      # the frames of a short signal are mostly padding: a threshold 6 dB down
            profile = denoise_ref.flat_profile(N0, ch, tilt_db=tilt)
            x = wander(rng, 2, in_len, ch)
            want = share.want(ref, p, profile, x)
            got = gpu_denoise(nae, ctx, p, profile, x)
            assert np.array_equal(bits(got), bits(want)), (in_len, ch, int(np.sum(bits(got) != bits(want))))
    share.check()


@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_every_frame_size(nae, ctx, ref, n_fft):
    rng = np.random.default_rng(n_fft)
    share = Share()
    p = denoise_ref.params(n_fft, 2, 2, 1.0, 0.1)
    profile = denoise_ref.flat_profile(n_fft, 2, tilt_db=-3.0)
    x = wander(rng, 2, 6 * n_fft + 5, 2, n_fft)
    want = share.want(ref, p, profile, x)
    got = gpu_denoise(nae, ctx, p, profile, x, "p", "i", chan_pad=3)
    assert np.array_equal(bits(got), bits(want)), int(np.sum(bits(got) != bits(want)))
    share.check()


@pytest.mark.parametrize("tn,fn", ((2, 2), (8, 4)))
def test_every_tiling_gives_the_same_bits(nae, ctx, ref, tn, fn):
    """23 blocks cut into tiles of 1, 2, 3 and 7 blocks and by the library's pick: a tile's decision front starts cold Tn frames early"""
    rng = np.random.default_rng(23 + tn)
    share = Share()
    p = denoise_ref.params(N0, tn, fn, 1.0, 0.2)
    profile = denoise_ref.flat_profile(N0, 2, tilt_db=-6.0)
    x = wander(rng, 2, 23 * H0 - 5, 2)
    want = share.want(ref, p, profile, x)
    try:
        for tile in (1, 2, 3, 7, 0):
            ctx.debug_set("dn_tile", tile)
            got = gpu_denoise(nae, ctx, p, profile, x)
            assert np.array_equal(bits(got), bits(want)), (tile, int(np.sum(bits(got) != bits(want))))
    finally:
        ctx.debug_set("dn_tile", 0)
    share.check()


@pytest.mark.parametrize("n_fft,tn,fn", ((512, 2, 2), (1024, 1, 3)))
def test_views_and_profile_channels(nae, ctx, ref, n_fft, tn, fn):
    """mono and stereo; interleaved and planar on either side, stream_stride 0, odd offsets, gaps, channel padding; one profile for every
    channel and one per channel (view_call checks the guard words around every destination signal)"""
    rng = np.random.default_rng(n_fft + tn)
    share = Share()
    in_len = 5 * (n_fft // 4) + 7
    p = denoise_ref.params(n_fft, tn, fn, 1.0, 0.3)
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        per_channel = denoise_ref.flat_profile(n_fft, ch, tilt_db=-6.0)
        per_channel[-1] *= 2.0                                     # the last channel's profile stands 3 dB above the first's
        x = wander(rng, n_streams, in_len, ch, n_fft, shared)
        outs = []
        for profile in (per_channel, per_channel[:1]):
            want = share.want(ref, p, profile, x)
            got = gpu_denoise(nae, ctx, p, profile, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
            assert np.array_equal(bits(got), bits(want)), (ch, n_streams, sl, dl, shared, profile.shape[0], int(np.sum(bits(got) != bits(want))))
            outs.append(want)
        if ch == 2:
            assert not np.array_equal(bits(outs[0][:, :, 1]), bits(outs[1][:, :, 1])), "profile_ch changes the second channel: the case tests it"
    share.check()


@pytest.mark.parametrize("shape", ("40 stereo streams x 20 blocks", "2 streams x 300 blocks"))
def test_launch_sizes(nae, ctx, ref, shape):
    """80 stream-channels, ten workgroups of eight waves; and 300 blocks, which the library's pick cuts into tiles of 34"""
    rng = np.random.default_rng(len(shape))
    share = Share()
    n_streams, n = (40, 20 * H0 - 3) if shape.startswith("40") else (2, 300 * H0 - 9)
    p = denoise_ref.params(N0, 2, 2, 1.0, 0.25)
    profile = denoise_ref.flat_profile(N0, 2, tilt_db=-6.0)
    x = wander(rng, n_streams, n, 2)
    want = share.want(ref, p, profile, x)
    got = gpu_denoise(nae, ctx, p, profile, x, "p", "i", chan_pad=1)
    assert np.array_equal(bits(got), bits(want)), int(np.sum(bits(got) != bits(want)))
    share.check()


@pytest.mark.parametrize("n_fft", denoise_ref.SIZES)
def test_profile_kernel(nae, ctx, ref, n_fft):
    """one frame exactly, a hop less one more, 33 frames and a rest; mono interleaved, stereo interleaved and planar.  One sample short of a
    frame: NAE_ERR_INVALID"""
    rng = np.random.default_rng(7 * n_fft)
    H = n_fft // 4
    for length in (n_fft, n_fft + H - 1, 9 * n_fft + 3):
        for ch, layout in ((1, "i"), (2, "i"), (2, "p")):
            x = wander(rng, 1, length, ch, n_fft)[0]
            want = denoise_ref.profile(ref, n_fft, x)
            got = gpu_profile(nae, ctx, n_fft, x, layout)
            assert np.array_equal(bits(got), bits(want)), (length, ch, layout, int(np.sum(bits(got) != bits(want))))
            assert np.all(want > 0)
    assert denoise_ref.profile(ref, n_fft, np.zeros((n_fft - 1, 1), np.float32)) is None
    d = ctx.array(np.zeros(n_fft + n_fft // 2 + 1, np.float32))
    sig = nae.Sig(d.ptr, 0, 1, 1)
    assert ctx.lib.nae_denoise_profile_f32(ctx.h, n_fft, C.byref(sig), n_fft - 1, 1, d.at(n_fft)) == INVALID
    d.free()


@pytest.mark.parametrize("put", (1, 7, H0, H0 + 1, 5000))
def test_handle_equals_the_block_call(nae, ctx, ref, put):
    """any cut of the input into puts gives the block call's bits, from host and from device memory; `available` follows
    floor((put - (Tn + 3) H) / H) blocks after every put (denoise_stream asserts it)"""
    in_len = {1: 900, 7: 1500, 5000: 2 * 5000 + 300}.get(put, 11 * H0 + 7)
    ch, tn = (1, 1) if put in (7, H0) else (2, 2)
    rng = np.random.default_rng(put)
    share = Share()
    p = denoise_ref.params(N0, tn, 2, 1.0, 0.25)
    profile = denoise_ref.flat_profile(N0, ch, tilt_db=-6.0)
    x = wander(rng, 1, in_len, ch)
    want = share.want(ref, p, profile, x)[0]
    block = gpu_denoise(nae, ctx, p, profile, x)[0]
    assert np.array_equal(bits(block), bits(want))
    for device in (False, True):
        got = denoise_stream(nae, ctx, p, profile, x[0], (put,), device=device)
        assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block)), device
    share.check()


def test_handle_mixed_puts(nae, ctx, ref):
    p = denoise_ref.params(N0, 8, 4, 1.0, 0.25)
    profile = denoise_ref.flat_profile(N0, 2, tilt_db=-6.0)
    x = wander(np.random.default_rng(77), 1, 40 * H0 + 77, 2)
    want = denoise_ref.run_streams(ref, p, profile, x)[0]
    for puts, device in (((1, 7, 127, 129, 2500), False), ((1025, 1, 1022, 7), True), ((H0,), False), ((41 * H0,), True), ((11 * H0 + 40, 3, H0), True)):
        assert np.array_equal(bits(denoise_stream(nae, ctx, p, profile[:1], x[0], puts, device)),
                              bits(denoise_ref.run_streams(ref, p, profile[:1], x)[0])), puts
    assert np.array_equal(bits(denoise_stream(nae, ctx, p, profile, x[0], (777,), (True, False))), bits(want))


@pytest.fixture(scope="module")
def long_stream(nae, ctx, ref):
    """x[100 000, 2] (three times what a handle's FIFOs start with): the block call's result, the statement's bits"""
    p = denoise_ref.params(N0, 2, 2, 1.0, 0.25)
    profile = denoise_ref.flat_profile(N0, 2, tilt_db=-6.0)
    x = wander(np.random.default_rng(100000), 1, 100000, 2)
    block = gpu_denoise(nae, ctx, p, profile, x)[0]
    assert np.array_equal(bits(block), bits(denoise_ref.run_streams(ref, p, profile, x)[0]))
    puts = tuple(int(k) for k in np.random.default_rng(9000).integers(1, 9001, 64))
    return p, profile, x[0], block, puts


@pytest.mark.parametrize("drive", ("received after every put", "received after the flush"))
def test_handle_long_stream(nae, ctx, long_stream, drive):
    """100 000 frames through a handle in seeded random puts of 1 ... 9000 frames, from the device and the host in turn, give the block
    call's bits: the input FIFO, which keeps Tn + 3 blocks, moves its live rest to the front again and again; with nothing received before
    the flush the output FIFO grows while all of it is live"""
    p, profile, x, block, puts = long_stream
    got = denoise_stream(nae, ctx, p, profile, x, puts, device=(True, False), defer=drive == "received after the flush")
    assert got.shape == block.shape and np.array_equal(bits(got), bits(block)), int(np.sum(bits(got) != bits(block)))


@pytest.mark.parametrize("tn", (0, 2, 8))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_sample_stays_local(nae, ctx, bad, tn):
    """a non-finite sample at index i: the samples before (floor(i / H) - Tn - 3) H and from (floor(i / H) + Tn + 4) H on have the clean run's
    bits, the other stream is untouched, the call returns NAE_OK and the sentinels around the destination stand (gpu_denoise checks them)"""
    i = 20 * H0 + 5
    lo, hi = (i // H0 - tn - 3) * H0, (i // H0 + tn + 4) * H0
    p = denoise_ref.params(N0, tn, 2, 1.0, 0.25)
    profile = denoise_ref.flat_profile(N0, 2)
    x = wander(np.random.default_rng(9), 2, 40 * H0 + 40, 2)
    try:
        ctx.debug_set("dn_tile", 5)                        # tiles start inside, in front of and behind the sample's reach
        clean = gpu_denoise(nae, ctx, p, profile, x, "p", "p", chan_pad=3)
        dirty_x = x.copy()
        dirty_x[0, i, 1] = bad
        got = gpu_denoise(nae, ctx, p, profile, dirty_x, "p", "p", chan_pad=3)
    finally:
        ctx.debug_set("dn_tile", 0)
    assert lo > 0 and hi < x.shape[1]
    assert np.array_equal(bits(got[0, :lo]), bits(clean[0, :lo])), "samples in front of the sample's reach changed"
    assert np.array_equal(bits(got[0, hi:]), bits(clean[0, hi:])), "samples behind the sample's reach changed"
    assert np.array_equal(bits(got[0, :, 0]), bits(clean[0, :, 0])), "the other channel changed"
    assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"


def test_zero_input(nae, ctx):
    p = denoise_ref.params(N0, 2, 2, 1.0, 0.25)
    z = np.zeros((2, 5 * H0 + 7, 2), np.float32)
    assert not np.any(gpu_denoise(nae, ctx, p, denoise_ref.flat_profile(N0, 1), z))
    assert not np.any(gpu_denoise(nae, ctx, p, np.zeros((1, N0 // 2 + 1), np.float32), z)), "a zero profile: nothing is above it"


def test_two_contexts_from_two_threads(nae, ref):
    """each thread creates, drives and destroys a context of its own, with its own parameters and frame size, at once"""
    ps = [denoise_ref.params(512, 2, 2, 1.0, 0.25), denoise_ref.params(1024, 1, 4, 2.0, 0.5)]
    xs = [wander(np.random.default_rng(61 + k), 3, 9 * 256 + 3, 2, ps[k].n_fft) for k in range(2)]
    profiles = [denoise_ref.flat_profile(ps[k].n_fft, 2, tilt_db=-6.0) for k in range(2)]
    out, errors = {}, []

    def worker(k):
        try:
            c = nae.Context(0)
            try:
                for _ in range(3):
                    out[k] = gpu_denoise(nae, c, ps[k], profiles[k], xs[k])
                    out[k + 2] = denoise_stream(nae, c, ps[k], profiles[k], xs[k][0], (777,))
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
        want = denoise_ref.run_streams(ref, ps[k], profiles[k], xs[k])
        assert np.array_equal(bits(out[k]), bits(want)) and np.array_equal(bits(out[k + 2]), bits(want[0])), k


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    prof = ctx.array(np.ones(2 * 257, np.float32))
    sig, out_sig = nae.Sig(d.ptr, 0, 1, 1), nae.Sig(d.at(32), 0, 1, 1)
    good = denoise_ref.params()

    def block(p, ch=1, profile=prof.ptr, profile_ch=1, src=C.byref(sig), dst=C.byref(out_sig), n=16, streams=1):
        return lib.nae_denoise_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, profile, profile_ch, src, n, ch, streams, dst)

    def create(p, profile=prof.ptr, profile_ch=1, ch=2, out=True):
        h = C.c_void_p()
        rc = lib.nae_denoise_create(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, profile, profile_ch, ch, C.byref(h) if out else None)
        assert rc == 0 or not h.value
        if h.value:
            lib.nae_denoise_destroy(h)
        return rc

    assert block(good) == 0 and create(good) == 0 and create(good, profile_ch=2) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID and block(good, profile=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, profile_ch=2) == INVALID and block(good, profile_ch=0) == INVALID and create(good, profile_ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    for field, values in (("time_smooth", (-1, 9)), ("freq_smooth", (-1, 5)), ("thr_scale", (-0.5, np.nan, np.inf)),
                          ("floor_gain", (-0.1, 1.5, np.nan, np.inf))):
        for v in values:
            p = denoise_ref.params()
            setattr(p, field, v)
            assert block(p) == INVALID, (field, v)
            assert block(p, n=0) == INVALID, "checked before the empty call returns"
            assert create(p) == INVALID, (field, v)
    for n_fft in (0, 256, 1000, 8192):
        assert block(denoise_ref.params(n_fft)) == UNSUPPORTED and create(denoise_ref.params(n_fft)) == UNSUPPORTED, n_fft
        assert lib.nae_denoise_profile_f32(ctx.h, n_fft, C.byref(sig), 16, 1, prof.ptr) == UNSUPPORTED
    assert block(denoise_ref.params(thr_scale=0.0, floor_gain=0.0)) == 0 and block(denoise_ref.params(floor_gain=1.0, time_smooth=8, freq_smooth=4)) == 0
    assert create(None) == INVALID and create(good, profile=None) == INVALID and create(good, ch=3) == INVALID and create(good, out=False) == INVALID
    assert lib.nae_denoise_profile_f32(ctx.h, 512, None, 512, 1, prof.ptr) == INVALID
    assert lib.nae_denoise_profile_f32(ctx.h, 512, C.byref(sig), 512, 1, None) == INVALID
    assert lib.nae_denoise_profile_f32(ctx.h, 512, C.byref(sig), 512, 3, prof.ptr) == INVALID
    h = nae.Denoise(ctx, lib_params(nae, good), prof.ptr, 1, 1)
    h.put_host(np.zeros(5, np.float32))
    h.flush()
    assert h._fn("put_host")(h.h, np.zeros(1, np.float32).ctypes.data, 1) == STATE, "put after flush: NAE_ERR_STATE"
    assert h.available() == 5
    h.close()
    assert lib.nae_debug_set(ctx.h, b"dn_tile", 5) == 0 and lib.nae_debug_set(ctx.h, b"dn_tile", 0) == 0
    assert lib.nae_debug_set(ctx.h, b"dn_tile", -1) == INVALID and lib.nae_debug_set(ctx.h, b"dn_tiles", 1) == INVALID
    ctx.sync()
    d.free()
    prof.free()


def test_host_node_graph(host):
    """source -> audio_denoise -> sink with 1152-sample frames: the source's frames, sizes and pts; the block call's samples with the profile
    learned from the stretch, also where the stretch reaches past the end of the stream"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DENOISE OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_stream_too_short_for_the_profile(host):
    """a stream that ends with fewer than fft_size samples in the stretch is a Runtime_error"""
    r = subprocess.run([host, "short"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DENOISE OK short" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
