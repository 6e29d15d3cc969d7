"""K20 multiband compressor on the GPU, bit for bit against the CPU statement (tests/mb_ref/ref_mb.c): every length around the lane and the chunk
at two, three and four bands and three look-aheads, linked stereo and mono; every view; every mask pattern; every slab and group; the
composition of the library's own eq and dyn entries; the streaming handle; a launch of 300 chunks; a batch of more waves than the chip holds;
non-finite input; the error codes; the host node (tests/mb_ref/host_mb_node.cpp) and a seeded run of tests/tools/fuzz_mb.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dyn_ref
import mb_ref
import node_harness
from block_gpu import CONFIGS, bits, each_stream, mismatch, statement
from mb_gpu import debug_keys, gpu_mb, lib_params, mb_stream

pytestmark = pytest.mark.gpu

T, CH = dyn_ref.LANE, mb_ref.CHUNK
LENGTHS = (1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH, 3 * CH + 7)
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ref():
    return statement(mb_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("mb_ref/host_mb_node.cpp", str(tmp_path_factory.mktemp("host_mb_gpu")))


def wander(rng, n_streams, n, ch, shared=False, period=411, level_db=-18.0):
    """noise whose level wanders +-14 dB around level_db, another phase per stream and channel: every band's compressor works and rests"""
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * 10.0 ** ((level_db + 14.0 * np.sin(2 * np.pi * t / period + ph)) / 20.0)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def same(nae, ctx, ref, p, x, *views, **kw):
    return mismatch(gpu_mb(nae, ctx, p, x, *views, **kw), mb_ref.run_streams(ref, p, x))


@pytest.mark.parametrize("n_bands", (2, 3, 4))
@pytest.mark.parametrize("la", (0, 17, 1024))
def test_lengths_bands_and_lookaheads(nae, ctx, ref, n_bands, la):
    """the lane edge and the chunk edge in the length; linked stereo and mono"""
    rng = np.random.default_rng(100 * n_bands + la)
    for in_len in LENGTHS:
        for link, ch in ((1, 2), (0, 1)):
            p = mb_ref.case(n_bands, la, link)
            message = same(nae, ctx, ref, p, wander(rng, 2, in_len, ch, period=97 if in_len < 3 * CH else 1500))
            assert not message, (in_len, n_bands, la, link, message)


def test_the_compressors_work(ref):
    """the shared case is no wire: every band's compressor changes its band, and the bands differ"""
    x = wander(np.random.default_rng(1), 1, 3 * CH + 7, 2, period=1500)[0]
    for n_bands in (2, 3, 4):
        p = mb_ref.case(n_bands, 17, 1)
        xb = mb_ref.bands(ref, p, x)
        for b in range(n_bands):
            yb = dyn_ref.run(ref, p.band[b], xb[b])
            assert np.mean(bits(yb) != bits(xb[b])) > 0.9, (n_bands, b)


@pytest.mark.parametrize("n_bands", (2, 3, 4))
def test_views(nae, ctx, ref, n_bands):
    """mono, stereo linked and unlinked; interleaved and planar on either side, stream_stride 0, odd offsets, gaps; 3 streams of distinct
    content; the guard words around the destination stand (view_call checks them)"""
    rng = np.random.default_rng(10 + n_bands)
    in_len = CH + 3 * T + 5
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        for link in (0, 1):
            p = mb_ref.case(n_bands, (0, 17, 200)[i % 3], link, speed=(None, dyn_ref.FAST, dyn_ref.SLOW)[(i + link) % 3])
            x = wander(rng, n_streams, in_len, ch, shared)
            message = same(nae, ctx, ref, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
            assert not message, (ch, n_streams, sl, dl, shared, link, message)


def test_in_place(nae, ctx, ref):
    """dst->base == src->base in the same view is allowed, at every slab: the chunk a slab computes ahead is read again by the next"""
    x = wander(np.random.default_rng(5), 3, 4 * CH + 9, 2)
    for n_bands, link, la, slab in ((2, 1, 0, 0), (3, 0, 300, 1), (4, 1, 1024, 2)):
        p = mb_ref.case(n_bands, la, link)
        d = ctx.array(x.reshape(-1))
        sig = nae.Sig(d.ptr, x.shape[1] * 2, 1, 2)
        with debug_keys(ctx, mb_slab=slab):
            ctx.mb_block(lib_params(nae, p), sig, x.shape[1], 2, 3, sig)
        got = d.download().reshape(x.shape)
        d.free()
        message = mismatch(got, mb_ref.run_streams(ref, p, x))
        assert not message, (n_bands, link, la, message)


@pytest.mark.parametrize("bypass", range(8))
def test_every_mask_pattern_at_three_bands(nae, ctx, ref, bypass):
    """every mute mask under every bypass mask; all bands muted is silence, one band left is a solo: that band's own bits"""
    x = wander(np.random.default_rng(30 + bypass), 2, 2 * CH + 7, 2, period=900)
    base = mb_ref.case(3, 17, 1)
    xb = [mb_ref.bands(ref, base, s) for s in x]
    for mute in range(8):
        p = mb_ref.with_masks(base, mute, bypass)
        got = gpu_mb(nae, ctx, p, x)
        message = mismatch(got, mb_ref.run_streams(ref, p, x))
        assert not message, (mute, bypass, message)
        if mute == 7:
            assert not np.any(bits(got)), "every band muted: +0.0"
        left = [b for b in range(3) if not mute >> b & 1]
        if len(left) == 1:
            b = left[0]
            solo = np.stack([s[b] if bypass >> b & 1 else dyn_ref.run(ref, base.band[b], s[b]) for s in xb])
            assert np.array_equal(bits(got), bits(solo)), (mute, bypass)


def test_bypass_is_the_wire_compressor(nae, ctx):
    """a band in bypass_mask and a band with slope 0 and make-up 0 give the same bits"""
    x = wander(np.random.default_rng(8), 2, 2 * CH + 7, 2)
    base = mb_ref.case(3, 17, 1)
    wire = dyn_ref.params(slope=0.0, makeup_db=0.0, lookahead=17, link=1)
    for b in range(3):
        bands = mb_ref.bands_of(base)
        bands[b] = wire
        assert np.array_equal(bits(gpu_mb(nae, ctx, mb_ref.with_masks(base, bypass_mask=1 << b), x)), bits(gpu_mb(nae, ctx, mb_ref.with_masks(base, bands=bands), x)))


@pytest.mark.parametrize("n_bands,la,link", ((2, 0, 1), (3, 17, 0), (4, 1024, 1)))
def test_slabs_and_groups(nae, ctx, ref, n_bands, la, link):
    """mb_slab 1, 2, 0 crossed with mb_group 1, 2, 0 on 3 streams of 5 C + 7 samples: one wave's carries cross every slab edge on the device, the
    chunk a slab computes ahead is computed again by the next, every group runs on the workspace's first planes: the same bits"""
    x = wander(np.random.default_rng(40 + n_bands), 3, 5 * CH + 7, 2, period=1700)
    p = mb_ref.case(n_bands, la, link, mute_mask=2 if n_bands == 3 else 0, bypass_mask=1 if n_bands == 4 else 0)
    want = mb_ref.run_streams(ref, p, x)
    for slab in (1, 2, 0):
        for group in (1, 2, 0):
            with debug_keys(ctx, mb_slab=slab, mb_group=group):
                message = mismatch(gpu_mb(nae, ctx, p, x, "i", "p", chan_pad=3), want)
            assert not message, (slab, group, message)
    lib = ctx.lib
    for key in (b"mb_slab", b"mb_group"):
        assert lib.nae_debug_set(ctx.h, key, -1) == INVALID and lib.nae_debug_set(ctx.h, key + b"s", 1) == INVALID


@pytest.mark.parametrize("n_bands", (2, 3, 4))
def test_call_equals_the_composition_of_the_library_entries(nae, ctx, n_bands):
    """the GPU call against ctx.eq_block on every path's sections, ctx.dyn_block on every band and a float64 sum in numpy: no statement"""
    in_len, n_streams, ch = 3 * CH + 7, 2, 2
    x = wander(np.random.default_rng(50 + n_bands), n_streams, in_len, ch, period=1500)
    for la, link, mute, bypass in ((0, 1, 0, 0), (17, 0, 0, 1 << (n_bands - 1)), (1024, 1, 1, 2)):
        p = mb_ref.case(n_bands, la, link, mute, bypass)
        got = gpu_mb(nae, ctx, p, x)
        d_x, d_b = ctx.array(x.reshape(-1)), ctx.empty(x.size)
        src, dst = nae.Sig(d_x.ptr, in_len * ch, 1, ch), nae.Sig(d_b.ptr, in_len * ch, 1, ch)
        acc = None
        for b in range(n_bands):
            coef = mb_ref.path_coef(p, b)
            ctx.eq_block(coef, src, in_len, ch, n_streams, dst)
            if not bypass >> b & 1:
                ctx.dyn_block(nae.DynParams(*dyn_ref.as_tuple(p.band[b])), dst, in_len, ch, n_streams, dst)
            yb = d_b.download().reshape(x.shape).astype(np.float64)
            if not mute >> b & 1:
                acc = yb if acc is None else acc + yb
        d_x.free()
        d_b.free()
        assert np.array_equal(bits(got), bits(acc.astype(np.float32))), (n_bands, la, link, mute, bypass)


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("put", (1, 7, 1024, 1025, "random"))
def test_handle_equals_the_block_call(nae, ctx, ref, put, la):
    """any cut of the input into puts gives the block call's bits; `available` follows floor((put - la) / 1024) chunks after every put and
    the flush releases the rest; a put after the flush is NAE_ERR_STATE (mb_stream asserts all three).  Puts of one frame cross a chunk edge"""
    in_len = {1: CH + 300, 7: 1500}.get(put, 3 * CH + 7)
    ch, link = (1, 0) if put in (7, 1024) else (2, 1 if put != 1025 else 0)
    puts = tuple(int(k) for k in np.random.default_rng(la).integers(1, 1500, 16)) if put == "random" else (put,)
    n_bands = 2 + (la + in_len) % 3
    p = mb_ref.case(n_bands, la, link, bypass_mask=1 if put == 7 else 0)
    x = wander(np.random.default_rng(la + in_len), 1, in_len, ch, period=1300)
    block = gpu_mb(nae, ctx, p, x)[0]
    assert np.array_equal(bits(block), bits(mb_ref.run(ref, p, x[0])))
    for device in (False, True):
        got = mb_stream(nae, ctx, p, x[0], puts, device=device)
        assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block)), device


@pytest.mark.parametrize("slab", (0, 2))
def test_handle_pieces_larger_than_a_slab(nae, ctx, ref, slab):
    """puts of 70 chunks and 3 frames into a handle whose slab is 64 chunks (the default) or 2 (mb_slab at its creation): a launch runs more
    than one slab; nothing is received before the flush, so the output grows while all of it is live"""
    in_len = 150 * CH + 11
    x = wander(np.random.default_rng(60), 1, in_len, 2, period=30000)
    p = mb_ref.case(4, 300, 1)
    want = mb_ref.run(ref, p, x[0])
    with debug_keys(ctx, mb_slab=slab):
        got = mb_stream(nae, ctx, p, x[0], (70 * CH + 3,), device=(True, False), defer=slab == 0)
    assert got.shape == want.shape and not mismatch(got[None], want[None])


def test_long_launch(nae, ctx, ref):
    """two stereo streams of 300 C + 7 samples with the slowest attack and release: a wave walks 301 chunks, the sections' and the detectors'
    carries have a memory of hundreds of them"""
    p = mb_ref.case(4, 1024, 1, speed=dyn_ref.SLOW)
    x = wander(np.random.default_rng(300), 2, 300 * CH + 7, 2, period=40000)
    message = same(nae, ctx, ref, p, x, "p", "i", chan_pad=3)
    assert not message, message


def test_batch_of_more_waves_than_the_chip_holds(nae, ctx, ref):
    """1030 stereo streams of 1029 samples at four bands, unlinked: 2060 split waves and 8240 band waves.  Stream s carries signal s mod 17 of 17
    seeded signals; the statement runs on each and every stream is compared"""
    base = wander(np.random.default_rng(90), 17, 1029, 2, period=700)
    p = mb_ref.case(4, 96, 0)
    want17 = each_stream(lambda i: mb_ref.run(ref, p, base[i]), 17)
    pick = np.arange(1030) % 17
    message = mismatch(gpu_mb(nae, ctx, p, base[pick]), want17[pick])
    assert not message, message


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_does_not_reach_back(nae, ctx, bad, la):
    """a non-finite sample at 2 C + 5: every sample before it by more than the look-ahead has the clean run's bits, the other stream is
    untouched, the call returns NAE_OK and the sentinels around the destination stand"""
    i = 2 * CH + 5
    x = wander(np.random.default_rng(9), 2, 3 * CH + 40, 2)
    dirty_x = x.copy()
    dirty_x[0, i, 0] = bad
    for n_bands in (2, 4):
        p = mb_ref.case(n_bands, la, 1)
        clean = gpu_mb(nae, ctx, p, x, "p", "p", chan_pad=3)
        got = gpu_mb(nae, ctx, p, dirty_x, "p", "p", chan_pad=3)
        assert np.array_equal(bits(got[:, :i - la]), bits(clean[:, :i - la])), "samples before i - la changed"
        assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"
        assert not np.all(np.isfinite(got[0, i:, 0])), "the sample shows in its own channel"


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = mb_ref.case(3)
    h = C.c_void_p()

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1):
        return lib.nae_mb_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    def both(p, code, why):
        assert block(p) == code, why
        assert block(p, n=0) == code, ("checked before the empty call returns", why)
        assert lib.nae_mb_create(ctx.h, C.byref(lib_params(nae, p)), 2, C.byref(h)) == code and not h.value, why

    assert block(good) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    coef, bands = mb_ref.coef_of(good), mb_ref.bands_of(good)
    both(mb_ref.params(coef, bands, n_bands=1), INVALID, "B < 2")
    both(mb_ref.params(coef, bands, n_bands=0), INVALID, "B < 2")
    both(mb_ref.params(coef, bands, n_bands=5), UNSUPPORTED, "B > 4")
    both(mb_ref.params(coef, bands, n_sections=4), INVALID, "n_sections not the tree's")
    both(mb_ref.params(coef, bands, n_sections=14), INVALID, "n_sections not the tree's")
    both(mb_ref.params(mb_ref.coef_of(mb_ref.case(4)), bands), INVALID, "n_sections not the tree's")
    for s in (0, 8):
        for bad in ((1, 0, 0, 0, 1.0), (1, 0, 0, 1.5, 0.5), (float("nan"), 0, 0, 0, 0), (1, float("inf"), 0, 0, 0)):
            c = coef.copy()
            c[s] = bad
            both(mb_ref.params(c, bands), INVALID, ("section", s, bad))
    for b in range(3):
        for field, v in (("threshold_db", 0.5), ("slope", 1.5), ("knee_db", float("nan")), ("alpha_attack", 1.0), ("makeup_db", 25.0), ("lookahead", -1), ("link", 2)):
            bb = mb_ref.bands_of(good)
            bb[b] = dyn_ref.Params(*dyn_ref.as_tuple(bb[b]))
            setattr(bb[b], field, v)
            both(mb_ref.params(coef, bb), INVALID, ("band", b, field, v))
        if b:
            bb = mb_ref.bands_of(good)
            bb[b] = dyn_ref.Params(*dyn_ref.as_tuple(bb[b]))
            bb[b].lookahead = 5
            both(mb_ref.params(coef, bb), INVALID, "unequal lookahead")
            bb[b].lookahead, bb[b].link = 0, 0
            both(mb_ref.params(coef, bb), INVALID, "unequal link")
    both(mb_ref.params(coef, bands, mute_mask=8), INVALID, "mask bit at B")
    both(mb_ref.params(coef, bands, bypass_mask=1 << 31), INVALID, "mask bit above B")
    both(mb_ref.case(3, 1025), UNSUPPORTED, "look-ahead above 1024")
    assert block(mb_ref.case(3, 1024, mute_mask=7, bypass_mask=7)) == 0
    assert lib.nae_mb_create(ctx.h, None, 2, C.byref(h)) == INVALID
    assert lib.nae_mb_create(ctx.h, C.byref(lib_params(nae, good)), 3, C.byref(h)) == INVALID
    assert lib.nae_mb_create(ctx.h, C.byref(lib_params(nae, good)), 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host):
    """source -> audio_multiband -> sink with 1152-sample frames: the source's frames, sizes and pts; the handle's bits with the designed
    parameters"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MB OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_bad_rate(host):
    """a crossover at or above Nyquist, or a look-ahead of more than 1024 samples at the stream's rate, is a Runtime_error on the first frame"""
    r = subprocess.run([host, "rate"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST MB OK rate" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_fuzz_mb_seeded(nae, ctx):
    """a seeded 20-case run of tests/tools/fuzz_mb.py: bands, crossovers, band records, masks, lengths, views, slabs, groups and put patterns"""
    sys.path.insert(0, os.path.join(mb_ref.ROOT, "tests", "tools"))
    import fuzz_mb
    assert fuzz_mb.main(cases=fuzz_mb.SEEDED[0], seed=fuzz_mb.SEEDED[1], ctx=ctx, nae=nae) == fuzz_mb.SEEDED[0]
