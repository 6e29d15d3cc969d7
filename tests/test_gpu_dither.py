"""K23 dither on the GPU, bit for bit against the CPU statement (tests/dither_ref/ref_dither.c): the lengths around the tile and the block, mono
and stereo, stream counts around one wave, every kind, tap count and word length, every view, a shared source, the streaming handle in
every put pattern, two contexts, both values of the debug key dither_roles, a batch of more stream-channels than a quarter of the chip
walks at once, non-finite input, the error codes, the host node (tests/dither_ref/host_dither_node.cpp) and a seeded run of
tests/tools/fuzz_dither.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import dither_ref
import node_harness
from block_gpu import CONFIGS, bits, mismatch, statement
from dither_gpu import dither_stream, gpu_dither, lib_params, same

pytestmark = pytest.mark.gpu

INVALID = -1
# 16: the error-feedback kernel's tile; 1024: the flat kernel's block (and 512 stereo frames of it)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4099)
TAPS = {0: (), 1: dither_ref.PRESETS["first"], 2: dither_ref.PRESETS["second"], 5: dither_ref.PRESETS["lipshitz"], 12: dither_ref.drawn_taps()}
FLAT = tuple(itertools.product(dither_ref.KINDS, (0,), (8, 16, 24)))                 # 12: kind x bits without taps
SHAPED = tuple(itertools.product(dither_ref.KINDS, (1, 2, 5, 12), (8, 16, 24)))      # 48: kind x K x bits
MODES = FLAT + SHAPED


@pytest.fixture(scope="module")
def ref():
    return statement(dither_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dither_ref/host_dither_node.cpp", str(tmp_path_factory.mktemp("host_dither_gpu")))


def mode(modes, i, seed=1):
    kind, k, b = modes[i % len(modes)]
    return dither_ref.params(b, kind, TAPS[k], seed)


@pytest.mark.parametrize("n_streams", (1, 31, 32, 33, 65))
def test_shapes(nae, ctx, ref, n_streams):
    """every length, mono and stereo, at one lane, one stereo wave less one stream, exactly one, one more, and two waves and a bit: at every
    shape one mode without taps and one with, the modes (kind x K x bits) taken in turn across the 170 shapes of the five cases"""
    rng = np.random.default_rng(n_streams)
    i = (1, 31, 32, 33, 65).index(n_streams) * 2 * len(LENGTHS)
    for in_len in LENGTHS:
        for ch in (1, 2):
            x = rng.uniform(-1.05, 1.05, (n_streams, in_len, ch)).astype(np.float32)
            for p in (mode(FLAT, i, seed=i), mode(SHAPED, i, seed=i)):
                message = same(nae, ctx, ref, p, x)
                assert not message, (in_len, ch, dither_ref.as_tuple(p), message)
            i += 1


def test_every_mode(nae, ctx, ref):
    """every kind at every tap count and word length, 3 stereo streams of 1025 samples that clip both ways"""
    x = np.random.default_rng(2).uniform(-1.2, 1.2, (3, 1025, 2)).astype(np.float32)
    for i in range(len(MODES)):
        message = same(nae, ctx, ref, mode(MODES, i, seed=i), x)
        assert not message, (MODES[i], message)


@pytest.mark.parametrize("k", (0, 5))
def test_views(nae, ctx, ref, k):
    """interleaved and planar on either side, stream_stride 0, odd offsets, gaps; the guard words around the destination stand and nothing
    outside a source signal is read (view_call fills it with NaN, which would count as zero and show).  With the shared source every
    stream's output equals the statement under its own key, and the streams differ from one another"""
    rng = np.random.default_rng(10 + k)
    for in_len in (1029, 64):
        for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
            for kind in ("triangular", "highpass"):
                p = dither_ref.params((16, 24, 8)[i % 3], kind, TAPS[k], seed=i)
                x = rng.uniform(-1, 1, (n_streams, in_len, ch)).astype(np.float32)
                if shared:
                    x[:] = x[0]
                for offset in (0, 1):                                   # 16-byte aligned bases, and bases that are 4-byte aligned only
                    got = gpu_dither(nae, ctx, p, x, sl, dl, shared, gap=(3 if offset else 4) if sl == "p" else 0,
                                     chan_pad=(5 if offset else 4 + (-in_len) % 4) if "p" in (sl, dl) else 0, offset=offset)
                    message = mismatch(got, dither_ref.run_streams(ref, p, x, shared))
                    assert not message, (ch, n_streams, sl, dl, shared, offset, message)
                    if shared and in_len > 64:
                        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2]), "every stream has its own dither"


@pytest.mark.parametrize("k", (0, 5))
def test_strided_views(nae, ctx, ref, k):
    """frames 3 floats apart with 2 channels on both sides (a third channel rides along and stays), and channels 2 frames apart: views that
    are neither interleaved nor planar"""
    n_streams, n = 3, 777
    x = np.random.default_rng(70 + k).uniform(-1, 1, (n_streams, n, 2)).astype(np.float32)
    p = dither_ref.params(16, "triangular", TAPS[k], seed=4)
    want = dither_ref.run_streams(ref, p, x)
    for fs, cs in ((3, 1), (5, 2)):
        host = np.full((n_streams, n, fs), -7.0, np.float32)
        host[:, :, 0], host[:, :, cs] = x[:, :, 0], x[:, :, 1]
        d_x, d_y = ctx.array(host.reshape(-1)), ctx.array(np.full(n_streams * n * fs, -9.0, np.float32))
        ctx.dither_block(lib_params(nae, p), nae.Sig(d_x.ptr, n * fs, cs, fs), n, 2, n_streams, nae.Sig(d_y.ptr, n * fs, cs, fs))
        out = d_y.download().reshape(n_streams, n, fs)
        d_x.free()
        d_y.free()
        message = mismatch(np.ascontiguousarray(out[:, :, (0, cs)]), want)
        assert not message, (fs, cs, message)
        rest = [c for c in range(fs) if c not in (0, cs)]
        assert np.all(out[:, :, rest] == -9.0), "nothing stored between the channels"


def test_in_place(nae, ctx, ref):
    """dst->base == src->base is allowed, interleaved and planar"""
    x = np.random.default_rng(5).uniform(-1, 1, (3, 2057, 2)).astype(np.float32)
    for k, kind in ((0, "triangular"), (5, "highpass"), (12, "rectangular")):
        p = dither_ref.params(16, kind, TAPS[k])
        want = dither_ref.run_streams(ref, p, x)
        d = ctx.array(x.reshape(-1))
        sig = nae.Sig(d.ptr, x.shape[1] * 2, 1, 2)
        ctx.dither_block(lib_params(nae, p), sig, x.shape[1], 2, 3, sig)
        got = d.download().reshape(x.shape)
        d.free()
        message = mismatch(got, want)
        assert not message, (k, "interleaved", message)
        d = ctx.array(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1))
        sig = nae.Sig(d.ptr, x.shape[1] * 2, x.shape[1], 1)
        ctx.dither_block(lib_params(nae, p), sig, x.shape[1], 2, 3, sig)
        got = np.ascontiguousarray(d.download().reshape(3, 2, -1).transpose(0, 2, 1))
        d.free()
        message = mismatch(got, want)
        assert not message, (k, "planar", message)


@pytest.mark.parametrize("k", (0, 5))
@pytest.mark.parametrize("put", (1, 7, 1000, 1024, 5000, "ragged"))
def test_handle_equals_the_block_call(nae, ctx, ref, put, k):
    """any cut of the input into puts gives the block call's bits; every frame put is available after that put; a put after the flush is
    NAE_ERR_STATE (dither_stream asserts both)"""
    in_len = {1: 150, 7: 1000}.get(put, 12007)
    puts = (1, 7, 1000, 1024, 5000, 1, 16, 15, 17) if put == "ragged" else (put,)
    for ch in (1, 2):
        x = np.random.default_rng(in_len + ch).uniform(-1, 1, (1, in_len, ch)).astype(np.float32)
        for kind in ("triangular", "highpass"):
            p = dither_ref.params(16, kind, TAPS[k], seed=6)
            want = dither_ref.run(ref, p, x[0])
            assert np.array_equal(bits(gpu_dither(nae, ctx, p, x)[0]), bits(want))
            for device in (False, True):
                got = dither_stream(nae, ctx, p, x[0], puts, device=device)
                assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(want)), (device, kind, ch)


def test_two_handles_on_one_context_and_on_two(nae, ctx, ref):
    """two handles fed in turn, on one context and on two: each gives its own statement's bits; a block call afterwards is unaffected"""
    x = np.random.default_rng(21).uniform(-1, 1, (2, 5100, 2)).astype(np.float32)
    ps = [dither_ref.params(16, "highpass", "lipshitz", seed=1), dither_ref.params(24, "triangular", TAPS[12], seed=2)]
    want = [dither_ref.run(ref, ps[k], x[k]) for k in range(2)]
    other = nae.Context(0)
    try:
        for ctxs in ((ctx, ctx), (ctx, other)):
            hs = [nae.Dither(ctxs[k], lib_params(nae, ps[k]), 2) for k in range(2)]
            parts = [[], []]
            try:
                for pos in range(0, x.shape[1], 777):
                    for k in range(2):
                        hs[k].put_host(x[k, pos:pos + 777].reshape(-1))
                        parts[k].append(hs[k].receive_host())
                for k in range(2):
                    hs[k].flush()
                    assert hs[k].available() == 0
            finally:
                for h in hs:
                    h.close()
            for k in range(2):
                got = np.concatenate(parts[k]).reshape(-1, 2)
                assert got.shape == want[k].shape and np.array_equal(bits(got), bits(want[k])), (k, ctxs[1] is other)
            message = same(nae, ctx, ref, ps[0], x)
            assert not message, "a block call after the handles starts at sample 0 with no error behind it: " + message
    finally:
        other.close()


def test_roles_give_the_same_bits(nae, ctx, ref):
    """debug key dither_roles: 0 (the library's choice), 1 (the producer waves) and 2 (the walking wave does everything) give the statement's
    bits, in the block call and in the handle; other values and other keys are refused"""
    x = np.random.default_rng(33).uniform(-1.1, 1.1, (33, 1041, 2)).astype(np.float32)
    try:
        for roles in (0, 1, 2):
            ctx.debug_set("dither_roles", roles)
            for k, kind in ((1, "rectangular"), (5, "highpass"), (12, "triangular"), (0, "triangular")):
                p = dither_ref.params(16, kind, TAPS[k], seed=8)
                message = same(nae, ctx, ref, p, x, "p", "i", chan_pad=3)
                assert not message, (roles, k, message)
                got = dither_stream(nae, ctx, p, x[0], (1000, 7, 16, 17), device=(True, False))
                assert np.array_equal(bits(got), bits(dither_ref.run(ref, p, x[0]))), (roles, k)
    finally:
        ctx.debug_set("dither_roles", 0)
    lib = ctx.lib
    assert lib.nae_debug_set(ctx.h, b"dither_roles", 3) == INVALID and lib.nae_debug_set(ctx.h, b"dither_roles", -1) == INVALID
    assert lib.nae_debug_set(ctx.h, b"dither_role", 1) == INVALID


def test_large_batch(nae, ctx, ref):
    """8201 stereo streams of 100 samples are 16402 stream-channels: more than the 16384 that a quarter of the chip walks with one wave per
    SIMD, 257 workgroups, the last one with 18 of its 64 lanes filled.  Stream s carries signal s mod 17; every stream has its own key, so
    the statement runs on each and every stream is compared.  Without taps the same batch is 8201 rows of the flat kernel"""
    base = np.random.default_rng(90).uniform(-1, 1, (17, 100, 2)).astype(np.float32)
    x = base[np.arange(8201) % 17]
    for k, kind in ((5, "triangular"), (0, "highpass")):
        p = dither_ref.params(16, kind, TAPS[k], seed=3)
        message = same(nae, ctx, ref, p, x)
        assert not message, (k, message)


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_counts_as_zero(nae, ctx, ref, bad):
    """the statement's rule on the GPU: the output is on the grid everywhere, and equals the statement's (which equals the run with a zero in
    the sample's place: tests/test_dither_cpu.py)"""
    x = np.random.default_rng(9).uniform(-1, 1, (2, 1100, 2)).astype(np.float32)
    x[0, 517, 0] = bad
    x[1, 0, 1] = bad
    for k in (0, 5):
        for kind in ("triangular", "highpass"):
            p = dither_ref.params(16, kind, TAPS[k])
            got = gpu_dither(nae, ctx, p, x, "p", "p", chan_pad=3)
            assert np.all(np.isfinite(got)) and not mismatch(got, dither_ref.run_streams(ref, p, x)), (k, kind)


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = dither_ref.params(16, "none", "lipshitz")

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1):
        return lib.nae_dither_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    assert block(good) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    h = C.c_void_p()
    for changes in dither_ref.BAD_PARAMS:
        p = dither_ref.bad_params(changes)
        assert block(p) == INVALID, changes
        assert block(p, n=0) == INVALID, "checked before the empty call returns"
        assert lib.nae_dither_create(ctx.h, C.byref(lib_params(nae, p)), 2, C.byref(h)) == INVALID and not h.value, changes
    for changes in dither_ref.BOUNDARY_PARAMS:
        assert block(dither_ref.params(**changes)) == 0, changes
    assert lib.nae_dither_create(ctx.h, None, 2, C.byref(h)) == INVALID
    assert lib.nae_dither_create(ctx.h, C.byref(lib_params(nae, good)), 3, C.byref(h)) == INVALID
    assert lib.nae_dither_create(ctx.h, C.byref(lib_params(nae, good)), 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host, ref, tmp_path):
    """source -> audio_dither -> sink with frames of 1000 samples and a short last one: the source's frames, sizes and pts, the block call's
    samples (the harness checks those), and the statement's samples with the node's seeds, channel c under the key of channel c"""
    r = subprocess.run([host, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DITHER OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    cases = {"defaults2": (2, dither_ref.params()), "defaults1": (1, dither_ref.params()), "shaped2": (2, dither_ref.params(12, "highpass", "lipshitz", 99)),
             "taps2": (2, dither_ref.params(24, "rectangular", (1.25, -0.5, 0.125), 1))}
    for name, (ch, p) in cases.items():
        x = np.fromfile(os.path.join(str(tmp_path), name + "_x.f32"), np.float32).reshape(-1, ch)
        y = np.fromfile(os.path.join(str(tmp_path), name + "_y.f32"), np.float32).reshape(-1, ch)
        assert len(x) == 20011 and np.array_equal(bits(y), bits(dither_ref.run(ref, p, x))), name


def test_fuzz_dither_seeded(nae, ctx):
    """a seeded run of tests/tools/fuzz_dither.py: word lengths, kinds, taps at their limits, seeds, lengths, views, levels, samples that are
    not finite, roles and put patterns"""
    sys.path.insert(0, os.path.join(dither_ref.ROOT, "tests", "tools"))
    import fuzz_dither
    assert fuzz_dither.main(cases=fuzz_dither.SEEDED[0], seed=fuzz_dither.SEEDED[1], ctx=ctx, nae=nae) == fuzz_dither.SEEDED[0]
