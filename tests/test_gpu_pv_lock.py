"""K7 with identity phase locking (NAE_STRETCH_PHASE_LOCK) on the GPU, against the CPU statement tests/pv_ref/ref_pv.c.

Bars: the integer synthesis phases are bit-exact; the samples are within 1e-4 relative RMS (the tolerance path of the unlocked node);
every tiling, the streaming handle and every batch position give the same bits; flags == 0 through the _ex entries is the unlocked call."""
import ctypes as C

import numpy as np
import pytest

import node_harness
import orc
import pv_ref
from conftest import rel_rms
from pv_gpu import block, signal, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
LOCK = 1          # NAE_STRETCH_PHASE_LOCK
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5), (0.5, 2.0)]   # those of test_k7_integer_phases_bit_exact


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("rate,pitch", PAIRS)
@pytest.mark.parametrize("tile", [64, 16])
def test_locked_integer_phases_bit_exact(nae, ref, rate, pitch, kind, tile):
    """Qs in front of every tile equals the restatement's locked phase of the frame before it, bit for bit"""
    L, ch = 40000, 2
    x = signal(kind, L, ch)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", tile)
        d_x = c.array(x)
        got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, 1, phase_lock=True)
        d_x.free()
    assert t == tile
    qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, lock=True)
    assert not np.array_equal(qs, pv_ref.synth_phase(ref, x, ch, rate, pitch, lock=False)), "locking changes the phases"
    n_tiles = got.shape[2]
    assert n_tiles >= 2
    for j in range(n_tiles):
        for c2 in range(ch):
            want = qs[j * tile - 1, c2] if j > 0 else np.zeros(513, np.int32)
            assert np.array_equal(got[0, c2, j], want), (j, c2, int(np.count_nonzero(got[0, c2, j] != want)))


@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("rate,pitch", PAIRS + [(0.6, 1 / 0.6), (1.0, 2 ** (-7 / 12))])
def test_locked_samples_vs_restatement(ctx, nae, ref, rate, pitch, kind):
    L, ch = 30000, 2
    x = signal(kind, L, ch, 43)
    got = block(ctx, nae, x, ch, rate, pitch, lock=True)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, lock=True)
    assert got.size == want.size and np.isfinite(got).all()
    e = rel_rms(got, want)
    print(f"locked rel RMS {rate:.4f}/{pitch:.4f} {kind}: {e:.3g}")
    assert e <= TOL, e
    assert rel_rms(got, pv_ref.stretch(ref, x, ch, rate, pitch, lock=False)) > 10 * TOL, "the locked output is not the unlocked one"


def test_locked_every_tiling_gives_the_same_bits(nae):
    """one tile, 16- and 64-frame tiles and the library's choice, on a long lone stream whose 16-frame tiling has >= 256 pass-1 tiles per
    stream-channel (the chunked map scan), equal bit for bit"""
    ch, L, rate, pitch = 2, 1_500_000, 1.0, 2 ** (3 / 12)
    x = (0.5 * orc.fill_uniform(L * ch, 99)).astype(np.float32)
    outs, launched = {}, {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("16-frame tiles", {"pv_tile": 16}), ("64-frame tiles", {"pv_tile": 64}),
                       ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            c.prof_reset(); c.prof_enable(True)
            outs[key] = block(c, nae, x, ch, rate, pitch, lock=True)
            c.prof_enable(False)
            launched[key] = set(c.prof_report())
    pl = nae.Context.stretch_plan(rate, pitch, L)
    assert (pl.frames + 15) // 16 >= 256
    assert "pvlock_scan_kernel" in launched["16-frame tiles"] and "pvlock_scan_kernel" not in launched["one tile"]
    assert not any("pv_pipe" in k or k == "pv_phase_kernel" for k in launched["library"]), launched["library"]
    for key in outs:
        assert np.array_equal(outs[key].view(np.uint32), outs["one tile"].view(np.uint32)), key


@pytest.mark.parametrize("rate,pitch", [(1.0, float(np.float32(2 ** (3 / 12)))), (1.0, float(np.float32(2 ** (-7 / 12)))),
                                        (1.5, float(np.float32(1 / 1.5)))])
def test_locked_stream_handle_equals_block(ctx, nae, rate, pitch):
    """uneven small pieces (one tile per segment, pass L3 carries the phase) equal the locked block call bit for bit"""
    L, ch = 150000, 2
    x = (0.5 * orc.fill_uniform(L * ch, 7)).astype(np.float32)
    blk = block(ctx, nae, x, ch, rate, pitch, lock=True)
    y = stream(ctx, x, ch, rate, pitch, [1152, 4001, 777, 20000], "ex", flags=LOCK)
    assert y.size == blk.size
    assert np.array_equal(y.view(np.uint32), blk.view(np.uint32))


def test_locked_stream_pieces_of_256_tiles(nae):
    """pieces of >= 256 pass-1 tiles (16-frame tiles): the chunked map scan with a phase carried in and out of every segment"""
    ch, L, rate, pitch = 2, 2_600_000, 1.0, float(np.float32(2 ** (3 / 12)))
    x = (0.5 * orc.fill_uniform(L * ch, 123)).astype(np.float32)
    with nae.Context(0) as c:
        blk = block(c, nae, x, ch, rate, pitch, lock=True)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", 16)
        c.prof_reset(); c.prof_enable(True)
        y = stream(c, x, ch, rate, pitch, [1_100_000, 1_100_000, 400_000], "ex", flags=LOCK, device_put=True)
        c.prof_enable(False)
        assert "pvlock_scan_kernel" in set(c.prof_report())
    assert y.size == blk.size
    assert np.array_equal(y.view(np.uint32), blk.view(np.uint32))


def test_locked_batch_of_1024_equals_lone_runs(ctx, nae):
    n, L, ch, pitch = 1024, 12000, 2, 2 ** (3 / 12)
    x = orc.fill_uniform(n * L * ch, 47)
    got = block(ctx, nae, x, ch, 1.0, pitch, lock=True, n_streams=n).reshape(n, -1)
    for s in (0, 1, 2, 3, 511, 1022, 1023):
        one = block(ctx, nae, x.reshape(n, -1)[s].copy(), ch, 1.0, pitch, lock=True)
        assert np.array_equal(one.view(np.uint32), got[s].view(np.uint32)), s


def test_locked_non_finite_sample_is_confined(ctx, nae, ref):
    """a NaN sample: non-finite output only where the restatement's is, the other channel and the rest within tolerance"""
    L, ch, pitch = 60000, 2, 2 ** (3 / 12)
    x = (0.5 * orc.fill_uniform(L * ch, 43)).reshape(L, ch).copy()
    x[30001, 0] = np.nan
    got = block(ctx, nae, x.reshape(-1), ch, 1.0, pitch, lock=True).reshape(-1, ch)
    want = pv_ref.stretch(ref, x.reshape(-1), ch, 1.0, pitch, lock=True).reshape(-1, ch)
    bad_ref, bad_got = ~np.isfinite(want), ~np.isfinite(got)
    assert not bad_ref[:, 1].any() and not bad_got[:, 1].any()
    assert 1000 < bad_ref[:, 0].sum() < 4000
    lo, hi = np.flatnonzero(bad_ref[:, 0])[[0, -1]]
    glo, ghi = np.flatnonzero(bad_got[:, 0])[[0, -1]]
    assert abs(int(lo) - int(glo)) <= 16 and abs(int(hi) - int(ghi)) <= 16, (lo, hi, glo, ghi)
    ok = np.ones(want.shape[0], bool)
    ok[min(lo, glo) - 16: max(hi, ghi) + 17] = False
    assert rel_rms(got[ok], want[ok]) <= TOL


def test_unknown_flag_bits_are_invalid(ctx, nae):
    lib = ctx.lib
    L, ch = 4096, 2
    d_x, d_o = ctx.empty(L * ch), ctx.empty(2 * L * ch)
    src, dst = nae.Sig.interleaved(d_x.ptr, L, ch), nae.Sig.interleaved(d_o.ptr, 2 * L, ch)
    h = C.c_void_p()
    nt, tf = C.c_size_t(), C.c_size_t()
    buf = np.zeros(64 * 513 * ch, np.int32)
    for flags in (2, 4, 0x80000000, LOCK | 2):
        assert lib.nae_stretch_block_ex_f32(ctx.h, 1.0, 1.2, flags, C.byref(src), L, ch, 1, C.byref(dst)) == -1
        assert lib.nae_stretch_create_ex(ctx.h, 48000, ch, 1.0, 1.2, flags, C.byref(h)) == -1
        assert lib.nae_debug_pv_tile_phase_ex(ctx.h, 1.0, 1.2, flags, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size,
                                              C.byref(nt), C.byref(tf)) == -1
    d_x.free(); d_o.free()


def test_flags_zero_is_the_existing_call(ctx, nae):
    lib = ctx.lib
    L, ch, rate, pitch = 40000, 2, 1.0, 2 ** (3 / 12)
    x = orc.fill_uniform(L * ch, 5)
    pl = ctx.stretch_plan(rate, pitch, L)
    d_x, d_a, d_b = ctx.array(x), ctx.empty(pl.out_len * ch), ctx.empty(pl.out_len * ch)
    src = nae.Sig.interleaved(d_x.ptr, L, ch)
    ctx.stretch_block(rate, pitch, src, L, ch, 1, nae.Sig.interleaved(d_a.ptr, pl.out_len, ch))
    assert lib.nae_stretch_block_ex_f32(ctx.h, rate, pitch, 0, C.byref(src), L, ch, 1,
                                        C.byref(nae.Sig.interleaved(d_b.ptr, pl.out_len, ch))) == 0
    assert np.array_equal(d_a.download().view(np.uint32), d_b.download().view(np.uint32))
    a, ta = ctx.debug_pv_tile_phase(rate, pitch, src, L, ch, 1)
    cap = ch * (pl.frames + 1) * 513
    b = np.zeros(cap, np.int32)
    nt, tf = C.c_size_t(), C.c_size_t()
    assert lib.nae_debug_pv_tile_phase_ex(ctx.h, rate, pitch, 0, C.byref(src), L, ch, 1, b.ctypes.data, cap, C.byref(nt), C.byref(tf)) == 0
    assert tf.value == ta and np.array_equal(a.reshape(-1), b[: a.size])
    d_x.free(); d_a.free(); d_b.free()
    p32 = float(np.float32(pitch))
    y0 = stream(ctx, x, ch, rate, p32, [1152, 3000], "ex", flags=0)
    h = C.c_void_p()
    assert lib.nae_stretch_create(ctx.h, 48000, ch, rate, p32, C.byref(h)) == 0
    assert lib.nae_stretch_put_host(h, x.ctypes.data, L) == 0 and lib.nae_stretch_flush(h) == 0
    n = lib.nae_stretch_available(h)
    y1 = np.empty(n * ch, np.float32)
    got = C.c_size_t()
    assert lib.nae_stretch_receive_host(h, y1.ctypes.data, n, C.byref(got)) == 0 and lib.nae_stretch_destroy(h) == 0
    assert np.array_equal(y0.view(np.uint32), y1.view(np.uint32))


def test_python_stretcher_phase_lock(ctx, nae):
    L, ch, pitch = 50000, 2, float(np.float32(2 ** (3 / 12)))
    x = (0.5 * orc.fill_uniform(L * ch, 11)).astype(np.float32)
    s = nae.Stretcher(ctx, 48000, ch, 1.0, pitch, phase_lock=True)
    s.put_host(x)
    s.flush()
    y = s.receive_host()
    s.close()
    assert np.array_equal(y.view(np.uint32), block(ctx, nae, x, ch, 1.0, pitch, lock=True).view(np.uint32))


def test_host_graph_pitch_node_phase_lock(tmp_path):
    """source -> Pitch_modifier {"pitch": 3, "phase_lock": true} -> sink equals the locked block call bit for bit (host mirror)"""
    import subprocess
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "gpu", "phase_lock"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST PV NODE OK gpu phase_lock" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
