"""K7 at vocoder frame sizes 512 ... 4096 on the GPU (kernels_pv_any.hip), against the CPU statement tests/pv_ref/ref_pv.c.

Bars: the integer synthesis phases are bit-exact; the samples are within 1e-4 relative RMS; every tiling, batch position, layout and the
streaming handle give the same bits; at 1024 the size-generic kernels (debug key pv_any) give the shipped kernels' integer phases, and _n at
1024 is the _ex call."""
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
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-5 / 12)), (1.5, 1 / 1.5), (0.5, 2.0)]   # those of tests/test_gpu_pv_lock.py
SIZES = [512, 2048, 4096]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def tile_phases(c, nae, x, ch, rate, pitch, n_fft):
    L = x.size // ch
    d_x = c.array(x)
    got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, 1, n_fft=n_fft)
    d_x.free()
    return got, t


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("rate,pitch", PAIRS)
@pytest.mark.parametrize("n_fft", SIZES)
def test_integer_phases_bit_exact(nae, ref, n_fft, rate, pitch, kind, ch):
    """Qs in front of every 16-frame tile equals the restatement's phase of the frame before it, bit for bit (both stage orders: +3
    semitones runs the transposer first, -5 semitones after; 1.5 / (1/1.5) runs no transposer)"""
    L, tile = 40000, 16
    x = signal(kind, L, ch)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", tile)
        got, t = tile_phases(c, nae, x, ch, rate, pitch, n_fft)
    assert t == tile
    qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft)
    n_tiles = got.shape[2]
    assert n_tiles >= 2 and got.shape[3] == n_fft // 2 + 1
    for j in range(n_tiles):
        for c2 in range(ch):
            want = qs[j * tile - 1, c2] if j > 0 else np.zeros(n_fft // 2 + 1, np.int32)
            assert np.array_equal(got[0, c2, j], want), (j, c2, int(np.count_nonzero(got[0, c2, j] != want)))


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("rate,pitch", PAIRS + [(0.6, 1 / 0.6), (2.0, 1.0)])
@pytest.mark.parametrize("n_fft", SIZES)
def test_samples_vs_restatement(ctx, nae, ref, n_fft, rate, pitch, kind, ch):
    """within 1e-4 relative RMS; (2.0, 1.0) is the transposer alone (the frame size has no effect there: bit-equal to 1024)"""
    L = 30000
    x = signal(kind, L, ch, 43)
    got = block(ctx, nae, x, ch, rate, pitch, n_fft)
    want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft)
    assert got.size == want.size and np.isfinite(got).all()
    e = rel_rms(got, want)
    print(f"N={n_fft} rel RMS {rate:.4f}/{pitch:.4f} {kind} ch{ch}: {e:.3g}")
    assert e <= TOL, e
    if rate == 2.0:
        assert np.array_equal(got.view(np.uint32), block(ctx, nae, x, ch, rate, pitch, 1024).view(np.uint32))


@pytest.mark.parametrize("n_fft", SIZES)
def test_every_tiling_gives_the_same_bits(nae, n_fft):
    """one tile, 1-, 16- and 64-frame tiles, pv_min_ptile and the library's choice; the 16-frame tiling of this long lone stream has >= 256
    tiles per stream-channel (the chunked scan); with 1-frame tiles, tile 1 starts at frame 1, whose priming frame is frame 0"""
    ch, rate, pitch = 2, 1.0, 2 ** (3 / 12)
    L = 16 * 260 * (n_fft // 4) + 4096
    x = (0.5 * orc.fill_uniform(L * ch, 99)).astype(np.float32)
    outs = {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("1-frame tiles", {"pv_tile": 1}), ("16-frame tiles", {"pv_tile": 16}),
                       ("64-frame tiles", {"pv_tile": 64}),
                       ("min 100", {"pv_min_ptile": 100}), ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            c.prof_reset(); c.prof_enable(True)
            outs[key] = block(c, nae, x, ch, rate, pitch, n_fft)
            c.prof_enable(False)
            launched = set(c.prof_report())
            if key == "16-frame tiles":
                assert "pv_any_scan_kernel" in launched
            assert not any(k.startswith("pv_pipe") or k.startswith("pv_flow") or k == "pv_phase_kernel" for k in launched), launched
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    assert (pl.frames + 15) // 16 >= 256
    for key in outs:
        assert np.array_equal(outs[key].view(np.uint32), outs["one tile"].view(np.uint32)), key


@pytest.mark.parametrize("n_fft", SIZES)
def test_batch_positions_and_layouts(ctx, nae, n_fft):
    """stream s of a batch equals its lone run bit for bit; interleaved, planar and shared-source (stream_stride 0) layouts agree"""
    n, L, ch, rate, pitch = 64, 12000, 2, 1.0, 2 ** (3 / 12)
    x = orc.fill_uniform(n * L * ch, 47)
    got = block(ctx, nae, x, ch, rate, pitch, n_fft, n_streams=n).reshape(n, -1)
    for s in (0, 1, 31, 62, 63):
        one = block(ctx, nae, x.reshape(n, -1)[s].copy(), ch, rate, pitch, n_fft)
        assert np.array_equal(one.view(np.uint32), got[s].view(np.uint32)), s
    pl = ctx.stretch_plan(rate, pitch, L, n_fft)
    one = x.reshape(n, -1)[3].copy()
    planar = np.ascontiguousarray(one.reshape(L, ch).T).reshape(-1)
    d_p, d_i, d_o = ctx.array(planar), ctx.array(one), ctx.empty(4 * pl.out_len * ch)
    ctx.stretch_block(rate, pitch, nae.Sig.planar(d_p.ptr, L, ch), L, ch, 1, nae.Sig.planar(d_o.ptr, pl.out_len, ch), n_fft=n_fft)
    yp = d_o.download()[: pl.out_len * ch].reshape(ch, -1).T.reshape(-1)
    ctx.stretch_block(rate, pitch, nae.Sig.interleaved(d_i.ptr, L, ch, shared=True), L, ch, 4,
                      nae.Sig.interleaved(d_o.ptr, pl.out_len, ch), n_fft=n_fft)
    ys = d_o.download()[: 4 * pl.out_len * ch].reshape(4, -1)
    want = got[3]
    assert np.array_equal(yp.view(np.uint32), want.view(np.uint32)), "planar"
    for s in range(4):
        assert np.array_equal(ys[s].view(np.uint32), want.view(np.uint32)), ("shared", s)
    d_p.free(); d_i.free(); d_o.free()


@pytest.mark.parametrize("rate,pitch", [(1.0, float(np.float32(2 ** (3 / 12)))), (1.0, float(np.float32(2 ** (-7 / 12)))),
                                        (1.5, float(np.float32(1 / 1.5)))])
@pytest.mark.parametrize("n_fft", SIZES)
def test_stream_handle_equals_block(ctx, nae, n_fft, rate, pitch):
    """1152-frame puts and seeded random cuts, flush included, equal the block call bit for bit"""
    L, ch = 150000, 2
    x = (0.5 * orc.fill_uniform(L * ch, 7)).astype(np.float32)
    blk = block(ctx, nae, x, ch, rate, pitch, n_fft)
    rng = np.random.default_rng(n_fft)
    for puts in ([1152], [int(v) for v in rng.integers(1, 30000, 40)]):
        y = stream(ctx, x, ch, rate, pitch, puts, "n", n_fft)
        assert y.size == blk.size
        assert np.array_equal(y.view(np.uint32), blk.view(np.uint32)), puts[:4]


@pytest.mark.parametrize("n_fft", SIZES)
def test_stream_segment_of_many_tiles_after_one_block(ctx, nae, n_fft):
    """a first put that completes exactly one hop block (frames 0 .. 3 available), then the rest in one put: the second segment starts at
    frame 1 and is cut into 64-frame tiles, so its first pass-1 tile primes with frame 0; equal to the block call bit for bit"""
    L, ch, rate, pitch = 600000, 2, 1.5, float(np.float32(1 / 1.5))
    x = (0.5 * orc.fill_uniform(L * ch, 17)).astype(np.float32)
    ha = n_fft // 4 * 1.5
    first = int(2 * ha + n_fft // 2) + n_fft // 16             # frame 3 ends inside it, frame 4 does not
    assert 2 * ha + n_fft // 2 <= first < 3 * ha + n_fft // 2
    blk = block(ctx, nae, x, ch, rate, pitch, n_fft)
    y = stream(ctx, x, ch, rate, pitch, [first, L], "n", n_fft)
    assert y.size == blk.size
    assert np.array_equal(y.view(np.uint32), blk.view(np.uint32))


def test_python_stretcher_n_fft(ctx, nae):
    L, ch, pitch = 50000, 2, float(np.float32(2 ** (3 / 12)))
    x = (0.5 * orc.fill_uniform(L * ch, 11)).astype(np.float32)
    s = nae.Stretcher(ctx, 48000, ch, 1.0, pitch, n_fft=2048)
    s.put_host(x)
    s.flush()
    y = s.receive_host()
    s.close()
    assert np.array_equal(y.view(np.uint32), block(ctx, nae, x, ch, 1.0, pitch, 2048).view(np.uint32))


@pytest.mark.parametrize("n_fft", SIZES)
def test_non_finite_sample_is_confined(ctx, nae, ref, n_fft):
    """a NaN sample: non-finite output only where the restatement's is (the frames that contain it), the other channel and the rest within
    tolerance"""
    L, ch, pitch = 60000, 2, 2 ** (3 / 12)
    x = (0.5 * orc.fill_uniform(L * ch, 43)).reshape(L, ch).copy()
    x[30001, 0] = np.nan
    got = block(ctx, nae, x.reshape(-1), ch, 1.0, pitch, n_fft).reshape(-1, ch)
    want = pv_ref.stretch(ref, x.reshape(-1), ch, 1.0, pitch, n_fft).reshape(-1, ch)
    bad_ref, bad_got = ~np.isfinite(want), ~np.isfinite(got)
    assert not bad_ref[:, 1].any() and not bad_got[:, 1].any()
    assert 0 < bad_ref[:, 0].sum() < 4 * n_fft
    lo, hi = np.flatnonzero(bad_ref[:, 0])[[0, -1]]
    glo, ghi = np.flatnonzero(bad_got[:, 0])[[0, -1]]
    assert abs(int(lo) - int(glo)) <= 16 and abs(int(hi) - int(ghi)) <= 16, (lo, hi, glo, ghi)
    ok = np.ones(want.shape[0], bool)
    ok[min(lo, glo) - 16: max(hi, ghi) + 17] = False
    assert rel_rms(got[ok], want[ok]) <= TOL


@pytest.mark.parametrize("kind", ["noise", "tone"])
@pytest.mark.parametrize("rate,pitch", PAIRS)
def test_generic_kernels_at_1024_match_the_shipped_ones(nae, rate, pitch, kind):
    """pv_any = 1 routes 1024 through the size-generic kernels: the same integer phases bit for bit, samples within 1e-4"""
    L, ch = 40000, 2
    x = signal(kind, L, ch)
    res = {}
    for key in (0, 1):
        with nae.Context(0) as c:
            c.debug_set("pv_tile", 16)
            c.debug_set("pv_any", key)
            c.prof_reset(); c.prof_enable(True)
            res[key] = tile_phases(c, nae, x, ch, rate, pitch, 1024)[0], block(c, nae, x, ch, rate, pitch, 1024)
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert ("pv_any_synth_kernel" in launched) == (key == 1), launched
    assert np.array_equal(res[0][0], res[1][0])
    e = rel_rms(res[1][1], res[0][1])
    print(f"pv_any at 1024 {rate:.4f}/{pitch:.4f} {kind}: {e:.3g}")
    assert e <= TOL, e


def test_n_1024_is_the_ex_call(ctx, nae):
    lib = ctx.lib
    L, ch, rate, pitch = 40000, 2, 1.0, 2 ** (3 / 12)
    x = orc.fill_uniform(L * ch, 5)
    pl = ctx.stretch_plan(rate, pitch, L)
    d_x, d_a, d_b = ctx.array(x), ctx.empty(pl.out_len * ch), ctx.empty(pl.out_len * ch)
    src = nae.Sig.interleaved(d_x.ptr, L, ch)
    for flags in (0, 1):
        assert lib.nae_stretch_block_ex_f32(ctx.h, rate, pitch, flags, C.byref(src), L, ch, 1,
                                            C.byref(nae.Sig.interleaved(d_a.ptr, pl.out_len, ch))) == 0
        assert lib.nae_stretch_block_n_f32(ctx.h, rate, pitch, flags, 1024, C.byref(src), L, ch, 1,
                                           C.byref(nae.Sig.interleaved(d_b.ptr, pl.out_len, ch))) == 0
        assert np.array_equal(d_a.download().view(np.uint32), d_b.download().view(np.uint32)), flags
        cap = ch * (pl.frames + 1) * 513
        a, b = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        nt, tf, nt2, tf2 = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.nae_debug_pv_tile_phase_ex(ctx.h, rate, pitch, flags, C.byref(src), L, ch, 1, a.ctypes.data, cap, C.byref(nt), C.byref(tf)) == 0
        assert lib.nae_debug_pv_tile_phase_n(ctx.h, rate, pitch, flags, 1024, C.byref(src), L, ch, 1, b.ctypes.data, cap, C.byref(nt2),
                                             C.byref(tf2)) == 0
        assert (nt.value, tf.value) == (nt2.value, tf2.value) and np.array_equal(a, b)
    d_x.free(); d_a.free(); d_b.free()


def test_error_codes(ctx, nae):
    lib = ctx.lib
    L, ch = 4096, 2
    d_x, d_o = ctx.empty(L * ch), ctx.empty(2 * L * ch)
    src, dst = nae.Sig.interleaved(d_x.ptr, L, ch), nae.Sig.interleaved(d_o.ptr, 2 * L, ch)
    h = C.c_void_p()
    nt, tf = C.c_size_t(), C.c_size_t()
    buf = np.zeros(64 * 2049 * ch, np.int32)

    def all3(flags, n_fft):
        return (lib.nae_stretch_block_n_f32(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, C.byref(dst)),
                lib.nae_stretch_create_n(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, C.byref(h)),
                lib.nae_debug_pv_tile_phase_n(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size,
                                              C.byref(nt), C.byref(tf)))

    for n_fft in (256, 8192, 1000, 0):
        assert all3(0, n_fft) == (-2, -2, -2), n_fft                       # NAE_ERR_UNSUPPORTED
    for n_fft in (512, 2048, 4096):
        assert all3(1, n_fft) == (-2, -2, -2), n_fft                       # phase lock at a size other than 1024
        assert all3(2, n_fft) == (-1, -1, -1), n_fft                       # unknown flag: NAE_ERR_INVALID
        ok = all3(0, n_fft)
        assert lib.nae_stretch_destroy(h) == 0
        assert ok == (0, 0, 0), n_fft
    d_x.free(); d_o.free()


def test_host_graph_pitch_node_fft_size(tmp_path, ref):
    """source -> Pitch_modifier {"pitch": 3, "fft_size": 4096} -> sink through the fiber runner equals the 4096-point block call bit for bit
    (host mirror) and the CPU restatement within 1e-4"""
    import subprocess
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    out = str(tmp_path / "graph.f32")
    r = subprocess.run([exe, "gpu", "fft_size", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST PV NODE OK gpu fft_size" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    data = np.fromfile(out, np.float32)
    x, got = data[: 60000 * 2], data[60000 * 2:]
    pitch = float(np.float32(2 ** (3 / 12)))
    want = pv_ref.stretch(ref, x, 2, 1.0, pitch, 4096)
    assert got.size == want.size
    assert rel_rms(got, want) <= TOL, rel_rms(got, want)
