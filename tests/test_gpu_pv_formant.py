"""Formant-preserving pitch shift on the GPU ("Formant preservation"), against the CPU statement tests/pv_ref/ref_pv.c.

Bars: samples within 1e-4 relative RMS at every frame size, in both stage orders, mono and stereo, interleaved and planar, locked at 1024, on
the formant kernels; without a pitch change a lifter changes no bit; every tiling, batch position and the streaming handle give the same
bits; the new entries' error codes; the host graph equals the block call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_gpu
import pv_ref
from conftest import rel_rms
from pv_gpu import block, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
ORDERS = [(1.0, 2.0), (0.25, 2.0), (1.0, 2 ** (4 / 12)), (1.0, 2 ** (-5 / 12))]   # rho = 2 / 1.26: transposer first; 1/2 / 0.75: vocoder first
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def vowel(L, f0=140.0, sr=48000):
    t = np.arange(L) / sr
    env = lambda f: 0.03 + np.exp(-0.5 * ((f - 700) / 130) ** 2) + 0.6 * np.exp(-0.5 * ((f - 1200) / 150) ** 2) + 0.3 * np.exp(-0.5 * ((f - 2600) / 220) ** 2)
    y = np.zeros(L)
    for h in range(1, int(8000 / f0)):
        y += env(h * f0) * np.sin(2 * np.pi * h * f0 * t + 0.7 * h * h)
    return (0.1 * y).astype(np.float32)


def signal(kind, L, ch, seed=41):
    return pv_gpu.signal(kind, L, ch, seed, vowel)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", ORDERS)
@pytest.mark.parametrize("n_fft", SIZES)
def test_samples_vs_statement(nae, ref, n_fft, rate, pitch, ch, planar):
    """noise and a vowel, within 1e-4 of the statement; the formant synthesis kernel ran and the unflagged one did not"""
    L, q = 30000, pv_ref.default_lifter(48000, n_fft)
    with nae.Context(0) as c:
        for kind in ("noise", "vowel"):
            x = signal(kind, L, ch, 43)
            c.prof_reset(); c.prof_enable(True)
            got = block(c, nae, x, ch, rate, pitch, n_fft, lifter=q, planar_in=planar, planar_out=planar)
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert "pv_any_synth_formant_kernel" in launched and "pv_any_synth_kernel" not in launched, launched
            assert not any(k.startswith("pv_pipe") or k.startswith("pv_flow") for k in launched), launched
            want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lifter=q)
            assert got.size == want.size and np.isfinite(got).all()
            e = rel_rms(got, want)
            print(f"N={n_fft} {rate:.4f}/{pitch:.4f} {kind} ch{ch} planar={planar}: {e:.3g}")
            assert e <= TOL, e


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", ORDERS)
def test_locked_formant_vs_statement(nae, ref, rate, pitch, ch):
    L, q = 30000, pv_ref.default_lifter(48000, 1024)
    with nae.Context(0) as c:
        for kind in ("noise", "vowel"):
            x = signal(kind, L, ch, 45)
            c.prof_reset(); c.prof_enable(True)
            got = block(c, nae, x, ch, rate, pitch, 1024, lock=True, lifter=q)
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert "pvlock_synth_formant_kernel" in launched and "pvlock_synth_kernel" not in launched, launched
            want = pv_ref.stretch(ref, x, ch, rate, pitch, 1024, lock=True, lifter=q)
            assert got.size == want.size and np.isfinite(got).all()
            e = rel_rms(got, want)
            print(f"locked {rate:.4f}/{pitch:.4f} {kind} ch{ch}: {e:.3g}")
            assert e <= TOL, e


@pytest.mark.parametrize("lock", [False, True])
@pytest.mark.parametrize("rate,pitch", [(0.5, 2.0), (1.5, 1 / 1.5), (2.0, 1.0), (1.0, 1.0)])
def test_no_pitch_change_is_the_n_call(ctx, nae, rate, pitch, lock):
    """rho = 1 (a tempo change alone), the transposer alone and neither stage: a lifter changes no bit"""
    L, ch = 30000, 2
    x = orc.fill_uniform(L * ch, 9)
    for n_fft in ([1024] if lock else SIZES):
        a = block(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=0)
        b = block(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=n_fft // 4)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n_fft


@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (2048, False), (4096, False)])
def test_every_tiling_gives_the_same_bits(nae, n_fft, lock):
    ch, rate, pitch = 2, 1.0, 2 ** (4 / 12)
    L = 300 * (n_fft // 4) + 4096
    x = (0.5 * orc.fill_uniform(L * ch, 99)).astype(np.float32)
    q = pv_ref.default_lifter(48000, n_fft)
    outs = {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("1-frame tiles", {"pv_tile": 1}), ("16-frame tiles", {"pv_tile": 16}),
                       ("64-frame tiles", {"pv_tile": 64}), ("min 100", {"pv_min_ptile": 100}), ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            outs[key] = block(c, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=q)
    for key in outs:
        assert np.array_equal(outs[key].view(np.uint32), outs["one tile"].view(np.uint32)), key


@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (4096, False)])
def test_forty_streams_each_equal_their_lone_run(ctx, nae, n_fft, lock):
    n, L, ch, rate, pitch = 40, 12000, 2, 1.0, 2 ** (-5 / 12)
    x = orc.fill_uniform(n * L * ch, 47)
    q = pv_ref.default_lifter(44100, n_fft)
    got = block(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=q, n_streams=n).reshape(n, -1)
    for s in range(n):
        one = block(ctx, nae, x.reshape(n, -1)[s].copy(), ch, rate, pitch, n_fft, lock=lock, lifter=q)
        assert np.array_equal(one.view(np.uint32), got[s].view(np.uint32)), s


@pytest.mark.parametrize("rate,pitch", [(1.0, float(np.float32(2 ** (4 / 12)))), (1.0, float(np.float32(2 ** (-5 / 12))))])
@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (2048, False), (4096, False)])
def test_stream_handle_equals_block(ctx, nae, n_fft, lock, rate, pitch):
    """puts of one vocoder hop (one frame each), seeded random cuts, flush: equal to the block call bit for bit"""
    L, ch = 40000, 2
    x = (0.5 * orc.fill_uniform(L * ch, 7)).astype(np.float32)
    q = pv_ref.default_lifter(48000, n_fft)
    blk = block(ctx, nae, x, ch, rate, pitch, n_fft, lock=lock, lifter=q)
    rng = np.random.default_rng(n_fft + lock)
    for puts in ([n_fft // 4], [int(v) for v in rng.integers(1, 12000, 12)]):
        y = stream(ctx, x, ch, rate, pitch, puts, "formant", n_fft, flags=int(lock), lifter=q)
        assert y.size == blk.size
        assert np.array_equal(y.view(np.uint32), blk.view(np.uint32)), puts[:4]


def test_python_stretcher_formant(ctx, nae):
    L, ch, pitch = 50000, 2, float(np.float32(2 ** (4 / 12)))
    x = (0.5 * orc.fill_uniform(L * ch, 11)).astype(np.float32)
    q = nae.formant_lifter(48000, 2048)
    s = nae.Stretcher(ctx, 48000, ch, 1.0, pitch, n_fft=2048, formant=q)
    s.put_host(x)
    s.flush()
    y = s.receive_host()
    s.close()
    assert np.array_equal(y.view(np.uint32), block(ctx, nae, x, ch, 1.0, pitch, 2048, lifter=q).view(np.uint32))


def test_error_codes(ctx, nae):
    lib = ctx.lib
    L, ch = 4096, 2
    d_x, d_o = ctx.empty(L * ch), ctx.empty(2 * L * ch)
    src, dst = nae.Sig.interleaved(d_x.ptr, L, ch), nae.Sig.interleaved(d_o.ptr, 2 * L, ch)
    h = C.c_void_p()

    def both(flags, n_fft, lifter):
        a = lib.nae_stretch_block_formant_f32(ctx.h, 1.0, 1.2, flags, n_fft, lifter, C.byref(src), L, ch, 1, C.byref(dst))
        b = lib.nae_stretch_create_formant(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, lifter, C.byref(h))
        if b == 0:
            assert lib.nae_stretch_destroy(h) == 0
        return a, b

    for n_fft in (256, 8192, 1000):
        assert both(0, n_fft, 1) == (UNSUPPORTED, UNSUPPORTED), n_fft
    for n_fft in (512, 2048, 4096):
        assert both(1, n_fft, 1) == (UNSUPPORTED, UNSUPPORTED), n_fft        # phase lock at a size other than 1024
    for n_fft in SIZES:
        assert both(2, n_fft, 1) == (INVALID, INVALID), n_fft                # unknown flag
        assert both(0, n_fft, -1) == (INVALID, INVALID), n_fft
        assert both(0, n_fft, n_fft // 4 + 1) == (INVALID, INVALID), n_fft
        assert both(0, n_fft, n_fft // 4) == (0, 0), n_fft
        assert both(0, n_fft, 0) == (0, 0), n_fft
    assert both(1, 1024, 256) == (0, 0)
    assert lib.nae_stretch_block_formant_f32(None, 1.0, 1.2, 0, 1024, 1, C.byref(src), L, ch, 1, C.byref(dst)) == INVALID
    d_x.free(); d_o.free()


def test_host_graph_pitch_node_formant(tmp_path, ref):
    """source -> Pitch_modifier {"pitch": 4, "formant": true} -> sink through the fiber runner equals the formant block call bit for bit
    (host mirror) and the CPU statement within 1e-4"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    out = str(tmp_path / "graph.f32")
    r = subprocess.run([exe, "gpu", "formant", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST PV NODE OK gpu formant" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    data = np.fromfile(out, np.float32)
    x, got = data[: 60000 * 2], data[60000 * 2:]
    pitch = float(np.float32(2 ** (4 / 12)))
    want = pv_ref.stretch(ref, x, 2, 1.0, pitch, 1024, lifter=68)
    assert got.size == want.size
    assert rel_rms(got, want) <= TOL, rel_rms(got, want)
