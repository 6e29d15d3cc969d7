"""Formant-preserving pitch shift on the GPU ("Formant preservation"), against the CPU statement tests/pv_formant/ref_pv_formant.c.

Bars: samples within 1e-4 relative RMS at every frame size, in both stage orders, mono and stereo, interleaved and planar, locked at 1024, on
the formant kernels; without a pitch change a lifter changes no bit; every tiling, batch position and the streaming handle give the same
bits; the new entries' error codes; the host graph equals the block call."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import orc
import pv_formant_ref
from conftest import rel_rms

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
ORDERS = [(1.0, 2.0), (0.25, 2.0), (1.0, 2 ** (4 / 12)), (1.0, 2 ** (-5 / 12))]   # rho = 2 / 1.26: transposer first; 1/2 / 0.75: vocoder first
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_formant_ref.build(str(tmp_path_factory.mktemp("ref_pv_formant")))


def vowel(L, f0=140.0, sr=48000):
    t = np.arange(L) / sr
    env = lambda f: 0.03 + np.exp(-0.5 * ((f - 700) / 130) ** 2) + 0.6 * np.exp(-0.5 * ((f - 1200) / 150) ** 2) + 0.3 * np.exp(-0.5 * ((f - 2600) / 220) ** 2)
    y = np.zeros(L)
    for h in range(1, int(8000 / f0)):
        y += env(h * f0) * np.sin(2 * np.pi * h * f0 * t + 0.7 * h * h)
    return (0.1 * y).astype(np.float32)


def signal(kind, L, ch, seed=41):
    if kind == "noise":
        return orc.fill_uniform(L * ch, seed)
    m = vowel(L)
    return np.stack([m, 0.5 * m], 1).reshape(-1).astype(np.float32) if ch == 2 else m


def run(ctx, nae, x, ch, rate, pitch, n_fft, lifter, lock=False, n_streams=1, planar=False):
    L = x.size // (ch * n_streams)
    pl = ctx.stretch_plan(rate, pitch, L, n_fft)
    if planar:
        assert n_streams == 1
        xp = np.ascontiguousarray(x.reshape(L, ch).T).reshape(-1)
        d_x, d_o = ctx.array(xp), ctx.empty(max(1, pl.out_len * ch))
        ctx.stretch_block(rate, pitch, nae.Sig.planar(d_x.ptr, L, ch), L, ch, 1, nae.Sig.planar(d_o.ptr, pl.out_len, ch), phase_lock=lock,
                          n_fft=n_fft, formant=lifter)
        out = d_o.download()[: pl.out_len * ch].reshape(ch, -1).T.reshape(-1).copy()
    else:
        d_x, d_o = ctx.array(x), ctx.empty(max(1, n_streams * pl.out_len * ch))
        ctx.stretch_block(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch),
                          phase_lock=lock, n_fft=n_fft, formant=lifter)
        out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    return out


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", ORDERS)
@pytest.mark.parametrize("n_fft", SIZES)
def test_samples_vs_statement(nae, ref, n_fft, rate, pitch, ch, planar):
    """noise and a vowel, within 1e-4 of the statement; the formant synthesis kernel ran and the unflagged one did not"""
    L, q = 30000, pv_formant_ref.default_lifter(48000, n_fft)
    with nae.Context(0) as c:
        for kind in ("noise", "vowel"):
            x = signal(kind, L, ch, 43)
            c.prof_reset(); c.prof_enable(True)
            got = run(c, nae, x, ch, rate, pitch, n_fft, q, planar=planar)
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert "pv_any_synth_formant_kernel" in launched and "pv_any_synth_kernel" not in launched, launched
            assert not any(k.startswith("pv_pipe") or k.startswith("pv_flow") for k in launched), launched
            want = pv_formant_ref.stretch(ref, x, ch, rate, pitch, n_fft, q)
            assert got.size == want.size and np.isfinite(got).all()
            e = rel_rms(got, want)
            print(f"N={n_fft} {rate:.4f}/{pitch:.4f} {kind} ch{ch} planar={planar}: {e:.3g}")
            assert e <= TOL, e


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("rate,pitch", ORDERS)
def test_locked_formant_vs_statement(nae, ref, rate, pitch, ch):
    L, q = 30000, pv_formant_ref.default_lifter(48000, 1024)
    with nae.Context(0) as c:
        for kind in ("noise", "vowel"):
            x = signal(kind, L, ch, 45)
            c.prof_reset(); c.prof_enable(True)
            got = run(c, nae, x, ch, rate, pitch, 1024, q, lock=True)
            c.prof_enable(False)
            launched = set(c.prof_report())
            assert "pvlock_synth_formant_kernel" in launched and "pvlock_synth_kernel" not in launched, launched
            want = pv_formant_ref.stretch(ref, x, ch, rate, pitch, 1024, q, lock=True)
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
        a = run(ctx, nae, x, ch, rate, pitch, n_fft, 0, lock=lock)
        b = run(ctx, nae, x, ch, rate, pitch, n_fft, n_fft // 4, lock=lock)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), n_fft


@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (2048, False), (4096, False)])
def test_every_tiling_gives_the_same_bits(nae, n_fft, lock):
    ch, rate, pitch = 2, 1.0, 2 ** (4 / 12)
    L = 300 * (n_fft // 4) + 4096
    x = (0.5 * orc.fill_uniform(L * ch, 99)).astype(np.float32)
    q = pv_formant_ref.default_lifter(48000, n_fft)
    outs = {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("1-frame tiles", {"pv_tile": 1}), ("16-frame tiles", {"pv_tile": 16}),
                       ("64-frame tiles", {"pv_tile": 64}), ("min 100", {"pv_min_ptile": 100}), ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            outs[key] = run(c, nae, x, ch, rate, pitch, n_fft, q, lock=lock)
    for key in outs:
        assert np.array_equal(outs[key].view(np.uint32), outs["one tile"].view(np.uint32)), key


@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (4096, False)])
def test_forty_streams_each_equal_their_lone_run(ctx, nae, n_fft, lock):
    n, L, ch, rate, pitch = 40, 12000, 2, 1.0, 2 ** (-5 / 12)
    x = orc.fill_uniform(n * L * ch, 47)
    q = pv_formant_ref.default_lifter(44100, n_fft)
    got = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock=lock, n_streams=n).reshape(n, -1)
    for s in range(n):
        one = run(ctx, nae, x.reshape(n, -1)[s].copy(), ch, rate, pitch, n_fft, q, lock=lock)
        assert np.array_equal(one.view(np.uint32), got[s].view(np.uint32)), s


def stream(ctx, x, ch, rate, pitch, n_fft, lifter, lock, put_sizes):
    lib = ctx.lib
    L = x.size // ch
    h = C.c_void_p()
    assert lib.nae_stretch_create_formant(ctx.h, 48000, ch, rate, pitch, 1 if lock else 0, n_fft, lifter, C.byref(h)) == 0
    outs, pos, i = [], 0, 0

    def drain():
        n = lib.nae_stretch_available(h)
        if n:
            buf = np.empty(n * ch, np.float32)
            got = C.c_size_t()
            assert lib.nae_stretch_receive_host(h, buf.ctypes.data, n, C.byref(got)) == 0
            outs.append(buf[: got.value * ch])

    while pos < L:
        n = min(put_sizes[i % len(put_sizes)], L - pos)
        i += 1
        chunk = np.ascontiguousarray(x[pos * ch:(pos + n) * ch])
        assert lib.nae_stretch_put_host(h, chunk.ctypes.data, n) == 0
        pos += n
        drain()
    assert lib.nae_stretch_flush(h) == 0
    drain()
    assert lib.nae_stretch_destroy(h) == 0
    return np.concatenate(outs) if outs else np.zeros(0, np.float32)


@pytest.mark.parametrize("rate,pitch", [(1.0, float(np.float32(2 ** (4 / 12)))), (1.0, float(np.float32(2 ** (-5 / 12))))])
@pytest.mark.parametrize("n_fft,lock", [(512, False), (1024, False), (1024, True), (2048, False), (4096, False)])
def test_stream_handle_equals_block(ctx, nae, n_fft, lock, rate, pitch):
    """puts of one vocoder hop (one frame each), seeded random cuts, flush: equal to the block call bit for bit"""
    L, ch = 40000, 2
    x = (0.5 * orc.fill_uniform(L * ch, 7)).astype(np.float32)
    q = pv_formant_ref.default_lifter(48000, n_fft)
    blk = run(ctx, nae, x, ch, rate, pitch, n_fft, q, lock=lock)
    rng = np.random.default_rng(n_fft + lock)
    for puts in ([n_fft // 4], [int(v) for v in rng.integers(1, 12000, 12)]):
        y = stream(ctx, x, ch, rate, pitch, n_fft, q, lock, puts)
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
    assert np.array_equal(y.view(np.uint32), run(ctx, nae, x, ch, 1.0, pitch, 2048, q).view(np.uint32))


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
    from test_pv_formant_cpu import build_host_pv_formant
    exe = build_host_pv_formant(str(tmp_path))
    out = str(tmp_path / "graph.f32")
    r = subprocess.run([exe, "gpu", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST PV FORMANT OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    data = np.fromfile(out, np.float32)
    x, got = data[: 60000 * 2], data[60000 * 2:]
    pitch = float(np.float32(2 ** (4 / 12)))
    want = pv_formant_ref.stretch(ref, x, 2, 1.0, pitch, 1024, 68)
    assert got.size == want.size
    assert rel_rms(got, want) <= TOL, rel_rms(got, want)
