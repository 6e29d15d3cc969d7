"""Formant shift independent of the pitch on the GPU ("Formant shift"), against the CPU statement tests/pv_ref/ref_pv.c.

Cases: A a pitch change (both stage orders), B a tempo change only, C a rate change only (both orders; the forced stage with the transposer),
D neither (the forced stage alone).  Bars: samples within 1e-4 relative RMS, the project's vocoder bar, at every frame size, mono and stereo,
interleaved and planar, formant_ratio on both sides of 1; lifter 0 is the _n call and formant_ratio 1 the _formant call bit for bit; every
tiling, batch position and the streaming handle give the block call's bits; the forced stage ignores the lock and transient preservation; the
new entries' error codes; the host graph equals the block call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import node_harness
import orc
import pv_gpu
import pv_ref
from conftest import rel_rms
from pv_gpu import same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
CASES = {"A_first": (1.0, 2 ** (4 / 12)), "A_last": (1.0, 2 ** (-5 / 12)), "B": (1.5, 1 / 1.5), "C_last": (0.8, 1.0), "C_first": (1.25, 1.0),
         "D": (1.0, 1.0)}
UP, DOWN = 2 ** (3 / 12), 2 ** (-4 / 12)     # neither equals a case's rate_eff: the envelope stage runs in every case
INVALID, UNSUPPORTED = -1, -2
LOCK, TRANSIENTS = 1, 4


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def block(c, nae, x, ch, rate, pitch, phi, n_fft=1024, lifter=0, lock=False, transients=False, n_streams=1, planar=False):
    """nae_stretch_block_formant_shift_f32 on x, [n_streams][L][ch] flattened -> interleaved [n_streams * out_len * ch]"""
    L = x.size // (ch * n_streams)
    pl = c.stretch_plan(rate, pitch, L, n_fft, formant=lifter, formant_ratio=phi)
    flat = np.ascontiguousarray(x.reshape(n_streams, L, ch).transpose(0, 2, 1)).reshape(-1) if planar else x
    d_x, d_o = c.array(np.ascontiguousarray(flat, np.float32)), c.empty(max(1, n_streams * pl.out_len * ch))
    src = nae.Sig.planar(d_x.ptr, L, ch) if planar else nae.Sig.interleaved(d_x.ptr, L, ch)
    dst = nae.Sig.planar(d_o.ptr, pl.out_len, ch) if planar else nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)
    c.stretch_block(rate, pitch, src, L, ch, n_streams, dst, phase_lock=lock, n_fft=n_fft, formant=lifter, transients=transients,
                    formant_ratio=phi)
    out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    if planar:
        out = np.ascontiguousarray(out.reshape(n_streams, ch, pl.out_len).transpose(0, 2, 1)).reshape(-1)
    return out


def forced(case):
    return case[0] in "CD"


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n_fft", SIZES)
def test_samples_vs_statement(nae, ref, n_fft, case, record_property):
    """noise, within 1e-4 of the statement, mono interleaved and stereo planar, formant_ratio above and below 1; cases C and D run
    pv_env_kernel and no phase pass, cases A and B the formant pass 3"""
    rate, pitch = CASES[case]
    L, q = 20000, pv_ref.default_lifter(48000, n_fft)
    with nae.Context(0) as c:
        for ch, planar, phi in ((1, False, UP), (2, True, DOWN), (2, False, UP), (1, True, DOWN)):
            x = pv_gpu.signal("noise", L, ch, 43)
            got, launched = pv_gpu.profiled(c, block, c, nae, x, ch, rate, pitch, phi, n_fft, q, planar=planar)
            if forced(case):
                assert "pv_env_kernel" in launched and not any(k.startswith("pv_any") or k.startswith("pv_phase") or "scan" in k for k in launched), launched
            else:
                assert "pv_any_synth_formant_kernel" in launched and "pv_env_kernel" not in launched, launched
            want = pv_ref.stretch(ref, x, ch, rate, pitch, n_fft, lifter=q, formant_ratio=phi)
            assert got.size == want.size
            e = rel_rms(got, want)
            print(f"fshift {case} N={n_fft} ch={ch} planar={planar} phi={phi:.4f}: {e:.3e}")
            assert e <= TOL, (ch, planar, phi, e)


def test_locked_pitch_change_vs_locked_statement(nae, ref):
    """case A at 1024 with NAE_STRETCH_PHASE_LOCK against the locked statement"""
    x = pv_gpu.signal("noise", 20000, 2, 47)
    with nae.Context(0) as c:
        for name in ("A_first", "A_last"):
            rate, pitch = CASES[name]
            got = block(c, nae, x, 2, rate, pitch, DOWN, 1024, 68, lock=True)
            want = pv_ref.stretch(ref, x, 2, rate, pitch, 1024, lock=True, lifter=68, formant_ratio=DOWN)
            e = rel_rms(got, want)
            print(f"fshift locked {name}: {e:.3e}")
            assert got.size == want.size and e <= TOL, e


@pytest.mark.parametrize("n_fft", SIZES)
def test_lifter_zero_and_ratio_one_bits(nae, n_fft):
    """lifter 0 with any ratio is the _n call; formant_ratio 1 is the _formant call in cases A, B, D"""
    q = pv_ref.default_lifter(48000, n_fft)
    x = pv_gpu.signal("noise", 15000, 2, 51)
    with nae.Context(0) as c:
        for case, (rate, pitch) in CASES.items():
            plain = pv_gpu.block(c, nae, x, 2, rate, pitch, n_fft)
            for phi in (0.25, DOWN, UP, 4.0):
                assert same_bits(block(c, nae, x, 2, rate, pitch, phi, n_fft, 0), plain), (case, phi)
            if not case.startswith("C"):
                assert same_bits(block(c, nae, x, 2, rate, pitch, 1.0, n_fft, q), pv_gpu.block(c, nae, x, 2, rate, pitch, n_fft, lifter=q)), case
            else:   # the _formant entry is a plain resampling there; the new entry with ratio 1 runs the envelope stage
                assert same_bits(pv_gpu.block(c, nae, x, 2, rate, pitch, n_fft, lifter=q), plain)
                assert not same_bits(block(c, nae, x, 2, rate, pitch, 1.0, n_fft, q), plain)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tilings_and_batch_give_the_same_bits(nae, case):
    """pv_tile = 7, 64, 1000 against the default tiling; a 40-stream batch against 40 lone runs; every N"""
    rate, pitch = CASES[case]
    L, ch = 12000, 2
    for n_fft in SIZES:
        q = pv_ref.default_lifter(48000, n_fft)
        xs = np.concatenate([pv_gpu.signal("noise", L, ch, 100 + s) for s in range(40)])
        with nae.Context(0) as c:
            base = block(c, nae, xs, ch, rate, pitch, UP, n_fft, q, n_streams=40)
            lone = np.concatenate([block(c, nae, xs[s * L * ch:(s + 1) * L * ch], ch, rate, pitch, UP, n_fft, q) for s in range(40)])
            assert same_bits(base, lone), n_fft
        for tile in (7, 64, 1000):
            with nae.Context(0) as c:
                c.debug_set("pv_tile", tile)
                assert same_bits(block(c, nae, xs[: 3 * L * ch], ch, rate, pitch, UP, n_fft, q, n_streams=3), base[: 3 * (base.size // 40)]), (n_fft, tile)


def stream(c, x, ch, rate, pitch, phi, put_sizes, n_fft, lifter, flags=0):
    lib = c.lib
    L = x.size // ch
    h = C.c_void_p()
    assert lib.nae_stretch_create_formant_shift(c.h, 48000, ch, rate, pitch, flags, n_fft, lifter, phi, C.byref(h)) == 0
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


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n_fft", SIZES)
def test_streaming_handle_equals_the_block_call(nae, n_fft, case):
    """random cuts into put calls, flush included: the block call's bits"""
    rate, pitch = CASES[case]
    # the handle takes float rate / pitch: the block call gets the same values
    rate, pitch = float(np.float32(rate)), float(np.float32(pitch))
    q = pv_ref.default_lifter(48000, n_fft)
    rng = np.random.default_rng(n_fft + len(case))
    for ch in (1, 2):
        x = pv_gpu.signal("noise", 30011, ch, 61)
        cuts = [int(v) for v in rng.integers(1, 5000, 64)]
        with nae.Context(0) as c:
            want = block(c, nae, x, ch, rate, pitch, DOWN, n_fft, q)
            got = stream(c, x, ch, rate, pitch, DOWN, cuts, n_fft, q)
            assert same_bits(got, want), (ch, got.size, want.size)
            one = stream(c, x, ch, rate, pitch, DOWN, [x.size], n_fft, q)
            assert same_bits(one, want), ch


def test_forced_stage_ignores_lock_and_transients(nae):
    """case D (and C) with the lock (1024) or transient preservation: the unflagged call's bits, block call and handle"""
    x = pv_gpu.signal("noise", 20000, 2, 71)
    x[8000:8002] = 0.9
    with nae.Context(0) as c:
        for case in ("D", "C_first", "C_last"):
            rate, pitch = (float(np.float32(v)) for v in CASES[case])     # the handle takes floats
            for n_fft in SIZES:
                q = pv_ref.default_lifter(48000, n_fft)
                base = block(c, nae, x, 2, rate, pitch, UP, n_fft, q)
                assert same_bits(block(c, nae, x, 2, rate, pitch, UP, n_fft, q, transients=True), base), (case, n_fft)
                assert same_bits(stream(c, x, 2, rate, pitch, UP, [3000, 777], n_fft, q, TRANSIENTS), base), (case, n_fft)
                if n_fft == 1024:
                    assert same_bits(block(c, nae, x, 2, rate, pitch, UP, n_fft, q, lock=True), base), case
                    assert same_bits(block(c, nae, x, 2, rate, pitch, UP, n_fft, q, lock=True, transients=True), base), case
                    assert same_bits(stream(c, x, 2, rate, pitch, UP, [3000, 777], n_fft, q, LOCK | TRANSIENTS), base), case


def test_python_stretcher_equals_the_block_call(nae):
    x = pv_gpu.signal("noise", 25000, 2, 81)
    with nae.Context(0) as c:
        for case in ("D", "A_first", "B"):
            rate, pitch = (float(np.float32(v)) for v in CASES[case])
            want = block(c, nae, x, 2, rate, pitch, UP, 2048, 68)
            s = nae.Stretcher(c, 48000, 2, rate, pitch, n_fft=2048, formant=68, formant_ratio=UP)
            outs = []
            for pos in range(0, 25000, 4096):
                s.put_host(x[pos * 2:(pos + 4096) * 2])
                outs.append(s.receive_host())
            s.flush()
            outs.append(s.receive_host())
            s.close()
            assert same_bits(np.concatenate(outs), want), case


def test_error_codes(nae):
    with nae.Context(0) as c:
        lib = c.lib
        d_x, d_o = c.empty(4000), c.empty(16000)
        src, dst = nae.Sig.interleaved(d_x.ptr, 2000, 2), nae.Sig.interleaved(d_o.ptr, 2000, 2)

        def blk(phi, flags=0, n_fft=1024, lifter=68, ctx=c.h, pitch=1.0):
            return lib.nae_stretch_block_formant_shift_f32(ctx, 1.0, pitch, flags, n_fft, lifter, phi, C.byref(src), 2000, 2, 1, C.byref(dst))

        def mk(phi, flags=0, n_fft=1024, lifter=68, ctx=c.h):
            h = C.c_void_p()
            rc = lib.nae_stretch_create_formant_shift(ctx, 48000, 2, 1.0, 1.0, flags, n_fft, lifter, phi, C.byref(h))
            if rc == 0:
                assert lib.nae_stretch_destroy(h) == 0
            return rc

        for f in (blk, mk):
            for phi in (0.0, -2.0, float("nan")):
                assert f(phi) == INVALID, (f.__name__, phi)
            for phi in (0.2, 5.0):
                assert f(phi) == UNSUPPORTED, (f.__name__, phi)
            for phi in (0.25, 1.0, 4.0):
                assert f(phi) == 0, (f.__name__, phi)
            assert f(UP, lifter=-1) == INVALID and f(UP, lifter=257) == INVALID and f(UP, lifter=256) == 0
            assert f(UP, n_fft=2048, lifter=512) == 0 and f(UP, n_fft=2048, lifter=513) == INVALID
            assert f(UP, flags=8) == INVALID and f(UP, flags=2) == INVALID
            assert f(UP, n_fft=1000) == UNSUPPORTED
            assert f(UP, flags=LOCK, n_fft=2048) == UNSUPPORTED and f(UP, flags=LOCK | TRANSIENTS, n_fft=512) == UNSUPPORTED
            assert f(UP, flags=LOCK) == 0 and f(UP, flags=LOCK | TRANSIENTS) == 0 and f(UP, flags=TRANSIENTS, n_fft=4096) == 0
            assert f(UP, ctx=None) == INVALID
        assert blk(UP, pitch=100.0) == UNSUPPORTED
        h = C.c_void_p()
        assert lib.nae_stretch_create_formant_shift(c.h, 48000, 2, 1.0, 1.0, 0, 1024, 68, UP, None) == INVALID
        d_x.free(); d_o.free()


@pytest.mark.parametrize("pitch_st,shift_st", [(0, 4), (4, -3)])
def test_host_graph(ref, tmp_path, pitch_st, shift_st):
    """source -> Pitch_modifier {"pitch": p, "formant_shift": s} -> sink through the fiber runner: the block call's bits (checked by the
    harness), and the CPU statement within 1e-4"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    fin, fout = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    r = subprocess.run([exe, "gpu", "formant_shift", str(pitch_st), str(shift_st), fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "HOST PV NODE OK gpu formant_shift" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    x, got = np.fromfile(fin, np.float32), np.fromfile(fout, np.float32)
    pitch = float(np.float32(2.0) ** np.float32(pitch_st / 12.0))
    want = pv_ref.stretch(ref, x, 2, 1.0, pitch, 1024, lifter=68, formant_ratio=2 ** (shift_st / 12))
    e = rel_rms(got, want)
    print(f"fshift host graph pitch {pitch_st:+d} shift {shift_st:+d}: {e:.3e}")
    assert got.size == want.size and e <= TOL, e
