"""Channel link (NAE_STRETCH_LINK_CHANNELS; DESIGN.md §3, "Channel link") on the GPU, against the CPU statement
tests/pv_ref/ref_pv.c.

Routes: every size with transient preservation, 1024 with the lock, 1024 with the lock and transient preservation.
Bars: the integer synthesis phases are bit-exact at every route and tiling (the chunked scan from 256 tiles on included); the samples are
within 1e-4 relative RMS of the statement, with and without the formant lifter and with the formant shift (cases A and B); every tiling,
the streaming handle and a batch give the lone block call's bits; where the link is not effective the call gives the unflagged call's bits;
the error codes, a NaN in one channel, and the host graph."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import node_harness
import pv_ref
from conftest import rel_rms
from pv_gpu import profiled, same_bits, scene, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
SIZES = [512, 1024, 2048, 4096]
LOCK, TR, LINK = 1, 4, 16                                   # NAE_STRETCH_PHASE_LOCK, _TRANSIENTS, _LINK_CHANNELS
PAIRS = [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12)), (1.5, 1 / 1.5)]   # transposer first, after, none
# (n_fft, lock, transients)
ROUTES = [pytest.param(512, False, True, id="512-tr"), pytest.param(1024, False, True, id="1024-tr"),
          pytest.param(1024, True, False, id="1024-lock"), pytest.param(1024, True, True, id="1024-lock-tr"),
          pytest.param(2048, False, True, id="2048-tr"), pytest.param(4096, False, True, id="4096-tr")]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pv_ref.build(str(tmp_path_factory.mktemp("ref_pv")))


def block(c, nae, x, ch, rate, pitch, n_fft, lock=False, transients=False, link=True, lifter=0, formant_ratio=None, n_streams=1):
    L = x.size // (ch * n_streams)
    pl = c.stretch_plan(rate, pitch, L, n_fft, formant=lifter, formant_ratio=formant_ratio) if formant_ratio is not None \
        else c.stretch_plan(rate, pitch, L, n_fft)
    d_x, d_o = c.array(x), c.empty(max(1, n_streams * pl.out_len * ch))
    c.stretch_block(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, n_streams, nae.Sig.interleaved(d_o.ptr, pl.out_len, ch),
                    n_fft=n_fft, formant=lifter, transients=transients, phase_lock=lock, formant_ratio=formant_ratio, link_channels=link)
    out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    return out


def tile_phases(c, nae, x, ch, rate, pitch, n_fft, lock=False, transients=False, link=True):
    L = x.size // ch
    d_x = c.array(x)
    got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, 1, phase_lock=lock, n_fft=n_fft,
                                   transients=transients, link_channels=link)
    d_x.free()
    return got, t


def check_tiles(got, tile, qs, ch):
    bins = qs.shape[2]
    for j in range(got.shape[2]):
        for c2 in range(ch):
            want = qs[j * tile - 1, c2] if j > 0 else np.zeros(bins, np.int32)
            assert np.array_equal(got[0, c2, j], want), (tile, j, c2, int(np.count_nonzero(got[0, c2, j] != want)))


@pytest.mark.parametrize("rate,pitch", PAIRS)
@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_integer_phases_bit_exact(nae, ref, n_fft, lock, tr, rate, pitch):
    """Qs in front of every tile equals the linked statement's phase of the frame before it, bit for bit, with tiles of 1, 3, 16 and 64
    frames; the linked phases are not the unlinked statement's"""
    L = 60000 * n_fft // 1024
    x = scene(L)
    qs = pv_ref.synth_phase(ref, x, 2, rate, pitch, n_fft, lock, tr, link=True)
    assert not np.array_equal(qs, pv_ref.synth_phase(ref, x, 2, rate, pitch, n_fft, lock, tr, link=False))
    for tile in (1, 3, 16, 64):
        with nae.Context(0) as c:
            c.debug_set("pv_tile", tile)
            got, t = tile_phases(c, nae, x, 2, rate, pitch, n_fft, lock, tr)
        assert t == tile
        check_tiles(got, tile, qs, 2)


@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_long_stream_every_tiling_gives_the_same_bits(nae, ref, n_fft, lock, tr):
    """a lone stereo stream of more than 256 16-frame tiles (the chunked scans): its phases at pv_tile 16 are the statement's, the linked
    kernels ran, and pv_tile 16, 64, one tile and the library's choice give the same samples bit for bit"""
    ch, rate, pitch = 2, 1.5, 1 / 1.5
    L = int(16 * 270 * (n_fft // 4) * 1.5)
    x = scene(L, seed=11, n_hits=60)
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    assert (pl.frames + 15) // 16 >= 256
    qs = pv_ref.synth_phase(ref, x, ch, rate, pitch, n_fft, lock, tr, link=True)
    with nae.Context(0) as c:
        c.debug_set("pv_tile", 16)
        (got, t), launched = profiled(c, tile_phases, c, nae, x, ch, rate, pitch, n_fft, lock, tr)
    if lock:
        want = {"pvlock_map_transient_link_kernel" if tr else "pvlock_map_link_kernel"}
    else:
        want = {"pv_any_phase_link_kernel", "pv_any_scan_chunked_transient_kernel"}
    assert want <= launched, launched
    check_tiles(got, 16, qs, ch)
    outs = {}
    for key, knobs in (("one tile", {"pv_tile": 1000000}), ("16", {"pv_tile": 16}), ("64", {"pv_tile": 64}), ("library", {})):
        with nae.Context(0) as c:
            for k, v in knobs.items():
                c.debug_set(k, v)
            outs[key] = block(c, nae, x, ch, rate, pitch, n_fft, lock, tr)
    for key in outs:
        assert same_bits(outs[key], outs["one tile"]), key


@pytest.mark.parametrize("stage", ["plain", "lifter", "shift-A", "shift-B"])
@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_samples_vs_statement(ctx, nae, ref, n_fft, lock, tr, stage):
    """within 1e-4 relative RMS of the linked CPU statement: without a lifter, with the default lifter (_formant), and with _formant_shift in case
    A (a pitch change) and case B (a tempo change only).  Measured values: DESIGN.md §3, "Channel link"."""
    x = scene(40000, seed=5)
    q = 0 if stage == "plain" else pv_ref.default_lifter(48000, n_fft)
    phi = 1.2 if stage.startswith("shift") else None
    pairs = [(1.5, 1 / 1.5)] if stage == "shift-B" else [(1.0, 2 ** (3 / 12)), (1.0, 2 ** (-7 / 12))] + ([(1.5, 1 / 1.5)] if stage == "plain" else [])
    for rate, pitch in pairs:
        got, launched = profiled(ctx, block, ctx, nae, x, 2, rate, pitch, n_fft, lock, tr, True, q, phi)
        want = pv_ref.stretch(ref, x, 2, rate, pitch, n_fft, lock, q, tr, link=True, formant_ratio=phi)
        unlinked = pv_ref.stretch(ref, x, 2, rate, pitch, n_fft, lock, q, tr, link=False, formant_ratio=phi)
        assert got.size == want.size and np.isfinite(got).all()
        e = rel_rms(got, want)
        print(f"N={n_fft} lock={lock} tr={tr} {stage} rel RMS {rate:.4f}/{pitch:.4f}: {e:.3g} (to the unlinked statement {rel_rms(got, unlinked):.3g})")
        assert e <= TOL, e
        assert rel_rms(want, unlinked) > 10 * TOL                 # on this input the linked statement is not the unlinked one
        synth = "pvlock_synth" if lock else "pv_any_synth"
        assert any(k.startswith(synth) and k.endswith("link_kernel") for k in launched), launched


@pytest.mark.parametrize("entry", ["n", "formant"])
@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_stream_handle_equals_block(ctx, nae, n_fft, lock, tr, entry):
    """irregular put sizes — seeded random cuts, 1152-frame puts, one frame short of and past a hop — flush included, equal the block call
    bit for bit (the _formant entry with its default lifter), in both stage orders and without the transposer"""
    L, ch = 100000, 2
    x = scene(L, seed=17)
    q = pv_ref.default_lifter(48000, n_fft) if entry == "formant" else 0
    flags = LINK | (TR if tr else 0) | (LOCK if lock else 0)
    rng = np.random.default_rng(n_fft)
    for rate, pitch in [(1.0, float(np.float32(2 ** (-7 / 12)))), (1.5, float(np.float32(1 / 1.5))), (1.0, float(np.float32(2 ** (3 / 12))))]:
        blk = block(ctx, nae, x, ch, rate, pitch, n_fft, lock, tr, True, q)
        assert not same_bits(blk, block(ctx, nae, x, ch, rate, pitch, n_fft, lock, tr, False, q))
        for puts in ([int(v) for v in rng.integers(1, 30000, 40)], [1152], [n_fft // 4 - 1, n_fft // 4 + 1, 7, 20011]):
            y = stream(ctx, x, ch, rate, pitch, puts, entry, n_fft, flags=flags, lifter=q)
            assert y.size == blk.size
            assert same_bits(y, blk), (rate, puts[:4])


@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_batch_streams_equal_their_lone_runs(ctx, nae, n_fft, lock, tr):
    """a batch of five different stereo streams: each stream's output is its lone run's, bit for bit"""
    L, ch, n = 30000 * n_fft // 1024, 2, 5
    xs = [scene(L, seed=30 + i) for i in range(n)]
    rate, pitch = 1.0, 2 ** (-7 / 12)
    got = block(ctx, nae, np.concatenate(xs), ch, rate, pitch, n_fft, lock, tr, n_streams=n).reshape(n, -1)
    for i in range(n):
        assert same_bits(np.ascontiguousarray(got[i]), block(ctx, nae, xs[i], ch, rate, pitch, n_fft, lock, tr)), i


def test_where_the_link_is_not_effective_the_flag_changes_nothing(ctx, nae):
    """mono, neither option, the forced plan (formant shift cases C and D) and no vocoder stage: the bits of the same call without the flag;
    and the routes of those calls are the unflagged ones (no *_link_kernel)"""
    x = scene(30000, seed=7)
    mono = np.ascontiguousarray(x[0::2])
    cases = []
    for n_fft in SIZES:
        q = pv_ref.default_lifter(48000, n_fft)
        cases += [
            dict(x=mono, ch=1, rate=1.5, pitch=1 / 1.5, n_fft=n_fft, transients=True),                     # mono
            dict(x=x, ch=2, rate=1.5, pitch=1 / 1.5, n_fft=n_fft),                                         # neither option
            dict(x=x, ch=2, rate=1.0, pitch=2 ** (3 / 12), n_fft=n_fft, lifter=q),
            dict(x=x, ch=2, rate=1.25, pitch=1.0, n_fft=n_fft, lifter=q, transients=True, formant_ratio=1.2),   # forced: case C
            dict(x=x, ch=2, rate=0.8, pitch=1.0, n_fft=n_fft, lifter=q, transients=True, formant_ratio=1.2),
            dict(x=x, ch=2, rate=1.0, pitch=1.0, n_fft=n_fft, lifter=q, transients=True, formant_ratio=1.2),    # forced: case D
            dict(x=x, ch=2, rate=2.0, pitch=1.0, n_fft=n_fft, transients=True),                            # no vocoder stage
            dict(x=x, ch=2, rate=1.0, pitch=1.0, n_fft=n_fft, transients=True),                            # a wire
        ]
    q = pv_ref.default_lifter(48000, 1024)
    cases += [dict(x=mono, ch=1, rate=1.5, pitch=1 / 1.5, n_fft=1024, lock=True, transients=True),
              dict(x=mono, ch=1, rate=1.5, pitch=1 / 1.5, n_fft=1024, lock=True),
              dict(x=x, ch=2, rate=1.25, pitch=1.0, n_fft=1024, lifter=q, lock=True, transients=True, formant_ratio=1.2),
              dict(x=x, ch=2, rate=1.0, pitch=1.0, n_fft=1024, lifter=q, lock=True, formant_ratio=1.2),
              dict(x=x, ch=2, rate=2.0, pitch=1.0, n_fft=1024, lock=True)]
    for kw in cases:
        kw = dict(kw)
        sig, ch, rate, pitch, n_fft = kw.pop("x"), kw.pop("ch"), kw.pop("rate"), kw.pop("pitch"), kw.pop("n_fft")
        on, launched = profiled(ctx, block, ctx, nae, sig, ch, rate, pitch, n_fft, link=True, **kw)
        off = block(ctx, nae, sig, ch, rate, pitch, n_fft, link=False, **kw)
        assert same_bits(on, off), (n_fft, ch, rate, kw)
        assert not any("link" in k for k in launched), launched


def test_error_codes(ctx, nae):
    """_n / _formant / _formant_shift accept 16, 16 | 4 at every size and 16 | 1, 16 | 4 | 1 at 1024; with the lock at another size
    NAE_ERR_UNSUPPORTED; 2, 8 and 16 | 2, 16 | 8 are NAE_ERR_INVALID; the _ex entries reject 16 with NAE_ERR_INVALID"""
    lib = ctx.lib
    L, ch = 4096, 2
    d_x, d_o = ctx.empty(L * ch), ctx.empty(2 * L * ch)
    src, dst = nae.Sig.interleaved(d_x.ptr, L, ch), nae.Sig.interleaved(d_o.ptr, 2 * L, ch)
    h = C.c_void_p()
    nt, tf = C.c_size_t(), C.c_size_t()
    buf = np.zeros(64 * 2049 * ch, np.int32)
    phi = C.c_double(1.2)

    def all7(flags, n_fft):
        rc = [lib.nae_stretch_block_n_f32(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, C.byref(dst)),
              lib.nae_stretch_create_n(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, C.byref(h))]
        if rc[1] == 0:
            assert lib.nae_stretch_destroy(h) == 0
        rc.append(lib.nae_debug_pv_tile_phase_n(ctx.h, 1.0, 1.2, flags, n_fft, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size,
                                                C.byref(nt), C.byref(tf)))
        rc.append(lib.nae_stretch_block_formant_f32(ctx.h, 1.0, 1.2, flags, n_fft, 8, C.byref(src), L, ch, 1, C.byref(dst)))
        rc.append(lib.nae_stretch_create_formant(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, 8, C.byref(h)))
        if rc[4] == 0:
            assert lib.nae_stretch_destroy(h) == 0
        rc.append(lib.nae_stretch_block_formant_shift_f32(ctx.h, 1.0, 1.2, flags, n_fft, 8, phi, C.byref(src), L, ch, 1, C.byref(dst)))
        rc.append(lib.nae_stretch_create_formant_shift(ctx.h, 48000, ch, 1.0, 1.2, flags, n_fft, 8, phi, C.byref(h)))
        if rc[6] == 0:
            assert lib.nae_stretch_destroy(h) == 0
        return tuple(rc)

    for n_fft in SIZES:
        assert all7(LINK, n_fft) == (0,) * 7, n_fft
        assert all7(LINK | TR, n_fft) == (0,) * 7, n_fft
        for f in (LINK | LOCK, LINK | TR | LOCK):
            assert all7(f, n_fft) == ((0,) * 7 if n_fft == 1024 else (-2,) * 7), (n_fft, f)     # else NAE_ERR_UNSUPPORTED
        for f in (2, 8, LINK | 2, LINK | 8, 32):
            assert all7(f, n_fft) == (-1,) * 7, (n_fft, f)                                       # NAE_ERR_INVALID
    for f in (LINK, LINK | LOCK):
        assert lib.nae_stretch_block_ex_f32(ctx.h, 1.0, 1.2, f, C.byref(src), L, ch, 1, C.byref(dst)) == -1
        assert lib.nae_stretch_create_ex(ctx.h, 48000, ch, 1.0, 1.2, f, C.byref(h)) == -1
        assert lib.nae_debug_pv_tile_phase_ex(ctx.h, 1.0, 1.2, f, C.byref(src), L, ch, 1, buf.ctypes.data, buf.size, C.byref(nt), C.byref(tf)) == -1
    d_x.free(); d_o.free()


@pytest.mark.parametrize("n_fft,lock,tr", ROUTES)
def test_nan_in_one_channel(nae, ref, n_fft, lock, tr):
    """a NaN sample in channel 1: Pl is NaN in the frames that hold it and compares false in both channels' waves; the integer phases are
    defined and equal the statement's at every tile"""
    L = 40000 * n_fft // 1024
    x = scene(L, seed=9).copy()
    x[2 * (L // 2) + 1] = np.nan
    qs = pv_ref.synth_phase(ref, x, 2, 1.5, 1 / 1.5, n_fft, lock, tr, link=True)
    for tile in (3, 16):
        with nae.Context(0) as c:
            c.debug_set("pv_tile", tile)
            got, t = tile_phases(c, nae, x, 2, 1.5, 1 / 1.5, n_fft, lock, tr)
        check_tiles(got, tile, qs, 2)


def test_host_graph_pitch_node_link_channels(tmp_path):
    """source -> Pitch_modifier {"pitch": 3, "fft_size": 2048, "transients": true, "link_channels": true} -> sink through the fiber runner
    equals the linked block call bit for bit and differs from the unlinked one; the same with {"pitch": 3, "phase_lock": true,
    "link_channels": true} at 1024"""
    exe = node_harness.build("pv_ref/host_pv_node.cpp", str(tmp_path))
    for mode in (["gpu", "link_channels"], ["gpu", "link_channels", "lock"]):
        r = subprocess.run([exe, *mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "HOST PV NODE OK " + " ".join(mode) in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
