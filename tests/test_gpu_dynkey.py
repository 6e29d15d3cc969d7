"""K15 keyed dynamics on the GPU, bit for bit against the CPU statement (tests/dynkey_ref/ref_dynkey.c): every length around the lane, the wave
and the chunk at every look-ahead, section count and pairing of signal and key channels; every view of the signal with the key interleaved,
planar and shared; the identities with nae_dyn_block_f32 and nae_eq_block_f32 through public entries only; the key filter's carry across
chunks and launches; the streaming handle; non-finite, zero and subnormal keys; two contexts from two threads; the error codes; the host
node (tests/dynkey_ref/host_dynkey_node.cpp)."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

import dyn_ref
import dynkey_ref
import eq_gpu
import node_harness
from block_gpu import CONFIGS, bits, noise, statement
from dyn_gpu import gpu_dyn
from dynkey_gpu import dynkey_stream, gpu_dynkey, lib_params

pytestmark = pytest.mark.gpu

T, CH = dyn_ref.LANE, dyn_ref.CHUNK
INVALID, UNSUPPORTED = -1, -2
MID = dict(alpha_attack=dyn_ref.alpha(0.002), alpha_release=dyn_ref.alpha(0.05))
FILTERS = dynkey_ref.key_filters()
# (ch, key_ch, link): internal and external keys, mono and stereo, linked and not
PAIRINGS = ((1, 0, 0), (1, 1, 0), (2, 0, 1), (2, 1, 1), (2, 2, 1), (2, 2, 0), (2, 1, 0))


@pytest.fixture(scope="module")
def ref():
    return statement(dynkey_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("dynkey_ref/host_dynkey_node.cpp", str(tmp_path_factory.mktemp("host_dynkey_gpu")))


def loud(rng, n_streams, n, ch):
    """noise whose level wanders from far under to far over the -18 dB threshold, another phase per stream and channel: a key"""
    if ch == 0:
        return None
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    return (rng.uniform(-1, 1, (n_streams, n, ch)) * 10.0 ** ((-18.0 + 14.0 * np.sin(2 * np.pi * t / 411.0 + ph)) / 20.0)).astype(np.float32)


def differs(got, want):
    return int(np.sum(bits(got) != bits(want)))


@pytest.mark.parametrize("la", (0, 15, 16, 17, 1024))
def test_lengths_lookaheads_sections_and_pairings(nae, ctx, ref, la):
    rng = np.random.default_rng(500 + la)
    for in_len in (1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH - 1 + la, 3 * CH + 7):
        for sections in (0, 1, 4):
            for ch, key_ch, link in PAIRINGS:
                p = dynkey_ref.params(dyn_ref.params(lookahead=la, link=link, **MID), key_ch, FILTERS[sections])
                # an internal key is the signal: it gets the key's wandering level
                x, key = (loud(rng, 2, in_len, ch), None) if key_ch == 0 else (noise(rng, 2, in_len, ch), loud(rng, 2, in_len, key_ch))
                want = dynkey_ref.run_streams(ref, p, x, key)
                got = gpu_dynkey(nae, ctx, p, x, key)
                assert np.array_equal(bits(got), bits(want)), (in_len, la, sections, ch, key_ch, link, differs(got, want))


@pytest.mark.parametrize("key_layout", ("i", "p", "s"))
def test_views(nae, ctx, ref, key_layout):
    """block_gpu.CONFIGS on the signal; the key interleaved, planar and with stream_stride = 0: one key for three different signals.  NaN
    stands outside the key's samples and outside the signal's, and the guard words around the destination stay intact (view_call)"""
    rng = np.random.default_rng(ord(key_layout))
    in_len = CH + 3 * T + 5
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        for key_ch in sorted({1, ch}):
            for link in (0, 1):
                p = dynkey_ref.params(dyn_ref.params(lookahead=(0, 17, 200)[i % 3], link=link, **MID), key_ch, FILTERS[(1, 4, 0)[i % 3]])
                x = noise(rng, n_streams, in_len, ch, shared)
                key = loud(rng, n_streams, in_len, key_ch)
                if key_layout == "s":
                    key = key[:1]
                want = dynkey_ref.run_streams(ref, p, x, key)
                got = gpu_dynkey(nae, ctx, p, x, np.broadcast_to(key, (n_streams,) + key.shape[1:]), sl, dl, shared, key_layout=key_layout,
                                 gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
                assert np.array_equal(bits(got), bits(want)), (ch, n_streams, sl, dl, shared, key_ch, link, differs(got, want))
                if key_layout == "s" and n_streams > 1 and not shared:
                    assert not np.array_equal(bits(got[0]), bits(got[1])), "three different signals under one key"


@pytest.mark.parametrize("ch,link", ((1, 0), (2, 1), (2, 0)))
def test_identities_through_public_entries(nae, ctx, ch, link):
    """an internal key and a key equal to the signal, with no section, are nae_dyn_block_f32; a key filtered by n sections is the call with no
    section keyed by nae_eq_block_f32's output of that key"""
    rng = np.random.default_rng(70 + ch + link)
    in_len = 2 * CH + 77
    dp = dyn_ref.params(lookahead=33, link=link, **MID)
    x = loud(rng, 2, in_len, ch)
    plain = gpu_dyn(nae, ctx, dp, x)
    assert np.array_equal(bits(gpu_dynkey(nae, ctx, dynkey_ref.params(dp, 0), x)), bits(plain)), "internal key"
    assert np.array_equal(bits(gpu_dynkey(nae, ctx, dynkey_ref.params(dp, ch), x, x)), bits(plain)), "the signal as an external key"
    for key_ch in sorted({1, ch}):
        key = loud(rng, 2, in_len, key_ch)
        for sections in (1, 4):
            filtered = eq_gpu.gpu_eq(nae, ctx, FILTERS[sections], key)
            got = gpu_dynkey(nae, ctx, dynkey_ref.params(dp, key_ch, FILTERS[sections]), noise(np.random.default_rng(5), 2, in_len, ch), key)
            want = gpu_dynkey(nae, ctx, dynkey_ref.params(dp, key_ch), noise(np.random.default_rng(5), 2, in_len, ch), filtered)
            assert np.array_equal(bits(got), bits(want)), (key_ch, sections, differs(got, want))
            assert not np.array_equal(bits(filtered), bits(key)), "the filter changes the key: the case tests it"


def test_carry_across_chunks(nae, ctx, ref):
    """a 40-chunk stereo launch with four slow sections and the longest look-ahead: the filter's carry and the detector's cross 39 chunk edges"""
    rng = np.random.default_rng(40)
    in_len = 40 * CH - 9
    for key_ch, link in ((2, 1), (0, 0)):
        p = dynkey_ref.params(dyn_ref.params(lookahead=1024, link=link, **dyn_ref.SLOW), key_ch, FILTERS[4])
        x, key = (loud(rng, 1, in_len, 2), None) if key_ch == 0 else (noise(rng, 1, in_len, 2), loud(rng, 1, in_len, key_ch))
        got, want = gpu_dynkey(nae, ctx, p, x, key, "p", "i", chan_pad=3), dynkey_ref.run_streams(ref, p, x, key)
        assert np.array_equal(bits(got), bits(want)), (key_ch, link, differs(got, want))


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("put", (1, 7, 1000, 1024, 1025, 5000))
def test_handle_equals_the_block_call(nae, ctx, ref, put, la):
    """any cut of the frames of ch + key_ch floats into puts gives the block call's bits, with four slow sections whose carry every launch hands
    on from in front of the chunk it levelled last; `available` follows floor((put - la) / 1024) chunks after every put (dynkey_stream)"""
    in_len = {1: 700, 7: 1500, 5000: 2 * 5000 + CH + 300}.get(put, 3 * CH + 7)
    ch, key_ch, link = {1: (2, 1, 1), 7: (1, 1, 0), 1000: (2, 2, 0), 1024: (1, 0, 0), 1025: (2, 2, 1), 5000: (2, 0, 1)}[put]
    p = dynkey_ref.params(dyn_ref.params(lookahead=la, link=link, **MID), key_ch, FILTERS[4])
    rng = np.random.default_rng(put + la)
    x, key = (loud(rng, 1, in_len, ch), None) if key_ch == 0 else (noise(rng, 1, in_len, ch), loud(rng, 1, in_len, key_ch))
    want = dynkey_ref.run_streams(ref, p, x, key)[0]
    for device in (False, True):
        got = dynkey_stream(nae, ctx, p, x[0], None if key is None else key[0], (put,), device=device)
        assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(want)), (device, differs(got, want))


@pytest.mark.parametrize("defer", (False, True))
def test_handle_random_puts(nae, ctx, ref, defer):
    """a seeded random mix of puts from the device and the host in turn, received after each put and only after the flush"""
    rng = np.random.default_rng(77)
    in_len = 12 * CH + 300
    puts = tuple(int(k) for k in rng.integers(1, 3001, 32))
    for ch, key_ch, link, sections in ((2, 2, 1, 4), (2, 1, 0, 1), (1, 1, 0, 0)):
        p = dynkey_ref.params(dyn_ref.params(lookahead=300, link=link, **dyn_ref.SLOW), key_ch, FILTERS[sections])
        x, key = noise(rng, 1, in_len, ch)[0], loud(rng, 1, in_len, key_ch)[0]
        got = dynkey_stream(nae, ctx, p, x, key, puts, device=(True, False), defer=defer)
        want = dynkey_ref.run(ref, p, x, key)
        assert np.array_equal(bits(got), bits(want)), (ch, key_ch, link, sections, differs(got, want))


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_samples(nae, ctx, bad, la):
    """a non-finite key sample at 2 C + 5 leaves every output sample before it by more than the look-ahead as it was, and the other stream
    untouched; with an external key a non-finite signal sample changes its own output sample only"""
    i = 2 * CH + 5
    rng = np.random.default_rng(9)
    x, key = noise(rng, 2, 3 * CH + 40, 2), loud(rng, 2, 3 * CH + 40, 2)
    for sections in (0, 1):
        p = dynkey_ref.params(dyn_ref.params(lookahead=la, link=1, **MID), 2, FILTERS[sections])
        clean = gpu_dynkey(nae, ctx, p, x, key, "p", "p", chan_pad=3)
        dirty_key = key.copy()
        dirty_key[0, i, 1] = bad
        got = gpu_dynkey(nae, ctx, p, x, dirty_key, "p", "p", chan_pad=3)
        assert np.array_equal(bits(got[:, :i - la]), bits(clean[:, :i - la])), "samples before i - la changed"
        assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"
        dirty_x = x.copy()
        dirty_x[0, i, 1] = bad
        got = gpu_dynkey(nae, ctx, p, dirty_x, key, "p", "p", chan_pad=3)
        same = np.ones(x.shape, bool)
        same[0, i, 1] = False
        assert np.array_equal(bits(got)[same], bits(clean)[same]), "a non-finite signal sample reached another output sample"
        assert not np.isfinite(got[0, i, 1])


def test_zero_and_subnormal_key(nae, ctx, ref):
    """a zero key: the signal under the make-up gain alone; an f32 subnormal key through a section: the statement's bits"""
    rng = np.random.default_rng(11)
    n = CH + 70
    x = noise(rng, 2, n, 2)
    for sections in (0, 1):
        p = dynkey_ref.params(dyn_ref.params(lookahead=40, link=1, makeup_db=6.0, **MID), 2, FILTERS[sections])
        z = np.zeros((2, n, 2), np.float32)
        got = gpu_dynkey(nae, ctx, p, x, z)
        assert np.array_equal(bits(got), bits(dynkey_ref.run_streams(ref, p, x, z)))
        assert np.allclose(got, x * 10.0 ** (6.0 / 20.0), rtol=1e-6, atol=0)
        key = (rng.integers(-(1 << 22), 1 << 22, (2, n, 2)).astype(np.int32) & np.int32(-0x7f800001)).view(np.float32)
        key = np.ascontiguousarray(key)
        key[:, ::5] = 0.0
        assert np.all(np.abs(key) < np.finfo(np.float32).tiny)
        got = gpu_dynkey(nae, ctx, p, x, key)
        assert not np.any(np.isnan(got)) and np.array_equal(bits(got), bits(dynkey_ref.run_streams(ref, p, x, key)))


def test_two_contexts_from_two_threads(nae, ref):
    """each thread creates, drives and destroys a context of its own, with its own parameters and key filter, at once"""
    rng = np.random.default_rng(61)
    x, key = noise(rng, 3, 2 * CH + 3, 2), loud(rng, 3, 2 * CH + 3, 2)
    ps = [dynkey_ref.params(dyn_ref.params(lookahead=33, link=1, **MID), 2, FILTERS[4]),
          dynkey_ref.params(dyn_ref.params(lookahead=500, link=0, knee_db=0.0, slope=1.0, **dyn_ref.FAST), 2, FILTERS[1])]
    out, errors = {}, []

    def worker(k):
        try:
            c = nae.Context(0)
            try:
                for _ in range(3):
                    out[k] = gpu_dynkey(nae, c, ps[k], x, key)
                    out[k + 2] = dynkey_stream(nae, c, ps[k], x[0], key[0], (777,))
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
        want = dynkey_ref.run_streams(ref, ps[k], x, key)
        assert np.array_equal(bits(out[k]), bits(want)) and np.array_equal(bits(out[k + 2]), bits(want[0])), k


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(128, np.float32))
    sig, ksig = nae.Sig(d.ptr, 32, 1, 1), nae.Sig(d.at(64), 32, 1, 1)
    hp = FILTERS[1]

    def block(p, ch=1, key="by key_ch", n=16, streams=1):
        k = (C.byref(ksig) if p.key_ch else None) if key == "by key_ch" else key
        return lib.nae_dynkey_block_f32(ctx.h, C.byref(lib_params(nae, p)), C.byref(sig), k, n, ch, streams, C.byref(sig))

    def create(p, ch=1):
        """the create entry's code; a failure hands no handle out"""
        h = C.c_void_p()
        rc = lib.nae_dynkey_create(ctx.h, C.byref(p if isinstance(p, nae.DynKeyParams) else lib_params(nae, p)), ch, C.byref(h))
        assert bool(h.value) == (rc == 0)
        if not rc:
            lib.nae_dynkey_destroy(h)
        return rc

    good = dynkey_ref.params(dyn_ref.params(), 1, hp)
    assert block(good) == 0 and create(good) == 0
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    # K12's rules, through the one check
    assert block(dynkey_ref.params(dyn_ref.params(slope=1.5), 1, hp)) == INVALID and block(good, ch=3) == INVALID
    assert block(dynkey_ref.params(dyn_ref.params(lookahead=1025), 1, hp)) == UNSUPPORTED
    assert create(dynkey_ref.params(dyn_ref.params(lookahead=1025), 1, hp)) == UNSUPPORTED
    # the key
    for key_ch, ch in ((2, 1), (3, 2), (-1, 1)):
        bad = dynkey_ref.params(dyn_ref.params(), key_ch, hp)
        assert block(bad, ch=ch, key=C.byref(ksig)) == INVALID and block(bad, ch=ch, key=C.byref(ksig), n=0) == INVALID, (key_ch, ch)
        assert create(bad, ch) == INVALID
    assert block(good, key=None) == INVALID, "no key view with key_ch > 0"
    assert block(dynkey_ref.params(dyn_ref.params(), 0, hp), key=C.byref(ksig)) == INVALID, "a key view with key_ch = 0"
    assert block(dynkey_ref.params(dyn_ref.params(), 0, hp)) == 0
    # the sections
    raw = lib_params(nae, good)
    for n_sections, code in ((-1, INVALID), (5, UNSUPPORTED), (0, 0), (4, 0)):
        raw.n_sections = n_sections
        for s in range(4):
            for i_, v in enumerate(hp[0]):
                raw.coef[s][i_] = v
        assert lib.nae_dynkey_block_f32(ctx.h, C.byref(raw), C.byref(sig), C.byref(ksig), 16, 1, 1, C.byref(sig)) == code, n_sections
        assert create(raw) == code
    for section in ((1, 0, 0, 0, 1.0), (1, 0, 0, 1.5, 0.5), (float("nan"), 0, 0, 0, 0), (1, 0, 0, float("inf"), 0)):
        bad = dynkey_ref.params(dyn_ref.params(), 1, np.array([hp[0], section]))
        assert block(bad) == INVALID and create(bad) == INVALID, section
    assert lib.nae_dynkey_block_f32(ctx.h, None, C.byref(sig), None, 16, 1, 1, C.byref(sig)) == INVALID
    h = C.c_void_p()
    assert lib.nae_dynkey_create(ctx.h, None, 1, C.byref(h)) == INVALID and lib.nae_dynkey_create(ctx.h, C.byref(raw), 1, None) == INVALID
    ctx.sync()
    d.free()


def test_host_node_graph(host):
    """two sources -> audio_sidechain -> sink: the key 100 samples late, 37 samples early, ending before the input, and not linked; each
    delivers the input's frames, sizes and pts and the block call's samples on the arrays lined up by o = llround((t_key - t_input) rate)"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYNKEY OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_errors(host):
    """a key of another sample rate, a key with more channels than the input, a look-ahead over 1024 samples and a key filter band above
    Nyquist are Runtime_errors on the first frames"""
    r = subprocess.run([host, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST DYNKEY OK errors" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
