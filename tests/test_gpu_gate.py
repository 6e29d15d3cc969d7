"""K19 gate on the GPU, bit for bit against the CPU statement (tests/gate_ref/ref_gate.c): every length around the lane and the chunk at every
look-ahead and hold, both modes, linked and unlinked detectors, every view, signals built to hit the edges of the hysteresis, the hold and
the look-ahead, silence and full scale, the streaming handle, two batches that fill the chip and more, a launch of 300 chunks, non-finite
input, the error codes, the host node (tests/gate_ref/host_gate_node.cpp) and a seeded run of tests/tools/fuzz_gate.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gate_ref
import node_harness
from block_gpu import CONFIGS, bits, each_stream, mismatch, statement
from gate_gpu import gate_stream, gpu_gate, lib_params

pytestmark = pytest.mark.gpu

T, CH = gate_ref.LANE, gate_ref.CHUNK
LENGTHS = (1, T - 1, T, T + 1, CH - 1, CH, CH + 1, 2 * CH, 3 * CH + 7)
LOOKAHEADS = (0, 1, 15, 16, 17, 1023, 1024)
HOLDS = (0, 1, 15, 16, 1024, 5000)
INVALID, UNSUPPORTED = -1, -2
MID = dict(alpha_attack=gate_ref.alpha(0.002), alpha_release=gate_ref.alpha(0.05))
OPEN, CLOSE = np.float32(0.1), np.float32(0.05)


@pytest.fixture(scope="module")
def ref():
    return statement(gate_ref)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return node_harness.build("gate_ref/host_gate_node.cpp", str(tmp_path_factory.mktemp("host_gate_gpu")))


def bursts(rng, n_streams, n, ch, shared=False, period=411, threshold_db=-30.0):
    """noise whose level wanders from far under to far over the threshold, another phase per stream and channel"""
    t = np.arange(n)[None, :, None]
    ph = rng.uniform(0, 2 * np.pi, (n_streams, 1, ch))
    x = (rng.uniform(-1, 1, (n_streams, n, ch)) * 10.0 ** ((threshold_db + 14.0 * np.sin(2 * np.pi * t / period + ph)) / 20.0)).astype(np.float32)
    if shared:
        x[:] = x[0]
    return x


def same(nae, ctx, ref, p, x, *views, **kw):
    got, want = gpu_gate(nae, ctx, p, x, *views, **kw), gate_ref.run_streams(ref, p, x)
    return mismatch(got, want)


@pytest.mark.parametrize("la", LOOKAHEADS)
def test_lengths_lookaheads_and_holds(nae, ctx, ref, la):
    """the lane edge and the chunk edge in the length, the look-ahead and the hold; both modes; linked stereo and mono"""
    rng = np.random.default_rng(100 + la)
    for k, in_len in enumerate(LENGTHS):
        for j, (link, ch) in enumerate(((1, 2), (0, 1))):
            hold = HOLDS[(k + j + la) % len(HOLDS)]
            for expand in (0, 1):
                p = gate_ref.params(lookahead=la, hold=hold, expand=expand, link=link, slope=1.5, **MID)
                message = same(nae, ctx, ref, p, bursts(rng, 2, in_len, ch, period=97 if in_len < 3 * CH else 1500))
                assert not message, (in_len, la, hold, expand, link, message)


@pytest.mark.parametrize("hold", HOLDS)
def test_holds_at_three_chunks(nae, ctx, ref, hold):
    """every hold at 3 C + 7 and at 6 C + 7 samples with sparse bursts: a hold of 5000 spans chunks that hold no set sample, so the last-set
    carry crosses them"""
    rng = np.random.default_rng(200 + hold)
    for n in (3 * CH + 7, 6 * CH + 7):
        x = (rng.uniform(-1, 1, (2, n, 2)) * 0.01).astype(np.float32)
        x[0, 100:130] = 0.5
        x[0, 5 * CH + 3 if n > 5 * CH + 3 else 2 * CH + 3] = 0.5
        x[1, CH - 1] = 0.5
        for la in (0, 17, 1024):
            for link in (0, 1):
                p = gate_ref.params(open_lin=OPEN, close_lin=CLOSE, lookahead=la, hold=hold, link=link, **MID)
                message = same(nae, ctx, ref, p, x)
                assert not message, (n, hold, la, link, message)


@pytest.mark.parametrize("expand", (0, 1))
def test_views_and_parameters(nae, ctx, ref, expand):
    """mono, stereo linked and unlinked; interleaved and planar on either side, stream_stride 0, odd offsets, gaps; 3 streams of distinct
    content; the guard words around the destination stand (view_call checks them)"""
    rng = np.random.default_rng(10 + expand)
    in_len = CH + 3 * T + 5
    speeds = (MID, gate_ref.FAST, gate_ref.SLOW)
    linked_differs = 0
    for i, (ch, n_streams, sl, dl, shared) in enumerate(CONFIGS):
        for link in (0, 1):
            kw = dict(lookahead=(0, 17, 200)[i % 3], hold=(0, 40, 300)[(i + link) % 3], expand=expand, slope=(0.5, 3.0)[i % 2], **speeds[i % 3])
            p = gate_ref.params(link=link, **kw)
            x = bursts(rng, n_streams, in_len, ch, shared)
            message = same(nae, ctx, ref, p, x, sl, dl, shared, gap=3 if sl == "p" else 0, chan_pad=5 if "p" in (sl, dl) else 0, offset=i % 2)
            assert not message, (ch, n_streams, sl, dl, shared, link, message)
            if link and ch == 2:
                linked_differs += not np.array_equal(bits(gate_ref.run_streams(ref, p, x)), bits(gate_ref.run_streams(ref, gate_ref.params(link=0, **kw), x)))
    assert linked_differs >= 3, "the link changes the result in most stereo views: the cases test it"


def test_in_place(nae, ctx, ref):
    """dst->base == src->base is allowed"""
    x = bursts(np.random.default_rng(5), 3, 2 * CH + 9, 2)
    for link, la in ((1, 0), (0, 300), (1, 1024)):
        p = gate_ref.params(lookahead=la, hold=20, link=link, expand=link, **MID)
        d = ctx.array(x.reshape(-1))
        sig = nae.Sig(d.ptr, x.shape[1] * 2, 1, 2)
        ctx.gate_block(lib_params(nae, p), sig, x.shape[1], 2, 3, sig)
        got = d.download().reshape(x.shape)
        d.free()
        message = mismatch(got, gate_ref.run_streams(ref, p, x))
        assert not message, (link, la, message)


def edge_signals():
    """[streams, n, 1] each, thresholds OPEN and CLOSE; n = 4 C + 7"""
    n = 4 * CH + 7
    rng = np.random.default_rng(7)
    band = lambda k: rng.uniform(float(CLOSE) * 1.01, float(OPEN) * 0.99, k).astype(np.float32)   # noqa: E731 — inside the hysteresis band: keeps
    low = lambda k: rng.uniform(0.0, float(CLOSE) * 0.99, k).astype(np.float32)                   # noqa: E731 — clears
    out = {}
    # magnitudes exactly at the thresholds: OPEN sets, CLOSE keeps, the next f32 under CLOSE clears
    x = np.tile(np.array([OPEN, CLOSE, np.nextafter(OPEN, np.float32(0)), CLOSE, np.nextafter(CLOSE, np.float32(0)), CLOSE, -OPEN, -CLOSE], np.float32), n // 8 + 1)[:n]
    out["exactly at the thresholds"] = x
    # a stretch inside the band that covers whole lanes and the whole of chunk 2, entered once open and once closed
    for name, first in (("band entered open", OPEN), ("band entered closed", np.float32(0.0))):
        x = low(n)
        x[CH - 40] = first
        x[CH - 39:3 * CH + 5] = band(2 * CH + 44)
        out[name] = x
    # a single set sample at the last and at the first sample of a chunk
    for name, at in (("set at a chunk's last sample", 2 * CH - 1), ("set at a chunk's first sample", 2 * CH), ("set at the first sample", 0),
                     ("set at the last sample", n - 1)):
        x = low(n)
        x[at] = 0.7
        out[name] = x
    # bursts whose gaps are hold - 1, hold and hold + 1 long, for the holds the test runs (gap: samples between two set samples, exclusive)
    for hold in (1, 16, 40, 1024):
        x = low(n)
        at = 5
        for gap in (hold - 1, hold, hold + 1, hold - 1, hold + 1, hold):
            if at < n:
                x[at] = 0.9
            at += gap + 1
        if at < n:
            x[at] = 0.9
        out[f"gaps around a hold of {hold}"] = x
    out["silence"] = np.zeros(n, np.float32)
    out["full scale"] = rng.choice(np.array([-1.0, 1.0], np.float32), n)
    return {k: v[None, :, None].copy() for k, v in out.items()}


@pytest.mark.parametrize("la", (0, 1, 17, 1024))
def test_edges_of_the_decisions(nae, ctx, ref, la):
    for name, x in edge_signals().items():
        holds = (int(name.rsplit(" ", 1)[1]),) if name.startswith("gaps") else (0, 16, 1500)
        for hold in holds:
            for expand in (0, 1):
                p = gate_ref.params(open_lin=OPEN, close_lin=CLOSE, threshold_db=-20.0, slope=2.0, lookahead=la, hold=hold, expand=expand, link=0, **MID)
                message = same(nae, ctx, ref, p, x)
                assert not message, (name, la, hold, expand, message)
                if name.startswith("gaps") and la == 0 and not expand:
                    o = gate_ref.full(ref, p, x[0], 1)["open"][:, 0]
                    assert 0 < o.sum() < len(o) and np.any(np.diff(o.astype(int)) == -1), "the gaps of hold + 1 close the gate, the others do not"


def test_wire_and_brick(nae, ctx, ref):
    """alpha_attack 0 and nothing under open_lin: the input's bits; both alphas 0, no hold, one threshold: x, or x times one constant"""
    rng = np.random.default_rng(3)
    n = 2 * CH + 7
    x = (rng.choice([-1.0, 1.0], (2, n, 2)) * rng.uniform(0.1, 1.0, (2, n, 2))).astype(np.float32)
    for expand in (0, 1):
        p = gate_ref.params(open_lin=0.1, close_lin=0.05, alpha_attack=0.0, alpha_release=gate_ref.alpha(0.1), expand=expand, hold=3, lookahead=7)
        assert np.array_equal(bits(gpu_gate(nae, ctx, p, x)), bits(x))
    x = rng.uniform(-1, 1, (2, n, 1)).astype(np.float32)
    p = gate_ref.params(open_lin=0.25, close_lin=0.25, range_db=37.0, alpha_attack=0.0, alpha_release=0.0)
    got = gpu_gate(nae, ctx, p, x)
    below = np.abs(x) < np.float32(0.25)
    g = gate_ref.full(ref, p, np.full((1, 1), 0.125, np.float32), 1)["yd"][0, 0] / 0.125
    assert np.array_equal(bits(got[~below]), bits(x[~below])) and np.array_equal(bits(got[below]), bits((x[below].astype(np.float64) * g).astype(np.float32)))


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("put", (1, 7, 1024, 1025, "random"))
def test_handle_equals_the_block_call(nae, ctx, ref, put, la):
    """any cut of the input into puts gives the block call's bits; `available` follows floor((put - la) / 1024) chunks after every put and
    the flush releases the rest; a put after the flush is NAE_ERR_STATE (gate_stream asserts all three)"""
    in_len = {1: 700, 7: 1500}.get(put, 3 * CH + 7)
    ch, link = (1, 0) if put in (7, 1024) else (2, 1 if put != 1025 else 0)
    puts = tuple(int(k) for k in np.random.default_rng(la).integers(1, 1500, 16)) if put == "random" else (put,)
    for expand, hold in ((0, 5000 if put == 1025 else 30), (1, 100)):
        p = gate_ref.params(lookahead=la, hold=hold, expand=expand, link=link, **MID)
        x = bursts(np.random.default_rng(la + in_len), 1, in_len, ch, period=1300)
        block = gpu_gate(nae, ctx, p, x)[0]
        assert np.array_equal(bits(block), bits(gate_ref.run(ref, p, x[0])))
        for device in (False, True):
            got = gate_stream(nae, ctx, p, x[0], puts, device=device)
            assert got.shape == (in_len, ch) and np.array_equal(bits(got), bits(block)), (device, expand)


def test_two_handles_on_one_context_and_on_two(nae, ctx, ref):
    """two handles fed in turn, on one context and on two: each gives its own block call's bits"""
    x = bursts(np.random.default_rng(21), 2, 3 * CH + 100, 2, period=900)
    ps = [gate_ref.params(lookahead=33, hold=200, link=1, **MID), gate_ref.params(lookahead=500, hold=7, link=0, expand=1, **gate_ref.FAST)]
    want = [gate_ref.run(ref, ps[k], x[k]) for k in range(2)]
    other = nae.Context(0)
    try:
        for ctxs in ((ctx, ctx), (ctx, other)):
            hs = [nae.Gate(ctxs[k], lib_params(nae, ps[k]), 2) for k in range(2)]
            parts = [[], []]
            try:
                for pos in range(0, x.shape[1], 777):
                    for k in range(2):
                        hs[k].put_host(x[k, pos:pos + 777].reshape(-1))
                        if hs[k].available():
                            parts[k].append(hs[k].receive_host())
                for k in range(2):
                    hs[k].flush()
                    parts[k].append(hs[k].receive_host())
            finally:
                for h in hs:
                    h.close()
            for k in range(2):
                got = np.concatenate(parts[k]).reshape(-1, 2)
                assert got.shape == want[k].shape and np.array_equal(bits(got), bits(want[k])), (k, ctxs[1] is other)
    finally:
        other.close()


@pytest.mark.parametrize("n_streams,n,link", ((1024, 3 * CH + 7, 1), (4099, 2 * CH + 7, 0)))
def test_batches(nae, ctx, ref, n_streams, n, link):
    """1024 linked stereo streams fill the chip; 4099 unlinked ones are 8198 waves, more than it holds, and a prime number of streams.  Stream s
    carries signal s mod 17 of 17 seeded signals; the statement runs on each and every stream is compared"""
    base = bursts(np.random.default_rng(90 + link), 17, n, 2, period=700)
    p = gate_ref.params(lookahead=96, hold=150, link=link, expand=1 - link, **MID)
    want17 = each_stream(lambda i: gate_ref.run(ref, p, base[i]), 17)
    pick = np.arange(n_streams) % 17
    message = mismatch(gpu_gate(nae, ctx, p, base[pick]), want17[pick])
    assert not message, message


@pytest.mark.parametrize("expand", (0, 1))
def test_long_launch(nae, ctx, ref, expand):
    """one stereo stream of 300 C + 7 samples, the slowest attack and release and a hold of 5000: one wave walks 301 chunks, and the smoothed
    depth it carries from chunk to chunk has a memory of hundreds of them"""
    p = gate_ref.params(lookahead=1024 * expand, hold=5000, link=1, expand=expand, **gate_ref.SLOW)
    x = bursts(np.random.default_rng(300 + expand), 1, 300 * CH + 7, 2, period=40000)
    message = same(nae, ctx, ref, p, x, "p", "i", chan_pad=3)
    assert not message, message
    o = gate_ref.full(ref, p, x[0], 1)["open"]
    assert 0.1 < o.mean() < 0.9, "the gate opens and closes"


@pytest.mark.parametrize("la", (0, 17, 1024))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_non_finite_input_does_not_reach_back(nae, ctx, ref, bad, la):
    """a non-finite sample at 2 C + 5: every sample before it by more than the look-ahead has the clean run's bits, the other stream is
    untouched, the call returns NAE_OK and the sentinels around the destination stand; the finite samples have the statement's bits"""
    i = 2 * CH + 5
    x = bursts(np.random.default_rng(9), 2, 3 * CH + 40, 2)
    dirty_x = x.copy()
    dirty_x[0, i, 0] = bad
    for expand in (0, 1):
        p = gate_ref.params(lookahead=la, hold=25, link=1, expand=expand, **MID)
        clean = gpu_gate(nae, ctx, p, x, "p", "p", chan_pad=3)
        got = gpu_gate(nae, ctx, p, dirty_x, "p", "p", chan_pad=3)
        assert np.array_equal(bits(got[:, :i - la]), bits(clean[:, :i - la])), "samples before i - la changed"
        assert np.array_equal(bits(got[1]), bits(clean[1])), "another stream changed"
        want = gate_ref.run_streams(ref, p, dirty_x)
        finite = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), finite) and np.array_equal(bits(got[finite]), bits(want[finite]))
        assert finite.sum() >= want.size - 1, "only the sample itself is not finite"


def test_errors(nae, ctx):
    lib = ctx.lib
    d = ctx.array(np.zeros(64, np.float32))
    sig = nae.Sig(d.ptr, 32, 1, 1)
    good = gate_ref.params()

    def block(p, ch=1, src=C.byref(sig), dst=C.byref(sig), n=16, streams=1):
        return lib.nae_gate_block_f32(ctx.h, C.byref(lib_params(nae, p)) if p is not None else None, src, n, ch, streams, dst)

    assert block(good) == 0
    assert block(None) == INVALID and block(good, src=None) == INVALID and block(good, dst=None) == INVALID
    assert block(good, ch=0) == INVALID and block(good, ch=3) == INVALID
    assert block(good, n=0) == 0 and block(good, streams=0) == 0, "nothing to do: NAE_OK"
    h = C.c_void_p()
    for field, values in (("open_lin", (0.001, np.inf, np.nan)), ("close_lin", (0.0, -0.01, 0.5, np.nan)), ("threshold_db", (-90.5, 0.5, np.nan)),
                          ("slope", (-0.1, 99.5, np.inf)), ("range_db", (-1.0, 120.5, np.nan)), ("alpha_attack", (-0.1, 1.0, np.nan)),
                          ("alpha_release", (-0.1, 1.0, np.inf)), ("hold", (-1,)), ("lookahead", (-1,)), ("expand", (2, -1)), ("link", (2, -1))):
        for v in values:
            p = gate_ref.params()
            setattr(p, field, v)
            assert block(p) == INVALID, (field, v)
            assert block(p, n=0) == INVALID, "checked before the empty call returns"
            assert lib.nae_gate_create(ctx.h, C.byref(lib_params(nae, p)), 2, C.byref(h)) == INVALID and not h.value, (field, v)
    for far in (gate_ref.params(lookahead=1025), gate_ref.params(hold=gate_ref.MAX_HOLD + 1)):
        assert block(far) == UNSUPPORTED and lib.nae_gate_create(ctx.h, C.byref(lib_params(nae, far)), 2, C.byref(h)) == UNSUPPORTED and not h.value
    assert block(gate_ref.params(lookahead=1024, hold=gate_ref.MAX_HOLD)) == 0
    assert lib.nae_gate_create(ctx.h, None, 2, C.byref(h)) == INVALID
    assert lib.nae_gate_create(ctx.h, C.byref(lib_params(nae, good)), 3, C.byref(h)) == INVALID
    assert lib.nae_gate_create(ctx.h, C.byref(lib_params(nae, good)), 2, None) == INVALID
    ctx.sync()
    assert np.array_equal(d.download()[16:32], np.zeros(16, np.float32))
    d.free()


def test_host_node_graph(host):
    """source -> audio_gate -> sink with 1152-sample frames: the source's frames, sizes and pts; the statement's samples with the designed
    parameters, and the block call's"""
    r = subprocess.run([host, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST GATE OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_host_node_lookahead_too_long(host):
    """a look-ahead of more than 1024 samples at the stream's rate is a Runtime_error on the first frame"""
    r = subprocess.run([host, "lookahead"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST GATE OK lookahead" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_fuzz_gate_seeded(nae, ctx):
    """a seeded run of tests/tools/fuzz_gate.py: parameters over their whole range, lengths, views and put patterns"""
    sys.path.insert(0, os.path.join(gate_ref.ROOT, "tests", "tools"))
    import fuzz_gate
    assert fuzz_gate.main(cases=fuzz_gate.SEEDED[0], seed=fuzz_gate.SEEDED[1], ctx=ctx, nae=nae) == fuzz_gate.SEEDED[0]
