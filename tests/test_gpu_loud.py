"""GPU: the loudness meter and normalizer (K14) through the C ABI, bit for bit against the CPU statement (tests/loud_ref/ref_loud.c): every field
of every record (doubles by their 64 bits) and every output sample — in all views of tests/block_gpu.py, at the lengths where the code takes
another path, through the measuring handle under every cut into puts, in a batch of 130 streams, and through the host node."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import loud_ref
import node_harness
from block_gpu import CONFIGS, STATE, bits, statement
from loud_gpu import gpu_measure, gpu_measure_apply, gpu_normalize, loud_stream, same_record

pytestmark = pytest.mark.gpu

# the stepped signal cut so that the last sub-block is incomplete: 8037 samples at 8 kHz (10 sub-blocks, chunks that meet three of them), and
# 3 * 4410 * 4 + 5 at 44.1 kHz (12 sub-blocks of 4410 samples, which is no multiple of a lane's 16)
VIEW_CASES = ((8000, 8037), (44100, 3 * 4410 * 4 + 5))


@pytest.fixture(scope="module")
def ref():
    return statement(loud_ref)


def _streams(sample_rate, ch, n_streams, in_len=None, shared=False):
    """n_streams stepped signals, each with its own noise and its own level (so a gain applied to the wrong stream shows)"""
    x = np.stack([loud_ref.stepped(sample_rate, ch, seed=1000 * sample_rate + 10 * s + ch, scale=0.5 ** s)[:in_len] for s in range(n_streams)])
    if shared:
        x[:] = x[0]
    return x


def _check(ref, params, x, y, records):
    """records and (if given) y against the statement, stream by stream"""
    gains = set()
    for s in range(x.shape[0]):
        want_y, want = loud_ref.normalize(ref, params, x[s])
        same_record(records[s], want)
        if y is not None:
            assert np.array_equal(bits(y[s]), bits(want_y)), f"stream {s}: {np.count_nonzero(bits(y[s]) != bits(want_y))} words differ"
        gains.add(want.gain_f32)
    return gains


@pytest.mark.parametrize("sample_rate,in_len", VIEW_CASES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}ch-{c[1]}st-{c[2]}{c[3]}{'-shared' if c[4] else ''}")
def test_views(nae, ctx, ref, cfg, sample_rate, in_len):
    ch, n_streams, src_layout, dst_layout, shared = cfg
    params = nae.Context.loud_design(sample_rate, max_gain_db=40.0)      # the quietest stream asks for +31 dB
    x = _streams(sample_rate, ch, n_streams, in_len, shared)
    kw = dict(gap=3, offset=1, chan_pad=5)
    records = gpu_measure(nae, ctx, params, x, src_layout, dst_layout, shared, **kw)
    gains = _check(ref, params, x, None, records)
    y, records = gpu_normalize(nae, ctx, params, x, src_layout, dst_layout, shared, **kw)
    _check(ref, params, x, y, records)
    assert len(gains) == (1 if shared else n_streams), "every stream has a gain of its own"
    assert 1.0 not in gains


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}ch-{c[1]}st-{c[2]}{c[3]}{'-shared' if c[4] else ''}")
def test_measure_then_apply_is_normalize(nae, ctx, ref, cfg):
    """nae_loud_apply_f32 as an entry of its own, on the records nae_loud_measure_f32 left: the statement's bits, which are normalize's"""
    ch, n_streams, src_layout, dst_layout, shared = cfg
    params = nae.Context.loud_design(8000, max_gain_db=40.0)
    x = _streams(8000, ch, n_streams, 8037, shared)
    y, records = gpu_measure_apply(nae, ctx, params, x, src_layout, dst_layout, shared, gap=3, offset=1, chan_pad=5)
    _check(ref, params, x, y, records)


def test_apply_in_place_and_empty(nae, ctx, ref):
    """dst may be src; in_len = 0 and n_streams = 0 are NAE_OK and touch nothing"""
    params = nae.Context.loud_design(8000)
    x = _streams(8000, 2, 1, 8037)[0]
    want_y, want = loud_ref.normalize(ref, params, x)
    d = ctx.array(x.reshape(-1))
    d_res = ctx.empty(C.sizeof(nae.LoudResult), np.uint8)
    sig = nae.Sig.interleaved(d.ptr, len(x), 2)
    ctx.loud_measure(params, sig, len(x), 2, 1, d_res.ptr)
    ctx.loud_apply(d_res.ptr, sig, 0, 2, 1, sig)
    ctx.loud_apply(d_res.ptr, sig, len(x), 2, 0, sig)
    assert np.array_equal(bits(d.download()), bits(x.reshape(-1)))
    ctx.loud_apply(d_res.ptr, sig, len(x), 2, 1, sig)
    assert np.array_equal(bits(d.download()), bits(want_y.reshape(-1)))
    same_record(ctx.loud_results(d_res.ptr, 1)[0], want)
    d.free()
    d_res.free()


def test_normalize_keeps_the_records_when_asked_to(nae, ctx, ref):
    params = nae.Context.loud_design(8000)
    x = _streams(8000, 2, 3, 8037)
    y, _ = gpu_normalize(nae, ctx, params, x, records=False)
    for s in range(3):
        assert np.array_equal(bits(y[s]), bits(loud_ref.normalize(ref, params, x[s])[0]))


def _edge_signal(n, rng, level=0.1):
    return (rng.uniform(-1.0, 1.0, (1, n, 2)) * level).astype(np.float32)


CHUNK_END = 20 * 1024
TAIL_LENGTHS = {"1024k-5": CHUNK_END - 5, "1024k-11": CHUNK_END - 11, "1024k": CHUNK_END}


def _tail_signal(name, rng):
    """noise at 0.1 whose last sample alone is 0.9: the oversampler's largest value falls five or six samples behind it.  For 1024k - 5 and
    1024k that is at or past the chunk end, in the one chunk more the true peak needs — a launch without it reads a smaller peak; for
    1024k - 11 it is in the last ten outputs the last whole chunk holds (n = in_len ... in_len + 10).  Asserted on the float64 restatement,
    so the case cannot drift back inside."""
    n = TAIL_LENGTHS[name]
    x = _edge_signal(n, rng)
    x[0, -1, :] = 0.9
    for c in range(2):
        at, peak = loud_ref.true_peak_at(x[0, :, c])
        inside = np.abs(np.stack([np.convolve(x[0, :, c].astype(np.float64), t) for t in loud_ref.taps64()]))[:, :min(CHUNK_END, n)].max()
        if name == "1024k-11":
            assert n <= at < CHUNK_END and at <= n + 10, at
        else:
            assert at >= CHUNK_END, at
        assert peak > 1.05 * inside, "without the tail the peak reads at least 5 % lower"
    return x


@pytest.mark.parametrize("name", ("1024k-5", "1024k-11", "1024k", "4B", "4B-1", "zeros", "ceiling", "max_gain"))
def test_edge_lengths_at_48k(nae, ctx, ref, name):
    """the lengths where the code takes another path, and the three things that can set the gain"""
    rng = np.random.default_rng(len(name))
    B = 4800
    design = dict(target_lufs=-14.0, ceiling_dbtp=-1.0, max_gain_db=20.0)
    if name in TAIL_LENGTHS:
        x = _tail_signal(name, rng)
    else:
        x = _edge_signal({"4B": 4 * B, "4B-1": 4 * B - 1}.get(name, 4 * B + 777), rng)
    if name == "zeros":
        x[:] = 0.0
    if name == "ceiling":
        design.update(target_lufs=-5.0, ceiling_dbtp=-6.0, max_gain_db=40.0)
    if name == "max_gain":
        x *= np.float32(0.01)
        design.update(max_gain_db=3.0)
    params = nae.Context.loud_design(48000, **design)
    y, records = gpu_normalize(nae, ctx, params, x)
    _check(ref, params, x, y, records)
    r = records[0]
    if name == "4B":
        assert r.blocks_total == 1 and r.blocks_rel == 1
    if name in ("4B-1", "zeros"):
        assert r.mean2 == 0.0 and r.gain == 1.0 and r.blocks_rel == 0 and np.array_equal(bits(y), bits(x)), "no loudness: gain 1, the input's bits"
        assert r.blocks_total == (0 if name == "4B-1" else 1)
    if name == "ceiling":
        assert r.gain == params.ceiling_lin / float(max(list(r.true_peak) + list(r.sample_peak)))
    if name == "max_gain":
        assert r.gain == params.max_gain_lin
    if name in TAIL_LENGTHS:
        for c in range(2):
            assert abs(r.true_peak[c] / loud_ref.true_peak_at(x[0, :, c])[1] - 1.0) < 1e-6, "the peak in the tail is the one that is read"


@pytest.mark.parametrize("puts,device", (((1000,), False), ((1024,), True), ((4096, 7), (True, False))), ids=("1000", "1024", "4096+7"))
@pytest.mark.parametrize("name", sorted(TAIL_LENGTHS))
def test_handle_tail(nae, ctx, ref, name, puts, device):
    """the flush measures the one chunk more where the true peak's tail reaches past the last chunk: the block call's record"""
    params = nae.Context.loud_design(48000)
    x = _tail_signal(name, np.random.default_rng(len(name)))[0]
    want, _ = loud_ref.measure(ref, params, x)
    assert abs(want.true_peak[0] / loud_ref.true_peak_at(x[:, 0])[1] - 1.0) < 1e-6
    same_record(loud_stream(nae, ctx, params, x, puts, device), want)


@pytest.mark.parametrize("puts,device", (((1,), False), ((799,), (False, True)), ((1024,), True), ((5000, 3), (True, False, False))),
                         ids=("1", "799", "1024", "5000+3"))
@pytest.mark.parametrize("sample_rate", (8000, 44100))
def test_handle(nae, ctx, ref, sample_rate, puts, device):
    """any cut into puts, from the host and from the device, gives the block call's bits"""
    if puts == (1,) and sample_rate == 44100:
        device = True                # 132 337 puts: from the device they need no wait each
    params = nae.Context.loud_design(sample_rate)
    x = loud_ref.stepped(sample_rate, 2)
    want, _ = loud_ref.measure(ref, params, x)
    same_record(loud_stream(nae, ctx, params, x, puts, device), want)


def test_two_handles_in_one_context(nae, ctx, ref):
    pa, pb = nae.Context.loud_design(8000), nae.Context.loud_design(44100, -23.0, -2.0, 10.0)
    xa, xb = loud_ref.stepped(8000, 2), loud_ref.stepped(44100, 1)
    a, b = nae.Loud(ctx, pa, 2), nae.Loud(ctx, pb, 1)
    try:
        ia = ib = 0
        while ia < len(xa) or ib < len(xb):
            a.put_host(xa[ia:ia + 1500].reshape(-1))
            b.put_host(xb[ib:ib + 7001].reshape(-1))
            ia, ib = ia + 1500, ib + 7001
        a.flush()
        probe = nae.LoudResult()
        assert b._fn("get_result")(b.h, C.byref(probe)) == STATE, "the other handle's flush is not this one's"
        b.flush()
        same_record(b.result(), loud_ref.measure(ref, pb, xb)[0])
        same_record(a.result(), loud_ref.measure(ref, pa, xa)[0])
    finally:
        a.close()
        b.close()


def test_handle_without_input(nae, ctx):
    with nae.Loud(ctx, nae.Context.loud_design(48000), 2) as h:
        h.flush()
        r = h.result()
        assert (r.mean2, r.gain, r.blocks_total, r.true_peak[0], r.sample_peak[1]) == (0.0, 1.0, 0, 0.0, 0.0)


def test_batch_independence(nae, ctx, ref):
    """130 streams of the 8 kHz signal, each with its own seed: every record and output equals the statement's for that stream alone, and the
    GPU's lone run of it"""
    params = nae.Context.loud_design(8000)
    x = np.stack([loud_ref.stepped(8000, 2, seed=7000 + s, scale=1.0 - 0.005 * s) for s in range(130)])
    y, records = gpu_normalize(nae, ctx, params, x)
    _check(ref, params, x, y, records)
    for s in (0, 64, 129):
        y1, r1 = gpu_normalize(nae, ctx, params, x[s:s + 1])
        assert bytes(r1[0]) == bytes(records[s]) and np.array_equal(bits(y1[0]), bits(y[s]))


def test_rejections(nae, ctx):
    lib = ctx.lib
    params = nae.Context.loud_design(48000)
    d = ctx.array(np.zeros(4096, np.float32))
    sig = nae.Sig.interleaved(d.ptr, 1024, 2)
    call = lambda p=params, src=sig, n=1024, ch=2, ns=1, res=d.ptr: lib.nae_loud_measure_f32(ctx.h, C.byref(p) if p else None, C.byref(src) if src else None,
                                                                                                n, ch, ns, res)
    assert call() == 0
    assert call(p=None) == -1 and call(src=None) == -1 and call(res=None) == -1 and call(ch=3) == -1 and call(ch=0) == -1
    assert call(n=0, src=nae.Sig(None, 0, 1, 2)) == 0 and call(ns=0) == 0, "nothing to do: NAE_OK after the checks"
    assert call(src=nae.Sig(None, 0, 1, 2)) == -1
    bad = nae.LoudParams.from_buffer_copy(bytes(params))
    bad.sample_rate = 44101
    assert call(p=bad) == -2
    bad = nae.LoudParams.from_buffer_copy(bytes(params))
    bad.sub_block = 4801
    assert call(p=bad) == -1
    bad = nae.LoudParams.from_buffer_copy(bytes(params))
    bad.coef[9] = 1.0
    assert call(p=bad) == -1, "a section that is not strictly stable"
    bad = nae.LoudParams.from_buffer_copy(bytes(params))
    bad.target = float("nan")
    assert call(p=bad) == -1
    h = C.c_void_p()
    assert lib.nae_loud_create(ctx.h, C.byref(bad), 2, C.byref(h)) == -1 and not h.value
    assert lib.nae_loud_create(ctx.h, C.byref(params), 3, C.byref(h)) == -1 and not h.value
    assert lib.nae_loud_apply_f32(ctx.h, None, C.byref(sig), 1024, 2, 1, C.byref(sig)) == -1
    assert lib.nae_loud_normalize_f32(ctx.h, C.byref(params), C.byref(sig), 1024, 2, 1, None, None) == -1
    ctx.sync()
    d.free()


def test_conformance_anchor_on_the_device(nae, ctx):
    """EBU Tech 3341 case 1 (1 kHz stereo sine at -23 dBFS) cut to 3 s reads -23.0 +- 0.1 LUFS on the device"""
    params = nae.Context.loud_design(48000)
    x = loud_ref.sine_steps(48000, [(3, -23)])[None]
    r = gpu_measure(nae, ctx, params, x)[0]
    print("case 1, 3 s:", r.lufs)
    assert abs(r.lufs - (-23.0)) <= 0.1 and r.blocks_total == 27


def test_host_node(nae, tmp_path):
    """source -> audio_loudness -> sink: the frames as received, the samples of nae_loud_normalize_f32 on the whole stream"""
    exe = node_harness.build("loud_ref/host_loud_node.cpp", str(tmp_path))
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HOST LOUD OK gpu" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
