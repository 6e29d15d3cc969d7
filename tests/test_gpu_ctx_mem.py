"""GPU: the context's device memory (csrc/ctx_mem.h): every workspace, table and last-call constant of a context is a CtxBuf or a CtxConst, so
what a call delivers must not depend on what the context ran before it.  The oracle of every comparison is a FRESH context that runs only the
call in question; the comparison is bit equality (the same code on the same device).  Four statements: the constants do not remember more
than their key (1), a hit launches nothing and a miss launches once (2), a workspace that grows waits for the work in flight (3), and a
context that held everything can be destroyed beside one that is in use (4)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 5 * 256 + 9          # frames: five half frames of the smallest FFT and a ragged end


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noise(seed, n_streams, n, ch=2):
    return np.random.default_rng(seed).uniform(-1, 1, (n_streams, n, ch)).astype(np.float32)


def prepare(c, call, x, per):
    """x[streams, n, ch] uploaded to context c and a zeroed destination of `per` floats per stream.  call(c, src, n, ch, n_streams, ptr, per) is
    a block entry on the interleaved source.  Returns (enqueue, result): enqueue() makes the call and waits for nothing; result() downloads
    [streams, per] (which waits) and frees."""
    nae = c.nae
    n_streams, n, ch = x.shape
    d_x, d_y = c.array(x.reshape(-1)), c.array(np.zeros(n_streams * per, np.float32))
    src = nae.Sig.interleaved(d_x.ptr, n, ch)

    def result():
        out = d_y.download().reshape(n_streams, per)
        d_x.free()
        d_y.free()
        return out
    return (lambda: call(c, src, n, ch, n_streams, d_y.ptr, per)), result


def run(c, call, x, per):
    enqueue, result = prepare(c, call, x, per)
    enqueue()
    return result()


def context(nae):
    c = nae.Context(0)
    c.nae = nae
    return c


def fresh(nae, call, x, per, setup=None):
    c = context(nae)
    try:
        if setup:
            setup(c)
        return run(c, call, x, per)
    finally:
        c.close()


def sig_call(fn):
    """a block entry with a destination view of as many channels as the source: fn(c, src, n, ch, n_streams, dst)"""
    return lambda c, src, n, ch, n_streams, ptr, per: fn(c, src, n, ch, n_streams, c.nae.Sig.interleaved(ptr, per // ch, ch))


# ---- one step of a walk: (key, call, x, floats per stream of the destination); equal keys are the same call
def fir_step(taps, n_fft, x, key):
    return key, sig_call(lambda c, s, n, ch, ns, d: c.fir_block(taps, s, n, ch, ns, d, n_fft)), x, x.shape[1] * x.shape[2]


def conv_step(taps, n_fft, x, key):
    return key, sig_call(lambda c, s, n, ch, ns, d: c.conv_block(taps, s, n, ch, ns, d, n_fft)), x, x.shape[1] * x.shape[2]


def eq_step(coef, x, key):
    return key, sig_call(lambda c, s, n, ch, ns, d: c.eq_block(coef, s, n, ch, ns, d)), x, x.shape[1] * x.shape[2]


def loud_step(params, x, key):
    return key, sig_call(lambda c, s, n, ch, ns, d: c.loud_normalize(params, s, n, ch, ns, d)), x, x.shape[1] * x.shape[2]


def sat_step(nae, oversample, x):
    p = nae.SatParams.make(oversample, 0, 4.0, 0.1, 0.8, 0.2)
    return ("sat", oversample), sig_call(lambda c, s, n, ch, ns, d: c.sat_block(p, s, n, ch, ns, d)), x, x.shape[1] * x.shape[2]


def echo_step(nae, x, key="echo"):
    p = nae.EchoParams.make((1500, 1024), 0.6, True, 0.5, 0.8, [nae.Context.eq_design("lowpass", 44100, 5000.0)])
    return key, sig_call(lambda c, s, n, ch, ns, d: c.echo_block(p, s, n, ch, ns, d)), x, x.shape[1] * x.shape[2]


def stretch_step(nae, rate, pitch, n_fft, x):
    pl = nae.Context.stretch_plan(rate, pitch, x.shape[1], n_fft)
    return (("stretch", rate, pitch, n_fft, x.shape), sig_call(lambda c, s, n, ch, ns, d: c.stretch_block(rate, pitch, s, n, ch, ns, d, n_fft=n_fft)), x,
            pl.out_len * x.shape[2])


def spectrum_step(nae, n_fft, x):
    hop, ch = n_fft // 4, x.shape[2]
    per = int(nae.load_library().nae_spectrum_frames_ex(x.shape[1], n_fft, hop)) * ch * (n_fft // 2 + 1)
    return ("spectrum", n_fft), (lambda c, s, n, ch_, ns, ptr, per_: c.spectrum_block_ex(n_fft, hop, s, n, ch_, ns, ptr, per_)), x, per


def wsola_step(nae, x, sr=44100, rate=1.0, pitch=1.26):
    pl = nae.Context.wsola_plan(sr, x.shape[2], rate, pitch, x.shape[1])
    return (("wsola", x.shape), sig_call(lambda c, s, n, ch, ns, d: c.wsola_block(sr, rate, pitch, s, n, ch, ns, d)), x, pl.out_len * x.shape[2])


def walk(nae, ctx, steps):
    """every step on the one context `ctx`, in order; each output is what a fresh context delivers for that step alone"""
    ctx.nae = nae
    want = {}
    for key, call, x, per in steps:
        if key not in want:
            want[key] = fresh(nae, call, x, per)
    for i, (key, call, x, per) in enumerate(steps):
        assert np.array_equal(bits(run(ctx, call, x, per)), bits(want[key])), (i, key)
    return want


def differ(want, *keys):
    """the walk's steps are different calls: their fresh results differ (else the walk would show nothing)"""
    first = want[keys[0]]
    return all(want[k].shape != first.shape or not np.array_equal(bits(want[k]), bits(first)) for k in keys[1:])


# ------------------------------------------------------------------------------------------------ 1. history independence of the constants
def test_fir_constant_has_no_history(nae, ctx):
    rng = np.random.default_rng(1)
    a, b = rng.uniform(-1, 1, 100).astype(np.float32), rng.uniform(-1, 1, 100).astype(np.float32)
    x = noise(2, 2, N)
    A, B, A1024 = fir_step(a, 512, x, "a512"), fir_step(b, 512, x, "b512"), fir_step(a, 1024, x, "a1024")
    want = walk(nae, ctx, [A, A, B, A, A, A1024, A])
    assert differ(want, "a512", "b512")


def test_eq_constant_has_no_history(nae, ctx):
    A = np.stack([nae.Context.eq_design("peak", 44100, 1000.0, 6.0, 1.0), nae.Context.eq_design("lowpass", 44100, 8000.0)])
    B = np.stack([nae.Context.eq_design("peak", 44100, 1200.0, -3.0, 2.0), nae.Context.eq_design("highpass", 44100, 90.0)])
    x = noise(3, 3, 4000)
    want = walk(nae, ctx, [eq_step(A, x, "A"), eq_step(A, x, "A"), eq_step(B, x, "B"), eq_step(A, x, "A")])
    assert differ(want, "A", "B")


def test_loud_constant_has_no_history(nae, ctx):
    """20000 frames: one gating block at either rate, so the K-weighting decides the gain"""
    A, B = nae.Context.loud_design(44100), nae.Context.loud_design(48000)
    x = 0.25 * noise(4, 2, 20000)
    want = walk(nae, ctx, [loud_step(A, x, "A"), loud_step(A, x, "A"), loud_step(B, x, "B"), loud_step(A, x, "A")])
    assert differ(want, "A", "B")


def test_sat_tap_slots_have_no_history(nae, ctx):
    x = noise(5, 2, 4000)
    want = walk(nae, ctx, [sat_step(nae, m, x) for m in (2, 4, 8, 2)])
    assert differ(want, ("sat", 2), ("sat", 4), ("sat", 8))


def test_transposer_table_has_no_history(nae, ctx):
    x = noise(6, 2, 4000)
    walk(nae, ctx, [stretch_step(nae, r, 1.0, 1024, x) for r in (1.25, 0.8, 1.25)])


def test_fft_tables_of_every_size_have_no_history(nae, ctx):
    x = noise(7, 2, 12000)
    walk(nae, ctx, [stretch_step(nae, 1.0, 1.25, n, x) for n in (512, 2048, 512)])
    walk(nae, ctx, [spectrum_step(nae, n, x) for n in (256, 4096, 256)])


def test_wsola_plan_cache_has_no_history(nae, ctx):
    x = noise(8, 2, 5000)
    a, b = wsola_step(nae, x[:, :3000]), wsola_step(nae, x)
    walk(nae, ctx, [a, a, b, a])


# ------------------------------------------------------------------------------------------------ 2. hit and miss are what they were
def test_a_hit_launches_nothing_and_a_miss_once(nae):
    """one taps launch per miss, none per hit: the FIR filter's a, a, b, then the long convolution's"""
    rng = np.random.default_rng(9)
    x = noise(10, 1, N)
    c = context(nae)
    try:
        c.prof_enable(True)
        a, b = rng.uniform(-1, 1, 100).astype(np.float32), rng.uniform(-1, 1, 100).astype(np.float32)
        for taps in (a, a, b):
            run(c, *fir_step(taps, 512, x, None)[1:])
        rep = c.prof_report()
        assert rep["fir_taps_kernel"][1] == 2 and rep["fir_block_kernel"][1] == 3, rep
        a, b = rng.uniform(-1, 1, 600).astype(np.float32), rng.uniform(-1, 1, 600).astype(np.float32)
        for taps in (a, a, b):
            run(c, *conv_step(taps, 512, x, None)[1:])
        rep = c.prof_report()
        assert rep["conv_taps_kernel"][1] == 2, rep
        assert rep["fir_taps_kernel"][1] == 2, "the two caches are separate"
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 3. a regrow waits for the work in flight
def grows(first, second):
    """a buffer reserved for `first` bytes (an eighth more and a page: ctx_mem.h) has no room for `second`"""
    return second > first + first // 8 + 4096


def regrow(nae, small, big, setup=None):
    """`small` then `big` on a new context with no wait in between — the second call's workspace does not fit the first one's, so it is freed
    and allocated again while the first call may still run on it — then `small` once more; every output is a fresh context's"""
    want = [fresh(nae, *step[1:], setup=setup) for step in (small, big)]
    c = context(nae)
    try:
        if setup:
            setup(c)
        jobs = [prepare(c, *step[1:]) for step in (small, big)]
        for enqueue, _ in jobs:
            enqueue()
        c.sync()
        got = [result() for _, result in jobs]
        again = run(c, *small[1:])
    finally:
        c.close()
    for i in range(2):
        assert np.array_equal(bits(got[i]), bits(want[i])), i
    assert np.array_equal(bits(again), bits(want[0])), "the small call behind the regrow"


def test_regrow_conv_ring(nae):
    """the ring of a launch group: [stream-channel][blocks + parts - 1][n_fft / 2 + 8] complex; 600 taps at 512 are 3 partitions"""
    taps = np.random.default_rng(11).uniform(-1, 1, 600).astype(np.float32)
    def ring_bytes(n_streams):
        return n_streams * 2 * ((N + 255) // 256 + 2) * (256 + 8) * 8
    assert grows(ring_bytes(1), ring_bytes(4))
    regrow(nae, conv_step(taps, 512, noise(12, 1, N), "1"), conv_step(taps, 512, noise(13, 4, N), "4"))


def test_regrow_echo_lines(nae):
    """one ring of at least the longest delay per stream-channel, so four streams need four times one stream's"""
    one = 1500 * 2 * 4                                          # a lower bound of one stream's lines, in bytes
    assert grows(one, 4 * one) and 4 * one - (one + one // 8) > 4096
    regrow(nae, echo_step(nae, noise(14, 1, 4000)), echo_step(nae, noise(15, 4, 4000)))


def test_regrow_loud_workspace(nae):
    """per stream: two channel states (two sections' carries, two peaks, 16 history samples: 104 bytes each), the sub-block energies
    [sub-block][channel] doubles, one record.  The workspace is small, so the second call takes 16 streams"""
    p = nae.Context.loud_design(8000)
    n = 8000

    def need(n_streams):
        return n_streams * (2 * 104 + (n // p.sub_block) * 2 * 8 + C.sizeof(nae.LoudResult))
    assert grows(need(1), need(16))
    regrow(nae, loud_step(p, 0.25 * noise(16, 1, n), "1"), loud_step(p, 0.25 * noise(17, 16, n), "16"))


@pytest.mark.parametrize("rate,pitch", ((1.25, 0.8), (1.0, 0.8)))
def test_regrow_vocoder_workspaces(nae, rate, pitch):
    """pv_tile 64, so that pass 1 runs and writes one record of 520 words per (stream-channel, tile) into the phase workspace.  At (1.25, 0.8)
    the transposer's ratio is 1 and the vocoder runs alone; at (1, 0.8) the vocoder writes the signal in between, padded to 4 frames per
    channel, into the second workspace and the transposer reads it"""
    n = 24000
    pl = [nae.Context.stretch_plan(rate, pitch, k * n) for k in (1, 8)]
    phase = [2 * ((p.frames + 63) // 64) * 520 * 4 for p in pl]
    assert pl[0].frames > 64 and grows(phase[0], phase[1])
    if pl[0].rs_on:
        mid = [2 * ((p.mid_len + 3) // 4 * 4) * 4 for p in pl]
        assert pl[0].pv_on and grows(mid[0], mid[1])
    regrow(nae, stretch_step(nae, rate, pitch, 1024, noise(18, 1, n)), stretch_step(nae, rate, pitch, 1024, noise(19, 1, 8 * n)),
           setup=lambda c: c.debug_set("pv_tile", 64))


def test_regrow_wsola_workspaces(nae):
    """the signals between the three stages: (length + 8) frames per stream, by the plan's stage order"""
    small, big = noise(20, 1, 3000), noise(21, 4, 12000)

    def need(x):
        pl = nae.Context.wsola_plan(44100, 2, 1.0, 1.26, x.shape[1])
        lens = {0: (pl.td_out_len, pl.aa_out_len), 1: (pl.aa_out_len, pl.cu_out_len)}.get(pl.order, (pl.cu_out_len, pl.aa_out_len))
        return [x.shape[0] * (k + 8) * 2 * 4 for k in lens]
    for first, second in zip(need(small), need(big)):
        assert grows(first, second)
    regrow(nae, wsola_step(nae, small), wsola_step(nae, big))


# ------------------------------------------------------------------------------------------------ 4. destroy with everything populated
def every_node(nae):
    """one call of every node that keeps memory with the context"""
    rng = np.random.default_rng(22)
    x = noise(23, 2, 6000)
    eq = np.stack([nae.Context.eq_design("peak", 44100, 1000.0, 6.0, 1.0)])
    dyn = nae.Context.dyn_design(44100)
    key = nae.DynKeyParams.make(dyn, 0, [nae.Context.eq_design("highpass", 44100, 150.0)])
    mod = nae.Context.mod_design(44100)
    gate = nae.Context.denoise_design(n_fft=2048)

    def denoise(c, s, n, ch, ns, d):
        prof = c.empty(ch * (2048 // 2 + 1))
        c.denoise_profile(2048, s, n, ch, prof.ptr)
        c.denoise_block(gate, prof.ptr, ch, s, n, ch, ns, d)
        prof.free()
    same = x.shape[1] * x.shape[2]
    return [fir_step(rng.uniform(-1, 1, 100).astype(np.float32), 512, x, "fir"), conv_step(rng.uniform(-1, 1, 600).astype(np.float32), 512, x, "conv"),
            eq_step(eq, x, "eq"), ("dynkey", sig_call(lambda c, s, n, ch, ns, d: c.dynkey_block(key, s, None, n, ch, ns, d)), x, same),
            ("dyn", sig_call(lambda c, s, n, ch, ns, d: c.dyn_block(dyn, s, n, ch, ns, d)), x, same), echo_step(nae, x),
            ("mod", sig_call(lambda c, s, n, ch, ns, d: c.mod_block(mod, s, n, ch, ns, d)), x, same),
            loud_step(nae.Context.loud_design(8000), 0.25 * x, "loud"), sat_step(nae, 4, x), ("denoise", sig_call(denoise), x, same),
            stretch_step(nae, 1.0, 0.8, 1024, x), stretch_step(nae, 1.0, 1.25, 2048, x), spectrum_step(nae, 1024, x), spectrum_step(nae, 4096, x),
            wsola_step(nae, x)]


def test_destroy_with_everything_populated(nae, ctx):
    ctx.nae = nae
    steps = every_node(nae)
    before = [run(ctx, *s[1:]) for s in steps]
    other = context(nae)
    try:
        on_other = [run(other, *s[1:]) for s in steps]
    finally:
        other.close()
    third = context(nae)
    try:
        on_third = [run(third, *s[1:]) for s in steps]
        after = [run(ctx, *s[1:]) for s in steps]
    finally:
        third.close()
    for s, b, o, t, a in zip(steps, before, on_other, on_third, after):
        assert np.array_equal(bits(b), bits(a)), s[0]
        assert np.array_equal(bits(b), bits(o)) and np.array_equal(bits(b), bits(t)), s[0]
