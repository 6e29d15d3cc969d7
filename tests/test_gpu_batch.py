"""Every effect node (K9 FIR, K10 long convolution, K11 equalizer, K12 dynamics, K13 noise gate, K14 loudness, K15 keyed dynamics, K16 echo)
in one block call at a batch that fills the chip, every stream of it bit for bit against the CPU statement.  The nodes' own suites stop at a
handful of streams, where every wave has its CU, its L1 and its LDS to itself and the whole launch is one dispatch round; a wrong stream or
channel index, a product that leaves an int, a wait a lone wave never needs or a stage reused one chunk early show only in company.

A case (the functions *_case below) is built without the device: distinct content per stream, the statement on every stream (no stream is
sampled), and the conditions on the statement's own output that make a pass mean something — the gain moves, the repeat is there, the gate
opens and closes, the gains differ.  tests/test_batch_cases_cpu.py builds every case at a few streams, so the conditions are checked where
there is no device.  `run` then makes the one block call through block_gpu.view_call, which checks the guard words behind every destination
signal, and on a mismatch names the number of differing streams and the first stream and channel indices (block_gpu.mismatch)."""
import numpy as np
import pytest

import conv_ref
import denoise_ref
import dyn_ref
import dynkey_ref
import echo_ref
import eq_ref
import fir_ref
import loud_ref
from block_gpu import bits, each_stream, mismatch, noise, statement
from denoise_gpu import gpu_denoise
from dyn_gpu import gpu_dyn
from dynkey_gpu import gpu_dynkey
from echo_gpu import gpu_echo
from eq_gpu import gpu_eq
from fir_gpu import MIN_TILE as FIR_MIN_TILE, gpu_fir
from loud_gpu import gpu_measure, gpu_normalize
from test_gpu_conv import gpu_conv
from test_gpu_dynkey import MID, loud

pytestmark = pytest.mark.gpu

# The headline workload: the stream count of BASELINE's C5 and of every tools/*_time.py.  The signals run several units long (a unit: the K11 /
# K12 chunk of 1024 samples, the FIR's and the convolution's block of n_fft / 2, the gate's hop block), so that the waves of a launch live
# side by side for several iterations.
WORKLOAD = 1024
# 4099 stereo streams are 8198 stream-channel waves.  The chip holds at most 256 CUs x 32 waves = 8192, whatever a kernel's registers or LDS
# allow, so every kernel needs a second dispatch round, with no occupancy measured; 4099 is odd and prime, so no workgroup packing divides it.
# The signals stay short (about three units and a ragged tail): the equalizer's case moves about 100 MB each way.
OVERFULL = 4099

UNIT = eq_ref.CHUNK
DENOISE_MIN_TILE = 32          # NAE_DENOISE_MIN_TILE
LOUD_RATE = 8000               # a 100 ms sub-block is 800 samples
ECHO_WS_BYTES = 256 << 20      # the cap of the echo's lines per launch (NAE_CONV_WS_BYTES)


class Case:
    """x[streams, n, ch], the statement's `want`, and gpu(nae, ctx) -> the block call's output in the case's view"""

    def __init__(self, x, want, gpu):
        self.x, self.want, self.gpu = x, want, gpu

    def run(self, nae, ctx):
        got = self.gpu(nae, ctx)
        message = mismatch(got, self.want)
        assert not message, message
        return got


def in_slices(make, n_streams, step=128):
    """make(k) -> [k, ...] for k streams, called for `step` streams at a time: a generator's float64 temporaries stay small"""
    return np.concatenate([make(min(step, n_streams - s)) for s in range(0, n_streams, step)])


# ------------------------------------------------------------------------------------ conditions, asserted on the statement's output
def moved_share(want, x):
    """per stream, the share of samples the statement changed"""
    return (bits(want) != bits(x)).reshape(len(x), -1).mean(axis=1)


def assert_the_gain_moves(want, x):
    share = moved_share(want, x)
    assert np.all(share >= 0.5), f"the statement changes at least half the samples of every stream: least {share.min():.3f} in stream {share.argmin()}"


def dry_only(p, x):
    """what the echo's statement gives where no repeat has arrived: one f32 rounding of dry * x"""
    return (p.dry * x.astype(np.float64)).astype(np.float32)


def assert_the_repeat_is_there(want, x, p):
    first = min(p.delay[0], p.delay[1])
    heard = (want[:, first:] != dry_only(p, x[:, first:])).reshape(len(x), -1).any(axis=1)
    assert np.all(heard), f"the statement differs from dry * x past the delay in every stream: not in {np.flatnonzero(~heard)[:8]}"


def assert_the_gate_works(want, x, floor_gain):
    """With every decision open the gate's output is the input, with every one closed it is floor_gain times the input, each up to the f32
    roundings of a transform and an overlap-add, some 1e-6 of the peak; one decision the other way moves a bin by (1 - floor_gain) of its
    content.  1e-3 of the peak lies far from both."""
    peak = np.abs(x).reshape(len(x), -1).max(axis=1)
    from_input = np.abs(want - x).reshape(len(x), -1).max(axis=1)
    from_floor = np.abs(want - np.float32(floor_gain) * x).reshape(len(x), -1).max(axis=1)
    assert np.all(from_input > 1e-3 * peak), f"the statement's output is not the input: streams {np.flatnonzero(from_input <= 1e-3 * peak)[:8]}"
    assert np.all(from_floor > 1e-3 * peak), f"the statement's output is not all at the floor gain: streams {np.flatnonzero(from_floor <= 1e-3 * peak)[:8]}"


def assert_the_gains_differ(records):
    """not all equal; and, as the gate kernel packs 64 streams into a workgroup, not within any 64 streams in a row either"""
    gains = np.array([r.gain_f32 for r in records])
    assert len(set(gains.tolist())) > 1, "the statement's gains are not all equal"
    for s in range(0, len(gains) - 1, 64):
        assert len(set(gains[s:s + 64].tolist())) > 1, f"the statement's gains differ within streams {s} ... {s + 63}"


# ------------------------------------------------------------------------------------ cases
VIEWS = {"ii": dict(src_layout="i", dst_layout="i"), "pp": dict(src_layout="p", dst_layout="p", chan_pad=5), "pi": dict(src_layout="p", dst_layout="i"),
         "shared": dict(src_layout="i", dst_layout="i", shared=True)}


def eq_case(n_streams, sections, units, view="ii"):
    """view "shared": one source for the whole batch (stream_stride = 0): every output equals the statement for stream 0"""
    ref, coef, n = statement(eq_ref), eq_ref.cascade(sections), units * UNIT + 7
    distinct = 1 if view == "shared" else n_streams
    x = noise(np.random.default_rng(1100 + sections), distinct, n, 2)
    want = each_stream(lambda i: eq_ref.run(ref, coef, x[i].reshape(-1), ch=2).reshape(n, 2), distinct)
    if view == "shared":
        x, want = np.broadcast_to(x, (n_streams, n, 2)), np.broadcast_to(want, (n_streams, n, 2))
    assert not np.array_equal(bits(want[0]), bits(x[0]))
    return Case(x, want, lambda nae, ctx: gpu_eq(nae, ctx, coef, x, **VIEWS[view]))


def dyn_case(n_streams, link, lookahead, units):
    ref, n = statement(dyn_ref), units * UNIT + 7
    p = dyn_ref.params(lookahead=lookahead, link=link, **MID)
    rng = np.random.default_rng(1200 + 2 * lookahead + link)
    x = in_slices(lambda k: loud(rng, k, n, 2), n_streams)
    want = each_stream(lambda i: dyn_ref.run(ref, p, x[i]), n_streams)
    assert_the_gain_moves(want, x)
    return Case(x, want, lambda nae, ctx: gpu_dyn(nae, ctx, p, x))


def dynkey_case(n_streams, kind, units):
    """kind "stereo key": a key of its own per stream through four slow sections; "shared key": one such key for the whole batch
    (stream_stride = 0); "self-keyed": key_ch = 0, the signal through two sections"""
    ref, n = statement(dynkey_ref), units * UNIT + 7
    filters = dynkey_ref.key_filters()
    rng = np.random.default_rng(1300 + len(kind))
    dp = dyn_ref.params(lookahead=48, link=1, **MID)
    if kind == "self-keyed":
        p, key = dynkey_ref.params(dp, 0, filters[4][:2]), None
        x = in_slices(lambda k: loud(rng, k, n, 2), n_streams)
    else:
        p = dynkey_ref.params(dp, 2, filters[4])
        x = noise(rng, n_streams, n, 2)
        key = in_slices(lambda k: loud(rng, k, n, 2), 1 if kind == "shared key" else n_streams)
    want = each_stream(lambda i: dynkey_ref.run(ref, p, x[i], None if key is None else key[min(i, len(key) - 1)]), n_streams)
    assert_the_gain_moves(want, x)
    keys = None if key is None else np.broadcast_to(key, (n_streams, n, 2)) if kind == "shared key" else key
    return Case(x, want, lambda nae, ctx: gpu_dynkey(nae, ctx, p, x, keys, key_layout="s" if kind == "shared key" else "i"))


def echo_case(n_streams, delay, cross, sections, units=None, view="ii"):
    """in_len: 3 R + 7, or units * 1024 + 7"""
    ref = statement(echo_ref)
    p = echo_ref.params(delay, -0.9 if cross else 0.9, cross, 0.6, 0.8, echo_ref.loop_filters()[sections])
    n = (3 * echo_ref.ring(p, 2) if units is None else units * UNIT) + 7
    x = noise(np.random.default_rng(1400 + delay[0] + 2 * delay[1] + sections), n_streams, n, 2)
    want = each_stream(lambda i: echo_ref.run(ref, p, x[i]), n_streams)
    if n > max(delay):
        assert_the_repeat_is_there(want, x, p)
    else:
        assert np.array_equal(want, dry_only(p, x)), "no repeat is reached: the statement is dry * x"
    case = Case(x, want, lambda nae, ctx: gpu_echo(nae, ctx, p, x, **VIEWS[view]))
    case.params = p
    return case


def fir_case(n_streams, n_fft, n_taps, blocks):
    ref, n = statement(fir_ref), blocks * (n_fft // 2) + 7
    rng = np.random.default_rng(1500 + n_fft)
    taps = rng.uniform(-1, 1, n_taps).astype(np.float32)
    x = noise(rng, n_streams, n, 2)
    want = each_stream(lambda i: fir_ref.run(ref, taps, n_fft, x[i].reshape(-1), ch=2).reshape(n, 2), n_streams)
    return Case(x, want, lambda nae, ctx: gpu_fir(nae, ctx, taps, n_fft, x))


def conv_case(n_streams, n_fft, n_taps, blocks):
    """one response per channel"""
    ref, n = statement(conv_ref), blocks * (n_fft // 2) + 7
    rng = np.random.default_rng(1600 + n_fft)
    taps = (rng.uniform(-1, 1, (2, n_taps)) * np.exp(-np.arange(n_taps) / 150.0)).astype(np.float32)
    x = noise(rng, n_streams, n, 2)
    want = each_stream(lambda i: conv_ref.run(ref, taps, n_fft, x[i].reshape(-1), ch=2).reshape(n, 2), n_streams)
    return Case(x, want, lambda nae, ctx: gpu_conv(nae, ctx, taps, n_fft, x))


def denoise_case(n_streams, n_fft, tiles):
    """`tiles` tiles of NAE_DENOISE_MIN_TILE hop blocks per stream-channel and a ragged tail; a profile per channel"""
    ref, hop = statement(denoise_ref), n_fft // 4
    n = tiles * DENOISE_MIN_TILE * hop + 37
    p = denoise_ref.params(n_fft, 2, 2, 1.0, 0.1)
    profile = denoise_ref.flat_profile(n_fft, 2, tilt_db=-3.0)
    rng = np.random.default_rng(1700 + n_fft)
    x = in_slices(lambda k: denoise_ref.wander(rng, k, n, 2, period=3.0 * n_fft), n_streams, 64)
    want = each_stream(lambda i: denoise_ref.run(ref, p, profile, x[i]), n_streams)
    assert_the_gate_works(want, x, p.floor_gain)
    return Case(x, want, lambda nae, ctx: gpu_denoise(nae, ctx, p, profile, x))


class LoudCase:
    """streams whose levels are spread over 40 dB, all 64 of the spread's steps within any 64 streams in a row (37 is coprime to 64); every
    stream 20 dB quieter in its first third, so the relative gate drops blocks"""

    def __init__(self, n_streams, n, normalize):
        ref = statement(loud_ref)
        self.normalize = normalize
        rc, params = loud_ref.design_c(ref, LOUD_RATE, max_gain_db=40.0)       # tests/test_loud_cpu.py: nae_loud_design's record, bit for bit
        assert rc == 0
        self.params = params
        rng = np.random.default_rng(1800)
        level_db = -6.0 - 40.0 * ((np.arange(n_streams) * 37) % 64) / 63.0 - 20.0 * (np.arange(n) < n // 3)[:, None]      # [n, streams]
        self.x = in_slices(lambda k: rng.uniform(-1, 1, (k, n, 2)), n_streams).astype(np.float32)
        self.x *= (10.0 ** (level_db.T / 20.0)).astype(np.float32)[:, :, None]
        self.records = [loud_ref.measure(ref, params, s)[0] for s in self.x]
        assert_the_gains_differ(self.records)
        assert all(r.blocks_rel > 0 for r in self.records), "every stream has loudness"
        if n >= LOUD_RATE:
            assert all(r.blocks_rel < r.blocks_abs for r in self.records), "over a second or more the relative gate drops blocks of every stream"
        self.want = self.x * np.array([r.gain_f32 for r in self.records], np.float32)[:, None, None] if normalize else None

    def run(self, nae, ctx):
        params = nae.LoudParams.from_buffer_copy(bytes(self.params))
        if self.normalize:
            y, records = gpu_normalize(nae, ctx, params, self.x)
        else:
            y, records = None, gpu_measure(nae, ctx, params, self.x)
        bad = [s for s, (g, w) in enumerate(zip(records, self.records)) if loud_ref.record_fields(g) != loud_ref.record_fields(w)]
        assert not bad, f"the records of {len(bad)} of {len(records)} streams differ; first streams: {bad[:8]}"
        if y is not None:
            message = mismatch(y, self.want)
            assert not message, message


def loud_case(n_streams, n, normalize=False):
    return LoudCase(n_streams, n, normalize)


# The case tables: name -> (builder, arguments behind the stream count).  tests/test_batch_cases_cpu.py builds them at a few streams.
WORKLOAD_CASES = {
    "eq-ii": (eq_case, (4, 5, "ii")), "eq-pp": (eq_case, (4, 5, "pp")), "eq-shared": (eq_case, (4, 5, "shared")),
    "dyn-linked-la0": (dyn_case, (1, 0, 5)), "dyn-linked-la48": (dyn_case, (1, 48, 5)),
    "dyn-unlinked-la0": (dyn_case, (0, 0, 5)), "dyn-unlinked-la48": (dyn_case, (0, 48, 5)),
    "dynkey-stereo-key": (dynkey_case, ("stereo key", 5)), "dynkey-shared-key": (dynkey_case, ("shared key", 5)),
    "dynkey-self-keyed": (dynkey_case, ("self-keyed", 5)),
    "fir-512": (fir_case, (512, 257, 9)), "fir-2048": (fir_case, (2048, 1025, 9)),
    "conv-512": (conv_case, (512, 700, 9)),
    "denoise-512": (denoise_case, (512, 2)), "denoise-2048": (denoise_case, (2048, 2)),
    "loud-measure": (loud_case, (3 * LOUD_RATE // 2 + 37, False)), "loud-normalize": (loud_case, (3 * LOUD_RATE // 2 + 37, True)),
}
ECHO_CASES = {f"echo-{d[0]}-{d[1]}-{'cross' if cross else 'straight'}-{sections}s": (d, cross, sections)
              for d, cross in (((1024, 1024), 1), ((1024, 1500), 1), ((1500, 1024), 0)) for sections in (0, 4)}
# 3 units + 7 frames; the FIR, the convolution and the gate one tile and a ragged block.  The loudness meter needs four sub-blocks of 800
# samples for its first 400 ms block, so its three units would leave every record without a block and every gain 1: it runs four.
OVERFULL_CASES = {
    "eq": (eq_case, (2, 3)), "dyn-unlinked": (dyn_case, (0, 48, 3)), "dynkey-self-keyed": (dynkey_case, ("self-keyed", 3)),
    "echo": (echo_case, ((1024, 1024), 1, 1, 3)), "loud-measure": (loud_case, (4 * UNIT + 7, False)),
    "fir-512": (fir_case, (512, 257, FIR_MIN_TILE)), "conv-512": (conv_case, (512, 700, FIR_MIN_TILE)),
    "denoise-512": (denoise_case, (512, 1)),
}
GROUPING = dict(n_streams=600, delay=(1 << 17, 1 << 17), units=2)


def build(table, name, n_streams):
    builder, args = table[name]
    return builder(n_streams, *args)


def grouping_case():
    """the echo's default grouping: the ring is sized by the delay, not the input, so 600 streams at a delay of 2^17 samples exceed the cap of
    one launch's lines while the signals stay tiny; a planar source and an interleaved destination, so a group's base moves by both strides"""
    case = echo_case(GROUPING["n_streams"], GROUPING["delay"], 1, 1, GROUPING["units"], view="pi")
    line_bytes = echo_ref.ring(case.params, 2) * 2 * 4
    assert 2 * (ECHO_WS_BYTES // line_bytes) < GROUPING["n_streams"], "the batch is cut into at least three groups, the last one short"
    return case


# ------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", sorted(WORKLOAD_CASES))
def test_workload(nae, ctx, name):
    build(WORKLOAD_CASES, name, WORKLOAD).run(nae, ctx)


@pytest.mark.parametrize("name", sorted(ECHO_CASES))
def test_workload_echo(nae, ctx, name):
    """in_len = 3 R + 7; once more under echo_group = 300 (four launches, the last one short, every one on the workspace's first rings): the
    default run's bits"""
    case = echo_case(WORKLOAD, *ECHO_CASES[name])
    got = case.run(nae, ctx)
    try:
        ctx.debug_set("echo_group", 300)
        grouped = case.gpu(nae, ctx)
    finally:
        ctx.debug_set("echo_group", 0)
    message = mismatch(grouped, got)
    assert not message, "echo_group = 300: " + message


def test_echo_default_grouping(nae, ctx):
    grouping_case().run(nae, ctx)


def test_workload_conv_wraps_its_ring(nae, ctx):
    """conv_ring = 5 at three partitions: slabs of three blocks, and the ten blocks wrap the five slots twice"""
    case = build(WORKLOAD_CASES, "conv-512", WORKLOAD)
    try:
        ctx.debug_set("conv_ring", 5)
        case.run(nae, ctx)
    finally:
        ctx.debug_set("conv_ring", 0)


@pytest.mark.parametrize("name", sorted(OVERFULL_CASES))
def test_overfull(nae, ctx, name):
    build(OVERFULL_CASES, name, OVERFULL).run(nae, ctx)
