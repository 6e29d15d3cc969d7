"""The vocoder pipeline's phase roles lost bookkeeping instructions (pv_roles.h: advance term, 32-bit loop indices); every output sample
keeps its bits.  tests/golden/pv_diet_parent.npz holds what the build before that change wrote, as float32 bit patterns; every shape of the
pipeline (one / two / four frames per step, both schedules, lean and rich, with and without forced time tiles) and a streaming handle must
still write exactly that.  At +3 semitones the size-generic route (pv_any) is held against the pipeline as
tests/test_gpu_pv_sizes.py::test_generic_kernels_at_1024_match_the_shipped_ones holds it: same integer phases, samples within 1e-4."""
import os

import numpy as np
import pytest

import orc
from conftest import rel_rms
from pv_gpu import block, same_bits, stream

pytestmark = pytest.mark.gpu

TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pv_diet_parent.npz")

# signal: (streams, channels, sample-frames, semitones)
SIGNALS = {
    "stereo_p3": (2, 2, 12000, 3),       # transposer first; both hop differences d occur
    "stereo_m3": (2, 2, 12000, -3),      # vocoder first
    "stereo_p12": (2, 2, 12000, 12),     # integer analysis hop: a single d
    "mono_p3": (1, 1, 9000, 3),
}
# pipeline shape: debug keys.  "lean" is the headline kernel (one frame per step, 64 VGPRs, two workgroups per CU)
SHAPES = {
    "library": {},
    "lean": {"pv_fps": 1, "pv_flow": 0, "pv_lean": 1},
    "lean_tiles": {"pv_fps": 1, "pv_flow": 0, "pv_lean": 1, "pv_tile": 16},
    "rich": {"pv_fps": 1, "pv_flow": 0},
    "fps2": {"pv_fps": 2, "pv_flow": 0},
    "fps2_tiles": {"pv_fps": 2, "pv_flow": 0, "pv_tile": 16},
    "fps4": {"pv_fps": 4, "pv_flow": 0},
    "fps4_tiles": {"pv_fps": 4, "pv_flow": 0, "pv_tile": 16},
    "flow1": {"pv_fps": 1, "pv_flow": 2},
    "flow1_tiles": {"pv_fps": 1, "pv_flow": 2, "pv_tile": 16},
    "flow2": {"pv_fps": 2, "pv_flow": 2},
    "flow4_tiles": {"pv_fps": 4, "pv_flow": 2, "pv_tile": 16},
}
STREAM_PUTS = (5000, 1234, 5766)         # three unequal puts of the 12 000 sample-frames of stream 0 of stereo_p3


def signal_of(name):
    n, ch, L, semi = SIGNALS[name]
    return (0.5 * orc.fill_uniform(n * L * ch, 77 + abs(semi))).astype(np.float32), n, ch, 2.0 ** (semi / 12)


def run_shape(nae, name, shape):
    x, n, ch, pitch = signal_of(name)
    with nae.Context(0) as c:
        for k, v in SHAPES[shape].items():
            c.debug_set(k, v)
        return block(c, nae, x, ch, 1.0, pitch, n_streams=n)


def run_stream(nae):
    x, n, ch, pitch = signal_of("stereo_p3")
    with nae.Context(0) as c:
        return stream(c, x[: x.size // n], ch, 1.0, pitch, STREAM_PUTS, "ex")


@pytest.fixture(scope="module")
def parent():
    return np.load(GOLDEN)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_pipeline_keeps_the_parents_bits(nae, parent, name, shape):
    got = run_shape(nae, name, shape)
    want = parent[name]
    assert got.size == want.size > 0
    diff = int(np.count_nonzero(got.view(np.uint32) != want))
    print(f"{name} {shape}: {diff} of {want.size} samples differ")
    assert diff == 0


def test_streaming_handle_keeps_the_parents_bits(nae, parent):
    got = run_stream(nae)
    want = parent["stream_p3"]
    assert got.size == want.size > 0
    assert int(np.count_nonzero(got.view(np.uint32) != want)) == 0


def test_generic_route_agrees_with_the_pipeline(nae, parent):
    """pv_any = 1 at N = 1024 (phase code of its own, pv_any.h): the integer phases in front of every 16-frame tile are the pipeline
    route's bit for bit, the samples within 1e-4 — and the pipeline's samples are the parent's"""
    x, n, ch, pitch = signal_of("stereo_p3")
    x = x[: x.size // n]
    L = x.size // ch
    res = {}
    for key in (0, 1):
        with nae.Context(0) as c:
            c.debug_set("pv_tile", 16)
            c.debug_set("pv_any", key)
            d_x = c.array(x)
            ph, t = c.debug_pv_tile_phase(1.0, pitch, nae.Sig.interleaved(d_x.ptr, L, ch), L, ch, 1)
            d_x.free()
            assert t == 16 and ph.shape[2] >= 2
            c.prof_reset(); c.prof_enable(True)
            out = block(c, nae, x, ch, 1.0, pitch)
            c.prof_enable(False)
            assert ("pv_any_synth_kernel" in set(c.prof_report())) == (key == 1)
            res[key] = ph, out
    assert np.array_equal(res[0][0], res[1][0])
    assert same_bits(res[0][1].view(np.uint32), parent["stereo_p3"][: res[0][1].size])
    e = rel_rms(res[1][1], res[0][1])
    print(f"pv_any at 1024, +3 semitones: {e:.3g}")
    assert e <= TOL, e
