"""GPU: a seeded, bounded subset of the randomised differential runs of tests/tools/fuzz_*.py (vocoder + spectrum, the
SoundTouch-shaped chain, the N2 converter, the FIR filter, the effect nodes K10 ... K17, the graph step mix -> pitch -> spectrum in every split
and layout, the vocoder's options — lock, transients, channel link, lifter, formant shift, batches, tilings, layouts, handle — on inputs with
onsets) against the CPU oracle and statements.  The full runs (python tests/tools/fuzz_X.py CASES SEED)
draw more cases from the same generators; these fixed seeds keep the driver's `-m gpu` run to a few seconds per test."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

pytestmark = pytest.mark.gpu


def test_fuzz_stretch_and_spectrum_seeded(nae, ctx):
    import fuzz_stretch
    worst = fuzz_stretch.main(cases=10, seed=3, ctx=ctx, nae=nae)
    assert worst <= 1e-4                      # vocoder within tolerance; the spectrum is asserted bit-exact inside


def test_fuzz_stretch_one_barrier_pipeline_in_every_shape(nae):
    """the same randomised run with `debug_set("pv_flow", 2)`: every vocoder launch of at most one workgroup per CU takes the one-barrier schedule (pv_flow_kernel), whatever its shape"""
    import os
    import fuzz_stretch
    with nae.Context(0) as c:
        c.debug_set("pv_flow", 2)
        assert fuzz_stretch.main(cases=10, seed=5, ctx=c, nae=nae) <= 1e-4


def test_fuzz_stretch_any_size_and_range_seeded(nae, ctx):
    """every frame size, the lock, tempo 1/64 ... 16 and rho 1/16 ... 16, edge lengths, batches around the tile-policy switch"""
    import fuzz_stretch_any
    assert fuzz_stretch_any.main(cases=16, seed=3, ctx=ctx, nae=nae) <= 1e-4


def test_fuzz_wsola_seeded(nae, ctx):
    import fuzz_wsola
    assert fuzz_wsola.main(cases=8, seed=3, ctx=ctx, nae=nae) >= 4     # samples and overlap offsets bit-exact


def test_fuzz_swr_seeded(nae, ctx):
    import fuzz_swr
    assert fuzz_swr.main(cases=10, seed=3, ctx=ctx, nae=nae) >= 6      # bit-exact for every cut into convert calls


def test_fuzz_fir_seeded(nae, ctx):
    import fuzz_fir
    assert fuzz_fir.main(cases=36, seed=3, ctx=ctx, nae=nae) == 36     # block call and handle bit-exact in every case drawn


@pytest.mark.parametrize("node", ("conv", "eq", "dyn", "dynkey", "denoise", "loud", "echo", "mod"))
def test_fuzz_effects_seeded(nae, ctx, node):
    """block entry and handle of every effect node bit-exact in every case drawn: parameters over the header's whole ranges, edge lengths, views,
    debug keys and put patterns (tests/test_fuzz_effects_cpu.py pins which edges these seeds reach)"""
    import fuzz_effects
    cases, seed = fuzz_effects.SEEDED[node]
    assert fuzz_effects.main(node, cases=cases, seed=seed, ctx=ctx, nae=nae) == cases


def test_fuzz_graph_seeded(nae, ctx):
    """the graph step input -> mix(2) -> pitch -> spectrum at drawn ragged lengths, base offsets and strides: nae_graph4_run, the same with the mix
    fuse off, the three nodes one by one and nae_debug_graph4_stages give the same bits, the expected kernels, the oracle's mix and spectrum and
    touch nothing outside their views (tests/test_fuzz_graph_cpu.py pins which edges this seed reaches)"""
    import fuzz_graph
    cases, seed = fuzz_graph.SEEDED
    assert fuzz_graph.main(cases=cases, seed=seed, ctx=ctx, nae=nae) == cases


def test_fuzz_pv_options_seeded(nae, ctx):
    """the vocoder's option space on the scene whose channels and streams have onsets of their own: integer phases bit-exact and samples
    within 1e-4 of the statement in every stream, every stream of a batch equal to its lone run, the handle equal to the block call, nothing
    written outside the destination view, and the kernels of the effective options (tests/test_fuzz_pv_cpu.py pins which edges this seed
    reaches)"""
    import fuzz_pv_options
    cases, seed = fuzz_pv_options.SEEDED
    assert fuzz_pv_options.main(cases=cases, seed=seed, ctx=ctx, nae=nae) == cases
