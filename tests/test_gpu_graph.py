"""GPU: the graph step input -> mix(2) -> pitch -> spectrum (nae_graph4_run) at the named edges of tests/graph_cases.py: a ragged end on the
fused mix + transposer (mix_resample_tile_kernel) in both mix layouts and at every occupancy of its four-stream group, the tile and ratio
edges, tiny and empty signals, every reason the fuse is refused, the volumes, the pitch output's alignments.  Every row runs four ways
(the graph, the graph with the fuse switched off, the three nodes one by one, nae_debug_graph4_stages with masks 1, 2, 4) into buffers filled
with a sentinel; tests/tools/fuzz_graph.run_case asserts the route, the mix and the spectrum bit-exact against the oracle, the pitch within
1e-4 of it, the four runs bit-identical and the sentinel everywhere outside the views.  Measured on an MI355X: pitch errors of 1.4e-7 ... 2.1e-7
on the rows of 900 frames and more; 1.8e-6 ... 5.2e-5 on the tiny rows, whose outputs sit on the window's edge and are measured against the floor
of 1e-4 under the denominator (fuzz_graph.signals says for which amplitude)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import graph_cases
import fuzz_graph

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,case", [(r[1], r[3]) for r in graph_cases.NAMED], ids=[r[0] for r in graph_cases.NAMED])
def test_graph4_splits_agree_at_the_edge(ctx, nae, route, case):
    assert fuzz_graph.expected_route(nae, case) == graph_cases.ROUTES[route]
    assert fuzz_graph.run_case(nae, ctx, case) <= fuzz_graph.TOL


@pytest.mark.parametrize("case", [c for _, c in graph_cases.MANY_STREAMS], ids=[n for n, _ in graph_cases.MANY_STREAMS])
def test_graph4_front_stage_with_more_streams_than_one_launch_indexes(ctx, nae, case):
    """65535 * 4 + 3 streams of 8 frames through the fused kernel: its second launch starts at stream 262140 of every view"""
    fuzz_graph.run_front_only(nae, ctx, case)
