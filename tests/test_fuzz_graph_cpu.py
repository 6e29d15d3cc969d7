"""No GPU: what tests/tools/fuzz_graph.py draws at the seed tests/test_gpu_fuzz.py runs, and what the named rows of tests/graph_cases.py claim.
The route rule (fuzz_graph.expected_route) needs nae_stretch_plan_make alone, which is static.  Within the cases the GPU test runs, the fused
kernel meets every length residue mod 4, every occupancy of its four-stream group, both tiles and both mix layouts, every reason to refuse the
fuse occurs, and so does the tiny class (a seed that loses one is changed, not the assertion); every named row takes the route its entry claims
and the tile-edge rows have the mid_len they claim."""
import numpy as np
import pytest

import graph_cases
import fuzz_graph

FUSED = ("mix_resample_tile_kernel",)


@pytest.fixture(scope="module")
def run():
    cases, seed = fuzz_graph.SEEDED
    assert 20 <= cases <= 32
    return list(fuzz_graph.draw(cases, seed))


def fused(nae, cases):
    return [c for c in cases if fuzz_graph.expected_route(nae, c) == FUSED]


def test_the_draw_is_the_seeds_alone(nae, run):
    again = list(fuzz_graph.draw(len(run), fuzz_graph.SEEDED[1]))
    assert again == run
    g = fuzz_graph.geometry(nae, run[0])
    assert all(np.array_equal(x, y) for x, y in zip(fuzz_graph.signals(run[0], g), fuzz_graph.signals(again[0], g)))


def test_every_record_stays_small_and_inside_its_buffers(nae, run):
    for c in run:
        assert 1 <= c["S"] <= 6000 and 1 <= c["n_streams"] <= 7, fuzz_graph.describe(c)
        g = fuzz_graph.geometry(nae, c)
        for key in ("a", "b", "mix", "pitch", "spec"):
            assert g[key].size == 0 or (g[key].min() >= 0 and g[key].max() < g["n_" + key])
        for key in ("mix", "pitch", "spec"):                     # a destination view never maps two elements to one word
            assert np.unique(g[key]).size == g[key].size, (key, fuzz_graph.describe(c))


def test_a_class_meant_for_the_fused_kernel_reaches_it(nae, run):
    for c in run:
        route, why = fuzz_graph.expected_route(nae, c), fuzz_graph.refusals(nae, c)
        if c["label"] in ("fused", "tiny"):
            assert why in ([], ["empty"]) and (route == FUSED) == (why == []), fuzz_graph.describe(c)
        elif c["label"] in fuzz_graph.REASONS:
            assert why == [c["label"]] and "resample_tile_kernel" in route and FUSED[0] not in route, (why, fuzz_graph.describe(c))
        else:
            assert not fuzz_graph.plan_of(nae, c).rs_first and len(route) == 1, fuzz_graph.describe(c)


def test_the_seeded_run_reaches_every_edge(nae, run):
    on = fused(nae, run)
    assert {c["S"] % 4 for c in on if c["S"] > 29} == {0, 1, 2, 3}, "every length residue on the fused route"
    assert {c["n_streams"] % 4 for c in on} == {0, 1, 2, 3}, "every occupancy of the last four-stream group"
    assert {c["n_streams"] % 4 for c in on if c["S"] % 4} == {0, 1, 2, 3}, "... at a ragged length"
    assert {fuzz_graph.tile_rule(fuzz_graph.plan_of(nae, c).step_q32)[0] for c in on if c["S"] % 4} == {fuzz_graph.TILE, fuzz_graph.TILE_WIDE}, "both tiles"
    assert {c["mix"]["fs"] for c in on if c["S"] % 4} == {1, 2}, "both mix layouts"
    assert any(c["b"]["ss"] == 0 for c in on) and any(c["b"]["ss"] for c in on), "in_b shared and per stream"
    assert any(fuzz_graph.plan_of(nae, c).mid_len > 2 * fuzz_graph.TILE_WIDE for c in on), "more than two tiles"
    assert any(c["rate"] != 1.0 for c in on), "a rate other than 1 with the transposer first"
    why = {r for c in run for r in fuzz_graph.refusals(nae, c)}
    assert why >= set(fuzz_graph.REASONS), "every reason to refuse the fuse"
    assert any(c["label"] == "rho" for c in run) and any(c["pitch"] == 1508 / 512 for c in on), "both sides of the fuse limit"
    assert sum(c["S"] in fuzz_graph.TINY for c in run) >= 2, "the tiny class"
    routes = {k for c in run for k in fuzz_graph.expected_route(nae, c)}
    assert routes >= {"mix_resample_tile_kernel", "amix_i2p_kernel", "amix_generic_kernel", "resample_tile_kernel"}, routes
    assert any(c["pitch_out"]["base"] == 2 for c in run) and any(c["pitch_out"]["base"] == 0 for c in run), "the pitch output aligned and 8 bytes off"
    assert any(c["spec_gap"] for c in run), "a gap between the spectrum's streams"


# ------------------------------------------------------------------------------------------------ the named rows
@pytest.mark.parametrize("name,route,mid_len,case", graph_cases.NAMED, ids=[r[0] for r in graph_cases.NAMED])
def test_named_row_takes_the_route_it_claims(nae, name, route, mid_len, case):
    assert case["S"] <= 20000 and case["n_streams"] <= 9
    assert fuzz_graph.expected_route(nae, case) == graph_cases.ROUTES[route], (fuzz_graph.refusals(nae, case), fuzz_graph.describe(case))
    if mid_len is not None:
        assert fuzz_graph.plan_of(nae, case).mid_len == mid_len
    if name.startswith("fallback-"):
        why = fuzz_graph.refusals(nae, case)
        assert len(why) == 1 and fuzz_graph.plan_of(nae, case).rs_first, why


def test_named_rows_cover_what_they_are_there_for(nae):
    rows = {name: (route, case) for name, route, _, case in graph_cases.NAMED}
    assert len(rows) == len(graph_cases.NAMED), "row names are unique"
    on = [c for route, c in rows.values() if route == "fused"]
    for planar in (1, 2):
        assert {c["S"] % 4 for c in on if c["mix"]["fs"] == planar and c["S"] > 29} >= {1, 2, 3}
    assert {c["n_streams"] for c in on if c["S"] % 4} >= {1, 2, 3, 4, 5, 7}
    tile = lambda name: fuzz_graph.tile_rule(fuzz_graph.plan_of(nae, rows[name][1]).step_q32)
    assert all(tile(f"tile-768{e}")[0] == 768 and tile(f"tile-512{e}")[0] == 512 for e in ("-minus-1", "", "-plus-1", "-twice"))
    assert tile("rho-1508-768-last-wide-tile") == (768, 1536) and tile("rho-1509-768-first-narrow-tile")[0] == 512
    assert tile("rho-1508-512-last-fused") == (512, 1536) and tile("rho-1509-512-first-unfused") == (512, 1537)
    why = {r for name, (_, c) in rows.items() if name.startswith("fallback-") for r in fuzz_graph.refusals(nae, c)}
    assert why >= {"a_base", "b_base", "a_stride", "mix_stride", "mix_plane", "mix_base", "rho"}, why
    # the fallbacks carry the signals of their fused sibling
    sib = rows["ragged-3001-planar-5-streams"][1]
    xs = fuzz_graph.signals(sib, fuzz_graph.geometry(nae, sib))
    ga = fuzz_graph.geometry(nae, sib)
    for name in ("fallback-in-a-base-1-float-off", "fallback-odd-plane-stride", "pitch-out-8-bytes-off"):
        c = rows[name][1]
        g = fuzz_graph.geometry(nae, c)
        ys = fuzz_graph.signals(c, g)
        assert np.array_equal(xs[0][ga["a"]], ys[0][g["a"]]) and np.array_equal(xs[1][ga["b"]], ys[1][g["b"]]), name
    for name, case in graph_cases.MANY_STREAMS:
        assert case["n_streams"] > fuzz_graph.PER_LAUNCH and fuzz_graph.expected_route(nae, case) == FUSED, name
