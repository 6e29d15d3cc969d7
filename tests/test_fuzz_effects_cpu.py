"""No GPU: what the generators of tests/tools/fuzz_effects.py draw at the seeds tests/test_gpu_fuzz.py runs.  Every record of 300 draws passes
its statement's own check; within the cases the GPU test runs the named edges occur (a seed that loses one is changed, not the assertion), the
statement's output is finite (bit equality then never compares NaN payloads) and, for the spectral gate, between 20 % and 80 % of the
statement's decisions are open."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import denoise_ref
import echo_ref
import fuzz_effects
import mod_ref
from block_gpu import statement

DRAWS = 300


@pytest.fixture(scope="module", params=fuzz_effects.NODES)
def drawn(request):
    """(node, the statement, the 300 records, the records the GPU test runs)"""
    node = request.param
    cases, seed = fuzz_effects.SEEDED[node]
    records = list(fuzz_effects.draw(node, DRAWS, seed))
    assert 0 < cases <= DRAWS
    return node, statement(fuzz_effects.REFS[node]), records, records[:cases]


def test_every_record_passes_the_statements_check(drawn):
    node, L, records, _ = drawn
    for k, case in enumerate(records):
        assert fuzz_effects.check(case, L) == 0, (k, fuzz_effects.describe(case))
        assert case["ch"] in (1, 2) and 1 <= case["n_streams"] <= 12 and case["in_len"] >= 1
        assert case["n_streams"] == 1 or case["n_streams"] * case["in_len"] * case["ch"] <= fuzz_effects.MAX_FLOATS
        assert 1 <= len(case["puts"]) <= 5 and all(1 <= p <= 6 * case["unit"] for p in case["puts"])


def test_the_draw_is_the_seeds_alone(drawn):
    node, _, records, _ = drawn
    again = list(fuzz_effects.draw(node, 12, fuzz_effects.SEEDED[node][1]))
    assert [fuzz_effects.describe(c) for c in again] == [fuzz_effects.describe(c) for c in records[:12]]
    assert all(np.array_equal(fuzz_effects.signals(a)["x"], fuzz_effects.signals(b)["x"]) for a, b in zip(again[:3], records[:3]))


def test_common_edges(drawn):
    _, _, _, run = drawn
    assert {c["ch"] for c in run} == {1, 2}, "both channel counts"
    assert any(c["shared"] and not c["handle"] and c["n_streams"] > 1 for c in run), "a shared source under several streams"
    assert any(c["handle"] for c in run) and any(not c["handle"] for c in run), "the handle and the block entry"
    assert any(c["in_len"] == 1 for c in run), "a length of 1"
    assert any(c["in_len"] % c["unit"] == 0 for c in run), "a length on a unit boundary"
    assert {c["src"] for c in run} == {"i", "p"} and {c["dst"] for c in run} == {"i", "p"}


def test_node_edges(drawn):
    node, _, _, run = drawn
    if node == "mod":
        runs = {mod_ref.sub_block(c["p"]) for c in run if c["p"].feedback != 0.0}
        assert 1 in runs and 64 in runs and len(runs - {1, 64}) >= 8, sorted(runs)
        assert any(c["p"].feedback == 0.0 for c in run) and any(c["p"].feedback != 0.0 for c in run)
        assert any(c["p"].delay + c["p"].depth == mod_ref.MAX_DELAY for c in run), "the reach to the ring's limit"
    if node == "echo":
        assert any(c["p"].delay[0] % echo_ref.CHUNK == 0 for c in run) and any(c["p"].delay[0] % echo_ref.CHUNK for c in run)
        assert any(c["ch"] == 2 and c["p"].cross and c["p"].delay[0] != c["p"].delay[1] for c in run), "unequal channels with cross"
        assert any(c["in_len"] > 2 * echo_ref.ring(c["p"], c["ch"]) for c in run), "a length past 2 R"
        longest = run[fuzz_effects.ECHO_LONGEST_AT]
        assert longest["p"].delay[0] == echo_ref.MAX_DELAY and (longest["ch"], longest["in_len"]) == (1, echo_ref.MAX_DELAY + 1025)
    if node in ("dyn", "dynkey"):
        dyn = [c["p"].dyn if node == "dynkey" else c["p"] for c in run]
        assert {0, 1024} <= {p.lookahead for p in dyn}, "look-ahead 0 and 1024"
        assert any(c["limiter"] and p.slope == 1.0 for c, p in zip(run, dyn)), "ratio infinity"
    if node == "dynkey":
        assert {c["p"].key_ch for c in run} == {0, 1, 2}
    if node == "eq":
        assert {1, 16} <= {c["coef"].shape[0] for c in run}, "1 and 16 sections"
    if node == "conv":
        assert any(c["parts"] == 1 for c in run) and any(c["parts"] >= 8 for c in run)
        blocks = lambda c: -(-c["in_len"] // c["unit"])
        assert any(c["debug"]["conv_ring"] > 0 and blocks(c) > max(c["debug"]["conv_ring"], c["parts"]) for c in run), "a wrapped ring"
    if node == "denoise":
        assert {0, denoise_ref.MAX_TIME} <= {c["p"].time_smooth for c in run} and {0, denoise_ref.MAX_FREQ} <= {c["p"].freq_smooth for c in run}
    if node == "loud":
        assert any(c["in_len"] < 4 * c["unit"] for c in run), "shorter than one gating block"
        assert any(c["in_len"] // c["unit"] - 3 >= 6 for c in run), "at least six gating blocks"


def test_a_gaining_echo_loop_is_cut_before_it_overflows():
    """300 draws at seed 7: before the generator cut the lengths of loops that gain, case 179 (delays 60127 and 1024, feedback -0.94 through a
    boosting section, 61447 frames: 60 repeats on the second channel) overflowed f32 in the statement and on the GPU alike, and bit equality
    compared NaN payloads.  Such records are still drawn, and every statement output is finite"""
    L = statement(echo_ref)
    gaining = 0
    for k, case in enumerate(fuzz_effects.draw("echo", DRAWS, 7)):
        p = case["p"]
        gaining += fuzz_effects.echo_loop_db(echo_ref.coef_of(p), p.feedback) > 0.0
        assert np.isfinite(fuzz_effects.want(case, fuzz_effects.signals(case), L)).all(), (k, fuzz_effects.describe(case))
    assert gaining >= 10, gaining


def test_statement_output_is_finite(drawn):
    node, L, _, run = drawn
    opened = total = 0
    for k, case in enumerate(run):
        sig = fuzz_effects.signals(case)
        out = fuzz_effects.want(case, sig, L)
        if node == "loud":
            out, records = out
            assert all(np.isfinite([r.mean2, r.momentary_max, r.gain, r.gain_f32]).all() for r in records), k
        assert np.isfinite(sig["x"]).all() and np.isfinite(out).all(), (k, fuzz_effects.describe(case))
        if node == "denoise":
            for s in sig["x"]:
                d = denoise_ref.run(L, case["p"], sig["profile"], s, detail=True)[1]
                opened, total = opened + int(d.sum()), total + d.size
    if node == "denoise":
        assert 0.2 <= opened / total <= 0.8, f"between a fifth and four fifths of the decisions are open: {opened / total:.3f}"
