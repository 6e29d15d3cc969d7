"""No GPU: what tests/tools/fuzz_pv_options.py draws at the seed tests/test_gpu_fuzz.py runs.  The generator needs the static plans
(nae_stretch_plan_make*) and the CPU statement (tests/pv_ref/ref_pv.c) alone.  Within the cases the GPU test runs, every frame size, the lock
with and without transient preservation, transient preservation unlinked stereo, linked stereo and mono, each plan case A ... D of the formant
shift, both stage orders and no transposer, every pv_tile, a transient batch of at least three streams, both layouts on both sides and a
misaligned base occur (a seed that loses one is changed, not the assertion); and the statement alone meets what the GPU run relies on: onsets
in one channel only, streams of a batch with different onsets, onsets on a tile's first, second and last frame."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import fuzz_pv_options as fz


@pytest.fixture(scope="module")
def run():
    cases, seed = fz.SEEDED
    assert 20 <= cases <= 32
    return list(fz.draw(cases, seed))


@pytest.fixture(scope="module")
def onsets(run):
    """per record, per stream, the verdicts [frames, ch] the call acts on; None where the transient flag is not effective"""
    return [fz.onset_sets(c) for c in run]


def test_the_draw_is_the_seeds_alone(run):
    again = list(fz.draw(len(run), fz.SEEDED[1]))
    assert again == run
    assert np.array_equal(fz.signals(run[0]), fz.signals(again[0]))
    other = dict(run[0], sub=run[0]["sub"] + 1)
    assert not np.array_equal(fz.signals(run[0]), fz.signals(other))
    if run[0]["n_streams"] > 1:
        x = fz.signals(run[0])
        assert not np.array_equal(x[0], x[1])


def test_every_record_stays_small_and_inside_its_buffers(run):
    for c in run:
        pl, pn = fz.plans(c)
        T = int(pl.out_len)
        assert 1 <= c["n_streams"] <= 5 and T > 0, fz.describe(c)
        assert c["n_streams"] * max(c["L"], T) * c["ch"] <= fz.MAX_SAMPLES, fz.describe(c)
        if pl.pv_on:
            assert fz.FRAMES[0] <= pl.frames <= fz.FRAMES[1] + 8, (pl.frames, fz.describe(c))     # + the frames of the N samples behind
        assert 512 <= c["n_fft"] <= 4096 and (not c["lock"] or c["n_fft"] == 1024) and 0 <= c["lifter"] <= c["n_fft"] // 4
        tempo, rho = 1 / c["pitch"], c["rate"] * c["pitch"]
        assert 0.3 * 0.999 <= tempo <= 8 * 1.001 and 0.5 * 0.999 <= rho <= 2.5 * 1.001, fz.describe(c)
        for key, S in (("src", c["L"]), ("dst", T)):
            idx, _, size = fz.view(c["n_streams"], S, c["ch"], c[key])
            assert idx.min() >= 0 and idx.max() < size
            assert np.unique(idx).size == idx.size, (key, fz.describe(c))       # a view never maps two elements to one word
        assert sum(fz.put_sizes(c)) > 0 and min(fz.put_sizes(c)) >= 1


def test_a_class_reaches_what_it_is_meant_for(run):
    for c in run:
        eff, kind = fz.resolve(c), c["label"]
        if kind.startswith("tr-") or kind == "lock-tr":
            assert eff["transients"], fz.describe(c)
        if kind in ("lock", "lock-tr"):
            assert c["lock"] and eff["stage"] and eff["transients"] == (kind == "lock-tr"), fz.describe(c)
        if kind == "tr-stereo":
            assert c["ch"] == 2 and not c["link"]
        if kind == "tr-link":
            assert eff["link"] and fz.expected_kernels(c)[0].endswith("link_kernel")
        if kind == "tr-mono":
            assert c["ch"] == 1 and not eff["link"]
        if kind == "tr-batch":
            assert c["n_streams"] >= 3
        if kind.startswith("shift-"):
            assert fz.plan_case(c) == kind[-1] and c["lifter"] > 0, fz.describe(c)
            assert eff["forced"] == (kind[-1] in "CD") and (eff["lifter"] > 0), fz.describe(c)
        if kind in ("shift-C", "shift-D", "no-pv"):
            assert not (eff["transients"] or eff["link"] or fz.expected_kernels(c)), fz.describe(c)
        if kind == "no-pv":
            assert not fz.plans(c)[0].pv_on


def test_the_seeded_run_reaches_every_edge(run):
    eff = [fz.resolve(c) for c in run]
    assert {c["n_fft"] for c in run} == set(fz.SIZES), "every frame size"
    assert {c["n_fft"] for c, e in zip(run, eff) if e["transients"]} == set(fz.SIZES), "... with transient preservation effective"
    assert {e["transients"] for c, e in zip(run, eff) if c["lock"] and e["stage"]} == {False, True}, "locked with and without transients"
    tr = [(c, e) for c, e in zip(run, eff) if e["transients"]]
    assert any(c["ch"] == 2 and not e["link"] for c, e in tr), "transients unlinked stereo"
    assert any(e["link"] for c, e in tr) and any(c["ch"] == 1 for c, e in tr), "transients linked stereo and mono"
    assert any(e["link"] and c["lock"] for c, e in zip(run, eff)), "the lock linked"
    assert {fz.plan_case(c) for c in run} >= {"A", "B", "C", "D"}, "each plan case of the formant shift"
    orders = {(int(fz.plans(c)[0].rs_on), int(fz.plans(c)[0].rs_first)) for c, e in zip(run, eff) if e["stage"]}
    assert orders == {(0, 0), (1, 0), (1, 1)}, "no transposer, the transposer behind the vocoder and in front of it"
    assert {(int(fz.plans(c)[0].rs_on), int(fz.plans(c)[0].rs_first)) for c, e in tr} == orders, "... with transient preservation effective"
    assert {c["pv_tile"] for c in run} == set(fz.TILES), "every pv_tile"
    assert {c["pv_tile"] for c, e in tr} >= {1, 16, 64}, "... one frame, 16 and 64 with transient preservation"
    assert any(c["n_streams"] >= 3 for c, e in tr), "a transient batch of at least 3 streams"
    assert any(e["stage"] and c["n_streams"] >= 2 and c["pv_tile"] in (0, 64) and fz.plans(c)[0].frames <= 64 for c, e in zip(run, eff)), \
        "a batch whose phases are asked in a single tile, after its block call has used the phase workspace"
    assert {c["src"]["planar"] for c in run} == {False, True} and {c["dst"]["planar"] for c in run} == {False, True}, "both layouts on both sides"
    assert any(c["src"]["base"] for c in run) and any(c["dst"]["base"] for c in run) and any(not c["dst"]["base"] for c in run), "a misaligned base"
    assert {c["puts"] for c in run} == set(fz.PUTS), "every put pattern"
    assert {bool(e["lifter"]) for c, e in tr} == {False, True}, "transients with and without the envelope stage"
    assert any(c["link"] and not e["link"] for c, e in zip(run, eff)) and any(c["transients"] and not e["transients"] for c, e in zip(run, eff)), \
        "flags that are set and not effective"
    assert {c["ch"] for c in run} == {1, 2} and {c["n_streams"] for c in run} >= {1, 2, 3}


def test_the_statement_meets_what_the_gpu_run_relies_on(run, onsets):
    places = set()
    for c, on in zip(run, onsets):
        eff = fz.resolve(c)
        assert (on is not None) == eff["transients"], fz.describe(c)
        if on is None:
            continue
        assert fz.conditions(c, on), fz.describe(c)
        assert all(o.any() for o in on), f"{fz.describe(c)}: a stream without an onset"
        assert len({o.tobytes() for o in on}) == len(on), f"{fz.describe(c)}: two streams with the same onsets"
        if c["ch"] == 2 and not eff["link"]:
            for s, o in enumerate(on):
                assert (o[:, 0] & ~o[:, 1]).any() and (o[:, 1] & ~o[:, 0]).any(), f"{fz.describe(c)}: stream {s} has no onset in one channel only"
        if c["ch"] == 2 and eff["link"]:
            assert all(np.array_equal(o[:, 0], o[:, 1]) for o in on), fz.describe(c)
        for o in on:
            places |= set(np.nonzero(o.any(1))[0] % 16)
    assert {0, 1, 15} <= places, f"onsets on the first, second and last frame of a 16-frame tile: {sorted(places)}"
