"""CPU: the cases of tests/test_gpu_batch.py are built without a device, so what they assert on the statement's output is checked here: every
case of the three tables at a few streams (65 for the loudness meter, whose condition speaks of 64 streams in a row), the echo's grouping case
as it stands; and the conditions and the batch message catch what they are there to catch."""
import numpy as np
import pytest

import test_gpu_batch as tb
from block_gpu import bits, each_stream, mismatch

FEW = 3


def streams_of(name):
    return 65 if name.startswith("loud") else FEW


@pytest.mark.parametrize("name", sorted(tb.WORKLOAD_CASES))
def test_workload_cases_hold_their_conditions(name):
    case = tb.build(tb.WORKLOAD_CASES, name, streams_of(name))
    assert len(case.x) == streams_of(name) and (case.want is None or case.want.shape == case.x.shape)


@pytest.mark.parametrize("name", sorted(tb.OVERFULL_CASES))
def test_overfull_cases_hold_their_conditions(name):
    case = tb.build(tb.OVERFULL_CASES, name, streams_of(name))
    assert len(case.x) == streams_of(name)


@pytest.mark.parametrize("name", sorted(tb.ECHO_CASES))
def test_echo_cases_hear_their_repeat(name):
    case = tb.echo_case(FEW, *tb.ECHO_CASES[name])
    assert case.x.shape[1] == 3 * (3072 if 1500 in tb.ECHO_CASES[name][0] else 2048) + 7


def test_the_grouping_case_exceeds_one_group():
    case = tb.grouping_case()
    assert case.x.shape == (600, 2 * 1024 + 7, 2) and np.array_equal(case.want, tb.dry_only(case.params, case.x))


def test_the_batches_are_what_the_reasoning_says():
    assert tb.WORKLOAD == 1024 and 2 * tb.OVERFULL > 256 * 32 and all(tb.OVERFULL % k for k in range(2, 65))


def test_the_conditions_catch_a_case_that_tests_nothing():
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (3, 4000, 2)).astype(np.float32)
    moved = x.copy()
    moved[:, ::2] *= np.float32(0.5)
    tb.assert_the_gain_moves(moved, x)
    moved[1, 10:] = x[1, 10:]
    with pytest.raises(AssertionError, match="stream 1"):
        tb.assert_the_gain_moves(moved, x)

    p = tb.echo_ref.params((1024, 1500), 0.5, 1, 0.6, 0.8)
    dry = tb.dry_only(p, x)
    heard = dry.copy()
    heard[:, 1024, 0] += np.float32(0.25)
    tb.assert_the_repeat_is_there(heard, x, p)
    heard[2] = dry[2]
    heard[2, 1023, 0] += np.float32(0.25)                   # in front of the delay: no repeat
    with pytest.raises(AssertionError, match=r"\[2\]"):
        tb.assert_the_repeat_is_there(heard, x, p)

    half = x * np.float32(0.55)
    tb.assert_the_gate_works(half, x, 0.1)
    for dead in (x * np.float32(0.1), x.copy()):
        half[0] = dead[0]
        with pytest.raises(AssertionError, match=r"\[0\]"):
            tb.assert_the_gate_works(half, x, 0.1)

    record = lambda g: tb.loud_ref.Result(gain_f32=g)
    tb.assert_the_gains_differ([record(1.0 + (s % 64)) for s in range(130)])
    with pytest.raises(AssertionError, match="not all equal"):
        tb.assert_the_gains_differ([record(2.0)] * 130)
    with pytest.raises(AssertionError, match="within streams 64"):
        tb.assert_the_gains_differ([record(1.0 + s) for s in range(64)] + [record(3.0)] * 64)


def test_the_batch_message_names_streams_and_channels():
    want = np.zeros((40, 50, 2), np.float32)
    assert mismatch(want.copy(), want) == ""
    got = want.copy()
    got[7, 30:, 1] = 1.0
    got[33, 5, 0] = -0.0                                     # another bit pattern of the same value
    message = mismatch(got, want)
    assert message.startswith("2 of 40 streams differ (2 stream-channels)") and "(7, 1, 30, 20), (33, 0, 5, 1)" in message
    got[:, 0, :] = 1.0
    assert mismatch(got, want).startswith("40 of 40 streams differ (80 stream-channels)") and mismatch(got, want).count("(") == 2 + 8


def test_each_stream_keeps_the_order_on_its_threads():
    out = each_stream(lambda i: np.full(3, i), 100)
    assert out.shape == (100, 3) and np.array_equal(out[:, 0], np.arange(100))
    assert np.array_equal(bits(each_stream(lambda i: np.float32([i]), 5)), bits(np.arange(5, dtype=np.float32)[:, None]))
