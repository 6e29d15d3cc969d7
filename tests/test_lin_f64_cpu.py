"""The CPU statements of the FIR filter (K9), the long convolution (K10) and the saturation (K18) against their float64 truths, per
stream-channel as whole-signal RMS, worst block and worst sample (tests/lin_f64.py): the local pin behind the whole-signal 1e-5 / 1e-4 of
tests/test_fir_cpu.py, test_conv_cpu.py and test_sat_cpu.py, which stay.  The GPU tests of these nodes compare bits with the statements, so a
slip the statement and the kernel share (a block edge, the last partition, a tile's halo, a tap row) is seen by a float64 comparison alone,
and a whole-signal figure cannot see anything local.

The matrix: level steps of 60 dB off the block boundaries, a one-block burst and its whole tail, stop-band filters, responses that decay by
100 dB with a ragged last partition, per-channel responses.  CAPS holds one cap per measure and node: 4 times the largest value the statement
reaches over the matrix, rounded up to one significant digit (four is the margin the project asks of its float64 pins, tests/test_conv_cpu.py).
The largest values, the cells that stand out and why: profiles/r29_lin_f64.md.  Then the instrument is shown to bite: planted faults that the
whole-signal bounds pass and a local measure sees at 10 caps or more (a plain gain on K10 at 4: no gain under 1e-5 reaches 10 of its caps,
test_conv_planted_faults); blocks that nothing feeds are exactly 0; and every compute kernel of
kernels_fir.hip, kernels_conv.hip and kernels_sat.hip is named by some case of tests/test_gpu_lin_f64.py."""
import os
import re

import numpy as np
import pytest

import conv_ref
import fir_ref
import lin_f64
import sat_ref
import test_gpu_lin_f64
from conftest import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nodey-audio-editor_amd", "csrc")
CAPS = lin_f64.CAPS
OLD_LIN, OLD_SAT = 1e-5, 1e-4           # RMS_BOUND of tests/test_fir_cpu.py and test_conv_cpu.py; the 1e-4 of tests/test_sat_cpu.py
SOFT, HARD = sat_ref.SOFT, sat_ref.HARD
SAT_SETS = ((SOFT, 4.0, 0.0, 1.0, 0.0), (SOFT, 15.8, 0.3, 0.5, 0.5), (HARD, 4.0, 0.0, 1.0, 0.0), (HARD, 2.0, 0.3, 0.7, 0.3))   # test_sat_cpu.py's
CONV_SHAPES = ((512, 16), (512, 64), (1024, 5), (4096, 3))


@pytest.fixture(scope="module")
def fir(tmp_path_factory):
    return fir_ref.build(str(tmp_path_factory.mktemp("ref_fir_f64")))


@pytest.fixture(scope="module")
def conv(tmp_path_factory):
    return conv_ref.build(str(tmp_path_factory.mktemp("ref_conv_f64")))


@pytest.fixture(scope="module")
def sat(tmp_path_factory):
    return sat_ref.build(str(tmp_path_factory.mktemp("ref_sat_f64")))


def under(m, caps):
    return all(a <= cap for a, cap in zip(m[:3], caps))


def fir_run(fir, h, n_fft, x):
    return fir_ref.run(fir, h, n_fft, x.reshape(-1), x.shape[1]).reshape(x.shape)


def conv_run(conv, h, n_fft, x):
    return conv_ref.run(conv, h, n_fft, x.reshape(-1), x.shape[1]).reshape(x.shape)


def conv_taps(kind, n_fft, P, ch=1, db=100.0):
    """L = P B - 3 taps, so that the last partition is ragged; stereo: a second response for channel 1"""
    L = P * (n_fft // 2) - 3
    seed = 7 + n_fft + P
    return lin_f64.taps(kind, L, seed, db) if ch == 1 else np.stack([lin_f64.taps(kind, L, seed + c, db) for c in range(ch)])


@pytest.mark.parametrize("n_fft", fir_ref.SIZES)
def test_fir_statement_per_block(fir, n_fft):
    """L = 1, 65 and B + 1; uniform taps and, from 65 taps on, the designed 1 kHz low-pass and 8 kHz high-pass (a one-tap design is the
    identity or 0: no stop band); every input kind; in_len = 12 B + 7.  A burst leaves blocks that nothing feeds: they are exactly 0."""
    B = n_fft // 2
    worst = [0.0] * 3
    for L in (1, 65, B + 1):
        for kind in (("uniform",) if L == 1 else ("uniform", "lowpass", "highpass")):
            h = lin_f64.taps(kind, L, 100 + n_fft + L)
            for i, what in enumerate(lin_f64.KINDS):
                x = lin_f64.content(what, 12 * B + 7, 1, B, n_fft + L + i)
                m = lin_f64.channel_measures(fir_run(fir, h, n_fft, x), lin_f64.truth(h, x), h, x, B)[0]
                print(f"LINF64 K9 {n_fft} L {L} {kind} {what}: {m[0]:.3g} {m[1]:.3g} {m[2]:.3g}, {m[3]} silent blocks")
                worst = [max(a, b) for a, b in zip(worst, m)]
                assert under(m, CAPS["K9"]), (L, kind, what, m, CAPS["K9"])
                assert (m[3] >= 9) == (what == "burst"), (L, kind, what, m[3])
    print(f"LINF64 K9 {n_fft} worst (e_rms, e_blk, e_max): {worst}")


@pytest.mark.parametrize("n_fft,P", CONV_SHAPES)
def test_conv_statement_per_block(conv, n_fft, P):
    """L = P B - 3, in_len = (P + 6) B + 7; the response that decays by 100 dB and the uniform one; every input kind; mono, and stereo with
    two responses.  Behind a burst blocks 0 ... P + 1 are fed, the five after them are exactly 0."""
    B = n_fft // 2
    worst = [0.0] * 3
    for kind in ("decay", "uniform"):
        for ch in (1, 2):
            h = conv_taps(kind, n_fft, P, ch)
            for i, what in enumerate(lin_f64.KINDS):
                x = lin_f64.content(what, (P + 6) * B + 7, ch, B, n_fft + P + i)
                for c, m in enumerate(lin_f64.channel_measures(conv_run(conv, h, n_fft, x), lin_f64.truth(h, x, long=True), h, x, B)):
                    print(f"LINF64 K10 {n_fft} P {P} {kind} {what} channel {c} of {ch}: {m[0]:.3g} {m[1]:.3g} {m[2]:.3g}, {m[3]} silent blocks")
                    worst = [max(a, b) for a, b in zip(worst, m)]
                    assert under(m, CAPS["K10"]), (kind, ch, what, m, CAPS["K10"])
                    assert m[3] == (5 if what == "burst" else 0), (kind, ch, what, m[3])
    print(f"LINF64 K10 {n_fft} P {P} worst (e_rms, e_blk, e_max): {worst}")


def sat_inputs(m):
    """6000 stereo samples: noise at amplitude 0.5, and `step` of it"""
    return [(what, lin_f64.content(what, 6000, 2, 256, 10 * m + i, amp=0.5)) for i, what in enumerate(("noise", "step"))]


@pytest.mark.parametrize("m", sat_ref.FACTORS)
def test_sat_statement_per_block(sat, m):
    """the four parameter sets of tests/test_sat_cpu.py (drives up to 15.8); M = 1 is a pointwise map: e_rms and e_max alone, under caps of
    their own"""
    hd = sat_ref.taps(sat, m)
    caps = CAPS["K18"] if m > 1 else (CAPS["K18 map"][0], np.inf, CAPS["K18 map"][1])
    worst = [0.0] * 3
    for curve, drive, bias, wet, dry in SAT_SETS:
        p = sat_ref.params(m, curve, drive, bias, wet, dry)
        for what, x in sat_inputs(m):
            for c, e in enumerate(lin_f64.sat_channel_measures(sat_ref.run(sat, p, x), sat_ref.run_np(p, x, hd))):
                print(f"LINF64 K18 M {m} curve {curve} drive {drive} bias {bias} {what} channel {c}: {e[0]:.3g} {e[1]:.3g} {e[2]:.3g}")
                worst = [max(a, b) for a, b in zip(worst, e)]
                assert under(e, caps), (curve, drive, what, e, caps)
    print(f"LINF64 K18 M {m} worst (e_rms, e_blk, e_max): {worst}")


def test_sat_at_the_largest_drive(sat):
    """drive 251 (48 dB): the curve's slope multiplies the up-sampler's rounding by up to 250, so the caps are not stated there; what the
    statement reaches is recorded (profiles/r29_lin_f64.md) and held to the 1e-4 of tests/test_sat_cpu.py.  Noise at 0.5, which the curve
    flattens almost everywhere, and at 1e-2, which stays on its steep part.  Reached: 1.1e-7 ... 2.8e-7 / 1.5e-7 ... 3.6e-7 / 5.9e-7 ...
    1.7e-6, the figures of the smaller drives: in units of the output's sigma the slope cancels."""
    for m in (2, 4, 8):
        p = sat_ref.params(m, SOFT, 251.0, 0.0, 1.0, 0.0)
        for amp in (0.5, 1e-2):
            x = lin_f64.content("noise", 6000, 2, 256, 40 + m, amp=amp)
            for c, e in enumerate(lin_f64.sat_channel_measures(sat_ref.run(sat, p, x), sat_ref.run_np(p, x, sat_ref.taps(sat, m)))):
                print(f"LINF64 K18 M {m} drive 251 noise at {amp:g} channel {c}: {e[0]:.3g} {e[1]:.3g} {e[2]:.3g}")
                assert e[0] <= OLD_SAT, (m, amp, c, e)


def test_measures_are_what_they_say():
    B = 4
    h = np.array([2.0, 0.0, 0.0, 0.0, 0.0, 1.0])                          # E_h = (4, 1)
    x = np.concatenate([np.zeros(4), [1.0, 1.0, 1.0, 1.0], np.zeros(13)])   # E_x = (0, 4, 0, 0, 0, 0): 21 samples, the last block ragged
    s = lin_f64.block_scale(h, x, B)
    assert s.shape == (6,) and np.array_equal(s, np.sqrt(np.array([0.0, 16.0, 16.0 + 4.0, 4.0, 0.0, 0.0]) / B))
    r = fir_ref.direct(h, x)
    assert not r[:4].any() and not r[16:].any(), "the truth is 0 where the scale is"
    y = r.copy()
    y[5] += 0.5
    y[9] -= 0.5                                                           # block 2, whose scale is sqrt(5): behind block 1 in both
    e_rms, e_blk, e_max, silent = lin_f64.measures(y, r, s, B)
    assert silent == 3 and e_max == 0.5 / 2.0 and e_blk == np.sqrt(0.25 / 4) / 2.0 and abs(e_rms - np.sqrt(0.5 / np.sum(r * r))) < 1e-15
    y = r.copy()
    y[20] = -0.0
    assert lin_f64.measures(y, r, s, B)[:3] == (0.0, 0.0, 0.0), "a zero of either sign"
    y[20] = 1e-30
    with pytest.raises(AssertionError):
        lin_f64.measures(y, r, s, B)                                      # the ragged last block is silent: nothing may stand there
    q = np.tile([2.0, -2.0], 100)
    z = q.copy()
    z[199] += 1.0                                                         # in the ragged last block of 8: it counts as a whole block
    assert lin_f64.sat_measures(z, q) == (np.sqrt(1.0 / 200) / 2, np.sqrt(1.0 / 64) / 2, 0.5)


def test_inputs_are_what_they_say():
    B = 256
    n = 12 * B + 7
    step, burst = lin_f64.content("step", n, 2, B, 3)[:, 1].astype(np.float64), lin_f64.content("burst", n, 2, B, 3)[:, 0]
    rms = lambda v: np.sqrt(np.mean(v * v))
    assert abs(20 * np.log10(rms(step[4 * B + 37:8 * B - 11]) / rms(step[:4 * B + 37])) + 60.0) < 0.5
    assert abs(step[4 * B + 36]) > 0.0011 or abs(step[4 * B + 35]) > 0.0011, "the edge is where it is said to be"
    assert np.abs(step[4 * B + 37:8 * B - 11]).max() <= 1e-3 and rms(step[8 * B - 11:]) > 0.5
    assert not burst[:5].any() and not burst[5 + B:].any() and np.count_nonzero(burst[5:5 + B]) >= B - 1
    a = lin_f64.content("tones", n, 2, B, 3)
    assert np.array_equal(a, lin_f64.content("tones", n, 2, B, 3)) and not np.array_equal(a[:, 0], a[:, 1])
    h = lin_f64.taps("decay", 16 * B - 3, 5).astype(np.float64)
    assert abs(10 * np.log10(np.mean(h[-B:] ** 2) / np.mean(h[:B] ** 2)) + 100.0 * 15 / 16) < 1.5
    lo, hi = (lin_f64.taps(k, 257, 0).astype(np.float64) for k in ("lowpass", "highpass"))
    assert abs(lo.sum() - 1.0) < 1e-6 and abs(hi.sum()) < 1e-6


# ---------------------------------------------------------------------------------------------- planted faults
def verdict(name, old, bound, m, caps, factor=10.0):
    """the two things asked of a planted fault: the whole-signal bound passes it, and a local measure is at 10 caps or more"""
    over = [a / cap for a, cap in zip(m[:3], caps)]
    print(f"LINF64 fault {name}: whole-signal {old:.3g} (bound {bound:g}); (e_rms, e_blk, e_max) in caps {over[0]:.3g} {over[1]:.3g} {over[2]:.3g}")
    assert old <= bound, (name, old)
    assert max(over) >= factor, (name, over)


# The sizes are not all the first guesses (a gain of 1 + 5e-6, a block times 1 + 4e-5, a last sample off by 1e-4 sigma, a tap off by 2^-12):
# a block of a stationary signal sits at S_b / sqrt(2), not at S_b (every tap reaches block b from input block b or from b - 1, and S_b
# counts both), and a cap is up to twice 4 floors after its rounding.  Each size is a round one at which the fault stays under the old
# bound and is at 10 caps; the caps did not move for any of them (profiles/r29_lin_f64.md).
FIR_GAIN = 9.7e-6        # seen in block 0, which input block 0 alone feeds, so that its scale is its level
FIR_BLOCK = 2.5e-5       # one block of 12, a loud one: 7.9e-6 of the whole (4e-5 is 1.3e-5 of it)
FIR_LAST = 4e-4          # in sigma, at B = 2048: 4e-4 / sqrt(2048) = 8.8e-6 of the whole


def test_fir_planted_faults(fir):
    n_fft, B = 512, 256
    h = lin_f64.taps("uniform", 65, 1)
    x = lin_f64.content("noise", 12 * B + 7, 1, B, 2)
    y, r = fir_run(fir, h, n_fft, x).astype(np.float64), lin_f64.truth(h, x)
    assert under(lin_f64.channel_measures(y, r, h, x, B)[0], CAPS["K9"])
    verdict(f"K9 gain 1 + {FIR_GAIN:g}", rel_rms(y * (1 + FIR_GAIN), r), OLD_LIN, lin_f64.channel_measures(y * (1 + FIR_GAIN), r, h, x, B)[0], CAPS["K9"])
    z = y.copy()
    z[5 * B:6 * B] *= 1 + FIR_BLOCK
    verdict(f"K9 block 5 times 1 + {FIR_BLOCK:g}", rel_rms(z, r), OLD_LIN, lin_f64.channel_measures(z, r, h, x, B)[0], CAPS["K9"])
    n_fft, B = 4096, 2048
    h = lin_f64.taps("uniform", B + 1, 3)
    x = lin_f64.content("noise", 12 * B + 7, 1, B, 4)
    y, r = fir_run(fir, h, n_fft, x).astype(np.float64), lin_f64.truth(h, x)
    z = y.copy()
    z[B - 1::B] += FIR_LAST * np.sqrt(np.mean(r * r))
    verdict(f"K9 last sample of every block off by {FIR_LAST:g} sigma", rel_rms(z, r), OLD_LIN, lin_f64.channel_measures(z, r, h, x, B)[0], CAPS["K9"])


CONV_GAIN = 9.5e-6
CONV_GAIN_CAPS = 4.0     # what a gain can reach, see test_conv_planted_faults
CONV_DECAY_DB = 110.0    # at 100 dB the dropped partition is 9.9e-6 of the whole on noise: under 1e-5 by a coincidence


def test_conv_planted_faults(conv):
    """the last partition dropped: the statement is fed taps whose last partition is 0, the truth the whole response.  On noise the loss is
    under the whole-signal 1e-5; behind a one-block burst block 15 loses half of its level and block 16, which that partition alone feeds, all
    of it (0.32 and 0.58 of their scales).
    A gain: the one listed fault that no size brings to 10 caps of K10.  A gain g that the whole-signal 1e-5 passes is below 1e-5, a block is
    off by g times its level, its level is at most its scale on noise, and 10 caps of e_blk are 2e-5: a gain reaches 1e-5 / 2e-6 = 5 caps of
    e_blk at most, whatever its size (here 3.7, and 6.3 caps of e_max in the worst sample, by the draw).  So this one fault is held to 4 caps:
    the local measures see a gain at a quarter of what the whole-signal bound lets through, not at a tenth."""
    n_fft, P, B = 512, 16, 256
    h = conv_taps("decay", n_fft, P, db=CONV_DECAY_DB)
    cut = h.copy()
    cut[(P - 1) * B:] = 0.0
    n = (P + 6) * B + 7
    noise, burst = lin_f64.content("noise", n, 1, B, 5), lin_f64.content("burst", n, 1, B, 6)
    y, r = conv_run(conv, h, n_fft, noise).astype(np.float64), lin_f64.truth(h, noise, long=True)
    assert under(lin_f64.channel_measures(y, r, h, noise, B)[0], CAPS["K10"])
    m = lin_f64.channel_measures(conv_run(conv, cut, n_fft, burst), lin_f64.truth(h, burst, long=True), h, burst, B)[0]
    verdict(f"K10 last of {P} partitions dropped, {CONV_DECAY_DB:g} dB decay", rel_rms(conv_run(conv, cut, n_fft, noise), r), OLD_LIN, m, CAPS["K10"])
    assert m[3] == 5
    verdict(f"K10 gain 1 + {CONV_GAIN:g}", rel_rms(y * (1 + CONV_GAIN), r), OLD_LIN, lin_f64.channel_measures(y * (1 + CONV_GAIN), r, h, noise, B)[0],
            CAPS["K10"], CONV_GAIN_CAPS)


@pytest.mark.parametrize("m", (2, 4, 8))
def test_sat_planted_faults(sat, m):
    """the tap: hd[16 M + 3], three behind the centre, off by 2^-15 M of the largest tap (2^-12 of it at M = 8, 2^-14 at 2: the largest tap
    is near 1 / M, so the same 2^-15 at every factor; 2^-12 at M = 2 and 4 is 2.4e-4 and 1.2e-4 of the whole, over the old bound).  The truth
    alone takes the changed taps"""
    hd = sat_ref.taps(sat, m)
    p = sat_ref.params(m, SOFT, 4.0, 0.0, 1.0, 0.0)
    x = sat_inputs(m)[0][1][:, :1]
    y, r = sat_ref.run(sat, p, x)[:, 0].astype(np.float64), sat_ref.run_np(p, x, hd)[:, 0]
    sigma = np.sqrt(np.mean(r * r))
    assert under(lin_f64.sat_measures(y, r), CAPS["K18"])
    verdict(f"K18 M {m} gain 1 + 5e-5", rel_rms(y * (1 + 5e-5), r), OLD_SAT, lin_f64.sat_measures(y * (1 + 5e-5), r), CAPS["K18"])
    piece = 2048 // m
    z = y.copy()
    z[piece - 1::piece] += 1e-3 * sigma
    verdict(f"K18 M {m} last sample of every piece of {piece} off by 1e-3 sigma", rel_rms(z, r), OLD_SAT, lin_f64.sat_measures(z, r), CAPS["K18"])
    bent = hd.astype(np.float64)
    bent[sat_ref.HALF * m + 3] += 2.0 ** -15 * m * np.abs(bent).max()
    r2 = sat_ref.run_np(p, x, bent)[:, 0]
    verdict(f"K18 M {m} tap {sat_ref.HALF * m + 3} off by 2^-15 M of the largest", rel_rms(y, r2), OLD_SAT, lin_f64.sat_measures(y, r2), CAPS["K18"])


# ---------------------------------------------------------------------------------------------- coverage
WANT = {"fir_block_kernel", "fir_taps_kernel", "conv_taps_kernel", "conv_spectra_kernel", "conv_mac_kernel", "sat_kernel", "sat_map_kernel",
        "sat_map_flat_kernel"}


def test_every_kernel_has_a_case():
    """the __global__ names of the three files, read from the sources, against the kernels the GPU cases name: a new kernel fails here until a
    case measures it"""
    names = set()
    for f in ("kernels_fir.hip", "kernels_conv.hip", "kernels_sat.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            names |= set(re.findall(r"__global__[^;{]*?\bvoid\s+([a-z0-9_]+)\s*\(", fh.read()))
    assert WANT <= names, WANT - names                       # the reader finds the names it is meant to find
    covered = set().union(*(c["kernels"] for c in test_gpu_lin_f64.CASES))
    assert names <= covered, names - covered
    assert covered <= names, covered - names                 # and no case expects a kernel that does not exist
    ids = [c["id"] for c in test_gpu_lin_f64.CASES]
    assert len(set(ids)) == len(ids)
