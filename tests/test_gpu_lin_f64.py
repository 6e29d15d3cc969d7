"""The FIR filter (K9), the long convolution (K10) and the saturation (K18) on the GPU against their float64 truths directly, per
stream-channel, per block and per sample (tests/lin_f64.py), under the caps the CPU statements are held to (lin_f64.CAPS,
tests/test_lin_f64_cpu.py).  The other GPU tests of these nodes compare bits with the CPU statements, which are the tiled forms the kernels
compute: this comparison stands even where a statement and its kernel share a slip.

Every case of CASES names the kernels it must launch (tests/test_lin_f64_cpu.py asserts that every compute kernel of kernels_fir.hip,
kernels_conv.hip and kernels_sat.hip is some case's), runs three streams of different contents on a context of its own (so that the tap
spectra are computed in the case), and asserts
  * that the kernels were launched,
  * that every stream-channel is under the caps against the float64 truth, and exactly 0 in the blocks that nothing feeds,
  * the statement's bits (block_gpu.mismatch): the nodes are specified bit for bit, and no GPU test has fed them level steps, bursts with
    their tails, stop-band filters or responses that decay by 100 dB before.
The streaming handles take one put pattern each (1, B - 1, 2 B + 1 frames and the rest): the carry across puts is where a halo slip would
live.  One line per stream-channel is printed (LINF64 ...); the measured values: profiles/r29_lin_f64.md."""
import numpy as np
import pytest

import conv_ref
import fir_ref
import lin_f64
import sat_ref
from block_gpu import mismatch, statement
from conv_gpu import conv_stream, gpu_conv
from fir_gpu import fir_stream, gpu_fir
from pv_gpu import profiled
from sat_gpu import gpu_sat, sat_stream

pytestmark = pytest.mark.gpu

N_STREAMS = 3
CAPS = lin_f64.CAPS
SOFT, HARD = sat_ref.SOFT, sat_ref.HARD
SAT_SETS = {SOFT: (SOFT, 15.8, 0.3, 0.5, 0.5), HARD: (HARD, 2.0, 0.3, 0.7, 0.3)}     # two of the CPU matrix's sets, both with a bias and a dry path
SAT_LEN, SAT_B = 3 * 1024 + 5, 256
FIR_KERNELS = ("fir_block_kernel", "fir_taps_kernel")
CONV_KERNELS = ("conv_taps_kernel", "conv_spectra_kernel", "conv_mac_kernel")
CASES = []


def case(node, kernels, tag, keys=None, **opts):
    c = dict(node=node, kernels=tuple(kernels), keys=dict(keys or {}), **opts)
    c["id"] = f"{node}-{tag}" + "".join(f"-{k}{v}" for k, v in c["keys"].items())
    CASES.append(c)


for n_fft in (512, 4096):
    for what in ("step", "burst"):
        for taps in ("highpass", "uniform"):
            for layout in ("i", "p"):
                for tile in (0, 1, 3):
                    case("K9", FIR_KERNELS, f"{n_fft}-{what}-{taps}-{layout}", {"fir_tile": tile}, n_fft=n_fft, what=what, taps=taps, layout=layout, ch=2)
for n_fft, P, taps, inputs in ((512, 16, "decay", ("burst", "step")), (4096, 3, "uniform", ("step",))):
    for what in inputs:
        for ch in (1, 2):
            for tile in (0, 1):
                for ring in (P + 1, P + 3):
                    case("K10", CONV_KERNELS, f"{n_fft}x{P}-{what}-{taps}-ch{ch}", {"conv_tile": tile, "conv_ring": ring}, n_fft=n_fft, P=P, what=what,
                         taps=taps, ch=ch)
for m in (2, 4, 8):
    for curve in (SOFT, HARD):
        for tile in (1, 0):
            case("K18", ("sat_kernel",), f"M{m}-{('soft', 'hard')[curve]}", {"sat_tile": tile}, m=m, curve=curve, view={})
for curve in (SOFT, HARD):
    # M = 1: a base one float past the allocation's start takes the general map; 16-byte aligned bases and stream strides of 6156 and 6172
    # floats (multiples of 4) take the flat one
    case("K18", ("sat_map_kernel",), f"M1-{('soft', 'hard')[curve]}-unaligned", m=1, curve=curve, view=dict(offset=1))
    case("K18", ("sat_map_flat_kernel",), f"M1-{('soft', 'hard')[curve]}-aligned", m=1, curve=curve, view=dict(gap=2, chan_pad=1))
case("K9", FIR_KERNELS, "handle-512-burst-uniform", n_fft=512, what="burst", taps="uniform", ch=2, handle=True)
case("K10", CONV_KERNELS, "handle-512x16-burst-decay-ch2", n_fft=512, P=16, what="burst", taps="decay", ch=2, handle=True)
case("K18", ("sat_kernel",), "handle-M4-soft", m=4, curve=SOFT, handle=True)

_refs = {}


def lin_reference(c):
    """(taps, x[streams, n, ch], the statement's output, the float64 truth, the scales [streams][ch]) of a K9 or K10 case: shared by the cases
    that differ in view and debug keys alone.  A handle delivers the statement on the input extended by L - 1 zero frames."""
    fir = c["node"] == "K9"
    key = (c["node"], c["n_fft"], c.get("P"), c["what"], c["taps"], c["ch"], bool(c.get("handle")))
    if key not in _refs:
        B = c["n_fft"] // 2
        if fir:
            L, n = B + 1, 12 * B + 7
            h = lin_f64.taps(c["taps"], L, 31 + c["n_fft"])
        else:
            L, n = c["P"] * B - 3, (c["P"] + 6) * B + 7
            h = lin_f64.taps(c["taps"], L, 41) if c["ch"] == 1 else np.stack([lin_f64.taps(c["taps"], L, 41 + k) for k in range(c["ch"])])
        x = np.stack([lin_f64.content(c["what"], n, c["ch"], B, 100 + 7 * s + c["n_fft"]) for s in range(N_STREAMS)])
        if c.get("handle"):
            x = np.concatenate([x, np.zeros((N_STREAMS, L - 1, c["ch"]), np.float32)], axis=1)
        ref = statement(fir_ref if fir else conv_ref)
        want = np.stack([(fir_ref if fir else conv_ref).run(ref, h, c["n_fft"], s.reshape(-1), c["ch"]).reshape(s.shape) for s in x])
        r = np.stack([lin_f64.truth(h, s, long=not fir) for s in x])
        for a in (x, want, r):
            a.setflags(write=False)
        _refs[key] = (h, x, want, r)
    return _refs[key]


def sat_reference(c):
    key = ("K18", c["m"], c["curve"], bool(c.get("handle")))
    if key not in _refs:
        p = sat_ref.params(c["m"], *SAT_SETS[c["curve"]])
        x = np.stack([lin_f64.content("step", SAT_LEN, 2, SAT_B, 200 + 7 * s + c["m"], amp=0.5) for s in range(N_STREAMS)])
        if c.get("handle"):
            x = np.concatenate([x, np.zeros((N_STREAMS, sat_ref.latency(c["m"]), 2), np.float32)], axis=1)
        ref = statement(sat_ref)
        want = sat_ref.run_streams(ref, p, x)
        r = np.stack([sat_ref.run_np(p, s, sat_ref.taps(ref, c["m"])) for s in x])
        for a in (x, want, r):
            a.setflags(write=False)
        _refs[key] = (p, x, want, r)
    return _refs[key]


def check(c, got, want, r, measure, caps):
    """every stream-channel of got[streams, n, ch] under the caps against r, then the statement's bits"""
    assert got.shape == want.shape == r.shape and np.isfinite(got).all()
    bad = []
    for s in range(got.shape[0]):
        for ch, (g, st) in enumerate(zip(measure(s, got[s]), measure(s, want[s]))):
            print("LINF64", c["node"], c["id"], s, ch, " ".join(f"{v:.4g}" for v in g[:3]), "|", " ".join(f"{v:.4g}" for v in st[:3]))
            bad += [(name, s, ch, a, cap) for name, a, cap in zip(("e_rms", "e_blk", "e_max"), g, caps) if not a <= cap]
    assert not bad, bad
    message = mismatch(got, want)
    assert not message, message


def setup(ctx, c):
    for k, v in c["keys"].items():
        ctx.debug_set(k, v)


@pytest.mark.parametrize("c", [c for c in CASES if c["node"] in ("K9", "K10")], ids=lambda c: c["id"])
def test_filters_against_float64(nae, c):
    h, x, want, r = lin_reference(c)
    B = c["n_fft"] // 2
    with nae.Context(0) as ctx:
        setup(ctx, c)
        if c.get("handle"):
            n = x.shape[1] - (h.shape[-1] - 1)
            run = fir_stream if c["node"] == "K9" else conv_stream
            got, launched = profiled(ctx, lambda: np.stack([run(nae, ctx, h, c["n_fft"], np.ascontiguousarray(s[:n]), (1, B - 1, 2 * B + 1, n)) for s in x]))
        elif c["node"] == "K9":
            got, launched = profiled(ctx, gpu_fir, nae, ctx, h, c["n_fft"], x, c["layout"], c["layout"])
        else:
            got, launched = profiled(ctx, gpu_conv, nae, ctx, h, c["n_fft"], x)
    assert set(c["kernels"]) <= launched, launched
    check(c, got, want, r, lambda s, y: lin_f64.channel_measures(y, r[s], h, x[s], B), CAPS[c["node"]])
    if c["what"] == "burst":
        assert all(m[3] >= 5 for s in range(N_STREAMS) for m in lin_f64.channel_measures(got[s], r[s], h, x[s], B)), "blocks that nothing feeds"


@pytest.mark.parametrize("c", [c for c in CASES if c["node"] == "K18"], ids=lambda c: c["id"])
def test_saturation_against_float64(nae, c):
    p, x, want, r = sat_reference(c)
    with nae.Context(0) as ctx:
        setup(ctx, c)
        if c.get("handle"):
            n = x.shape[1] - sat_ref.latency(c["m"])
            got, launched = profiled(ctx, lambda: np.stack([sat_stream(nae, ctx, p, np.ascontiguousarray(s[:n]), (1, SAT_B - 1, 2 * SAT_B + 1, n)) for s in x]))
        else:
            got, launched = profiled(ctx, gpu_sat, nae, ctx, p, x, **c["view"])
    assert set(c["kernels"]) <= launched, launched
    assert not (launched - set(c["kernels"])) & {"sat_kernel", "sat_map_kernel", "sat_map_flat_kernel"}, launched
    caps = CAPS["K18"] if c["m"] > 1 else (CAPS["K18 map"][0], np.inf, CAPS["K18 map"][1])
    check(c, got, want, r, lambda s, y: lin_f64.sat_channel_measures(y, r[s]), caps)
