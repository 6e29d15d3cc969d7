#!/usr/bin/env python3
"""Randomised differential run (GPU box): the effect nodes K10 ... K17 (long convolution, equalizer, dynamics, keyed dynamics, spectral gate,
loudness, echo, modulated delay), block entry and streaming handle, against their CPU statements under tests/*_ref/, bit for bit.  Every node
has one generator (draw_NODE(rng, ref module) -> a plain case record, no device needed) that draws the parameters over the whole range the
header states, a length from the node's edges or a uniform one, channel and stream counts, views with gaps, a shared source, the node's debug
keys and, for one case in three, the handle with random put sizes from the host and the device in turn.  One driver turns a record into the
GPU call and the statement call.  tests/test_fuzz_effects_cpu.py pins, without a GPU, what the seeds of tests/test_gpu_fuzz.py draw.
    python tests/tools/fuzz_effects.py NODE [cases=60] [seed=1]        NODE: conv eq dyn dynkey denoise loud echo mod"""
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conv_ref
import denoise_ref
import dyn_ref
import dynkey_ref
import echo_ref
import eq_ref
import loud_ref
import mod_ref
from block_gpu import bits, noise, statement

NODES = ("conv", "eq", "dyn", "dynkey", "denoise", "loud", "echo", "mod")
REFS = {"conv": conv_ref, "eq": eq_ref, "dyn": dyn_ref, "dynkey": dynkey_ref, "denoise": denoise_ref, "loud": loud_ref, "echo": echo_ref,
        "mod": mod_ref}
DEBUG_KEYS = {"conv": ("conv_tile", "conv_ring"), "denoise": ("dn_tile",), "echo": ("echo_group",), "mod": ("mod_sub",)}
CHUNK = eq_ref.CHUNK
RATES = (8000, 44100, 48000, 96000, 192000)
EQ_MIN_Q, EQ_MAX_Q, EQ_MAX_GAIN_DB = 0.1, 40.0, 24.0            # NAE_EQ_MIN_Q, NAE_EQ_MAX_Q, NAE_EQ_MAX_GAIN_DB
# NAE_DENOISE_MAX_REDUCTION_DB, NAE_DENOISE_MIN_SENSITIVITY_DB and NAE_DENOISE_MAX_SENSITIVITY_DB
DENOISE_MAX_REDUCTION_DB, DENOISE_SENSITIVITY_DB = 48.0, (-6.0, 24.0)
# NAE_LOUD_MIN_TARGET_LUFS and NAE_LOUD_MAX_TARGET_LUFS, NAE_LOUD_MIN_CEILING_DBTP, NAE_LOUD_MAX_GAIN_DB
LOUD_TARGET_LUFS, LOUD_MIN_CEILING_DBTP, LOUD_MAX_GAIN_DB = (-70.0, -5.0), -20.0, 40.0
MAX_FLOATS = 1 << 21                                             # a case's signal: 8 MiB
ECHO_LONGEST_AT = 5                                              # the case index that runs NAE_ECHO_MAX_DELAY
# (cases, seed) of the seeded runs of tests/test_gpu_fuzz.py; tests/test_fuzz_effects_cpu.py asserts the edges these draws reach
SEEDED = {"conv": (72, 3), "eq": (96, 3), "dyn": (96, 3), "dynkey": (36, 3), "denoise": (72, 3), "loud": (36, 3), "echo": (72, 3), "mod": (96, 3)}


# ---------------------------------------------------------------------------------------------------- what the generators share
def pick(rng, options):
    return options[int(rng.integers(len(options)))]


def log_uniform(rng, lo, hi):
    return float(lo * (hi / lo) ** rng.uniform())


def draw_section(rng, eq):
    """one section of eq_ref.design: any kind, rate, frequency 20 Hz ... 0.45 rate and q (both log-uniform) and gain of nae_eq_design's ranges"""
    kind, rate = pick(rng, eq.KINDS), pick(rng, RATES)
    freq, q = log_uniform(rng, 20.0, 0.45 * rate), log_uniform(rng, EQ_MIN_Q, EQ_MAX_Q)
    return eq.design(kind, rate, freq, float(rng.uniform(-EQ_MAX_GAIN_DB, EQ_MAX_GAIN_DB)), q)


def draw_sections(rng, eq, n):
    return np.stack([draw_section(rng, eq) for _ in range(n)]) if n else np.zeros((0, 5))


def unit_lengths(rng, unit, most=8):
    """the lengths around a unit's grid: 1, unit - 1, unit, unit + 1, k unit - 1, k unit, k unit + 1 for one k in 1 ... 5, and a uniform one"""
    k = int(rng.integers(1, 6))
    return [1, unit - 1, unit, unit + 1, k * unit - 1, k * unit, k * unit + 1, int(rng.integers(1, most * unit + 1))]


def chunk_lengths(rng):
    return [63, 64, 65] + unit_lengths(rng, CHUNK)


def finish(rng, case, ch, lengths, unit):
    """what every node's record holds besides its parameters: the length (one of `lengths`, at least 1), the stream count (1 ... 12, halved
    until the signal fits MAX_FLOATS), the layouts, a shared source one time in four, gap / chan_pad / offset, the handle one time in three
    with 1 ... 5 put sizes of 1 ... 6 units from the host and the device in turn, and the seed of the signals"""
    in_len = max(1, int(pick(rng, lengths)))
    n_streams = int(rng.integers(1, 13))
    while n_streams > 1 and n_streams * in_len * ch > MAX_FLOATS:
        n_streams //= 2
    case.update(ch=ch, in_len=in_len, unit=unit, n_streams=n_streams, src=pick(rng, "ip"), dst=pick(rng, "ip"), shared=bool(rng.integers(4) == 0))
    case["gap"], case["chan_pad"], case["offset"] = (int(pick(rng, (0, 1, 37))) for _ in range(3))
    case["handle"] = bool(rng.integers(3) == 0)
    case["puts"] = [int(p) for p in rng.integers(1, 6 * unit + 1, int(rng.integers(1, 6)))]
    case["device"] = pick(rng, ((False, True), (True, False)))
    case["x_seed"] = int(rng.integers(1 << 31))
    case.setdefault("debug", {})
    return case


# ---------------------------------------------------------------------------------------------------- the generators
def draw_conv(rng, ref):
    n_fft = int(pick(rng, ref.SIZES))
    B = n_fft // 2
    L = int(pick(rng, (1, B - 1, B, B + 1, 2 * B, 2 * B + 1, int(rng.integers(1, 20 * B + 1)))))
    P = ref.parts(L, n_fft)
    ch = int(rng.integers(1, 3))
    kb = int(rng.integers(1, 12))
    lengths = [1, B - 1, B + 1, kb * B - 1, kb * B, kb * B + 1, P * B - 1, P * B, P * B + 1, (P + 1) * B + 1, int(rng.integers(1, 70 * B + 1))]
    case = finish(rng, dict(node="conv", n_fft=n_fft, n_taps=L, parts=P, taps_ch=int(rng.integers(1, ch + 1))), ch, lengths, B)
    blocks = -(-case["in_len"] // B)
    case["debug"] = {"conv_tile": int(pick(rng, (0, 1, 2, 3, int(rng.integers(1, blocks + 3))))), "conv_ring": int(pick(rng, (0, P, P + 1, 2 * P + 3)))}
    return case


def draw_eq(rng, ref):
    coef = draw_sections(rng, ref, int(rng.integers(1, ref.MAX_SECTIONS + 1)))
    good = np.asarray(pick(rng, ref.GOOD_SECTIONS), np.float64)
    if rng.integers(8) == 0:                                     # a hand-made section at the rim of the stability triangle, behind the others
        coef = np.concatenate([coef[:ref.MAX_SECTIONS - 1], good[None]])
    return finish(rng, dict(node="eq", coef=np.ascontiguousarray(coef)), int(rng.integers(1, 3)), chunk_lengths(rng), CHUNK)


def draw_dyn_params(rng, ref):
    """dyn_ref.design over nae_dyn_design's ranges; ratio 1, a limiter's, or log-uniform 1 ... 100; knee and attack 0 one time in three; the
    look-ahead then one of 0, 1, 15, 16, 17, 1023, 1024 or a uniform one"""
    ratio = pick(rng, (1.0, math.inf, log_uniform(rng, 1.0, 100.0)))
    knee = float(pick(rng, (0.0, rng.uniform(0.0, 24.0), rng.uniform(0.0, 24.0))))
    attack = float(pick(rng, (0.0, log_uniform(rng, 1e-5, 0.5), log_uniform(rng, 1e-5, 0.5))))
    p = ref.design(pick(rng, RATES), float(rng.uniform(-60.0, 0.0)), ratio, knee, attack, log_uniform(rng, 0.001, 5.0), 0.0,
                   float(rng.uniform(-24.0, 24.0)), int(rng.integers(2)))
    p.lookahead = int(pick(rng, (0, 1, 15, 16, 17, 1023, 1024, int(rng.integers(0, ref.MAX_LOOKAHEAD + 1)))))
    return p, math.isinf(ratio)


def draw_dyn(rng, ref):
    p, limiter = draw_dyn_params(rng, ref)
    case = dict(node="dyn", p=p, limiter=limiter, scale=10.0 ** rng.uniform(-3.0, 0.3))      # levels on both sides of any threshold
    return finish(rng, case, int(rng.integers(1, 3)), chunk_lengths(rng), CHUNK)


def draw_dynkey(rng, ref):
    ch = int(rng.integers(1, 3))
    dyn, limiter = draw_dyn_params(rng, dyn_ref)
    key_ch = int(rng.integers(0, ch + 1))                        # 0 (the signal is its own key), 1, or ch
    p = ref.params(dyn, key_ch, draw_sections(rng, eq_ref, int(rng.integers(0, ref.MAX_SECTIONS + 1))))
    case = dict(node="dynkey", p=p, limiter=limiter, scale=10.0 ** rng.uniform(-3.0, 0.3), key_scale=10.0 ** rng.uniform(-3.0, 0.3),
                key_layout=pick(rng, "ips"))
    return finish(rng, case, ch, chunk_lengths(rng), CHUNK)


def draw_denoise(rng, ref):
    """the signal's level is drawn around the threshold the design puts on a profile of level 1, so that the gate opens and closes"""
    n_fft = int(pick(rng, ref.SIZES))
    H = n_fft // 4
    thr, floor = ref.design(statement(ref), float(rng.uniform(0.0, DENOISE_MAX_REDUCTION_DB)), float(rng.uniform(*DENOISE_SENSITIVITY_DB)))
    p = ref.params(n_fft, int(rng.integers(0, ref.MAX_TIME + 1)), int(rng.integers(0, ref.MAX_FREQ + 1)), thr, floor)
    ch = int(rng.integers(1, 3))
    case = dict(node="denoise", p=p, profile_ch=int(rng.integers(1, ch + 1)), tilt_db=float(rng.uniform(-6.0, 0.0)),
                level=math.sqrt(thr) * 10.0 ** (rng.uniform(-4.0, 4.0) / 20.0))
    lengths = [n_fft - 1, n_fft, n_fft + 1] + unit_lengths(rng, H, 60)
    finish(rng, case, ch, lengths, H)
    blocks = -(-case["in_len"] // H)
    case["debug"] = {"dn_tile": int(pick(rng, (0, 1, int(rng.integers(1, blocks + 3)))))}
    return case


def draw_loud(rng, ref):
    """the stepped signal (0.5 s far under the absolute gate, then programme) from its start or from the programme's, cut to the length"""
    rate = int(pick(rng, (8000, 22050, 44100, 48000, 96000, 192000, 10 * int(rng.integers(800, 19201)))))
    B = rate // 10
    case = dict(node="loud", sample_rate=rate, target_lufs=float(rng.uniform(*LOUD_TARGET_LUFS)),
                ceiling_dbtp=float(rng.uniform(LOUD_MIN_CEILING_DBTP, 0.0)), max_gain_db=float(rng.uniform(0.0, LOUD_MAX_GAIN_DB)),
                start=int(pick(rng, (0, rate // 2))), scale=10.0 ** rng.uniform(-1.5, 0.5))
    whole = 3 * rate + 37 - case["start"]
    k, c = int(rng.integers(1, 26)), int(rng.integers(1, whole // CHUNK + 1))
    lengths = [1, B - 1, B, B + 1, 4 * B - 1, 4 * B, 4 * B + 1, k * B - 1, k * B, k * B + 1, c * CHUNK - 1, c * CHUNK, c * CHUNK + 1,
               int(rng.integers(1, whole + 1)), whole]
    return finish(rng, case, int(rng.integers(1, 3)), [min(n, whole) for n in lengths], B)


def echo_loop_db(coef, g):
    """the loop's gain per repeat in dB: |g| times the sections' largest magnitude, on a grid that resolves q = 40 at 20 Hz and 192 kHz"""
    f = np.concatenate([np.geomspace(1e-5, 0.5, 4096), np.linspace(0.0, 0.5, 1025)])
    z = np.exp(-2j * np.pi * f)
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in coef:
        h *= (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return 20.0 * math.log10(max(abs(g) * float(np.abs(h).max()), 1e-300))


def draw_echo(rng, ref):
    """a loop that gains (sections that boost, under a feedback near 1) grows with every repeat, and the line is f32: its lengths are cut to
    the repeats that keep it under 300 dB, so that the statement stays finite"""
    ch = int(rng.integers(1, 3))
    d0 = int(pick(rng, (1024, 1025, int(rng.integers(1024, 9001)), int(rng.integers(1024, 70001)))))
    d1 = int(pick(rng, (d0, d0 + 1, int(pick(rng, (1024, 1025, int(rng.integers(1024, 9001)), int(rng.integers(1024, 70001))))))))
    g = float(pick(rng, (0.0, ref.MAX_FEEDBACK, -ref.MAX_FEEDBACK, rng.uniform(-ref.MAX_FEEDBACK, ref.MAX_FEEDBACK))))
    coef = draw_sections(rng, eq_ref, int(rng.integers(0, ref.MAX_SECTIONS + 1)))
    p = ref.params((d0, d1), g, int(rng.integers(2)), float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), coef)
    R, D = ref.ring(p, ch), max(d0, d1) if ch == 2 else d0
    lengths = chunk_lengths(rng) + [d0, d0 + 1, 2 * D + 1, R + 7, int(rng.integers(1, 3 * R + 8))]
    gain_db = echo_loop_db(coef, g) + 3.0                        # 3 dB for the sections' transients
    if gain_db > 0.0:
        most = (min(d0, d1) if ch == 2 else d0) * max(1, int(300.0 / gain_db))
        lengths = [min(n, most) for n in lengths]
    case = finish(rng, dict(node="echo", p=p), ch, lengths, CHUNK)
    case["debug"] = {"echo_group": int(pick(rng, (0, 1, 3)))}
    return case


def echo_longest(case):
    """the record turned into the longest line: NAE_ECHO_MAX_DELAY on one mono stream of D + 1025 samples, through the block entry"""
    case["p"].delay[0] = case["p"].delay[1] = echo_ref.MAX_DELAY
    case.update(ch=1, n_streams=1, in_len=echo_ref.MAX_DELAY + 1025, handle=False, shared=False)
    return case


def draw_mod(rng, ref):
    """the sweep by its reaches: lo = delay - depth (its floor less 1 is the run length under feedback), hi = delay + depth"""
    lo = float(pick(rng, (ref.MIN_DELAY, ref.MIN_DELAY + rng.uniform(0.0, 70.0), rng.uniform(ref.MIN_DELAY, ref.MAX_DELAY))))
    hi = float(pick(rng, (ref.MAX_DELAY, rng.uniform(lo, ref.MAX_DELAY))))
    delay, depth = (lo + hi) / 2.0, (hi - lo) / 2.0
    while depth > 0.0 and not (delay - depth >= ref.MIN_DELAY and delay + depth <= ref.MAX_DELAY):   # the rounding of the two halves
        depth = float(np.nextafter(depth, 0.0))
    g = float(pick(rng, (0.0, ref.MAX_FEEDBACK, -ref.MAX_FEEDBACK, rng.uniform(-ref.MAX_FEEDBACK, ref.MAX_FEEDBACK))))
    voices = tuple(int(v) for v in rng.integers(0, 1 << 32, int(rng.integers(1, ref.MAX_VOICES + 1)), dtype=np.uint64))
    rate_inc = int(pick(rng, (ref.hz(float(rng.uniform(0.0, 20.0))), int(rng.integers(0, 1 << 32, dtype=np.uint64)))))
    p = ref.params(delay, depth, g, float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), rate_inc, int(rng.integers(0, 1 << 32, dtype=np.uint64)),
                   int(rng.integers(0, 1 << 32, dtype=np.uint64)), voices, int(rng.integers(2)))
    lengths = chunk_lengths(rng) + [4096, 4097]
    if rng.integers(2):
        lengths = [n + 4096 for n in lengths]                    # the ring wraps
    case = finish(rng, dict(node="mod", p=p), int(rng.integers(1, 3)), lengths, CHUNK)
    case["debug"] = {"mod_sub": int(pick(rng, (0, 0, int(rng.integers(1, 65)))))}
    return case


GENERATORS = {"conv": draw_conv, "eq": draw_eq, "dyn": draw_dyn, "dynkey": draw_dynkey, "denoise": draw_denoise, "loud": draw_loud,
              "echo": draw_echo, "mod": draw_mod}


def draw(node, cases, seed):
    """the records a run of `cases` cases at `seed` makes, in order; needs no device"""
    rng = np.random.default_rng(seed)
    for k in range(cases):
        case = GENERATORS[node](rng, REFS[node])
        yield echo_longest(case) if node == "echo" and k == ECHO_LONGEST_AT else case


# ---------------------------------------------------------------------------------------------------- a record's signals and its statement
def check(case, L):
    """the statement's own verdict on the record's parameters: 0 where it is valid"""
    node, ch = case["node"], case["ch"]
    if node == "conv":
        ok = case["n_fft"] in conv_ref.SIZES and 1 <= case["n_taps"] <= conv_ref.MAX_TAPS and case["parts"] <= conv_ref.MAX_PARTS
        return 0 if ok and case["taps_ch"] in (1, ch) else -1
    if node == "eq":
        return L.ref_eq_check(case["coef"].ctypes.data, case["coef"].shape[0])
    if node == "dyn":
        return L.ref_dyn_check(C.byref(case["p"]))
    if node in ("dynkey", "echo", "mod"):
        return getattr(L, f"ref_{node}_check")(C.byref(case["p"]), ch)
    if node == "denoise":
        p = case["p"]
        rc = L.ref_denoise_run(p.n_fft, p.time_smooth, p.freq_smooth, p.thr_scale, p.floor_gain, None, None, 0, 1, None, None, None, None)
        return rc if math.isfinite(p.thr_scale) and p.thr_scale >= 0.0 and 0.0 <= p.floor_gain <= 1.0 and case["profile_ch"] in (1, ch) else -1
    return loud_ref.design_c(L, case["sample_rate"], case["target_lufs"], case["ceiling_dbtp"], case["max_gain_db"])[0]


def signals(case):
    """the record's signals from its seed: x[streams, n, ch] (one stream for a handle case) and what else the node reads"""
    rng = np.random.default_rng(case["x_seed"])
    node, n, ch = case["node"], case["in_len"], case["ch"]
    n_streams, shared = (1, False) if case["handle"] else (case["n_streams"], case["shared"])
    sig = {}
    if node == "denoise":
        sig["x"] = denoise_ref.wander(rng, n_streams, n, ch, level=case["level"], period=3.0 * case["p"].n_fft, shared=shared)
        sig["profile"] = denoise_ref.flat_profile(case["p"].n_fft, case["profile_ch"], tilt_db=case["tilt_db"])
    elif node == "loud":
        at = case["start"]
        x = np.stack([loud_ref.stepped(case["sample_rate"], ch, seed=case["x_seed"] + s, scale=case["scale"] * 0.5 ** s)[at:at + n] for s in range(n_streams)])
        if shared:
            x[:] = x[0]
        sig["x"] = x
    else:
        sig["x"] = noise(rng, n_streams, n, ch, shared) * np.float32(case.get("scale", 1.0))
    if node == "conv":
        sig["taps"] = rng.uniform(-1, 1, case["n_taps"] if case["taps_ch"] == 1 else (case["taps_ch"], case["n_taps"])).astype(np.float32)
    if node == "dynkey" and case["p"].key_ch:
        sig["key"] = noise(rng, 1 if case["key_layout"] == "s" and not case["handle"] else n_streams, n, case["p"].key_ch) * np.float32(case["key_scale"])
    return sig


def want(case, sig, L):
    """the statement on the record's signals -> [streams, frames, ch] (a handle case: one stream, in the length the flushed handle delivers);
    for the loudness also the records"""
    node, x = case["node"], sig["x"]
    if node == "conv":
        if case["handle"]:
            x = np.concatenate([x, np.zeros((1, case["n_taps"] - 1, case["ch"]), np.float32)], 1)
        return conv_ref.run_streams(L, sig["taps"], case["n_fft"], x)
    if node == "eq":
        return eq_ref.run_streams(L, case["coef"], x)
    if node == "dyn":
        return dyn_ref.run_streams(L, case["p"], x)
    if node == "dynkey":
        return dynkey_ref.run_streams(L, case["p"], x, sig.get("key"))
    if node == "denoise":
        return denoise_ref.run_streams(L, case["p"], sig["profile"], x)
    if node == "loud":
        params = loud_ref.design_c(L, case["sample_rate"], case["target_lufs"], case["ceiling_dbtp"], case["max_gain_db"])[1]
        pairs = [loud_ref.normalize(L, params, s) for s in x]
        return np.stack([y for y, _ in pairs]), [r for _, r in pairs]
    return REFS[node].run_streams(L, case["p"], x)


# ---------------------------------------------------------------------------------------------------- the GPU side
def on_gpu(nae, ctx, case, sig):
    """the record through the block entry in its view, or through the handle under its puts -> what `want` returns"""
    import conv_gpu, denoise_gpu, dyn_gpu, dynkey_gpu, echo_gpu, eq_gpu, loud_gpu, mod_gpu
    node, x = case["node"], sig["x"]
    views = (case["src"], case["dst"], case["shared"])
    kw = dict(gap=case["gap"], offset=case["offset"], chan_pad=case["chan_pad"])
    handle, puts, device = case["handle"], case["puts"], case["device"]
    if node == "loud":
        params = nae.Context.loud_design(case["sample_rate"], case["target_lufs"], case["ceiling_dbtp"], case["max_gain_db"])
        if handle:
            return None, [loud_gpu.loud_stream(nae, ctx, params, x[0], puts, device)]
        return loud_gpu.gpu_normalize(nae, ctx, params, x, *views, **kw)
    if node == "conv":
        args, block, stream = (sig["taps"], case["n_fft"]), conv_gpu.gpu_conv, conv_gpu.conv_stream
    elif node == "eq":
        args, block, stream = (case["coef"],), eq_gpu.gpu_eq, eq_gpu.eq_stream
    elif node == "dyn":
        args, block, stream = (case["p"],), dyn_gpu.gpu_dyn, dyn_gpu.dyn_stream
    elif node == "denoise":
        args, block, stream = (case["p"], sig["profile"]), denoise_gpu.gpu_denoise, denoise_gpu.denoise_stream
    elif node == "echo":
        args, block, stream = (case["p"],), echo_gpu.gpu_echo, echo_gpu.echo_stream
    elif node == "mod":
        args, block, stream = (case["p"],), mod_gpu.gpu_mod, mod_gpu.mod_stream
    else:
        key = sig.get("key")
        if handle:
            return dynkey_gpu.dynkey_stream(nae, ctx, case["p"], x[0], None if key is None else key[0], puts, device)[None]
        return dynkey_gpu.gpu_dynkey(nae, ctx, case["p"], x, key, *views, key_layout=case["key_layout"], **kw)
    if handle:
        return stream(nae, ctx, *args, x[0], puts, device)[None]
    return block(nae, ctx, *args, x, *views, **kw)


def describe(case):
    skip = ("node", "p", "coef", "puts", "device", "x_seed", "unit", "debug")
    what = " ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in case.items() if k not in skip)
    if case["node"] == "eq":
        what += f" sections {case['coef'].shape[0]}"
    if "p" in case:
        p = case["p"]
        what += " " + " ".join(f"{f} {getattr(p, f)}" for f, t in p._fields_ if t in (C.c_int, C.c_double, C.c_float, C.c_uint32))
        if hasattr(p, "dyn"):
            what += f" lookahead {p.dyn.lookahead} link {p.dyn.link}"
        if case["node"] == "echo":
            what += f" delays {p.delay[0]} {p.delay[1]}"
    if case["handle"]:
        what += f" puts {case['puts']} {'device' if case['device'][0] else 'host'} first"
    return what + "".join(f" {k} {v}" for k, v in case["debug"].items())


def main(node, cases=60, seed=1, ctx=None, nae=None):
    assert node in NODES, f"NODE is one of {' '.join(NODES)}"
    if nae is None:
        import naeload
        nae = naeload.load()
    if ctx is None:
        ctx = nae.Context(0)
    from loud_gpu import same_record
    L = statement(REFS[node])
    done = 0
    try:
        for k, case in enumerate(draw(node, cases, seed)):
            assert check(case, L) == 0, f"case {k}: the generator drew a record the statement rejects: {describe(case)}"
            for key in DEBUG_KEYS.get(node, ()):
                ctx.debug_set(key, case["debug"][key])
            sig = signals(case)
            exp = want(case, sig, L)
            assert np.isfinite(exp[0] if node == "loud" else exp).all(), f"case {k}: {describe(case)}: the statement's output is not finite (the draw's fault, not the kernel's)"
            got = on_gpu(nae, ctx, case, sig)
            if node == "loud":
                (got, got_records), (exp, exp_records) = got, exp
                for r, w in zip(got_records, exp_records):
                    same_record(r, w)
            if got is not None:
                assert got.shape == exp.shape, (k, got.shape, exp.shape)
                differ = int(np.count_nonzero(bits(got) != bits(exp)))
                assert differ == 0, f"case {k}: {describe(case)}: {differ} words differ, the first at {np.argwhere(bits(got) != bits(exp))[0].tolist()}"
            done += 1
            print(f"case {k:3d}: {describe(case)}  bit-exact", flush=True)
    finally:
        for key in DEBUG_KEYS.get(node, ()):
            ctx.debug_set(key, 0)
    print(f"{node}: {done} cases bit-exact")
    return done


if __name__ == "__main__":
    main(sys.argv[1], *(int(a) for a in sys.argv[2:4]))
