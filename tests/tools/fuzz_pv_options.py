#!/usr/bin/env python3
"""Randomised differential run (GPU box) over the option space of the K7 phase vocoder: the four frame sizes, NAE_STRETCH_PHASE_LOCK (1024),
NAE_STRETCH_TRANSIENTS, NAE_STRETCH_LINK_CHANNELS, the formant lifter, the formant shift in its four plan cases A ... D, both stage orders,
mono and stereo, batches of 1 ... 5 streams, the tilings, source and destination layouts and the streaming handle, against the CPU statement
tests/pv_ref/ref_pv.c.  One generator (draw -> plain case records; no device needed, it runs the CPU statement) draws a record per case;
the class of case k is PLAN[k % len(PLAN)], so every option meets every other over a run.  The input is the scene of tests/pv_gpu.py (two
partials per channel over quiet noise, clicks and bursts in the left channel only, the right only, or both), every stream from a seed of its
own, at a length that gives the vocoder 48 ... 160 frames: several 16-frame tiles and a 64-frame tile edge.  Uniform noise, which the other
vocoder fuzzers feed, fires no onset in the statement and would reach none of the reset logic.  Where the transient flag is effective, draw
re-places the hits (the next sub-seed) until the statement has an onset in every stream, no two streams of a batch have the same onsets, and,
unlinked stereo, every stream has an onset in the left channel only and one in the right only.
run_case asserts, with describe(case) in every message:
    (a) the integer phases in front of every tile (debug_pv_tile_phase, the case's flags and stream count) equal the statement's of every
        stream and channel, bit for bit, where the plan has the vocoder stage and does not force it;
    (b) every stream within TOL relative RMS of the statement called with the same options (orc.stretch at 1024 without flags and lifter),
        and finite;
    (c) every stream of a batch equal to its lone run with the same options, tile and layouts, bit for bit;
    (d) the handle of the matching create entry (_n, _formant, _formant_shift), fed stream 0 in the drawn put pattern with host and device
        puts in turns, equal to the block call, bit for bit;
    (e) the sentinel in every word of the destination buffer outside the view;
    (f) the kernels of the effective options launched (expected_kernels restates nae_pv_resolve and the launchers' names), no *link* or
        *transient* kernel where nae_pv_resolve makes the flag a no-op, and there the bits of the same call without the flag.
tests/test_fuzz_pv_cpu.py pins, without a GPU, what SEEDED draws.
    python tests/tools/fuzz_pv_options.py [cases=200] [seed=1]"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from fuzz_graph import SENTINEL, TOL, bits, first_difference, pick     # the vocoder's bar of every file; no output reaches the sentinel

SEEDED = (24, 6)                                                 # (cases, seed) of tests/test_gpu_fuzz.py::test_fuzz_pv_options_seeded
SIZES = (512, 1024, 2048, 4096)
LOCK, TR, LINK = 1, 4, 16                                        # NAE_STRETCH_PHASE_LOCK, _TRANSIENTS, _LINK_CHANNELS
TILES = (0, 1, 2, 3, 16, 64)                                     # debug key pv_tile; 0: the library's choice (the phases: 64)
PUTS = ("frames", "1152", "hop", "all")
MAX_SAMPLES = 2_000_000                                          # n_streams * max(L, out_len) * ch of a record
FRAMES = (48, 160)
SUB_SEEDS = 64                                                   # places tried for the hits before a record is given up (an error)
# tr-*: transient preservation unlinked stereo, linked stereo, mono, in a batch of 3 ... 5; lock, lock-tr: 1024 locked; shift-A ... D: the
# formant shift's plan cases; plain: neither option; no-pv: the transposer alone or a wire, the flags set
PLAN = ("tr-stereo", "shift-A", "tr-link", "lock", "tr-batch", "shift-C", "tr-mono", "lock-tr", "shift-B", "plain", "shift-D", "no-pv")

_nae = None
_ref = None


def lib():
    """the package (its plans are static: no device) and the CPU statement"""
    global _nae, _ref
    if _nae is None:
        import naeload
        import pv_ref
        _nae = naeload.load()
        _ref = pv_ref.build(tempfile.mkdtemp(prefix="fuzz_pv_"))
    return _nae, _ref


# ---------------------------------------------------------------------------------------------------- the record
def draw_layout(rng, clean):
    """interleaved or planar; unless clean, padded frame / plane and stream strides and a base 1 ... 3 floats off (tests/test_gpu_nodes.py::_place)"""
    planar = bool(rng.integers(2))
    if clean:
        return dict(planar=planar, base=0, pad=0, pad_s=0)
    return dict(planar=planar, base=int(rng.integers(1, 4)), pad=int(rng.integers(0, 5 if planar else 3)), pad_s=int(rng.integers(0, 7)))


def draw_one(rng, kind):
    n_fft = 1024 if kind in ("lock", "lock-tr") else int(pick(rng, SIZES))
    H = n_fft // 4
    ch = {"tr-stereo": 2, "tr-link": 2, "tr-mono": 1}.get(kind, int(rng.integers(1, 3)))
    lock = kind in ("lock", "lock-tr") or (kind.startswith("shift") or kind == "no-pv") and n_fft == 1024 and bool(rng.integers(2))
    transients = kind.startswith("tr-") or kind == "lock-tr" or (kind not in ("lock", "plain") and bool(rng.integers(2)))
    if ch == 2 and (lock or transients):
        link = kind == "tr-link" or (kind != "tr-stereo" and bool(rng.integers(2)))
    else:
        link = bool(rng.random() < 0.1)                           # a no-op on purpose
    shift = kind.startswith("shift")
    q_default = min(max(48000 // 700, 1), n_fft // 4)
    lifter = int(pick(rng, (q_default, int(rng.integers(1, n_fft // 4 + 1))) if shift else (0, 0, q_default, int(rng.integers(1, n_fft // 4 + 1)))))
    tempo = 1.0 if kind in ("shift-C", "shift-D", "no-pv") else float(np.exp(rng.uniform(np.log(0.3), np.log(8.0))))
    if abs(tempo - 1.0) < 0.02 and kind not in ("shift-C", "shift-D", "no-pv"):
        tempo = 1.25
    rhos = (1.0, float(rng.uniform(0.5, 0.97)), float(rng.uniform(1.03, 2.5)))    # no transposer, behind the vocoder, in front of it
    rho = {"shift-A": rhos[1 + int(rng.integers(2))], "shift-B": 1.0, "shift-C": rhos[1 + int(rng.integers(2))], "shift-D": 1.0,
           "no-pv": float(pick(rng, (2.0, 0.75, 1.0)))}.get(kind, rhos[int(rng.integers(3))])
    rate, pitch = float(np.float32(rho * tempo)), float(np.float32(1.0 / tempo))   # a handle takes floats
    phi = None
    while shift and (phi is None or abs(rho / phi - 1.0) < 0.02):
        phi = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0))))
    n_streams = int(rng.integers(3, 6)) if kind == "tr-batch" else int(rng.integers(1, 6))
    frames = int(rng.integers(FRAMES[0], FRAMES[1] + 1))
    scale = max(rho, 1.0)                                         # the transposer first: the vocoder reads L / rho samples
    size = lambda f, n: n * ch * max(f * H * tempo * scale + n_fft, (f * H * tempo * scale + n_fft) / (rho * tempo)) * 1.02
    while size(frames, n_streams) > MAX_SAMPLES and frames > FRAMES[0]:
        frames = max(FRAMES[0], frames * 3 // 4)
    while size(frames, n_streams) > MAX_SAMPLES and n_streams > 1:
        n_streams -= 1
    L = int(frames * H * tempo * scale) + n_fft
    clean = bool(rng.integers(2))
    return dict(label=kind, n_fft=n_fft, lock=bool(lock), transients=bool(transients), link=bool(link), lifter=lifter, formant_ratio=phi, ch=ch,
                n_streams=n_streams, rate=rate, pitch=pitch, L=L, pv_tile=int(pick(rng, TILES)), src=draw_layout(rng, clean),
                dst=draw_layout(rng, clean), puts=str(pick(rng, PUTS)), seed=int(rng.integers(1 << 31)), sub=0)


def plans(case):
    """(the plan the call runs, the _n plan)"""
    nae, _ = lib()
    pn = nae.Context.stretch_plan(case["rate"], case["pitch"], case["L"], case["n_fft"])
    if case["formant_ratio"] is None:
        return pn, pn
    return nae.Context.stretch_plan(case["rate"], case["pitch"], case["L"], case["n_fft"], formant=case["lifter"], formant_ratio=case["formant_ratio"]), pn


def plan_case(case):
    """the formant shift's plan case A ... D (include/nae_gpu.h), None without a shift"""
    if case["formant_ratio"] is None:
        return None
    pn = plans(case)[1]
    return {(1, 1): "A", (1, 0): "B", (0, 1): "C", (0, 0): "D"}[int(pn.pv_on), int(pn.rs_on)]


def resolve(case):
    """nae_pv_resolve restated: dict(stage: the vocoder stage runs and is not forced, forced, transients, link: the flags as they are
    effective, lifter: the effective lifter)"""
    pl, _ = plans(case)
    forced = bool(pl.pv_on) and pl.tempo_eff == 1.0
    stage = bool(pl.pv_on) and not forced
    r = pl.rate_eff / (case["formant_ratio"] or 1.0) - 1.0
    lifter = case["lifter"] if pl.pv_on and case["lifter"] > 0 and (r <= -1e-6 or r >= 1e-6) else 0
    tr = case["transients"] and stage
    return dict(stage=stage, forced=forced, transients=tr, link=case["link"] and case["ch"] == 2 and stage and (case["lock"] or tr), lifter=lifter)


def expected_kernels(case):
    """the pass-3 kernel a call with an effective transient flag or link launches (the launchers' names in kernels_pv_any.hip and
    kernels_pvlock.hip), else none: the unflagged routes are other tests'.  Pass 1 has the same suffixes, and a stream of one tile runs
    without it."""
    eff = resolve(case)
    if not (eff["transients"] or eff["link"]):
        return ()
    f = "_formant" if eff["lifter"] else ""
    if case["lock"]:
        return (f"pvlock_synth{f}{'_transient' if eff['transients'] else ''}{'_link' if eff['link'] else ''}_kernel",)
    return (f"pv_any_synth{f}{'_link' if eff['link'] else '_transient'}_kernel",)


def signals(case):
    """the streams' contents [n_streams, L, ch] from the record's seed and sub-seed alone: the scene, every stream from a seed of its own (mono:
    the scene's left channel), about one hit in ten frames"""
    from pv_gpu import scene
    L, n_fft = case["L"], case["n_fft"]
    frames = max(FRAMES[0], int(plans(case)[0].frames))
    xs = [scene(L, seed=(case["seed"], s, case["sub"]), n_hits=max(6, frames // 10)).reshape(L, 2)[:, :case["ch"]] for s in range(case["n_streams"])]
    return np.ascontiguousarray(np.stack(xs), np.float32)


def onset_sets(case, x=None):
    """per stream, the statement's onset verdicts [frames, ch] as the call acts on them (linked where the link is effective); None where
    the transient flag is not effective"""
    import pv_ref
    eff = resolve(case)
    if not eff["transients"]:
        return None
    x = signals(case) if x is None else x
    _, ref = lib()
    return [pv_ref.taps(ref, x[s].reshape(-1), case["ch"], case["rate"], case["pitch"], case["n_fft"], case["lock"], True, eff["link"])[1]
            for s in range(case["n_streams"])]


def conditions(case, on):
    """what the GPU run relies on, on the statement alone: an onset in every stream; no two streams with the same onsets; unlinked stereo, an
    onset in the left channel only and one in the right only in every stream"""
    if on is None:
        return True
    if not all(o.any() for o in on):
        return False
    if len({o.tobytes() for o in on}) != len(on):
        return False
    if case["ch"] == 2 and not resolve(case)["link"]:
        return all((o[:, 0] & ~o[:, 1]).any() and (o[:, 1] & ~o[:, 0]).any() for o in on)
    return True


def draw(cases, seed):
    """the records a run of `cases` cases at `seed` makes, in order; needs no device"""
    rng = np.random.default_rng(seed)
    for k in range(cases):
        case = draw_one(rng, PLAN[k % len(PLAN)])
        while not conditions(case, onset_sets(case)):
            case["sub"] += 1
            assert case["sub"] < SUB_SEEDS, f"{describe(case)}: no place of the hits meets the conditions"
        yield case


def describe(case):
    lay = lambda d: ("planar" if d["planar"] else "interleaved") + (f" base {d['base']} pad {d['pad']} stream pad {d['pad_s']}" if d["base"] else "")
    flags = " ".join(k for k in ("lock", "transients", "link") if case[k]) or "no flags"
    return (f"[{case['label']}] N {case['n_fft']} {flags} lifter {case['lifter']} phi {case['formant_ratio']} ch {case['ch']} streams "
            f"{case['n_streams']} rate {case['rate']:.6g} pitch {case['pitch']:.6g} L {case['L']} pv_tile {case['pv_tile']} src ({lay(case['src'])}) "
            f"dst ({lay(case['dst'])}) puts {case['puts']} seed {case['seed']}.{case['sub']}")


# ---------------------------------------------------------------------------------------------------- layouts
def view(n, S, ch, lay):
    """a layout record as (index array [stream, channel, frame] -> float offset, (base, stream, channel, frame strides), the buffer's floats)"""
    if lay["planar"]:
        fs, cs = 1, S + lay["pad"]
        span = ch * cs
    else:
        fs, cs = ch + lay["pad"], 1
        span = S * fs
    ss = span + lay["pad_s"]
    s, c, i = np.arange(n, dtype=np.int64)[:, None, None], np.arange(ch, dtype=np.int64)[None, :, None], np.arange(S, dtype=np.int64)[None, None, :]
    return lay["base"] + s * ss + c * cs + i * fs, (lay["base"], ss, cs, fs), lay["base"] + n * ss + 9


def put_sizes(case):
    """the handle's put pattern: one-frame puts for a stretch, then seeded random cuts; 1152; H - 1, H + 1, 7 and a long one; everything at once"""
    H, L = case["n_fft"] // 4, case["L"]
    if case["puts"] == "frames":
        return [1] * 40 + [int(v) for v in np.random.default_rng(case["seed"] + 2).integers(1, L // 6 + 2, 64)]
    return {"1152": [1152], "hop": [H - 1, H + 1, 7, L // 5 + 1], "all": [L]}[case["puts"]]


# ---------------------------------------------------------------------------------------------------- the run
def run_block(nae, c, case, x, flags=None):
    """the block call on x [n, L, ch] in the record's layouts into a buffer full of the sentinel -> (out [n, T, ch], the whole destination buffer,
    its view's index array); flags: (lock, transients, link) where not the record's"""
    n, L, ch = x.shape
    lock, tr, link = flags or (case["lock"], case["transients"], case["link"])
    T = int(plans(case)[0].out_len)
    si, (sb, sss, scs, sfs), sn = view(n, L, ch, case["src"])
    di, (db, dss, dcs, dfs), dn = view(n, T, ch, case["dst"])
    host = np.random.default_rng(case["seed"] + 1).uniform(-1, 1, sn).astype(np.float32)      # other values in the gaps
    host[si] = x.transpose(0, 2, 1)
    d_x, d_o = c.array(host), c.array(np.full(dn, SENTINEL, np.float32))
    c.stretch_block(case["rate"], case["pitch"], nae.Sig(d_x.at(sb), sss, scs, sfs), L, ch, n, nae.Sig(d_o.at(db), dss, dcs, dfs), phase_lock=lock,
                    n_fft=case["n_fft"], formant=case["lifter"], transients=tr, formant_ratio=case["formant_ratio"], link_channels=link)
    buf = d_o.download()
    d_x.free(); d_o.free()
    return np.ascontiguousarray(buf[di].transpose(0, 2, 1)), buf, di


def run_case(nae, case, verbose=False):
    """the record under the assertions (a) ... (f) of the module's docstring, on a context of its own -> the worst sample error"""
    import orc
    import pv_ref
    from pv_gpu import profiled, stream
    _, ref = lib()
    what = describe(case)
    x = signals(case)
    n, L, ch = x.shape
    n_fft, rate, pitch, lock, tr, link, q, phi = (case[k] for k in ("n_fft", "rate", "pitch", "lock", "transients", "link", "lifter", "formant_ratio"))
    pl, eff = plans(case)[0], resolve(case)
    assert conditions(case, onset_sets(case, x)), what
    worst = 0.0
    with nae.Context(0) as c:
        if case["pv_tile"]:
            c.debug_set("pv_tile", case["pv_tile"])
        (out, buf, di), launched = profiled(c, run_block, nae, c, case, x)
        # (e) nothing outside the view, (b) finite
        outside = np.ones(buf.size, bool)
        outside[di.ravel()] = False
        hit = np.flatnonzero(outside & (bits(buf) != bits(SENTINEL)))
        assert hit.size == 0, f"{what}: {hit.size} words of the destination buffer outside the view were written, the first at float {int(hit[0])}"
        assert np.isfinite(out).all(), f"{what}: non-finite output"
        # (f) the kernels
        want = expected_kernels(case)
        assert set(want) <= launched, f"{what}: launched {sorted(launched)}, expected {want}"
        for flag, word in (("link", "link"), ("transients", "transient")):
            assert eff[flag] or not any(word in k for k in launched), f"{what}: {flag} is not effective, launched {sorted(launched)}"
        if (link, tr) != (eff["link"], eff["transients"]):
            plain = run_block(nae, c, case, x, flags=(lock, eff["transients"], eff["link"]))[0]
            assert np.array_equal(bits(out), bits(plain)), f"{what}: against the call without the flags that are not effective: {first_difference(out.ravel(), plain.ravel())}"
        # (c) every stream against its lone run
        for s in range(n if n > 1 else 0):
            lone = run_block(nae, c, case, x[s:s + 1])[0]
            assert np.array_equal(bits(out[s]), bits(lone[0])), f"{what}: stream {s} against its lone run: {first_difference(out[s].ravel(), lone.ravel())}"
        # (b) the samples against the statement
        for s in range(n):
            xs = x[s].reshape(-1)
            if n_fft == 1024 and not (lock or tr or link or q or phi is not None):
                ref_out = orc.stretch(xs, ch, rate, pitch)
            else:
                ref_out = pv_ref.stretch(ref, xs, ch, rate, pitch, n_fft, lock, q, tr, phi, link)
            assert ref_out.size == out[s].size, f"{what}: stream {s}: {out[s].size} samples, the statement has {ref_out.size}"
            den = np.sqrt(np.mean(ref_out.astype(np.float64) ** 2))
            e = float(np.sqrt(np.mean((out[s].reshape(-1).astype(np.float64) - ref_out) ** 2)) / max(den, 1e-30))
            worst = max(worst, e)
            if verbose:
                print(f"    stream {s}: sample error {e:.3e} (RMS of the statement {den:.3e})", flush=True)
            assert e <= TOL, f"{what}: stream {s}: sample error {e:.3e} (RMS of the statement {den:.3e})"
        # (a) the integer phases
        if eff["stage"]:
            si, (sb, sss, scs, sfs), sn = view(n, L, ch, case["src"])
            host = np.zeros(sn, np.float32)
            host[si] = x.transpose(0, 2, 1)
            d_x = c.array(host)
            got, t = c.debug_pv_tile_phase(rate, pitch, nae.Sig(d_x.at(sb), sss, scs, sfs), L, ch, n, phase_lock=lock, n_fft=n_fft, transients=tr,
                                           link_channels=link)
            d_x.free()
            assert t == (case["pv_tile"] or 64) and got.shape[:2] == (n, ch), (what, t, got.shape)
            for s in range(n):
                qs = pv_ref.synth_phase(ref, x[s].reshape(-1), ch, rate, pitch, n_fft, lock, tr, link)
                assert got.shape[2] == (qs.shape[0] + t - 1) // t, (what, got.shape, qs.shape)
                for j in range(got.shape[2]):
                    w = qs[j * t - 1] if j else np.zeros((ch, qs.shape[2]), np.int32)
                    assert np.array_equal(got[s, :, j], w), f"{what}: stream {s}: the phases in front of tile {j}: {int(np.count_nonzero(got[s, :, j] != w))} differ"
        # (d) the handle on stream 0
        entry = "formant_shift" if phi is not None else "formant" if q else "n"
        y = stream(c, x[0].reshape(-1), ch, rate, pitch, put_sizes(case), entry, n_fft, flags=(LOCK if lock else 0) | (TR if tr else 0) | (LINK if link else 0),
                   lifter=q, device_put="alternate", formant_ratio=phi if phi is not None else 1.0)
        assert y.size == out[0].size, f"{what}: the handle gave {y.size} samples, the block call {out[0].size}"
        assert np.array_equal(bits(y), bits(out[0].reshape(-1))), f"{what}: the handle against the block call: {first_difference(y, out[0].reshape(-1))}"
    return worst


def main(cases=200, seed=1, ctx=None, nae=None):
    """-> the number of cases that passed (every case runs on a context of its own, which carries its pv_tile; ctx is not used)"""
    if nae is None:
        nae = lib()[0]
    done, worst = 0, 0.0
    for k, case in enumerate(draw(cases, seed)):
        e = run_case(nae, case)
        worst = max(worst, e)
        done += 1
        print(f"case {k:3d}: {describe(case)}  plan case {plan_case(case)}  kernels {' + '.join(expected_kernels(case)) or 'unflagged'}  sample error {e:.2e}", flush=True)
    print(f"pv options: {done} cases, worst sample error {worst:.2e} (tolerance {TOL:g})")
    return done


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
