#!/usr/bin/env python3
"""Randomised differential run (GPU box) of the graph step input -> mix(2) -> pitch -> spectrum (nae_graph4_run) in every split the library
offers, at ragged lengths and drawn layouts.  One generator (draw -> plain case records, no device needed) draws the length, the stream count,
rate and pitch, the volumes and a full layout per signal: a base offset of 0 ... 3 floats and strides that are either padded up to a multiple
of 4 (so that a length that is no multiple of 4 still reaches the 16-byte routes) or forced to 1, 2, 3 (mod 4).  expected_route restates the
fuse rule of nae_launch_mix_resample, the tile rule of rs_pick_tile and the `fast` rule of nae_amix_sig_f32, and names the kernels the front
stage (the mix node, and the transposer where it runs first) must launch.  run_case runs the record four ways into separate buffers that were
filled with a sentinel:
    D0  nae_graph4_run
    D1  nae_graph4_run under debug_set("no_mix_fuse", 1)
    D2  nae_amix_sig_f32 -> nae_stretch_block_f32 -> nae_spectrum_block_f32 on the same views
    D3  nae_debug_graph4_stages with mask 1, then 2, then 4
and asserts (a) the kernels D0 launched (and D1's, and those of D3's first stage) are the expected ones, (b) the mix bit-exact against orc.amix
in every split, (c) mix, pitch and spectrum bit-identical across D0 ... D3, (d) the pitch within 1e-4 of orc.stretch of the oracle's mix, measured
against max(RMS, 1e-4) as tests/tools/fuzz_tiny.py does, (e) the spectrum bit-exact against orc.spectrum of the pitch that was delivered and
(f) the sentinel in every word outside the three destination views.  D2 is the route the rest of the suite pins to the oracle: where (c) fails
while (b) holds, the split that departs from D2 is the one at fault.  tests/test_fuzz_graph_cpu.py pins, without a GPU, what SEEDED draws.
    python tests/tools/fuzz_graph.py [cases=200] [seed=1]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SEEDED = (24, 4)                                                # (cases, seed) of tests/test_gpu_fuzz.py::test_fuzz_graph_seeded
RS_TAPS = 16                                                     # NAE_RS_TAPS
TILE_WIDE, TILE = 768, 512                                       # kRsOutWide, kRsOut
FUSE_SPAN, RS_MAX_SPAN = 1536, 4096 + 32                         # the 4-stream staging row; kRsMaxSpan
PER_LAUNCH = 65535 * 4                                           # streams one launch of the fused kernel indexes
SENTINEL = np.float32(7.0)                                       # no output reaches it: the mix stays within 0.5 (signals)
TOL = 1e-4
BINS = 513
FRONT = ("mix_resample_tile_kernel", "amix_i2p_kernel", "amix_generic_kernel", "resample_tile_kernel", "resample_kernel")
# why nae_launch_mix_resample refuses a graph whose transposer runs first
REASONS = ("a_base", "a_stride", "b_base", "b_stride", "mix_base", "mix_stride", "mix_plane", "rho")
VOLUMES = ((0.5, 0.5), (0.0, 0.0), (0.0, 0.7), (-0.5, 1.0), (1.0, 1.0), (0.3, 0.9))
TINY = (1, 2, 3, 5, 15, 16, 17, 29)                              # around the 16 taps
# the class of case k is PLAN[k % len(PLAN)]: every second case is meant for the fused kernel, every reason to refuse it comes once in 24
PLAN = ("fused", "a_base", "fused", "tiny", "fused", "b_base", "fused", "a_stride", "fused", "rho", "fused", "mix_plane",
        "fused", "b_stride", "fused", "tiny", "fused", "mix_base", "fused", "mix_stride", "fused", "pv_first", "fused", "tiny")


def pick(rng, options):
    return options[int(rng.integers(len(options)))]


def pad4(n):
    return (n + 3) & ~3


# ---------------------------------------------------------------------------------------------------- the record
def make_case(S, n_streams, rate=1.0, pitch=2.0 ** (3 / 12), vols=(0.5, 0.5), planar=True, shared_b=True, a_base=0, a_pad=0, b_base=0, b_pad=0,
              mix_base=0, plane_pad=0, mix_pad=0, pitch_base=0, pitch_pad=0, spec_gap=0, seed=1, label=""):
    """a record with every stride padded up to a multiple of 4, plus the given pads: in_a / in_b interleaved with stream stride
    pad4(2 S) + a_pad / b_pad (in_b: 0 where shared), a planar mix of plane stride pad4(S) + plane_pad and stream stride
    pad4(2 plane) + mix_pad or an interleaved one of stream stride pad4(2 S) + mix_pad; bases in floats behind a 16-byte aligned address"""
    cs = pad4(S) + plane_pad if planar else 1
    return dict(label=label, S=int(S), n_streams=int(n_streams), rate=float(rate), pitch=float(pitch), vols=(float(vols[0]), float(vols[1])),
                a=dict(base=a_base, ss=pad4(2 * S) + a_pad), b=dict(base=b_base, ss=0 if shared_b else pad4(2 * S) + b_pad),
                mix=dict(base=mix_base, ss=pad4(2 * cs if planar else 2 * S) + mix_pad, cs=cs, fs=1 if planar else 2),
                pitch_out=dict(base=pitch_base, pad=pitch_pad), spec_gap=int(spec_gap), seed=int(seed))


def draw_one(rng, kind):
    r = int(pick(rng, (1, 2, 3, 1, 2, 3, 0)))
    S = int(pick(rng, TINY)) if kind == "tiny" else 4 * int(rng.integers(150, 1500)) + r
    pitch = float(pick(rng, (2.0 ** (3 / 12), 2.0 ** (5 / 12), 2.0, 1.0005, 1508 / 768, 1509 / 768, 1508 / 512,
                             float(np.exp(rng.uniform(np.log(1.03), np.log(2.3)))), float(np.exp(rng.uniform(np.log(1.03), np.log(2.3)))))))
    rate = float(pick(rng, (1.0, 1.0, 1.0, 1.25, 0.8)))
    if not 1.0 < rate * pitch <= 1508 / 512:
        rate = 1.0
    if kind == "rho":
        rate, pitch = 1.0, float(pick(rng, (1509 / 512, rng.uniform(2.95, 3.9))))
    if kind == "pv_first":                                       # the vocoder first, the transposer alone, or neither
        rate, pitch = pick(rng, ((1.0, 2.0 ** (-4 / 12)), (1.5, 1.0), (1.0, 1.0), (0.8, 2.0 ** (-2 / 12))))
    planar = bool(rng.integers(2)) or kind in ("mix_base", "mix_stride", "mix_plane")
    shared = bool(rng.integers(3) == 0) and kind != "b_stride"
    case = make_case(S, int(rng.integers(1, 8)), rate, pitch, pick(rng, VOLUMES), planar, shared,
                     a_base=4 * int(rng.integers(3)), a_pad=4 * int(pick(rng, (0, 0, 1, 3))), b_base=4 * int(rng.integers(3)),
                     b_pad=4 * int(pick(rng, (0, 0, 1, 3))), mix_base=4 * int(rng.integers(3)) if planar else int(rng.integers(4)),
                     plane_pad=4 * int(pick(rng, (0, 0, 2))), mix_pad=4 * int(pick(rng, (0, 1))) if planar else int(pick(rng, (0, 1, 2, 3, 5))),
                     pitch_base=int(pick(rng, (0, 0, 2, 2, 1, 3))), pitch_pad=int(pick(rng, (0, 0, 1, 2, 6))), spec_gap=int(pick(rng, (0, 0, 1, 6, 513))),
                     seed=int(rng.integers(1 << 31)), label=kind)
    off = int(pick(rng, (1, 2, 3)))                              # what takes the layout off the 16-byte route
    if kind in ("a_base", "b_base", "mix_base"):
        case[kind[:-5]]["base"] += off
    elif kind in ("a_stride", "b_stride", "mix_stride"):
        case[kind[:-7]]["ss"] += off
    elif kind == "mix_plane":
        case["mix"]["cs"] += off
        case["mix"]["ss"] = pad4(2 * case["mix"]["cs"])
    return case


def draw(cases, seed):
    """the records a run of `cases` cases at `seed` makes, in order; needs no device"""
    rng = np.random.default_rng(seed)
    for k in range(cases):
        yield draw_one(rng, PLAN[k % len(PLAN)])


def describe(case):
    v = lambda d: " ".join(f"{k} {d[k]}" for k in d)
    return (f"[{case['label']}] S {case['S']} streams {case['n_streams']} rate {case['rate']:.6g} pitch {case['pitch']:.6g} vols {case['vols']} "
            f"a ({v(case['a'])}) b ({v(case['b'])}) mix ({v(case['mix'])}) pitch_out ({v(case['pitch_out'])}) spec gap {case['spec_gap']}")


# ---------------------------------------------------------------------------------------------------- the route rule
def plan_of(nae, case):
    return nae.Context.stretch_plan(case["rate"], case["pitch"], case["S"])


def tile_rule(step_q32):
    """rs_pick_tile: (output frames per transposer workgroup, the staging row it needs)"""
    rho = step_q32 / 4294967296.0
    need = lambda tile: int(tile * rho) + RS_TAPS + 8 + 4
    tile = TILE_WIDE if need(TILE_WIDE) <= FUSE_SPAN else TILE
    return tile, need(tile)


def refusals(nae, case):
    """the reasons (of REASONS, or "empty") for which nae_launch_mix_resample would not fuse this record; none: it fuses"""
    pl = plan_of(nae, case)
    a, b, mix = case["a"], case["b"], case["mix"]
    why = [f"{name}_{what}" for name, v in (("a", a), ("b", b)) for what, bad in (("base", v["base"] % 4), ("stride", v["ss"] % 4)) if bad]
    if mix["fs"] == 1:
        why += [f"mix_{what}" for what, bad in (("base", mix["base"] % 4), ("stride", mix["ss"] % 4), ("plane", mix["cs"] % 4)) if bad]
    span_need = tile_rule(pl.step_q32)[1]
    if span_need > RS_MAX_SPAN or pad4(span_need) > FUSE_SPAN:
        why.append("rho")
    if case["n_streams"] == 0 or case["S"] == 0 or pl.mid_len == 0:
        why.append("empty")
    return why


def amix_kernel(case):
    """nae_amix_sig_f32's `fast`: a planar output and interleaved inputs, every base 16-byte aligned, every stream and plane stride a multiple of 4"""
    mix = case["mix"]
    fast = mix["fs"] == 1 and mix["base"] % 4 == 0 and mix["ss"] % 4 == 0 and mix["cs"] % 4 == 0
    fast = fast and all(v["base"] % 4 == 0 and v["ss"] % 4 == 0 for v in (case["a"], case["b"]))
    return "amix_i2p_kernel" if fast else "amix_generic_kernel"


def expected_route(nae, case, fuse=True):
    """the kernels the front stage launches (fuse=False: under debug_set("no_mix_fuse", 1)), as a sorted tuple of names"""
    pl = plan_of(nae, case)
    if case["S"] == 0 or case["n_streams"] == 0:
        return ()
    if pl.out_len and pl.rs_first:
        if fuse and not refusals(nae, case):
            return ("mix_resample_tile_kernel",)
        if pl.mid_len:
            return tuple(sorted((amix_kernel(case), "resample_tile_kernel" if tile_rule(pl.step_q32)[1] <= RS_MAX_SPAN else "resample_kernel")))
    return (amix_kernel(case),)


def back_transposer(nae, case):
    """the transposer's kernel where it runs behind the front stage (the vocoder first, or no vocoder), else none"""
    pl = plan_of(nae, case)
    if case["S"] == 0 or case["n_streams"] == 0 or pl.out_len == 0 or not pl.rs_on or pl.rs_first:
        return ()
    return ("resample_tile_kernel" if tile_rule(pl.step_q32)[1] <= RS_MAX_SPAN else "resample_kernel",)


# ---------------------------------------------------------------------------------------------------- layouts and signals
def geometry(nae, case):
    """the views as index arrays into their buffers ([stream, channel, frame] -> float offset) and the buffers' sizes in floats"""
    pl = plan_of(nae, case)
    S, n, T = case["S"], case["n_streams"], int(pl.out_len)
    F = 0 if T < 1024 else (T - 1024) // 256 + 1                 # nae_spectrum_frames
    s, c = np.arange(n, dtype=np.int64)[:, None, None], np.arange(2, dtype=np.int64)[None, :, None]
    i, t = np.arange(S, dtype=np.int64)[None, None, :], np.arange(T, dtype=np.int64)[None, None, :]
    a, b, mix, po = case["a"], case["b"], case["mix"], case["pitch_out"]
    g = dict(pl=pl, T=T, F=F, pitch_ss=2 * T + po["pad"], spec_ss=F * 2 * BINS + case["spec_gap"])
    g["a"] = a["base"] + s * a["ss"] + c + 2 * i
    g["b"] = b["base"] + s * b["ss"] + c + 2 * i
    g["mix"] = mix["base"] + s * mix["ss"] + c * mix["cs"] + i * mix["fs"]
    g["pitch"] = po["base"] + s * g["pitch_ss"] + c + 2 * t
    g["spec"] = (s * g["spec_ss"] + np.arange(F * 2 * BINS, dtype=np.int64)[None, None, :])[:, 0, :]
    for k in ("a", "b", "mix", "pitch", "spec"):
        g["n_" + k] = (int(g[k].max()) + 1 if g[k].size else 0) + 9      # room behind the last element: a write past the view lands in the buffer
    return g


def signals(case, g):
    """the two input buffers: the views' contents [stream, channel, frame] from the record's seed alone (records that differ in layout only carry
    the same signals; a shared in_b: stream 0's for every stream), other values in the gaps between the views.  Uniform within
    0.5 / max(1, |va| + |vb|), so that the mix, which is what the vocoder reads, stays within the amplitude of 0.5 of tests/tools/fuzz_tiny.py: the
    floor of 1e-4 under the pitch error's denominator is an absolute bound of 1e-8, the rounding noise of outputs on the window's edge at that
    amplitude (at S = 5 the oracle's own output, RMS 2e-8 for a mix of amplitude 0.9, moves by 4e-9 when its input moves by one ulp)"""
    rng, gaps = np.random.default_rng(case["seed"]), np.random.default_rng(case["seed"] + 1)
    amp = 0.5 / max(1.0, abs(case["vols"][0]) + abs(case["vols"][1]))
    bufs = []
    for key in ("a", "b"):
        x = rng.uniform(-amp, amp, g[key].shape).astype(np.float32)
        if case[key]["ss"] == 0:
            x[:] = x[:1]
        buf = gaps.uniform(-1, 1, g["n_" + key]).astype(np.float32)
        buf[g[key]] = x
        bufs.append(buf)
    return bufs


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def first_difference(a, b):
    at = np.flatnonzero(bits(a) != bits(b))
    return f"{at.size} words differ, the first at float {int(at[0])}: {a[at[0]]!r} against {b[at[0]]!r}" if at.size else "equal"


def graph_of(nae, case, g, d_a, d_b, d_mix, d_pitch, d_spec):
    a, b, mix, po = case["a"], case["b"], case["mix"], case["pitch_out"]
    G = nae.Graph4()
    G.in_a = nae.Sig(d_a.at(a["base"]), a["ss"], 1, 2)
    G.in_b = nae.Sig(d_b.at(b["base"]), b["ss"], 1, 2)
    G.vol_a, G.vol_b = case["vols"]
    G.mix_out = nae.Sig(d_mix.at(mix["base"]), mix["ss"], mix["cs"], mix["fs"])
    G.rate, G.pitch = case["rate"], case["pitch"]
    G.pitch_out = nae.Sig(d_pitch.at(po["base"]), g["pitch_ss"], 1, 2)
    G.spec_out, G.spec_stream_stride = d_spec.ptr, g["spec_ss"]
    G.S, G.n_streams = case["S"], case["n_streams"]
    return G


def launched(ctx, call):
    """the names of the kernels `call` launches"""
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        call()
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    return tuple(sorted(ctx.prof_report()))


SPLITS = ("D0 graph4", "D1 graph4 no_mix_fuse", "D2 node by node", "D3 stages 1, 2, 4")


def run_case(nae, ctx, case, verbose=False):
    """the record through D0 ... D3 under the assertions (a) ... (f) of the module's docstring -> the worst pitch error (verbose: every stream's
    pitch error is printed before it is asserted)"""
    import orc
    what = describe(case)
    g = geometry(nae, case)
    pl, S, n, T, F = g["pl"], case["S"], case["n_streams"], g["T"], g["F"]
    host_a, host_b = signals(case, g)
    d_a, d_b = ctx.array(host_a), ctx.array(host_b)
    routes, outs = {}, []
    for split in range(4):
        bufs = [ctx.array(np.full(g["n_" + k], SENTINEL, np.float32)) for k in ("mix", "pitch", "spec")]
        G = graph_of(nae, case, g, d_a, d_b, *bufs)
        if split == 0:
            routes["D0"] = launched(ctx, lambda: ctx.graph4(G))
        elif split == 1:
            ctx.debug_set("no_mix_fuse", 1)
            try:
                routes["D1"] = launched(ctx, lambda: ctx.graph4(G))
            finally:
                ctx.debug_set("no_mix_fuse", 0)
        elif split == 2:
            ctx.amix_sig([G.in_a, G.in_b], case["vols"], G.mix_out, S, n)
            ctx.stretch_block(case["rate"], case["pitch"], G.mix_out, S, 2, n, G.pitch_out)
            ctx.spectrum_block(G.pitch_out, T, 2, n, G.spec_out, G.spec_stream_stride)
        else:
            routes["D3 front"] = launched(ctx, lambda: ctx.graph4_stages(G, 1))
            ctx.graph4_stages(G, 2)
            ctx.graph4_stages(G, 4)
        ctx.sync()
        outs.append([d.download() for d in bufs])
        for d in bufs:
            d.free()
    d_a.free(); d_b.free()
    # (a) the route
    want, unfused, back = expected_route(nae, case), expected_route(nae, case, fuse=False), back_transposer(nae, case)
    front = lambda names, behind=(): tuple(k for k in names if k in FRONT and k not in behind)
    assert front(routes["D0"], back) == want and set(back) <= set(routes["D0"]), f"{what}: D0 launched {routes['D0']}, the front stage is {want}"
    assert front(routes["D1"], back) == unfused and set(back) <= set(routes["D1"]), f"{what}: D1 launched {routes['D1']}, the front stage is {unfused}"
    assert routes["D3 front"] == want, f"{what}: stage mask 1 launched {routes['D3 front']}, the front stage is {want}"
    # (b) the mix against the oracle, (f) the sentinel outside the views
    xa, xb = host_a[g["a"]], host_b[g["b"]]
    ref_mix = np.empty((n, 2, S), np.float32)
    for s in range(n):
        ref_mix[s] = orc.amix([xa[s, 0], xb[s, 0]], [xa[s, 1], xb[s, 1]], list(case["vols"]))
    for name, (mix, pitch, spec) in zip(SPLITS, outs):
        assert np.array_equal(bits(mix[g["mix"]]), bits(ref_mix)), f"{what}: {name}: mix against orc.amix: {first_difference(mix[g['mix']].ravel(), ref_mix.ravel())}"
        for key, buf in (("mix", mix), ("pitch", pitch), ("spec", spec)):
            outside = np.ones(buf.size, bool)
            outside[g[key].ravel()] = False
            hit = np.flatnonzero(outside & (bits(buf) != bits(SENTINEL)))
            assert hit.size == 0, f"{what}: {name}: {hit.size} words of the {key} buffer outside the view were written, the first at float {int(hit[0])}"
    # (c) the splits against D2
    for name, out in zip(SPLITS, outs):
        for key, got, ref in zip(("mix", "pitch", "spec"), out, outs[2]):
            assert np.array_equal(bits(got), bits(ref)), f"{what}: {key} of {name} against D2: {first_difference(got, ref)}"
    # (d) the pitch within the tolerance, (e) the spectrum of the pitch that was delivered
    worst = 0.0
    for s in range(n if T else 0):
        ref = orc.stretch(np.ascontiguousarray(ref_mix[s].T).reshape(-1), 2, case["rate"], case["pitch"])
        assert ref.size == 2 * T, (what, ref.size, T)
        den = max(np.sqrt(np.mean(ref.astype(np.float64) ** 2)), 1e-4)
        for name, (_, pitch, spec) in zip(SPLITS, outs):
            got = np.ascontiguousarray(pitch[g["pitch"][s]].T).reshape(-1)
            e = float(np.sqrt(np.mean((got.astype(np.float64) - ref) ** 2)) / den)
            worst = max(worst, e)
            if verbose and name == SPLITS[2]:
                print(f"    stream {s}: pitch error {e:.3e} (RMS of the reference {den:.3e})", flush=True)
            assert e <= TOL, f"{what}: {name}: stream {s}: pitch error {e:.3e} (RMS of the reference {den:.3e})"
            if F:
                assert np.array_equal(bits(spec[g["spec"][s]]), bits(orc.spectrum(got, 2).reshape(-1))), f"{what}: {name}: stream {s}: spectrum against orc.spectrum"
    return worst


def run_front_only(nae, ctx, case):
    """the front stage alone (stage mask 1: no vocoder, no oracle) for more streams than one launch indexes: the route, its launch count, the
    mix of every stream against the numpy statement of (0 + a va) + b vb, and the sentinel outside the view"""
    what = describe(case)
    g = geometry(nae, case)
    host_a, host_b = signals(case, g)
    d_a, d_b = ctx.array(host_a), ctx.array(host_b)
    bufs = [ctx.array(np.full(g["n_" + k], SENTINEL, np.float32)) for k in ("mix", "pitch", "spec")]
    G = graph_of(nae, case, g, d_a, d_b, *bufs)
    route = launched(ctx, lambda: ctx.graph4_stages(G, 1))
    report = ctx.prof_report()
    mix, pitch, spec = (d.download() for d in bufs)
    for d in [d_a, d_b] + bufs:
        d.free()
    want = expected_route(nae, case)
    assert route == want, f"{what}: stage mask 1 launched {route}, the front stage is {want}"
    if want == ("mix_resample_tile_kernel",):
        assert report[want[0]][1] == -(-case["n_streams"] // PER_LAUNCH), report
    va, vb = (np.float32(v) for v in case["vols"])
    ref = ((np.float32(0) + host_a[g["a"]] * va).astype(np.float32) + (host_b[g["b"]] * vb).astype(np.float32)).astype(np.float32)
    assert np.array_equal(bits(mix[g["mix"]]), bits(ref)), f"{what}: mix: {first_difference(mix[g['mix']].ravel(), ref.ravel())}"
    outside = np.ones(mix.size, bool)
    outside[g["mix"].ravel()] = False
    assert np.array_equal(bits(mix[outside]), bits(np.full(int(outside.sum()), SENTINEL))), f"{what}: words outside the mix view were written"
    assert np.array_equal(bits(pitch), bits(np.full(pitch.size, SENTINEL))) and np.array_equal(bits(spec), bits(np.full(spec.size, SENTINEL))), what


def main(cases=200, seed=1, ctx=None, nae=None):
    if nae is None:
        import naeload
        nae = naeload.load()
    if ctx is None:
        ctx = nae.Context(0)
    done, worst = 0, 0.0
    for k, case in enumerate(draw(cases, seed)):
        e = run_case(nae, ctx, case)
        worst = max(worst, e)
        done += 1
        print(f"case {k:3d}: {describe(case)}  route {' + '.join(expected_route(nae, case)) or 'nothing'}  splits bit-identical, pitch {e:.2e}", flush=True)
    print(f"graph: {done} cases, worst pitch error {worst:.2e}")
    return done


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
