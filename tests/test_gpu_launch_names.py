"""The launch layer, pinned: which kernels a block call launches, under which profile names and how often.

Every row is one block call with profiling on in a fresh context; the complete {profile name: launches} dictionary is compared with
tests/golden/launch_names.json.  The rows are the smallest shapes that still take every launcher of the tiled kernels — the vocoder at
every size, flag combination and layout (pass 1, scan and pass 3 all launch), the 1024-point pipeline in its six shapes, and the four
effect nodes — so a launcher that picks another instantiation's name, launches once more or once less, or drops a launch shows here.
The "node" rows do the same for K1 - K8, the WSOLA chain and the input conversion, one row per branch of each launcher's variant pick
(nae_debug_diff_u32 launches outside the profile: its row pins that it stays there).

The golden file is not written by the library under test: it was recorded by running this file as a script
(python tests/test_gpu_launch_names.py --record tests/golden/launch_names.json) on the commit in front of the one that wrote the launch
layer once (its "recorded_on" entry names that commit), and a later change of the launches records it again the same way."""
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_names.json")
SIZES = (512, 1024, 2048, 4096)
PITCH = 2 ** (3 / 12)
N_STREAMS, CH, L_PV, L_FX = 2, 2, 40000, 5000
FLAGS = {"none": {}, "transients": {"transients": True}, "transients+link": {"transients": True, "link_channels": True}}
LOCK_FLAGS = {"lock": {"phase_lock": True}, "lock+transients": {"phase_lock": True, "transients": True},
              "lock+link": {"phase_lock": True, "link_channels": True},
              "lock+transients+link": {"phase_lock": True, "transients": True, "link_channels": True}}


def rows():
    """[(row id, kind, arguments)]"""
    out = []
    for layout in ("planar", "interleaved"):
        for n in SIZES:
            for fname, flags in {**FLAGS, **(LOCK_FLAGS if n == 1024 else {})}.items():
                for formant in (False, True):
                    out.append((f"pv {n} {fname}{' formant' if formant else ''} {layout}", "pv",
                                dict(n_fft=n, flags=flags, formant=formant, shift=False, layout=layout, debug={"pv_tile": 16})))
            out.append((f"pv {n} fshift {layout}", "pv", dict(n_fft=n, flags={}, formant=True, shift=True, layout=layout, debug={"pv_tile": 16})))
        for fps in (1, 2, 4):
            for flow in (0, 2):
                out.append((f"pipe fps={fps} flow={flow} {layout}", "pv",
                            dict(n_fft=1024, flags={}, formant=False, shift=False, layout=layout,
                                 debug={"pv_tile": 16, "pv_fps": fps, "pv_flow": flow})))
        for fx in ("fir", "conv", "eq", "dyn link=0", "dyn link=1"):
            out.append((f"{fx} {layout}", "fx", dict(fx=fx, layout=layout)))
    # K1 - K8, the WSOLA chain and the input conversion: one row per branch of each launcher's variant pick
    for mode in ("i2p", "p2i", "flat", "generic"):
        for scale in (False, True):
            out.append((f"copy_sig {mode}{' scaled' if scale else ''}", "node", dict(op="copy_sig", mode=mode, scale=scale)))
    for op in ("gain f32", "gain s16", "gain s32", "amix planes", "amix_sig fast", "amix_sig generic", "bimix", "downmix", "bimix2_interleave",
               "mono_to_stereo", "fill_uniform", "diff_u32", "swr"):
        out.append((op, "node", dict(op=op)))
    for fmt in ("FLT", "FLTP", "S16", "S16P", "S32", "S32P"):
        out.append((f"to_f32 {fmt}", "node", dict(op="to_f32", fmt=fmt)))
    out.append(("spectrum stereo", "node", dict(op="spectrum", layout="interleaved")))
    out.append(("spectrum generic unit stride", "node", dict(op="spectrum", layout="planar")))
    out.append(("spectrum generic frame stride 2", "node", dict(op="spectrum", layout="interleaved", debug={"spec_generic": 1})))
    for n in (256, 512, 1024, 2048, 4096):
        out.append((f"spectrum_any {n} hop {n // 2}", "node", dict(op="spectrum", layout="planar", n_fft=n, hop=n // 2)))
    out.append(("spectrum_any 512 hop 100 frame stride 2", "node", dict(op="spectrum", layout="interleaved", n_fft=512, hop=100)))
    out.append(("transposer stereo group of 4", "node", dict(op="transposer", ch=2, n_streams=4, rate=1.25)))
    out.append(("transposer stereo alone", "node", dict(op="transposer", ch=2, n_streams=2, rate=1.25)))
    out.append(("transposer mono", "node", dict(op="transposer", ch=1, n_streams=2, rate=1.25)))
    out.append(("transposer direct", "node", dict(op="transposer", ch=2, n_streams=2, rate=4101 / 512)))
    out.append(("graph4 front stage: fused mix", "node", dict(op="graph4 front")))
    for ch in (1, 2):
        for name, rate, pitch in (("below 1", 0.8, 1.0), ("at 1", 0.5, 2.0), ("above 1", 1.25, 1.0)):    # effective rate = rate * pitch
            out.append((f"wsola ch={ch} rate {name} nc=2", "node", dict(op="wsola", ch=ch, rate=rate, pitch=pitch, sr=48000, debug={"td_nc": 2})))
        out.append((f"wsola ch={ch} rate above 1 nc=4", "node", dict(op="wsola", ch=ch, rate=1.25, pitch=1.0, sr=48000, debug={"td_nc": 4})))
        # the block call fuses the cubic stage into the filter's launch; st_unfused gives it a launch of its own
        out.append((f"wsola ch={ch} rate above 1 unfused", "node", dict(op="wsola", ch=ch, rate=1.25, pitch=1.0, sr=48000, debug={"st_unfused": 1})))
    out.append(("wsola ch=2 44.1 kHz nc=4", "node", dict(op="wsola", ch=2, rate=1.25, pitch=1.0, sr=44100, debug={"td_nc": 4})))
    return out


ROWS = rows()
# run twice in one context: the second launch of a kernel with more than 64 KiB of dynamic LDS finds its attribute set
TWICE = ("pv 1024 lock+transients+link formant planar", "pipe fps=2 flow=0 interleaved")


def _sig(nae, ptr, L, layout):
    return nae.Sig.planar(ptr, L, CH) if layout == "planar" else nae.Sig.interleaved(ptr, L, CH)


def _node(nae, c, a):
    """one call of a K1 - K8, WSOLA or conversion row on context c: the buffers are made first, the call alone is profiled"""
    import ctypes as C
    op, L, N = a["op"], L_FX, N_STREAMS
    bufs = []

    def dev(n, dtype=np.float32):
        d = c.empty(n, dtype)
        if dtype == np.float32:
            c.fill_uniform(d.ptr, n, n, 1, 0, len(bufs))
        else:
            d.zero()
        bufs.append(d)
        return d

    def inter(d, length, ch=CH):
        return nae.Sig.interleaved(d.ptr, length, ch)

    if op == "copy_sig":
        x, o = dev(N * L * CH), dev(N * (L + 1) * CH)
        src = nae.Sig.planar(x.ptr, L, CH) if a["mode"] == "p2i" else inter(x, L)
        dst = {"i2p": nae.Sig.planar(o.ptr, L, CH), "p2i": inter(o, L), "flat": inter(o, L),
               "generic": nae.Sig.planar(o.ptr, L, CH, plane_stride=L + 1)}[a["mode"]]      # planes that are not 16-byte aligned
        run = (lambda: c.gain_sig(src, dst, L, CH, N, 0.5)) if a["scale"] else (lambda: c.copy_sig(src, dst, L, CH, N))
    elif op.startswith("gain "):
        dt = {"f32": np.float32, "s16": np.int16, "s32": np.int32}[op[5:]]
        x, o = dev(L, dt), dev(L, dt)
        run = lambda: c.gain(dt, [x.ptr], [o.ptr], L, 0.5)
    elif op == "amix planes":
        p = [dev(L) for _ in range(6)]
        run = lambda: c.amix([p[0].ptr, p[1].ptr], [p[2].ptr, p[3].ptr], [0.5, 0.25], p[4].ptr, p[5].ptr, L)
    elif op.startswith("amix_sig"):
        x, y, o = dev(N * L * CH), dev(N * L * CH), dev(N * L * CH)
        dst = nae.Sig.planar(o.ptr, L, CH) if op.endswith("fast") else inter(o, L)
        run = lambda: c.amix_sig([inter(x, L), inter(y, L)], [0.5, 0.25], dst, L, N)
    elif op == "bimix":
        p = [dev(L) for _ in range(6)]
        run = lambda: c.bimix(p[0].ptr, p[1].ptr, p[2].ptr, p[3].ptr, 0.25, p[4].ptr, p[5].ptr, L)
    elif op == "downmix":
        p = [dev(L) for _ in range(3)]
        run = lambda: c.bimix2_downmix(p[0].ptr, p[1].ptr, p[2].ptr, L)
    elif op == "bimix2_interleave":
        e, l, o = dev(L), dev(L), dev(2 * L)
        run = lambda: c.bimix2_interleave(o.ptr, e.ptr, l.ptr, 100, L - 100, 0)
    elif op == "mono_to_stereo":
        m, o = dev(L), dev(2 * L)
        run = lambda: c._ck(c.lib.nae_mono_to_stereo_f32(c.h, m.ptr, o.ptr, L, 0.5))
    elif op == "fill_uniform":
        x = dev(N * L)
        run = lambda: c.fill_uniform(x.ptr, L, L, N, 0, 0)
    elif op == "diff_u32":
        x, y, cnt = dev(L), dev(L), dev(1, np.uint64)
        run = lambda: c.diff_words(x.ptr, y.ptr, L, cnt.ptr)
    elif op == "to_f32":
        fmt = a["fmt"]
        x = dev(L * CH, {"FLT": np.float32, "S16": np.int16, "S32": np.int32}[fmt.rstrip("P")])
        planes = [x.at(0), x.at(L)] if fmt.endswith("P") else [x.ptr]
        o = dev(L * CH)

        def run():
            assert c.to_f32_interleaved(getattr(nae, "FMT_" + fmt), planes, L, CH, o.ptr) == 0
    elif op == "swr":
        host = np.zeros(2 * 4410, np.float32)

        def run():
            h, got = C.c_void_p(), C.c_size_t()
            outL, outR = np.zeros(6000, np.float32), np.zeros(6000, np.float32)
            assert c.lib.nae_swr_create(c.h, nae.FMT_FLT, 44100, 2, 48000, C.byref(h)) == 0
            assert c.lib.nae_swr_convert_host(h, (C.c_void_p * 1)(host.ctypes.data), 4410, outL.ctypes.data, outR.ctypes.data, 6000, C.byref(got)) == 0
            assert got.value > 0 and c.lib.nae_swr_destroy(h) == 0
    elif op == "spectrum":
        x = dev(N * L * CH)
        src = _sig(nae, x.ptr, L, a["layout"])
        n, hop = a.get("n_fft", 1024), a.get("hop", 256)
        F = c.spectrum_frames_ex(L, n, hop)
        assert F > 0
        o = dev(N * F * CH * (n // 2 + 1))
        if "n_fft" in a:
            run = lambda: c.spectrum_block_ex(n, hop, src, L, CH, N, o.ptr, F * CH * (n // 2 + 1))
        else:
            run = lambda: c.spectrum_block(src, L, CH, N, o.ptr, F * CH * 513)
    elif op == "transposer":
        ch, n, rate = a["ch"], a["n_streams"], a["rate"]
        pl = c.stretch_plan(rate, 1.0, L)
        assert pl.rs_on and not pl.pv_on
        x, o = dev(n * L * ch), dev(n * pl.out_len * ch)
        run = lambda: c.stretch_block(rate, 1.0, inter(x, L, ch), L, ch, n, inter(o, pl.out_len, ch))
    elif op == "graph4 front":
        pl = c.stretch_plan(1.0, PITCH, L)
        F = c.spectrum_frames(pl.out_len)
        x, y, mix, pitch, spec = dev(N * L * 2), dev(N * L * 2), dev(N * L * 2), dev(N * pl.out_len * 2), dev(N * F * 2 * 513)
        g = nae.Graph4()
        g.in_a, g.in_b, g.vol_a, g.vol_b = inter(x, L), inter(y, L), 0.5, 0.5
        g.mix_out, g.rate, g.pitch, g.pitch_out = nae.Sig.planar(mix.ptr, L, 2), 1.0, PITCH, inter(pitch, pl.out_len)
        g.spec_out, g.spec_stream_stride, g.S, g.n_streams = spec.ptr, F * 2 * 513, L, N
        run = lambda: c.graph4_stages(g, 1)
    else:
        assert op == "wsola", op
        ch, Lw = a["ch"], L_PV
        pl = c.wsola_plan(a["sr"], ch, a["rate"], a["pitch"], Lw)
        x, o = dev(N * Lw * ch), dev(max(1, N * pl.out_len * ch))
        run = lambda: c.wsola_block(a["sr"], a["rate"], a["pitch"], inter(x, Lw, ch), Lw, ch, N, inter(o, pl.out_len, ch))
    c.sync()
    c.prof_reset()
    c.prof_enable(True)
    run()
    c.sync()
    c.prof_enable(False)
    for d in bufs:
        d.free()


def _call(nae, c, kind, a):
    """one block call of the row on context c (the signal is uniform noise: the launches do not depend on it)"""
    if kind == "node":
        return _node(nae, c, a)
    L = L_PV if kind == "pv" else L_FX
    d_x = c.empty(N_STREAMS * L * CH)
    c.fill_uniform(d_x.ptr, L * CH, L * CH, N_STREAMS, 0, 0)
    src = _sig(nae, d_x.ptr, L, a["layout"])
    c.prof_reset()
    c.prof_enable(True)
    if kind == "pv":
        n = a["n_fft"]
        lifter = nae.formant_lifter(48000, n) if a["formant"] else 0
        rate, pitch, ratio = (1.0, 1.0, 1.25) if a["shift"] else (1.0, PITCH, None)
        pl = c.stretch_plan(rate, pitch, L, n, formant=lifter, formant_ratio=ratio)
        d_o = c.empty(N_STREAMS * pl.out_len * CH)
        c.stretch_block(rate, pitch, src, L, CH, N_STREAMS, _sig(nae, d_o.ptr, pl.out_len, a["layout"]), n_fft=n, formant=lifter,
                        formant_ratio=ratio, **a["flags"])
    else:
        d_o = c.empty(N_STREAMS * L * CH)
        dst = _sig(nae, d_o.ptr, L, a["layout"])
        fx = a["fx"]
        if fx == "fir":
            c.fir_block(c.fir_design("lowpass", 48000, 0.0, 8000.0, 33), src, L, CH, N_STREAMS, dst, n_fft=512)
        elif fx == "conv":
            c.conv_block(np.linspace(1.0, 0.0, 1000, dtype=np.float32), src, L, CH, N_STREAMS, dst, n_fft=512)
        elif fx == "eq":
            c.eq_block(np.stack([c.eq_design("peak", 48000, 1000.0, 6.0), c.eq_design("highpass", 48000, 80.0)]), src, L, CH, N_STREAMS, dst)
        else:
            c.dyn_block(c.dyn_design(48000, link=fx.endswith("1")), src, L, CH, N_STREAMS, dst)
    c.sync()
    c.prof_enable(False)
    d_x.free()
    d_o.free()


def launches(nae, ids):
    """{profile name: launches} of the rows `ids`, run one after the other in ONE fresh context"""
    table = {rid: (kind, a) for rid, kind, a in ROWS}
    total = {}
    with nae.Context(0) as c:
        for rid in ids:
            kind, a = table[rid]
            for key, value in a.get("debug", {}).items():
                c.debug_set(key, value)
            _call(nae, c, kind, a)
            for name, (_, count) in c.prof_report().items():
                total[name] = total.get(name, 0) + int(count)
    return dict(sorted(total.items()))


def twice_id():
    return "twice: " + " + ".join(TWICE)


@pytest.fixture(scope="module")
def golden_names():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def test_rows_are_the_recorded_ones(golden_names):
    assert sorted(golden_names) == sorted([rid for rid, _, _ in ROWS] + [twice_id()])


@pytest.mark.gpu
@pytest.mark.parametrize("rid", [rid for rid, _, _ in ROWS])
def test_gpu_launch_names(nae, golden_names, rid):
    got = launches(nae, [rid])
    print(rid, got)
    assert got == golden_names[rid]


@pytest.mark.gpu
def test_gpu_launch_names_twice_in_one_context(nae, golden_names):
    got = launches(nae, list(TWICE) * 2)
    print(got)
    assert got == golden_names[twice_id()]


if __name__ == "__main__":
    assert len(sys.argv) == 4 and sys.argv[1] == "--record", "usage: test_gpu_launch_names.py --record OUT.json 'COMMIT the library was built from'"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import naeload
    nae_ = naeload.load()
    rec = {rid: launches(nae_, [rid]) for rid, _, _ in ROWS}
    rec[twice_id()] = launches(nae_, list(TWICE) * 2)
    with open(sys.argv[2], "w") as f:
        json.dump({"recorded_by": "python tests/test_gpu_launch_names.py --record, with the library built from the commit in recorded_on",
                   "recorded_on": sys.argv[3], "rows": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} rows recorded")
