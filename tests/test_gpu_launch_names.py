"""The launch layer, pinned: which kernels a block call launches, under which profile names and how often.

Every row is one block call with profiling on in a fresh context; the complete {profile name: launches} dictionary is compared with
tests/golden/launch_names.json.  The rows are the smallest shapes that still take every launcher of the tiled kernels — the vocoder at
every size, flag combination and layout (pass 1, scan and pass 3 all launch), the 1024-point pipeline in its six shapes, and the four
effect nodes — so a launcher that picks another instantiation's name, launches once more or once less, or drops a launch shows here.

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
    return out


ROWS = rows()
# run twice in one context: the second launch of a kernel with more than 64 KiB of dynamic LDS finds its attribute set
TWICE = ("pv 1024 lock+transients+link formant planar", "pipe fps=2 flow=0 interleaved")


def _sig(nae, ptr, L, layout):
    return nae.Sig.planar(ptr, L, CH) if layout == "planar" else nae.Sig.interleaved(ptr, L, CH)


def _call(nae, c, kind, a):
    """one block call of the row on context c (the signal is uniform noise: the launches do not depend on it)"""
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
