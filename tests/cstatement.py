"""The one compile line of the CPU statements (tests/fir_ref.py, conv_ref.py, eq_ref.py, dyn_ref.py, pv_ref.py).  The suite's bit-equality
claims rest on every statement being built with these flags: no contraction into fused multiply-adds, no fast-math."""
import ctypes as C
import os
import subprocess


def build(src, out_dir, extra=()):
    """src: a statement's C file -> its shared library lib<name>.so in out_dir, loaded; extra: link flags in front of -lm"""
    so = os.path.join(out_dir, "lib" + os.path.splitext(os.path.basename(src))[0] + ".so")
    r = subprocess.run(["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", src, "-o", so, *extra, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(so)
