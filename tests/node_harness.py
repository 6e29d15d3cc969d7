"""Builds a host node harness (tests/pv_ref/host_pv_node.cpp, tests/spec_sizes/host_spectrum.cpp and the four effect nodes'
tests/*_ref/host_*_node.cpp; all include tests/node_harness.hpp) against a current library and host archive, with the flags of
tests/host/Makefile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nodey-audio-editor_amd")


def build(src, out_dir):
    """src: the harness's path under tests/; returns the executable's path"""
    for d in (PKG, os.path.join(PKG, "host")):
        r = subprocess.run(["make", "-C", d, "-j4"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exe = os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0])
    cmd = ["g++", "-O1", "-g", "-std=c++20", "-pthread", "-Wall", "-Wno-unused-parameter", "-I" + os.path.join(PKG, "host"),
           "-I" + os.path.join(ROOT, "include"), "-ffp-contract=off", os.path.join(ROOT, "tests", src), "-o", exe,
           os.path.join(PKG, "host", "libnae_host.a"), "-L" + PKG, "-lnae_gpu", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
