"""What the effect nodes' timing tools (tools/*_time.py) share: the driver that gives every step a process and a time limit of its own, the
two timing loops between a pair of nae_event_records, and the set-up of the two signal buffers.

A tool is a driver when it is started without its step flag, and one step's measurement when it is started with it.  The driver never
loads the library: a process that has opened the device only measures and exits, and the first step that fails ends the run."""
import argparse
import os
import statistics
import subprocess
import sys

# (name, n_streams, T) of stereo at 48 kHz; a tool with other shapes keeps a table of its own
SHAPES = {"large": ("1024 streams x 10 s", 1024, 480000), "small": ("8 streams x 10 s", 8, 480000),
          "quick-large": ("64 streams x 2 s", 64, 96000), "quick-small": ("8 streams x 2 s", 8, 96000)}


def parser(limit, quick="a sixteenth of the large shape's streams, and a fifth of the length", runs=7, step="--shape", what="shape", **step_kw):
    """the arguments every tool has: limit is the tool's default --limit, quick the help of --quick, step the flag the driver starts a
    child with (step_kw: its choices or type)"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=runs)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help=quick)
    ap.add_argument("--limit", type=float, default=limit, help=f"seconds each {what}'s process may take")
    ap.add_argument(step, help=f"run this one {what} in this process (what the driver starts)", **step_kw)
    return ap


def shape_steps(quick, keys=("large", "small")):
    """the steps of a tool whose table has a quick-KEY beside every KEY"""
    return [(k, ["--shape", k]) for k in (("quick-" + k if quick else k) for k in keys)]


def counts(args):
    return ["--runs", str(args.runs), "--warmup", str(args.warmup)]


def drive(script, steps, limit, passthrough):
    """Runs script once per (label, argv-tail) of steps, each in a fresh child process that may take limit seconds, and stops at the first
    that fails: returns 0, 124 after a timeout (the child is killed), the child's status, or 128 + n for a child that signal n killed."""
    for label, tail in steps:
        cmd = [sys.executable, os.path.abspath(script)] + list(tail) + list(passthrough)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{label}: no result within {limit:g} s; stopping", flush=True)
            return 124
        if rc:
            rc = 128 - rc if rc < 0 else rc
            print(f"{label}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def setup(nae, ctx, n_streams, T, ch=2):
    """n_streams streams of T frames of uniform noise and as much room for the result: the two device arrays and their interleaved Sigs"""
    d_in, d_out = ctx.empty(n_streams * T * ch), ctx.empty(n_streams * T * ch)
    ctx.fill_uniform(d_in.ptr, T * ch, T * ch, n_streams, 0, 0)
    return d_in, d_out, nae.Sig.interleaved(d_in.ptr, T, ch), nae.Sig.interleaved(d_out.ptr, T, ch)


def release(*arrays):
    for d in arrays:
        d.free()


def timed(ctx, fn, runs, warmup):
    """one call after the other: (median, min, max) of runs timings of fn() after warmup untimed ones"""
    a, b = ctx.event(), ctx.event()
    for _ in range(warmup):
        fn()
    ctx.sync()
    ms = []
    for _ in range(runs):
        ctx.record(a)
        fn()
        ctx.record(b)
        ms.append(ctx.elapsed_ms(a, b))
    ctx.destroy_event(a)
    ctx.destroy_event(b)
    return statistics.median(ms), min(ms), max(ms)


def timed_behind(ctx, before, fn, runs, warmup):
    """as timed, with before() queued on the stream in front of every call and outside its pair of events"""
    a, b = ctx.event(), ctx.event()
    ms = []
    for i in range(warmup + runs):
        before()
        ctx.record(a)
        fn()
        ctx.record(b)
        t = ctx.elapsed_ms(a, b)
        if i >= warmup:
            ms.append(t)
    ctx.destroy_event(a)
    ctx.destroy_event(b)
    return statistics.median(ms), min(ms), max(ms)


def rounds(ctx, cases, runs, warmup, clock=True):
    """interleaved: every round times every case of cases, (tag, what, fn, ...), once and in turn.  Returns the milliseconds per tag and the
    shader clock before and after the timed rounds (None where clock is false: the probe kernel is not run)"""
    a, b = ctx.event(), ctx.event()
    for _ in range(warmup):
        for case in cases:
            case[2]()
    ctx.sync()
    clock_before = ctx.clock_ghz() if clock else None
    ms = {case[0]: [] for case in cases}
    for _ in range(runs):
        for case in cases:
            ctx.record(a)
            case[2]()
            ctx.record(b)
            ms[case[0]].append(ctx.elapsed_ms(a, b))
    clock_after = ctx.clock_ghz() if clock else None
    ctx.destroy_event(a)
    ctx.destroy_event(b)
    return ms, clock_before, clock_after
