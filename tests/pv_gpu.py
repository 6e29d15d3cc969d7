"""What the vocoder's GPU tests share (tests/test_gpu_pv_*.py, tests/test_gpu_stretch_range.py, tests/tools/fuzz_pv_options.py): the two-tone
and noise signals, the stereo scene whose channels decide on their own, clicks placed on chosen frames, a bit comparison, the block call and
the streaming handle.  The tone, the scene and the placed clicks are also the CPU tests' (tests/test_pv_*_cpu.py, tests/test_fuzz_pv_cpu.py)."""
import ctypes as C

import numpy as np

import orc

ENTRIES = ("ex", "n", "formant")          # nae_stretch_create_ex / _n / _formant


def tone(L, amp=(0.5, 0.25), f=(1000.0, 3300.0)):
    n = np.arange(L)
    return sum(a * np.sin(2 * np.pi * fr * n / 48000) for a, fr in zip(amp, f)).astype(np.float32)


def signal(kind, L, ch, seed=41, tonal=tone):
    """noise, or tonal(L) (the second channel at half level)"""
    if kind == "noise":
        return orc.fill_uniform(L * ch, seed)
    m = tonal(L)
    return np.stack([m, 0.5 * m], 1).reshape(-1).astype(np.float32) if ch == 2 else m


def scene(L, seed=3, n_hits=None):
    """a stereo stream whose channels decide differently on their own: two partials at different levels per channel over independent quiet
    noise, with clicks and decaying noise bursts at seeded places — a third in the left channel only, a third in the right only, a third in
    both at different levels"""
    rng = np.random.default_rng(seed)
    n = np.arange(L)
    a, b = np.sin(2 * np.pi * 1000.0 * n / 48000), np.sin(2 * np.pi * 3300.0 * n / 48000)
    x = 0.01 * rng.standard_normal((L, 2))
    x[:, 0] += 0.05 * a + 0.01 * b
    x[:, 1] += 0.01 * a + 0.04 * b
    n_hits = n_hits or max(6, L // 6000)
    for i, p in enumerate(np.sort(rng.choice(np.arange(2000, L - 3000), n_hits, replace=False))):
        gains = ((1.0, 0.0), (0.0, 1.0), (1.0, 0.3))[i % 3]
        if rng.random() < 0.5:
            hit = np.zeros(2400)
            hit[0] = 0.9
        else:
            hit = 0.6 * np.exp(-np.arange(2400) / 300.0) * rng.standard_normal(2400)
        x[p:p + 2400, 0] += gains[0] * hit
        x[p:p + 2400, 1] += gains[1] * hit
    return np.ascontiguousarray(x, np.float32).reshape(-1)


SIDES = ((1.0, 0.0), (0.0, 1.0), (1.0, 0.7))                # a hit in the left channel only, the right only, both


def placed_clicks(nae, L, ch, rate, pitch, n_fft, tile=16, first=2, every=3, depth=None, sides=False, floor=0.0, seed=1, amp=0.9):
    """clicks in silence placed so that onsets fall on frames 16 k, 16 k + 1 and 16 k + 15 (a 16-frame tile's first, second and last frame):
    a click N/8 inside the end of frame F's window (Hann weight 0.15, above the floor at every size) lies past frame F - 1's window at a tempo
    above 1/2.  With the transposer first the vocoder reads the transposed signal, so the place is scaled by the transposer's ratio.
    The tiles are first, first + every, ... (every third, so that the clicks do not meet at a tempo near 1/2); depth: the click's distance
    from the window's end where it is not N/8 (at most the analysis hop, it still lies past frame F - 1's window); sides (stereo):
    successive clicks in the left channel only, the right only and both, a tile's three places each met by another side — otherwise the
    second channel is 0.7 of the first; floor: the sigma of independent seeded noise per channel under the clicks; amp: the clicks' height."""
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    scale = pl.rate_eff if pl.rs_first else 1.0
    depth = n_fft // 8 if depth is None else depth
    x = (floor * np.random.default_rng(seed).standard_normal((L, ch)) if floor else np.zeros((L, ch))).astype(np.float32)
    for i, k in enumerate(range(first, 10 ** 6, every)):
        F = tile * k + (0, 1, tile - 1)[(k // every) % 3]
        p = int(round(((((F - 1) * pl.ha_q24 + (1 << 23)) >> 24) - n_fft // 2 + n_fft - depth) * scale))
        if p >= L - 2 * n_fft:
            break
        x[p] = amp * np.asarray(SIDES[(i + i // 3) % 3][:ch]) if sides else amp
    if ch == 2 and not sides:
        x[:, 1] *= 0.7
    return np.ascontiguousarray(x, np.float32).reshape(-1)


RANGE_TEMPOS = (0.26, 3.9, 8.0, 16.0, 1 / 64)               # the rows of the tempo-range tests: each with every ratio of RANGE_RHOS
RANGE_RHOS = (1.0, 0.5, 3.0)                                # no transposer, the transposer behind the vocoder, in front of it


def hard_bursts(nae, L, rate, pitch, n_fft, seed=1):
    """noise bursts of N samples that start hard out of near-silence (sigma 1e-4), one every 6 N samples of the vocoder's input: the left
    channel only, the right only, both.  At a tempo below 1/2 a click enters the window over several frames and no frame quadruples it;
    a burst's start does: its first frame is above the floor in every bin over a frame that held the near-silence alone"""
    pl = nae.Context.stretch_plan(rate, pitch, L, n_fft)
    scale = pl.rate_eff if pl.rs_first else 1.0
    rng = np.random.default_rng(seed)
    x = 1e-4 * rng.standard_normal((L, 2))
    step, length = int(6 * n_fft * scale), int(n_fft * scale)
    for i, p in enumerate(range(step // 2, L - step, step)):
        x[p:p + length] += (0.5 * rng.standard_normal(length))[:, None] * np.asarray(SIDES[i % 3])
    return np.ascontiguousarray(x, np.float32).reshape(-1)


def range_case(nae, n_fft, tempo, rho):
    """the stereo input of one row of the tempo-range tests -> (x, L, rate, pitch), the vocoder at `tempo` and the transposer at `rho`.
    Above 1/2: clicks over a quiet floor placed on a tile's first, second and last frame (about 70 frames), as deep in the window as the
    analysis hop allows.  0.26: hard_bursts (465 frames).  1/64: the analysis hop is N/256 samples, and no input within full scale fired
    in the CPU statement — a click enters at a Hann weight of 1.5e-4, under the floor NAE_TRANSIENT_FLOOR, and once it is above the floor
    no hop quadruples it.  A click of height 4096 in digital silence, one hop inside the window's end, does fire: it is above the floor in the
    first frame that holds it, over a frame of exact zeros.  The first click in each channel fires; the later ones enter a window that
    still holds an earlier one (it stays for 256 frames) and do not."""
    H = n_fft // 4
    rate, pitch = rho * tempo, 1 / tempo
    scale = rho if rho > 1 else 1.0
    if tempo > 0.5:
        L = int((68 * H * tempo + 3 * n_fft) * scale)
        x = placed_clicks(nae, L, 2, rate, pitch, n_fft, first=1, every=1, depth=min(n_fft // 2, int(0.9 * H * tempo)), sides=True, floor=1e-4)
    elif tempo > 1 / 32:
        L = int(30 * n_fft * scale)
        x = hard_bursts(nae, L, rate, pitch, n_fft)
    else:
        L = int((100 * H * tempo + 3 * n_fft) * scale)
        x = placed_clicks(nae, L, 2, rate, pitch, n_fft, first=1, every=1, depth=int(H * tempo), sides=True, amp=4096.0)
    return x, L, rate, pitch


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def profiled(c, fn, *args, **kw):
    """(fn(*args, **kw), the set of kernels it launched on context c)"""
    c.prof_reset(); c.prof_enable(True)
    out = fn(*args, **kw)
    c.prof_enable(False)
    return out, set(c.prof_report())


def block(c, nae, x, ch, rate, pitch, n_fft=1024, lock=False, lifter=0, n_streams=1, planar_in=False, planar_out=False, transients=False,
          link=False, formant_ratio=None):
    """the block call on x, [n_streams][L][ch] flattened -> interleaved [n_streams * out_len * ch], whatever the layouts on the device;
    formant_ratio given: the _formant_shift entry and its plan"""
    L = x.size // (ch * n_streams)
    pl = c.stretch_plan(rate, pitch, L, n_fft, lifter, formant_ratio) if formant_ratio is not None else c.stretch_plan(rate, pitch, L, n_fft)
    flat = np.ascontiguousarray(x.reshape(n_streams, L, ch).transpose(0, 2, 1)).reshape(-1) if planar_in else x
    d_x, d_o = c.array(np.ascontiguousarray(flat, np.float32)), c.empty(max(1, n_streams * pl.out_len * ch))
    src = nae.Sig.planar(d_x.ptr, L, ch) if planar_in else nae.Sig.interleaved(d_x.ptr, L, ch)
    dst = nae.Sig.planar(d_o.ptr, pl.out_len, ch) if planar_out else nae.Sig.interleaved(d_o.ptr, pl.out_len, ch)
    c.stretch_block(rate, pitch, src, L, ch, n_streams, dst, phase_lock=lock, n_fft=n_fft, formant=lifter, transients=transients,
                    formant_ratio=formant_ratio, link_channels=link)
    out = d_o.download()[: n_streams * pl.out_len * ch]
    d_x.free(); d_o.free()
    if planar_out:
        out = np.ascontiguousarray(out.reshape(n_streams, ch, pl.out_len).transpose(0, 2, 1)).reshape(-1)
    return out


def stream(c, x, ch, rate, pitch, put_sizes, entry, n_fft=1024, flags=0, lifter=0, sample_rate=48000, repeat_last=False,
           device_put=False, formant_ratio=1.0):
    """the streaming handle made by nae_stretch_create_<entry> (ENTRIES, or "formant_shift" with formant_ratio): puts of put_sizes (cycled,
    or with repeat_last the last one repeated) from the host, from device memory with device_put, or in turns with device_put =
    "alternate"; a receive after every put, then flush and receive: the whole output, interleaved"""
    lib = c.lib
    L = x.size // ch
    h = C.c_void_p()
    if entry == "ex":
        rc = lib.nae_stretch_create_ex(c.h, sample_rate, ch, rate, pitch, flags, C.byref(h))
    elif entry == "n":
        rc = lib.nae_stretch_create_n(c.h, sample_rate, ch, rate, pitch, flags, n_fft, C.byref(h))
    elif entry == "formant":
        rc = lib.nae_stretch_create_formant(c.h, sample_rate, ch, rate, pitch, flags, n_fft, lifter, C.byref(h))
    else:
        assert entry == "formant_shift", entry
        rc = lib.nae_stretch_create_formant_shift(c.h, sample_rate, ch, rate, pitch, flags, n_fft, lifter, formant_ratio, C.byref(h))
    assert rc == 0, rc
    outs, pos, i = [], 0, 0
    d_x = c.array(x) if device_put else None

    def drain():
        n = lib.nae_stretch_available(h)
        if n:
            buf = np.empty(n * ch, np.float32)
            got = C.c_size_t()
            assert lib.nae_stretch_receive_host(h, buf.ctypes.data, n, C.byref(got)) == 0
            outs.append(buf[: got.value * ch])

    while pos < L:
        size = put_sizes[-1] if repeat_last and i >= len(put_sizes) else put_sizes[i % len(put_sizes)]
        n = min(size, L - pos)
        i += 1
        if device_put is True or (device_put == "alternate" and i % 2 == 0):
            assert lib.nae_stretch_put(h, d_x.at(pos * ch), n) == 0
        else:
            chunk = np.ascontiguousarray(x[pos * ch:(pos + n) * ch])
            assert lib.nae_stretch_put_host(h, chunk.ctypes.data, n) == 0
        pos += n
        drain()
    assert lib.nae_stretch_flush(h) == 0
    drain()
    assert lib.nae_stretch_destroy(h) == 0
    if d_x is not None:
        d_x.free()
    return np.concatenate(outs) if outs else np.zeros(0, np.float32)
