"""ctypes binding of the CPU statement of the loudness meter (tests/loud_ref/ref_loud.c), built by tests/cstatement.py, its float64 numpy
restatement (the plain sequential recurrence, np.sum, np.convolve: nothing of the GPU's tiling, nothing in f32), and the signals the tests
share: the stepped noise and EBU Tech 3341's sines."""
import ctypes as C
import math
import os

import numpy as np

import cstatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "loud_ref", "ref_loud.c")
CHUNK, TP_REACH = 1024, 11                      # NAE_EQ_CHUNK; the true peak runs NAE_LOUD_TP_TAPS - 1 samples past the end
PHASES, TAPS, KAISER_BETA = 4, 12, 8.0          # NAE_LOUD_TP_PHASES, NAE_LOUD_TP_TAPS, NAE_FIR_KAISER_BETA
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416)   # NAE_LOUD_SHELF_F0, _GAIN_DB, _Q, _VB_EXP
HIGHPASS = (38.13547087602444, 0.5003270373238773)                                       # NAE_LOUD_HP_F0, _Q
INVALID, UNSUPPORTED = -1, -2                   # NAE_ERR_INVALID, NAE_ERR_UNSUPPORTED
# ITU-R BS.1770-4, table 1 and table 2: the K-weighting at 48 kHz as published (the high-pass numerator is 1, -2, 1)
BS1770_SHELF_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
BS1770_HIGHPASS_48K = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


class Params(C.Structure):
    """nae_loud_params, field for field (binding.LoudParams has the same layout)"""
    _fields_ = [("sample_rate", C.c_int), ("sub_block", C.c_int), ("coef", C.c_double * 10), ("gate_abs", C.c_double), ("target", C.c_double),
                ("ceiling_lin", C.c_double), ("max_gain_lin", C.c_double)]


class Result(C.Structure):
    """nae_loud_result, field for field (binding.LoudResult has the same layout)"""
    _fields_ = [("mean2", C.c_double), ("momentary_max", C.c_double), ("gain", C.c_double), ("gain_f32", C.c_float), ("true_peak", C.c_float * 2),
                ("sample_peak", C.c_float * 2), ("blocks_total", C.c_uint), ("blocks_abs", C.c_uint), ("blocks_rel", C.c_uint)]


def build(out_dir):
    L = cstatement.build(SRC, out_dir)
    L.ref_loud_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    L.ref_loud_taps.argtypes, L.ref_loud_taps.restype = [C.c_void_p], None
    L.ref_loud_measure.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.ref_loud_lufs.argtypes, L.ref_loud_lufs.restype = [C.c_double], C.c_double
    return L


def design_c(L, sample_rate, target_lufs=-14.0, ceiling_dbtp=-1.0, max_gain_db=20.0):
    """the statement's design -> (return code, Params)"""
    p = Params()
    return L.ref_loud_design(sample_rate, target_lufs, ceiling_dbtp, max_gain_db, C.byref(p)), p


def as_params(p):
    """any record of nae_loud_params' layout (the library's LoudParams) as the statement's"""
    return Params.from_buffer_copy(bytes(p))


def taps_c(L):
    out = np.zeros((PHASES, TAPS), np.float32)
    L.ref_loud_taps(out.ctypes.data)
    return out


def measure(L, params, x, tiled=True):
    """x[n, ch] f32 -> (Result, E[U, ch]): the tiled statement (what the GPU computes) or the sequential one"""
    x = np.ascontiguousarray(x, np.float32)
    n, ch = x.shape
    params = as_params(params)
    E = np.zeros((max(n // params.sub_block, 1), ch), np.float64)
    r = Result()
    rc = L.ref_loud_measure(C.byref(params), x.ctypes.data, n, ch, 1 if tiled else 0, C.byref(r), E.ctypes.data)
    assert rc == 0, rc
    return r, E[: n // params.sub_block]


def normalize(L, params, x):
    """x[n, ch] -> (y[n, ch], Result): the tiled statement's record, and y = x * gain_f32 as one f32 product"""
    r, _ = measure(L, params, x)
    return np.ascontiguousarray(x, np.float32) * np.float32(r.gain_f32), r


def lufs(energy):
    return -0.691 + 10.0 * math.log10(energy) if energy > 0.0 else float("-inf")


def record_fields(r):
    """a record's fields as exact integers: doubles by their 64 bits, floats by their 32"""
    f64 = lambda v: int(np.float64(v).view(np.uint64))
    f32 = lambda v: int(np.float32(v).view(np.uint32))
    return {"mean2": f64(r.mean2), "momentary_max": f64(r.momentary_max), "gain": f64(r.gain), "gain_f32": f32(r.gain_f32),
            "true_peak": [f32(v) for v in r.true_peak], "sample_peak": [f32(v) for v in r.sample_peak],
            "blocks": (int(r.blocks_total), int(r.blocks_abs), int(r.blocks_rel))}


# ------------------------------------------------------------------------------------------------ the float64 restatement
def kweight(sample_rate):
    """float64 restatement of the K-weighting of nae_loud_design: [2][5], tan and the powers from libm through `math`, as the library's"""
    f0, gain_db, q, vb_exp = SHELF
    K = math.tan(math.pi * f0 / float(sample_rate))
    Vh = math.pow(10.0, gain_db / 20.0)
    Vb = math.pow(Vh, vb_exp)
    kq, kk = K / q, K * K
    a0 = 1.0 + kq + kk
    shelf = [(Vh + Vb * kq + kk) / a0, 2.0 * (kk - Vh) / a0, (Vh - Vb * kq + kk) / a0, 2.0 * (kk - 1.0) / a0, (1.0 - kq + kk) / a0]
    f0, q = HIGHPASS
    K = math.tan(math.pi * f0 / float(sample_rate))
    kq, kk = K / q, K * K
    a0 = 1.0 + kq + kk
    return np.array([shelf, [1.0, -2.0, 1.0, 2.0 * (kk - 1.0) / a0, (1.0 - kq + kk) / a0]], np.float64)


def levels(target_lufs, ceiling_dbtp, max_gain_db):
    """(gate_abs, target, ceiling_lin, max_gain_lin) of nae_loud_design"""
    return (math.pow(10.0, (-70.0 + 0.691) / 10.0), math.pow(10.0, (target_lufs + 0.691) / 10.0), math.pow(10.0, ceiling_dbtp / 20.0),
            math.pow(10.0, max_gain_db / 20.0))


def _i0(x):
    s = term = 1.0
    q = x * x / 4.0
    for k in range(1, 64):
        term *= q / (float(k) * float(k))
        s += term
        if term < 1e-18 * s:
            break
    return s


def taps64():
    """the true-peak phases [4][12] in float64, not rounded to f32"""
    half = 0.5 * (PHASES * TAPS - 1)
    h = []
    for i in range(PHASES * TAPS):
        t = float(i) - half
        a = t / half
        r = 1.0 - a * a
        w = _i0(KAISER_BETA * math.sqrt(r if r > 0.0 else 0.0)) / _i0(KAISER_BETA)
        arg = math.pi * (t / PHASES)
        h.append(math.sin(arg) / arg * w)
    h = np.array(h, np.float64)
    return np.stack([h[p::PHASES] / np.sum(h[p::PHASES]) for p in range(PHASES)])


def _biquad(coef, x):
    """the plain sequential recurrence (transposed direct form II) in Python floats, which are IEEE doubles"""
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    z1 = z2 = 0.0
    y = [0.0] * len(x)
    for n, xv in enumerate(x):
        yv = b0 * xv + z1
        z1 = (b1 * xv - a1 * yv) + z2
        z2 = b2 * xv - a2 * yv
        y[n] = yv
    return y


def measure64(sample_rate, x, target_lufs=-14.0, ceiling_dbtp=-1.0, max_gain_db=20.0):
    """x[n, ch] -> a dict: the whole measurement in float64, on the plain definitions of BS.1770-4"""
    x = np.asarray(x, np.float64)
    n, ch = x.shape
    B = sample_rate // 10
    U = n // B
    gate_abs, target, ceiling_lin, max_gain_lin = levels(target_lufs, ceiling_dbtp, max_gain_db)
    coef = kweight(sample_rate)
    E = np.zeros((U, ch), np.float64)
    true_peak, sample_peak = [], []
    t64 = taps64()
    for c in range(ch):
        w = np.array(_biquad(coef[1], _biquad(coef[0], x[:, c].tolist())), np.float64)
        for u in range(U):
            E[u, c] = np.sum(w[u * B:(u + 1) * B] ** 2)
        true_peak.append(max(float(np.max(np.abs(np.convolve(x[:, c], t64[p])))) for p in range(PHASES)))
        sample_peak.append(float(np.max(np.abs(x[:, c]))))
    blocks = max(U - 3, 0)
    p = np.array([np.sum(E[j:j + 4].sum(axis=0) / (4.0 * B)) for j in range(blocks)], np.float64)
    past_abs = p[p > gate_abs]
    gate_rel = 0.1 * float(np.mean(past_abs)) if past_abs.size else 0.0
    past_rel = p[(p > gate_abs) & (p > gate_rel)]
    mean2 = float(np.mean(past_rel)) if past_rel.size else 0.0
    gain = 1.0
    if past_rel.size:
        peak = max(true_peak + sample_peak)
        gain = math.sqrt(target / mean2)
        if gain * peak > ceiling_lin:
            gain = ceiling_lin / peak
        gain = min(gain, max_gain_lin)
    return {"E": E, "p": p, "gate_abs": gate_abs, "gate_rel": gate_rel, "mean2": mean2, "momentary_max": float(p.max()) if blocks else 0.0,
            "gain": gain, "true_peak": true_peak, "sample_peak": sample_peak, "blocks": (blocks, int(past_abs.size), int(past_rel.size))}


def true_peak_at(x):
    """one channel x[n] -> (n, |v_p[n]|) of the largest oversampled value in float64, n = 0 ... len(x) + 10: where the true peak falls"""
    v = np.abs(np.stack([np.convolve(np.asarray(x, np.float64), t) for t in taps64()]))
    n = int(np.argmax(v.max(axis=0)))
    return n, float(v[:, n].max())


# ------------------------------------------------------------------------------------------------ signals
def stepped(sample_rate, ch, seed=None, scale=1.0):
    """uniform noise from default_rng(sample_rate + ch) at -80 dB for 0.5 s, -30 dB for 1 s, -12 dB for 1 s, -45 dB for 0.5 s plus 37 samples;
    the second channel times 0.5: silence under the absolute gate, a stretch the relative gate drops, programme -> [n, ch] f32"""
    rng = np.random.default_rng(sample_rate + ch if seed is None else seed)
    parts = []
    for db, n in ((-80.0, sample_rate // 2), (-30.0, sample_rate), (-12.0, sample_rate), (-45.0, sample_rate // 2 + 37)):
        parts.append(rng.uniform(-1.0, 1.0, (n, ch)) * 10.0 ** (db / 20.0))
    x = np.concatenate(parts) * scale
    if ch == 2:
        x[:, 1] *= 0.5
    return x.astype(np.float32)


def sine_steps(sample_rate, steps, freq=1000.0, channels=(1.0, 1.0)):
    """one sine of `freq` running through the stretches (seconds, dBFS peak) of `steps`, with the per-channel factors `channels` -> [n, ch] f32"""
    amp = np.concatenate([np.full(int(round(sec * sample_rate)), 10.0 ** (db / 20.0)) for sec, db in steps])
    s = amp * np.sin(2.0 * np.pi * freq * np.arange(amp.size) / sample_rate)
    return np.stack([s * g for g in channels], axis=1).astype(np.float32)
