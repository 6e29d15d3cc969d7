"""ctypes binding of include/nae_gpu.h.  No CPU compute lives here — every method enqueues HIP work."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Iterable, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

FMT_S16, FMT_S32, FMT_FLT, FMT_S16P, FMT_S32P, FMT_FLTP = 1, 2, 3, 6, 7, 8
FFT_N, HOP, BINS = 1024, 256, 513

# every entry point include/nae_gpu.h declares (tests check the library exports exactly these)
EXPORTED_SYMBOLS = [
    "nae_abi_version", "nae_device_count", "nae_ctx_create", "nae_ctx_destroy", "nae_ctx_set_stream",
    "nae_ctx_stream", "nae_sync", "nae_poll", "nae_last_error", "nae_device_name", "nae_malloc", "nae_free",
    "nae_memcpy_h2d", "nae_memcpy_d2h", "nae_memcpy_d2d", "nae_memset", "nae_event_create", "nae_event_record",
    "nae_event_query", "nae_ctx_wait_event", "nae_debug_graph4_stages",
    "nae_event_elapsed_ms", "nae_event_destroy", "nae_prof_enable", "nae_prof_reset", "nae_prof_get",
    "nae_malloc_host", "nae_free_host", "nae_debug_clock_ghz", "nae_debug_set", "nae_debug_diff_u32", "nae_fill_uniform_f32", "nae_gain_f32", "nae_gain_s16", "nae_gain_s32", "nae_gain_frame",
    "nae_deinterleave_f32", "nae_interleave_f32", "nae_copy_sig_f32", "nae_gain_sig_f32", "nae_amix_f32",
    "nae_amix_sig_f32", "nae_bimix_f32", "nae_bimix2_downmix_f32", "nae_bimix2_interleave_f32",
    "nae_to_f32_interleaved", "nae_clamp_f32", "nae_stretch_plan_make", "nae_stretch_block_f32",
    "nae_debug_pv_tile_phase", "nae_stretch_block_ex_f32", "nae_debug_pv_tile_phase_ex", "nae_stretch_create_ex",
    "nae_stretch_plan_make_n", "nae_stretch_block_n_f32", "nae_debug_pv_tile_phase_n", "nae_stretch_create_n",
    "nae_stretch_formant_lifter", "nae_stretch_block_formant_f32", "nae_stretch_create_formant",
    "nae_stretch_plan_make_shift", "nae_stretch_block_formant_shift_f32", "nae_stretch_create_formant_shift", "nae_stretch_create", "nae_stretch_put", "nae_stretch_put_host", "nae_stretch_flush",
    "nae_stretch_available", "nae_stretch_receive", "nae_stretch_receive_host", "nae_stretch_destroy",
    "nae_swr_create", "nae_swr_convert_host", "nae_swr_convert", "nae_swr_buffered", "nae_swr_destroy", "nae_mono_to_stereo_f32",
    "nae_spectrum_frames", "nae_spectrum_block_f32", "nae_spectrum_frames_ex", "nae_spectrum_block_ex_f32", "nae_spectrum_create", "nae_spectrum_put",
    "nae_spectrum_available", "nae_spectrum_receive", "nae_spectrum_destroy", "nae_graph4_run",
    "nae_wsola_plan_make", "nae_wsola_block_f32", "nae_wsola_create", "nae_wsola_put", "nae_wsola_put_host",
    "nae_wsola_flush", "nae_wsola_available", "nae_wsola_receive", "nae_wsola_receive_host", "nae_wsola_destroy",
    "nae_fir_pick_n_fft", "nae_fir_block_f32", "nae_fir_design", "nae_fir_create", "nae_fir_put", "nae_fir_put_host", "nae_fir_flush",
    "nae_fir_available", "nae_fir_receive", "nae_fir_receive_host", "nae_fir_destroy",
    "nae_conv_pick_n_fft", "nae_conv_block_f32", "nae_conv_reverb_taps", "nae_conv_design_reverb", "nae_conv_create", "nae_conv_put",
    "nae_conv_put_host", "nae_conv_flush", "nae_conv_available", "nae_conv_receive", "nae_conv_receive_host", "nae_conv_destroy",
    "nae_eq_design", "nae_eq_block_f32", "nae_eq_create", "nae_eq_put", "nae_eq_put_host", "nae_eq_flush", "nae_eq_available", "nae_eq_receive",
    "nae_eq_receive_host", "nae_eq_destroy",
    "nae_dyn_design", "nae_dyn_block_f32", "nae_dyn_create", "nae_dyn_put", "nae_dyn_put_host", "nae_dyn_flush", "nae_dyn_available",
    "nae_dyn_receive", "nae_dyn_receive_host", "nae_dyn_destroy",
    "nae_dynkey_block_f32", "nae_dynkey_create", "nae_dynkey_put", "nae_dynkey_put_host", "nae_dynkey_flush", "nae_dynkey_available",
    "nae_dynkey_receive", "nae_dynkey_receive_host", "nae_dynkey_destroy",
    "nae_echo_design", "nae_echo_block_f32", "nae_echo_create", "nae_echo_put", "nae_echo_put_host", "nae_echo_flush", "nae_echo_available",
    "nae_echo_receive", "nae_echo_receive_host", "nae_echo_destroy",
    "nae_mod_design", "nae_mod_block_f32", "nae_mod_create", "nae_mod_put", "nae_mod_put_host", "nae_mod_flush", "nae_mod_available",
    "nae_mod_receive", "nae_mod_receive_host", "nae_mod_destroy",
    "nae_sat_latency", "nae_sat_taps", "nae_sat_design", "nae_sat_block_f32", "nae_sat_create", "nae_sat_put", "nae_sat_put_host", "nae_sat_flush",
    "nae_sat_available", "nae_sat_receive", "nae_sat_receive_host", "nae_sat_destroy",
    "nae_gate_design", "nae_gate_block_f32", "nae_gate_create", "nae_gate_put", "nae_gate_put_host", "nae_gate_flush", "nae_gate_available",
    "nae_gate_receive", "nae_gate_receive_host", "nae_gate_destroy",
    "nae_mb_design", "nae_mb_block_f32", "nae_mb_create", "nae_mb_put", "nae_mb_put_host", "nae_mb_flush", "nae_mb_available",
    "nae_mb_receive", "nae_mb_receive_host", "nae_mb_destroy",
    "nae_denoise_design", "nae_denoise_profile_f32", "nae_denoise_block_f32", "nae_denoise_create", "nae_denoise_put", "nae_denoise_put_host",
    "nae_denoise_flush", "nae_denoise_available", "nae_denoise_receive", "nae_denoise_receive_host", "nae_denoise_destroy",
    "nae_hpss_design", "nae_hpss_block_f32", "nae_hpss_create", "nae_hpss_put", "nae_hpss_put_host", "nae_hpss_flush", "nae_hpss_available",
    "nae_hpss_receive", "nae_hpss_receive_host", "nae_hpss_destroy",
    "nae_lim_design", "nae_lim_block_f32", "nae_lim_create", "nae_lim_put", "nae_lim_put_host", "nae_lim_flush", "nae_lim_available",
    "nae_lim_receive", "nae_lim_receive_host", "nae_lim_destroy",
    "nae_dither_design", "nae_dither_block_f32", "nae_dither_create", "nae_dither_put", "nae_dither_put_host", "nae_dither_flush",
    "nae_dither_available", "nae_dither_receive", "nae_dither_receive_host", "nae_dither_destroy",
    "nae_loud_design", "nae_loud_lufs", "nae_loud_measure_f32", "nae_loud_apply_f32", "nae_loud_normalize_f32", "nae_loud_create", "nae_loud_put",
    "nae_loud_put_host", "nae_loud_flush", "nae_loud_get_result", "nae_loud_destroy",
]


STRETCH_PHASE_LOCK = 1       # NAE_STRETCH_PHASE_LOCK (include/nae_gpu.h)
STRETCH_TRANSIENTS = 4       # NAE_STRETCH_TRANSIENTS (include/nae_gpu.h): the _n and _formant entries only
STRETCH_LINK_CHANNELS = 16   # NAE_STRETCH_LINK_CHANNELS: one onset decision and one lock map per stereo stream; the same entries
FORMANT_SHIFT_MIN, FORMANT_SHIFT_MAX = 0.25, 4.0   # NAE_FORMANT_SHIFT_MIN / _MAX (include/nae_dsp_spec.h): the range of formant_ratio
FIR_SIZES = (512, 1024, 2048, 4096)                 # frame sizes of the FIR filter: at most n_fft / 2 + 1 taps
FIR_KINDS = {"lowpass": 0, "highpass": 1, "bandpass": 2, "bandstop": 3}   # `kind` of nae_fir_design
EQ_KINDS = ("peak", "lowshelf", "highshelf", "lowpass", "highpass", "notch")   # `kind` of nae_eq_design: NAE_EQ_PEAK ... NAE_EQ_NOTCH
DYNKEY_MAX_SECTIONS = 4                             # NAE_DYNKEY_MAX_SECTIONS (include/nae_dsp_spec.h): the key filter's sections
ECHO_MIN_DELAY, ECHO_MAX_DELAY, ECHO_MAX_SECTIONS, ECHO_MAX_FEEDBACK = 1024, 1 << 20, 4, 0.99   # NAE_ECHO_* (include/nae_dsp_spec.h)
MOD_MIN_DELAY, MOD_MAX_DELAY, MOD_MAX_VOICES, MOD_MAX_FEEDBACK = 2.0, 3070.0, 4, 0.95   # NAE_MOD_* (include/nae_dsp_spec.h)
MOD_SHAPES = ("sine", "triangle")                   # `shape` of nae_mod_params: NAE_MOD_SINE, NAE_MOD_TRIANGLE
SAT_HALF, SAT_MAX_OS = 16, 8                        # NAE_SAT_HALF, NAE_SAT_MAX_OS (include/nae_dsp_spec.h)
SAT_CURVES = ("soft", "hard")                       # `curve` of nae_sat_params: NAE_SAT_SOFT, NAE_SAT_HARD
GATE_MAX_HOLD = 1 << 21                             # NAE_GATE_MAX_HOLD (include/nae_dsp_spec.h)
GATE_MODES = ("gate", "expander")                   # `mode` of nae_gate_design: NAE_GATE_MODE_GATE, NAE_GATE_MODE_EXPANDER
MB_MAX_BANDS, MB_MAX_SECTIONS = 4, 14               # NAE_MB_MAX_BANDS, NAE_MB_MAX_SECTIONS (include/nae_dsp_spec.h)
HPSS_MAX_SPAN = 8                                   # NAE_HPSS_MAX_SPAN (include/nae_dsp_spec.h)
HPSS_MASKS = ("soft", "hard")                       # `hard` of nae_hpss_design: 0, 1
LIM_MAX_LOOKAHEAD, LIM_TP_REACH = 1018, 6           # NAE_LIM_MAX_LOOKAHEAD, NAE_LIM_TP_REACH (include/nae_dsp_spec.h)
DITHER_MIN_BITS, DITHER_MAX_BITS, DITHER_MAX_TAPS = 8, 24, 12   # NAE_DITHER_MIN_BITS, NAE_DITHER_MAX_BITS, NAE_DITHER_MAX_TAPS (include/nae_dsp_spec.h)
DITHER_KINDS = ("none", "rectangular", "triangular", "highpass")   # `kind` of nae_dither_params: NAE_DITHER_NONE ... NAE_DITHER_HIGHPASS
DITHER_SHAPINGS = ("none", "first", "second", "lipshitz")          # `shaping` of nae_dither_design: NAE_DITHER_SHAPE_NONE ... _LIPSHITZ
HANDLE_PREFIXES = ("nae_stretch", "nae_wsola", "nae_fir", "nae_conv", "nae_eq", "nae_dyn", "nae_dynkey", "nae_denoise", "nae_echo", "nae_mod", "nae_sat", "nae_gate", "nae_mb", "nae_hpss", "nae_lim", "nae_dither")   # the handles with the full put / receive set of entries


class NaeError(RuntimeError):
    pass


def lib_path() -> str:
    # NAE_GPU_LIB selects another build of the same ABI (A/B timing of kernel variants on one GPU box)
    return os.environ.get("NAE_GPU_LIB") or os.path.join(_HERE, "libnae_gpu.so")


def build_library(verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of libnae_gpu.so (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", _HERE, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise NaeError("building libnae_gpu.so failed")
    return lib_path()


class Sig(C.Structure):
    """nae_sig: element (s, c, i) at base[s*stream_stride + c*chan_stride + i*frame_stride]"""
    _fields_ = [("base", C.c_void_p), ("stream_stride", C.c_size_t), ("chan_stride", C.c_size_t),
                ("frame_stride", C.c_size_t)]

    @staticmethod
    def interleaved(ptr: int, S: int, ch: int, shared: bool = False, stream_stride: Optional[int] = None) -> "Sig":
        ss = 0 if shared else (S * ch if stream_stride is None else stream_stride)
        return Sig(ptr, ss, 1, ch)

    @staticmethod
    def planar(ptr: int, S: int, ch: int, shared: bool = False, plane_stride: Optional[int] = None,
               stream_stride: Optional[int] = None) -> "Sig":
        ps = S if plane_stride is None else plane_stride
        ss = 0 if shared else (ps * ch if stream_stride is None else stream_stride)
        return Sig(ptr, ss, ps, 1)


class DynParams(C.Structure):
    """nae_dyn_params: the dynamics processor's parameters (include/nae_gpu.h); nae_dyn_design makes them from times and a ratio"""
    _fields_ = [("threshold_db", C.c_double), ("slope", C.c_double), ("knee_db", C.c_double), ("alpha_attack", C.c_double),
                ("alpha_release", C.c_double), ("makeup_db", C.c_double), ("lookahead", C.c_int), ("link", C.c_int)]


class DynKeyParams(C.Structure):
    """nae_dynkey_params: the keyed dynamics' parameters (include/nae_gpu.h): nae_dyn_params, the key's channels (0: the signal is its own
    key) and the key filter's sections (b0, b1, b2, a1, a2), which nae_eq_design makes"""
    _fields_ = [("dyn", DynParams), ("key_ch", C.c_int), ("n_sections", C.c_int), ("coef", (C.c_double * 5) * DYNKEY_MAX_SECTIONS)]

    @staticmethod
    def make(dyn: DynParams, key_ch: int = 0, coef=()) -> "DynKeyParams":
        """coef: [n][5], at most DYNKEY_MAX_SECTIONS sections (more raise: the record has no room for them)"""
        coef = np.asarray(coef, np.float64).reshape(-1, 5)
        if coef.shape[0] > DYNKEY_MAX_SECTIONS:
            raise NaeError(f"nae_dynkey_params holds at most {DYNKEY_MAX_SECTIONS} sections")
        p = DynKeyParams()
        p.dyn = dyn
        p.key_ch, p.n_sections = key_ch, coef.shape[0]
        for s_, row in enumerate(coef):
            for i_, v in enumerate(row):
                p.coef[s_][i_] = v
        return p


class EchoParams(C.Structure):
    """nae_echo_params: the echo's parameters (include/nae_gpu.h): the channels' delays in samples, the feedback, ping-pong, wet and dry, and the
    loop's damping sections (b0, b1, b2, a1, a2); nae_echo_design makes them from seconds and corner frequencies"""
    _fields_ = [("delay", C.c_int * 2), ("feedback", C.c_double), ("cross", C.c_int), ("wet", C.c_double), ("dry", C.c_double),
                ("n_sections", C.c_int), ("coef", (C.c_double * 5) * ECHO_MAX_SECTIONS)]

    @staticmethod
    def make(delay, feedback: float, cross: bool = False, wet: float = 1.0, dry: float = 1.0, coef=()) -> "EchoParams":
        """delay: samples, one number or (left, right); coef: [n][5], at most ECHO_MAX_SECTIONS sections (more raise)"""
        coef = np.asarray(coef, np.float64).reshape(-1, 5)
        if coef.shape[0] > ECHO_MAX_SECTIONS:
            raise NaeError(f"nae_echo_params holds at most {ECHO_MAX_SECTIONS} sections")
        left, right = (delay, delay) if np.isscalar(delay) else delay
        p = EchoParams()
        p.delay[0], p.delay[1] = int(left), int(right)
        p.feedback, p.cross, p.wet, p.dry, p.n_sections = feedback, int(cross), wet, dry, coef.shape[0]
        for s_, row in enumerate(coef):
            for i_, v in enumerate(row):
                p.coef[s_][i_] = v
        return p


class ModParams(C.Structure):
    """nae_mod_params: the modulated delay's parameters (include/nae_gpu.h): the centre delay and the sweep's depth in samples, the feedback, wet
    and dry, the LFO's phase step, start phase and stereo spread in turns 2^32, the voices' phase offsets and the shape; nae_mod_design makes
    them from milliseconds and hertz"""
    _fields_ = [("delay", C.c_double), ("depth", C.c_double), ("feedback", C.c_double), ("wet", C.c_double), ("dry", C.c_double),
                ("rate_inc", C.c_uint32), ("phase0", C.c_uint32), ("phase_ch", C.c_uint32), ("n_voices", C.c_int),
                ("voice_phase", C.c_uint32 * MOD_MAX_VOICES), ("shape", C.c_int)]

    @staticmethod
    def make(delay: float, depth: float, feedback: float = 0.0, wet: float = 1.0, dry: float = 1.0, rate_inc: int = 0, phase0: int = 0,
             phase_ch: int = 0, voice_phase=(0,), shape: int = 0) -> "ModParams":
        """voice_phase: one offset per voice, at most MOD_MAX_VOICES (more raise)"""
        if len(voice_phase) > MOD_MAX_VOICES:
            raise NaeError(f"nae_mod_params holds at most {MOD_MAX_VOICES} voices")
        p = ModParams()
        p.delay, p.depth, p.feedback, p.wet, p.dry = delay, depth, feedback, wet, dry
        p.rate_inc, p.phase0, p.phase_ch, p.n_voices, p.shape = rate_inc & 0xffffffff, phase0 & 0xffffffff, phase_ch & 0xffffffff, len(voice_phase), shape
        for v, ph in enumerate(voice_phase):
            p.voice_phase[v] = ph & 0xffffffff
        return p


class SatParams(C.Structure):
    """nae_sat_params: the saturation's parameters (include/nae_gpu.h): the oversampling factor, the curve, the drive g, the bias b, wet and dry;
    nae_sat_design makes them from decibels and a mix"""
    _fields_ = [("oversample", C.c_int), ("curve", C.c_int), ("drive", C.c_float), ("bias", C.c_float), ("wet", C.c_float), ("dry", C.c_float)]

    @staticmethod
    def make(oversample: int = 4, curve: int = 0, drive: float = 1.0, bias: float = 0.0, wet: float = 1.0, dry: float = 0.0) -> "SatParams":
        p = SatParams()
        p.oversample, p.curve, p.drive, p.bias, p.wet, p.dry = oversample, curve, drive, bias, wet, dry
        return p


class GateParams(C.Structure):
    """nae_gate_params: the gate's parameters (include/nae_gpu.h): the two thresholds as magnitudes, the expander's threshold and slope, the
    range, the two smoothing coefficients, hold and look-ahead in samples, the mode and the channel link; nae_gate_design makes them from
    decibels and times"""
    _fields_ = [("open_lin", C.c_float), ("close_lin", C.c_float), ("threshold_db", C.c_double), ("slope", C.c_double), ("range_db", C.c_double),
                ("alpha_attack", C.c_double), ("alpha_release", C.c_double), ("hold", C.c_int), ("lookahead", C.c_int), ("expand", C.c_int),
                ("link", C.c_int)]


class MbParams(C.Structure):
    """nae_mb_params: the multiband compressor's parameters (include/nae_gpu.h): the band count, the crossover tree's sections (b0, b1, b2, a1,
    a2) in their fixed slots, one nae_dyn_params per band, and the mute and bypass masks; nae_mb_design makes them from crossover frequencies"""
    _fields_ = [("n_bands", C.c_int), ("n_sections", C.c_int), ("coef", (C.c_double * 5) * MB_MAX_SECTIONS), ("band", DynParams * MB_MAX_BANDS),
                ("mute_mask", C.c_uint), ("bypass_mask", C.c_uint)]

    @staticmethod
    def make(coef, bands, mute_mask: int = 0, bypass_mask: int = 0, n_bands: Optional[int] = None, n_sections: Optional[int] = None) -> "MbParams":
        """coef: [n][5], at most MB_MAX_SECTIONS sections; bands: at most MB_MAX_BANDS DynParams (more of either raise: the record has no room
        for them); n_bands, n_sections: counts that differ from the lengths, for the rejections"""
        coef = np.asarray(coef, np.float64).reshape(-1, 5)
        if coef.shape[0] > MB_MAX_SECTIONS or len(bands) > MB_MAX_BANDS:
            raise NaeError(f"nae_mb_params holds at most {MB_MAX_SECTIONS} sections and {MB_MAX_BANDS} bands")
        p = MbParams()
        p.n_bands, p.n_sections = len(bands) if n_bands is None else n_bands, coef.shape[0] if n_sections is None else n_sections
        for s_, row in enumerate(coef):
            for i_, v in enumerate(row):
                p.coef[s_][i_] = v
        for b_, band in enumerate(bands):
            p.band[b_] = band
        p.mute_mask, p.bypass_mask = mute_mask, bypass_mask
        return p


class DenoiseParams(C.Structure):
    """nae_denoise_params: the spectral gate's parameters (include/nae_gpu.h); nae_denoise_design makes them from decibels"""
    _fields_ = [("n_fft", C.c_int), ("time_smooth", C.c_int), ("freq_smooth", C.c_int), ("thr_scale", C.c_float), ("floor_gain", C.c_float)]


class LimParams(C.Structure):
    """nae_lim_params: the limiter's parameters (include/nae_gpu.h): the ceiling and the drive in decibels, the release coefficient, the
    look-ahead in samples, the true-peak detector and the channel link; nae_lim_design makes them from decibels and times"""
    _fields_ = [("ceiling_db", C.c_double), ("gain_db", C.c_double), ("alpha_release", C.c_double), ("lookahead", C.c_int),
                ("true_peak", C.c_int), ("link", C.c_int)]


class DitherParams(C.Structure):
    """nae_dither_params: the dither's parameters (include/nae_gpu.h): the word length, the dither's kind, the error feedback's taps c_1 ... c_K
    and the seed; nae_dither_design makes them from a preset's name"""
    _fields_ = [("bits", C.c_int), ("kind", C.c_int), ("n_taps", C.c_int), ("taps", C.c_double * 12), ("seed", C.c_uint64)]


class HpssParams(C.Structure):
    """nae_hpss_params: the separation's parameters (include/nae_gpu.h); nae_hpss_design makes them from decibels"""
    _fields_ = [("n_fft", C.c_int), ("time_span", C.c_int), ("freq_span", C.c_int), ("hard", C.c_int), ("gain_h", C.c_float), ("gain_p", C.c_float)]


class LoudParams(C.Structure):
    """nae_loud_params: the loudness meter's parameters (include/nae_gpu.h); nae_loud_design makes them from a sample rate and decibels"""
    _fields_ = [("sample_rate", C.c_int), ("sub_block", C.c_int), ("coef", C.c_double * 10), ("gate_abs", C.c_double), ("target", C.c_double),
                ("ceiling_lin", C.c_double), ("max_gain_lin", C.c_double)]


class LoudResult(C.Structure):
    """nae_loud_result: one stream's measurement and gain (include/nae_gpu.h)"""
    _fields_ = [("mean2", C.c_double), ("momentary_max", C.c_double), ("gain", C.c_double), ("gain_f32", C.c_float), ("true_peak", C.c_float * 2),
                ("sample_peak", C.c_float * 2), ("blocks_total", C.c_uint), ("blocks_abs", C.c_uint), ("blocks_rel", C.c_uint)]

    @property
    def lufs(self) -> float:
        """the integrated loudness; -inf for a stream without loudness"""
        return float("-inf") if self.mean2 == 0.0 else load_library().nae_loud_lufs(self.mean2)


class StretchPlan(C.Structure):
    _fields_ = [("pv_on", C.c_int), ("rs_on", C.c_int), ("tempo_eff", C.c_double), ("rate_eff", C.c_double),
                ("ha_q24", C.c_int64), ("d0", C.c_int32), ("r_q24", C.c_uint32 * 2), ("step_q32", C.c_uint64),
                ("out_len", C.c_size_t), ("mid_len", C.c_size_t), ("frames", C.c_size_t), ("rs_first", C.c_int)]


class WsolaPlan(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("channels", C.c_int), ("rate_eff", C.c_double), ("tempo_eff", C.c_double),
                ("order", C.c_int), ("overlap_len", C.c_int), ("seq_len", C.c_int), ("seek_len", C.c_int),
                ("sample_req", C.c_int), ("nominal_skip", C.c_double), ("in_len", C.c_size_t),
                ("flush_zeros", C.c_size_t), ("n_seq", C.c_size_t), ("td_out_len", C.c_size_t),
                ("aa_out_len", C.c_size_t), ("cu_out_len", C.c_size_t), ("out_len", C.c_size_t)]


class Graph4(C.Structure):
    _fields_ = [("in_a", Sig), ("in_b", Sig), ("vol_a", C.c_float), ("vol_b", C.c_float), ("mix_out", Sig),
                ("rate", C.c_double), ("pitch", C.c_double), ("pitch_out", Sig), ("spec_out", C.c_void_p),
                ("spec_stream_stride", C.c_size_t), ("S", C.c_size_t), ("n_streams", C.c_size_t)]


_lib = None


def load_library() -> C.CDLL:
    """Load libnae_gpu.so.  Fails loudly: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise NaeError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    lib = C.CDLL(p)
    vp, sz, i, u, f, d = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_float, C.c_double
    P = C.POINTER
    sigs = {
        "nae_abi_version": (i, []), "nae_device_count": (i, []),
        "nae_ctx_create": (i, [i, P(vp)]), "nae_ctx_destroy": (i, [vp]), "nae_ctx_set_stream": (i, [vp, vp]),
        "nae_ctx_stream": (vp, [vp]), "nae_sync": (i, [vp]), "nae_poll": (i, [vp]),
        "nae_last_error": (C.c_char_p, [vp]), "nae_device_name": (C.c_char_p, [vp]),
        "nae_malloc": (i, [vp, sz, P(vp)]), "nae_free": (i, [vp, vp]),
        "nae_memcpy_h2d": (i, [vp, vp, vp, sz]), "nae_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "nae_memcpy_d2d": (i, [vp, vp, vp, sz]), "nae_memset": (i, [vp, vp, i, sz]),
        "nae_event_create": (i, [vp, P(vp)]), "nae_event_record": (i, [vp, vp]),
        "nae_event_query": (i, [vp]), "nae_ctx_wait_event": (i, [vp, vp]), "nae_debug_graph4_stages": (i, [vp, P(Graph4), i]),
        "nae_event_elapsed_ms": (i, [vp, vp, P(f)]), "nae_event_destroy": (i, [vp]),
        "nae_prof_enable": (i, [vp, i]), "nae_prof_reset": (i, [vp]),
        "nae_prof_get": (i, [vp, i, C.c_char_p, sz, P(d), P(C.c_uint64)]),
        "nae_malloc_host": (i, [vp, sz, P(vp)]), "nae_free_host": (i, [vp, vp]),
        "nae_debug_clock_ghz": (i, [vp, P(C.c_double)]), "nae_debug_set": (i, [vp, C.c_char_p, C.c_longlong]),
        "nae_debug_diff_u32": (i, [vp, vp, vp, sz, vp]),
        "nae_fill_uniform_f32": (i, [vp, vp, sz, sz, sz, C.c_uint64, C.c_uint64]),
        "nae_gain_f32": (i, [vp, P(vp), P(vp), i, sz, f]), "nae_gain_s16": (i, [vp, P(vp), P(vp), i, sz, f]),
        "nae_gain_s32": (i, [vp, P(vp), P(vp), i, sz, f]),
        "nae_gain_frame": (i, [vp, i, P(vp), P(vp), sz, i, f]),
        "nae_deinterleave_f32": (i, [vp, vp, P(vp), sz, i]), "nae_interleave_f32": (i, [vp, P(vp), vp, sz, i]),
        "nae_copy_sig_f32": (i, [vp, P(Sig), P(Sig), sz, i, sz]),
        "nae_gain_sig_f32": (i, [vp, P(Sig), P(Sig), sz, i, sz, f]),
        "nae_amix_f32": (i, [vp, P(vp), P(vp), P(f), i, vp, vp, sz]),
        "nae_amix_sig_f32": (i, [vp, P(Sig), P(f), i, P(Sig), sz, sz]),
        "nae_bimix_f32": (i, [vp, vp, vp, vp, vp, f, vp, vp, sz]),
        "nae_bimix2_downmix_f32": (i, [vp, vp, vp, vp, sz]),
        "nae_bimix2_interleave_f32": (i, [vp, vp, vp, vp, sz, sz, i]),
        "nae_to_f32_interleaved": (i, [vp, i, P(vp), sz, i, vp]), "nae_clamp_f32": (i, [vp, vp, sz]),
        "nae_stretch_plan_make": (i, [d, d, sz, P(StretchPlan)]),
        "nae_stretch_block_f32": (i, [vp, d, d, P(Sig), sz, i, sz, P(Sig)]),
        "nae_debug_pv_tile_phase": (i, [vp, d, d, P(Sig), sz, i, sz, vp, sz, P(sz), P(sz)]),
        "nae_stretch_block_ex_f32": (i, [vp, d, d, u, P(Sig), sz, i, sz, P(Sig)]),
        "nae_debug_pv_tile_phase_ex": (i, [vp, d, d, u, P(Sig), sz, i, sz, vp, sz, P(sz), P(sz)]),
        "nae_stretch_create_ex": (i, [vp, i, i, f, f, u, P(vp)]),
        "nae_stretch_plan_make_n": (i, [d, d, i, sz, P(StretchPlan)]),
        "nae_stretch_block_n_f32": (i, [vp, d, d, u, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_debug_pv_tile_phase_n": (i, [vp, d, d, u, i, P(Sig), sz, i, sz, vp, sz, P(sz), P(sz)]),
        "nae_stretch_create_n": (i, [vp, i, i, f, f, u, i, P(vp)]),
        "nae_stretch_formant_lifter": (i, [i, i]),
        "nae_stretch_block_formant_f32": (i, [vp, d, d, u, i, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_stretch_create_formant": (i, [vp, i, i, f, f, u, i, i, P(vp)]),
        "nae_stretch_plan_make_shift": (i, [d, d, d, i, i, sz, P(StretchPlan)]),
        "nae_stretch_block_formant_shift_f32": (i, [vp, d, d, u, i, i, d, P(Sig), sz, i, sz, P(Sig)]),
        "nae_stretch_create_formant_shift": (i, [vp, i, i, f, f, u, i, i, d, P(vp)]),
        "nae_stretch_create": (i, [vp, i, i, f, f, P(vp)]),
        "nae_swr_create": (i, [vp, i, i, i, i, P(vp)]),
        "nae_swr_convert_host": (i, [vp, P(vp), sz, vp, vp, sz, P(sz)]), "nae_swr_convert": (i, [vp, P(vp), sz, vp, vp, sz, P(sz)]),
        "nae_swr_buffered": (sz, [vp]),
        "nae_swr_destroy": (i, [vp]), "nae_mono_to_stereo_f32": (i, [vp, vp, vp, sz, f]),
        "nae_spectrum_frames": (sz, [sz]), "nae_spectrum_block_f32": (i, [vp, P(Sig), sz, i, sz, vp, sz]),
        "nae_spectrum_frames_ex": (sz, [sz, i, i]), "nae_spectrum_block_ex_f32": (i, [vp, i, i, P(Sig), sz, i, sz, vp, sz]),
        "nae_spectrum_create": (i, [vp, i, i, i, P(vp)]), "nae_spectrum_put": (i, [vp, vp, sz]),
        "nae_spectrum_available": (sz, [vp]), "nae_spectrum_receive": (i, [vp, vp, sz, P(sz)]),
        "nae_spectrum_destroy": (i, [vp]), "nae_graph4_run": (i, [vp, P(Graph4)]),
        "nae_wsola_plan_make": (i, [i, i, d, d, sz, P(WsolaPlan)]),
        "nae_wsola_block_f32": (i, [vp, i, d, d, P(Sig), sz, i, sz, P(Sig), vp]),
        "nae_wsola_create": (i, [vp, i, i, d, d, P(vp)]),
        "nae_fir_pick_n_fft": (i, [i]), "nae_fir_block_f32": (i, [vp, vp, i, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_fir_design": (i, [i, i, d, d, i, vp]), "nae_fir_create": (i, [vp, vp, i, i, i, P(vp)]),
        "nae_conv_pick_n_fft": (i, [i]), "nae_conv_block_f32": (i, [vp, vp, i, i, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_conv_reverb_taps": (i, [i, d, d]), "nae_conv_design_reverb": (i, [i, d, d, d, d, C.c_uint64, i, vp]),
        "nae_conv_create": (i, [vp, vp, i, i, i, i, P(vp)]),
        "nae_eq_design": (i, [i, i, d, d, d, vp]), "nae_eq_block_f32": (i, [vp, vp, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_eq_create": (i, [vp, vp, i, i, P(vp)]),
        "nae_dyn_design": (i, [i, d, d, d, d, d, d, d, i, P(DynParams)]), "nae_dyn_block_f32": (i, [vp, P(DynParams), P(Sig), sz, i, sz, P(Sig)]),
        "nae_dyn_create": (i, [vp, P(DynParams), i, P(vp)]),
        "nae_dynkey_block_f32": (i, [vp, P(DynKeyParams), P(Sig), P(Sig), sz, i, sz, P(Sig)]), "nae_dynkey_create": (i, [vp, P(DynKeyParams), i, P(vp)]),
        "nae_echo_design": (i, [i, d, d, d, d, d, d, d, i, P(EchoParams)]),
        "nae_echo_block_f32": (i, [vp, P(EchoParams), P(Sig), sz, i, sz, P(Sig)]), "nae_echo_create": (i, [vp, P(EchoParams), i, P(vp)]),
        "nae_mod_design": (i, [i, d, d, d, d, i, d, i, d, d, P(ModParams)]),
        "nae_mod_block_f32": (i, [vp, P(ModParams), P(Sig), sz, i, sz, P(Sig)]), "nae_mod_create": (i, [vp, P(ModParams), i, P(vp)]),
        "nae_sat_latency": (i, [i]), "nae_sat_taps": (i, [i, vp]), "nae_sat_design": (i, [d, d, i, i, d, d, P(SatParams)]),
        "nae_sat_block_f32": (i, [vp, P(SatParams), P(Sig), sz, i, sz, P(Sig)]), "nae_sat_create": (i, [vp, P(SatParams), i, P(vp)]),
        "nae_gate_design": (i, [i, i, d, d, d, d, d, d, d, d, i, P(GateParams)]),
        "nae_gate_block_f32": (i, [vp, P(GateParams), P(Sig), sz, i, sz, P(Sig)]), "nae_gate_create": (i, [vp, P(GateParams), i, P(vp)]),
        "nae_mb_design": (i, [i, i, vp, vp, C.c_uint, C.c_uint, P(MbParams)]),
        "nae_mb_block_f32": (i, [vp, P(MbParams), P(Sig), sz, i, sz, P(Sig)]), "nae_mb_create": (i, [vp, P(MbParams), i, P(vp)]),
        "nae_denoise_design": (i, [d, d, i, i, i, P(DenoiseParams)]), "nae_denoise_profile_f32": (i, [vp, i, P(Sig), sz, i, vp]),
        "nae_denoise_block_f32": (i, [vp, P(DenoiseParams), vp, i, P(Sig), sz, i, sz, P(Sig)]),
        "nae_denoise_create": (i, [vp, P(DenoiseParams), vp, i, i, P(vp)]),
        "nae_lim_design": (i, [i, d, d, d, d, i, i, P(LimParams)]),
        "nae_lim_block_f32": (i, [vp, P(LimParams), P(Sig), sz, i, sz, P(Sig)]), "nae_lim_create": (i, [vp, P(LimParams), i, P(vp)]),
        "nae_dither_design": (i, [i, i, i, C.c_uint64, P(DitherParams)]),
        "nae_dither_block_f32": (i, [vp, P(DitherParams), P(Sig), sz, i, sz, P(Sig)]), "nae_dither_create": (i, [vp, P(DitherParams), i, P(vp)]),
        "nae_hpss_design": (i, [d, d, i, i, i, i, P(HpssParams)]),
        "nae_hpss_block_f32": (i, [vp, P(HpssParams), P(Sig), sz, i, sz, P(Sig)]), "nae_hpss_create": (i, [vp, P(HpssParams), i, P(vp)]),
        "nae_loud_design": (i, [i, d, d, d, P(LoudParams)]), "nae_loud_lufs": (d, [d]),
        "nae_loud_measure_f32": (i, [vp, P(LoudParams), P(Sig), sz, i, sz, vp]), "nae_loud_apply_f32": (i, [vp, vp, P(Sig), sz, i, sz, P(Sig)]),
        "nae_loud_normalize_f32": (i, [vp, P(LoudParams), P(Sig), sz, i, sz, P(Sig), vp]),
        "nae_loud_create": (i, [vp, P(LoudParams), i, P(vp)]), "nae_loud_put": (i, [vp, vp, sz]), "nae_loud_put_host": (i, [vp, vp, sz]),
        "nae_loud_flush": (i, [vp]), "nae_loud_get_result": (i, [vp, P(LoudResult)]), "nae_loud_destroy": (i, [vp]),
    }
    # the seven entries every put / receive handle has besides its create (the spectrum handle has four of them: spelled out above)
    for prefix in HANDLE_PREFIXES:
        sigs.update({prefix + "_put": (i, [vp, vp, sz]), prefix + "_put_host": (i, [vp, vp, sz]), prefix + "_flush": (i, [vp]),
                     prefix + "_available": (sz, [vp]), prefix + "_receive": (i, [vp, vp, sz, P(sz)]),
                     prefix + "_receive_host": (i, [vp, vp, sz, P(sz)]), prefix + "_destroy": (i, [vp])})
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class DeviceArray:
    """A typed device allocation owned by a Context (hipMalloc through nae_malloc)."""

    def __init__(self, ctx: "Context", shape: Sequence[int], dtype=np.float32):
        self.ctx = ctx
        self.shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        ctx._ck(ctx.lib.nae_malloc(ctx.h, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value
        ctx._allocs.add(self)

    @property
    def size(self) -> int:
        return self.nbytes // self.dtype.itemsize

    def at(self, elem_offset: int) -> int:
        return self.ptr + int(elem_offset) * self.dtype.itemsize

    def upload(self, host: np.ndarray) -> "DeviceArray":
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.nbytes, (host.nbytes, self.nbytes)
        self.ctx._ck(self.ctx.lib.nae_memcpy_h2d(self.ctx.h, self.ptr, host.ctypes.data, self.nbytes))
        self.ctx.sync()
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        self.ctx._ck(self.ctx.lib.nae_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes))
        self.ctx.sync()
        return out

    def zero(self) -> "DeviceArray":
        self.ctx._ck(self.ctx.lib.nae_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self

    def free(self) -> None:
        if self.ptr:
            self.ctx.sync()
            self.ctx.lib.nae_free(self.ctx.h, self.ptr)
            self.ptr = 0
            self.ctx._allocs.discard(self)


def _ptr_array(ptrs: Iterable[int]):
    ptrs = list(ptrs)
    return (C.c_void_p * len(ptrs))(*ptrs)


class Context:
    """nae_ctx wrapper.  One per GPU."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.nae_ctx_create(device, C.byref(h))
        if rc != 0:
            why = ("no such device, or a bad assignment in $NAE_DEBUG" if rc == -1 else "no usable HIP device")
            raise NaeError(f"nae_ctx_create(device={device}) failed with {rc}: {why} — this library has no CPU fallback")
        self.h = h
        self.device = device
        self._allocs = set()
        self._pinned = {}

    # -- plumbing
    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise NaeError(f"nae error {rc}: {self.lib.nae_last_error(self.h).decode(errors='replace')}")

    def name(self) -> str:
        return self.lib.nae_device_name(self.h).decode()

    def sync(self) -> None:
        self._ck(self.lib.nae_sync(self.h))

    def poll(self) -> int:
        return self.lib.nae_poll(self.h)

    def set_stream(self, hip_stream: int) -> None:
        self._ck(self.lib.nae_ctx_set_stream(self.h, C.c_void_p(hip_stream)))

    def empty(self, shape, dtype=np.float32) -> DeviceArray:
        return DeviceArray(self, shape, dtype)

    def array(self, host: np.ndarray) -> DeviceArray:
        host = np.ascontiguousarray(host)
        return DeviceArray(self, host.shape, host.dtype).upload(host)

    def close(self) -> None:
        if self.h:
            for a in list(self._allocs):
                a.free()
            self.lib.nae_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def debug_set(self, key: str, value: int) -> "Context":
        """tuning / A-B switch of this context (include/nae_gpu.h lists the keys); returns self so that calls chain"""
        self._ck(self.lib.nae_debug_set(self.h, key.encode(), int(value)))
        return self

    # -- events
    def event(self) -> C.c_void_p:
        e = C.c_void_p()
        self._ck(self.lib.nae_event_create(self.h, C.byref(e)))
        return e

    def destroy_event(self, ev) -> None:
        """events are destroyed BEFORE the context they were created from (include/nae_gpu.h)"""
        rc = self.lib.nae_event_destroy(ev)
        if rc:
            raise NaeError(f"nae_event_destroy failed: {rc}")

    def record(self, ev) -> None:
        self._ck(self.lib.nae_event_record(self.h, ev))

    def query(self, ev) -> int:
        """1 = the work in front of the event's last record is done, 0 = pending (never blocks)"""
        rc = self.lib.nae_event_query(ev)
        if rc < 0:
            raise NaeError(f"nae_event_query failed: {rc}")
        return rc

    def wait_event(self, ev) -> None:
        """work enqueued on this context from now on waits (on the device) for the event's last record"""
        self._ck(self.lib.nae_ctx_wait_event(self.h, ev))

    def elapsed_ms(self, a, b) -> float:
        ms = C.c_float()
        rc = self.lib.nae_event_elapsed_ms(a, b, C.byref(ms))
        if rc:
            raise NaeError(f"nae_event_elapsed_ms failed: {rc}")
        return float(ms.value)

    # -- per-kernel timing / synthetic input
    def prof_enable(self, on: bool = True) -> None:
        self._ck(self.lib.nae_prof_enable(self.h, 1 if on else 0))

    def prof_reset(self) -> None:
        self._ck(self.lib.nae_prof_reset(self.h))

    def prof_report(self) -> dict:
        """{kernel: (total_ms, launches)} accumulated since the last reset"""
        out = {}
        n = self.lib.nae_prof_get(self.h, -1, None, 0, None, None)
        for k in range(n):
            name = C.create_string_buffer(128)
            ms, cnt = C.c_double(), C.c_uint64()
            self.lib.nae_prof_get(self.h, k, name, 128, C.byref(ms), C.byref(cnt))
            out[name.value.decode()] = (ms.value, cnt.value)
        return out

    def pinned(self, shape, dtype=np.float32) -> np.ndarray:
        """numpy view of page-locked host memory (nae_malloc_host); release with free_pinned(array)"""
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._ck(self.lib.nae_malloc_host(self.h, max(nbytes, 16), C.byref(p)))
        buf = (C.c_char * max(nbytes, 16)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        self._pinned[arr.ctypes.data] = p.value
        return arr

    def free_pinned(self, arr: np.ndarray) -> None:
        p = self._pinned.pop(arr.ctypes.data, None)
        if p:
            self.sync()
            self.lib.nae_free_host(self.h, p)

    def diff_words(self, a: int, b: int, n_words: int, d_count: int) -> None:
        """adds the number of differing 32-bit words of device buffers a, b to the device uint64 at d_count (asynchronous)"""
        self._ck(self.lib.nae_debug_diff_u32(self.h, a, b, n_words, d_count))

    def clock_ghz(self) -> float:
        """shader clock the GPU holds right now (probe kernel on the context's stream)"""
        g = C.c_double()
        self._ck(self.lib.nae_debug_clock_ghz(self.h, C.byref(g)))
        return g.value

    def fill_uniform(self, dst: int, n_per_stream: int, stream_stride: int, n_streams: int, first_stream: int = 0,
                     input_index: int = 0) -> None:
        self._ck(self.lib.nae_fill_uniform_f32(self.h, dst, n_per_stream, stream_stride, n_streams, first_stream,
                                               input_index))

    # -- K1
    def gain(self, fmt_dtype, src_planes: Sequence[int], dst_planes: Sequence[int], elems: int, volume: float):
        fn = {np.dtype(np.float32): self.lib.nae_gain_f32, np.dtype(np.int16): self.lib.nae_gain_s16,
              np.dtype(np.int32): self.lib.nae_gain_s32}[np.dtype(fmt_dtype)]
        self._ck(fn(self.h, _ptr_array(src_planes), _ptr_array(dst_planes), len(src_planes), elems, volume))

    def gain_frame(self, fmt: int, src_planes, dst_planes, S: int, ch: int, volume: float) -> int:
        return self.lib.nae_gain_frame(self.h, fmt, _ptr_array(src_planes), _ptr_array(dst_planes), S, ch, volume)

    # -- K2
    def deinterleave(self, src: int, dst_planes: Sequence[int], S: int, ch: int):
        self._ck(self.lib.nae_deinterleave_f32(self.h, src, _ptr_array(dst_planes), S, ch))

    def interleave(self, src_planes: Sequence[int], dst: int, S: int, ch: int):
        self._ck(self.lib.nae_interleave_f32(self.h, _ptr_array(src_planes), dst, S, ch))

    def copy_sig(self, src: Sig, dst: Sig, S: int, ch: int, n_streams: int):
        self._ck(self.lib.nae_copy_sig_f32(self.h, C.byref(src), C.byref(dst), S, ch, n_streams))

    def gain_sig(self, src: Sig, dst: Sig, S: int, ch: int, n_streams: int, volume: float):
        self._ck(self.lib.nae_gain_sig_f32(self.h, C.byref(src), C.byref(dst), S, ch, n_streams, volume))

    # -- K3
    def amix(self, inL: Sequence[int], inR: Sequence[int], vol: Sequence[float], outL: int, outR: int, S: int):
        n = len(inL)
        v = (C.c_float * n)(*[float(x) for x in vol])
        self._ck(self.lib.nae_amix_f32(self.h, _ptr_array(inL), _ptr_array(inR), v, n, outL, outR, S))

    def amix_sig(self, inputs: Sequence[Sig], vol: Sequence[float], out: Sig, S: int, n_streams: int):
        n = len(inputs)
        arr = (Sig * n)(*inputs)
        v = (C.c_float * n)(*[float(x) for x in vol])
        self._ck(self.lib.nae_amix_sig_f32(self.h, arr, v, n, C.byref(out), S, n_streams))

    # -- K4 / K5 / K6
    def bimix(self, ll, lr, rl, rr, bias: float, outL, outR, S: int):
        self._ck(self.lib.nae_bimix_f32(self.h, ll, lr, rl, rr, bias, outL, outR, S))

    def bimix2_downmix(self, l, r, mono, S: int):
        self._ck(self.lib.nae_bimix2_downmix_f32(self.h, l, r, mono, S))

    def bimix2_interleave(self, dst, earlier, later, unaligned: int, aligned: int, earlier_offset: int):
        self._ck(self.lib.nae_bimix2_interleave_f32(self.h, dst, earlier, later, unaligned, aligned, earlier_offset))

    def to_f32_interleaved(self, fmt: int, planes: Sequence[int], S: int, ch: int, dst: int) -> int:
        return self.lib.nae_to_f32_interleaved(self.h, fmt, _ptr_array(planes), S, ch, dst)

    def clamp(self, data: int, n: int):
        self._ck(self.lib.nae_clamp_f32(self.h, data, n))

    # -- K7
    @staticmethod
    def stretch_plan(rate: float, pitch: float, in_len: int, n_fft: int = 1024, formant: int = 0,
                     formant_ratio: Optional[float] = None) -> StretchPlan:
        """n_fft: vocoder frame size 512 / 1024 / 2048 / 4096 (1024 calls nae_stretch_plan_make); formant_ratio: the plan of the formant
        shift with lifter `formant` (nae_stretch_plan_make_shift)"""
        pl = StretchPlan()
        if formant_ratio is not None:
            rc = load_library().nae_stretch_plan_make_shift(rate, pitch, formant_ratio, formant, n_fft, in_len, C.byref(pl))
        elif n_fft == 1024:
            rc = load_library().nae_stretch_plan_make(rate, pitch, in_len, C.byref(pl))
        else:
            rc = load_library().nae_stretch_plan_make_n(rate, pitch, n_fft, in_len, C.byref(pl))
        if rc:
            raise NaeError(f"nae_stretch_plan_make({rate}, {pitch}, n_fft={n_fft}) failed: {rc}")
        return pl

    def stretch_block(self, rate: float, pitch: float, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig,
                      phase_lock: bool = False, n_fft: int = 1024, formant: int = 0, transients: bool = False,
                      formant_ratio: Optional[float] = None, link_channels: bool = False):
        """formant: the lifter of formant preservation (formant_lifter() gives the default), 0 = off; transients: transient preservation
        (nae_stretch_block_n_f32 at every size); formant_ratio: the formant shift with that lifter (nae_stretch_block_formant_shift_f32;
        dst receives stretch_plan(..., formant=, formant_ratio=).out_len frames); link_channels: the channel link (the _n entries, as
        transients)"""
        flags = (STRETCH_PHASE_LOCK if phase_lock else 0) | (STRETCH_TRANSIENTS if transients else 0) | (STRETCH_LINK_CHANNELS if link_channels else 0)
        if formant_ratio is not None:
            self._ck(self.lib.nae_stretch_block_formant_shift_f32(self.h, rate, pitch, flags, n_fft, formant, formant_ratio,
                                                                  C.byref(src), in_len, ch, n_streams, C.byref(dst)))
        elif formant:
            self._ck(self.lib.nae_stretch_block_formant_f32(self.h, rate, pitch, flags, n_fft, formant,
                                                            C.byref(src), in_len, ch, n_streams, C.byref(dst)))
        elif n_fft != 1024 or transients or link_channels:
            self._ck(self.lib.nae_stretch_block_n_f32(self.h, rate, pitch, flags, n_fft, C.byref(src), in_len,
                                                      ch, n_streams, C.byref(dst)))
        elif phase_lock:
            self._ck(self.lib.nae_stretch_block_ex_f32(self.h, rate, pitch, STRETCH_PHASE_LOCK, C.byref(src), in_len, ch, n_streams,
                                                       C.byref(dst)))
        else:
            self._ck(self.lib.nae_stretch_block_f32(self.h, rate, pitch, C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    def debug_pv_tile_phase(self, rate: float, pitch: float, src: Sig, in_len: int, ch: int, n_streams: int,
                            phase_lock: bool = False, n_fft: int = 1024, transients: bool = False, link_channels: bool = False):
        pl = self.stretch_plan(rate, pitch, in_len, n_fft)
        bins = n_fft // 2 + 1
        cap = n_streams * ch * (pl.frames + 1) * bins
        out = np.zeros(cap, np.int32)
        nt, tf = C.c_size_t(), C.c_size_t()
        if n_fft != 1024 or transients or link_channels:
            flags = ((STRETCH_PHASE_LOCK if phase_lock else 0) | (STRETCH_TRANSIENTS if transients else 0)
                     | (STRETCH_LINK_CHANNELS if link_channels else 0))
            self._ck(self.lib.nae_debug_pv_tile_phase_n(self.h, rate, pitch, flags, n_fft, C.byref(src), in_len,
                                                        ch, n_streams, out.ctypes.data, cap, C.byref(nt), C.byref(tf)))
            return out[: n_streams * ch * nt.value * bins].reshape(n_streams, ch, nt.value, bins), tf.value
        if phase_lock:
            self._ck(self.lib.nae_debug_pv_tile_phase_ex(self.h, rate, pitch, STRETCH_PHASE_LOCK, C.byref(src), in_len, ch, n_streams,
                                                         out.ctypes.data, cap, C.byref(nt), C.byref(tf)))
        else:
            self._ck(self.lib.nae_debug_pv_tile_phase(self.h, rate, pitch, C.byref(src), in_len, ch, n_streams,
                                                      out.ctypes.data, cap, C.byref(nt), C.byref(tf)))
        return out[: n_streams * ch * nt.value * BINS].reshape(n_streams, ch, nt.value, BINS), tf.value

    # -- K7 option A: SoundTouch-shaped WSOLA chain
    @staticmethod
    def wsola_plan(sample_rate: int, ch: int, rate: float, pitch: float, in_len: int) -> WsolaPlan:
        pl = WsolaPlan()
        rc = load_library().nae_wsola_plan_make(sample_rate, ch, rate, pitch, in_len, C.byref(pl))
        if rc:
            raise NaeError(f"nae_wsola_plan_make({sample_rate}, {ch}, {rate}, {pitch}) failed: {rc}")
        return pl

    def wsola_block(self, sample_rate: int, rate: float, pitch: float, src: Sig, in_len: int, ch: int, n_streams: int,
                    dst: Sig, offsets_dbg: int = 0):
        self._ck(self.lib.nae_wsola_block_f32(self.h, sample_rate, rate, pitch, C.byref(src), in_len, ch, n_streams,
                                              C.byref(dst), offsets_dbg))

    # -- K8
    def spectrum_frames(self, T: int) -> int:
        return int(self.lib.nae_spectrum_frames(T))

    def spectrum_block(self, src: Sig, T: int, ch: int, n_streams: int, dst: int, dst_stream_stride: int):
        self._ck(self.lib.nae_spectrum_block_f32(self.h, C.byref(src), T, ch, n_streams, dst, dst_stream_stride))

    def spectrum_frames_ex(self, T: int, n_fft: int, hop: int) -> int:
        """frames of T samples at (n_fft, hop); 0 for parameters the library does not support"""
        return int(self.lib.nae_spectrum_frames_ex(T, n_fft, hop))

    def spectrum_block_ex(self, n_fft: int, hop: int, src: Sig, T: int, ch: int, n_streams: int, dst: int, dst_stream_stride: int):
        """any size 256..4096 and hop 1..n_fft; records of n_fft/2 + 1 floats"""
        self._ck(self.lib.nae_spectrum_block_ex_f32(self.h, n_fft, hop, C.byref(src), T, ch, n_streams, dst, dst_stream_stride))

    # -- K9
    @staticmethod
    def fir_pick_n_fft(n_taps: int) -> int:
        """the smallest frame size with n_fft / 2 + 1 >= n_taps; 0 when there is none"""
        return int(load_library().nae_fir_pick_n_fft(n_taps))

    @staticmethod
    def fir_design(kind, sample_rate: int, f_lo: float, f_hi: float, n_taps: int) -> np.ndarray:
        """Kaiser-8 linear-phase taps (nae_fir_design); kind: "lowpass" (f_hi) | "highpass" (f_lo) | "bandpass" | "bandstop", or 0 ... 3"""
        taps = np.empty(max(n_taps, 1), np.float32)
        rc = load_library().nae_fir_design(FIR_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind), sample_rate, f_lo, f_hi, n_taps,
                                           taps.ctypes.data)
        if rc:
            raise NaeError(f"nae_fir_design({kind}, {sample_rate}, {f_lo}, {f_hi}, {n_taps}) failed: {rc}")
        return taps[:n_taps]

    def fir_block(self, taps: np.ndarray, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig, n_fft: int = 0):
        """y = h * x per stream and channel by overlap-save at frame size n_fft (0: fir_pick_n_fft(len(taps))); dst receives in_len frames"""
        taps = np.ascontiguousarray(taps, np.float32)
        self._ck(self.lib.nae_fir_block_f32(self.h, taps.ctypes.data, taps.size, n_fft, C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K10
    @staticmethod
    def conv_pick_n_fft(n_taps: int) -> int:
        """the smallest frame size with at most 16 partitions of n_fft / 2 taps, else 4096; 0 when the response is not supported"""
        return int(load_library().nae_conv_pick_n_fft(n_taps))

    @staticmethod
    def conv_reverb_taps(sample_rate: int, rt60_s: float, predelay_s: float) -> int:
        """length of a designed response to its -60 dB point (nae_conv_reverb_taps)"""
        n = int(load_library().nae_conv_reverb_taps(sample_rate, rt60_s, predelay_s))
        if n < 0:
            raise NaeError(f"nae_conv_reverb_taps({sample_rate}, {rt60_s}, {predelay_s}) failed: {n}")
        return n

    @staticmethod
    def conv_design_reverb(sample_rate: int, rt60_s: float, predelay_s: float, dry: float, wet: float, seed: int,
                           n_taps: Optional[int] = None) -> np.ndarray:
        """exponentially decaying noise of unit energy behind the pre-delay, h = wet r + dry delta (nae_conv_design_reverb)"""
        lib = load_library()
        if n_taps is None:
            n_taps = Context.conv_reverb_taps(sample_rate, rt60_s, predelay_s)
        taps = np.empty(max(n_taps, 1), np.float32)
        rc = lib.nae_conv_design_reverb(sample_rate, rt60_s, predelay_s, dry, wet, seed, n_taps, taps.ctypes.data)
        if rc:
            raise NaeError(f"nae_conv_design_reverb({sample_rate}, {rt60_s}, {predelay_s}, {dry}, {wet}, {seed}, {n_taps}) failed: {rc}")
        return taps[:n_taps]

    def conv_block(self, taps: np.ndarray, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig, n_fft: int = 0):
        """y = h_c * x per stream and channel by partitioned overlap-save; taps [L] (one set) or [taps_ch][L]; dst receives in_len frames"""
        taps = np.ascontiguousarray(taps, np.float32)
        taps_ch, n_taps = (1, taps.size) if taps.ndim == 1 else taps.shape
        self._ck(self.lib.nae_conv_block_f32(self.h, taps.ctypes.data, n_taps, taps_ch, n_fft, C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K11
    @staticmethod
    def eq_design(kind, sample_rate: int, freq: float, gain_db: float = 0.0, q: float = 0.7071) -> np.ndarray:
        """one section (b0, b1, b2, a1, a2) by the Audio EQ Cookbook's forms (nae_eq_design); kind: a name of EQ_KINDS or its number"""
        k = EQ_KINDS.index(kind) if isinstance(kind, str) else int(kind)
        coef = np.empty(5, np.float64)
        rc = load_library().nae_eq_design(k, sample_rate, freq, gain_db, q, coef.ctypes.data)
        if rc:
            raise NaeError(f"nae_eq_design({kind}, {sample_rate}, {freq}, {gain_db}, {q}) failed: {rc}")
        return coef

    def eq_block(self, coef: np.ndarray, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the biquad cascade coef[S][5] (doubles; a0 = 1) over every stream and channel; dst receives in_len frames"""
        coef = np.ascontiguousarray(coef, np.float64).reshape(-1, 5)
        self._ck(self.lib.nae_eq_block_f32(self.h, coef.ctypes.data, coef.shape[0], C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K16
    @staticmethod
    def echo_design(sample_rate: int, delay_s: float = 0.35, delay_s_right: Optional[float] = None, feedback: float = 0.4, damp_hz: float = 0.0,
                    lowcut_hz: float = 0.0, wet: float = 0.35, dry: float = 1.0, cross: bool = False) -> "EchoParams":
        """the echo's parameters from seconds and corner frequencies (nae_echo_design); delay_s_right None: the left delay"""
        out = EchoParams()
        right = delay_s if delay_s_right is None else delay_s_right
        rc = load_library().nae_echo_design(sample_rate, delay_s, right, feedback, damp_hz, lowcut_hz, wet, dry, int(cross), C.byref(out))
        if rc:
            raise NaeError(f"nae_echo_design({sample_rate}, {delay_s}, {right}, {feedback}, {damp_hz}, {lowcut_hz}, {wet}, {dry}, {cross}) failed: {rc}")
        return out

    def echo_block(self, params: "EchoParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the echo `params` over every stream (nae_echo_block_f32); dst receives in_len frames"""
        self._ck(self.lib.nae_echo_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K17
    @staticmethod
    def mod_design(sample_rate: int, rate_hz: float = 0.8, delay_ms: float = 12.0, depth_ms: float = 3.0, feedback: float = 0.0, voices: int = 3,
                   spread: float = 0.5, shape: str = "sine", wet: float = 0.5, dry: float = 1.0) -> "ModParams":
        """the modulated delay's parameters from milliseconds and hertz (nae_mod_design); the defaults are a chorus"""
        out = ModParams()
        rc = load_library().nae_mod_design(sample_rate, rate_hz, delay_ms, depth_ms, feedback, voices, spread, MOD_SHAPES.index(shape), wet, dry, C.byref(out))
        if rc:
            raise NaeError(f"nae_mod_design({sample_rate}, {rate_hz}, {delay_ms}, {depth_ms}, {feedback}, {voices}, {spread}, {shape}, {wet}, {dry}) failed: {rc}")
        return out

    def mod_block(self, params: "ModParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the modulated delay `params` over every stream (nae_mod_block_f32); dst receives in_len frames"""
        self._ck(self.lib.nae_mod_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K18
    @staticmethod
    def sat_latency(oversample: int) -> int:
        """the saturation's latency in samples (nae_sat_latency): 0 at 1, 32 at 2, 4 and 8, -1 otherwise"""
        return load_library().nae_sat_latency(oversample)

    @staticmethod
    def sat_taps(oversample: int) -> np.ndarray:
        """the anti-alias prototype hd of an oversampling factor (nae_sat_taps): 32 M + 1 taps, none at 1"""
        taps = np.empty(2 * SAT_HALF * SAT_MAX_OS + 1, np.float32)
        n = load_library().nae_sat_taps(oversample, taps.ctypes.data)
        return taps[:n].copy()

    @staticmethod
    def sat_design(drive_db: float = 12.0, bias: float = 0.0, curve: str = "soft", oversample: int = 4, output_db: float = 0.0,
                   mix: float = 1.0) -> "SatParams":
        """the saturation's parameters from decibels and a mix (nae_sat_design)"""
        out = SatParams()
        rc = load_library().nae_sat_design(drive_db, bias, SAT_CURVES.index(curve), oversample, output_db, mix, C.byref(out))
        if rc:
            raise NaeError(f"nae_sat_design({drive_db}, {bias}, {curve}, {oversample}, {output_db}, {mix}) failed: {rc}")
        return out

    def sat_block(self, params: "SatParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the saturation `params` over every stream (nae_sat_block_f32); dst receives in_len frames and must not be src"""
        self._ck(self.lib.nae_sat_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K19
    @staticmethod
    def gate_design(sample_rate: int, mode: str = "gate", threshold_db: float = -40.0, hysteresis_db: float = 3.0, range_db: float = 60.0,
                    ratio: float = 2.0, attack_s: float = 0.001, hold_s: float = 0.05, release_s: float = 0.1, lookahead_s: float = 0.0,
                    link: bool = True) -> "GateParams":
        """the gate's parameters from decibels and times (nae_gate_design); mode "expander" reads `ratio`"""
        out = GateParams()
        rc = load_library().nae_gate_design(sample_rate, GATE_MODES.index(mode), threshold_db, hysteresis_db, range_db, ratio, attack_s, hold_s,
                                            release_s, lookahead_s, int(link), C.byref(out))
        if rc:
            raise NaeError(f"nae_gate_design({sample_rate}, {mode}, {threshold_db}, {hysteresis_db}, {range_db}, {ratio}, {attack_s}, {hold_s}, "
                           f"{release_s}, {lookahead_s}, {link}) failed: {rc}")
        return out

    def gate_block(self, params: "GateParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the gate / expander `params` over every stream (nae_gate_block_f32); dst receives in_len frames, compensated for the look-ahead"""
        self._ck(self.lib.nae_gate_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K20
    @staticmethod
    def mb_design(sample_rate: int, crossover_hz, bands, mute_mask: int = 0, bypass_mask: int = 0) -> "MbParams":
        """the multiband compressor's parameters from len(bands) - 1 ascending crossover frequencies and the bands' DynParams (nae_mb_design)"""
        xs = np.ascontiguousarray(crossover_hz, np.float64).reshape(-1)
        if len(bands) != xs.size + 1:
            raise NaeError(f"nae_mb_design: {xs.size} crossovers need {xs.size + 1} bands, not {len(bands)}")
        recs = (DynParams * max(len(bands), 1))(*bands)
        out = MbParams()
        rc = load_library().nae_mb_design(sample_rate, len(bands), xs.ctypes.data, C.addressof(recs), mute_mask, bypass_mask, C.byref(out))
        if rc:
            raise NaeError(f"nae_mb_design({sample_rate}, {xs.tolist()}, {len(bands)} bands, {mute_mask}, {bypass_mask}) failed: {rc}")
        return out

    def mb_block(self, params: "MbParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the multiband compressor `params` over every stream (nae_mb_block_f32); dst receives in_len frames, compensated for the look-ahead"""
        self._ck(self.lib.nae_mb_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K12
    @staticmethod
    def dyn_design(sample_rate: int, threshold_db: float = -18.0, ratio: float = 4.0, knee_db: float = 6.0, attack_s: float = 0.005,
                   release_s: float = 0.1, lookahead_s: float = 0.0, makeup_db: float = 0.0, link: bool = True) -> "DynParams":
        """the parameters of the dynamics processor from times and a ratio (nae_dyn_design); ratio = float("inf") is a limiter"""
        out = DynParams()
        rc = load_library().nae_dyn_design(sample_rate, threshold_db, ratio, knee_db, attack_s, release_s, lookahead_s, makeup_db, int(link),
                                           C.byref(out))
        if rc:
            raise NaeError(f"nae_dyn_design({sample_rate}, {threshold_db}, {ratio}, {knee_db}, {attack_s}, {release_s}, {lookahead_s}, "
                           f"{makeup_db}, {link}) failed: {rc}")
        return out

    def dynkey_block(self, params: "DynKeyParams", src: Sig, key: Optional[Sig], in_len: int, ch: int, n_streams: int, dst: Sig):
        """the keyed dynamics (nae_dynkey_block_f32): key is None exactly when params.key_ch is 0"""
        self._ck(self.lib.nae_dynkey_block_f32(self.h, C.byref(params), C.byref(src), C.byref(key) if key is not None else None, in_len, ch,
                                               n_streams, C.byref(dst)))

    def dyn_block(self, params: "DynParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the compressor / limiter `params` over every stream; dst receives in_len frames, compensated for the look-ahead"""
        self._ck(self.lib.nae_dyn_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K13
    @staticmethod
    def denoise_design(reduction_db: float = 12.0, sensitivity_db: float = 6.0, n_fft: int = 2048, time_smooth: int = 2,
                       freq_smooth: int = 2) -> "DenoiseParams":
        """the parameters of the spectral gate from decibels (nae_denoise_design)"""
        out = DenoiseParams()
        rc = load_library().nae_denoise_design(reduction_db, sensitivity_db, n_fft, time_smooth, freq_smooth, C.byref(out))
        if rc:
            raise NaeError(f"nae_denoise_design({reduction_db}, {sensitivity_db}, {n_fft}, {time_smooth}, {freq_smooth}) failed: {rc}")
        return out

    @staticmethod
    def hpss_design(harmonic_db: float = 0.0, percussive_db: float = -120.0, n_fft: int = 2048, time_span: int = 8, freq_span: int = 8,
                    mask: str = "soft") -> "HpssParams":
        """the parameters of the harmonic/percussive separation from decibels (nae_hpss_design); a level of -120 dB is gain 0"""
        out = HpssParams()
        rc = load_library().nae_hpss_design(harmonic_db, percussive_db, n_fft, time_span, freq_span, HPSS_MASKS.index(mask), C.byref(out))
        if rc:
            raise NaeError(f"nae_hpss_design({harmonic_db}, {percussive_db}, {n_fft}, {time_span}, {freq_span}, {mask}) failed: {rc}")
        return out

    def hpss_block(self, params: "HpssParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the separation `params` over every stream (nae_hpss_block_f32); dst receives in_len frames"""
        self._ck(self.lib.nae_hpss_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K22
    @staticmethod
    def lim_design(sample_rate: int, ceiling_db: float = -1.0, gain_db: float = 0.0, release_s: float = 0.1, lookahead_s: float = 0.0015,
                   true_peak: bool = True, link: bool = True) -> "LimParams":
        """the limiter's parameters from decibels and times (nae_lim_design)"""
        out = LimParams()
        rc = load_library().nae_lim_design(sample_rate, ceiling_db, gain_db, release_s, lookahead_s, int(true_peak), int(link), C.byref(out))
        if rc:
            raise NaeError(f"nae_lim_design({sample_rate}, {ceiling_db}, {gain_db}, {release_s}, {lookahead_s}, {true_peak}, {link}) failed: {rc}")
        return out

    def lim_block(self, params: "LimParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the limiter `params` over every stream (nae_lim_block_f32); dst receives in_len frames, compensated for the look-ahead"""
        self._ck(self.lib.nae_lim_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K23
    @staticmethod
    def dither_design(bits: int = 16, kind: str = "triangular", shaping: str = "none", seed: int = 1) -> "DitherParams":
        """the dither's parameters from the names of the kind and of the shaping preset (nae_dither_design)"""
        if kind not in DITHER_KINDS or shaping not in DITHER_SHAPINGS:
            raise NaeError(f"dither_design: kind {kind!r} or shaping {shaping!r} is not a name of DITHER_KINDS / DITHER_SHAPINGS")
        out = DitherParams()
        rc = load_library().nae_dither_design(bits, DITHER_KINDS.index(kind), DITHER_SHAPINGS.index(shaping), seed, C.byref(out))
        if rc:
            raise NaeError(f"nae_dither_design({bits}, {kind}, {shaping}, {seed}) failed: {rc}")
        return out

    def dither_block(self, params: "DitherParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the dither `params` over every stream (nae_dither_block_f32); dst receives in_len frames on the grid of params.bits bits"""
        self._ck(self.lib.nae_dither_block_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    def denoise_profile(self, n_fft: int, src: Sig, length: int, ch: int, profile_ptr: int):
        """the noise powers [ch][n_fft / 2 + 1] of the excerpt's whole frames into device memory at profile_ptr (asynchronous)"""
        self._ck(self.lib.nae_denoise_profile_f32(self.h, n_fft, C.byref(src), length, ch, profile_ptr))

    def denoise_block(self, params: "DenoiseParams", profile_ptr: int, profile_ch: int, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """the spectral gate `params` against the device profile [profile_ch][n_fft / 2 + 1] over every stream; dst receives in_len frames"""
        self._ck(self.lib.nae_denoise_block_f32(self.h, C.byref(params), profile_ptr, profile_ch, C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    # -- K14
    @staticmethod
    def loud_design(sample_rate: int, target_lufs: float = -14.0, ceiling_dbtp: float = -1.0, max_gain_db: float = 20.0) -> "LoudParams":
        """the K-weighting at sample_rate and the levels of the normalizer as energies and linear gains (nae_loud_design)"""
        out = LoudParams()
        rc = load_library().nae_loud_design(sample_rate, target_lufs, ceiling_dbtp, max_gain_db, C.byref(out))
        if rc:
            raise NaeError(f"nae_loud_design({sample_rate}, {target_lufs}, {ceiling_dbtp}, {max_gain_db}) failed: {rc}")
        return out

    def loud_measure(self, params: "LoudParams", src: Sig, in_len: int, ch: int, n_streams: int, results_ptr: int):
        """BS.1770 loudness, peaks and normalizing gain of every stream into n_streams nae_loud_result records at results_ptr (asynchronous)"""
        self._ck(self.lib.nae_loud_measure_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, results_ptr))

    def loud_apply(self, results_ptr: int, src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig):
        """every stream times the gain_f32 of its record at results_ptr"""
        self._ck(self.lib.nae_loud_apply_f32(self.h, results_ptr, C.byref(src), in_len, ch, n_streams, C.byref(dst)))

    def loud_normalize(self, params: "LoudParams", src: Sig, in_len: int, ch: int, n_streams: int, dst: Sig, results_ptr: int = 0):
        """loud_measure, then loud_apply; results_ptr 0: the records stay in the library's workspace"""
        self._ck(self.lib.nae_loud_normalize_f32(self.h, C.byref(params), C.byref(src), in_len, ch, n_streams, C.byref(dst), results_ptr or None))

    def loud_results(self, results_ptr: int, n_streams: int):
        """the n_streams records at results_ptr, on the host (waits for the stream)"""
        out = (LoudResult * n_streams)()
        self._ck(self.lib.nae_memcpy_d2h(self.h, C.addressof(out), results_ptr, C.sizeof(out)))
        self.sync()
        return list(out)

    # -- graph
    def graph4(self, g: Graph4):
        self._ck(self.lib.nae_graph4_run(self.h, C.byref(g)))

    def graph4_stages(self, g: Graph4, mask: int):
        """stages of the graph: 1 = mix (+ transposer when first), 2 = rest of the pitch node, 4 = spectrum"""
        self._ck(self.lib.nae_debug_graph4_stages(self.h, C.byref(g), mask))


def formant_lifter(sample_rate: int, n_fft: int = 1024) -> int:
    """the default lifter of formant preservation (nae_stretch_formant_lifter); 0 for an unsupported size"""
    return int(load_library().nae_stretch_formant_lifter(sample_rate, n_fft))


class _Handle:
    """What the streaming handles share: put / put_host / flush / available / receive / receive_host / close on the entries `_prefix`_*.
    A subclass's __init__ calls this one and then its create entry on self.h."""
    _prefix = ""

    def __init__(self, ctx: Context, channels: int):
        self.ctx, self.ch, self.h = ctx, channels, C.c_void_p()

    def _fn(self, name: str):
        return getattr(self.ctx.lib, f"{self._prefix}_{name}")

    def put(self, dev_ptr: int, frames: int) -> None:
        self.ctx._ck(self._fn("put")(self.h, dev_ptr, frames))

    def put_host(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, np.float32)
        self.ctx._ck(self._fn("put_host")(self.h, x.ctypes.data, x.size // self.ch))

    def flush(self) -> None:
        self.ctx._ck(self._fn("flush")(self.h))

    def available(self) -> int:
        return self._fn("available")(self.h)

    def receive(self, dev_ptr: int, max_frames: int) -> int:
        got = C.c_size_t()
        self.ctx._ck(self._fn("receive")(self.h, dev_ptr, max_frames, C.byref(got)))
        return got.value

    def receive_host(self, max_frames: Optional[int] = None) -> np.ndarray:
        n = self.available() if max_frames is None else max_frames
        out = np.empty(max(n, 1) * self.ch, np.float32)
        got = C.c_size_t()
        self.ctx._ck(self._fn("receive_host")(self.h, out.ctypes.data, n, C.byref(got)))
        return out[: got.value * self.ch]

    def close(self) -> None:
        if self.h:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Stretcher(_Handle):
    """The SoundTouch-shaped streaming handle (nae_stretch_create_ex; nae_stretch_create_n for an n_fft other than 1024;
    nae_stretch_create_formant with a formant lifter; nae_stretch_create_formant_shift with a formant_ratio): put interleaved f32, flush,
    receive."""

    _prefix = "nae_stretch"

    def __init__(self, ctx: Context, sample_rate: int, channels: int, rate: float, pitch: float, phase_lock: bool = False,
                 n_fft: int = 1024, formant: int = 0, transients: bool = False, formant_ratio: Optional[float] = None,
                 link_channels: bool = False):
        super().__init__(ctx, channels)
        flags = (STRETCH_PHASE_LOCK if phase_lock else 0) | (STRETCH_TRANSIENTS if transients else 0) | (STRETCH_LINK_CHANNELS if link_channels else 0)
        if formant_ratio is not None:
            ctx._ck(ctx.lib.nae_stretch_create_formant_shift(ctx.h, sample_rate, channels, rate, pitch, flags, n_fft, formant, formant_ratio,
                                                             C.byref(self.h)))
        elif formant:
            ctx._ck(ctx.lib.nae_stretch_create_formant(ctx.h, sample_rate, channels, rate, pitch, flags, n_fft, formant, C.byref(self.h)))
        elif n_fft != 1024 or transients or link_channels:
            ctx._ck(ctx.lib.nae_stretch_create_n(ctx.h, sample_rate, channels, rate, pitch, flags, n_fft, C.byref(self.h)))
        else:
            ctx._ck(ctx.lib.nae_stretch_create_ex(ctx.h, sample_rate, channels, rate, pitch, flags, C.byref(self.h)))


class Fir(_Handle):
    """The FIR filter's streaming handle (nae_fir_create): put interleaved f32, flush (the tail: len(taps) - 1 more frames), receive."""

    _prefix = "nae_fir"

    def __init__(self, ctx: Context, taps: np.ndarray, channels: int, n_fft: int = 0):
        super().__init__(ctx, channels)
        taps = np.ascontiguousarray(taps, np.float32)
        ctx._ck(ctx.lib.nae_fir_create(ctx.h, taps.ctypes.data, taps.size, n_fft, channels, C.byref(self.h)))


class Conv(_Handle):
    """The long convolution's streaming handle (nae_conv_create): put interleaved f32, flush (the tail: n_taps - 1 more frames), receive.
    taps [L] (one set for every channel) or [channels][L]."""

    _prefix = "nae_conv"

    def __init__(self, ctx: Context, taps: np.ndarray, channels: int, n_fft: int = 0):
        super().__init__(ctx, channels)
        taps = np.ascontiguousarray(taps, np.float32)
        taps_ch, n_taps = (1, taps.size) if taps.ndim == 1 else taps.shape
        ctx._ck(ctx.lib.nae_conv_create(ctx.h, taps.ctypes.data, n_taps, taps_ch, n_fft, channels, C.byref(self.h)))


class Eq(_Handle):
    """The biquad cascade's streaming handle (nae_eq_create): put interleaved f32, flush (the partial last chunk), receive.  coef [S][5]."""

    _prefix = "nae_eq"

    def __init__(self, ctx: Context, coef: np.ndarray, channels: int):
        super().__init__(ctx, channels)
        coef = np.ascontiguousarray(coef, np.float64).reshape(-1, 5)
        ctx._ck(ctx.lib.nae_eq_create(ctx.h, coef.ctypes.data, coef.shape[0], channels, C.byref(self.h)))


class Dyn(_Handle):
    """The dynamics processor's streaming handle (nae_dyn_create): put interleaved f32, flush, receive.  Before the flush the whole chunks
    whose look-ahead is complete are available; the flush releases the rest."""

    _prefix = "nae_dyn"

    def __init__(self, ctx: Context, params: DynParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_dyn_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class DynKey(_Handle):
    """The keyed dynamics' streaming handle (nae_dynkey_create): a put carries frames of channels + key_ch floats, the signal's channels and
    then the key's; a receive delivers frames of `channels` floats.  Availability and flush as Dyn's."""

    _prefix = "nae_dynkey"

    def __init__(self, ctx: Context, params: DynKeyParams, channels: int):
        super().__init__(ctx, channels)
        self.in_width = channels + params.key_ch
        ctx._ck(ctx.lib.nae_dynkey_create(ctx.h, C.byref(params), channels, C.byref(self.h)))

    def put_host(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, np.float32)
        self.ctx._ck(self._fn("put_host")(self.h, x.ctypes.data, x.size // self.in_width))


class Echo(_Handle):
    """The echo's streaming handle (nae_echo_create): put interleaved f32, flush (the partial last chunk; the echoes' tail is dropped), receive."""

    _prefix = "nae_echo"

    def __init__(self, ctx: Context, params: EchoParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_echo_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Mod(_Handle):
    """The modulated delay's streaming handle (nae_mod_create): put interleaved f32, flush (the partial last chunk; the tail is dropped), receive."""

    _prefix = "nae_mod"

    def __init__(self, ctx: Context, params: ModParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_mod_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Sat(_Handle):
    """The saturation's streaming handle (nae_sat_create): put interleaved f32, flush (the latency's tail: in_len + D frames come out in all), receive."""

    _prefix = "nae_sat"

    def __init__(self, ctx: Context, params: SatParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_sat_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Gate(_Handle):
    """The gate's streaming handle (nae_gate_create): put interleaved f32, flush, receive.  Before the flush the whole chunks of 1024 frames
    with `lookahead` frames behind them are available."""

    _prefix = "nae_gate"

    def __init__(self, ctx: Context, params: GateParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_gate_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Multiband(_Handle):
    """The multiband compressor's streaming handle (nae_mb_create): put interleaved f32, flush, receive.  Before the flush the whole chunks of
    1024 frames with `lookahead` frames behind them are available."""

    _prefix = "nae_mb"

    def __init__(self, ctx: Context, params: MbParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_mb_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Denoise(_Handle):
    """The spectral gate's streaming handle (nae_denoise_create): put interleaved f32, flush, receive.  The device profile
    [profile_ch][n_fft / 2 + 1] is copied at creation.  Before the flush the hop blocks with time_smooth + 3 blocks behind them are available."""

    _prefix = "nae_denoise"

    def __init__(self, ctx: Context, params: DenoiseParams, profile_ptr: int, profile_ch: int, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_denoise_create(ctx.h, C.byref(params), profile_ptr, profile_ch, channels, C.byref(self.h)))


class Limiter(_Handle):
    """The limiter's streaming handle (nae_lim_create): put interleaved f32, flush, receive.  Before the flush the whole chunks of 1024 frames
    with `lookahead` frames, and 6 more with `true_peak`, behind them are available."""

    _prefix = "nae_lim"

    def __init__(self, ctx: Context, params: LimParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_lim_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Dither(_Handle):
    """The dither's streaming handle (nae_dither_create): put interleaved f32, flush, receive.  No latency: every frame put is available
    after that put."""

    _prefix = "nae_dither"

    def __init__(self, ctx: Context, params: DitherParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_dither_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


dither_design = Context.dither_design


class Hpss(_Handle):
    """The separation's streaming handle (nae_hpss_create): put interleaved f32, flush, receive.  Before the flush the hop blocks with
    time_span + 3 blocks behind them are available."""

    _prefix = "nae_hpss"

    def __init__(self, ctx: Context, params: HpssParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_hpss_create(ctx.h, C.byref(params), channels, C.byref(self.h)))


class Loud(_Handle):
    """The loudness meter's handle (nae_loud_create): put interleaved f32, flush, result().  It hands out no samples: available() is 0 and there
    is nothing to receive."""

    _prefix = "nae_loud"

    def __init__(self, ctx: Context, params: LoudParams, channels: int):
        super().__init__(ctx, channels)
        ctx._ck(ctx.lib.nae_loud_create(ctx.h, C.byref(params), channels, C.byref(self.h)))

    def available(self) -> int:
        return 0

    def result(self) -> LoudResult:
        """the record behind the flush (NAE_ERR_STATE in front of it)"""
        out = LoudResult()
        self.ctx._ck(self.ctx.lib.nae_loud_get_result(self.h, C.byref(out)))
        return out
