"""nodey-audio-editor_amd — MI355X-native per-node audio DSP (gain, split/merge, mix, tempo/pitch, FFT spectrum, FIR filter, long convolution, equalizer, dynamics, noise reduction, loudness, echo, modulated delay, saturation, gate, multiband compressor, harmonic/percussive separation, limiter, dither).

The product is ``libnae_gpu.so`` (HIP kernels for gfx950 behind the C ABI of ``include/nae_gpu.h``) plus the
C++ adapter classes in ``host/`` that mirror the reference's ``infra::Processor`` plugin interface.  This Python
package is only the ctypes binding the tests and ``bench.py`` drive the C ABI with.  It never computes on the
CPU: if the shared library is missing or HIP is unusable, it raises.

The directory name carries a hyphen (it mirrors the upstream repository name), so import it through
``naeload.load()`` at the repo root, which registers it as ``nodey_audio_editor_amd``.
"""
from .binding import (  # noqa: F401
    NaeError, Context, DeviceArray, Sig, StretchPlan, WsolaPlan, Graph4, Stretcher, Fir, Conv, Eq, Dyn, DynParams, DynKey, DynKeyParams, DYNKEY_MAX_SECTIONS, Echo, EchoParams, ECHO_MIN_DELAY, ECHO_MAX_DELAY, ECHO_MAX_SECTIONS, ECHO_MAX_FEEDBACK, Mod, ModParams, MOD_MIN_DELAY, MOD_MAX_DELAY, MOD_MAX_VOICES, MOD_MAX_FEEDBACK, MOD_SHAPES, Sat, SatParams, SAT_HALF, SAT_MAX_OS, SAT_CURVES, Gate, GateParams, GATE_MAX_HOLD, GATE_MODES, Multiband, MbParams, MB_MAX_BANDS, MB_MAX_SECTIONS, Denoise, DenoiseParams, Hpss, HpssParams, Limiter, LimParams, LIM_MAX_LOOKAHEAD, LIM_TP_REACH, Dither, DitherParams, dither_design, DITHER_MIN_BITS, DITHER_MAX_BITS, DITHER_MAX_TAPS, DITHER_KINDS, DITHER_SHAPINGS, HPSS_MAX_SPAN, HPSS_MASKS, Loud, LoudParams, LoudResult, FIR_SIZES, FIR_KINDS, EQ_KINDS, STRETCH_PHASE_LOCK, STRETCH_TRANSIENTS, STRETCH_LINK_CHANNELS, FORMANT_SHIFT_MIN, FORMANT_SHIFT_MAX,
    formant_lifter, lib_path, load_library,
    build_library,
    FMT_S16, FMT_S32, FMT_FLT, FMT_S16P, FMT_S32P, FMT_FLTP, FFT_N, HOP, BINS, EXPORTED_SYMBOLS,
)
