/* nae_dsp_spec.h — numeric constants of the builder-defined DSP nodes (K7 tempo/pitch, K8 spectrum).
 *
 * The reference has NO code for the FFT spectrum node (FFTW is only a declared dependency,
 * /root/reference/xmake.lua:15,33) and delegates tempo/pitch to SoundTouch 2.3.2, which is not in the
 * tree (/root/reference/src/processor/audio-velocity.cpp:286,369-385).  BASELINE.json:north_star prescribes
 * "hand-written radix-2/4 LDS FFTs plus phase-vocoder analysis/resynthesis", so the algorithm is specified
 * HERE, once, and implemented twice: by the HIP kernels (nodey-audio-editor_amd/csrc) and, independently,
 * by the CPU oracle (oracle/).  Only constants live in this header — no shared code.
 *
 * The full algorithm text is DESIGN.md §3 ("K7/K8 specification").
 */
#ifndef NAE_DSP_SPEC_H
#define NAE_DSP_SPEC_H

/* STFT geometry (BASELINE.json configs[2]: "1024-pt FFT, 75 % overlap") */
#define NAE_FFT_N 1024          /* real frame length                       */
#define NAE_FFT_NC 512          /* packed complex length (N/2)             */
#define NAE_FFT_BINS 513        /* r2c bins k = 0..N/2                     */
#define NAE_HOP 256             /* synthesis hop / spectrum hop (N/4)      */
#define NAE_OLA_GAIN (2.0f / 3.0f) /* 1 / sum_t hann^2 at hop N/4 = 1/1.5  */
#define NAE_FORMANT_MAX_GAIN 16.0f /* formant preservation: largest envelope gain of a bin ("Formant preservation") */
/* formant shift ("Formant shift"): the range of formant_ratio, +-24 semitones */
#define NAE_FORMANT_SHIFT_MIN 0.25
#define NAE_FORMANT_SHIFT_MAX 4.0
/* K9 FIR filter ("K9 FIR filter"): overlap-save at frame size N = 512 ... 4096 with N / 2 new samples per block, so at most
 * N / 2 + 1 taps — 2049 at 4096; the designs are Kaiser-windowed sincs with the transposer's beta; a tile the library chooses has at least
 * NAE_FIR_MIN_TILE blocks (it re-reads half a block at its head) */
#define NAE_FIR_MAX_TAPS 2049
#define NAE_FIR_KAISER_BETA 8.0
#define NAE_FIR_MIN_TILE 8
/* K10 long convolution ("K10 long convolution"): uniformly partitioned overlap-save, P = ceil(L / (N / 2)) partitions at frame size
 * N = 512 ... 4096; nae_conv_pick_n_fft takes the smallest N with at most NAE_CONV_PICK_PARTS partitions (a rule, not a measurement), else 4096 */
#define NAE_CONV_MAX_TAPS 262144
#define NAE_CONV_MAX_PARTS 512
#define NAE_CONV_PICK_PARTS 16
/* K11 biquad cascade ("K11 biquad cascade"): up to NAE_EQ_MAX_SECTIONS sections in double, tiled in time: a lane runs
 * NAE_EQ_LANE samples, 64 lanes make a chunk of NAE_EQ_CHUNK samples on a grid that starts at the stream's sample 0.  The tiling is part of
 * the specification: the bits depend on it. */
#define NAE_EQ_MAX_SECTIONS 16
#define NAE_EQ_LANE 16
#define NAE_EQ_CHUNK (64 * NAE_EQ_LANE)
/* nae_eq_design: the kinds, and the limits of q and gain_db */
#define NAE_EQ_PEAK 0
#define NAE_EQ_LOWSHELF 1
#define NAE_EQ_HIGHSHELF 2
#define NAE_EQ_LOWPASS 3
#define NAE_EQ_HIGHPASS 4
#define NAE_EQ_NOTCH 5
#define NAE_EQ_MIN_Q 0.1
#define NAE_EQ_MAX_Q 40.0
#define NAE_EQ_MAX_GAIN_DB 24.0
/* K12 dynamics ("K12 dynamics"): a compressor / look-ahead limiter in double, tiled in time as K11: a lane runs NAE_DYN_LANE
 * samples, 64 lanes make a chunk of NAE_DYN_CHUNK samples on a grid that starts at the stream's sample 0; the look-ahead reaches at most
 * NAE_DYN_MAX_LOOKAHEAD samples, one chunk; a zero sample stands at NAE_DYN_FLOOR_DB.  The tiling is part of the specification. */
#define NAE_DYN_LANE 16
#define NAE_DYN_CHUNK (64 * NAE_DYN_LANE)
#define NAE_DYN_MAX_LOOKAHEAD 1024
#define NAE_DYN_FLOOR_DB (-1000.0)
/* nae_dyn_design: the ranges of its arguments (ratio: at least 1, INFINITY a limiter) */
#define NAE_DYN_MIN_THRESHOLD_DB (-60.0)
#define NAE_DYN_MAX_THRESHOLD_DB 0.0
#define NAE_DYN_MAX_KNEE_DB 24.0
#define NAE_DYN_MAX_ATTACK_S 0.5
#define NAE_DYN_MIN_RELEASE_S 0.001
#define NAE_DYN_MAX_RELEASE_S 5.0
#define NAE_DYN_MAX_MAKEUP_DB 24.0
/* K15 keyed dynamics ("K15 keyed dynamics"): K12 whose detector reads a key through at most this many K11 sections */
#define NAE_DYNKEY_MAX_SECTIONS 4
/* K16 echo ("K16 echo"): a feedback delay whose loop is one K11 cascade per chunk.  The delay is at least one K11 chunk, so the
 * delayed input of a chunk lies wholly in the past; the loop's damping filter has at most NAE_ECHO_MAX_SECTIONS K11 sections; |feedback| is at
 * most NAE_ECHO_MAX_FEEDBACK */
#define NAE_ECHO_MIN_DELAY NAE_EQ_CHUNK
#define NAE_ECHO_MAX_DELAY (1 << 20)
#define NAE_ECHO_MAX_SECTIONS 4
#define NAE_ECHO_MAX_FEEDBACK 0.99
/* K17 modulated delay ("K17 modulated delay"): chorus, flanger and vibrato: one short delay d = delay + depth l(n) swept by an
 * LFO l, read between samples by 4-point Lagrange interpolation, with feedback.  delay - depth >= NAE_MOD_MIN_DELAY keeps the newest sample a
 * tap reads behind the one it computes; delay + depth <= NAE_MOD_MAX_DELAY (64 ms at 48 kHz) lets a ring of 4096 floats hold one chunk of
 * NAE_EQ_CHUNK samples and the deepest reach, floor(d) + 2; at most NAE_MOD_MAX_VOICES taps of one LFO at different phases; |feedback| is at
 * most NAE_MOD_MAX_FEEDBACK */
#define NAE_MOD_MIN_DELAY 2.0
#define NAE_MOD_MAX_DELAY 3070.0
#define NAE_MOD_MAX_VOICES 4
#define NAE_MOD_MAX_FEEDBACK 0.95
#define NAE_MOD_SINE 0
#define NAE_MOD_TRIANGLE 1
/* K18 saturation ("K18 saturation"): a static curve run oversampled by M = 1, 2, 4 or NAE_SAT_MAX_OS.  The anti-alias prototype is
 * nae_fir_design's Kaiser low-pass with 2 NAE_SAT_HALF M + 1 taps at cutoff 1 / M: NAE_SAT_HALF taps of the base rate to either side, once up
 * and once down, so the latency is 2 NAE_SAT_HALF samples for every M > 1 */
#define NAE_SAT_HALF 16
#define NAE_SAT_MAX_OS 8
#define NAE_SAT_SOFT 0
#define NAE_SAT_HARD 1
/* K19 gate ("K19 gate"): a noise gate / downward expander on K12's tiling (NAE_DYN_LANE, NAE_DYN_CHUNK), look-ahead limit
 * (NAE_DYN_MAX_LOOKAHEAD) and floor (NAE_DYN_FLOOR_DB); the hold reaches at most NAE_GATE_MAX_HOLD samples */
#define NAE_GATE_MAX_HOLD (1 << 21)
#define NAE_GATE_MIN_THRESHOLD_DB (-90.0)
#define NAE_GATE_MAX_THRESHOLD_DB 0.0
#define NAE_GATE_MAX_SLOPE 99.0
#define NAE_GATE_MAX_RANGE_DB 120.0
/* nae_gate_design: the ranges of its arguments (attack and release are K12's: NAE_DYN_MAX_ATTACK_S, NAE_DYN_MIN_RELEASE_S, NAE_DYN_MAX_RELEASE_S) */
#define NAE_GATE_MAX_HYSTERESIS_DB 24.0
#define NAE_GATE_MAX_RATIO 100.0
#define NAE_GATE_MAX_HOLD_S 10.0
#define NAE_GATE_MODE_GATE 0
#define NAE_GATE_MODE_EXPANDER 1
/* K22 limiter ("K22 limiter"): a true-peak look-ahead brickwall on K12's tiling (NAE_DYN_LANE, NAE_DYN_CHUNK), floor
 * (NAE_DYN_FLOOR_DB) and release range (NAE_DYN_MIN_RELEASE_S, NAE_DYN_MAX_RELEASE_S), with K14's oversampler (NAE_LOUD_TP_PHASES,
 * NAE_LOUD_TP_TAPS) as the detector: its level reaches NAE_LIM_TP_REACH samples to either side of a sample, and the look-ahead with that
 * reach stays within one chunk.  The attack is a moving sum of ceil(y1 NAE_LIM_Q_SCALE) as integers. */
#define NAE_LIM_TP_REACH 6
#define NAE_LIM_MAX_LOOKAHEAD (NAE_DYN_CHUNK - NAE_LIM_TP_REACH)
#define NAE_LIM_Q_SCALE 16777216.0
#define NAE_LIM_MIN_CEILING_DB (-20.0)
#define NAE_LIM_MAX_CEILING_DB 0.0
#define NAE_LIM_MAX_GAIN_DB 24.0
/* K23 dither ("K23 dither"): requantisation to NAE_DITHER_MIN_BITS ... NAE_DITHER_MAX_BITS bits with dither of one of four kinds
 * and an error feedback of at most NAE_DITHER_MAX_TAPS taps whose absolute sum is at most NAE_DITHER_MAX_TAP_SUM. */
#define NAE_DITHER_MIN_BITS 8
#define NAE_DITHER_MAX_BITS 24
#define NAE_DITHER_MAX_TAPS 12
#define NAE_DITHER_MAX_TAP_SUM 64.0
#define NAE_DITHER_NONE 0
#define NAE_DITHER_RECTANGULAR 1
#define NAE_DITHER_TRIANGULAR 2
#define NAE_DITHER_HIGHPASS 3
#define NAE_DITHER_SHAPE_NONE 0
#define NAE_DITHER_SHAPE_FIRST 1
#define NAE_DITHER_SHAPE_SECOND 2
#define NAE_DITHER_SHAPE_LIPSHITZ 3
/* K20 multiband ("K20 multiband"): a Linkwitz-Riley crossover tree of K11 sections into 2 ... NAE_MB_MAX_BANDS bands, K12 on every
 * band, and the bands' sum.  The tree of B bands has 4, 9 or 14 sections in fixed slots: at most NAE_MB_MAX_SECTIONS, inside K11's constant
 * block of NAE_EQ_MAX_SECTIONS */
#define NAE_MB_MAX_BANDS 4
#define NAE_MB_MAX_SECTIONS 14
/* K13 spectral gate ("K13 spectral gate"): noise reduction on the STFT at N = 512 ... 4096 and hop N / 4: a per-bin decision
 * against a learned power profile, smoothed by an integer triangle over at most NAE_DENOISE_MAX_TIME frames and NAE_DENOISE_MAX_FREQ bins to
 * either side (a wider frequency triangle pulls a pure tone down: DESIGN.md gives the figure); a tile the library chooses has at least
 * NAE_DENOISE_MIN_TILE hop blocks (it pays 3 Tn + 3 analyses beyond its own frames) */
#define NAE_DENOISE_MAX_TIME 8
#define NAE_DENOISE_MAX_FREQ 4
#define NAE_DENOISE_MIN_TILE 32
/* nae_denoise_design: the ranges of its arguments */
#define NAE_DENOISE_MAX_REDUCTION_DB 48.0
#define NAE_DENOISE_MIN_SENSITIVITY_DB (-6.0)
#define NAE_DENOISE_MAX_SENSITIVITY_DB 24.0
/* K21 separation ("K21 separation"): harmonic/percussive separation on K13's STFT: the median of the 16-bit keys of the power
 * over at most NAE_HPSS_MAX_SPAN frames to either side against the median over at most NAE_HPSS_MAX_SPAN bins to either side; a tile the
 * library chooses has at least NAE_HPSS_MIN_TILE hop blocks (it pays 2 Tn key analyses and three whole frames beyond its own) */
#define NAE_HPSS_MAX_SPAN 8
#define NAE_HPSS_MIN_TILE 64
/* nae_hpss_design: the range of its two levels; NAE_HPSS_MIN_DB itself is gain 0 */
#define NAE_HPSS_MIN_DB (-120.0)
#define NAE_HPSS_MAX_DB 12.0
/* K14 loudness ("K14 loudness"): the BS.1770-4 meter.  The K-weighting's analog prototypes (nae_loud_design maps them to a
 * sample rate by the bilinear form); sample rates NAE_LOUD_MIN_RATE ... NAE_LOUD_MAX_RATE that are multiples of NAE_LOUD_SUBS_PER_S, so the
 * 100 ms sub-block is a whole number of samples; the cascade is K11's tiling with NAE_LOUD_SECTIONS sections.  The true-peak oversampler:
 * NAE_LOUD_TP_PHASES phases of NAE_LOUD_TP_TAPS taps from one Kaiser-windowed sinc (beta NAE_FIR_KAISER_BETA) of their product taps. */
#define NAE_LOUD_SHELF_F0 1681.974450955533
#define NAE_LOUD_SHELF_GAIN_DB 3.999843853973347
#define NAE_LOUD_SHELF_Q 0.7071752369554196
#define NAE_LOUD_SHELF_VB_EXP 0.4996667741545416
#define NAE_LOUD_HP_F0 38.13547087602444
#define NAE_LOUD_HP_Q 0.5003270373238773
#define NAE_LOUD_SECTIONS 2
#define NAE_LOUD_MIN_RATE 8000
#define NAE_LOUD_MAX_RATE 192000
#define NAE_LOUD_SUBS_PER_S 10
#define NAE_LOUD_BLOCK_SUBS 4
#define NAE_LOUD_ABS_GATE_LUFS (-70.0)
#define NAE_LOUD_OFFSET 0.691
#define NAE_LOUD_REL_GATE 0.1
#define NAE_LOUD_TP_PHASES 4
#define NAE_LOUD_TP_TAPS 12
/* nae_loud_design: the ranges of its arguments */
#define NAE_LOUD_MIN_TARGET_LUFS (-70.0)
#define NAE_LOUD_MAX_TARGET_LUFS (-5.0)
#define NAE_LOUD_MIN_CEILING_DBTP (-20.0)
#define NAE_LOUD_MAX_GAIN_DB 40.0
/* transient preservation ("Transient preservation"): bin k of frame f rises iff P_f[k] > RISE * P_{f-1}[k] and
 * P_f[k] > FLOOR * N; frame f is "high" iff DEN * (rising bins) >= NUM * (N/2 + 1); an onset is an upward crossing of "high" at f >= 2.
 * RISE is +6 dB: at +3 dB steady white noise crosses 3/8 at N = 512 and 1024 (DESIGN.md gives the numbers). */
#define NAE_TRANSIENT_RISE 4.0f
#define NAE_TRANSIENT_FLOOR 0x1p-20f
#define NAE_TRANSIENT_NUM 3
#define NAE_TRANSIENT_DEN 8

/* atan2 -> Q0.32 turns (revision 2 of the K7 / phase specification).  Every step is an IEEE f32 add / mul /
 * fma or a two's-complement integer operation, so C and the GPU give the same 32 bits — and none of them is a division:
 *   ax = |re|, ay = |im|,  mx = max(ax, ay, NAE_ATAN_TINY),  mn = min(ax, ay)
 *   r  = bits_to_float(NAE_RCP_MAGIC - float_to_bits(mx));   three times:  e = fma(-mx, r, 1),  r = fma(r, e, r)
 *   t  = mn * r,  s = t * t,  p = t * Q(s)      Q = Horner with fma over c6 .. c0, coefficients pre-scaled by 2^32:
 *                                               atan(t)/(2 pi) = t * Q(s) / 2^32, degree-6 minimax, max err 5.5e-8 turn
 *   i  = (int32) rint(p)                        first octant, 0 .. 2^29
 *   ay > ax:        i = 0x40000000 - i          (1/4 turn - angle)
 *   sign bit of re: i = 0x80000000 - i          (1/2 turn - angle;  wraps: +1/2 and -1/2 turn are the same phase)
 *   sign bit of im: i = -i
 * The octants follow the SIGN BITS (atan2(+0, -0) is half a turn, as in C); a vanishing bin (mx < 2^-100) has t = 0; a bin
 * with |re| + |im| not below NAE_ATAN_HUGE = 2^100 — which includes NaN, Inf and a sum that overflows — has phase 0 (beyond
 * 1.6e38 the integer seed would wrap; the cut sits where the accuracy guarantee ends).  Accurate for 2^-100 <= mx < 2^100.    */
#define NAE_ATAN_C0 1.591543257e-01f
#define NAE_ATAN_C1 -5.302623659e-02f
#define NAE_ATAN_C2 3.152511641e-02f
#define NAE_ATAN_C3 -2.106151544e-02f
#define NAE_ATAN_C4 1.267249603e-02f
#define NAE_ATAN_C5 -5.348273553e-03f
#define NAE_ATAN_C6 1.084129326e-03f
#define NAE_ATAN_SCALE 4294967296.0f   /* 2^32: multiplying a coefficient by it is exact */
#define NAE_ATAN_TINY 7.888609052e-31f /* 2^-100 */
#define NAE_ATAN_HUGE 1.267650600e+30f /* 2^100  */
#define NAE_RCP_MAGIC 0x7EF311C7u      /* integer seed of 1/x: relative error < 0.13, three Newton steps -> < 1e-7 */

/* 1/sqrt(2) rounded to f32, used by the 8-point butterflies */
#define NAE_SQRT1_2 0.70710678118654752440f

/* phase vocoder fixed-point formats */
#define NAE_HA_FRAC_BITS 24     /* analysis hop Ha = Hs * tempo, Q39.24                      */
#define NAE_R_FRAC_BITS 24      /* synthesis/analysis hop ratio Hs/d_t, Q8.24                 */
#define NAE_TEMPO_MIN (1.0 / 64.0)   /* Ha >= 4 samples  */
#define NAE_TEMPO_MAX 16.0

/* resampler (rate transposer): 16-tap Kaiser-windowed sinc, 128 phases, linear phase interpolation */
#define NAE_RS_TAPS 16
#define NAE_RS_PHASES 128
#define NAE_RS_KAISER_BETA 8.0
#define NAE_RS_CUTOFF 0.94      /* fraction of the narrower Nyquist */
#define NAE_RATE_MIN (1.0 / 16.0)
#define NAE_RATE_MAX 16.0

/* N2 input resampler: libswresample's defaults when only rates / formats / layouts are set (SURVEY.md Appendix B;
 * /root/reference/src/processor/audio-amix.cpp:217-232 never touches the resampler options): polyphase
 * Kaiser-windowed sinc, filter_size 32, phase_shift 10 (at most 1024 phases, nearest phase, no interpolation between phases),
 * kaiser_beta 9, cutoff 0.97, exact_rational on (a ratio out/in whose reduced numerator is <= 1024 uses exactly that many
 * phases: 160 for 44.1 -> 48 kHz, 320 for 22.05 -> 48, 6 for 8 -> 48, 1 for 96 -> 48; others keep 1024).  Restated from public knowledge of FFmpeg 7.1's resample.c — UNPINNED versus FFmpeg. */
#define NAE_SWR_FILTER_SIZE 32
#define NAE_SWR_PHASE_SHIFT 10
#define NAE_SWR_KAISER_BETA 9.0
#define NAE_SWR_CUTOFF 0.97
#define NAE_SWR_MAX_TAPS 512    /* filter_length = ceil(32 / factor): down-conversion by up to ~15x */

/* x86 "integer indefinite" produced by cvttss2si on overflow/NaN: what the reference's
 * truncating float->int32 gain path yields out of range (audio-vol.cpp:98, int32_t case). */
#define NAE_X86_INT_INDEFINITE (-2147483647 - 1)

#endif
