/* nae_gpu.h — C-ABI of the MI355X (gfx950) audio-DSP hot path.
 *
 * Drop-in boundary for the per-node sample transforms of Stehsaer/nodey-audio-editor
 * (reference paths below are relative to /root/reference).  Every entry point replaces one CPU inner loop
 * that today runs inside a `processor::*::process_payload` fiber (include/infra/processor.hpp:108-113);
 * the adapter classes in nodey-audio-editor_amd/host/ call these from the same place.
 *
 * Conventions
 *  - plain C, no exceptions cross the ABI: every function returns NAE_OK (0) or a negative nae_status;
 *    nae_last_error(ctx) gives the text.  The adapter converts non-zero into
 *    infra::Processor::Runtime_error (include/infra/processor.hpp:64-77).
 *  - all sample pointers are DEVICE pointers (hipMalloc / nae_malloc) unless the name ends in _host.
 *    "plane pointer arrays" (const T* const*) are HOST arrays whose elements are device pointers — the
 *    same shape as AVFrame::data (audio-vol.cpp:185-186).
 *  - every call only ENQUEUES work on the context's HIP stream and returns; nae_sync() blocks,
 *    nae_poll() never blocks (a Boost fiber polls it and yields: src/infra/runner.cpp:65-83 runs every node
 *    on ONE OS thread, so a blocking wait would stall the whole graph).
 *  - sample formats use FFmpeg's AVSampleFormat numbering so frame->format passes through unchanged.
 */
#ifndef NAE_GPU_H
#define NAE_GPU_H
#include <stddef.h>
#include <stdint.h>
#include "nae_dsp_spec.h" /* NAE_DYNKEY_MAX_SECTIONS, NAE_ECHO_MAX_SECTIONS and NAE_MOD_MAX_VOICES, the extents of nae_dynkey_params::coef, nae_echo_params::coef and nae_mod_params::voice_phase */

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  2 (round 5): additions since 1 — nae_event_query, nae_ctx_wait_event, nae_debug_graph4_stages, page-locked memory,
 * nae_wsola_*, nae_swr_* — and one CHANGED behaviour: nae_ctx_create of a second device used to return NAE_ERR_UNSUPPORTED behind a
 * process-wide latch; now a context may sit on any device, and an index outside [0, nae_device_count()) is NAE_ERR_INVALID.
 * A caller built against 1 keeps working (nothing was removed or re-typed); a caller that needs the additions checks
 * nae_abi_version() >= 2.
 * 3 (round 6): addition — nae_debug_set (the tuning / A-B switches, formerly 14 environment variables read at context creation).
 *   Later additions within 3 (the version number did not move; a caller probes for them by symbol, e.g. dlsym): nae_spectrum_frames_ex
 *   and nae_spectrum_block_ex_f32 (spectrum sizes 256 ... 4096, any hop); nae_spectrum_create accepts those sizes and hops;
 *   NAE_STRETCH_PHASE_LOCK with nae_stretch_block_ex_f32, nae_stretch_create_ex and nae_debug_pv_tile_phase_ex (identity phase locking of the
 *   vocoder); nae_stretch_plan_make_n, nae_stretch_block_n_f32, nae_debug_pv_tile_phase_n and nae_stretch_create_n (vocoder frame sizes
 *   512 ... 4096); nae_stretch_formant_lifter, nae_stretch_block_formant_f32 and nae_stretch_create_formant (formant-preserving pitch
 *   shift); NAE_STRETCH_TRANSIENTS with the _n and _formant entries (transient preservation), which a caller probes for by its return code:
 *   a library without it answers NAE_ERR_INVALID; nae_stretch_plan_make_shift, nae_stretch_block_formant_shift_f32 and
 *   nae_stretch_create_formant_shift (formant shift independent of the pitch); NAE_STRETCH_LINK_CHANNELS with the _n, _formant and
 *   _formant_shift entries (one onset decision and one phase-lock region map per stereo stream), probed by return code as
 *   NAE_STRETCH_TRANSIENTS is; nae_fir_pick_n_fft, nae_fir_block_f32, nae_fir_design and the nae_fir handle (nae_fir_create, _put, _put_host, _flush,
 *   _available, _receive, _receive_host, _destroy): the FIR filter, K9; nae_conv_pick_n_fft, nae_conv_block_f32, nae_conv_reverb_taps,
 *   nae_conv_design_reverb and the nae_conv handle (the same eight entries): the long convolution, K10; nae_eq_design, nae_eq_block_f32 and
 *   the nae_eq handle (the same eight entries): the biquad cascade, K11; nae_dyn_design, nae_dyn_block_f32 and the nae_dyn handle (the same
 *   eight entries) with the record nae_dyn_params: the dynamics processor, K12; nae_denoise_design, nae_denoise_profile_f32,
 *   nae_denoise_block_f32 and the nae_denoise handle (the same eight entries) with the record nae_denoise_params: the spectral gate, K13;
 *   nae_loud_design, nae_loud_lufs, nae_loud_measure_f32, nae_loud_apply_f32, nae_loud_normalize_f32 and the measuring handle nae_loud
 *   (nae_loud_create, _put, _put_host, _flush, _get_result, _destroy) with the records nae_loud_params and nae_loud_result: the BS.1770
 *   loudness meter and normalizer, K14; nae_dynkey_block_f32 and the nae_dynkey handle (the same eight entries) with the record
 *   nae_dynkey_params: the keyed (side-chain) dynamics, K15; nae_echo_design, nae_echo_block_f32 and the nae_echo handle (the same eight
 *   entries) with the record nae_echo_params: the echo, K16; nae_mod_design, nae_mod_block_f32 and the nae_mod handle (the same eight
 *   entries) with the record nae_mod_params: the modulated delay (chorus, flanger, vibrato), K17; nae_sat_latency, nae_sat_taps,
 *   nae_sat_design, nae_sat_block_f32 and the nae_sat handle (the same eight entries) with the record nae_sat_params: the saturation, K18;
 *   nae_gate_design, nae_gate_block_f32 and the nae_gate handle (the same eight entries) with the record nae_gate_params: the noise gate and
 *   downward expander, K19; nae_mb_design, nae_mb_block_f32 and the nae_mb handle (the same eight entries) with the record nae_mb_params:
 *   the multiband compressor, K20; nae_hpss_design, nae_hpss_block_f32 and the nae_hpss handle (the same eight entries) with the record
 *   nae_hpss_params: the harmonic/percussive separation, K21; nae_lim_design, nae_lim_block_f32 and the nae_lim handle (the same eight
 *   entries) with the record nae_lim_params: the true-peak look-ahead limiter, K22; nae_dither_design, nae_dither_block_f32 and the
 *   nae_dither handle (the same eight entries) with the record nae_dither_params: word-length reduction with dither and noise shaping,
 *   K23. */
#define NAE_ABI_VERSION 3

typedef enum nae_status {
    NAE_OK = 0,
    NAE_ERR_INVALID = -1,     /* bad argument (null pointer, channel count not 1/2 where the reference rejects it, ...) */
    NAE_ERR_UNSUPPORTED = -2, /* sample format / parameter outside the reference's envelope            */
    NAE_ERR_HIP = -3,         /* HIP runtime error; nae_last_error has hipGetErrorString               */
    NAE_ERR_NOMEM = -4,
    NAE_ERR_STATE = -5        /* call order violation on a stateful handle                            */
} nae_status;

/* == AVSampleFormat (libavutil/samplefmt.h) for the formats audio-vol.cpp:188-244 and
 * audio-velocity.cpp:160-229 accept */
typedef enum nae_fmt {
    NAE_FMT_S16 = 1, NAE_FMT_S32 = 2, NAE_FMT_FLT = 3, NAE_FMT_S16P = 6, NAE_FMT_S32P = 7, NAE_FMT_FLTP = 8
} nae_fmt;

typedef struct nae_ctx nae_ctx;
typedef struct nae_event nae_event;
typedef struct nae_stretch nae_stretch;
typedef struct nae_spectrum nae_spectrum;
typedef struct nae_fir nae_fir;
typedef struct nae_conv nae_conv;
typedef struct nae_eq nae_eq;
typedef struct nae_dyn nae_dyn;
typedef struct nae_dynkey nae_dynkey;
typedef struct nae_echo nae_echo;
typedef struct nae_mod nae_mod;
typedef struct nae_sat nae_sat;
typedef struct nae_gate nae_gate;
typedef struct nae_mb nae_mb;
typedef struct nae_denoise nae_denoise;
typedef struct nae_hpss nae_hpss;
typedef struct nae_lim nae_lim;
typedef struct nae_dither nae_dither;
typedef struct nae_loud nae_loud;

/* ------------------------------------------------------------------ context / plumbing */
int nae_abi_version(void);
int nae_device_count(void);
/* Devices.  A process may hold contexts on SEVERAL devices (the reference runs every node of a graph in one process on one
 * thread, src/infra/runner.cpp:65-83,142-154, so the drop-in reaches all GPUs of the node from there): a context remembers
 * its device, and every entry point that takes a context — allocation, launches, copies, memset, event record / wait, nae_sync,
 * nae_poll, nae_free — selects that device for the calling thread when the thread's current HIP device differs, and leaves it
 * selected.  `device` outside [0, nae_device_count()) returns
 * NAE_ERR_INVALID.  Several contexts on one device are fine — each has its own stream, so their work overlaps.
 * (More than one device per process is exercised on one-GPU boxes only, through two contexts on device 0 and the
 * rejection of device 1: N > 1 devices from one process are UNMEASURED on hardware.)
 * Threads.  The library keeps no process-global mutable HOST state.  ONE thread at a time drives a given context and the
 * handles / events created from it; different contexts may be created, driven and destroyed from different threads
 * concurrently.  nae_event_query / nae_poll may be called from the thread that drives the context.
 * One piece of DEVICE-global state exists: `g_cu_arrivals` (csrc/kernels_pvpipe.hip), per-CU arrival counters from which the
 * vocoder pipeline's two workgroups of a CU derive which of them starts with the higher issue priority.  It is shared by all
 * contexts of a device and never reset; two contexts running the pipeline concurrently can hand both workgroups of a CU the
 * same parity — a scheduling hint only: results do not depend on it (tests/test_gpu_multi_ctx.py runs two contexts interleaved
 * bit for bit).  The host mirror's own shared state (context pool, device round-robin) is guarded by a mutex
 * (host/processor/gpu-context.hpp); it keeps every node on ONE device unless $NAE_DEVICES asks for more. */
int nae_ctx_create(int device, nae_ctx** out);
int nae_ctx_destroy(nae_ctx* ctx);
int nae_ctx_set_stream(nae_ctx* ctx, void* hip_stream); /* borrow a hipStream_t (e.g. torch's current stream) */
void* nae_ctx_stream(nae_ctx* ctx);
int nae_sync(nae_ctx* ctx);                             /* hipStreamSynchronize                               */
int nae_poll(nae_ctx* ctx);                             /* 1 = idle, 0 = work pending, <0 = error; never blocks */
const char* nae_last_error(nae_ctx* ctx);
const char* nae_device_name(nae_ctx* ctx);

int nae_malloc(nae_ctx* ctx, size_t bytes, void** dptr);
int nae_free(nae_ctx* ctx, void* dptr);
/* page-locked host memory (hipHostMalloc): copies to and from it are truly asynchronous and run at the full PCIe rate, so
 * uploads, kernels and downloads of consecutive batches can overlap on two contexts / streams */
int nae_malloc_host(nae_ctx* ctx, size_t bytes, void** hptr);
int nae_free_host(nae_ctx* ctx, void* hptr);
int nae_memcpy_h2d(nae_ctx* ctx, void* dst, const void* src_host, size_t bytes); /* async on the ctx stream */
int nae_memcpy_d2h(nae_ctx* ctx, void* dst_host, const void* src, size_t bytes); /* async on the ctx stream */
int nae_memcpy_d2d(nae_ctx* ctx, void* dst, const void* src, size_t bytes);
int nae_memset(nae_ctx* ctx, void* dst, int value, size_t bytes);

int nae_event_create(nae_ctx* ctx, nae_event** ev);
int nae_event_record(nae_ctx* ctx, nae_event* ev);      /* on the ctx stream */
/* 1 = everything enqueued before the last nae_event_record(ev) has completed, 0 = still pending, < 0 = error; never blocks.
 * The wait a node's fiber spins on for ITS OWN batch (include/infra/processor.hpp:108-113 — process_payload of one node — while
 * other nodes' work may still be queued on the same or another context): record behind the batch, poll, yield. */
int nae_event_query(nae_event* ev);
/* makes everything enqueued on ctx's stream AFTER this call wait for the work captured by the last record of `ev`
 * (hipStreamWaitEvent): a device-side dependency between two contexts of the same device, nothing blocks on the host */
int nae_ctx_wait_event(nae_ctx* ctx, nae_event* ev);
int nae_event_elapsed_ms(nae_event* start, nae_event* stop, float* ms); /* synchronises on `stop` */
int nae_event_destroy(nae_event* ev);

/* per-kernel timing: when enabled every kernel launch is bracketed by two hipEvents on the ctx stream.
 * nae_prof_get(index) returns the number of distinct kernels seen; call with index = -1 to get only the count. */
int nae_prof_enable(nae_ctx* ctx, int on);
int nae_prof_reset(nae_ctx* ctx);
int nae_prof_get(nae_ctx* ctx, int index, char* name, size_t name_cap, double* total_ms, uint64_t* launches);

/* shader clock (GHz) the GPU holds at this moment, from s_memtime / s_memrealtime stamps of a 1024-workgroup probe kernel
 * launched on the context's stream: lets a benchmark turn its own kernel times into cycles without assuming a clock. */
int nae_debug_clock_ghz(nae_ctx* ctx, double* ghz);

/* Tuning / A-B switches of one context (tests and measurement tools; the defaults are the product).  Takes effect from the next call on.
 * Unknown key or value out of range: NAE_ERR_INVALID.  Keys (value 0 = the library's own choice unless said otherwise):
 *   pv_tile         frames per phase-vocoder time tile (pass 1 and pass 3);  pv_min_ptile  shortest pass-1 tile the library may choose (default 16)
 *   pv_fps          1 | 2 | 4: frames per step of the vocoder pipeline
 *   pv_flow         0 | 1 | 2: launches of at most one workgroup per CU run the one-barrier schedule never / with one frame per step (default 1) / always
 *   pv_lean         1: the pipeline keeps its 64-VGPR two-workgroups-per-CU build even when one workgroup per CU would allow 128
 *   rs_single, rs_direct, no_mix_fuse      1: transposer with one stream per workgroup / the direct (unstaged) kernel / mix and transposer as two launches
 *   spec_generic, spec_narrow              1: skip the interleaved-stereo spectrum kernel / its dword stores instead of 16-byte ones
 *   spec_chunk, spec_fine, spec_fine_rounds   frames per chunk of the stereo spectrum kernel / of the short chunks at a launch's end / how many of those per wave
 *   spec_any        1: 1024-point spectrum launches (nae_spectrum_block_f32, _ex at 1024 / 256, the graph's spectrum node) run the size-generic
 *                   kernel of the other sizes instead of the 1024-point ones, whatever spec_generic says (same results, bit for bit)
 *   pv_any          1: unlocked 1024-point vocoder launches run the size-generic kernels of the other frame sizes (the same integer phases, bit
 *                   for bit; samples within the tolerance); the tile is pv_tile, else one of at least pv_min_ptile frames (default 64)
 *   td_nc           1 | 2 | 4: candidates per thread of the WSOLA search;  st_unfused  1: filter and cubic stage of the WSOLA chain as two launches
 *   fir_tile        blocks (of n_fft / 2 samples) one wave of the FIR filter walks; every tiling gives the same bits
 *   conv_tile       blocks one wave of the long convolution's accumulate kernel walks (0: the register tile, nae_pick_conv_tile)
 *   conv_ring       spectrum slots per stream-channel of the long convolution's workspace ring (0: from the workspace cap; at least the
 *                   partition count is used); a handle reads it when it is created.  Neither changes a result
 *   dn_tile         hop blocks (of n_fft / 4 samples) one wave of the spectral gate walks (0: nae_pick_denoise_tile); every tiling gives the same bits
 *   hpss_tile       hop blocks (of n_fft / 4 samples) one wave of the separation walks (0: nae_pick_hpss_tile); every tiling gives the same bits
 *   dither_roles    who does the feed-forward work of the dither's error-feedback kernel: 1 the four producer waves of the workgroup, 2 the walking
 *                   wave itself (0: the library's choice, 1); every value gives the same bits
 *   echo_group      streams per launch of nae_echo_block_f32 (0: as many as keep the delay lines inside the 256 MiB workspace cap); every grouping
 *                   gives the same bits
 *   mod_sub         samples one wave of the modulated delay computes in parallel, 1 ... 64 (0: 64 without feedback, else min(64, floor(delay -
 *                   depth) - 1)); a value above that rule's is cut down to it; every value gives the same bits
 *   sat_tile        chunks (of NAE_EQ_CHUNK samples) one wave of the saturation walks (0: nae_pick_sat_tile, which cuts a small batch until the CUs
 *                   are full); every tiling gives the same bits
 *   mb_group        streams per launch group of nae_mb_block_f32 (0: as many as keep the band planes inside the 256 MiB workspace cap)
 *   mb_slab         chunks (of NAE_EQ_CHUNK samples) per slab of the multiband compressor's three kernels (0: as many as the cap then holds; a
 *                   handle reads it when it is created, 0: 64).  Every grouping and every slab gives the same bits
 * The same assignments, comma separated, in the environment variable NAE_DEBUG ("pv_flow=2,pv_fps=4") are applied when a context is created
 * (for measuring a program that creates its contexts itself, e.g. bench.py); an unknown key there fails nae_ctx_create with NAE_ERR_INVALID. */
int nae_debug_set(nae_ctx* ctx, const char* key, long long value);

/* test utility: adds the number of differing 32-bit words of two device buffers to the device counter *d_count (zero it
 * first with nae_memset); asynchronous on the context's stream. */
int nae_debug_diff_u32(nae_ctx* ctx, const void* a, const void* b, size_t n_words, uint64_t* d_count);

/* synthetic input: dst[s*stream_stride + i] = uniform[-1,1) from splitmix64 with
 * seed(s) = 0x9E3779B97F4A7C15*(1 + first_stream + s) + input_index, i < n_per_stream.  Benchmark/test utility. */
int nae_fill_uniform_f32(nae_ctx* ctx, float* dst, size_t n_per_stream, size_t stream_stride, size_t n_streams,
                         uint64_t first_stream, uint64_t input_index);

/* ------------------------------------------------------------------ batched signal view
 * element (stream s, channel c, sample-frame i) lives at base[s*stream_stride + c*chan_stride + i*frame_stride]
 * (strides in ELEMENTS).  interleaved [S][ch]: chan_stride 1, frame_stride ch;  planar [ch][S]: chan_stride S,
 * frame_stride 1.  stream_stride 0 = every stream reads the same buffer (a shared source). */
typedef struct nae_sig {
    void* base;
    size_t stream_stride;
    size_t chan_stride;
    size_t frame_stride;
} nae_sig;

/* ------------------------------------------------------------------ K1 gain
 * replaces change_volume<T>, src/processor/audio-vol.cpp:75-100 (dispatch :188-244).
 * dst[p][i] = T(float(src[p][i]) * volume); f32: one IEEE multiply; s16/s32: truncation toward zero,
 * no clamp, x86 out-of-range result (0x80000000, then modular narrowing for s16).  src == dst allowed. */
int nae_gain_f32(nae_ctx* ctx, const float* const* src_planes, float* const* dst_planes, int planes,
                 size_t elems, float volume);
int nae_gain_s16(nae_ctx* ctx, const int16_t* const* src_planes, int16_t* const* dst_planes, int planes,
                 size_t elems, float volume);
int nae_gain_s32(nae_ctx* ctx, const int32_t* const* src_planes, int32_t* const* dst_planes, int planes,
                 size_t elems, float volume);
/* whole-frame entry mirroring the format switch at audio-vol.cpp:184-244: `planes` has 1 pointer for packed
 * formats and `ch` pointers for planar ones; ch must be 1 or 2 (:177-182) */
int nae_gain_frame(nae_ctx* ctx, int fmt, const void* const* src_planes, void* const* dst_planes, size_t S,
                   int ch, float volume);

/* ------------------------------------------------------------------ K2 split / merge
 * deinterleave replaces swr_convert FLT->FLTP at equal rate/layout (audio-amix.cpp:263-269,
 * audio-bimix.cpp:259-265); interleave replaces audio-velocity.cpp:169-180. Bit copies. */
int nae_deinterleave_f32(nae_ctx* ctx, const float* src, float* const* dst_planes, size_t S, int ch);
int nae_interleave_f32(nae_ctx* ctx, const float* const* src_planes, float* dst, size_t S, int ch);
/* batched: n_streams x ch x S through nae_sig views (configs[1]: 1000 buffers of 4096) */
int nae_copy_sig_f32(nae_ctx* ctx, const nae_sig* src, const nae_sig* dst, size_t S, int ch, size_t n_streams);
/* fused split -> gain -> merge on interleaved stereo (the three nodes of configs[1] in one pass) */
int nae_gain_sig_f32(nae_ctx* ctx, const nae_sig* src, const nae_sig* dst, size_t S, int ch, size_t n_streams,
                     float volume);

/* ------------------------------------------------------------------ K3 N-input mix
 * replaces the loop at audio-amix.cpp:293-307: L[j] = (((0 + a0L[j]*v0) + a1L[j]*v1) + ...), same for R;
 * multiply and add are never fused.  1 <= n <= 16 (audio-amix.cpp:342). */
int nae_amix_f32(nae_ctx* ctx, const float* const* inL, const float* const* inR, const float* vol_host, int n,
                 float* outL, float* outR, size_t S);
/* batched over streams; inputs may be interleaved (the node's swr FLT->FLTP step is folded in) or planar */
int nae_amix_sig_f32(nae_ctx* ctx, const nae_sig* inputs, const float* vol_host, int n, const nae_sig* out,
                     size_t S, size_t n_streams);

/* ------------------------------------------------------------------ K4 channel mix v1
 * replaces audio-bimix.cpp:310-317: outL = (ll/2 + lr/2)*(1-bias), outR = (rl/2 + rr/2)*(1+bias) */
int nae_bimix_f32(nae_ctx* ctx, const float* ll, const float* lr, const float* rl, const float* rr, float bias,
                  float* outL, float* outR, size_t S);

/* ------------------------------------------------------------------ K5 channel mix v2
 * downmix replaces audio-bimix.cpp:624-627,717-720 (mono = (l+r)*0.5); interleave replaces :797-803,
 * :833-850 and the single-sided tails :736-742,:759-765 (later == NULL, aligned == 0). */
int nae_bimix2_downmix_f32(nae_ctx* ctx, const float* l, const float* r, float* mono, size_t S);
int nae_bimix2_interleave_f32(nae_ctx* ctx, float* dst, const float* earlier, const float* later,
                              size_t unaligned, size_t aligned, int earlier_offset);

/* ------------------------------------------------------------------ K6 any format -> interleaved f32
 * replaces extract_samples_interleaved, audio-velocity.cpp:150-232 (divisors 32768.0f / 32767 /
 * 2147483648.0f / (double)2147483647 kept literally).  NAE_ERR_UNSUPPORTED where the reference throws. */
int nae_to_f32_interleaved(nae_ctx* ctx, int fmt, const void* const* planes, size_t S, int ch, float* dst);

/* sink-side clamp, audio-io.cpp:617-618 */
int nae_clamp_f32(nae_ctx* ctx, float* data, size_t n);

/* ------------------------------------------------------------------ K7 tempo / pitch
 * replaces the SoundTouch object driven by soundtouch_process_payload, audio-velocity.cpp:265-443
 * (setSampleRate/setChannels/setRate/setPitch :381-385, putSamples :403, numSamples :399,414,419,
 * receiveSamples :298, flush :427).  Algorithm: phase vocoder (N=1024, hop 256) + windowed-sinc rate
 * transposer, DESIGN.md §3 — NOT SoundTouch's WSOLA; parity vs SoundTouch is unpinned.
 * Velocity_modifier passes (rate = velocity, pitch = keep_pitch ? 1/velocity : 1) (:445-460);
 * Pitch_modifier passes (rate = 1, pitch = 2^(semitones/12)) (:462-477). */
typedef struct nae_stretch_plan {
    int pv_on, rs_on;
    double tempo_eff, rate_eff;
    int64_t ha_q24;
    int32_t d0;
    uint32_t r_q24[2];
    uint64_t step_q32;
    size_t out_len, mid_len, frames;
    int rs_first;             /* both stages on and rate_eff > 1: the transposer runs FIRST (fewer samples reach the
                                 vocoder; SoundTouch orders its stages by the same rule) and mid_len is ITS output */
} nae_stretch_plan;
int nae_stretch_plan_make(double rate, double pitch, size_t in_len, nae_stretch_plan* plan);

/* block form: n_streams independent signals of in_len sample-frames each; dst receives plan.out_len frames.
 * Workspace is owned by the context and grown on demand (never freed between calls). */
int nae_stretch_block_f32(nae_ctx* ctx, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                          size_t n_streams, const nae_sig* dst);
/* debugging tap used by the parity tests: synthesis phase (Q0.32) in front of every PV tile,
 * dst_host[n_streams][ch][n_tiles][513] int32; returns n_tiles through *n_tiles and the tile length in frames */
int nae_debug_pv_tile_phase(nae_ctx* ctx, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                            size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles,
                            size_t* tile_frames);

/* Options of the _ex entries (flags; an unknown bit returns NAE_ERR_INVALID, flags == 0 is exactly the call without _ex).
 * NAE_STRETCH_PHASE_LOCK: identity phase locking (Laroche & Dolson 1999; DESIGN.md §3, "Phase locking").  Frame f >= 1 advances only the
 * phase of each spectral peak of the power spectrum and keeps every other bin at its analysis phase offset from its nearest peak:
 * Qs_f[k] = Qs_{f-1}[p] + inc_f[p] + (Qa_f[k] - Qa_f[p]), p = the peak of bin k (a frame without a peak runs unlocked).  A steady tone keeps its
 * amplitude (the unlocked vocoder loses 2-16 % on an off-centre tone).  Everything else — analysis, transposer, stage order, lengths — is the
 * unlocked node's.  Integer phases are bit-exact against the CPU statement (tests/pv_ref/ref_pv.c) and independent of the tiling. */
#define NAE_STRETCH_PHASE_LOCK 1u
int nae_stretch_block_ex_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, const nae_sig* src, size_t in_len, int ch,
                             size_t n_streams, const nae_sig* dst);
/* the phase tap of the vocoder selected by `flags` (locked: Qs in front of every tile of the locked recurrence) */
int nae_debug_pv_tile_phase_ex(nae_ctx* ctx, double rate, double pitch, unsigned flags, const nae_sig* src, size_t in_len, int ch,
                               size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles, size_t* tile_frames);

/* SoundTouch-shaped streaming handle (interleaved f32, device pointers) */
int nae_stretch_create(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, nae_stretch** h);
/* the same with the flags of nae_stretch_block_ex_f32; the handle's output equals the block call's with those flags */
int nae_stretch_create_ex(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, nae_stretch** h);

/* Vocoder frame size n_fft = 512, 1024, 2048 or 4096: analysis and synthesis frames of n_fft samples, synthesis hop n_fft / 4,
 * Hann / Hann, gain 2/3.  A longer frame resolves low partials (bins of 48000 / n_fft Hz), a shorter one smears transients less.  The plan's hop,
 * phase-advance ratios and frame count follow the size; out_len, mid_len, the stage order, the transposer and the rate / tempo limits do not.
 * n_fft = 1024 is exactly the call without _n (nae_stretch_plan_make, the _ex entries).  Another size: NAE_ERR_UNSUPPORTED, and so is
 * NAE_STRETCH_PHASE_LOCK at a size other than 1024; an unknown flag bit: NAE_ERR_INVALID.  Integer phases are bit-exact against the CPU
 * statement (tests/pv_ref/ref_pv.c) and independent of the tiling; a handle's output equals the block call's. */
int nae_stretch_plan_make_n(double rate, double pitch, int n_fft, size_t in_len, nae_stretch_plan* plan);
int nae_stretch_block_n_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, const nae_sig* src, size_t in_len, int ch,
                            size_t n_streams, const nae_sig* dst);
/* dst_host[n_streams][ch][n_tiles][n_fft/2 + 1] */
int nae_debug_pv_tile_phase_n(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, const nae_sig* src, size_t in_len, int ch,
                              size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles, size_t* tile_frames);
int nae_stretch_create_n(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, int n_fft, nae_stretch** h);

/* Formant preservation ("Formant preservation"): when the node runs both the vocoder and the transposer (a pitch change), each
 * synthesis frame's magnitudes are multiplied by G[k] = min(E(k rho) / E(k), NAE_FORMANT_MAX_GAIN), where E is the frame's cepstral envelope
 * (the log2 spectrum liftered to quefrencies below `lifter` samples) and rho = plan.rate_eff, so the output keeps the input's spectral
 * envelope while its harmonics move.  Phases, lengths, stage order and the transposer are the _n call's; so are flags and n_fft
 * (NAE_STRETCH_PHASE_LOCK at 1024).  lifter == 0 is exactly the _n call; lifter < 0 or > n_fft / 4: NAE_ERR_INVALID.  Without a pitch change
 * (no transposer, or no vocoder) a lifter changes nothing.  Samples follow the tolerance path against tests/pv_ref/ref_pv.c;
 * the result is independent of the tiling, and a handle's output equals the block call's.
 * nae_stretch_formant_lifter: the default lifter, min(max(sample_rate / 700, 1), n_fft / 4) (68 at 48 kHz, 63 at 44.1 kHz, n_fft 1024); 0 for
 * an unsupported n_fft or a sample_rate <= 0. */
int nae_stretch_formant_lifter(int sample_rate, int n_fft);
int nae_stretch_block_formant_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, int lifter,
                                  const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
int nae_stretch_create_formant(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags,
                               int n_fft, int lifter, nae_stretch** h);

/* Formant shift ("Formant shift"): the output's spectral envelope is the input's scaled in frequency by formant_ratio (phi > 0),
 * E_out(f) = E_in(f / phi), with or without a pitch change; phi = 1 is formant preservation.  The gain rule is the _formant entries' with the
 * ratio g = (float)(plan.rate_eff / phi).  The envelope stage runs when lifter > 0 and |plan.rate_eff / phi - 1| >= 1e-6; otherwise the call is
 * the _n call with the same flags, bit for bit (lifter == 0 is exactly the _n call, whatever the valid phi).  Four cases:
 *   A  a pitch change (vocoder and transposer): the formant pass with the new g, locked or not;
 *   B  a tempo change only (rate_eff = 1, e.g. rate = 1 / pitch): the same pass with g = 1 / phi;
 *   C  a rate change only (pitch = 1): the vocoder stage is forced on at tempo 1 and runs with the transposer in the usual order (transposer
 *      first when rate_eff > 1);
 *   D  neither (rate pitch = 1, pitch = 1): the forced stage alone, out_len = in_len.
 * The forced stage is an STFT pass — analysis, Y = G X, c2r, Hann, overlap-add, gain 2/3; the synthesis phase equals the analysis phase in every
 * frame, so NAE_STRETCH_PHASE_LOCK (1024) and NAE_STRETCH_TRANSIENTS are accepted and change nothing there.  nae_stretch_plan_make_shift is the
 * plan: nae_stretch_plan_make_n's, and in cases C and D with the stage on pv_on = 1, tempo_eff = 1, ha_q24 = (n_fft / 4) << 24,
 * d0 = n_fft / 4, r_q24[0] = 2^24 and the frame count of the usual formula; out_len, mid_len, rs_first and the transposer are unchanged.
 * With phi = 1 cases A, B and D give the _formant call's bits.  Case C differs: the _formant entries do nothing without a pitch change, so
 * there they are a plain resampling (the formants move with the rate), while this entry with phi = 1 runs the envelope stage and keeps the
 * formants in place.  Flags, n_fft and lifter follow the _formant entries' rules.  phi not finite or <= 0: NAE_ERR_INVALID; outside
 * [NAE_FORMANT_SHIFT_MIN, NAE_FORMANT_SHIFT_MAX] = [0.25, 4] (+-24 semitones): NAE_ERR_UNSUPPORTED; phi is checked whatever the lifter.  The
 * cap NAE_FORMANT_MAX_GAIN stays.  Samples follow the tolerance path against tests/pv_ref/ref_pv.c; the result is independent of the
 * tiling, and a handle's output equals the block call's. */
int nae_stretch_plan_make_shift(double rate, double pitch, double formant_ratio, int lifter, int n_fft, size_t in_len, nae_stretch_plan* plan);
int nae_stretch_block_formant_shift_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, int lifter, double formant_ratio,
                                        const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
int nae_stretch_create_formant_shift(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, int n_fft, int lifter,
                                     double formant_ratio, nae_stretch** h);

/* NAE_STRETCH_TRANSIENTS: transient preservation ("Transient preservation"), a flag of the _n and _formant entries
 * (nae_stretch_block_n_f32, nae_stretch_create_n, nae_debug_pv_tile_phase_n, nae_stretch_block_formant_f32, nae_stretch_create_formant) at
 * every n_fft.  Frame f >= 2 is an onset when the number of bins whose power rises more than NAE_TRANSIENT_RISE times (+6 dB) over frame
 * f - 1 crosses NAE_TRANSIENT_NUM / NAE_TRANSIENT_DEN of the bins upwards; an onset frame takes its analysis phase as its synthesis phase, so an
 * attack keeps its shape instead of spreading over the frame.  Other frames, magnitudes, lengths and the transposer are unchanged; a signal
 * without onsets gives the unflagged call's bits.  It combines with NAE_STRETCH_PHASE_LOCK at 1024 (the locked maps reset too; the lock
 * at another size stays NAE_ERR_UNSUPPORTED); the _ex entries answer NAE_ERR_INVALID.  Without the vocoder stage (no tempo change) the flag
 * changes nothing.  Integer phases are bit-exact against the CPU
 * statement (tests/pv_ref/ref_pv.c) and independent of the tiling; a handle's output equals the block call's. */
#define NAE_STRETCH_TRANSIENTS 4u
/* NAE_STRETCH_LINK_CHANNELS: channel link ("Channel link"), a flag of the _n, _formant and _formant_shift entries (block, create
 * and nae_debug_pv_tile_phase_n).  On a stereo stream the onset rule of NAE_STRETCH_TRANSIENTS and the peaks and regions of
 * NAE_STRETCH_PHASE_LOCK read the linked power Pl[k] = 0.5f (P0[k] + P1[k]) of the two channels in place of each channel's own, so both
 * channels reset at the same frames and lock to the same bins; each channel keeps its own analysis phase, increments, magnitudes and
 * synthesis phase.  The link is effective with ch == 2, the vocoder stage on and not forced, and the lock or transient preservation
 * effective; in every other case (mono, neither option, a forced stage, no vocoder stage) the call gives the bits of the call without
 * the flag.  With the lock at a size other than 1024 the call stays NAE_ERR_UNSUPPORTED; the _ex entries answer NAE_ERR_INVALID; bits 2
 * and 8 stay unknown flags.  Integer phases are bit-exact against the CPU statement (tests/pv_ref/ref_pv.c) and independent of the
 * tiling; a handle's output equals the block call's. */
#define NAE_STRETCH_LINK_CHANNELS 16u
int nae_stretch_put(nae_stretch* h, const float* interleaved, size_t S);
int nae_stretch_put_host(nae_stretch* h, const float* interleaved_host, size_t S);
int nae_stretch_flush(nae_stretch* h);
size_t nae_stretch_available(nae_stretch* h);                          /* == SoundTouch::numSamples()    */
int nae_stretch_receive(nae_stretch* h, float* dst, size_t max_frames, size_t* got);
int nae_stretch_receive_host(nae_stretch* h, float* dst_host, size_t max_frames, size_t* got);
int nae_stretch_destroy(nae_stretch* h);

/* ------------------------------------------------------------------ K7 option A (N1): SoundTouch-shaped time-domain chain
 * The same call sites as above (audio-velocity.cpp:369-385 create + setSampleRate/setChannels/setRate/setPitch,
 * :403 putSamples, :399 numSamples, :298 receiveSamples, :427 flush), with SoundTouch 2.3.2's own algorithm instead
 * of the phase vocoder: WSOLA stretcher (8 ms overlap, automatic 40-90 ms sequence / 15-20 ms seek window,
 * exhaustive normalised cross-correlation search), 64-tap anti-alias FIR and 4-point cubic transposer, in the
 * library's stage order (stretcher first for rate > 1, transposer first otherwise) and with its flush rule
 * (zero blocks of 128 frames until round(in / rate) frames exist, at most 200 of them).  The library is not in the
 * reference tree, so the algorithm is restated and parity versus SoundTouch itself is UNPINNED;
 * the GPU result is bit-exact versus oracle/orc_wsola.c.  `rate`, `pitch` as for nae_stretch_create. */
typedef struct nae_wsola nae_wsola;
typedef struct nae_wsola_plan {
    int sample_rate, channels;
    double rate_eff, tempo_eff;      /* rate*pitch, 1/pitch */
    int order;                       /* 0: stretcher, filter, transposer (rate_eff > 1)   1: filter, transposer,
                                        stretcher (== 1)   2: transposer, filter, stretcher (< 1) */
    int overlap_len, seq_len, seek_len, sample_req;
    double nominal_skip;
    size_t in_len, flush_zeros;      /* zeros the flush rule appends */
    size_t n_seq;                    /* WSOLA sequences */
    size_t td_out_len, aa_out_len, cu_out_len;
    size_t out_len;                  /* frames delivered for in_len frames of input */
} nae_wsola_plan;
int nae_wsola_plan_make(int sample_rate, int channels, double rate, double pitch, size_t in_len, nae_wsola_plan* plan);
/* block form: n_streams independent signals of in_len frames; dst receives plan.out_len frames per stream (one put,
 * flush, receive-all).  offsets_dbg (device, optional): [n_streams][n_seq - 1] chosen overlap offsets. */
int nae_wsola_block_f32(nae_ctx* ctx, int sample_rate, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                        size_t n_streams, const nae_sig* dst, int32_t* offsets_dbg);
/* streaming form: the calls and the argument rule of the other handles.  A null handle, a null `got`, or a null pointer with a non-zero
 * count: NAE_ERR_INVALID whatever the handle's state; a put after the flush: NAE_ERR_STATE.  What comes out follows the put sequence (every
 * put runs the chain on what has arrived, and the flush counts from the frames received so far), as SoundTouch's does. */
int nae_wsola_create(nae_ctx* ctx, int sample_rate, int channels, double rate, double pitch, nae_wsola** h);
int nae_wsola_put(nae_wsola* h, const float* interleaved, size_t S);
int nae_wsola_put_host(nae_wsola* h, const float* interleaved_host, size_t S);
int nae_wsola_flush(nae_wsola* h);
size_t nae_wsola_available(const nae_wsola* h);
int nae_wsola_receive(nae_wsola* h, float* dst, size_t max_frames, size_t* got);
int nae_wsola_receive_host(nae_wsola* h, float* dst_host, size_t max_frames, size_t* got);
int nae_wsola_destroy(nae_wsola* h);

/* ------------------------------------------------------------------ N2 input conversion (libswresample's role)
 * replaces the SwrContext every mixer input runs through (audio-amix.cpp:212-240,263-282; audio-bimix.cpp:198-240,
 * 259-294; utility/sw-resample.hpp:55-70): any supported format / mono|stereo / rate -> `out_rate` stereo f32.
 * Identity inputs (same rate, stereo float) are a bit copy — the only case the reference pins.  Everything else restates
 * libswresample's defaults and is UNPINNED versus FFmpeg itself: sample scaling as K6, mono -> stereo as L = R = m/sqrt(2)
 * (swr's default float rematrix), rate change by swr's default polyphase resampler (filter_size 32, at most 1024 phases — exact_rational: 160 for 44.1 -> 48 kHz —, nearest
 * phase, Kaiser beta 9, cutoff 0.97, reflected ends; include/nae_dsp_spec.h, oracle/orc_swr.c).  Ratios beyond ~15x down
 * are refused with NAE_ERR_UNSUPPORTED.
 * convert() follows swr_convert(ctx, out, out_count, in, in_count): it consumes all n_in input frames, hands out at
 * most max_out frames and keeps the rest buffered; planes == NULL drains (the flush idiom at audio-amix.cpp:281-282). */
typedef struct nae_swr nae_swr;
int nae_swr_create(nae_ctx* ctx, int in_fmt, int in_rate, int in_channels, int out_rate, nae_swr** h);
int nae_swr_convert_host(nae_swr* h, const void* const* planes_host, size_t n_in, float* outL_host, float* outR_host,
                         size_t max_out, size_t* n_out);
/* The same with DEVICE output planes and nothing waited for: the upload, the conversion and the two planes are queued on
 * the context's stream and *n_out (known from frame counts alone) is returned at once.  The caller keeps planes_host alive
 * until it has waited for the stream (nae_sync / nae_poll).  For hosts that queue several frames — or several inputs of a
 * mixer — behind one wait; results are those of nae_swr_convert_host. */
int nae_swr_convert(nae_swr* h, const void* const* planes_host, size_t n_in, float* outL_dev, float* outR_dev,
                    size_t max_out, size_t* n_out);
size_t nae_swr_buffered(nae_swr* h);   /* output frames ready without more input */
int nae_swr_destroy(nae_swr* h);
/* mono -> interleaved stereo with gain (the rematrix step above), device pointers */
int nae_mono_to_stereo_f32(nae_ctx* ctx, const float* mono, float* dst_interleaved, size_t S, float gain);

/* ------------------------------------------------------------------ K8 FFT spectrum
 * no reference code (FFTW declared at xmake.lua:15,33, never called).  Spec: per channel, periodic-Hann
 * windowed 1024-point forward r2c DFT every 256 sample-frames, un-normalised (FFTW convention),
 * |X[k]| for k = 0..512.  frames = T < 1024 ? 0 : (T-1024)/256 + 1.
 * dst element (s, frame f, channel c, bin k) at dst_base[s*dst_stream_stride + (f*ch + c)*513 + k]. */
size_t nae_spectrum_frames(size_t T);
int nae_spectrum_block_f32(nae_ctx* ctx, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                           size_t dst_stream_stride);
/* Any size: n_fft a power of two in [256, 4096] (else NAE_ERR_UNSUPPORTED), 1 <= hop <= n_fft (else NAE_ERR_INVALID).  Frame f starts at
 * f*hop; frames = T < n_fft ? 0 : (T-n_fft)/hop + 1; per channel periodic Hann_N, un-normalised r2c DFT, |X[k]| for k = 0..n_fft/2
 * (canonical FFT of DESIGN.md §3: bit-exact against its CPU restatement, and at 1024 the bits of nae_spectrum_block_f32).
 * dst element (s, frame f, channel c, bin k) at dst_base[s*dst_stream_stride + (f*ch + c)*(n_fft/2 + 1) + k].
 * nae_spectrum_frames_ex returns 0 for parameters that are not supported.  nae_spectrum_block_f32 and nae_spectrum_frames are
 * these calls at 1024 / 256. */
size_t nae_spectrum_frames_ex(size_t T, int n_fft, int hop);
int nae_spectrum_block_ex_f32(nae_ctx* ctx, int n_fft, int hop, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                              size_t dst_stream_stride);
/* streaming handle: put interleaved samples, receive whole frames [ch][n_fft/2 + 1]; the sizes and hops of _ex */
int nae_spectrum_create(nae_ctx* ctx, int n_fft, int hop, int channels, nae_spectrum** h);
int nae_spectrum_put(nae_spectrum* h, const float* interleaved, size_t S);
size_t nae_spectrum_available(nae_spectrum* h);                         /* whole frames ready */
int nae_spectrum_receive(nae_spectrum* h, float* dst, size_t max_frames, size_t* got);
int nae_spectrum_destroy(nae_spectrum* h);

/* ------------------------------------------------------------------ K9 FIR filter
 * no reference code (the reference has no filter node).  Spec ("K9 FIR filter"): taps h[0 ... L-1] in f32, one set for every stream
 * and channel of a call; the result is the causal convolution y[n] = sum_{j < L} h[j] x[n - j], 0 <= n < in_len, x[n] = 0 for n < 0, computed by
 * overlap-save at frame size N = n_fft = 512, 1024, 2048 or 4096 with M = B = N / 2 and 1 <= L <= B + 1, every step an IEEE operation in a fixed
 * order:
 *   1  H = r2c_N(h zero-padded to N), the canonical r2c without a window, bins 0 ... M — on the device, once per call or handle;
 *   2  block b = 0 ... ceil(in_len / B) - 1 reads u[n] = x[b B - B + n], n < N (zero outside [0, in_len)); U = r2c_N(u), no window;
 *   3  Y[k] = (U.x H.x - U.y H.y, U.x H.y + U.y H.x): four products, one subtract, one add, no FMA;
 *   4  v = c2r_N(Y), the canonical c2r (split with T_N, conjugate, forward FFT_M, scale 1 / M; the imaginary parts of bins 0 and M dropped);
 *   5  y[b B + n] = v[B + n], n < B, wherever b B + n < in_len.
 * Bit-exact against the CPU statement (tests/fir_ref/ref_fir.c) and independent of the tiling.  A non-finite input sample changes only the
 * blocks whose u contains it.  The bits depend on N, so N is part of the call: n_fft = 0 means nae_fir_pick_n_fft(n_taps), the smallest
 * supported N with N / 2 + 1 >= n_taps (0 when there is none, or n_taps < 1).
 * Errors: a null pointer, n_taps < 1 or ch not 1 or 2: NAE_ERR_INVALID; an unsupported n_fft, or n_taps > n_fft / 2 + 1: NAE_ERR_UNSUPPORTED;
 * in_len = 0 or n_streams = 0: NAE_OK, nothing is launched.  src and dst are interleaved or planar views (src->stream_stride may be 0); dst
 * receives in_len frames.  The context keeps the taps and H of its last block call: a call with the same taps and size computes neither again. */
int nae_fir_pick_n_fft(int n_taps);
int nae_fir_block_f32(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                      const nae_sig* dst);
/* SoundTouch-shaped streaming handle (interleaved f32, device pointers), parameters and errors as the block call's.  The first in_len frames it
 * delivers equal the block call's bit for bit, however the input is cut into puts (whole blocks come out as they fill).  nae_fir_flush appends
 * n_taps - 1 zero frames, so the tail of the convolution comes out too: in_len + n_taps - 1 frames in all, the block call on the input
 * extended by those zeros.  A put after the flush: NAE_ERR_STATE. */
int nae_fir_create(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, int channels, nae_fir** h);
int nae_fir_put(nae_fir* h, const float* interleaved, size_t S);
int nae_fir_put_host(nae_fir* h, const float* interleaved_host, size_t S);
int nae_fir_flush(nae_fir* h);
size_t nae_fir_available(nae_fir* h);
int nae_fir_receive(nae_fir* h, float* dst, size_t max_frames, size_t* got);
int nae_fir_receive_host(nae_fir* h, float* dst_host, size_t max_frames, size_t* got);
int nae_fir_destroy(nae_fir* h);
/* Linear-phase (type I) designs on the host, in double, rounded once to f32: n_taps = L odd, Kaiser window beta = 8 (the transposer's),
 *   lp(fc)[n] = s[n] / sum s,  s[n] = c sinc(pi c t) w[n],  c = 2 fc / sample_rate,  t = n - (L - 1) / 2,  sinc(0) = 1,
 *   w[n] = I0(beta sqrt(1 - a^2)) / I0(beta),  a = t / ((L - 1) / 2)  (L = 1: w = 1),
 * kind 0 low-pass lp(f_hi); 1 high-pass delta[(L - 1) / 2] - lp(f_lo); 2 band-pass lp(f_hi) - lp(f_lo); 3 band-stop delta - (lp(f_hi) - lp(f_lo)).
 * The frequencies a kind uses lie in (0, sample_rate / 2), f_lo < f_hi for kinds 2 and 3; the other one is ignored.  Anything else — another
 * kind, an even or non-positive n_taps, sample_rate <= 0, a null pointer — is NAE_ERR_INVALID.  No context, no device work. */
int nae_fir_design(int kind, int sample_rate, double f_lo, double f_hi, int n_taps, float* taps_host);

/* ------------------------------------------------------------------ K10 long convolution
 * no reference code.  Spec ("K10 long convolution"): taps h_c[0 ... L-1] in f32, 1 <= L <= NAE_CONV_MAX_TAPS, laid out
 * [taps_ch][L] on the host: taps_ch = 1, one set for every channel, or taps_ch = ch, one per channel; one set (or pair) for every stream.  The
 * result is the causal convolution y[n] = sum_{j < L} h_c[j] x[n - j], 0 <= n < in_len, x = 0 before the signal, by uniformly partitioned
 * overlap-save at N = n_fft = 512 ... 4096, M = B = N / 2, P = ceil(L / B) <= NAE_CONV_MAX_PARTS partitions, every step an IEEE operation in a
 * fixed order:
 *   1  H_{c,p} = r2c_N(h_c[p B ... p B + B - 1] zero-padded to N), p < P (on the device, K9's routine);
 *   2  U_b = r2c_N(u_b), u_b[n] = x[b B - B + n] (K9 step 2);
 *   3  Y_b[k] = sum_{p = 0}^{min(b, P-1)} U_{b-p}[k] H_{c,p}[k], every product in K9's form, summed in increasing p from the p = 0 product by
 *      one add per component and term;
 *   4  v = c2r_N(Y_b);   5  y[b B + n] = v[B + n], n < B, wherever b B + n < in_len (K9 steps 4 and 5).
 * Bit-exact against the CPU statement (tests/conv_ref/ref_conv.c), independent of every tiling, slab and ring size; with L <= B the bits of
 * nae_fir_block_f32 at the same N.  A non-finite input sample i changes only blocks floor(i / B) ... floor(i / B) + P.  n_fft = 0 means
 * nae_conv_pick_n_fft(n_taps): the smallest N with at most 16 partitions, else 4096; 0 when n_taps < 1, > NAE_CONV_MAX_TAPS or P > NAE_CONV_MAX_PARTS.
 * Errors: a null pointer, n_taps < 1, ch not 1 or 2, taps_ch not 1 or ch: NAE_ERR_INVALID; more than NAE_CONV_MAX_TAPS taps, an unsupported
 * n_fft or more than NAE_CONV_MAX_PARTS partitions: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after the checks.  Views as K9's.
 * The context keeps the taps and H of its last block call, apart from the FIR filter's. */
int nae_conv_pick_n_fft(int n_taps);
int nae_conv_block_f32(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, const nae_sig* src, size_t in_len, int ch,
                       size_t n_streams, const nae_sig* dst);
/* Streaming handle, nae_fir's in every respect (channels = ch): the first in_len frames equal the block call's however the input is cut;
 * nae_conv_flush appends n_taps - 1 zero frames, so in_len + n_taps - 1 frames come out.  A put after the flush: NAE_ERR_STATE. */
int nae_conv_create(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, int channels, nae_conv** h);
int nae_conv_put(nae_conv* h, const float* interleaved, size_t S);
int nae_conv_put_host(nae_conv* h, const float* interleaved_host, size_t S);
int nae_conv_flush(nae_conv* h);
size_t nae_conv_available(nae_conv* h);
int nae_conv_receive(nae_conv* h, float* dst, size_t max_frames, size_t* got);
int nae_conv_receive_host(nae_conv* h, float* dst_host, size_t max_frames, size_t* got);
int nae_conv_destroy(nae_conv* h);
/* A synthetic room response on the host, in double, rounded once to f32: d = round(predelay_s sample_rate) silent taps, then noise
 * g[n] = 2 u - 1, u = (z >> 11) 2^-53, z = splitmix64's output function of seed + (n + 1) 0x9E3779B97F4A7C15, under the envelope
 * exp(-ln(1000) (n - d) / (rt60_s sample_rate)); r = e / sqrt(sum e^2) (summed in increasing n: unit energy), h[n] = wet r[n] + dry delta[n].
 * nae_conv_reverb_taps gives the length to the -60 dB point, d + ceil(rt60_s sample_rate).  NAE_ERR_INVALID: sample_rate <= 0, rt60_s outside
 * (0, 10], predelay_s outside [0, 1], dry or wet not finite, n_taps < d + 1, a null pointer.  No context, no device work. */
int nae_conv_reverb_taps(int sample_rate, double rt60_s, double predelay_s);
int nae_conv_design_reverb(int sample_rate, double rt60_s, double predelay_s, double dry, double wet, uint64_t seed, int n_taps, float* taps_host);

/* ------------------------------------------------------------------ K11 biquad cascade
 * no reference code.  Spec ("K11 biquad cascade"): S sections, 1 <= S <= NAE_EQ_MAX_SECTIONS, each five doubles
 * (b0, b1, b2, a1, a2) with a0 = 1, laid out [S][5] on the host; one set for every channel and stream.  f32 samples are widened to double,
 * every section runs in double in transposed direct form II (y = b0 x + z1; z1 = (b1 x - a1 y) + z2; z2 = b2 x - a2 y), the signal stays in
 * double between the sections and is rounded once to f32 behind the last.  The recurrence is computed parallel in time, and the tiling is
 * part of the specification: chunks of NAE_EQ_CHUNK samples on a grid from sample 0, 64 lanes of NAE_EQ_LANE samples; per section a
 * zero-state pass of every lane, a Kogge-Stone scan of the lanes' end states with the powers of the 16-step state map, and a correction of
 * every sample with the zero-input responses p and q; every step one IEEE operation in a fixed order (DESIGN.md gives it).  Input past in_len
 * is zero, output past in_len is not stored.  Bit-exact against the CPU statement (tests/eq_ref/ref_eq.c); any cut of the input into puts
 * gives the same bits; a non-finite input sample i leaves every output sample before i as it was.
 * Errors: a null pointer, n_sections < 1, ch not 1 or 2, a non-finite coefficient or a section that is not strictly stable (|a2| < 1 and
 * |a1| < 1 + a2): NAE_ERR_INVALID; more than NAE_EQ_MAX_SECTIONS sections: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after
 * the checks, nothing is launched.  Views as K9's: interleaved or planar on either side, stream_stride 0 on the source.  The context keeps
 * the tables of its last block call. */
int nae_eq_block_f32(nae_ctx* ctx, const double* coef_host, int n_sections, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                     const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): whole chunks come out as they fill; nae_eq_flush releases the partial last
 * chunk, so in_len frames come out in all (an IIR has no tail to append), equal to the block call's however the input is cut.  A put after
 * the flush: NAE_ERR_STATE. */
int nae_eq_create(nae_ctx* ctx, const double* coef_host, int n_sections, int channels, nae_eq** h);
int nae_eq_put(nae_eq* h, const float* interleaved, size_t S);
int nae_eq_put_host(nae_eq* h, const float* interleaved_host, size_t S);
int nae_eq_flush(nae_eq* h);
size_t nae_eq_available(nae_eq* h);
int nae_eq_receive(nae_eq* h, float* dst, size_t max_frames, size_t* got);
int nae_eq_receive_host(nae_eq* h, float* dst_host, size_t max_frames, size_t* got);
int nae_eq_destroy(nae_eq* h);
/* One section on the host, in double, by the Audio EQ Cookbook's forms: A = 10^(gain_db / 40), w0 = 2 pi freq / sample_rate,
 * alpha = sin w0 / (2 q), every kind divided through by its a0.  kind: NAE_EQ_PEAK, NAE_EQ_LOWSHELF, NAE_EQ_HIGHSHELF (with 2 sqrt(A) alpha),
 * NAE_EQ_LOWPASS, NAE_EQ_HIGHPASS, NAE_EQ_NOTCH (gain_db ignored) of nae_dsp_spec.h.  NAE_ERR_INVALID: an unknown kind, sample_rate <= 0,
 * freq outside (0, sample_rate / 2), q outside [0.1, 40], |gain_db| > 24 or not finite, a null pointer.  No context, no device work. */
int nae_eq_design(int kind, int sample_rate, double freq, double gain_db, double q, double coef_host[5]);

/* ------------------------------------------------------------------ K12 dynamics
 * no reference code.  Spec ("K12 dynamics"): a feed-forward compressor / look-ahead limiter in the dB domain with the smooth
 * decoupled peak detector of Giannoulis, Massberg and Reiss, in double throughout, rounded once to f32.  One detector per stream-channel, or
 * with link = 1 on a stereo stream one per stream on the larger of the two magnitudes.  Per sample: the level xg = K log2|x| (K = 20 log10 2;
 * a zero sample stands at NAE_DYN_FLOOR_DB), the static curve's gain-reduction demand r >= 0 (threshold, slope = 1 - 1 / ratio, a quadratic
 * knee of knee_db), the look-ahead d[n] = max(r[n] ... r[n + lookahead]), the release y1[n] = max(d[n], alpha_release y1[n-1] +
 * (1 - alpha_release) d[n]), the attack yl[n] = alpha_attack yl[n-1] + (1 - alpha_attack) y1[n], and the gain 2^((makeup_db - yl[n]) / K).
 * The log2 and the 2^x are fixed sequences of IEEE double operations that DESIGN.md states with their coefficients; the two recurrences are
 * computed parallel in time on chunks of NAE_DYN_CHUNK samples on a grid from sample 0 (64 lanes of NAE_DYN_LANE samples, a Kogge-Stone scan
 * of the lanes' step maps), and that tiling is part of the specification.  The call is compensated: output sample n is input sample n under
 * a gain that has seen `lookahead` samples ahead; input past in_len is zero, in_len frames come out, output past in_len is not stored.
 * Bit-exact against the CPU statement (tests/dyn_ref/ref_dyn.c); any cut of the input into puts gives the same bits; a non-finite input
 * sample i leaves every output sample before i - lookahead as it was (from there on the output is unspecified; the call returns NAE_OK).
 * With slope = 1, knee_db = 0 and alpha_attack = 0 no output exceeds 10^((threshold_db + makeup_db) / 20) but by the final rounding.
 * Errors: a null pointer, ch not 1 or 2, a parameter that is not finite or outside its range (threshold_db -60 ... 0, slope 0 ... 1,
 * knee_db 0 ... 24, both alphas in [0, 1), makeup_db -24 ... 24, lookahead >= 0, link 0 or 1): NAE_ERR_INVALID; lookahead above
 * NAE_DYN_MAX_LOOKAHEAD: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as K11's. */
typedef struct nae_dyn_params {
    double threshold_db;    /* dB re full scale, -60 ... 0 */
    double slope;           /* 1 - 1 / ratio, 0 ... 1; 1 is a limiter */
    double knee_db;         /* width of the quadratic knee, 0 ... 24 */
    double alpha_attack;    /* exp(-1 / (attack_s sample_rate)), 0 for no smoothing; [0, 1) */
    double alpha_release;   /* exp(-1 / (release_s sample_rate)); [0, 1) */
    double makeup_db;       /* -24 ... 24 */
    int lookahead;          /* samples, 0 ... NAE_DYN_MAX_LOOKAHEAD */
    int link;               /* 1: one detector per stereo stream */
} nae_dyn_params;
int nae_dyn_block_f32(nae_ctx* ctx, const nae_dyn_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                      const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch).  Before the flush the whole chunks whose look-ahead is complete are available:
 * floor((put - lookahead) / NAE_DYN_CHUNK) chunks, never negative; nae_dyn_flush releases the rest, so in_len frames come out in all, equal
 * to the block call's however the input is cut.  A put after the flush: NAE_ERR_STATE. */
int nae_dyn_create(nae_ctx* ctx, const nae_dyn_params* params, int channels, nae_dyn** h);
int nae_dyn_put(nae_dyn* h, const float* interleaved, size_t S);
int nae_dyn_put_host(nae_dyn* h, const float* interleaved_host, size_t S);
int nae_dyn_flush(nae_dyn* h);
size_t nae_dyn_available(nae_dyn* h);
int nae_dyn_receive(nae_dyn* h, float* dst, size_t max_frames, size_t* got);
int nae_dyn_receive_host(nae_dyn* h, float* dst_host, size_t max_frames, size_t* got);
int nae_dyn_destroy(nae_dyn* h);
/* The parameters on the host: slope = 1 - 1 / ratio (ratio = INFINITY: 1), alpha = exp(-1 / (t sample_rate)) (attack_s = 0: 0),
 * lookahead = lround(lookahead_s sample_rate).  NAE_ERR_INVALID: sample_rate <= 0, link not 0 or 1, a null pointer, an argument that is
 * not finite (but ratio = INFINITY) or outside threshold_db -60 ... 0, ratio >= 1, knee_db 0 ... 24, attack_s 0 ... 0.5, release_s
 * 0.001 ... 5, makeup_db -24 ... 24, lookahead_s >= 0 (the constants of nae_dsp_spec.h); NAE_ERR_UNSUPPORTED: a look-ahead above
 * NAE_DYN_MAX_LOOKAHEAD samples at this rate.  No context, no device work. */
int nae_dyn_design(int sample_rate, double threshold_db, double ratio, double knee_db, double attack_s, double release_s, double lookahead_s,
                   double makeup_db, int link, nae_dyn_params* out);

/* ------------------------------------------------------------------ K15 keyed dynamics
 * no reference code.  Spec ("K15 keyed dynamics"): K12 with a side-chain.  The detector's level comes from a key magnitude m[n]
 * instead of |x[n]|: the key is the signal itself (key_ch = 0, `key` null) or an external view of in_len samples with 1 or ch channels
 * (every view K11 takes, stream_stride = 0 included: one key for many streams), run per key channel through n_sections biquads in K11's tiled
 * form exactly (coefficients b0 b1 b2 a1 a2 in double under K11's stability rule, the same tables, order of operations and carry), and
 * m = (float)|w|, rounded once; with n_sections = 0 m = |key|.  A linked stereo detector reads the larger m of the key's channels; unlinked,
 * detector c reads key channel c, or channel 0 of a mono key.  The demand is zero from in_len on: the key is zero there, and the filter's
 * ringing past the end is no demand.  Everything else is K12's, applied to the signal: y = (float)((double)x gain), compensated, in_len
 * frames out.  So an internal key, or a key equal to the signal, with no section gives nae_dyn_block_f32's bits, and a key filtered by n
 * sections the bits of the call with no section keyed by nae_eq_block_f32's output of that key.  Bit-exact against the CPU statement
 * (tests/dynkey_ref/ref_dynkey.c).  A non-finite key sample i leaves every output sample before i - lookahead as it was (nothing is specified
 * from there on: an IIR carries it); with an external key a non-finite signal sample changes its own output sample only.
 * Errors: K12's, then NAE_ERR_INVALID for key_ch not 0, 1 or ch, a key view with key_ch = 0 or none with key_ch > 0, negative n_sections,
 * a non-finite or not strictly stable section; NAE_ERR_UNSUPPORTED for more than NAE_DYNKEY_MAX_SECTIONS sections; in_len = 0 or
 * n_streams = 0: NAE_OK after the checks.  nae_dyn_design and nae_eq_design fill the record. */
typedef struct nae_dynkey_params {
    nae_dyn_params dyn;
    int key_ch;                                   /* 0: the signal is its own key; else 1 or ch */
    int n_sections;                               /* 0 ... NAE_DYNKEY_MAX_SECTIONS */
    double coef[NAE_DYNKEY_MAX_SECTIONS][5];
} nae_dynkey_params;
int nae_dynkey_block_f32(nae_ctx* ctx, const nae_dynkey_params* params, const nae_sig* src, const nae_sig* key /* null iff key_ch = 0 */,
                         size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
/* Streaming handle.  A put carries frames of channels + key_ch floats, the signal's channels and then the key's, so the two cannot fall out
 * of step; a receive delivers frames of `channels` floats.  Availability, flush and errors as nae_dyn's; any cut of the input into puts gives
 * the block call's bits. */
int nae_dynkey_create(nae_ctx* ctx, const nae_dynkey_params* params, int channels, nae_dynkey** h);
int nae_dynkey_put(nae_dynkey* h, const float* interleaved, size_t S);
int nae_dynkey_put_host(nae_dynkey* h, const float* interleaved_host, size_t S);
int nae_dynkey_flush(nae_dynkey* h);
size_t nae_dynkey_available(nae_dynkey* h);
int nae_dynkey_receive(nae_dynkey* h, float* dst, size_t max_frames, size_t* got);
int nae_dynkey_receive_host(nae_dynkey* h, float* dst_host, size_t max_frames, size_t* got);
int nae_dynkey_destroy(nae_dynkey* h);

/* ------------------------------------------------------------------ K16 echo
 * no reference code.  Spec ("K16 echo"): a feedback delay with a damping filter in the loop and optional ping-pong.  Per
 * stream-channel c a delay line w_c of f32 samples; s(c) = 1 - c with cross = 1 on a stereo stream, else c; D_c = delay[c] (mono: delay[0]).
 * For n = 0 ... in_len - 1, every step one IEEE double operation in the order written:
 *   v_c[n] = n >= D_c ? (double)w_s(c)[n - D_c] : 0
 *   f_c    = the n_sections biquads of K11 over v_c in K11's tiled form exactly (chunks of NAE_EQ_CHUNK samples from n = 0, zero state in front
 *            of n = 0, the same tables, order of operations and carry), kept in double; n_sections = 0: f_c = v_c
 *   w_c[n] = (float)((double)x_c[n] + (feedback f_c[n]))            the line: rounded once per trip
 *   y_c[n] = (float)((dry (double)x_c[n]) + (wet f_c[n]))
 * A delay of at least one chunk puts the whole delayed input of a chunk in the past, so the loop needs no scan over the delay: a chunk is one
 * K11 cascade over known samples.  Input past in_len is zero, output past in_len is not stored; the echoes' tail past in_len is dropped (a
 * caller who wants it puts zeros).  Bit-exact against the CPU statement (tests/echo_ref/ref_echo.c); any cut of the input into puts gives the
 * same bits.  A non-finite sample stays in its own stream (and, without cross, in its own channel) and reaches no sample before it.
 * Stability: with |feedback| < 1 the loop is stable when no section's gain exceeds 1 at any frequency, which holds for what nae_echo_design
 * makes; with the caller's own coefficients the loop gain is the caller's responsibility: nothing here checks it.
 * Errors: a null pointer, ch not 1 or 2, feedback, wet or dry not finite, |feedback| > NAE_ECHO_MAX_FEEDBACK, cross not 0 or 1, negative
 * n_sections, a non-finite or not strictly stable section: NAE_ERR_INVALID; a delay (of a channel the call has) outside
 * [NAE_ECHO_MIN_DELAY, NAE_ECHO_MAX_DELAY] or more than NAE_ECHO_MAX_SECTIONS sections: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0:
 * NAE_OK after the checks, nothing is launched.  Views and aliasing as nae_eq_block_f32's.  The lines of a block call live in a grow-only
 * workspace of the context; a batch whose lines exceed 256 MiB runs in groups of streams (debug key echo_group). */
typedef struct nae_echo_params {
    int delay[2];                                 /* samples per channel, NAE_ECHO_MIN_DELAY ... NAE_ECHO_MAX_DELAY; mono reads delay[0] */
    double feedback;                              /* g, |g| <= NAE_ECHO_MAX_FEEDBACK */
    int cross;                                    /* 1: ping-pong, each channel's loop reads the other channel's line (stereo only) */
    double wet, dry;
    int n_sections;                               /* 0 ... NAE_ECHO_MAX_SECTIONS */
    double coef[NAE_ECHO_MAX_SECTIONS][5];        /* the loop's damping filter: K11 sections b0 b1 b2 a1 a2 */
} nae_echo_params;
int nae_echo_block_f32(nae_ctx* ctx, const nae_echo_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                       const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): whole chunks of NAE_EQ_CHUNK frames come out as they fill; nae_echo_flush
 * releases the partial last chunk, so in_len frames come out in all, equal to the block call's however the input is cut (the chunks are
 * counted from the stream's first sample).  The handle owns its delay lines and the sections' carries.  A put after the flush: NAE_ERR_STATE. */
int nae_echo_create(nae_ctx* ctx, const nae_echo_params* params, int channels, nae_echo** h);
int nae_echo_put(nae_echo* h, const float* interleaved, size_t S);
int nae_echo_put_host(nae_echo* h, const float* interleaved_host, size_t S);
int nae_echo_flush(nae_echo* h);
size_t nae_echo_available(nae_echo* h);
int nae_echo_receive(nae_echo* h, float* dst, size_t max_frames, size_t* got);
int nae_echo_receive_host(nae_echo* h, float* dst_host, size_t max_frames, size_t* got);
int nae_echo_destroy(nae_echo* h);
/* The record on the host: delay[c] = lround(delay_s sample_rate) for the left and the right channel; damp_hz > 0 adds a NAE_EQ_LOWPASS section,
 * then lowcut_hz > 0 a NAE_EQ_HIGHPASS section, both by nae_eq_design with q = 1 / sqrt 2 (Butterworth sections: their gain never exceeds 1,
 * so the designed loop with |feedback| < 1 is stable).  NAE_ERR_INVALID: sample_rate <= 0, a null pointer, an argument that is not finite,
 * a delay outside [NAE_ECHO_MIN_DELAY, NAE_ECHO_MAX_DELAY] samples at this rate, |feedback| > NAE_ECHO_MAX_FEEDBACK, a negative corner or one
 * at or above sample_rate / 2, cross not 0 or 1.  No context, no device work. */
int nae_echo_design(int sample_rate, double delay_s_left, double delay_s_right, double feedback, double damp_hz, double lowcut_hz, double wet,
                    double dry, int cross, nae_echo_params* out);

/* ------------------------------------------------------------------ K17 modulated delay (chorus, flanger, vibrato)
 * no reference code.  Spec ("K17 modulated delay"): one short delay whose length an LFO sweeps, read between samples, with
 * feedback.  Per stream-channel c a line w of f32 samples.  For n = 0 ... in_len - 1 (n counts from the stream's first sample, 64-bit) and
 * voice v = 0 ... n_voices - 1, every step one IEEE double operation in the order written:
 *   phi = (uint32)(phase0 + voice_phase[v] + (c == 1 ? phase_ch : 0) + (uint32)((uint64)n rate_inc))          all mod 2^32
 *   t   = (double)(int32)phi 2^-31                                                                            in [-1, 1)
 *   l   = NAE_MOD_SINE:     y = (4 t) (1 - |t|);  l = (0.225 ((y |y|) - y)) + y          within 1.1e-3 of sin(pi t), |l| <= 1
 *         NAE_MOD_TRIANGLE: l = (2 |t|) - 1
 *   d = delay + (depth l);  k = floor(d);  f = d - k
 *   a = w[n - k + 1], b = w[n - k], c2 = w[n - k - 1], e = w[n - k - 2]                  as double; an index below 0 reads 0
 *   ca = ((-(f (f - 1))) (f - 2)) (1 / 6);  cb = (((f + 1) (f - 1)) (f - 2)) 0.5;  cc = ((-((f + 1) f)) (f - 2)) 0.5;  ce = (((f + 1) f) (f - 1)) (1 / 6)
 *   tap_v = (((ca a) + (cb b)) + (cc c2)) + (ce e)                                       4-point Lagrange interpolation
 * then v = tap_0 (+ tap_1 ... in voice order), u = v (1 / n_voices) and
 *   w[n] = feedback == 0 ? x[n] : (float)((double)x[n] + (feedback u))                   the line: rounded once per trip
 *   y[n] = (float)((dry (double)x[n]) + (wet u))
 * delay - depth >= NAE_MOD_MIN_DELAY puts the newest sample a tap reads, n - k + 1, behind n: floor(delay - depth) - 1 consecutive samples read
 * only line samples in front of them and are computed in parallel; no sample's arithmetic depends on how many are.  Output past in_len is
 * not stored and the tail past in_len is dropped (a caller who wants it puts zeros).  Bit-exact against the CPU statement
 * (tests/mod_ref/ref_mod.c); any cut of the input into puts gives the same bits.  A non-finite sample stays in its stream-channel and reaches
 * no sample before it.
 * Errors: a null pointer, ch not 1 or 2, a non-finite delay, depth, feedback, wet or dry, |feedback| > NAE_MOD_MAX_FEEDBACK, depth < 0,
 * n_voices < 1, an unknown shape: NAE_ERR_INVALID; delay - depth < NAE_MOD_MIN_DELAY, delay + depth > NAE_MOD_MAX_DELAY (both in double as
 * written) or more than NAE_MOD_MAX_VOICES voices: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is
 * launched.  Views as nae_eq_block_f32's, stream_stride 0 on the source included; dst may be src in the same view.  No workspace. */
typedef struct nae_mod_params {
    double delay;                                 /* the centre delay in samples */
    double depth;                                 /* the sweep's amplitude in samples, >= 0 */
    double feedback;                              /* g, |g| <= NAE_MOD_MAX_FEEDBACK */
    double wet, dry;
    uint32_t rate_inc;                            /* the LFO's phase step per sample, in turns 2^32 */
    uint32_t phase0;                              /* the LFO's phase at n = 0 */
    uint32_t phase_ch;                            /* added on channel 1 only: the stereo spread (mono does not read it) */
    int n_voices;                                 /* 1 ... NAE_MOD_MAX_VOICES */
    uint32_t voice_phase[NAE_MOD_MAX_VOICES];     /* every voice's phase offset */
    int shape;                                    /* NAE_MOD_SINE or NAE_MOD_TRIANGLE */
} nae_mod_params;
int nae_mod_block_f32(nae_ctx* ctx, const nae_mod_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): whole chunks of NAE_EQ_CHUNK frames come out as they fill; nae_mod_flush
 * releases the partial last chunk, so in_len frames come out in all, equal to the block call's however the input is cut (phases and samples
 * are counted from the stream's first sample).  The handle keeps the last 3072 line samples of every channel and the sample count.  A put
 * after the flush: NAE_ERR_STATE. */
int nae_mod_create(nae_ctx* ctx, const nae_mod_params* params, int channels, nae_mod** h);
int nae_mod_put(nae_mod* h, const float* interleaved, size_t S);
int nae_mod_put_host(nae_mod* h, const float* interleaved_host, size_t S);
int nae_mod_flush(nae_mod* h);
size_t nae_mod_available(nae_mod* h);
int nae_mod_receive(nae_mod* h, float* dst, size_t max_frames, size_t* got);
int nae_mod_receive_host(nae_mod* h, float* dst_host, size_t max_frames, size_t* got);
int nae_mod_destroy(nae_mod* h);
/* The record on the host: delay = (delay_ms 1e-3) sample_rate and depth = (depth_ms 1e-3) sample_rate in double, not rounded;
 * rate_inc = (uint32)llround((rate_hz / sample_rate) 2^32); voice_phase[v] = (uint32)(((uint64)v << 32) / voices): the voices spread evenly over
 * a turn; phase_ch = (uint32)llround(spread 2^31): a spread of 1 puts the right channel half a turn behind; phase0 = 0.  rate_hz = 0 is a
 * fixed comb.  NAE_ERR_INVALID: sample_rate <= 0, a null pointer, an argument that is not finite, rate_hz outside [0, 20], depth_ms < 0,
 * a delay range outside [NAE_MOD_MIN_DELAY, NAE_MOD_MAX_DELAY] samples at this rate, |feedback| > NAE_MOD_MAX_FEEDBACK, voices outside
 * 1 ... NAE_MOD_MAX_VOICES, spread outside [0, 1], an unknown shape.  No context, no device work. */
int nae_mod_design(int sample_rate, double rate_hz, double delay_ms, double depth_ms, double feedback, int voices, double spread, int shape,
                   double wet, double dry, nae_mod_params* out);

/* ------------------------------------------------------------------ K18 saturation (drive, soft and hard clipping)
 * no reference code.  Spec ("K18 saturation"): a static curve run at M = oversample times the sample rate, M in {1, 2, 4, 8}, so that
 * the harmonics it makes do not fold back into the audible band.  K = NAE_SAT_HALF = 16.
 * Taps, M > 1: N = 2 K M + 1; hd[j] = nae_fir_design(kind 0, sample_rate 2 M, f_hi 1.0, n_taps N)[j] (Kaiser beta 8, cutoff 1 / M, unit sum, rounded
 * once to f32); hu[j] = M hd[j] (exact).  No tap is skipped, whatever its value.
 * Per stream-channel, n = 0 ... in_len - 1, x[i] = 0 for i < 0, every step one IEEE f32 operation in the order written, fma the fused one:
 *   up     for p = 0 ... M - 1, m = M n + p:  a = hu[p] x[n];  for i = 1, 2, ... while p + i M <= 2 K M:  a = fma(hu[p + i M], x[n - i], a);  u[m] = a
 *   shape  t = fma(g, u[m], b);  v[m] = f(t) - f(b);  v[m] = 0 for m < 0
 *            NAE_SAT_SOFT: c = t > 3 ? 3 : (t < -3 ? -3 : t);  q = c c;  f = (c (27 + q)) / (27 + (9 q))          the Pade form of tanh
 *            NAE_SAT_HARD: f = t > 1 ? 1 : (t < -1 ? -1 : t)
 *   down   s = hd[0] v[M n];  for j = 1 ... 2 K M:  s = fma(hd[j], v[M n - j], s)
 *   mix    y[n] = (dry x[n - D]) + (wet s),  D = 2 K = 32 the latency
 * M = 1: no filter, D = 0: y[n] = (dry x[n]) + (wet (f(fma(g, x[n], b)) - f(b))).
 * y[n] depends on x[n - 64 ... n] alone: any cut into chunks, tiles, launches or puts gives the same bits; with b = 0 negating x negates y; a
 * non-finite x[n] reaches y[n ... n + 64] of its own stream-channel and nothing else; output past in_len is not stored.  Bit-exact against the
 * CPU statement (tests/sat_ref/ref_sat.c).
 * Errors: a null pointer, ch not 1 or 2, a non-finite field, an unknown curve: NAE_ERR_INVALID; oversample not 1, 2, 4 or 8: NAE_ERR_UNSUPPORTED;
 * dst->base equal to src->base: NAE_ERR_INVALID (a tile reads the 64 samples in front of it after a neighbouring wave may have written them: the
 * call does not work in place; views that overlap otherwise are not detected and give undefined samples); in_len = 0 or n_streams = 0: NAE_OK
 * after the checks, nothing is launched.  The block call is causal and writes in_len frames (a caller who wants the last D puts D zeros).  Views
 * as nae_eq_block_f32's, stream_stride 0 on the source included.  The context keeps the device taps of every M it has run: a warm call allocates
 * and waits for nothing.  No workspace. */
typedef struct nae_sat_params {
    int oversample;     /* M: 1, 2, 4 or 8 */
    int curve;          /* NAE_SAT_SOFT or NAE_SAT_HARD */
    float drive;        /* g */
    float bias;         /* b */
    float wet, dry;
} nae_sat_params;
int nae_sat_latency(int oversample);                       /* D: 0 for 1, 32 for 2, 4 and 8, -1 otherwise */
int nae_sat_taps(int oversample, float* hd_host);          /* writes the 2 K M + 1 taps hd and returns their count; 0 for M = 1 (and for an M that is not supported, or null) */
int nae_sat_block_f32(nae_ctx* ctx, const nae_sat_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): whole chunks of NAE_EQ_CHUNK frames come out as they fill (the last chunk of input
 * stays for the 64 samples the next one reads in front of it); nae_sat_flush puts D zero frames behind the input and releases the rest, so
 * in_len + D frames come out in all, equal to the block call's on the input extended by D zeros however the input is cut.  A put after the
 * flush: NAE_ERR_STATE. */
int nae_sat_create(nae_ctx* ctx, const nae_sat_params* params, int channels, nae_sat** h);
int nae_sat_put(nae_sat* h, const float* interleaved, size_t S);
int nae_sat_put_host(nae_sat* h, const float* interleaved_host, size_t S);
int nae_sat_flush(nae_sat* h);
size_t nae_sat_available(nae_sat* h);
int nae_sat_receive(nae_sat* h, float* dst, size_t max_frames, size_t* got);
int nae_sat_receive_host(nae_sat* h, float* dst_host, size_t max_frames, size_t* got);
int nae_sat_destroy(nae_sat* h);
/* The record on the host, in double, each field rounded once to f32: drive = 10^(drive_db / 20), drive_db in [0, 48]; bias in [0, 1] (an
 * asymmetric curve: even harmonics); wet = mix 10^(output_db / 20), output_db in [-24, 24], mix in [0, 1]; dry = 1 - mix.  NAE_ERR_INVALID: a
 * null pointer, an argument that is not finite or outside its range, an unknown curve; NAE_ERR_UNSUPPORTED: oversample not 1, 2, 4 or 8.  No
 * context, no device work. */
int nae_sat_design(double drive_db, double bias, int curve, int oversample, double output_db, double mix, nae_sat_params* out);

/* ------------------------------------------------------------------ K19 gate (noise gate and downward expander)
 * no reference code.  Spec ("K19 gate"): one detector per stream-channel, or with link = 1 on a stereo stream one per stream.
 * Arithmetic is double, every step one IEEE operation in the order written, rounded once to f32.  K = 20 log10(2), KINV = 1 / K, dyn_log2 and
 * dyn_exp2 are K12's.  Per detector, n = 0 ... in_len - 1, input at or past in_len zero:
 *   level       a[n] = |x[n]| in f32, with link the larger of the two channels' (b > a ? b : a, a the first channel's)
 *   hysteresis  s[n] = 1 where a[n] >= open_lin, 0 where a[n] < close_lin, else s[n - 1]; s[-1] = 0; a NaN keeps the state
 *   hold        the gate is open at n iff some m in [n - hold, n + lookahead] has s[m] = 1 (integers, exact)
 *   depth       expand = 0: range_db.  expand = 1: xg = K dyn_log2((double)a[n]), a zero sample at NAE_DYN_FLOOR_DB; u = threshold_db - xg;
 *               v = slope u; depth = u <= 0 ? 0 : (v < range_db ? v : range_db)
 *   smoother    y[n] = (alpha y[n - 1]) + b; open: alpha = alpha_attack, b = 0.0; closed: alpha = alpha_release,
 *               b = (1 - alpha_release) depth[n], the factor made once; y[-1] = range_db
 *   gain        g[n] = dyn_exp2((0.0 - y[n]) KINV); out_c[n] = (float)((double)x_c[n] g[n]) for each channel of the detector
 * The smoother is tiled on K12's grid (NAE_DYN_LANE samples per lane, chunks of NAE_DYN_CHUNK counted from the stream's sample 0): a lane
 * composes its 16 maps, the 64 maps are scanned in six Kogge-Stone steps, a lane starts from the scanned map of the lane below it applied to
 * the chunk's carry and runs the plain recurrence; the tiling is part of the specification.  The call is compensated as K12 is: output
 * sample n is input sample n under a decision that has seen lookahead samples ahead; in_len frames come out and nothing past in_len is
 * stored.  So any cut into puts gives the block call's bits; with alpha_attack = 0 a signal that never falls below open_lin comes out bit
 * for bit; a non-finite sample i leaves every output sample before i - lookahead as it was, and the call returns NAE_OK.  Bit-exact against
 * the CPU statement (tests/gate_ref/ref_gate.c).
 * Errors: a null pointer, ch not 1 or 2, a field that is not finite or outside its range (0 < close_lin <= open_lin; threshold_db -90 ... 0;
 * slope 0 ... 99; range_db 0 ... 120; the alphas in [0, 1); hold and lookahead not negative; expand and link 0 or 1): NAE_ERR_INVALID; a
 * lookahead above NAE_DYN_MAX_LOOKAHEAD or a hold above NAE_GATE_MAX_HOLD: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after
 * the checks, nothing is launched.  Views as nae_dyn_block_f32's: stream_stride 0 on the source and dst->base == src->base are allowed. */
typedef struct nae_gate_params {
    float open_lin, close_lin;   /* the two thresholds as magnitudes */
    double threshold_db;         /* the expander's depth starts here */
    double slope;                /* ratio - 1; not read with expand = 0 */
    double range_db;             /* the deepest attenuation */
    double alpha_attack, alpha_release;
    int hold;                    /* samples */
    int lookahead;               /* samples */
    int expand;                  /* 0: gate, 1: downward expander */
    int link;                    /* 1: one detector per stereo stream */
} nae_gate_params;
int nae_gate_block_f32(nae_ctx* ctx, const nae_gate_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                       const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): before the flush floor((put - lookahead) / NAE_DYN_CHUNK) whole chunks are
 * available, never negative; nae_gate_flush releases the rest, so in_len frames come out in all, equal to the block call's however the input
 * is cut.  A put after the flush: NAE_ERR_STATE. */
int nae_gate_create(nae_ctx* ctx, const nae_gate_params* params, int channels, nae_gate** h);
int nae_gate_put(nae_gate* h, const float* interleaved, size_t S);
int nae_gate_put_host(nae_gate* h, const float* interleaved_host, size_t S);
int nae_gate_flush(nae_gate* h);
size_t nae_gate_available(nae_gate* h);
int nae_gate_receive(nae_gate* h, float* dst, size_t max_frames, size_t* got);
int nae_gate_receive_host(nae_gate* h, float* dst_host, size_t max_frames, size_t* got);
int nae_gate_destroy(nae_gate* h);
/* The record on the host, in double: open_lin = (float)10^(threshold_db / 20); close_lin = (float)10^((threshold_db - hysteresis_db) / 20);
 * slope = ratio - 1; alpha = exp(-1 / (t sample_rate)), attack_s = 0 gives 0; hold = lround(hold_s sample_rate); lookahead as nae_dyn_design
 * makes it; expand = mode.  mode: NAE_GATE_MODE_GATE or NAE_GATE_MODE_EXPANDER.  Ranges: threshold_db -90 ... 0, hysteresis_db 0 ... 24,
 * range_db 0 ... 120, ratio 1 ... 100, attack_s 0 ... 0.5, hold_s 0 ... 10, release_s 0.001 ... 5, lookahead_s not negative.
 * NAE_ERR_INVALID: a null pointer, sample_rate <= 0, an unknown mode, link not 0 or 1, an argument that is not finite or outside its range;
 * NAE_ERR_UNSUPPORTED: a look-ahead above NAE_DYN_MAX_LOOKAHEAD samples or a hold above NAE_GATE_MAX_HOLD samples at that rate.  No
 * context, no device work. */
int nae_gate_design(int sample_rate, int mode, double threshold_db, double hysteresis_db, double range_db, double ratio, double attack_s,
                    double hold_s, double release_s, double lookahead_s, int link, nae_gate_params* out);

/* ------------------------------------------------------------------ K20 multiband (crossover and per-band compressor)
 * no reference code.  Spec ("K20 multiband"): a crossover tree of K11 sections splits every channel into B = n_bands bands,
 * 2 ... NAE_MB_MAX_BANDS; K12 runs on every band under the band's own record; the bands are added.  The sections coef[s] = (b0, b1, b2, a1, a2)
 * stand in fixed slots, n_sections = 4, 9 or 14 of them, each under K11's stability rule, each run in K11's tiled form exactly (the tables
 * of nae_eq_block_f32, the same order of operations, the same carry), the signal double between the sections of a path:
 *   B = 2   s0 s1 = LP(f1); s2 s3 = HP(f1).                                   band0 = x s0 s1; band1 = x s2 s3
 *   B = 3   s0 s1 = LP(f1); s2 = AP(f2); s3 s4 = HP(f1); s5 s6 = LP(f2); s7 s8 = HP(f2).
 *           band0 = x s0 s1 s2; h = x s3 s4; band1 = h s5 s6; band2 = h s7 s8
 *   B = 4   s0 s1 = LP(f2); s2 = AP(f3); s3 s4 = LP(f1); s5 s6 = HP(f1); s7 s8 = HP(f2); s9 = AP(f1); s10 s11 = LP(f3); s12 s13 = HP(f3).
 *           l = x s0 s1 s2; band0 = l s3 s4; band1 = l s5 s6; h = x s7 s8 s9; band2 = h s10 s11; band3 = h s12 s13
 * The block call takes any checked sections in these slots; nae_mb_design fills them with the halves of fourth-order Linkwitz-Riley
 * crossovers and the all-passes that make the bands add to AP(f1) ... AP(f_(B-1)), a flat magnitude.
 *   band signal  xb_b[n] = (float)w_b[n], the path's double output rounded once: nae_eq_block_f32's output for the path's sections, bit for bit
 *   per band     yb_b = K12 on xb_b with band[b]: steps 1 - 6 and the tiling of nae_dyn_block_f32, zero demand from in_len on; lookahead and
 *                link are equal in all bands.  A band in bypass_mask has yb_b = xb_b (a band with slope 0 and makeup_db 0 gives the same bits:
 *                dyn_exp2(0) is exactly 1)
 *   sum          y[n] = (float)((((double)yb_0 + (double)yb_1) + (double)yb_2) + (double)yb_3) over the bands not in mute_mask, in band order,
 *                starting from the first of them; 0.0f where every band is muted.  Muting all bands but one is a solo
 * So the call equals the composition of the existing entries per band, eq then dyn then the sum; every tiling, slab, group of streams and cut
 * into puts gives the same bits; in_len frames come out, compensated for the look-ahead as K12 is; a non-finite sample i leaves every output
 * sample before i - lookahead as it was, and the call returns NAE_OK.  Bit-exact against the CPU statement (tests/mb_ref/ref_mb.c).
 * Errors: a null pointer, ch not 1 or 2, n_bands < 2, n_sections not the tree's count for n_bands, a section that is not finite or not
 * strictly stable, a band record nae_dyn_block_f32 would refuse as invalid, lookahead or link unequal between the bands, a mask bit at or
 * above n_bands: NAE_ERR_INVALID; n_bands above NAE_MB_MAX_BANDS or a lookahead above NAE_DYN_MAX_LOOKAHEAD: NAE_ERR_UNSUPPORTED; in_len = 0
 * or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as nae_eq_block_f32's: stream_stride 0 on the source and
 * dst->base == src->base in the same view are allowed.  The band signals stand in a workspace of the context of at most 256 MiB: a larger
 * batch runs in groups of streams and slabs of chunks (debug keys mb_group, mb_slab). */
typedef struct nae_mb_params {
    int n_bands;                          /* B: 2 ... NAE_MB_MAX_BANDS */
    int n_sections;                       /* 4, 9 or 14: the tree of B bands */
    double coef[NAE_MB_MAX_SECTIONS][5];  /* the slots' sections */
    nae_dyn_params band[NAE_MB_MAX_BANDS];
    unsigned mute_mask, bypass_mask;      /* bit b: band b is left out of the sum / passes its compressor by */
} nae_mb_params;
int nae_mb_block_f32(nae_ctx* ctx, const nae_mb_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): before the flush floor((put - lookahead) / NAE_DYN_CHUNK) whole chunks are
 * available, never negative; nae_mb_flush releases the rest, so in_len frames come out in all, equal to the block call's however the input
 * is cut.  A put after the flush: NAE_ERR_STATE. */
int nae_mb_create(nae_ctx* ctx, const nae_mb_params* params, int channels, nae_mb** h);
int nae_mb_put(nae_mb* h, const float* interleaved, size_t S);
int nae_mb_put_host(nae_mb* h, const float* interleaved_host, size_t S);
int nae_mb_flush(nae_mb* h);
size_t nae_mb_available(nae_mb* h);
int nae_mb_receive(nae_mb* h, float* dst, size_t max_frames, size_t* got);
int nae_mb_receive_host(nae_mb* h, float* dst_host, size_t max_frames, size_t* got);
int nae_mb_destroy(nae_mb* h);
/* The record on the host, in double: crossover_hz[0 ... n_bands - 2] strictly ascending, each valid for nae_eq_design at sample_rate; LP(f) and
 * HP(f) are nae_eq_design(NAE_EQ_LOWPASS | NAE_EQ_HIGHPASS, sample_rate, f, 0, 0.7071067811865476), two of each in a row a fourth-order
 * Linkwitz-Riley half; AP(f) is the cookbook's all-pass of the same w0, alpha and q: b = (1 - alpha, -2 cos w0, 1 + alpha) / a0,
 * a = (-2 cos w0, 1 - alpha) / a0, a0 = 1 + alpha.  bands[0 ... n_bands - 1] come from nae_dyn_design.  Anything the block call would refuse, a
 * null pointer, sample_rate <= 0 or n_bands outside 2 ... NAE_MB_MAX_BANDS: NAE_ERR_INVALID.  No context, no device work. */
int nae_mb_design(int sample_rate, int n_bands, const double* crossover_hz, const nae_dyn_params* bands, unsigned mute_mask, unsigned bypass_mask,
                  nae_mb_params* out);

/* ------------------------------------------------------------------ K13 spectral gate
 * no reference code.  Spec ("K13 spectral gate"): noise reduction on the STFT at n_fft = 512 ... 4096, hop H = n_fft / 4, in the
 * vocoder's geometry at tempo 1 (frame f starts at sample (f - 3) H; the signal is zero outside [0, in_len)).  Per frame and bin the power
 * p = X.x X.x + X.y X.y of the canonical r2c of the Hann-windowed frame is compared with the channel's learned noise power:
 * d = p > profile[c][k] thr_scale (one f32 product; a NaN compares false; frames outside the signal are closed).  The decisions are smoothed
 * in integers by a triangle over time_smooth frames and freq_smooth bins to either side (mirrored at bins 0 and n_fft / 2) to a count c of at
 * most C = (time_smooth + 1)^2 (freq_smooth + 1)^2; the bin's gain is 1 where c = C and floor_gain + span ((float)c inv_c) elsewhere, with
 * span = (float)(1 - floor_gain) and inv_c = (float)(1 / C) rounded once from double.  Synthesis is the vocoder's: c2r, window, overlap-add in
 * increasing frame order, NAE_OLA_GAIN.  The output has the input's length and is aligned with it sample for sample; with floor_gain = 1 the
 * call is the STFT identity.  Bit-exact against the CPU statement (tests/denoise_ref/ref_denoise.c) under every tiling (debug key dn_tile)
 * and any cut of the input into puts.  A non-finite sample i changes only the samples from (floor(i / H) - time_smooth - 3) H up to, not
 * including, (floor(i / H) + time_smooth + 4) H of its own stream-channel; the call returns NAE_OK.
 * profile_dev: device memory, [profile_ch][n_fft / 2 + 1] noise powers; profile_ch = 1 is one profile for every channel.  It is read by the
 * launch: keep it alive and unchanged until the stream has run it (a handle copies it at creation).
 * Errors: a null pointer, ch not 1 or 2, profile_ch not 1 or ch, time_smooth outside 0 ... NAE_DENOISE_MAX_TIME, freq_smooth outside
 * 0 ... NAE_DENOISE_MAX_FREQ, thr_scale negative or not finite, floor_gain outside [0, 1] or not finite: NAE_ERR_INVALID; n_fft other than 512,
 * 1024, 2048, 4096: NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as K9's. */
typedef struct nae_denoise_params {
    int n_fft;              /* 512, 1024, 2048 or 4096 */
    int time_smooth;        /* Tn: frames to either side, 0 ... NAE_DENOISE_MAX_TIME */
    int freq_smooth;        /* Fn: bins to either side, 0 ... NAE_DENOISE_MAX_FREQ */
    float thr_scale;        /* a bin is open where its power exceeds profile * thr_scale; >= 0 */
    float floor_gain;       /* gain of a fully closed bin, 0 ... 1 */
} nae_denoise_params;
/* The parameters on the host: thr_scale = (float)10^(sensitivity_db / 10), floor_gain = (float)10^(-reduction_db / 20).  NAE_ERR_INVALID: a null
 * pointer, an argument that is not finite, reduction_db outside 0 ... 48, sensitivity_db outside -6 ... 24, a smoothing width outside its range;
 * NAE_ERR_UNSUPPORTED: n_fft other than 512 ... 4096.  No context, no device work. */
int nae_denoise_design(double reduction_db, double sensitivity_db, int n_fft, int time_smooth, int freq_smooth, nae_denoise_params* out);
/* The noise profile of an excerpt: channel c of stream 0 of `src`, `len` samples.  The frames start at 0, H, 2 H, ... while start + n_fft <= len
 * (n of them; n = 0: NAE_ERR_INVALID); profile_dev[c][k] = (float)(sum over the frames, in order, of (double)p[k] / (double)n).  Asynchronous on
 * the context's stream, like the block entries; profile_dev receives [ch][n_fft / 2 + 1] floats. */
int nae_denoise_profile_f32(nae_ctx* ctx, int n_fft, const nae_sig* src, size_t len, int ch, float* profile_dev);
int nae_denoise_block_f32(nae_ctx* ctx, const nae_denoise_params* params, const float* profile_dev, int profile_ch, const nae_sig* src,
                          size_t in_len, int ch, size_t n_streams, const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch); the profile is copied into memory the handle owns (on the context's stream: no
 * wait).  With H = n_fft / 4, after every put floor((put total - (time_smooth + 3) H) / H) H frames have become available in all, never fewer
 * than zero; nae_denoise_flush releases the rest, so in_len frames come out in all, equal to the block call's however the input is cut.  A put
 * after the flush: NAE_ERR_STATE. */
int nae_denoise_create(nae_ctx* ctx, const nae_denoise_params* params, const float* profile_dev, int profile_ch, int channels, nae_denoise** h);
int nae_denoise_put(nae_denoise* h, const float* interleaved, size_t S);
int nae_denoise_put_host(nae_denoise* h, const float* interleaved_host, size_t S);
int nae_denoise_flush(nae_denoise* h);
size_t nae_denoise_available(nae_denoise* h);
int nae_denoise_receive(nae_denoise* h, float* dst, size_t max_frames, size_t* got);
int nae_denoise_receive_host(nae_denoise* h, float* dst_host, size_t max_frames, size_t* got);
int nae_denoise_destroy(nae_denoise* h);

/* ------------------------------------------------------------------ K21 separation
 * no reference code.  Spec ("K21 separation"): harmonic/percussive separation by medians over the STFT (Fitzgerald), in K13's
 * geometry: n_fft = 512 ... 4096, hop H = n_fft / 4, frame f starts at sample (f - 3) H, the signal is zero outside [0, in_len).  Per frame
 * and bin the key q = (uint16)(bits(p) >> 16) is the upper half of the f32 power p = X.x X.x + X.y X.y (0 for a frame outside the signal);
 * value(q) is the float whose bits are q << 16.  Hq is the median of the keys of time_span frames to either side at that bin, Pq the median
 * of the keys of freq_span bins to either side in that frame (mirrored at bins 0 and n_fft / 2), both in integers.  The mask m is, hard:
 * 1 where Hq >= Pq, else 0; soft: with h = value(Hq), p = value(Pq) and s = (double)h + (double)p, 0.5 where s = 0, else (float)((double)h / s).
 * The bin's gain is G = gain_p + d m (one product, one add) with d = (float)((double)gain_h - (double)gain_p).  Synthesis is the vocoder's:
 * c2r, window, overlap-add in increasing frame order, NAE_OLA_GAIN.  The output has the input's length and is aligned with it sample for
 * sample; with gain_h = gain_p the call is the STFT identity times that gain.  Bit-exact against the CPU statement
 * (tests/hpss_ref/ref_hpss.c) under every tiling (debug key hpss_tile) and any cut of the input into puts.  Finite inputs whose power
 * overflows f32 are unspecified.  A non-finite sample i changes only the samples from (floor(i / H) - time_span - 3) H up to, not
 * including, (floor(i / H) + time_span + 4) H of its own stream-channel, and the output is non-finite only from (floor(i / H) - 3) H up
 * to, not including, (floor(i / H) + 4) H: the blocks fed by the four frames that hold the sample.  Outside those blocks the output is
 * finite and has the statement's bits; the call returns NAE_OK.  (The sample makes every key of its four frames non-finite; such a key
 * ranks above every finite one whatever its sign and payload, and a frame without the sample sees at most min(4, time_span) of them among
 * its 2 time_span + 1, never a majority: its medians stay finite.  The overflow sentence is about finite samples alone: their spectrum stays
 * finite while a power is +Inf, and the mask there is not specified; a non-finite sample's frames are non-finite under any mask.)
 * Errors: a null pointer, ch not 1 or 2, a span outside 0 ... NAE_HPSS_MAX_SPAN, hard not 0 or 1, a gain that is negative, above
 * (float)10^(NAE_HPSS_MAX_DB / 20) or not finite: NAE_ERR_INVALID; n_fft other than 512, 1024, 2048, 4096: NAE_ERR_UNSUPPORTED; in_len = 0 or
 * n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as K9's. */
typedef struct nae_hpss_params {
    int n_fft;              /* 512, 1024, 2048 or 4096 */
    int time_span;          /* Tn: frames to either side of the harmonic median, 0 ... NAE_HPSS_MAX_SPAN */
    int freq_span;          /* Fn: bins to either side of the percussive median, 0 ... NAE_HPSS_MAX_SPAN */
    int hard;               /* 1: the binary mask; 0: the soft one */
    float gain_h;           /* gain of a bin that is all harmonic (m = 1) */
    float gain_p;           /* gain of a bin that is all percussive (m = 0) */
} nae_hpss_params;
/* The parameters on the host, in double: a level at or below NAE_HPSS_MIN_DB is gain 0, else gain = (float)10^(dB / 20).  NAE_ERR_INVALID: a
 * null pointer, a level that is not finite or outside NAE_HPSS_MIN_DB ... NAE_HPSS_MAX_DB, a span outside 0 ... NAE_HPSS_MAX_SPAN, hard not
 * 0 or 1; NAE_ERR_UNSUPPORTED: n_fft other than 512 ... 4096.  No context, no device work. */
int nae_hpss_design(double harmonic_db, double percussive_db, int n_fft, int time_span, int freq_span, int hard, nae_hpss_params* out);
int nae_hpss_block_f32(nae_ctx* ctx, const nae_hpss_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                       const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch).  With H = n_fft / 4, after every put floor((put total - (time_span + 3) H) / H) H
 * frames have become available in all, never fewer than zero; nae_hpss_flush releases the rest, so in_len frames come out in all, equal to
 * the block call's however the input is cut.  A put after the flush: NAE_ERR_STATE. */
int nae_hpss_create(nae_ctx* ctx, const nae_hpss_params* params, int channels, nae_hpss** h);
int nae_hpss_put(nae_hpss* h, const float* interleaved, size_t S);
int nae_hpss_put_host(nae_hpss* h, const float* interleaved_host, size_t S);
int nae_hpss_flush(nae_hpss* h);
size_t nae_hpss_available(nae_hpss* h);
int nae_hpss_receive(nae_hpss* h, float* dst, size_t max_frames, size_t* got);
int nae_hpss_receive_host(nae_hpss* h, float* dst_host, size_t max_frames, size_t* got);
int nae_hpss_destroy(nae_hpss* h);

/* ------------------------------------------------------------------ K22 limiter (true-peak look-ahead brickwall)
 * no reference code.  Spec ("K22 limiter"): one detector per stream-channel, or with link = 1 on a stereo stream one per stream.
 * Every step is one IEEE operation in the order written, the output rounded once to f32.  K = 20 log10(2), KINV = 1 / K, dyn_log2 and
 * dyn_exp2 are K12's; every maximum of f32 is a > m ? a : m.  Per detector, x zero outside [0, in_len), la = lookahead:
 *   level       a_c[n] = |x_c[n]|.  true_peak = 1: v_p[m] = K14's phase p at m (the same taps, tap 0 times x[m] first), e_c[m] the largest
 *               |v_p[m]| over p = 0 ... 3 from 0.0f on, L_c[n] = max(a_c[n], e_c[n + 5], e_c[n + 6]) in that order, D = 6; true_peak = 0:
 *               L_c = a_c, D = 0.  Linked: L = L_1 > L_0 ? L_1 : L_0
 *   demand      xg = K dyn_log2((double)L), a zero L at NAE_DYN_FLOOR_DB; u = (xg + gain_db) - ceiling_db; r[n] = u > 0 ? u : 0
 *   look-ahead  d[n] = max(r[n] ... r[n + la])
 *   release     y1[n] = max(d[n], (alpha_release y1[n - 1]) + (omr d[n])), omr = 1 - alpha_release made once, y1[-1] = 0, in K12's tiled
 *               form (NAE_DYN_LANE samples per lane, chunks of NAE_DYN_CHUNK from the stream's sample 0, six Kogge-Stone steps)
 *   attack      q[n] = (int64) ceil(y1[n] 2^24), 0 where that is not finite; q[n] = q[0] for n < 0; W[n] = q[n - la] + ... + q[n] in
 *               integers; s[n] = (double)W[n] / (double)((la + 1) 2^24)
 *   gain        g[n] = dyn_exp2((gain_db - s[n]) KINV); out_c[n] = (float)((double)x_c[n] g[n]) for each channel of the detector
 * The call is compensated as K12 is: output n is input n under a gain that has seen la + D samples ahead; in_len frames come out and
 * nothing past in_len is stored.  s[n] >= r[n], so |out[n]| <= 10^(ceiling_db / 20) (1 + 2^-22) for any input, release and look-ahead; the
 * gain starts at its reduced value (no ramp at sample 0); any cut into puts gives the block call's bits; a non-finite sample i leaves every
 * output before i - la - D as it was, and the call returns NAE_OK.  Bit-exact against the CPU statement (tests/lim_ref/ref_lim.c).
 * Errors: a null pointer, ch not 1 or 2, a field that is not finite or outside its range (ceiling_db -20 ... 0; gain_db -24 ... 24;
 * alpha_release in [0, 1); lookahead not negative; true_peak and link 0 or 1): NAE_ERR_INVALID; a lookahead above NAE_LIM_MAX_LOOKAHEAD:
 * NAE_ERR_UNSUPPORTED; in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as nae_dyn_block_f32's:
 * stream_stride 0 on the source and dst->base == src->base are allowed. */
typedef struct nae_lim_params {
    double ceiling_db;           /* no output sample lies above it */
    double gain_db;              /* the drive in front of the limiter */
    double alpha_release;
    int lookahead;               /* samples: the length of the attack's box less one */
    int true_peak;               /* 1: the detector hears K14's 4x oversampled signal */
    int link;                    /* 1: one detector per stereo stream */
} nae_lim_params;
int nae_lim_block_f32(nae_ctx* ctx, const nae_lim_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                      const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): before the flush floor((put - lookahead - D) / NAE_DYN_CHUNK) whole chunks are
 * available, never negative; nae_lim_flush releases the rest, so in_len frames come out in all, equal to the block call's however the input
 * is cut.  A put after the flush: NAE_ERR_STATE. */
int nae_lim_create(nae_ctx* ctx, const nae_lim_params* params, int channels, nae_lim** h);
int nae_lim_put(nae_lim* h, const float* interleaved, size_t S);
int nae_lim_put_host(nae_lim* h, const float* interleaved_host, size_t S);
int nae_lim_flush(nae_lim* h);
size_t nae_lim_available(nae_lim* h);
int nae_lim_receive(nae_lim* h, float* dst, size_t max_frames, size_t* got);
int nae_lim_receive_host(nae_lim* h, float* dst_host, size_t max_frames, size_t* got);
int nae_lim_destroy(nae_lim* h);
/* The record on the host, in double: alpha_release = exp(-1 / (release_s sample_rate)); lookahead = lround(lookahead_s sample_rate).
 * Ranges: ceiling_db -20 ... 0, gain_db -24 ... 24, release_s 0.001 ... 5, lookahead_s not negative, true_peak and link 0 or 1.
 * NAE_ERR_INVALID: a null pointer, sample_rate <= 0, an argument that is not finite or outside its range; NAE_ERR_UNSUPPORTED: a look-ahead
 * above NAE_LIM_MAX_LOOKAHEAD samples at that rate.  No context, no device work. */
int nae_lim_design(int sample_rate, double ceiling_db, double gain_db, double release_s, double lookahead_s, int true_peak, int link,
                   nae_lim_params* out);

/* ------------------------------------------------------------------ K23 dither (word-length reduction: TPDF dither, noise-shaped requantisation)
 * no reference code.  Spec ("K23 dither"): the f32 output lies on the grid of a `bits`-bit word, b = bits, S = 2^(b - 1).  Per
 * stream-channel, sample index n >= 0, all in double; "fused" is one fma with one rounding, every other step one IEEE operation:
 *   t[n] = (double)x[n] S                          one multiply, exact; a sample that is not finite counts as x[n] = 0
 *   u[n] = t[n] - sum c_k e[n - k]                  K fused steps u = fma(-c_k, e[n - k], u) from k = K down to k = 1; e[m] = 0 for m < 0
 *   q[n] = rint(u[n] + d[n])                        one add, one round to nearest, ties to even
 *   e[n] = q[n] - u[n]                              one subtract: the dithered quantiser's whole error, taken before the clamp
 *   y[n] = (float)(clamp(q[n], -S, S - 1) / S)      exact
 * so y - x = (e * ntf) / S with NTF(z) = 1 - sum c_k z^-k.  Dither d[n] in LSB, a function of (seed, stream index in the call, channel, n):
 * fin(z) is the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31), G =
 * 0x9E3779B97F4A7C15, all modulo 2^64; key = fin(fin(fin(seed + G) + stream) + channel); h[n] = fin(key + G n); r1[n] = (int32)(h >> 32) 2^-32,
 * r2[n] = (int32)(h & 0xffffffff) 2^-32.  kind NAE_DITHER_NONE: d = 0; _RECTANGULAR: d = r1; _TRIANGULAR: d = r1 + r2; _HIGHPASS: d[n] = r1[n] -
 * r1[n - 1], r1[-1] = 0.  A source with stream_stride 0 still gives every stream its own dither.  y S is an integer in [-S, S - 1]: any later
 * conversion to an integer format of at least `bits` bits reproduces it exactly; integer output planes are not part of this entry.  The
 * presets' curves are fixed in z: the `lipshitz` taps were designed for 44.1 kHz, and their curve moves with the sample rate.
 * Bit-exact against the CPU statement (tests/dither_ref/ref_dither.c) under either value of the debug key dither_roles and any cut of the
 * input into puts.  Errors: a null pointer, ch not 1 or 2, bits outside 8 ... 24, an unknown kind, n_taps outside 0 ... 12, a tap that is
 * not finite, sum |c_k| above 64: NAE_ERR_INVALID; in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as
 * nae_dyn_block_f32's: stream_stride 0 on the source and dst->base == src->base are allowed. */
typedef struct nae_dither_params {
    int bits;                    /* word length, 8 ... 24 */
    int kind;                    /* NAE_DITHER_NONE, _RECTANGULAR, _TRIANGULAR, _HIGHPASS (include/nae_dsp_spec.h) */
    int n_taps;                  /* K, 0 ... 12 */
    double taps[12];             /* c_1 ... c_K of NTF(z) = 1 - sum c_k z^-k */
    unsigned long long seed;
} nae_dither_params;
int nae_dither_block_f32(nae_ctx* ctx, const nae_dither_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                         const nae_sig* dst);
/* Streaming handle on the shared device FIFO (channels = ch): no latency, every frame put is available after that put.  The handle is stream
 * 0 of its call; the K errors per channel and the position n stay on the device and in the handle between launches, so any cut of the
 * input gives the block call's bits for one stream.  A put after the flush: NAE_ERR_STATE. */
int nae_dither_create(nae_ctx* ctx, const nae_dither_params* params, int channels, nae_dither** h);
int nae_dither_put(nae_dither* h, const float* interleaved, size_t S);
int nae_dither_put_host(nae_dither* h, const float* interleaved_host, size_t S);
int nae_dither_flush(nae_dither* h);
size_t nae_dither_available(nae_dither* h);
int nae_dither_receive(nae_dither* h, float* dst, size_t max_frames, size_t* got);
int nae_dither_receive_host(nae_dither* h, float* dst_host, size_t max_frames, size_t* got);
int nae_dither_destroy(nae_dither* h);
/* The record on the host: shaping NAE_DITHER_SHAPE_NONE (no taps), _FIRST {1}, _SECOND {2, -1}, _LIPSHITZ {2.033, -2.165, 1.959, -1.590,
 * 0.6149}.  NAE_ERR_INVALID: a null pointer, bits outside 8 ... 24, an unknown kind or preset.  No context, no device work. */
int nae_dither_design(int bits, int kind, int shaping, unsigned long long seed, nae_dither_params* out);

/* ------------------------------------------------------------------ K14 loudness
 * no reference code.  Spec ("K14 loudness"): the programme loudness of ITU-R BS.1770-4 / EBU R 128 with the true peak, and the one
 * gain that brings a stream to a target loudness under a true-peak ceiling.  ch is 1 or 2, every channel weight is 1.  Per channel the f32
 * samples run through the K-weighting, two biquads in double in K11's tiled form (chunks of NAE_EQ_CHUNK samples from sample 0, 64 lanes of
 * NAE_EQ_LANE samples, K11's tables; the signal w stays a double).  With B = sample_rate / 10 (100 ms) the energy E_c[u] of sub-block u is the
 * sum of w w over [u B, (u + 1) B), for the U = floor(in_len / B) complete sub-blocks, in a fixed order: per chunk every lane adds its own
 * samples of the sub-block in index order from 0.0, the 64 lane sums are added by a butterfly over the distances 32, 16, 8, 4, 2, 1, and the
 * chunk's sum is added to E_c[u] in chunk order.  Gating block j = 0 ... U - 4 (400 ms, 75 % overlap) has
 * z_c[j] = ((E[j] + E[j + 1]) + (E[j + 2] + E[j + 3])) / (4 B) and p[j] = z_0[j] (+ z_1[j]).  mean1 is the mean of the p[j] > gate_abs, summed
 * in block order; mean2 the mean of the p[j] with p > gate_abs and p > 0.1 mean1.  No block past the gates: mean2 = 0, the stream "has no
 * loudness" and its gain is 1.  The true peak of a channel, in f32: max |v_p[n]| over the four phases p and n = 0 ... in_len + 10 of
 * v_p[n] = sum over k = 0 ... 11, in this order, of t_p[k] x[n - k] (x zero outside the signal; the taps: nae_dsp_spec.h, NAE_LOUD_TP_*).
 * gain = sqrt(target / mean2); with P the largest of the channels' true and sample peaks and gain P > ceiling_lin it is ceiling_lin / P; it is
 * at most max_gain_lin; gain_f32 = (float)gain, and normalizing is y = x gain_f32, one f32 product.  Bit-exact against the CPU statement
 * (tests/loud_ref/ref_loud.c): every field of the record and every output sample.  A non-finite input sample does not fault; the record of
 * its stream is then unspecified.
 * Errors: a null pointer, ch not 1 or 2, a record nae_loud_design did not make (coefficients not finite or not strictly stable, sub_block not
 * sample_rate / 10, a level that is not positive and finite): NAE_ERR_INVALID; a sample rate outside the rate rule: NAE_ERR_UNSUPPORTED;
 * in_len = 0 or n_streams = 0: NAE_OK after the checks, nothing is launched.  Views as K11's.  All three entries are asynchronous on the
 * context's stream; the sub-block energies live in a workspace of the context (8 bytes per stream-channel and 100 ms). */
typedef struct nae_loud_params {
    int sample_rate;        /* 8000 ... 192000, a multiple of 10 */
    int sub_block;          /* B = sample_rate / 10 */
    double coef[10];        /* the K-weighting: shelf, high-pass, each (b0, b1, b2, a1, a2) */
    double gate_abs;        /* 10^((-70 + 0.691) / 10): the absolute gate as an energy */
    double target;          /* 10^((target_lufs + 0.691) / 10) */
    double ceiling_lin;     /* 10^(ceiling_dbtp / 20) */
    double max_gain_lin;    /* 10^(max_gain_db / 20) */
} nae_loud_params;
typedef struct nae_loud_result {
    double mean2;           /* gated mean energy; 0: the stream has no loudness.  LUFS = nae_loud_lufs(mean2) */
    double momentary_max;   /* the largest p[j]; 0 without a block */
    double gain;
    float gain_f32;
    float true_peak[2];     /* per channel, linear; [1] is 0 with one channel */
    float sample_peak[2];
    unsigned blocks_total, blocks_abs, blocks_rel;   /* gating blocks, those past the absolute gate, those past both gates */
} nae_loud_result;
/* The parameters on the host.  The K-weighting from its analog prototypes by the bilinear form, K = tan(pi f0 / sample_rate): the shelf
 * f0 = NAE_LOUD_SHELF_F0, Vh = 10^(NAE_LOUD_SHELF_GAIN_DB / 20), Vb = Vh^NAE_LOUD_SHELF_VB_EXP, Q = NAE_LOUD_SHELF_Q:
 * a0 = 1 + K / Q + K K, b = (Vh + Vb K / Q + K K, 2 (K K - Vh), Vh - Vb K / Q + K K) / a0, a = (2 (K K - 1), 1 - K / Q + K K) / a0; the high-pass
 * f0 = NAE_LOUD_HP_F0, Q = NAE_LOUD_HP_Q: b = (1, -2, 1), a as the shelf's.  At 48 kHz this is BS.1770's table to better than 1e-13.
 * NAE_ERR_INVALID: a null pointer, an argument that is not finite, target_lufs outside -70 ... -5, ceiling_dbtp outside -20 ... 0, max_gain_db
 * outside 0 ... 40; NAE_ERR_UNSUPPORTED: sample_rate outside 8000 ... 192000 or not a multiple of 10.  No context, no device work. */
int nae_loud_design(int sample_rate, double target_lufs, double ceiling_dbtp, double max_gain_db, nae_loud_params* out);
/* -0.691 + 10 log10(energy): the loudness of a mean energy (mean2, momentary_max) in LUFS; -infinity for 0.  Host only. */
double nae_loud_lufs(double energy);
/* results_dev: device memory, one nae_loud_result per stream */
int nae_loud_measure_f32(nae_ctx* ctx, const nae_loud_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                         nae_loud_result* results_dev);
/* y = x results_dev[stream].gain_f32 */
int nae_loud_apply_f32(nae_ctx* ctx, const nae_loud_result* results_dev, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                       const nae_sig* dst);
/* measure, then apply; results_dev may be null (the records then stay in the context's workspace); dst may be src */
int nae_loud_normalize_f32(nae_ctx* ctx, const nae_loud_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                           const nae_sig* dst, nae_loud_result* results_dev);
/* Measuring handle on the shared device FIFO (channels = ch): whole chunks are measured as they fill and leave the FIFO, the sub-block
 * energies grow on the device; nae_loud_flush measures the rest and runs the gates; nae_loud_get_result then copies the record to the host
 * (it waits for the stream).  The record equals the block call's however the input is cut.  nae_loud_get_result before the flush, or a put
 * after it: NAE_ERR_STATE. */
int nae_loud_create(nae_ctx* ctx, const nae_loud_params* params, int channels, nae_loud** h);
int nae_loud_put(nae_loud* h, const float* interleaved, size_t S);
int nae_loud_put_host(nae_loud* h, const float* interleaved_host, size_t S);
int nae_loud_flush(nae_loud* h);
int nae_loud_get_result(nae_loud* h, nae_loud_result* out_host);
int nae_loud_destroy(nae_loud* h);

/* ------------------------------------------------------------------ the 4-node graph of BASELINE.json
 * input -> mix(2) -> pitch -> FFT spectrum, one launch sequence over n_streams independent streams.
 * Each node still materialises its output in HBM (the plugin contract: one Audio_stream per link,
 * src/infra/runner.cpp:35-50), so the intermediate buffers are caller-provided. */
typedef struct nae_graph4 {
    nae_sig in_a, in_b;       /* two mix inputs, interleaved stereo f32; in_b.stream_stride may be 0 (shared) */
    float vol_a, vol_b;
    nae_sig mix_out;          /* planar stereo (the amix node emits FLTP, audio-amix.cpp:198)                 */
    double rate, pitch;       /* pitch node parameters                                                         */
    nae_sig pitch_out;        /* interleaved stereo (construct_audio_frame_float emits FLT, audio-velocity.cpp:247) */
    float* spec_out;          /* [n_streams][frames][2][513]                                                  */
    size_t spec_stream_stride;
    size_t S;                 /* sample-frames per stream                                                      */
    size_t n_streams;
} nae_graph4;
int nae_graph4_run(nae_ctx* ctx, const nae_graph4* g);
/* the same graph, only the stages selected by `mask`: 1 = mix node (+ the pitch node's transposer when it runs first),
 * 2 = the rest of the pitch node, 4 = spectrum node.  Scheduling experiments and tests; 7 == nae_graph4_run on one stream. */
int nae_debug_graph4_stages(nae_ctx* ctx, const nae_graph4* g, int mask);

#ifdef __cplusplus
}
#endif
#endif
