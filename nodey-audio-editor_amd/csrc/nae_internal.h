// nae_internal.h — shared between the translation units of libnae_gpu.so (not installed)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <memory>
#include <vector>
#include "../../include/nae_gpu.h"
#include "../../include/nae_dsp_spec.h"

#include "ctx_mem.h"

namespace nae { struct cf; }
struct nae_wsola_cache;
void nae_wsola_cache_free(nae_wsola_cache* c);   // nae_wsola.hip: the one release hook of the incomplete type (its members free themselves)
struct nae_wsola_cache_deleter { void operator()(nae_wsola_cache* c) const { nae_wsola_cache_free(c); } };

struct nae_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    char err[512] = {0};
    char name[256] = {0};
    int n_cu = 256;              // compute units of the device (launch-shape decisions)
    // The context's device memory is CtxBuf and CtxConst members (ctx_mem.h) and nothing else: each frees itself when the context goes, so
    // nae_ctx_destroy lists no node, and a node that adds memory adds a member.
    // read-only FFT tables of n_fft = 256 ... 4096, slot log2 n_fft - 8 (built on the host in double, rounded once to f32): 1024's
    // with the context, the others on first use (nae_fft_tab_ensure; the layout of a slot: nae_fft_tab_of below)
    CtxBuf fft_tab[5];
    CtxBuf spec_ctr;             // work counter of the persistent stereo spectrum kernel (zeroed on the stream in front of every drawing launch; kernels_spectrum.hip)
    CtxBuf ws_phase;             // the vocoder's phase records (nae_pv_reserve_ws; the stretch handle's segments run on it too)
    CtxBuf ws_mid;               // the signal between the transposer and the vocoder
    CtxConst rs_tab;             // the transposer's coefficient table, keyed by rate_eff (nae_ensure_rs_table)
    std::unique_ptr<nae_wsola_cache, nae_wsola_cache_deleter> wsola_cache;   // plan + workspaces of nae_wsola_block_f32 (nae_wsola.hip)
    int pv_tile = 0;             // frames per phase-vocoder tile; 0 = choose per call (nae_pick_pv_shape)
    int pv_fps = 0;              // pv_fps = 1|2|4: frames per step of the vocoder pipeline (0 = choose per call)
    int fir_tile = 0;            // blocks per tile of the FIR filter; 0 = choose per launch (nae_pick_fir_tile)
    CtxConst fir_spec;           // nae_fir_block_f32's [padded taps | H] of the last call's n_fft and taps (kernels_fir.hip)
    int conv_tile = 0;           // blocks per wave of the long convolution's accumulate kernel; 0 = nae_pick_conv_tile
    int conv_ring = 0;           // spectrum slots per stream-channel of its workspace ring; 0 = from NAE_CONV_WS_BYTES (nae_pick_conv_ring)
    CtxConst conv_spec;          // nae_conv_block_f32's spectra of the last call's n_fft, taps_ch and taps, apart from the FIR filter's (kernels_conv.hip)
    CtxBuf ws_conv;              // the ring of its launches
    int dn_tile = 0;             // hop blocks per tile of the spectral gate; 0 = choose per launch (nae_pick_denoise_tile)
    int hpss_tile = 0;           // hop blocks per tile of the separation; 0 = choose per launch (nae_pick_hpss_tile)
    CtxConst eq_block;           // the constant block of the last call's sections: the EQ, echo and keyed-dynamics block calls (nae_eq_cached_block)
    CtxConst loud_block;         // the loudness entries' constant block of the last call's K-weighting (kernels_loud.hip)
    CtxBuf ws_loud;              // their workspace: states, sub-block energies, records
    CtxBuf ws_echo;              // nae_echo_block_f32's delay lines, one ring per stream-channel of a launch group (kernels_echo.hip)
    int dither_roles = 0;        // who does the dither's feed-forward work: 0 / 1 the producer waves, 2 the walking wave (kernels_dither.hip)
    int echo_group = 0;          // streams per launch of the echo's block call; 0 = from NAE_CONV_WS_BYTES
    int mod_sub = 0;             // samples a wave of the modulated delay computes in parallel, 1 ... 64; 0 = the rule of kernels_mod.hip
    int sat_tile = 0;            // chunks per wave of the saturation; 0 = choose per launch (nae_pick_sat_tile)
    CtxBuf ws_mb;                // nae_mb_block_f32's carries and band planes of a launch group and slab (kernels_mb.hip)
    int mb_group = 0;            // streams per launch group of the multiband compressor's block call; 0 = from NAE_CONV_WS_BYTES
    int mb_slab = 0;             // chunks per slab of its three kernels; 0 = from NAE_CONV_WS_BYTES (a handle: 64)
    // the saturation keeps the device taps of every oversampling factor it has run (kernels_sat.hip): three slots [hd | hu], bit i of sat_taps_have:
    // slot i is there.  No last-call constant: a slot never changes once uploaded
    CtxBuf sat_taps; unsigned sat_taps_have = 0;
    // tuning / A-B switches: nae_debug_set(ctx, key, value) (include/nae_gpu.h lists the keys; NAE_DEBUG="key=value,..." applies them at context creation)
    bool dbg_st_unfused = false;     // st_unfused: WSOLA chain runs filter and cubic stage as separate launches
    int dbg_td_nc = 0;               // td_nc = 1|2|4: candidates per thread of the WSOLA search (0: by batch size)
    bool dbg_no_mix_fuse = false;    // no_mix_fuse: graph4 runs mix and transposer as separate launches
    bool dbg_rs_single = false;      // rs_single: one stream per transposer workgroup (no coefficient sharing)
    bool dbg_rs_direct = false;      // rs_direct: direct (unstaged) transposer kernel
    bool dbg_spec_generic = false;   // spec_generic: skip the interleaved-stereo spectrum fast path
    bool dbg_spec_narrow = false;    // spec_narrow: the stereo spectrum kernel stores dword pieces (round 1-4 form) instead of 16-byte ones
    int dbg_spec_fine = 0, dbg_spec_fine_rounds = 0;   // spec_fine / spec_fine_rounds: frames of the short chunks at the end of a large launch's list / how many of them per resident wave
    int dbg_spec_chunk = 0;          // spec_chunk: frames one wave of the stereo spectrum kernel walks (0: spec_pick_chunk)
    bool dbg_spec_any = false;       // spec_any: 1024-point spectrum launches run the size-generic kernel (kernels_spectrum.hip)
    bool dbg_pv_any = false;         // pv_any: unlocked 1024-point vocoder launches run the size-generic kernels (kernels_pv_any.hip)
    int dbg_pv_min_ptile = 0;        // pv_min_ptile: shortest pass-1 tile in frames (0: 16)
    int pv_flow = 1;                 // pv_flow = 0|1|2: launches of at most one workgroup per CU run the one-barrier schedule (pv_flow_kernel) never / with one
                                     // frame per step (default: where it is faster, profiles/r05_flow.md) / in every shape
    bool pv_lean = false;            // pv_lean: the vocoder pipeline keeps its 64-VGPR shape even when one workgroup per CU would allow
                                     // 128 (leaves half of the register file and 94 KB of LDS to a co-resident kernel: tools/coresidency.py)
    // per-context, per-device launch state (a kernel attribute is set once per device: the record lives with the context's device)
    std::vector<const void*> lds_attr_done;   // the kernels (pv_pipe_kernel / pv_flow_kernel / pvlock_* instantiations, by address) whose
                                              // dynamic-LDS attribute has been set through this context (nae_pv_lds_attr, launch.h)
    // optional per-kernel timing (hipEvent pairs on the ctx stream), used by bench.py for the roofline line
    bool prof_on = false;
    struct ProfSlot { const char* name; double total_ms; uint64_t launches; };
    struct ProfPair { int slot; hipEvent_t a, b; };
    std::vector<ProfSlot> prof_slots;
    std::vector<ProfPair> prof_pairs;
};

// RAII: brackets one kernel launch with two events when profiling is on
struct NaeProfScope {
    nae_ctx* ctx; int idx;
    NaeProfScope(nae_ctx* c, const char* name);
    ~NaeProfScope();
};

// Several devices in one process: a context remembers its device and every entry point that allocates, launches or records
// selects it when the calling thread's current device differs (one hipGetDevice on the fast path).  The thread's current device is
// left on the context's.
static inline int nae_use_device(nae_ctx* ctx)
{
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == ctx->device) return 0;
    return hipSetDevice(ctx->device) == hipSuccess ? 0 : -3 /* NAE_ERR_HIP */;
}

#define NAE_KLAUNCH(ctx, name_str, ...)          \
    do {                                          \
        (void)nae_use_device(ctx);                \
        NaeProfScope nae_ps_(ctx, name_str);      \
        hipLaunchKernelGGL(__VA_ARGS__);          \
    } while (0)

struct nae_event { hipEvent_t ev; };

int nae_check(nae_ctx* ctx, hipError_t e, const char* what);
int nae_fail(nae_ctx* ctx, int code, const char* what);
// the nae_*_check functions' failure: ctx may be null (a caller that wants the code alone), no message then
inline int nae_fail_opt(nae_ctx* ctx, int code, const char* what) { return ctx ? nae_fail(ctx, code, what) : code; }

// kernels_spectrum.hip: the tables of size n_fft in ctx->fft_tab, built at the size's first call.  A slot is one buffer, every table on a
// 256-byte boundary as an allocation of its own would be: Hann_N [N] floats | T_N[k] = exp(-2 pi i k / N), k = 0 ... M = N / 2 | W_M[k], k < M.
// Kernels may read T_N in 16-byte pieces: at every size its M + 1 entries are followed by 31 zero ones (1024 had 520 entries for its 513).
// W512, which every size reads, is the W_M of 1024.
int nae_fft_tab_ensure(nae_ctx* ctx, int n_fft);
struct nae_fft_tab { const float* hann; const nae::cf* tn; const nae::cf* wm; };
constexpr size_t nae_fft_tab_tn(int n_fft) { return (size_t)n_fft * sizeof(float); }                               // byte offsets
constexpr size_t nae_fft_tab_wm(int n_fft) { return nae_fft_tab_tn(n_fft) + (size_t)n_fft / 2 * 8 + 256; }
constexpr size_t nae_fft_tab_bytes(int n_fft) { return nae_fft_tab_wm(n_fft) + (size_t)n_fft / 2 * 8; }
inline nae_fft_tab nae_fft_tab_of(const nae_ctx* ctx, int n_fft)
{
    const char* p = ctx->fft_tab[__builtin_ctz((unsigned)n_fft) - 8].as<char>();
    return nae_fft_tab{reinterpret_cast<const float*>(p), reinterpret_cast<const nae::cf*>(p + nae_fft_tab_tn(n_fft)),
                       reinterpret_cast<const nae::cf*>(p + nae_fft_tab_wm(n_fft))};
}

// kernels_spectrum.hip: every supported size and hop (arguments checked by the caller); picks the kernel
int nae_launch_spectrum(nae_ctx* ctx, int n_fft, int hop, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                        size_t dst_stream_stride);
// the one statement of the spectrum's parameter rules (nae_spectrum_frames_ex, nae_spectrum_block_ex_f32, nae_spectrum_create):
// n_fft a power of two in [256, 4096], else NAE_ERR_UNSUPPORTED; 1 <= hop <= n_fft, else NAE_ERR_INVALID
inline int nae_spectrum_check(int n_fft, int hop)
{
    if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)) != 0) return NAE_ERR_UNSUPPORTED;
    if (hop < 1 || hop > n_fft) return NAE_ERR_INVALID;
    return NAE_OK;
}
// the frame sizes of the vocoder, the FIR filter and the long convolution (each caller has its own error text)
inline bool nae_size_ok(int n_fft) { return n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096; }
// nae_api.hip: the modified Bessel function I0 of the Kaiser windows (the transposer's table, nae_fir_design), by its power series
double nae_bessel_i0(double x);
// nae_api.hip: the one tile rule of the launches that walk one tile per wave (the vocoder's pass 3 off the pipeline; the FIR filter and the long
// convolution's spectra).  `forced` > 0 is the tile.  Else `units` frames or blocks of n_sc stream-channels are cut for one round of the
// `resident` waves a CU holds where the stream-channels alone do not give them, into tiles of at least min_tile units: at most
// ceil(units / min_tile) tiles, or with max_tiles_down floor(units / min_tile) — the FIR filter's, 41 blocks are 5 tiles of 9, not 6 of 7.
int nae_pick_tile(nae_ctx* ctx, int forced, size_t units, size_t n_sc, size_t resident, size_t min_tile, bool max_tiles_down);
// The block calls whose workspace holds `group` streams at a time (the long convolution's ring, the echo's lines): f(src, dst, n) on the views
// of streams [s0, s0 + n), group after group; the first non-zero return ends the call.
template <class F>
int nae_for_stream_groups(const nae_sig* src, const nae_sig* dst, size_t n_streams, size_t group, const F& f)
{
    for (size_t s0 = 0; s0 < n_streams; s0 += group) {
        nae_sig gs = *src, gd = *dst;
        gs.base = static_cast<float*>(src->base) + s0 * src->stream_stride;
        gd.base = static_cast<float*>(dst->base) + s0 * dst->stream_stride;
        const int rc = f(gs, gd, s0 + group < n_streams ? group : n_streams - s0);
        if (rc) return rc;
    }
    return NAE_OK;
}
// a continued stream processes frames / hop blocks [f_origin, f_origin + f_count) per call
struct nae_pv_segment {
    long long f_origin, f_count;
    long long f_limit;            // frames >= f_limit are not available yet (or do not exist)
    long long mid_limit;          // stretched samples >= mid_limit are not stored
    const uint32_t* carry_in;     // [n_streams*ch][520] phase behind frame f_origin-1 (null: zero)
    uint32_t* carry_out;          // receives the phase behind frame f_origin+f_count-1 (null: not wanted)
    bool carry_by_synth = false;  // the segment is synthesised as ONE tile and pass 3 itself writes carry_out (no pass 1)
};
// What an entry's caller asked of the vocoder: lock = NAE_STRETCH_PHASE_LOCK, transients = NAE_STRETCH_TRANSIENTS, link =
// NAE_STRETCH_LINK_CHANNELS, lifter 0 = no formant stage.
// shift: a _formant_shift entry, whose plan (nae_stretch_plan_make_shift) may force the vocoder stage on; it says more than formant_ratio != 1 (the
// _formant entries with a lifter and a rate-only change run the transposer alone, _formant_shift with ratio 1 the forced envelope stage).
struct nae_pv_opts {
    int n_fft = NAE_FFT_N, lifter = 0;
    bool lock = false, transients = false, shift = false;
    double formant_ratio = 1.0;
    bool link = false;
};
// nae_api.hip: the one statement of the entries' option rules, in this order: a null context NAE_ERR_INVALID (nothing touched); a flag outside
// `allowed` (the _ex entries NAE_STRETCH_PHASE_LOCK, the others kPvFlagsN) NAE_ERR_INVALID; a size outside 512 ... 4096, the lock
// at a size other than 1024, NAE_ERR_UNSUPPORTED; a lifter outside 0 ... n_fft / 4 NAE_ERR_INVALID.  formant_ratio given: a _formant_shift entry.
constexpr unsigned kPvFlagsN = NAE_STRETCH_PHASE_LOCK | NAE_STRETCH_TRANSIENTS | NAE_STRETCH_LINK_CHANNELS;   // the _n, _formant and _formant_shift entries
int nae_pv_opts_check(nae_ctx* ctx, unsigned flags, unsigned allowed, int n_fft, int lifter, const double* formant_ratio, nae_pv_opts* o);
// nae_api.hip: the plan of a call with these options (the _shift plan of the _formant_shift entries, else the _n plan); a failure leaves its text
int nae_pv_plan_make(nae_ctx* ctx, const nae_pv_opts& o, double rate, double pitch, size_t in_len, nae_stretch_plan* pl);
// the envelope stage runs on the vocoder's frames ("Formant shift") when the envelope's ratio rate_eff / formant_ratio is not 1.
// With formant_ratio = 1 (the _formant entries) that is a plan with both the vocoder and the transposer (rate_eff is snapped to 1 within 1e-6);
// the _formant_shift entries' plan (nae_stretch_plan_make_shift) has the vocoder stage forced on where the stage runs at tempo 1.
inline bool nae_formant_stage_on(double rate_eff, int lifter, double formant_ratio)
{
    const double r = rate_eff / formant_ratio - 1.0;
    return lifter > 0 && (r <= -1e-6 || r >= 1e-6);
}
inline int nae_formant_lifter_eff(const nae_stretch_plan& pl, int lifter, double formant_ratio)
{
    return pl.pv_on && nae_formant_stage_on(pl.rate_eff, lifter, formant_ratio) ? lifter : 0;
}
// the transposer ratio g of the gain rule: one rounding of rate_eff / formant_ratio (at formant_ratio = 1, (float)rate_eff)
inline float nae_formant_g(const nae_stretch_plan& pl, double formant_ratio) { return (float)(pl.rate_eff / formant_ratio); }
// a plan with the vocoder stage forced on at tempo 1 (nae_stretch_plan_make_shift): Qs = Qa in every frame, the stage is the envelope pass alone
inline bool nae_plan_forced(const nae_stretch_plan& pl) { return pl.pv_on && pl.tempo_eff == 1.0; }
// The options as a plan runs them: what the tile choice, the two pass launchers and a handle's priming read (nothing works them out again)
struct nae_pv_run {
    int n_fft; bool lock;
    int lifter;        // the effective lifter (nae_formant_lifter_eff): > 0 where pass 3 runs the envelope stage
    float g;           // its transposer ratio (nae_formant_g); 0 with the stage off
    bool forced;       // nae_plan_forced: the envelope pass alone — no pass 1, no scan, no phase workspace, nothing carried
    bool transients;   // the flag, with the stage on and not forced (a forced stage has Qs = Qa: nothing to reset)
    bool link;         // the channel link as it is effective ("Channel link", rule 4): the flag, two channels, the stage on and not
                       // forced, and the lock or transient preservation effective — else the call is the unflagged one
};
inline nae_pv_run nae_pv_resolve(const nae_pv_opts& o, const nae_stretch_plan& pl, int ch)
{
    const int lifter = nae_formant_lifter_eff(pl, o.lifter, o.formant_ratio);
    const bool forced = nae_plan_forced(pl);
    const bool stage = pl.pv_on && !forced;
    const bool transients = o.transients && stage;
    return {o.n_fft, o.lock, lifter, lifter > 0 ? nae_formant_g(pl, o.formant_ratio) : 0.0f, forced, transients,
            o.link && ch == 2 && stage && (o.lock || transients)};
}
// The kernels a vocoder call runs, for the tile choice of a block call, nae_launch_pv_phase and nae_launch_pv_synth:
//   pass 1  kShipped: pv_phase_kernel (1024 points); kAny: pv_any_phase_kernel<N> (kernels_pv_any.hip); kLock: pvlock_map_kernel and its scan;
//   pass 3  kShipped: the pipeline (kernels_pvpipe.hip);  kAny: pv_any_synth_kernel<N>;                   kLock: pvlock_synth_kernel.
// Locked calls (1024 only: nae_pv_opts_check) run the locked kernels; unlocked calls at other sizes, or under the debug key pv_any, the size-generic
// ones.  Pass 1 does not depend on the lifter.  Unlocked 1024-point calls with formant preservation (nae_pv_run::lifter > 0) run the shipped pass 1
// and the size-generic pass 3: the pipeline has no formant stage, and the two passes share the record layout.  Unlocked calls with transient
// preservation run the size-generic passes at every size, 1024 included: the shipped pass 1 and the pipeline have no onset detector; locked
// ones the transient instantiations of the locked kernels.  A linked call (nae_pv_run::link) runs the kLink instantiations of the same kernels: unlocked
// it routes to the size-generic passes at every size, as a transient call does.
//   kEnv (a forced plan, nae_plan_forced): pass 3 is pv_env_kernel<N> (kernels_pvenv.hip) — there is no pass 1 and no scan, and the lock and
//   transient preservation change nothing (Qs = Qa either way).
// Asked at each launch, not kept in nae_pv_run: the debug key may change during a handle's life.
enum class PvKernels { kShipped, kAny, kLock, kEnv };
struct nae_pv_route { PvKernels pass1, pass3; };
inline nae_pv_route nae_pv_route_of(const nae_ctx* ctx, const nae_pv_run& r)
{
    if (r.forced) return {PvKernels::kEnv, PvKernels::kEnv};
    if (r.lock) return {PvKernels::kLock, PvKernels::kLock};
    const PvKernels pass1 = r.n_fft != NAE_FFT_N || ctx->dbg_pv_any || r.transients || r.link ? PvKernels::kAny : PvKernels::kShipped;
    return {pass1, r.lifter > 0 ? PvKernels::kAny : pass1};
}
// kernels_stft.hip: the vocoder's passes on the kernels nae_pv_route_of says, and their phase workspace (nae_pv_reserve_ws: none for a forced plan)
size_t nae_pv_workspace_bytes(bool lock, int n_fft, size_t n_frames, int ch, size_t n_streams, int tile);
int nae_pv_reserve_ws(nae_ctx* ctx, const nae_pv_run& r, size_t n_frames, int ch, size_t n_streams, int tile);
int nae_launch_pv_phase(nae_ctx* ctx, const nae_pv_run& r, const nae_stretch_plan* pl, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                        int tile, int synth_tile, uint32_t* phase_ws, const nae_pv_segment* seg);
int nae_launch_pv_synth(nae_ctx* ctx, const nae_pv_run& r, const nae_stretch_plan* pl, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                        int tile, int phase_tile, uint32_t* phase_ws, const nae_sig* out, const nae_pv_segment* seg, int frames_per_step);
// kernels_pv_any.hip: the record length of a size (int32: N/2 + 1 padded to a multiple of 8), the
// pass-3 waves a CU holds on the kernels `pass3` (kAny: PvAny<N, formant, transients, link>::kResident3; kEnv: PvEnv<N>::kResident; kLock: 16)
size_t nae_pv_record_pad(int n_fft);
int nae_pv_resident(nae_ctx* ctx, const nae_pv_run& r, PvKernels pass3);
// kernels_resample.hip: the rate transposer alone (outputs [j_begin, j_end)), and with the two-input mix fused into its staging
int nae_launch_resample(nae_ctx* ctx, const nae_stretch_plan* pl, const nae_sig* src, size_t src_len, int ch,
                        size_t n_streams, const float* d_tab, const nae_sig* out, size_t j_begin, size_t j_end);
int nae_launch_mix_resample(nae_ctx* ctx, const nae_stretch_plan* pl, const nae_sig* a, const nae_sig* b, float va, float vb,
                            const nae_sig* mix_out, size_t S, size_t n_streams, const float* d_tab, const nae_sig* out);
int nae_ensure_rs_table(nae_ctx* ctx, double rate_eff);
int nae_pick_pv_shape(nae_ctx* ctx, size_t frames, size_t n_sc, int* phase_tile, int* frames_per_step);
constexpr int kPhasePad = 520; // int32 per (stream-channel, tile) record in the phase workspace

// kernels_fir.hip: the FIR filter ("K9 FIR filter").  nae_fir_check: the parameter rules of the block call and the handle (n_taps < 1
// or ch not 1 / 2 NAE_ERR_INVALID; a size other than 512 ... 4096 or more than n_fft / 2 + 1 taps NAE_ERR_UNSUPPORTED; *n_fft 0 becomes the pick).
// A spectrum buffer holds nae_fir_spec_floats(n_fft) floats: the taps zero-padded to n_fft, then H[0 ... n_fft / 2] (nae_fir_make_spec, which
// waits for the upload of the host taps).  nae_launch_fir runs blocks [b_origin, b_stop) of signals of in_len samples, absolutely indexed.
int nae_fir_check(nae_ctx* ctx, int n_taps, int ch, int* n_fft);
size_t nae_fir_spec_floats(int n_fft);
int nae_fir_make_spec(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, float* d_spec);
int nae_launch_fir(nae_ctx* ctx, int n_fft, const float* d_spec, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t b_origin, size_t b_stop);
int nae_pick_fir_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc);

// kernels_conv.hip: the long convolution ("K10 long convolution").  nae_conv_check: the parameter rules of the block call and the handle
// (n_taps < 1, ch not 1 / 2 or taps_ch not 1 / ch NAE_ERR_INVALID; more than NAE_CONV_MAX_TAPS taps, a size other than 512 ... 4096 or more than
// NAE_CONV_MAX_PARTS partitions NAE_ERR_UNSUPPORTED; *n_fft 0 becomes the pick).  A spectrum buffer holds nae_conv_spec_floats floats: the
// [taps_ch][parts n_fft / 2] padded taps, then H [taps_ch][parts][n_fft / 2 + 8] complex (nae_conv_make_spec, which waits for the upload).  A ring
// holds nae_conv_ring_floats floats: [stream-channel][ring][n_fft / 2 + 8] complex, block j in slot j mod ring.  nae_launch_conv runs blocks
// [b_origin, b_stop) of absolutely indexed signals in slabs of ring - (parts - 1) blocks and leaves the last spectra in the ring.
// The workspace of a block call is capped at NAE_CONV_WS_BYTES: 256 MiB is the chip's Infinity Cache, so a slab's spectra written by one kernel
// are still on the chip when the next reads them, and it holds slabs of NAE_CONV_MIN_SLAB blocks for 60 stereo streams at 4096 / 128 partitions;
// larger batches run in groups of streams.  A handle's ring has room for slabs of NAE_CONV_HANDLE_SLAB blocks.
constexpr size_t NAE_CONV_WS_BYTES = (size_t)256 << 20;
constexpr int NAE_CONV_MIN_SLAB = 8, NAE_CONV_HANDLE_SLAB = 64;
int nae_conv_check(nae_ctx* ctx, int n_taps, int taps_ch, int ch, int* n_fft);
int nae_conv_parts(int n_taps, int n_fft);
size_t nae_conv_spec_floats(int n_fft, int parts, int taps_ch);
size_t nae_conv_ring_floats(int n_fft, size_t n_sc, size_t ring);
int nae_conv_make_spec(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, float* d_spec);
int nae_launch_conv(nae_ctx* ctx, int n_fft, int parts, int taps_ch, const float* d_spec, float* d_ring, size_t ring, const nae_sig* src,
                    size_t in_len, int ch, size_t n_streams, const nae_sig* dst, size_t b_origin, size_t b_stop);
int nae_pick_conv_tile(nae_ctx* ctx, int n_fft);
size_t nae_pick_conv_ring(nae_ctx* ctx, int n_fft, int parts, size_t blocks, size_t n_sc);

// kernels_eq.hip: the biquad cascade ("K11 biquad cascade").  nae_eq_check: the parameter rules of the block call and the handle (a
// null pointer, n_sections < 1, ch not 1 / 2, a non-finite coefficient or a section that is not strictly stable NAE_ERR_INVALID; more than
// NAE_EQ_MAX_SECTIONS sections NAE_ERR_UNSUPPORTED).  A constant block holds nae_eq_block_doubles() doubles: the coefficients [16][5], then per
// section p[16], q[16] and the six state maps (nae_eq_make_block, which waits for the upload).  nae_launch_eq runs chunks [c_origin, c_stop) of
// absolutely indexed signals; d_state, [stream-channel][16][2] doubles, is the carry in front of c_origin and receives the one behind c_stop - 1
// (null: zero, and nothing kept).
size_t nae_eq_block_doubles();
int nae_eq_check(nae_ctx* ctx, const double* coef, int n_sections, int ch);
int nae_eq_make_block(nae_ctx* ctx, const double* coef, int n_sections, double* d_block);
int nae_launch_eq(nae_ctx* ctx, const double* d_block, int n_sections, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                  const nae_sig* dst, size_t c_origin, size_t c_stop, double* d_state);
// the context's own constant block, made of checked coefficients unless they are the last call's (nae_eq_block_f32 and nae_dynkey_block_f32)
int nae_eq_cached_block(nae_ctx* ctx, const double* coef_host, int n_sections, double** d_block);

// kernels_dyn.hip: the dynamics processor ("K12 dynamics").  nae_dyn_check: the parameter rules of the block call and the handle.
// nae_dyn_detectors: one per stream with `link` on stereo, else one per stream-channel.  nae_launch_dyn runs chunks [c_origin, c_stop) of
// absolutely indexed signals and reads up to `lookahead` samples behind them (zero from in_len on); d_state, [detector][2] doubles, holds the
// carries (y1, yl) in front of c_origin and receives the ones behind c_stop - 1 (null: zero, and nothing kept).
int nae_dyn_check(nae_ctx* ctx, const nae_dyn_params* p, int ch);
size_t nae_dyn_detectors(const nae_dyn_params* p, int ch, size_t n_streams);
int nae_launch_dyn(nae_ctx* ctx, const nae_dyn_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, double* d_state);

// kernels_dynkey.hip: the keyed dynamics ("K15 keyed dynamics").  nae_dynkey_check: K12's rules, then the key's (key_ch not 0, 1
// or ch, negative n_sections, a non-finite or not strictly stable section NAE_ERR_INVALID; more than NAE_DYNKEY_MAX_SECTIONS
// NAE_ERR_UNSUPPORTED).  nae_launch_dynkey is nae_launch_dyn under a key (`key` is not read with key_ch = 0: the signal is its own key);
// d_block: the key filter's K11 constant block (unused with no section); d_fstate, nae_dynkey_filter_doubles() doubles, holds the filter's
// carries in front of c_origin and receives the ones in front of c_stop, the chunk the next launch levels first (null: zero, nothing kept).
int nae_dynkey_check(nae_ctx* ctx, const nae_dynkey_params* p, int ch);
size_t nae_dynkey_filter_doubles(const nae_dynkey_params* p, int ch, size_t n_streams);
int nae_launch_dynkey(nae_ctx* ctx, const nae_dynkey_params* p, const double* d_block, const nae_sig* src, const nae_sig* key, size_t in_len, int ch,
                      size_t n_streams, const nae_sig* dst, size_t c_origin, size_t c_stop, double* d_state, double* d_fstate);

// kernels_echo.hip: the echo ("K16 echo").  nae_echo_check: the parameter rules of the block call and the handle.  nae_echo_ring: R, the
// samples of a stream-channel's delay line.  nae_launch_echo runs chunks [c_origin, c_stop) of absolutely indexed signals, one workgroup per
// stream: d_block is the sections' K11 constant block (unused with no section); d_line, n_streams x ch rings of R floats, holds every line's
// last R samples by absolute index mod R (never read in front of sample 0: nothing to clear); d_state, [stream-channel][NAE_ECHO_MAX_SECTIONS][2]
// doubles, is the sections' carry in front of c_origin and receives the one behind c_stop - 1 (null: zero, and nothing kept).
int nae_echo_check(nae_ctx* ctx, const nae_echo_params* p, int ch);
size_t nae_echo_ring(const nae_echo_params* p, int ch);
int nae_launch_echo(nae_ctx* ctx, const nae_echo_params* p, const double* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                    const nae_sig* dst, size_t c_origin, size_t c_stop, float* d_line, double* d_state);

// kernels_mod.hip: the modulated delay ("K17 modulated delay").  nae_mod_check: the parameter rules of the block call and the handle.
// nae_launch_mod runs chunks [c_origin, c_stop) of absolutely indexed signals, one wave per stream-channel: d_state, [stream-channel]
// [NAE_MOD_KEEP] floats, is every line's last NAE_MOD_KEEP samples in front of chunk c_origin and receives those in front of chunk c_stop
// (null: zero, and nothing kept: the block call, which starts at chunk 0).
constexpr size_t NAE_MOD_KEEP = 3072;
int nae_mod_check(nae_ctx* ctx, const nae_mod_params* p, int ch);
int nae_launch_mod(nae_ctx* ctx, const nae_mod_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, float* d_state);

// kernels_sat.hip: the saturation ("K18 saturation").  nae_sat_check: the parameter rules of the block call and the handle.
// nae_launch_sat runs chunks [c_origin, c_stop) of absolutely indexed signals of in_len samples, one wave per stream-channel and tile of
// nae_pick_sat_tile chunks: it reads from 64 samples in front of chunk c_origin on (zero below sample 0 and from in_len on) and keeps nothing
// between launches.
int nae_sat_check(nae_ctx* ctx, const nae_sat_params* p, int ch);
int nae_launch_sat(nae_ctx* ctx, const nae_sat_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop);
int nae_pick_sat_tile(nae_ctx* ctx, size_t chunks, size_t n_sc);

// kernels_gate.hip: the gate ("K19 gate").  nae_gate_check: the parameter rules of the block call and the handle.
// nae_gate_detectors: one per stream with `link` on stereo, else one per stream-channel.  nae_launch_gate runs chunks [c_origin, c_stop) of
// absolutely indexed signals of in_len samples; d_state, three 64-bit words per detector, holds the carries in front of chunk c_origin (the
// hysteresis state, the last set sample or -1, y's bits) and then the ones in front of chunk c_stop; null: the start of a stream, nothing kept.
int nae_gate_check(nae_ctx* ctx, const nae_gate_params* p, int ch);
size_t nae_gate_detectors(const nae_gate_params* p, int ch, size_t n_streams);
int nae_launch_gate(nae_ctx* ctx, const nae_gate_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                    size_t c_origin, size_t c_stop, long long* d_state);

// kernels_mb.hip: the multiband compressor ("K20 multiband").  nae_mb_check: the parameter rules of the block call and the handle.
// nae_mb_run runs chunks [c_origin, c_stop) of absolutely indexed signals of in_len samples in slabs of at most `slab` chunks: d_block is the
// tree's K11 constant block; d_planes, nae_mb_plane_floats() floats, holds a slab's band signals and the chunk behind it; d_state,
// nae_mb_state_doubles() doubles, holds the sections' carries [stream-channel][16][2] and then the detectors' [band][detector][2] in front of
// chunk c_origin (zero at the start of a stream) and receives the ones in front of chunk c_stop.  nae_mb_handle_slab: the slab of a handle.
int nae_mb_check(nae_ctx* ctx, const nae_mb_params* p, int ch);
size_t nae_mb_plane_floats(const nae_mb_params* p, int ch, size_t n_streams, size_t slab);
size_t nae_mb_state_doubles(const nae_mb_params* p, int ch, size_t n_streams);
size_t nae_mb_handle_slab(const nae_ctx* ctx);
int nae_mb_run(nae_ctx* ctx, const nae_mb_params* p, const double* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
               const nae_sig* dst, size_t c_origin, size_t c_stop, float* d_planes, size_t slab, double* d_state);

// kernels_denoise.hip: the spectral gate ("K13 spectral gate").  nae_denoise_check: the parameter rules of the block call and the
// handle.  nae_launch_denoise runs hop blocks [b_origin, b_stop) of absolutely indexed signals of in_len samples: it reads from
// (b_origin - time_smooth - 3) H on and, in front of a block, time_smooth + 3 blocks ahead (zero from in_len on), and keeps nothing between launches.
int nae_denoise_check(nae_ctx* ctx, const nae_denoise_params* p, const float* profile_dev, int profile_ch, int ch);
int nae_launch_denoise(nae_ctx* ctx, const nae_denoise_params* p, const float* d_profile, int profile_ch, const nae_sig* src, size_t in_len, int ch,
                       size_t n_streams, const nae_sig* dst, size_t b_origin, size_t b_stop);
int nae_pick_denoise_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc);

// kernels_hpss.hip: the harmonic/percussive separation ("K21 separation").  nae_hpss_check: the parameter rules of the block call
// and the handle.  nae_launch_hpss runs hop blocks [b_origin, b_stop) of absolutely indexed signals of in_len samples: it reads from
// (b_origin - time_span - 3) H on and, in front of a block, time_span + 3 blocks ahead (zero from in_len on), and keeps nothing between launches.
int nae_hpss_check(nae_ctx* ctx, const nae_hpss_params* p, int ch);
int nae_launch_hpss(nae_ctx* ctx, const nae_hpss_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                    size_t b_origin, size_t b_stop);
int nae_pick_hpss_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc);

// kernels_lim.hip: the limiter ("K22 limiter").  nae_lim_check: the parameter rules of the block call and the handle.
// nae_lim_detectors: one per stream with `link` on stereo, else one per stream-channel.  nae_lim_wait: lookahead + D, the samples behind a chunk
// its gain reads.  nae_launch_lim runs chunks [c_origin, c_stop) of absolutely indexed signals of in_len samples and reads from 16 samples in
// front of chunk c_origin on (zero below sample 0 and from in_len on); d_state, nae_lim_state_words() 64-bit words per detector, holds the
// carries in front of chunk c_origin (y1's bits, the running total of q, the prefix sums of chunk c_origin - 1) and then the ones in front of
// chunk c_stop; all zero or null: the start of a stream (null: nothing kept).
int nae_lim_check(nae_ctx* ctx, const nae_lim_params* p, int ch);
size_t nae_lim_detectors(const nae_lim_params* p, int ch, size_t n_streams);
size_t nae_lim_state_words();
size_t nae_lim_wait(const nae_lim_params* p);
int nae_launch_lim(nae_ctx* ctx, const nae_lim_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, unsigned long long* d_state);

// kernels_dither.hip: the dither ("K23 dither").  nae_dither_check: the parameter rules of the block call and the handle.
// nae_launch_dither computes frames [first, stop) of absolutely indexed signals, frame i being sample n = i of its stream; d_state,
// NAE_DITHER_MAX_TAPS doubles per stream-channel, holds the errors e[first - 1], e[first - 2], ... on entry and those in front of `stop` on
// return; null: the start of a stream (nothing kept).  Without taps it is not read.
int nae_dither_check(nae_ctx* ctx, const nae_dither_params* p, int ch);
int nae_launch_dither(nae_ctx* ctx, const nae_dither_params* p, const nae_sig* src, int ch, size_t n_streams, const nae_sig* dst, size_t first,
                      size_t stop, double* d_state);

// kernels_loud.hip: the loudness meter ("K14 loudness").  nae_loud_check: the parameter rules of the block entries and the handle.  A
// constant block holds nae_loud_block_bytes() bytes: K11's block of the two K-weighting sections, then the true-peak taps (nae_loud_make_block,
// which waits for the upload).  nae_launch_loud_measure runs chunks [c_origin, c_stop) of absolutely indexed signals: d_state, n_streams x ch
// records of nae_loud_state_bytes() bytes, is what a stream-channel carries (zero in front of sample 0) and holds the peaks behind c_stop - 1;
// d_E holds the sub-block energies, sub-block u of channel c of stream s at [s * e_ss + u * ch + c], zero before the first launch; sums of
// sub-blocks from n_sub on are dropped.  nae_loud_chunks: the chunks of in_len samples a handle has measured before its flush (the whole ones)
// and behind it (the true peak reaches 11 samples past the end).  nae_launch_loud_gate: the gates and the gain of signals of in_len samples.
size_t nae_loud_block_bytes();
size_t nae_loud_state_bytes();
int nae_loud_check(nae_ctx* ctx, const nae_loud_params* p, int ch);
int nae_loud_make_block(nae_ctx* ctx, const nae_loud_params* p, void* d_block);
size_t nae_loud_chunks(size_t in_len, bool flushed);
void nae_loud_taps(float* out);   // the 48 true-peak taps [phase][k] as f32: K14's, and K22's detector
int nae_launch_loud_measure(nae_ctx* ctx, const nae_loud_params* p, const void* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                            size_t c_origin, size_t c_stop, void* d_state, double* d_E, size_t e_ss, size_t n_sub);
int nae_launch_loud_gate(nae_ctx* ctx, const nae_loud_params* p, size_t in_len, int ch, size_t n_streams, const void* d_state, const double* d_E,
                         size_t e_ss, nae_loud_result* d_results);

// kernels_nodes.hip
int nae_launch_copy_sig(nae_ctx* ctx, const nae_sig* src, const nae_sig* dst, size_t S, int ch, size_t n_streams,
                        bool scale, float volume);
