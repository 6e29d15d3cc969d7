// stft_common.h — kernel-side types and vocoder launch helpers shared by the STFT translation units (kernels_stft.hip, kernels_pvpipe.hip,
// kernels_spectrum.hip, kernels_pvlock.hip) and the rate transposer (kernels_resample.hip).
#pragma once
#include "launch.h"
#include "stft_device.h"

namespace nae {

constexpr int kT1024Pad = kPhasePad;             // 513 split twiddles / phases, padded to 520

struct Tables { const cf* w512; const cf* t1024; const float* hann; };
// the context's own, built at its creation (nae_fft_tab_ensure): W512 is the W_M of the size
inline Tables tables_1024(const nae_ctx* ctx)
{
    const nae_fft_tab t = nae_fft_tab_of(ctx, NAE_FFT_N);
    return Tables{t.wm, t.tn, t.hann};
}
// the 1024-point kernels on the padded FFT (spectrum, vocoder pass 1): 8-wave workgroups that stage Hann, the split twiddles,
// W64 and the pass-A twiddles in LDS, followed by one padded FFT scratch per wave
constexpr int kWaves = 8;                        // waves per workgroup
constexpr int kThreads = kWaves * 64;
constexpr size_t kLdsTablesPad = NAE_FFT_N * sizeof(float) + (kT1024Pad + 64 + kTwaCf) * sizeof(cf);

// stages the four tables at the front of the LDS (kLdsTablesPad bytes) with n_threads threads; the caller issues the barrier
__device__ __forceinline__ void stage_tables(unsigned char* smem, const Tables& tb, int n_threads, float*& hann, cf*& t1024, cf*& w64, cf*& twa)
{
    hann = reinterpret_cast<float*>(smem);
    t1024 = reinterpret_cast<cf*>(smem + NAE_FFT_N * sizeof(float));
    w64 = t1024 + kT1024Pad;
    twa = w64 + 64;
    for (int i = threadIdx.x; i < NAE_FFT_N; i += n_threads) hann[i] = tb.hann[i];
    for (int i = threadIdx.x; i < NAE_FFT_BINS; i += n_threads) t1024[i] = tb.t1024[i];
    if (threadIdx.x < 64) w64[threadIdx.x] = tb.w512[8 * (threadIdx.x >> 3) * (threadIdx.x & 7)];
    fill_twa(twa, tb.w512, threadIdx.x, n_threads);
}

// wave index as a SCALAR: hipcc cannot prove threadIdx.x >> 6 wave-uniform, and everything derived from it
// (stream / tile / frame addresses) would otherwise be carried in VGPRs with 64-bit vector address math
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

struct PvParams {
    long long ha_q24;
    long long in_len;     // valid input sample-frames per stream
    long long frames;     // F
    long long mid_len;    // PV-stage output samples wanted
    int d0;
    unsigned r_q24_0, r_q24_1;
    int ch;
    int tile;             // frames (== output hop blocks) per tile
    int n_tiles;
    long long f_origin;   // first frame / output block of tile 0 (0 in block mode; > 0 when a stream is continued)
    long long f_stop;     // one past the last frame / block this launch is responsible for
    int skip_from;        // pass 1 only: tiles >= skip_from are not analysed (their sums are not needed)
    int phase_step;       // pass 3 only: pass 1 ran on tiles `phase_step` times shorter (more waves for the same frames);
    int phase_tiles;      //              the base phase of tile t is record t * phase_step of `phase_tiles` per stream-channel
    int base_zero;        // pass 3: the base phase of every tile is zero (one tile per stream-channel, nothing carried in): no workspace read
    uint32_t* carry_out;  // pass 3, optional: receives the synthesis phase behind frame `carry_frame`, [stream-channel][520] (a continued
    long long carry_frame; //             stream whose segment is ONE tile: no pass 1 is needed just to carry the phase on)
};

inline PvParams make_pv_params(const nae_stretch_plan& pl, size_t in_len, int ch, int tile, const nae_pv_segment* seg)
{
    PvParams p;
    p.ha_q24 = pl.ha_q24;
    p.in_len = (long long)in_len;
    p.frames = seg ? seg->f_limit : (long long)pl.frames;
    p.mid_len = seg ? seg->mid_limit : (long long)pl.mid_len;
    p.d0 = pl.d0;
    p.r_q24_0 = pl.r_q24[0];
    p.r_q24_1 = pl.r_q24[1];
    p.ch = ch;
    p.tile = tile;
    p.f_origin = seg ? seg->f_origin : 0;
    const long long cnt = seg ? seg->f_count : (long long)pl.frames;
    p.f_stop = p.f_origin + cnt;
    p.n_tiles = (int)((cnt + tile - 1) / tile);
    p.skip_from = p.n_tiles;
    p.phase_step = 1;
    p.phase_tiles = p.n_tiles;
    p.carry_out = nullptr;
    p.carry_frame = -1;
    p.base_zero = 0;
    return p;
}

// The kernels that walk one wave per (stream-channel, tile) number their items with the tile fastest: stream-channel sc = (stream s_idx, channel c)
struct WaveTile { long long sc, s_idx; int tile, c; };
__device__ __forceinline__ WaveTile wave_tile(long long item, int n_tiles, int ch)
{
    const long long sc = item / n_tiles;
    return WaveTile{sc, sc / ch, (int)(item % n_tiles), (int)(sc % ch)};
}

__device__ __forceinline__ long long frame_start(const PvParams& p, long long f)
{
    return (((f - 1) * p.ha_q24 + (1ll << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - NAE_FFT_N / 2;
}

// canonical phases of this lane's 9 bins (k = lane + 64 r, and 512)
__device__ __forceinline__ void phases_of(const cf (&v)[8], cf nyq, uint32_t (&qa)[9])
{
#pragma unroll
    for (int r = 0; r < 8; r++) qa[r] = atan2_q32(v[r].y, v[r].x);
    qa[8] = (nyq.x < 0.0f) ? 0x80000000u : 0u;     // bin N/2 of a real signal is real
}

// phase increment of one hop for this lane's 9 bins (integer, exact)
__device__ __forceinline__ void phase_inc(const uint32_t (&qa)[9], const uint32_t (&qp)[9], uint32_t (&acc)[9],
                                          int kl, unsigned d, unsigned R)
{
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const unsigned k = (r < 8) ? (unsigned)(kl + 64 * r) : 512u;
        const uint32_t e = ((k * d) & (NAE_FFT_N - 1)) << 22;
        const int32_t dw = (int32_t)(qa[r] - qp[r] - e);
        const uint32_t adv = ((k * NAE_HOP) & (NAE_FFT_N - 1)) << 22;
        // R <= 2^26 (d >= 64), so it is a positive int32: one signed 32x32->64 multiply-add (v_mad_i64_i32)
        const long long scaled = ((long long)dw * (long long)(int32_t)R + (1ll << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
        acc[r] += adv + (uint32_t)scaled;
    }
}

} // namespace nae

// What the vocoder's leaf launchers share, as nae_launch_pv_phase / nae_launch_pv_synth (kernels_stft.hip) built it from the nae_pv_run.  Pass 1
// has no `out` and writes `phase_ws`, pass 3 reads it; lifter > 0 (pass 3): formant preservation with that lifter and transposer ratio g ("Formant
// preservation"); transients: passes 1 and 3 detect onsets and reset Qs there, pass 1 flags its records and the scan is the segmented one;
// link: the kLink instantiations — the onset rule and the lock's peaks and regions read the linked power of the stream's two channels
namespace nae {
struct PvJob {
    int n_fft;
    PvParams p;
    SigViewD src; OutViewD out;
    long long n_sc; bool unit_stride;
    uint32_t* phase_ws;
    int lifter; float g; bool transients, link;
};
}

// kernels_pvpipe.hip: pass 3 at 1024 points (no lifter, no transients)
int nae_launch_pv_pipe(nae_ctx* ctx, const nae::PvJob& j, int frames_per_step);
// kernels_pvlock.hip: the locked passes L1 + L2 (the maps of tiles [0, n_needed), then the records in phase_ws; maps / sig16: the tile maps'
// c and sigma, nae_pv_workspace_bytes) and pass L3
int nae_launch_pvlock_phase(nae_ctx* ctx, const nae::PvJob& j, int n_needed, uint32_t* maps, uint16_t* sig16, const uint32_t* carry_in,
                            uint32_t* carry_out);
int nae_launch_pvlock_synth(nae_ctx* ctx, const nae::PvJob& j);
// kernels_pv_any.hip: pass 1 and pass 3 of the vocoder at n_fft = 512 ... 4096 (records of nae_pv_record_pad(n_fft) int32), and pass 2 of the
// unlocked vocoder after either pass 1 (the records of tiles [0, n_read) in phase_ws; `name`: the profile name)
int nae_launch_pvany_phase(nae_ctx* ctx, const nae::PvJob& j);
int nae_launch_pv_scan(nae_ctx* ctx, int n_fft, const char* name, uint32_t* phase_ws, long long n_sc, int n_tiles, const uint32_t* carry_in,
                       uint32_t* carry_out, int n_read, bool segmented);
int nae_launch_pvany_synth(nae_ctx* ctx, const nae::PvJob& j);
// kernels_pvenv.hip: the envelope pass of a forced plan (formant shift at tempo 1) — analysis, gain with lifter and ratio g, synthesis; no phases
int nae_launch_pvenv(nae_ctx* ctx, const nae::PvJob& j);
