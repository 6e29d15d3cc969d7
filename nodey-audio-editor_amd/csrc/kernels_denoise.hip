// kernels_denoise.hip — K13, the spectral gate ("K13 spectral gate") at frame sizes N = 512, 1024, 2048, 4096 for gfx950.
//
// An STFT pass in the vocoder's geometry at tempo 1, as pv_env_kernel (kernels_pvenv.hip) is and from the same helpers (pv_any.h): analysis, a
// gain per bin, c2r, window, overlap-add.  The gain comes from decisions d_f[k] = p_f[k] > profile[k] thr_scale, one bit per bin, smoothed in
// integers over 2 Tn + 1 frames and 2 Fn + 1 bins.  denoise_gate_kernel is one wave per (stream-channel, tile of hop blocks) and starts cold: for
// the tile [b0, b_end) it takes the decisions of frames b0 - Tn ... b_end + 2 + Tn and synthesises frames b0 ... b_end + 2, so the decision front
// runs Tn frames ahead of the synthesis and a frame is analysed twice (Tn = 0: once) — three FFTs per frame against pv_env_kernel's four.
// Lane l holds bins l + 64 r, so a wave ballot is the decisions of 64 bins; the ballots of the last 2 Tn + 1 frames stay in an LDS ring, v (the
// time sum) is summed per lane from the ring (one word per lane, handed round as scalars) into one LDS array of 16-bit counts, and c (the
// frequency sum) is read from that array.  Every
// count is an integer: any order of summation gives the same c, and every tiling and the streaming handle give the same bits.  A wave's FFT
// scratch, the frame's spectrum Y, the counts and the ring live in LDS (Dn<N>), the three open overlap-add blocks in registers.
// denoise_profile_kernel learns the profile: one wave per channel walks the excerpt's frames in order with its bins' sums in double.
// Built with -ffp-contract=off: every f32 step is one IEEE operation in the order of the CPU statement (tests/denoise_ref/ref_denoise.c).
#include "pv_any.h"
#include <math.h>

namespace nae {

constexpr int kDnRing = 2 * NAE_DENOISE_MAX_TIME + 1;     // frames of decisions a wave keeps

// A wave's LDS: the FFT scratch and Y as PvEnv<N>, the counts v in 16 bits (at most (Tn + 1)^2 = 81) where PvEnv<N> has L in 32, and the ring of
// ballots: 8 / 8 / 7 / 3 waves per workgroup at N = 512 ... 4096, PvEnv<N>'s
template <int N>
struct Dn {
    using A = PvAny<N>;
    static constexpr int NB = A::NB;
    static constexpr int kUnroll = N == 4096 ? 1 : 2;    // bins in flight in the per-bin loops: at 4096 two of them spill
    static constexpr int VPAD = A::PAD;                   // counts of bins 0 ... M (the mirror keeps every read inside them)
    static constexpr size_t kWave = A::Gm::SCR * sizeof(cf) + A::PAD * sizeof(cf) + VPAD * sizeof(uint16_t) + kDnRing * NB * sizeof(uint64_t);
    static constexpr int kMaxWaves = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave);
    static constexpr int kWaves = kMaxWaves < 8 ? kMaxWaves : 8;
    // waves a CU holds: whole workgroups by LDS (24, 8, 7, 3 at N = 512 ... 4096), and no more than the registers hold — 114 / 123 VGPRs at
    // 512 (4 waves per SIMD: 16), 188 ... 256 above (2 per SIMD: 8; `make resources`, profiles/r19_denoise.md): 16, 8, 7, 3
    static constexpr int kLdsResident = (int)((160 * 1024) / (512 * sizeof(cf) + kWaves * kWave)) * kWaves;
    static constexpr int kVgprResident = N == 512 ? 16 : 8;
    static constexpr int kResident = kLdsResident < kVgprResident ? kLdsResident : kVgprResident;
    static_assert(kWaves >= 1, "a wave's state fits a CU's LDS");
};

struct DnGate {
    const float* prof;     // [profile_ch][M + 1]
    long long prof_cs;     // floats between two channels' profiles (0: one profile for every channel)
    float thr_scale, floor_gain, span, inv_c;
    int tn, fn, c_full;    // C = (Tn + 1)^2 (Fn + 1)^2
};

// p = X.x X.x + X.y X.y: two products and one add
__device__ __forceinline__ float dn_power(cf x) { return x.x * x.x + x.y * x.y; }

// the decisions of frame g into ring slot `slot`: a frame outside [0, frames) is silence, closed and not analysed
template <int N, bool kUnit>
__device__ __forceinline__ void dn_decide(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in, const PvParams& p, const float* prof,
                                          float thr_scale, uint64_t* ring, int slot, long long g, int lane)
{
    using D = Dn<N>;
    using Gm = typename D::A::Gm;
    uint64_t* rw = ring + slot * D::NB;
    if (g < 0 || g >= p.frames) {                          // wave-uniform
        for (int r = lane; r < D::NB; r += 64) rw[r] = 0;
        return;
    }
    pva_analyse<N, kUnit>(scr, w512l, tb, in, pva_frame_start<N>(p, g), lane);
#pragma unroll (Dn<N>::kUnroll)
    for (int r = 0; r < D::NB; r++) {
        const int k = lane + 64 * r;
        bool d = false;
        if (k <= D::A::M) d = dn_power(any_rfft_bin<Gm>(scr, tb.tn, k)) > prof[k] * thr_scale;
        const uint64_t word = __ballot(d);
        if (lane == 0) rw[r] = word;
    }
    wave_lds_sync();                                       // the next analysis rewrites the scratch; the ring is read by every lane
}

template <int N, bool kUnit>
__global__ __launch_bounds__(64 * (Dn<N>::kWaves)) void denoise_gate_kernel(SigViewD src, PvParams p, long long n_items, OutViewD out, SpecAnyTables tb,
                                                                           DnGate gt)
{
    using P = PvAny<N>;
    using D = Dn<N>;
    using Gm = typename P::Gm;
    constexpr int M = P::M;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[D::kWaves * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[D::kWaves * P::PAD];
    __shared__ __attribute__((aligned(16))) uint64_t ringbuf[D::kWaves * kDnRing * D::NB];
    __shared__ __attribute__((aligned(16))) uint16_t vbuf[D::kWaves * D::VPAD];
    for (int i = threadIdx.x; i < 512; i += 64 * D::kWaves) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * D::kWaves + wave_id();
    if (item >= n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * P::PAD;
    uint64_t* ring = ringbuf + wave_id() * (kDnRing * D::NB);
    uint16_t* vb = vbuf + wave_id() * D::VPAD;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    const ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const float* prof = gt.prof + c * gt.prof_cs;
    const long long b0 = p.f_origin + (long long)tile * p.tile;
    const long long b_end = b0 + p.tile < p.f_stop ? b0 + p.tile : p.f_stop;
    long long f_end = b_end + 3;                           // frames b0 .. b_end+2 feed blocks b0 .. b_end-1
    if (f_end > p.frames) f_end = p.frames;
    float* optr = out.base + s_idx * out.ss + c * out.cs;
    const int tn = gt.tn, fn = gt.fn, nring = 2 * tn + 1;

    // the decision front: frames b0 - Tn ... b0 + Tn - 1 before the first synthesis; frame g sits in slot (g - (b0 - Tn)) mod (2 Tn + 1)
    int head = 0;                                          // the slot of frame f - Tn, the oldest one frame f reads
#pragma unroll 1
    for (int j = 0; j < 2 * tn; j++) dn_decide<N, kUnit>(scr, w512l, tb, in, p, prof, gt.thr_scale, ring, j, b0 - tn + j, lane);

    float r0[P::K], r1[P::K], r2[P::K];
#pragma unroll
    for (int i = 0; i < P::K; i++) r0[i] = r1[i] = r2[i] = 0.0f;
#pragma unroll 1
    for (long long f = b0; f < f_end; f++) {
        const int newest = head == 0 ? nring - 1 : head - 1;   // the slot of frame f + Tn: the one frame f - Tn - 1 had
        if (tn > 0) dn_decide<N, kUnit>(scr, w512l, tb, in, p, prof, gt.thr_scale, ring, newest, f + tn, lane);
        pva_analyse<N, kUnit>(scr, w512l, tb, in, pva_frame_start<N>(p, f), lane);
        // Y = X, and the time sum v_f[k] = sum_j (Tn + 1 - |j|) d_{f+j}[k] of this lane's bins
#pragma unroll (Dn<N>::kUnroll)
        for (int r = 0; r < D::NB; r++) {
            const int k = lane + 64 * r;
            cf x = cf{0.0f, 0.0f};
            if (k <= M) {
                x = any_rfft_bin<Gm>(scr, tb.tn, k);
                lds_st(ys + k, x);
            }
            int v;
            if (tn == 0) {                                 // the frame decides for itself: no second analysis
                v = (k <= M && dn_power(x) > prof[k] * gt.thr_scale) ? 1 : 0;
            } else {
                // lane t < 2 Tn + 1 fetches the ballot of frame f - Tn + t: one LDS read in flight per lane instead of 2 Tn + 1 dependent
                // ones; the words then travel as scalars
                int slot = head + lane;
                slot = slot >= nring ? slot - nring : slot;
                const uint64_t mine = lane < nring ? ring[slot * D::NB + r] : 0;
                const int lo = (int)(uint32_t)mine, hi = (int)(uint32_t)(mine >> 32);
                v = 0;
#pragma unroll 1
                for (int t = 0; t < nring; t++) {
                    const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane(lo, t), wh = (uint32_t)__builtin_amdgcn_readlane(hi, t);
                    const int wgt = t <= tn ? t + 1 : nring - t;   // Tn + 1 - |t - Tn|
                    v += (((lane & 32) ? wh : wl) >> (lane & 31)) & 1u ? wgt : 0;
                }
            }
            if (k <= M) vb[k] = (uint16_t)v;
        }
        wave_lds_sync();
        // the frequency sum c_f[k] = sum_i (Fn + 1 - |i|) v_f[mir(k + i)] and the gain
#pragma unroll (Dn<N>::kUnroll)
        for (int r = 0; r < D::NB; r++) {
            const int k = lane + 64 * r;
            if (k <= M) {
                int cnt = 0;
                // every offset of the widest triangle, the ones beyond Fn with weight 0: nine independent reads, no branch between them
#pragma unroll
                for (int i = -NAE_DENOISE_MAX_FREQ; i <= NAE_DENOISE_MAX_FREQ; i++) {
                    int kk = k + i;
                    kk = kk < 0 ? -kk : (kk > M ? 2 * M - kk : kk);
                    const int wgt = fn + 1 - (i < 0 ? -i : i);
                    cnt += (wgt > 0 ? wgt : 0) * (int)vb[kk];
                }
                const float G = cnt == gt.c_full ? 1.0f : gt.floor_gain + gt.span * ((float)cnt * gt.inv_c);
                const cf y = ys[k];
                ys[k] = cf{G * y.x, G * y.y};
            }
        }
        wave_lds_sync();
        float o[P::K];
        pva_synth_frame<N>(scr, w512l, tb, ys, r0, r1, r2, o, lane);
        pva_store_block<N>(p, b0, b_end, optr, out.fs, f - 3, o, lane);
        head = head + 1 == nring ? 0 : head + 1;
    }
    pva_drain<N>(p, b0, b_end, f_end, optr, out.fs, r0, r1, r2, lane);
}

struct DnProfParams {
    long long n_frames;    // frames at 0, H, 2 H, ...: all inside the excerpt
    long long len;
    long long bins_stride; // floats between two channels' profiles: M + 1
};

// one wave per channel: the frames of the excerpt in order, this lane's bins summed in double; profile = (float)(sum / n)
template <int N, bool kUnit>
__global__ __launch_bounds__(64) void denoise_profile_kernel(SigViewD src, DnProfParams pp, long long n_items, float* __restrict__ profile,
                                                            SpecAnyTables tb)
{
    using P = PvAny<N>;
    using Gm = typename P::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scr[Gm::SCR];
    for (int i = threadIdx.x; i < 512; i += 64) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long c = blockIdx.x;
    if (c >= n_items) return;
    const ChanView in{src.base + c * src.cs, src.fs, pp.len};
    double acc[P::NB];
#pragma unroll
    for (int r = 0; r < P::NB; r++) acc[r] = 0.0;
#pragma unroll 1
    for (long long f = 0; f < pp.n_frames; f++) {
        pva_analyse<N, kUnit>(scr, w512l, tb, in, f * P::H, lane);
#pragma unroll
        for (int r = 0; r < P::NB; r++) {
            const int k = lane + 64 * r;
            if (k <= P::M) acc[r] += (double)dn_power(any_rfft_bin<Gm>(scr, tb.tn, k));
        }
        wave_lds_sync();                                   // the next frame rewrites the scratch
    }
    const double n = (double)pp.n_frames;
#pragma unroll
    for (int r = 0; r < P::NB; r++) {
        const int k = lane + 64 * r;
        if (k <= P::M) profile[c * pp.bins_stride + k] = (float)(acc[r] / n);
    }
}

template <int N>
static int launch_gate(nae_ctx* ctx, const SigViewD& src, const OutViewD& out, const PvParams& p, long long n_sc, const DnGate& gt,
                       const SpecAnyTables& tb)
{
    using D = Dn<N>;
    const long long items = n_sc * p.n_tiles;
    if (items == 0) return NAE_OK;
    return with_flags(src.fs == 1 && out.fs == 1, [&](auto unit) {
        return nae_launch_tiles(ctx, "denoise_gate_kernel", "denoise_gate_kernel: grid too large", denoise_gate_kernel<N, unit.value>, items, D::kWaves,
                                64 * D::kWaves, 0, src, p, items, out, tb, gt);
    });
}

template <int N>
static int launch_profile(nae_ctx* ctx, const SigViewD& src, const DnProfParams& pp, int ch, float* profile, const SpecAnyTables& tb)
{
    return with_flags(src.fs == 1, [&](auto unit) {
        return nae_launch_tiles(ctx, "denoise_profile_kernel", "denoise_profile_kernel: grid too large", denoise_profile_kernel<N, unit.value>,
                                (long long)ch, 1, 64, 0, src, pp, (long long)ch, profile, tb);
    });
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// Hop blocks per tile of a launch over `blocks` blocks of n_sc stream-channels: the one tile rule (nae_pick_tile) for the waves a CU holds
// (Dn<N>::kResident), never shorter than NAE_DENOISE_MIN_TILE blocks (a tile pays 3 Tn + 3 analyses beyond its own frames' — 9 at the
// default Tn = 2 against 3 per block: under a tenth of its work at 32 blocks), the number of tiles rounded down.  dn_tile forces the tile.
// profiles/r19_denoise.md has the measurement the rule was checked against.
int nae_pick_denoise_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc)
{
    const size_t resident = n_fft == 512 ? Dn<512>::kResident : n_fft == 1024 ? Dn<1024>::kResident : n_fft == 2048 ? Dn<2048>::kResident
                                                                                                                     : Dn<4096>::kResident;
    return nae_pick_tile(ctx, ctx->dn_tile, blocks, n_sc, resident, NAE_DENOISE_MIN_TILE, true);
}

// the one statement of the parameter rules of nae_denoise_block_f32 and nae_denoise_create
int nae_denoise_check(nae_ctx* ctx, const nae_denoise_params* p, const float* profile_dev, int profile_ch, int ch)
{
    if (!p || !profile_dev) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: null pointer");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (profile_ch != 1 && profile_ch != ch) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: profile_ch must be 1 or the channel count");
    if (p->time_smooth < 0 || p->time_smooth > NAE_DENOISE_MAX_TIME) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: time_smooth outside 0 ... 8");
    if (p->freq_smooth < 0 || p->freq_smooth > NAE_DENOISE_MAX_FREQ) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: freq_smooth outside 0 ... 4");
    if (!isfinite(p->thr_scale) || p->thr_scale < 0.0f) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: thr_scale negative or not finite");
    if (!isfinite(p->floor_gain) || p->floor_gain < 0.0f || p->floor_gain > 1.0f) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: floor_gain outside 0 ... 1");
    if (!nae_size_ok(p->n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "denoise: n_fft must be 512, 1024, 2048 or 4096");
    return NAE_OK;
}

// hop blocks [b_origin, b_stop) of n_streams x ch signals of in_len samples (absolute indexing) with the profile in d_profile
int nae_launch_denoise(nae_ctx* ctx, const nae_denoise_params* dp, const float* d_profile, int profile_ch, const nae_sig* src, size_t in_len, int ch,
                       size_t n_streams, const nae_sig* dst, size_t b_origin, size_t b_stop)
{
    if (b_stop <= b_origin || n_streams == 0) return NAE_OK;
    const int n_fft = dp->n_fft, H = n_fft / 4;
    SpecAnyTables tb;
    const int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    const size_t blocks = b_stop - b_origin, n_sc = n_streams * (size_t)ch;
    const int tile = nae_pick_denoise_tile(ctx, n_fft, blocks, n_sc);
    const size_t n_tiles = (blocks + (size_t)tile - 1) / (size_t)tile;
    if (n_tiles > 0x7fffffffull) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: too many tiles");
    PvParams p{};
    p.ha_q24 = (long long)H << NAE_HA_FRAC_BITS;           // tempo 1: frame f starts at (f - 3) H
    p.in_len = (long long)in_len;
    p.frames = (long long)((in_len + (size_t)H - 1) / (size_t)H) + 3;
    p.mid_len = (long long)in_len;
    p.ch = ch;
    p.tile = tile;
    p.n_tiles = (int)n_tiles;
    p.f_origin = (long long)b_origin;
    p.f_stop = (long long)b_stop;
    const int tn = dp->time_smooth, fn = dp->freq_smooth, c_full = (tn + 1) * (tn + 1) * (fn + 1) * (fn + 1);
    const DnGate gt{d_profile, profile_ch == 1 ? 0ll : (long long)(n_fft / 2 + 1), dp->thr_scale, dp->floor_gain,
                    (float)(1.0 - (double)dp->floor_gain), (float)(1.0 / (double)c_full), tn, fn, c_full};
    return at_size(ctx, n_fft, [&](auto n) { return launch_gate<decltype(n)::value>(ctx, to_view(src), to_out(dst), p, (long long)n_sc, gt, tb); });
}

extern "C" {

int nae_denoise_design(double reduction_db, double sensitivity_db, int n_fft, int time_smooth, int freq_smooth, nae_denoise_params* out)
{
    if (!out || !isfinite(reduction_db) || !isfinite(sensitivity_db)) return NAE_ERR_INVALID;
    if (reduction_db < 0.0 || reduction_db > NAE_DENOISE_MAX_REDUCTION_DB || sensitivity_db < NAE_DENOISE_MIN_SENSITIVITY_DB ||
        sensitivity_db > NAE_DENOISE_MAX_SENSITIVITY_DB || time_smooth < 0 || time_smooth > NAE_DENOISE_MAX_TIME || freq_smooth < 0 ||
        freq_smooth > NAE_DENOISE_MAX_FREQ)
        return NAE_ERR_INVALID;
    if (!nae_size_ok(n_fft)) return NAE_ERR_UNSUPPORTED;
    out->n_fft = n_fft;
    out->time_smooth = time_smooth;
    out->freq_smooth = freq_smooth;
    out->thr_scale = (float)pow(10.0, sensitivity_db / 10.0);
    out->floor_gain = (float)pow(10.0, -reduction_db / 20.0);
    return NAE_OK;
}

int nae_denoise_profile_f32(nae_ctx* ctx, int n_fft, const nae_sig* src, size_t len, int ch, float* profile_dev)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!src || !profile_dev || !src->base) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: null pointer");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!nae_size_ok(n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "denoise: n_fft must be 512, 1024, 2048 or 4096");
    if (len < (size_t)n_fft) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: the excerpt holds no whole frame");
    SpecAnyTables tb;
    const int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    const DnProfParams pp{(long long)((len - (size_t)n_fft) / (size_t)(n_fft / 4)) + 1, (long long)len, (long long)(n_fft / 2 + 1)};
    return at_size(ctx, n_fft, [&](auto n) { return launch_profile<decltype(n)::value>(ctx, to_view(src), pp, ch, profile_dev, tb); });
}

int nae_denoise_block_f32(nae_ctx* ctx, const nae_denoise_params* params, const float* profile_dev, int profile_ch, const nae_sig* src, size_t in_len,
                          int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: null pointer");
    const int rc = nae_denoise_check(ctx, params, profile_dev, profile_ch, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "denoise: null pointer");
    const size_t H = (size_t)params->n_fft / 4;
    return nae_launch_denoise(ctx, params, profile_dev, profile_ch, src, in_len, ch, n_streams, dst, 0, (in_len + H - 1) / H);
}

} // extern "C"
