// kernels_pvenv.hip — the formant shift at tempo 1 ("Formant shift") at frame sizes N = 512, 1024, 2048, 4096 for gfx950.
//
// With analysis hop = synthesis hop = H the vocoder's recurrence gives Qs_f = Qa_f for every frame (d = H, R = 2^24: inc = Qa_f - Qa_{f-1}
// exactly; the same locked, and an onset reset is the identity), so the stage is an STFT pass: analysis, cepstral envelope, Y = G X, c2r, window,
// overlap-add, gain.  pv_env_kernel is that pass and nothing else — no atan2, no sin / cos, no 64-bit multiply, no pass 1, no scan, no carried
// phase.  One wave per (stream-channel, tile of hop blocks); it starts cold: frames b0 ... b_end + 2 feed blocks b0 ... b_end - 1, each block in
// increasing frame order, so every tiling and the streaming handle give the same bits.  A wave's FFT scratch, the frame's spectrum and the
// L / c' / Ls array live in LDS (PvEnv<N>), the three open overlap-add blocks in registers, as in pv_any_synth_kernel, whose helpers (pv_any.h) it
// is built from.
#include "pv_any.h"

namespace nae {

template <int N, bool kUnit>
__global__ __launch_bounds__(64 * (PvEnv<N>::kWaves)) void pv_env_kernel(SigViewD src, PvParams p, long long n_items, OutViewD out, SpecAnyTables tb,
                                                                        int lifter, float g)
{
    using P = PvAny<N, true>;
    using E = PvEnv<N>;
    using Gm = typename P::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[E::kWaves * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[E::kWaves * P::PAD];
    __shared__ float lbuf[E::kWaves * P::PAD];             // L, then c', then Ls
    for (int i = threadIdx.x; i < 512; i += 64 * E::kWaves) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * E::kWaves + wave_id();
    if (item >= n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * P::PAD;
    float* lb = lbuf + wave_id() * P::PAD;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    const ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const long long b0 = p.f_origin + (long long)tile * p.tile;
    const long long b_end = b0 + p.tile < p.f_stop ? b0 + p.tile : p.f_stop;
    long long f_end = b_end + 3;                           // frames b0 .. b_end+2 feed blocks b0 .. b_end-1
    if (f_end > p.frames) f_end = p.frames;
    float* optr = out.base + s_idx * out.ss + c * out.cs;

    float r0[P::K], r1[P::K], r2[P::K];
#pragma unroll
    for (int i = 0; i < P::K; i++) r0[i] = r1[i] = r2[i] = 0.0f;
#pragma unroll 1
    for (long long f = b0; f < f_end; f++) {
        pva_analyse<N, kUnit>(scr, w512l, tb, in, pva_frame_start<N>(p, f), lane);
#pragma unroll 2
        for (int r = 0; r < P::NB; r++) {
            const int k = lane + 64 * r;
            if (k < P::B) {
                const cf x = any_rfft_bin<Gm>(scr, tb.tn, k);
                lds_st(ys + k, x);                         // Y = X: the gain of pva_formant makes it G X
                lb[k] = pva_log_mag(x);
            }
        }
        wave_lds_sync();
        pva_formant<N>(scr, w512l, tb, ys, lb, lifter, g, lane);
        float o[P::K];
        pva_synth_frame<N>(scr, w512l, tb, ys, r0, r1, r2, o, lane);
        pva_store_block<N>(p, b0, b_end, optr, out.fs, f - 3, o, lane);
    }
    pva_drain<N>(p, b0, b_end, f_end, optr, out.fs, r0, r1, r2, lane);
}

template <int N>
static int launch_env(nae_ctx* ctx, const PvJob& j, const SpecAnyTables& tb)
{
    using E = PvEnv<N>;
    const long long items = j.n_sc * j.p.n_tiles;
    if (items == 0) return NAE_OK;
    return with_flags(j.unit_stride, [&](auto unit) {
        return nae_launch_tiles(ctx, "pv_env_kernel", "pv_env_kernel: grid too large", pv_env_kernel<N, unit.value>, items, E::kWaves, 64 * E::kWaves, 0,
                                j.src, j.p, items, j.out, tb, j.lifter, j.g);
    });
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

int nae_launch_pvenv(nae_ctx* ctx, const PvJob& j)
{
    SpecAnyTables tb;
    const int rc = nae_spec_any_tables(ctx, j.n_fft, &tb);
    if (rc) return rc;
    return at_size(ctx, j.n_fft, [&](auto n) { return launch_env<decltype(n)::value>(ctx, j, tb); });
}
