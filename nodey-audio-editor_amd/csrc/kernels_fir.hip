// kernels_fir.hip — K9, the FIR filter by FFT fast convolution ("K9 FIR filter") at frame sizes N = 512, 1024, 2048, 4096 for gfx950.
//
// Overlap-save with B = N / 2 new samples per block: block b reads u[n] = x[b B - B + n], n < N (zero outside the signal), U = r2c_N(u) without a
// window, Y = U H (four products, one subtract, one add: no FMA), v = c2r_N(Y), and y[b B + n] = v[B + n].  fir_block_kernel is that pass, built
// from the wave-level FFT of fft_any.h and the c2r of pv_any.h as pv_env_kernel is: one wave per (stream-channel, tile of consecutive blocks),
// the FFT scratch and the block's spectrum Y in LDS.  A wave walks its blocks in order and keeps the second half of u — packed point m at
// carry[m - M/2] of its own lane — as the next block's first half, so every input sample is read once per tile plus one half block at the tile
// head.  H = r2c_N(h zero-padded) comes from fir_taps_kernel, the same first pass, radix passes and split on one wave; the blocks read it from
// global memory (16 KiB at 4096, shared by every wave of the launch: it stays in the vector L1 / L2).  Blocks do not depend on each other beyond
// the samples they share, so every tiling and the streaming handle give the same bits.  The geometry, the tile head and the r2c of a block live in
// fir_block.h, which the long convolution (kernels_conv.hip) shares.
#include "fir_block.h"
#include <string.h>
#include <math.h>
#include <new>

namespace nae {

struct FirParams {
    long long in_len;      // samples of a stream-channel: reads outside [0, in_len) give zero, samples >= in_len are not stored
    long long b_origin;    // blocks [b_origin, b_stop) are computed (a handle continues where it stopped)
    long long b_stop;
    long long n_items;     // (stream-channel, tile) pairs
    int tile, n_tiles, ch;
};

template <int N, bool kUnit>
__global__ __launch_bounds__(64 * (Fir<N>::kWaves)) void fir_block_kernel(SigViewD src, OutViewD out, FirParams p, const cf* __restrict__ hspec,
                                                                         SpecAnyTables tb)
{
    using F = Fir<N>;
    using Gm = typename F::Gm;
    constexpr int M = F::M, B = F::B;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[F::kWaves * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[F::kWaves * F::PAD];
    __shared__ __attribute__((aligned(16))) cf carry[F::kWaves * (M / 2)];
    for (int i = threadIdx.x; i < 512; i += 64 * F::kWaves) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * F::kWaves + wave_id();
    if (item >= p.n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * F::PAD;
    cf* cw = carry + wave_id() * (M / 2);
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const float* ip = src.base + w.s_idx * src.ss + w.c * src.cs;
    float* op = out.base + w.s_idx * out.ss + w.c * out.cs;
    const long long b0 = p.b_origin + (long long)w.tile * p.tile;
    const long long b_end = b0 + p.tile < p.b_stop ? b0 + p.tile : p.b_stop;

    fir_tile_head<N, kUnit>(cw, ip, src.fs, p.in_len, b0, lane);
#pragma unroll 1
    for (long long b = b0; b < b_end; b++) {
        const long long n0 = b * B;
        const bool full = n0 + B <= p.in_len;              // wave-uniform
        fir_block_r2c<N, kUnit>(scr, cw, w512l, tb, ip, src.fs, p.in_len, n0, full, lane);       // U = r2c_N(u), the carry moves on
        // Y = U H: four products, one subtract, one add (-ffp-contract=off: nothing fuses)
#pragma unroll 2
        for (int r = 0; r < F::NB; r++) {
            const int k = lane + 64 * r;
            if (k <= M) {
                const cf u = any_rfft_bin<Gm>(scr, tb.tn, k);
                const cf h = hspec[k];
                lds_st(ys + k, cf{u.x * h.x - u.y * h.y, u.x * h.y + u.y * h.x});
            }
        }
        wave_lds_sync();
        // (fir_block.h restates this second half as fir_block_c2r_store for the long convolution.  This kernel keeps its own text: built on that
        // helper its unit-stride instantiation at 512 takes 82 VGPRs instead of 79 — five waves per SIMD instead of six — and the kernel is to
        // keep its resource figures.)
        // v = c2r_N(Y): split with T_N, conjugate, forward FFT_M, scale by 1 / M and conjugate back (pva_synth_frame's)
        any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, [&](int m) -> cf {
            cf xk = ys[m], xm = ys[M - m];
            if (m == 0) { xk.y = 0.0f; xm.y = 0.0f; }
            const cf E = {0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y)};
            const cf D = {0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)};
            const cf T = tb.tn[m];
            const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};   // conj(T) D
            return cf{E.x - Q.y, -(E.y + Q.x)};
        });
        any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
        wave_lds_sync();
        // y[b B + n] = v[B + n]: this lane's samples 2 (lane + 64 j) + {0, 1} of the block
#pragma unroll
        for (int j = 0; j < F::KP; j++) {
            const int t = lane + 64 * j;
            const cf z = lds_ld(scr + padx(zpos<Gm>(M / 2 + t)));
            const float v0 = z.x * (1.0f / M), v1 = -z.y * (1.0f / M);
            const long long n = n0 + 2 * t;
            if (full && kUnit) {
                f2u o;
                o.x = v0;
                o.y = v1;
                *reinterpret_cast<f2u*>(op + n) = o;
            } else {
                if (n < p.in_len) op[n * out.fs] = v0;
                if (n + 1 < p.in_len) op[(n + 1) * out.fs] = v1;
            }
        }
        wave_lds_sync();                                   // the next block rewrites the scratch and Y
    }
}

// H = r2c_N(h zero-padded to N), bins 0 ... M, on one wave: the routine the blocks use
template <int N>
__global__ __launch_bounds__(64) void fir_taps_kernel(const float* __restrict__ hpad, cf* __restrict__ hspec, SpecAnyTables tb)
{
    using F = Fir<N>;
    using Gm = typename F::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scr[Gm::SCR];
    for (int i = threadIdx.x; i < 512; i += 64) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    fir_taps_r2c<N>(scr, w512l, tb, hpad, N, hspec, lane);
}

template <int N>
static int launch_fir(nae_ctx* ctx, const SigViewD& src, const OutViewD& out, const FirParams& p, const cf* hspec, const SpecAnyTables& tb)
{
    using F = Fir<N>;
    return with_flags(src.fs == 1 && out.fs == 1, [&](auto unit) {
        return nae_launch_tiles(ctx, "fir_block_kernel", "fir_block_kernel: grid too large", fir_block_kernel<N, unit.value>, p.n_items, F::kWaves,
                                64 * F::kWaves, 0, src, out, p, hspec, tb);
    });
}

template <int N>
static int launch_fir_taps(nae_ctx* ctx, const float* hpad, cf* hspec, const SpecAnyTables& tb)
{
    return nae_launch_grid(ctx, "fir_taps_kernel", fir_taps_kernel<N>, dim3(1), dim3(64), 0, hpad, hspec, tb);
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

size_t nae_fir_spec_floats(int n_fft) { return (size_t)n_fft + 2 * ((size_t)n_fft / 2 + 1); }

// Blocks per tile of a launch over `blocks` blocks of n_sc stream-channels: the one tile rule (nae_pick_tile) for the waves a CU holds
// (Fir<N>::kResident), never shorter than NAE_FIR_MIN_TILE blocks, the number of tiles rounded down.  fir_tile forces the tile.
int nae_pick_fir_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc)
{
    const size_t resident = n_fft == 512 ? Fir<512>::kResident : n_fft == 1024 ? Fir<1024>::kResident : n_fft == 2048 ? Fir<2048>::kResident
                                                                                                                       : Fir<4096>::kResident;
    return nae_pick_tile(ctx, ctx->fir_tile, blocks, n_sc, resident, NAE_FIR_MIN_TILE, true);
}

// H of n_taps host taps into d_spec (nae_fir_spec_floats(n_fft) floats: the padded taps, then H[0 ... n_fft / 2]); waits for the upload
int nae_fir_make_spec(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, float* d_spec)
{
    SpecAnyTables tb;
    int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    hipError_t e = hipMemsetAsync(d_spec, 0, (size_t)n_fft * sizeof(float), ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_spec, taps_host, (size_t)n_taps * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);            // the caller may reuse its taps
    if (e != hipSuccess) return nae_check(ctx, e, "fir: taps upload");
    cf* hspec = reinterpret_cast<cf*>(d_spec + n_fft);
    return at_size(ctx, n_fft, [&](auto n) { return launch_fir_taps<decltype(n)::value>(ctx, d_spec, hspec, tb); });
}

// blocks [b_origin, b_stop) of n_streams x ch signals of in_len samples (absolute indexing) with the spectrum in d_spec
int nae_launch_fir(nae_ctx* ctx, int n_fft, const float* d_spec, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t b_origin, size_t b_stop)
{
    if (b_stop <= b_origin || n_streams == 0) return NAE_OK;
    SpecAnyTables tb;
    const int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    const size_t blocks = b_stop - b_origin, n_sc = n_streams * (size_t)ch;
    FirParams p;
    p.in_len = (long long)in_len;
    p.b_origin = (long long)b_origin;
    p.b_stop = (long long)b_stop;
    p.tile = nae_pick_fir_tile(ctx, n_fft, blocks, n_sc);
    const size_t n_tiles = (blocks + (size_t)p.tile - 1) / (size_t)p.tile;
    if (n_tiles > 0x7fffffffull) return nae_fail(ctx, NAE_ERR_INVALID, "fir: too many tiles");
    p.n_tiles = (int)n_tiles;
    p.ch = ch;
    p.n_items = (long long)(n_sc * n_tiles);
    const cf* hspec = reinterpret_cast<const cf*>(d_spec + n_fft);
    return at_size(ctx, n_fft, [&](auto n) { return launch_fir<decltype(n)::value>(ctx, to_view(src), to_out(dst), p, hspec, tb); });
}

// the one statement of the parameter rules of nae_fir_block_f32 and nae_fir_create; *n_fft 0 becomes the library's pick
int nae_fir_check(nae_ctx* ctx, int n_taps, int ch, int* n_fft)
{
    if (n_taps < 1) return nae_fail(ctx, NAE_ERR_INVALID, "fir: n_taps must be at least 1");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (*n_fft == 0) *n_fft = nae_fir_pick_n_fft(n_taps);
    if (!nae_size_ok(*n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "fir: n_fft must be 512, 1024, 2048 or 4096, and at most 2049 taps");
    if (n_taps > *n_fft / 2 + 1) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "fir: at most n_fft / 2 + 1 taps");
    return NAE_OK;
}

extern "C" {

int nae_fir_pick_n_fft(int n_taps)
{
    if (n_taps < 1) return 0;
    for (int n = 512; n <= 4096; n *= 2)
        if (n / 2 + 1 >= n_taps) return n;
    return 0;
}

int nae_fir_block_f32(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                      const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!taps_host || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "fir: null pointer");
    int rc = nae_fir_check(ctx, n_taps, ch, &n_fft);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "fir: null pointer");
    (void)nae_use_device(ctx);
    // H is kept with the context: a call with the taps and the size of the last one computes nothing again
    rc = ctx->fir_spec.get(ctx, {n_fft}, taps_host, (size_t)n_taps * sizeof(float), nae_fir_spec_floats(n_fft) * sizeof(float), "fir spectrum",
                           [&] { return nae_fir_make_spec(ctx, taps_host, n_taps, n_fft, ctx->fir_spec.as<float>()); });
    if (rc) return rc;
    const size_t B = (size_t)n_fft / 2;
    return nae_launch_fir(ctx, n_fft, ctx->fir_spec.as<float>(), src, in_len, ch, n_streams, dst, 0, (in_len + B - 1) / B);
}

// DESIGN.md §3, "K9 FIR filter", "Design": Kaiser-windowed sinc in double, rounded once
static void fir_lowpass(double fc, int sample_rate, int L, double* h)
{
    const double pi = 3.14159265358979323846;
    const double c = 2.0 * fc / (double)sample_rate, half = 0.5 * (double)(L - 1), i0b = nae_bessel_i0(NAE_FIR_KAISER_BETA);
    double sum = 0.0;
    for (int n = 0; n < L; n++) {
        const double t = (double)n - half;
        const double a = L > 1 ? t / half : 0.0;
        const double r = 1.0 - a * a;
        const double w = nae_bessel_i0(NAE_FIR_KAISER_BETA * sqrt(r > 0.0 ? r : 0.0)) / i0b;
        const double arg = pi * c * t;
        const double sinc = arg == 0.0 ? 1.0 : sin(arg) / arg;
        h[n] = c * sinc * w;
        sum += h[n];
    }
    for (int n = 0; n < L; n++) h[n] /= sum;
}

int nae_fir_design(int kind, int sample_rate, double f_lo, double f_hi, int n_taps, float* taps_host)
{
    if (!taps_host || kind < 0 || kind > 3 || sample_rate <= 0 || n_taps < 1 || (n_taps & 1) == 0) return NAE_ERR_INVALID;
    const double nyq = 0.5 * (double)sample_rate;
    const bool need_lo = kind != 0, need_hi = kind != 1;
    if (need_lo && !(f_lo > 0.0 && f_lo < nyq)) return NAE_ERR_INVALID;
    if (need_hi && !(f_hi > 0.0 && f_hi < nyq)) return NAE_ERR_INVALID;
    if (need_lo && need_hi && !(f_lo < f_hi)) return NAE_ERR_INVALID;
    double* lo = new (std::nothrow) double[2 * (size_t)n_taps];
    if (!lo) return NAE_ERR_NOMEM;
    double* hi = lo + n_taps;
    if (need_lo) fir_lowpass(f_lo, sample_rate, n_taps, lo);
    if (need_hi) fir_lowpass(f_hi, sample_rate, n_taps, hi);
    const int mid = (n_taps - 1) / 2;
    for (int n = 0; n < n_taps; n++) {
        const double delta = n == mid ? 1.0 : 0.0;
        double v;
        if (kind == 0) v = hi[n];
        else if (kind == 1) v = delta - lo[n];
        else if (kind == 2) v = hi[n] - lo[n];
        else v = delta - (hi[n] - lo[n]);
        taps_host[n] = (float)v;
    }
    delete[] lo;
    return NAE_OK;
}

} // extern "C"
