// pv_any.h — device helpers of the size-generic vocoder (N = 512 ... 4096, hop N/4) shared by its translation units:
// kernels_pv_any.hip (passes 1-3) and kernels_pvenv.hip (the envelope-only pass of the formant shift at tempo 1).
#pragma once
#include "pv_roles.h"
#include "fft_any.h"

namespace nae {

template <int N, bool kFormant = false, bool kTransient = false, bool kLink = false>
struct PvAny {
    static constexpr int M = N / 2, H = N / 4, B = M + 1;
    static constexpr int PAD = (B + 7) & ~7;              // int32 per record: 520 at N = 1024, as the shipped kernels
    static constexpr int SH = 32 - ilog2c(N);             // a bin's phase advance per sample, in Q0.32: 2^SH
    static constexpr int NB = M / 64 + 1;                 // bins per lane: k = lane + 64 r; r = NB - 1 is bin M (lane 0)
    static constexpr int JQ = N / 512;                    // sample pairs per lane in each quarter (hop block) of a frame
    static constexpr int K = 2 * JQ;                      // samples per lane in each hop block
    using Gm = FftGeom<M, 1>;
    static constexpr int ST = NB * 64;                    // uint32 per per-bin state array of a wave
    static constexpr size_t kWave1 = Gm::SCR * sizeof(cf) + 2 * ST * sizeof(uint32_t)                     // scratch, Qa_{f-1}, sum
                                   + (kTransient ? ST * sizeof(float) : 0)                                 // transients: P_{f-1}
                                   + (kLink ? ST * sizeof(float) : 0);                                     // link: the other channel's P_f
    static constexpr size_t kWave3 = Gm::SCR * sizeof(cf) + PAD * sizeof(cf) + 2 * ST * sizeof(uint32_t) // scratch, Y, Qa_{f-1}, Qs
                                   + (kFormant ? PAD * sizeof(float) : 0)                                  // formant: L / c' / Ls
                                   + (kTransient ? ST * sizeof(float) : 0)                                 // transients: P_{f-1}
                                   + (kLink ? ST * sizeof(float) : 0);                                     // link: the other channel's P_f
    static constexpr int kMaxWaves1 = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave1);
    static constexpr int kMaxWaves3 = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave3);
    static constexpr int kWaves1 = kMaxWaves1 < 8 ? kMaxWaves1 : 8;   // 8, 8, 8, 4 waves per workgroup at N = 512 ... 4096 (transients: 8, 8, 7, 3; linked: 8, 8, 6, 3)
    static constexpr int kWaves3 = kMaxWaves3 < 8 ? kMaxWaves3 : 8;   // 8, 8, 6, 3 (formant: 8, 8, 5, 2; transients: 8, 8, 5, 2; both: 8, 8, 4, 2; linked: 8, 8, 4, 2, with formant 8, 7, 4, 2)
    // pass-3 waves a CU holds: whole workgroups by LDS (16, 8, 6, 3 at N = 512 ... 4096, formant 16, 8, 5, 2; registers allow as many; transients
    // 16, 8, 5, 2; formant and transients 16, 8, 4, 2).  Linked (with transients): by LDS 16, 8, 4, 2 and with formants 8, 7, 4, 2; the linked
    // kernels at 512 take 132 ... 157 VGPRs, three waves per SIMD and so one workgroup of 8 waves: 8, 8, 4, 2 and 8, 7, 4, 2
    // (profiles/r14_pv_link.md)
    static constexpr int kLdsResident3 = (int)((160 * 1024) / (512 * sizeof(cf) + kWaves3 * kWave3)) * kWaves3;
    static constexpr int kResident3 = kLink && N == 512 && kLdsResident3 > 8 ? 8 : kLdsResident3;
    static_assert(N >= 512 && N <= 4096 && (N & (N - 1)) == 0, "vocoder sizes 512 ... 4096");
    static_assert(kWaves1 >= 1 && kWaves3 >= 1, "a wave's state fits a CU's LDS");
};

template <int N>
__device__ __forceinline__ long long pva_frame_start(const PvParams& p, long long f)
{
    return (((f - 1) * p.ha_q24 + (1ll << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - N / 2;
}

// one frame: window, canonical FFT of M packed points into the wave's scratch (zero outside [0, in.len))
template <int N, bool kUnit>
__device__ __forceinline__ void pva_analyse(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in, long long s, int lane)
{
    using Gm = typename PvAny<N>::Gm;
    const bool interior = s >= 0 && s + N <= in.len;       // wave-uniform
    auto get = [&](int m) -> cf {
        const float2 h = *reinterpret_cast<const float2*>(tb.hann + 2 * m);
        const long long i0 = s + 2 * m;
        float x0, x1;
        if (interior) {
            if (kUnit) {
                const f2u x = *reinterpret_cast<const f2u*>(in.p + i0);
                x0 = x.x;
                x1 = x.y;
            } else {
                x0 = in.p[i0 * in.fs];
                x1 = in.p[(i0 + 1) * in.fs];
            }
        } else {
            x0 = (i0 >= 0 && i0 < in.len) ? in.p[i0 * in.fs] : 0.0f;
            x1 = (i0 + 1 >= 0 && i0 + 1 < in.len) ? in.p[(i0 + 1) * in.fs] : 0.0f;
        }
        return cf{x0 * h.x, x1 * h.y};
    };
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, get);
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
}

// hop block `be` of the tile: this lane's samples 2 (lane + 64 jj) + {0, 1} of the block, stored below mid_len
template <int N>
__device__ __forceinline__ void pva_store_block(const PvParams& p, long long b0, long long b_end, float* optr, long long fs, long long be,
                                                const float (&o)[PvAny<N>::K], int lane)
{
    using P = PvAny<N>;
    if (be < b0 || be >= b_end) return;                    // wave-uniform
    const long long n0 = be * P::H;
#pragma unroll
    for (int i = 0; i < P::K; i++) {
        const long long n = n0 + 2 * (lane + 64 * (i >> 1)) + (i & 1);
        if (n < p.mid_len) optr[n * fs] = o[i];
    }
}

// c2r input point m of a real half spectrum R[0..M] (the synthesis's split with T_N, conjugated; pass 3's zc with Y = R + 0i)
template <int M>
__device__ __forceinline__ cf pva_c2r_real_point(const float* rs, const cf* tn, int m)
{
    const cf xk = {rs[m], 0.0f}, xm = {rs[M - m], 0.0f};
    const cf E = {0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y)};
    const cf D = {0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)};
    const cf T = tn[m];
    const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};   // conj(T) D
    return cf{E.x - Q.y, -(E.y + Q.x)};
}

// formant preservation ("Formant preservation"), steps 2-5 of one frame: lb[k] = L[k] (k <= M) on entry, ys = the synthesis
// spectrum.  The cepstrum c = c2r_N(L), lifted to n < q and n > N - q, goes back into lb (c[n] at lb[n], c[N - j] at lb[M - j]: q <= N/4, so the
// two ranges do not meet); the envelope Ls = Re r2c_N(c') replaces it; then Y[k] *= G[k] = min(2^(Ls(k g) - Ls[k]), NAE_FORMANT_MAX_GAIN).
template <int N>
__device__ __forceinline__ void pva_formant(cf* scr, const cf* w512l, const SpecAnyTables& tb, cf* ys, float* lb, int q, float g, int lane)
{
    using Gm = typename PvAny<N, true>::Gm;
    constexpr int M = N / 2;
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, [&](int m) { return pva_c2r_real_point<M>(lb, tb.tn, m); });
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
#pragma unroll 1
    for (int t = lane; t < M; t += 64) {
        const int n = t < q ? t : (t > M - q ? t + M : -1);
        if (n >= 0) {
            const cf z = lds_ld(scr + padx(zpos<Gm>(n >> 1)));
            lb[t] = (n & 1) ? -z.y * (1.0f / M) : z.x * (1.0f / M);
        }
    }
    wave_lds_sync();
    auto lifted = [&](int n) -> float { return n < q ? lb[n] : (n > N - q ? lb[n - M] : 0.0f); };
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, [&](int m) { return cf{lifted(2 * m), lifted(2 * m + 1)}; });
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
#pragma unroll 1
    for (int k = lane; k <= M; k += 64) lb[k] = any_rfft_bin<Gm>(scr, tb.tn, k).x;
    wave_lds_sync();
#pragma unroll 1
    for (int k = lane; k <= M; k += 64) {
        const float u = (float)k * g;
        float G = 0.0f;
        if (u <= (float)M) {
            const int i = (int)u;
            const float t = u - (float)i;
            const float lu = i == M ? lb[M] : lb[i] + t * (lb[i + 1] - lb[i]);
            G = fminf(__builtin_amdgcn_exp2f(lu - lb[k]), NAE_FORMANT_MAX_GAIN);
        }
        const cf y = ys[k];
        ys[k] = cf{G * y.x, G * y.y};
    }
    wave_lds_sync();
}

// L[k] of formant preservation, step 1: log2 max(|X|, 2^-40)
__device__ __forceinline__ float pva_log_mag(cf x) { return __builtin_amdgcn_logf(fmaxf(sqrt_rn(x.x * x.x + x.y * x.y), 0x1p-40f)); }

// (pva_synth_frame and pva_drain restate the frame synthesis and the drain of pv_any_synth_kernel for pv_env_kernel.  pv_any_synth_kernel keeps
// its own text: built on these helpers its instantiations schedule differently — up to 33 instructions and 2 VGPRs at N = 4096 — and the existing
// kernels are to compile to the instructions they compiled to.)
// synthesis of one frame from its spectrum ys: c2r — split with T_N, conjugate, forward FFT_M (the first pass builds its inputs from Y), scale by
// 1/M and conjugate back — then the window and the overlap-add into the three open blocks r0, r1, r2 in increasing frame order; o is the block
// the frame completes (block f - 3 of frame f), with the gain
template <int N>
__device__ __forceinline__ void pva_synth_frame(cf* scr, const cf* w512l, const SpecAnyTables& tb, const cf* ys, float (&r0)[PvAny<N>::K],
                                                float (&r1)[PvAny<N>::K], float (&r2)[PvAny<N>::K], float (&o)[PvAny<N>::K], int lane)
{
    using P = PvAny<N>;
    using Gm = typename P::Gm;
    auto zc = [&](int m) -> cf {
        cf xk = ys[m], xm = ys[P::M - m];
        if (m == 0) { xk.y = 0.0f; xm.y = 0.0f; }
        const cf E = {0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y)};
        const cf D = {0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)};
        const cf T = tb.tn[m];
        const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};   // conj(T) D
        return cf{E.x - Q.y, -(E.y + Q.x)};
    };
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, zc);
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
    // windowed samples 2m, 2m + 1 (m = lane + 64 j) of quarter q = j / JQ, overlap-added in increasing frame order: block f - 3 is complete
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        float y[P::K];
#pragma unroll
        for (int jj = 0; jj < P::JQ; jj++) {
            const int m = lane + 64 * (q * P::JQ + jj);
            const cf z = lds_ld(scr + padx(zpos<Gm>(m)));
            const float2 w = *reinterpret_cast<const float2*>(tb.hann + 2 * m);
            y[2 * jj] = w.x * (z.x * (1.0f / P::M));
            y[2 * jj + 1] = w.y * (-z.y * (1.0f / P::M));
        }
#pragma unroll
        for (int i = 0; i < P::K; i++) {
            if (q == 0) o[i] = (r0[i] + y[i]) * NAE_OLA_GAIN;
            else if (q == 1) r0[i] = r1[i] + y[i];
            else if (q == 2) r1[i] = r2[i] + y[i];
            else r2[i] = y[i];
        }
    }
    wave_lds_sync();                                   // the next frame rewrites the scratch and Y
}

// frames past the last one (f_end) do not exist: the blocks they would have completed get nothing more
template <int N>
__device__ __forceinline__ void pva_drain(const PvParams& p, long long b0, long long b_end, long long f_end, float* optr, long long fs,
                                          float (&r0)[PvAny<N>::K], float (&r1)[PvAny<N>::K], float (&r2)[PvAny<N>::K], int lane)
{
    using P = PvAny<N>;
#pragma unroll 1
    for (long long f = f_end > b0 ? f_end : b0; f < b_end + 3; f++) {
        float o[P::K];
#pragma unroll
        for (int i = 0; i < P::K; i++) {
            o[i] = r0[i] * NAE_OLA_GAIN;
            r0[i] = r1[i];
            r1[i] = r2[i];
            r2[i] = 0.0f;
        }
        pva_store_block<N>(p, b0, b_end, optr, fs, f - 3, o, lane);
    }
}

// the envelope-only pass of the formant shift at tempo 1 (pv_env_kernel, kernels_pvenv.hip; DESIGN.md §3, "Formant shift"): a wave keeps the FFT
// scratch, the frame's spectrum Y and the L / c' / Ls array in LDS and no phase state — 8 / 8 / 7 / 3 waves per workgroup at N = 512 ... 4096
// (the formant pass 3: 8 / 8 / 5 / 2)
template <int N>
struct PvEnv {
    using A = PvAny<N, true>;
    static constexpr size_t kWave = A::Gm::SCR * sizeof(cf) + A::PAD * sizeof(cf) + A::PAD * sizeof(float);   // scratch, Y, L / c' / Ls
    static constexpr int kMaxWaves = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave);
    static constexpr int kWaves = kMaxWaves < 8 ? kMaxWaves : 8;
    // waves a CU holds: whole workgroups by LDS (24, 8, 7, 3 at N = 512 ... 4096), and no more than the registers hold — the kernel takes 115
    // VGPRs at 512 (4 waves per SIMD: 16) and 165 ... 256 above (2 per SIMD: 8): 16, 8, 7, 3
    static constexpr int kLdsResident = (int)((160 * 1024) / (512 * sizeof(cf) + kWaves * kWave)) * kWaves;
    static constexpr int kVgprResident = N == 512 ? 16 : 8;
    static constexpr int kResident = kLdsResident < kVgprResident ? kLdsResident : kVgprResident;
    static_assert(kWaves >= 1, "a wave's state fits a CU's LDS");
};

} // namespace nae
