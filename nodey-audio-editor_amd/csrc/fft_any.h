// fft_any.h — the canonical FFT of DESIGN.md §3 ("K8 spectrum, every size") as wave-level device code, shared by the size-generic spectrum
// kernel (kernels_spectrum.hip) and the size-generic phase vocoder (kernels_pv_any.hip).
//
// M packed complex points (M = n_fft / 2) as an in-place decimation-in-frequency sequence of radix passes through a wave-private LDS scratch:
//   first pass radix R1 = 2, 4 or 8 (M = R1 * 8^s), twiddle W_M^(l q) on its outputs q >= 1;
//   then s radix-8 passes on blocks of MT = M / (R1 8^(t-1)) points, twiddle W_MT^(l q) = W512[(512/MT) l q] (none when MT = 8).
// At M = 512 this is the FFT512 of the 1024-point kernels pass for pass, so n_fft = 1024 gives their bits.
// A wave transforms G consecutive frames at once (Gm::G).  A pass gives each lane G*M/(64 R) butterflies; its R inputs are read from the
// scratch (the first pass reads them from wherever its caller says) and its R outputs go back to the same positions, so a pass needs no buffer
// of its own and only a wave-level LDS ordering between passes.  Scratch position p lives at p + p/8: 8-byte accesses of the stride-64, stride-8
// and stride-1 passes hit distinct banks.  Output: Z[k] of frame g at padx(g M + zpos(k)).
#pragma once
#include "stft_device.h"

struct nae_ctx;

namespace nae {

struct SpecAnyTables {
    const float* hann;   // Hann_N[n], n < N
    const cf* tn;        // T_N[k] = exp(-2 pi i k / N), k = 0..M
    const cf* wm;        // W_M[k], k < M (only read by the first pass when M > 512)
    const cf* w512;      // W512[k]
};

constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x / 2); }

// geometry of an M-point transform of G frames per wave
template <int M_, int G_>
struct FftGeom {
    static constexpr int M = M_;
    static constexpr int kLog = ilog2c(M);
    static constexpr int R1 = kLog % 3 == 0 ? 8 : (1 << (kLog % 3));
    static constexpr int S8 = (kLog - ilog2c(R1)) / 3;      // radix-8 passes behind the first
    static constexpr int G = G_;                             // frames per wave
    static constexpr int BINS = M + 1;
    static constexpr int SCR = (G * M) + (G * M) / 8;        // padded scratch of one wave, complex
};

// the spectrum's: one wave = max(1, 512/M) frames (every lane has a butterfly in every pass)
template <int N>
struct SpecGeom : FftGeom<N / 2, (N / 2 >= 512 ? 1 : 512 / (N / 2))> {};

__device__ __forceinline__ int padx(int p) { return p + (p >> 3); }

__device__ __forceinline__ cf mul_mi_any(cf a) { return cf{a.y, -a.x}; }

template <int R>
__device__ __forceinline__ void dft_r(cf (&a)[R])
{
    if constexpr (R == 2) {
        const cf s = cf{a[0].x + a[1].x, a[0].y + a[1].y}, d = cf{a[0].x - a[1].x, a[0].y - a[1].y};
        a[0] = s;
        a[1] = d;
    } else if constexpr (R == 4) {
        // the inner layers of DFT8: two radix-2 DIF layers, natural-order output
        const cf s0 = cf{a[0].x + a[2].x, a[0].y + a[2].y}, d0 = cf{a[0].x - a[2].x, a[0].y - a[2].y};
        const cf s1 = cf{a[1].x + a[3].x, a[1].y + a[3].y};
        const cf d1 = mul_mi_any(cf{a[1].x - a[3].x, a[1].y - a[3].y});
        a[0] = cf{s0.x + s1.x, s0.y + s1.y};
        a[2] = cf{s0.x - s1.x, s0.y - s1.y};
        a[1] = cf{d0.x + d1.x, d0.y + d1.y};
        a[3] = cf{d0.x - d1.x, d0.y - d1.y};
    } else {
        dft8_fwd(a);
    }
}

// position of Z[k] after the passes: k = q1 + R1 k', k' with s octal digits -> q1 (M/R1) + (k' digit-reversed)
template <class Gm>
__device__ __forceinline__ int zpos(int k)
{
    const int q1 = k & (Gm::R1 - 1);
    int kp = k >> ilog2c(Gm::R1), rev = 0;
#pragma unroll
    for (int t = 0; t < Gm::S8; t++) {
        rev = (rev << 3) | (kp & 7);
        kp >>= 3;
    }
    return q1 * (Gm::M / Gm::R1) + rev;
}

// how a frame's samples are addressed: frame stride 1 (8-byte pair loads), a stride whose offsets inside one frame fit 32 bits
// (a wave-uniform base plus an unsigned 32-bit lane offset: no 64-bit vector address arithmetic), or any stride
enum { kLoadUnit = 0, kLoadStride32 = 1, kLoadStride64 = 2 };

// first pass: windowed samples from memory -> radix R1 -> twiddle -> scratch
template <class Gm, int kLoad>
__device__ __forceinline__ void any_first_pass(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in,
                                               long long s0, long long hop, int nvalid, int lane)
{
    constexpr int R = Gm::R1, S = Gm::M / R, BPL = Gm::G * Gm::M / (R * 64);
    static_assert(S % 64 == 0, "a first-pass butterfly row is whole waves: its frame is wave-uniform");
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int g = (64 * i) / S;                          // wave-uniform
        const int l = t & (S - 1);
        cf v[R];
        if (g < nvalid) {
            const float* p = in.p + (s0 + g * hop) * in.fs;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int m = l + S * j;
                const float2 h = *reinterpret_cast<const float2*>(tb.hann + 2 * m);
                if (kLoad == kLoadUnit) {
                    const f2u x = *reinterpret_cast<const f2u*>(p + 2 * m);
                    v[j] = cf{x.x * h.x, x.y * h.y};
                } else if (kLoad == kLoadStride32) {
                    const unsigned fs = (unsigned)in.fs, o0 = (unsigned)(2 * m) * fs;
                    v[j] = cf{p[o0] * h.x, p[o0 + fs] * h.y};
                } else {
                    const long long fs = in.fs;
                    v[j] = cf{p[(2 * m) * fs] * h.x, p[(2 * m + 1) * fs] * h.y};
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < R; j++) v[j] = cf{0.0f, 0.0f};
        }
        dft_r<R>(v);
#pragma unroll
        for (int q = 1; q < R; q++) {
            const cf w = Gm::M > 512 ? tb.wm[l * q] : lds_ld(w512l + (512 / Gm::M) * l * q);
            v[q] = cmul_tw(v[q], w);
        }
        const int base = g * Gm::M + l;
#pragma unroll
        for (int j = 0; j < R; j++) lds_st(scr + padx(base + S * j), v[j]);
    }
}

// the same first pass on one frame (G = 1) whose packed input point m the caller supplies: get(m) -> cf
template <class Gm, class Get>
__device__ __forceinline__ void any_first_pass_from(cf* scr, const cf* w512l, const cf* wm, int lane, Get get)
{
    constexpr int R = Gm::R1, S = Gm::M / R, BPL = Gm::M / (R * 64);
    static_assert(Gm::G == 1 && S % 64 == 0, "one frame per wave, whole-wave butterfly rows");
    // two rows in flight: fully unrolled, the loads of all rows (up to 8 at M = 2048) are hoisted in front of the first butterfly and the
    // vocoder kernels around this pass spill
#pragma unroll 2
    for (int i = 0; i < BPL; i++) {
        const int l = lane + 64 * i;
        cf v[R];
#pragma unroll
        for (int j = 0; j < R; j++) v[j] = get(l + S * j);
        dft_r<R>(v);
#pragma unroll
        for (int q = 1; q < R; q++) {
            const cf w = Gm::M > 512 ? wm[l * q] : lds_ld(w512l + (512 / Gm::M) * l * q);
            v[q] = cmul_tw(v[q], w);
        }
#pragma unroll
        for (int j = 0; j < R; j++) lds_st(scr + padx(l + S * j), v[j]);
    }
}

// one radix-8 pass on blocks of MT points.  NB butterflies: fewer than a wave's lanes only when G M < 512 (the vocoder's 512-point frame)
template <class Gm, int MT>
__device__ __forceinline__ void any_pass8(cf* scr, const cf* w512l, int lane)
{
    constexpr int S = MT / 8, NB = Gm::G * Gm::M / 8, BPL = (NB + 63) / 64;
    cf v[BPL][8];
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int base = (t / S) * MT + (t & (S - 1));
        if (NB % 64 == 0 || t < NB) {
#pragma unroll
            for (int j = 0; j < 8; j++) v[i][j] = lds_ld(scr + padx(base + S * j));
        }
    }
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int l = t & (S - 1);
        const int base = (t / S) * MT + l;
        if (NB % 64 == 0 || t < NB) {
            dft8_fwd(v[i]);
            if (MT > 8) {
#pragma unroll
                for (int q = 1; q < 8; q++) v[i][q] = cmul_tw(v[i][q], lds_ld(w512l + (512 / MT) * l * q));
            }
#pragma unroll
            for (int j = 0; j < 8; j++) lds_st(scr + padx(base + S * j), v[i][j]);
        }
    }
}

template <class Gm, int MT>
__device__ __forceinline__ void any_passes8(cf* scr, const cf* w512l, int lane)
{
    if constexpr (MT >= 8) {
        wave_lds_sync();
        any_pass8<Gm, MT>(scr, w512l, lane);
        any_passes8<Gm, MT / 8>(scr, w512l, lane);
    }
}

// canonical r2c split of bin k (0 <= k <= M) from the transform of one frame (zf: its scratch, padx-addressed)
template <class Gm>
__device__ __forceinline__ cf any_rfft_bin(const cf* zf, const cf* tn, int k)
{
    const cf A = lds_ld(zf + padx(zpos<Gm>(k & (Gm::M - 1))));
    const cf B = lds_ld(zf + padx(zpos<Gm>((Gm::M - k) & (Gm::M - 1))));
    const cf E = cf{0.5f * (A.x + B.x), 0.5f * (A.y - B.y)};
    const cf O = cf{0.5f * (A.x - B.x), 0.5f * (A.y + B.y)};
    const cf P = cmul_tw(O, tn[k]);
    return cf{E.x + P.y, E.y - P.x};
}

// Hann_N, T_N, W_M and W512 of a size that passed nae_spectrum_check, built on first use (kernels_spectrum.hip)
int nae_spec_any_tables(nae_ctx* ctx, int n_fft, SpecAnyTables* tb);

} // namespace nae
