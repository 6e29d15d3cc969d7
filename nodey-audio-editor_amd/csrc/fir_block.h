// fir_block.h — the two halves of an overlap-save block ("K9 FIR filter", steps 2 and 4-5) as wave-level device code, shared by the
// FIR filter (kernels_fir.hip) and the long convolution (kernels_conv.hip): the geometry Fir<N>, the tile head and the carried half block, the
// r2c of a block into the wave's scratch, and the c2r of a spectrum Y with the store of the block's second half.
#pragma once
#include "pv_any.h"

namespace nae {

template <int N>
struct Fir {
    static constexpr int M = N / 2, B = N / 2, BINS = M + 1;
    static constexpr int PAD = (BINS + 7) & ~7;           // complex per spectrum Y of a wave
    static constexpr int NB = M / 64 + 1;                 // bins per lane: k = lane + 64 r; r = NB - 1 is bin M (lane 0)
    static constexpr int KP = M / 128;                    // packed points per lane in a half block: m = lane + 64 j
    using Gm = FftGeom<M, 1>;
    static constexpr size_t kWave = (Gm::SCR + PAD + M / 2) * sizeof(cf);   // scratch, Y, the carried half block
    static constexpr int kMaxWaves = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave);
    static constexpr int kWaves = kMaxWaves < 8 ? kMaxWaves : 8;           // 8, 8, 7, 3 waves per workgroup at N = 512 ... 4096 (PvEnv<N>'s)
    // waves a CU holds: whole workgroups by LDS (24, 8, 7, 3), and no more than the registers hold — `make resources`: 79 / 84 VGPRs at 512 (unit /
    // any stride: six / five waves per SIMD, so two workgroups always fit and a third only sometimes), 108 ... 251 above: 16, 8, 7, 3
    static constexpr int kLdsResident = (int)((160 * 1024) / (512 * sizeof(cf) + kWaves * kWave)) * kWaves;
    static constexpr int kResident = kLdsResident < 16 ? kLdsResident : 16;
    static_assert(kWaves >= 1, "a wave's state fits a CU's LDS");
};

// packed point (x[i0], x[i0 + 1]) of one stream-channel; `inside`: both lie in [0, len) (wave-uniform)
template <bool kUnit>
__device__ __forceinline__ cf fir_load_pair(const float* p, long long fs, long long len, long long i0, bool inside)
{
    if (inside) {
        if (kUnit) {
            const f2u x = *reinterpret_cast<const f2u*>(p + i0);
            return cf{x.x, x.y};
        }
        return cf{p[i0 * fs], p[(i0 + 1) * fs]};
    }
    return cf{(i0 >= 0 && i0 < len) ? p[i0 * fs] : 0.0f, (i0 + 1 >= 0 && i0 + 1 < len) ? p[(i0 + 1) * fs] : 0.0f};
}

// tile head: the half block in front of block b0 (zero in front of the signal; inside it otherwise: block b0 exists, so b0 B < in_len)
template <int N, bool kUnit>
__device__ __forceinline__ void fir_tile_head(cf* cw, const float* ip, long long fs, long long in_len, long long b0, int lane)
{
    using F = Fir<N>;
#pragma unroll
    for (int j = 0; j < F::KP; j++) {
        const int m = lane + 64 * j;
        lds_st(cw + m, b0 > 0 ? fir_load_pair<kUnit>(ip, fs, in_len, (b0 - 1) * F::B + 2 * m, true) : cf{0.0f, 0.0f});
    }
}

// U = r2c_N(u) of the block at sample n0, left in the scratch for any_rfft_bin.  Point m of the first half comes from the carry; point m of the
// second half is read from memory and replaces carry[m - M/2].  A butterfly row asks for m = l + S j in increasing j, so the lane that reads
// carry[m - M/2] (j < R1 / 2) is the one that overwrites it afterwards (j >= R1 / 2): the LDS accesses are volatile and stay in that order.
template <int N, bool kUnit>
__device__ __forceinline__ void fir_block_r2c(cf* scr, cf* cw, const cf* w512l, const SpecAnyTables& tb, const float* ip, long long fs,
                                              long long in_len, long long n0, bool full, int lane)
{
    using Gm = typename Fir<N>::Gm;
    constexpr int M = Fir<N>::M;
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, [&](int m) -> cf {
        if (m < M / 2) return lds_ld(cw + m);
        const cf x = fir_load_pair<kUnit>(ip, fs, in_len, n0 + 2 * (m - M / 2), full);
        lds_st(cw + (m - M / 2), x);
        return x;
    });
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
}

// v = c2r_N(Y): split with T_N, conjugate, forward FFT_M, scale by 1 / M and conjugate back (pva_synth_frame's); then y[b B + n] = v[B + n]:
// this lane's samples 2 (lane + 64 j) + {0, 1} of the block
template <int N, bool kUnit>
__device__ __forceinline__ void fir_block_c2r_store(cf* scr, const cf* ys, const cf* w512l, const SpecAnyTables& tb, float* op, long long ofs,
                                                    long long in_len, long long n0, bool full, int lane)
{
    using F = Fir<N>;
    using Gm = typename F::Gm;
    constexpr int M = F::M;
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
            if (n < in_len) op[n * ofs] = v0;
            if (n + 1 < in_len) op[(n + 1) * ofs] = v1;
        }
    }
}

// H = r2c_N(h zero-padded to N), bins 0 ... M, of the n_real <= N leading reals at h (the rest are zeros), on one wave
template <int N>
__device__ __forceinline__ void fir_taps_r2c(cf* scr, const cf* w512l, const SpecAnyTables& tb, const float* h, int n_real, cf* hspec, int lane)
{
    using F = Fir<N>;
    using Gm = typename F::Gm;
    any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, [&](int m) -> cf { return 2 * m < n_real ? cf{h[2 * m], h[2 * m + 1]} : cf{0.0f, 0.0f}; });
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();
#pragma unroll 1
    for (int k = lane; k <= F::M; k += 64) hspec[k] = any_rfft_bin<Gm>(scr, tb.tn, k);
}

} // namespace nae
