// kernels_resample.hip — K7's rate transposer for gfx950: the 16-tap polyphase resampler behind (or, with mix -> pitch, in front of) the phase
// vocoder.  The direct kernel, the tiled kernel (mono; stereo alone or four streams to a workgroup), the kernel that mixes two inputs while it
// stages (the headline step's first launch), the two rules that shape a launch (rs_pick_rot, rs_pick_tile) and the two launchers.
// The vocoder itself: kernels_stft.hip (pass 1, host driver), kernels_pv_any.hip, kernels_pvlock.hip, kernels_pvpipe.hip.
#include "stft_common.h"
#include <stdlib.h>

namespace nae {

// rate transposer: out[j] = sum_i tab(phase)[i] * v[idx - 7 + i],  pos = j * step (Q32.32)
struct RsParams { unsigned long long step_q32; long long src_len; long long out_len; int ch; long long j_begin; int rot; int tile_out; };

// position of output j: the source index and the 32-bit fraction behind it
struct RsPos { long long idx; unsigned frac; };
__device__ __forceinline__ RsPos rs_pos(long long j, unsigned long long step_q32)
{
    const unsigned long long lo = (unsigned long long)j * step_q32;
    const unsigned long long hi = __umul64hi((unsigned long long)j, step_q32);
    return RsPos{(long long)((hi << 32) | (lo >> 32)), (unsigned)lo};
}

// LDS slot of coefficient row ph in the tiled kernels.  Neighbouring outputs advance the phase by a fixed amount (24.2
// rows at the default +3 semitones), and with rows stored in order every other lane of a 16-lane read group lands on the
// same banks (3-way conflicts on each of the 8 coefficient reads of an output).  Rotating the 7-bit row number right by
// `rot` makes the bank group of a row depend on bits rot..rot+3 of the phase; the launcher picks the rotation that
// spreads the lanes of this ratio best (rs_pick_rot).  Row NAE_RS_PHASES (read as "ph + 1" of the last phase) keeps its place.
__host__ __device__ __forceinline__ unsigned rs_slot(unsigned ph, int rot)
{
    return ph >= NAE_RS_PHASES ? ph : (ph >> rot) | ((ph & ((1u << rot) - 1u)) << (7 - rot));
}
static_assert(NAE_RS_PHASES == 128, "rs_slot rotates a 7-bit row number");

__global__ __launch_bounds__(256) void resample_kernel(SigViewD src, RsParams p, long long n_streams,
                                                      const float* __restrict__ tab, OutViewD out)
{
    __shared__ float stab[(NAE_RS_PHASES + 1) * NAE_RS_TAPS];
    for (int i = threadIdx.x; i < (NAE_RS_PHASES + 1) * NAE_RS_TAPS; i += blockDim.x) stab[i] = tab[i];
    __syncthreads();
    const long long j = p.j_begin + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long s = blockIdx.y;
    if (j >= p.out_len) return;
    const auto [idx, frac] = rs_pos(j, p.step_q32);
    const unsigned ph = frac >> 25;
    const float alpha = (float)(frac & 0x1FFFFFFu) * (1.0f / 33554432.0f);
    const float* t0 = stab + ph * NAE_RS_TAPS;
    const float* t1 = t0 + NAE_RS_TAPS;
    float coef[NAE_RS_TAPS];
#pragma unroll
    for (int i = 0; i < NAE_RS_TAPS; i++) coef[i] = t0[i] + alpha * (t1[i] - t0[i]);
    for (int c = 0; c < p.ch; c++) {
        const float* v = src.base + s * src.ss + c * src.cs;
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < NAE_RS_TAPS; i++) {
            const long long m = idx - (NAE_RS_TAPS / 2 - 1) + i;
            const float x = (m >= 0 && m < p.src_len) ? v[m * src.fs] : 0.0f;
            acc += coef[i] * x;
        }
        out.base[s * out.ss + c * out.cs + j * out.fs] = acc;
    }
}

// tiled rate transposer: a 256-thread workgroup produces kRsOut consecutive output frames of one stream; the
// source span it needs (kRsOut*rho + 16 samples per channel) is staged once into LDS with 16-byte loads, the
// 16 taps are read from LDS, and interleaved stereo output leaves as one 8-byte store per frame.
constexpr int kRsOut = 512;                      // output frames per workgroup when the wider tile does not fit.  Round 1: 256 -> 3.6 ms, 512 -> 3.07,
                                                 // 1024 -> 3.4 (C5 mix+transposer; LDS per workgroup sets the occupancy)
constexpr int kRsOutWide = 768;                  // round 4 (16-byte tap reads): 384 -> 2.58 ms, 512 -> 2.44, 768 -> 2.35, 1024 -> 2.70 on one box — three
                                                 // longer-lived workgroups per CU beat five; used while 4 streams of 768 rho + 28 frames fit the
                                                 // 1536-frame staging rows (rho <= 1.96), see rs_pick_tile
constexpr int kRsRow = 20;                       // LDS row stride of the coefficient table (16 taps + 4 pad): a 64-B
                                                 // stride maps every row to one of 4 bank slots (4-way conflicts on b128)
constexpr int kRsMaxSpan = 4096 + 32;            // staged source samples per channel: 512-frame tiles up to floor(512 rho) + 28 <= 4128,
                                                 // i.e. rho < 4101/512 ~ 8.01 (tests/test_gpu_stretch_range.py pins the switch)

// coefficient table -> LDS (rows rotated by rs_slot): 16-byte loads, ALL of a thread's loads requested before the first LDS write.
// (The table is 8 KB per workgroup out of L2; one dword per thread and trip with a wait in every trip — what the first version
// did — put eight serial L2 round trips in front of every workgroup's staging loads.)
// Assumes (checked where it can be): workgroups of kRsThreads threads (every caller's __launch_bounds__), a 16-byte aligned
// table (nae_ctx::rs_tab, an allocation of its own), rows of a whole number of float4.
constexpr int kRsThreads = 256;
constexpr int kRsRowQuads = NAE_RS_TAPS / 4;                                 // float4 per coefficient row
static_assert(NAE_RS_TAPS % 4 == 0 && (kRsRowQuads & (kRsRowQuads - 1)) == 0, "a coefficient row is a power-of-two number of float4");
static_assert(kRsRow % 4 == 0 && kRsRow >= NAE_RS_TAPS, "LDS rows keep 16-byte alignment and hold a whole row");
__device__ __forceinline__ void rs_fill_table(float* stab, const float* __restrict__ tab, int rot)
{
    constexpr int kQuads = (NAE_RS_PHASES + 1) * kRsRowQuads;                // 516 float4
    constexpr int kTrips = (kQuads + kRsThreads - 1) / kRsThreads;
    const float4* t4 = reinterpret_cast<const float4*>(tab);
    float4 v[kTrips];
#pragma unroll
    for (int u = 0; u < kTrips; u++) {
        const int i = threadIdx.x + kRsThreads * u;
        v[u] = i < kQuads ? t4[i] : float4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int u = 0; u < kTrips; u++) {
        const int i = threadIdx.x + kRsThreads * u;
        if (i < kQuads) *reinterpret_cast<float4*>(stab + rs_slot(i / kRsRowQuads, rot) * kRsRow + 4 * (i % kRsRowQuads)) = v[u];
    }
}


// Stereo taps.  The two channels are staged INTERLEAVED in LDS (one read feeds both accumulators), and NS streams share a workgroup:
// the 16 interpolated coefficients of an output depend on its position only, so they are built once (8 x 128-bit LDS reads, 48
// instructions) and applied to every stream.
// The taps are read 16 BYTES at a time (round 4).  With one ds_read_b64 per tap (rounds 1-3) the 32 lanes of a read group span 32 rho
// frames (38 at +3 semitones) = more words than the 64 banks: every tap read was a 2-way conflict, half of the kernel's LDS cycles
// (profiles/r03_v3_sq_stalls.md: bank-conflict share 0.49 at 86 % LDS-busy).  A ds_read_b128 is served 16 lanes at a time and moves
// 256 B per LDS cycle: 16 CONSECUTIVE outputs span 16 rho + 1 frames = at most 40 words at rho <= 1.2 — conflict-free — if
//   (i)  the 16 lanes of a hardware group hold consecutive outputs: the groups are not contiguous in the wave ({0-3,12-15,20-27},
//        {4-11,16-19,28-31} and the same + 32: MI355X_MICROARCH.md §LDS), so the output a lane works on is permuted (rs_slot_of_lane);
//   (ii) the reads are 16-byte aligned: a lane whose first tap frame o is odd reads from o - 1 and SHIFTS ITS COEFFICIENTS instead of
//        its data — cz[i'] = c[i' - (o & 1)], 17 positions, built once per output and used for all NS streams; the end positions
//        0 and 16 belong to one parity each and are added under a select, so a non-finite sample outside the window stays outside.
// The accumulation order per output is unchanged (tap 0 first, separate multiply and add): same bits.
__device__ __forceinline__ int rs_slot_of_lane(int lane)
{
    const int l5 = lane & 31;
    const bool b = (l5 >= 4 && l5 < 12) || (l5 >= 16 && l5 < 20) || l5 >= 28;        // second group of the half-wave
    const int pos = l5 < 4 ? l5 : l5 < 12 ? l5 - 4 : l5 < 16 ? l5 - 8 : l5 < 20 ? l5 - 8 : l5 < 28 ? l5 - 12 : l5 - 16;
    return (lane & 32) + (b ? 16 : 0) + pos;
}

template <int NS>
__device__ __forceinline__ void rs_apply_stereo(const float* stab, const float* stage, int span_alloc, const RsParams& p, long long j0,
                                                     long long j1, long long m_lo, const OutViewD& out, long long s0, long long n_streams)
{
    const bool out_pair = (out.cs == 1) && (out.fs == 2) && ((out.ss & 1) == 0) && ((reinterpret_cast<uintptr_t>(out.base) & 7) == 0);
    const int slot = (int)(threadIdx.x & ~63u) + rs_slot_of_lane((int)(threadIdx.x & 63u));
    for (long long jb = j0; jb < j1; jb += 256) {
        const long long j = jb + slot;
        const bool live = j < j1;
        const long long jj = live ? j : j1 - 1;                   // idle lanes repeat the last output (reads stay inside the staged span)
        const auto [idx, frac] = rs_pos(jj, p.step_q32);
        const unsigned ph = frac >> 25;
        const float alpha = (float)(frac & 0x1FFFFFFu) * (1.0f / 33554432.0f);
        const float4* t0 = reinterpret_cast<const float4*>(stab + rs_slot(ph, p.rot) * kRsRow);
        const float4* t1 = reinterpret_cast<const float4*>(stab + rs_slot(ph + 1, p.rot) * kRsRow);
        float coef[NAE_RS_TAPS];
#pragma unroll
        for (int q = 0; q < NAE_RS_TAPS / 4; q++) {
            const float4 a = t0[q], b = t1[q];
            coef[4 * q + 0] = a.x + alpha * (b.x - a.x);
            coef[4 * q + 1] = a.y + alpha * (b.y - a.y);
            coef[4 * q + 2] = a.z + alpha * (b.z - a.z);
            coef[4 * q + 3] = a.w + alpha * (b.w - a.w);
        }
        const int o = (int)(idx - (NAE_RS_TAPS / 2 - 1) - m_lo);
        const bool odd = (o & 1) != 0;
        float cz[NAE_RS_TAPS + 1];
        cz[0] = coef[0];
#pragma unroll
        for (int i = 1; i < NAE_RS_TAPS; i++) cz[i] = odd ? coef[i - 1] : coef[i];
        cz[NAE_RS_TAPS] = coef[NAE_RS_TAPS - 1];
        const int q0 = (o - (odd ? 1 : 0)) >> 1;                  // float4 index of the aligned pair of frames
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (s0 + k < n_streams) {
                const float4* st = reinterpret_cast<const float4*>(stage + (size_t)k * 2 * span_alloc) + q0;
                float4 x[NAE_RS_TAPS / 2];
#pragma unroll
                for (int t = 0; t < NAE_RS_TAPS / 2; t++) x[t] = st[t];
                const float2 xe = *reinterpret_cast<const float2*>(st + NAE_RS_TAPS / 2);      // frame 16 of the aligned window
                // position 0: even lanes only
                const float e0 = 0.0f + cz[0] * x[0].x, e1 = 0.0f + cz[0] * x[0].y;
                float a0 = odd ? 0.0f : e0, a1 = odd ? 0.0f : e1;
#pragma unroll
                for (int i = 1; i < NAE_RS_TAPS; i++) {
                    const float xl = (i & 1) ? x[i >> 1].z : x[i >> 1].x, xr = (i & 1) ? x[i >> 1].w : x[i >> 1].y;
                    a0 += cz[i] * xl;
                    a1 += cz[i] * xr;
                }
                // position 16: odd lanes only
                const float f0 = a0 + cz[NAE_RS_TAPS] * xe.x, f1 = a1 + cz[NAE_RS_TAPS] * xe.y;
                a0 = odd ? f0 : a0;
                a1 = odd ? f1 : a1;
                if (live) {
                    float* ob = out.base + (s0 + k) * out.ss;
                    if (out_pair) {
                        *reinterpret_cast<float2*>(ob + 2 * j) = float2{a0, a1};
                    } else {
                        ob[j * out.fs] = a0;
                        ob[out.cs + j * out.fs] = a1;
                    }
                }
            }
        }
    }
}

template <bool kStereo, int NS>
__global__ __launch_bounds__(kRsThreads) void resample_tile_kernel(SigViewD src, RsParams p, const float* __restrict__ tab,
                                                           OutViewD out, int span_alloc, long long n_streams)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    float* stab = reinterpret_cast<float*>(rs_smem);                           // (PHASES+1) x kRsRow
    float* stage = stab + (NAE_RS_PHASES + 1) * kRsRow;                        // stereo: [NS][span_alloc][2]; else [ch][span_alloc]
    rs_fill_table(stab, tab, p.rot);
    const long long s0 = (long long)blockIdx.y * NS;
    const long long j0 = p.j_begin + (long long)blockIdx.x * p.tile_out;
    long long j1 = j0 + p.tile_out;
    if (j1 > p.out_len) j1 = p.out_len;
    // source window [m_lo, m_hi) of this tile, m_lo rounded down to a multiple of 4 samples
    // (rs_pos written out: both products in front of both indices is the order the two stereo instantiations' scalar code was scheduled from,
    // and through the helper their instructions move)
    const unsigned long long lo0 = (unsigned long long)j0 * p.step_q32, hi0 = __umul64hi((unsigned long long)j0, p.step_q32);
    const unsigned long long lo1 = (unsigned long long)(j1 - 1) * p.step_q32, hi1 = __umul64hi((unsigned long long)(j1 - 1), p.step_q32);
    const long long idx_first = (long long)((hi0 << 32) | (lo0 >> 32));
    const long long idx_last = (long long)((hi1 << 32) | (lo1 >> 32));
    const long long m_lo = (idx_first - (NAE_RS_TAPS / 2 - 1)) & ~3ll;          // floor to 4 (arithmetic on negatives too)
    const long long m_hi = idx_last + NAE_RS_TAPS / 2 + 1;
    const int span = (int)(m_hi - m_lo);
    if (kStereo) {
#pragma unroll 1
        for (int k = 0; k < NS; k++) {
            if (s0 + k >= n_streams) break;
            const float* v0 = src.base + (s0 + k) * src.ss;
            const float* v1 = v0 + src.cs;
            float* stg = stage + (size_t)k * 2 * span_alloc;
            const bool vec = (src.fs == 1) && (((reinterpret_cast<uintptr_t>(v0) | reinterpret_cast<uintptr_t>(v1)) & 15) == 0);
            if (vec) {
                for (int i = 4 * threadIdx.x; i < span; i += 4 * 256) {
                    const long long m = m_lo + i;
                    float4 x, y;
                    if (m >= 0 && m + 4 <= p.src_len) {
                        x = *reinterpret_cast<const float4*>(v0 + m);
                        y = *reinterpret_cast<const float4*>(v1 + m);
                    } else {
                        float xe[4], ye[4];
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const bool ok = (m + e >= 0) && (m + e < p.src_len);
                            xe[e] = ok ? v0[m + e] : 0.0f;
                            ye[e] = ok ? v1[m + e] : 0.0f;
                        }
                        x = float4{xe[0], xe[1], xe[2], xe[3]};
                        y = float4{ye[0], ye[1], ye[2], ye[3]};
                    }
                    *reinterpret_cast<float4*>(stg + 2 * i) = float4{x.x, y.x, x.y, y.y};
                    *reinterpret_cast<float4*>(stg + 2 * i + 4) = float4{x.z, y.z, x.w, y.w};
                }
            } else {
                for (int i = threadIdx.x; i < span; i += 256) {
                    const long long m = m_lo + i;
                    const bool ok = m >= 0 && m < p.src_len;
                    *reinterpret_cast<float2*>(stg + 2 * i) = float2{ok ? v0[m * src.fs] : 0.0f, ok ? v1[m * src.fs] : 0.0f};
                }
            }
        }
    } else {
        const float* v0 = src.base + s0 * src.ss;
        for (int c = 0; c < p.ch; c++) {
            const float* v = v0 + c * src.cs;
            float* st = stage + c * span_alloc;
            for (int i = threadIdx.x; i < span; i += 256) {
                const long long m = m_lo + i;
                st[i] = (m >= 0 && m < p.src_len) ? v[m * src.fs] : 0.0f;
            }
        }
    }
    __syncthreads();
    if (kStereo) {
        rs_apply_stereo<NS>(stab, stage, span_alloc, p, j0, j1, m_lo, out, s0, n_streams);
    } else {
        for (long long j = j0 + threadIdx.x; j < j1; j += 256) {
            const auto [idx, frac] = rs_pos(j, p.step_q32);
            const unsigned ph = frac >> 25;
            const float alpha = (float)(frac & 0x1FFFFFFu) * (1.0f / 33554432.0f);
            const float* t0 = stab + rs_slot(ph, p.rot) * kRsRow;
            const float* t1 = stab + rs_slot(ph + 1, p.rot) * kRsRow;
            float coef[NAE_RS_TAPS];
#pragma unroll
            for (int i = 0; i < NAE_RS_TAPS; i++) coef[i] = t0[i] + alpha * (t1[i] - t0[i]);
            const int o = (int)(idx - (NAE_RS_TAPS / 2 - 1) - m_lo);
            for (int c = 0; c < p.ch; c++) {
                const float* st = stage + c * span_alloc + o;
                float a = 0.0f;
#pragma unroll
                for (int i = 0; i < NAE_RS_TAPS; i++) a += coef[i] * st[i];
                out.base[s0 * out.ss + c * out.cs + j * out.fs] = a;
            }
        }
    }
}

// mix(2) fused into the transposer's staging (graph: mix -> pitch with the transposer first).  The tile's source span
// is mixed on the fly from the two interleaved inputs — out = (0 + a*va) + b*vb, the reference's order
// (audio-amix.cpp:293-307) — written to the mix node's output for the frames this tile owns, and staged for the taps.
// Saves the mix kernel's launch and one read of the mix buffer.
struct MixFuseD {
    const float* a; long long a_ss;       // interleaved stereo, 16-byte aligned
    const float* b; long long b_ss;       // same; b_ss = 0: one buffer shared by every stream
    float va, vb;
    float* mix; long long mix_ss, mix_cs, mix_fs;
};
inline MixFuseD at_stream(MixFuseD f, size_t s0)
{
    f.a += (long long)s0 * f.a_ss;
    f.b += (long long)s0 * f.b_ss;
    f.mix += (long long)s0 * f.mix_ss;
    return f;
}

template <int NS>
__global__ __launch_bounds__(kRsThreads) void mix_resample_tile_kernel(MixFuseD f, RsParams p, const float* __restrict__ tab, OutViewD out,
                                                               int span_alloc, long long n_streams)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    float* stab = reinterpret_cast<float*>(rs_smem);
    float* stage = stab + (NAE_RS_PHASES + 1) * kRsRow;
    const long long s0 = (long long)blockIdx.y * NS;
    const long long j0 = (long long)blockIdx.x * p.tile_out;
    long long j1 = j0 + p.tile_out;
    const bool last = j1 >= p.out_len;
    if (last) j1 = p.out_len;
    auto idx_of = [&](long long j) { return rs_pos(j, p.step_q32).idx; };
    const long long idx_first = idx_of(j0), idx_last = idx_of(j1 - 1);
    const long long m_lo = (idx_first - (NAE_RS_TAPS / 2 - 1)) & ~3ll;
    const long long m_hi = idx_last + NAE_RS_TAPS / 2 + 1;
    // frames of the mix output this tile writes: from its first output's position to the next tile's
    const long long own_lo = blockIdx.x == 0 ? 0 : idx_first;
    const long long own_hi = last ? p.src_len : idx_of(j1);
    const bool mix_planar = f.mix_fs == 1;
    // four frames per thread and trip (a 512-output tile spans ~640 source frames: one trip).  The loads of all NS
    // streams are issued before anything is stored — the staging is bound by round trips to HBM — and the mix leaves
    // as 16-byte stores per plane, like the stand-alone mix kernel's.
    const long long m_end = last ? (p.src_len > m_hi ? p.src_len : m_hi) : m_hi;
    auto load = [&](long long m, float4 (&xa)[NS][2], float4 (&xb)[NS][2]) {
        const bool inside = m >= 0 && m + 4 <= p.src_len;
#pragma unroll
        for (int k = 0; k < NS; k++) {
            xa[k][0] = xa[k][1] = xb[k][0] = xb[k][1] = float4{0.0f, 0.0f, 0.0f, 0.0f};
            if (s0 + k < n_streams) {
                const float* __restrict__ a = f.a + (s0 + k) * f.a_ss;
                const float* __restrict__ b = f.b + (s0 + k) * f.b_ss;
                if (inside) {
                    xa[k][0] = *reinterpret_cast<const float4*>(a + 2 * m);
                    xa[k][1] = *reinterpret_cast<const float4*>(a + 2 * m + 4);
                    xb[k][0] = *reinterpret_cast<const float4*>(b + 2 * m);
                    xb[k][1] = *reinterpret_cast<const float4*>(b + 2 * m + 4);
                } else {
                    float ta[8], tb[8];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const bool ok = m + e >= 0 && m + e < p.src_len;
                        ta[2 * e] = ok ? a[2 * (m + e)] : 0.0f;
                        ta[2 * e + 1] = ok ? a[2 * (m + e) + 1] : 0.0f;
                        tb[2 * e] = ok ? b[2 * (m + e)] : 0.0f;
                        tb[2 * e + 1] = ok ? b[2 * (m + e) + 1] : 0.0f;
                    }
                    xa[k][0] = float4{ta[0], ta[1], ta[2], ta[3]}; xa[k][1] = float4{ta[4], ta[5], ta[6], ta[7]};
                    xb[k][0] = float4{tb[0], tb[1], tb[2], tb[3]}; xb[k][1] = float4{tb[4], tb[5], tb[6], tb[7]};
                }
            }
        }
    };
    auto finish = [&](long long m, const float4 (&xa)[NS][2], const float4 (&xb)[NS][2]) {
        bool own[4], in[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            own[e] = m + e >= own_lo && m + e < own_hi;
            in[e] = m + e >= 0 && m + e < p.src_len;
        }
        const bool own_all = own[0] && own[3];
#pragma unroll
        for (int k = 0; k < NS; k++) {
            if (s0 + k < n_streams) {
                float y[8];
                const float av[8] = {xa[k][0].x, xa[k][0].y, xa[k][0].z, xa[k][0].w, xa[k][1].x, xa[k][1].y, xa[k][1].z, xa[k][1].w};
                const float bv[8] = {xb[k][0].x, xb[k][0].y, xb[k][0].z, xb[k][0].w, xb[k][1].x, xb[k][1].y, xb[k][1].z, xb[k][1].w};
#pragma unroll
                for (int i = 0; i < 8; i++) y[i] = in[i >> 1] ? (0.0f + av[i] * f.va) + bv[i] * f.vb : 0.0f;
                float* stg = stage + (size_t)k * 2 * span_alloc + 2 * (m - m_lo);
                if (m + 3 < m_hi) {
                    *reinterpret_cast<float4*>(stg) = float4{y[0], y[1], y[2], y[3]};
                    *reinterpret_cast<float4*>(stg + 4) = float4{y[4], y[5], y[6], y[7]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (m + e < m_hi) *reinterpret_cast<float2*>(stg + 2 * e) = float2{y[2 * e], y[2 * e + 1]};
                }
                float* __restrict__ mx = f.mix + (s0 + k) * f.mix_ss;
                if (own_all && mix_planar) {
                    *reinterpret_cast<float4*>(mx + m) = float4{y[0], y[2], y[4], y[6]};
                    *reinterpret_cast<float4*>(mx + f.mix_cs + m) = float4{y[1], y[3], y[5], y[7]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (own[e]) { mx[(m + e) * f.mix_fs] = y[2 * e]; mx[f.mix_cs + (m + e) * f.mix_fs] = y[2 * e + 1]; }
                }
            }
        }
    };
    // first trip: its HBM loads are requested, THEN the coefficient table (L2) is fetched and laid out while they travel
    {
        float4 xa[NS][2], xb[NS][2];
        const long long m = m_lo + 4 * threadIdx.x;
        const bool has = m < m_end;
        if (has) load(m, xa, xb);
        rs_fill_table(stab, tab, p.rot);
        if (has) finish(m, xa, xb);
    }
    for (long long m = m_lo + 4 * threadIdx.x + 4 * 256; m < m_end; m += 4 * 256) {
        float4 xa[NS][2], xb[NS][2];
        load(m, xa, xb);
        finish(m, xa, xb);
    }
    __syncthreads();
    rs_apply_stereo<NS>(stab, stage, span_alloc, p, j0, j1, m_lo, out, s0, n_streams);
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// rotation of the coefficient rows (rs_slot) with the fewest bank conflicts for this ratio: the 8 x 128-bit reads of an
// output are served 16 lanes at a time, a row's bank group is 5 * slot mod 16; count the worst multiplicity per group of
// lanes over the first 256 outputs
static int rs_pick_rot(unsigned long long step_q32)
{
    int best = 0;
    long best_cost = -1;
    for (int rot = 0; rot < 4; rot++) {
        long cost = 0;
        for (int g = 0; g < 16; g++) {
            int n0[16] = {0}, n1[16] = {0};
            unsigned seen0[16], seen1[16];          // distinct rows only: lanes reading the same row share the access
            for (int l = 0; l < 16; l++) {
                const unsigned long long pos = (unsigned long long)(16 * g + l) * step_q32;
                const unsigned ph = (unsigned)(pos & 0xFFFFFFFFull) >> 25;
                const unsigned s0 = rs_slot(ph, rot), s1 = rs_slot(ph + 1, rot);
                bool dup0 = false, dup1 = false;
                for (int k = 0; k < l; k++) { dup0 |= seen0[k] == s0; dup1 |= seen1[k] == s1; }
                seen0[l] = s0; seen1[l] = s1;
                if (!dup0) n0[(5 * s0) & 15]++;
                if (!dup1) n1[(5 * s1) & 15]++;
            }
            int m0 = 0, m1 = 0;
            for (int b = 0; b < 16; b++) { m0 = n0[b] > m0 ? n0[b] : m0; m1 = n1[b] > m1 ? n1[b] : m1; }
            cost += m0 + m1;
        }
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = rot; }
    }
    return best;
}

// output frames per transposer workgroup and the staging row it needs (frames per channel, a multiple of 4)
static int rs_pick_tile(double rho, long long* span_need)
{
    auto need = [&](int tile) { return (long long)(tile * rho) + NAE_RS_TAPS + 8 + 4; };   // + 4: the aligned 16-byte tap reads look one pair of frames further
    const int tile = need(kRsOutWide) <= 1536 ? kRsOutWide : kRsOut;
    *span_need = need(tile);
    return tile;
}

// outputs [j_begin, j_end)
int nae_launch_resample(nae_ctx* ctx, const nae_stretch_plan* pl, const nae_sig* src, size_t src_len, int ch,
                        size_t n_streams, const float* d_tab, const nae_sig* out, size_t j_begin, size_t j_end)
{
    if (j_end <= j_begin || n_streams == 0) return NAE_OK;
    const size_t count = j_end - j_begin;
    // tiled kernel while one tile's source span fits the staging buffer (rho < 4101/512 ~ 8.01), else the direct kernel
    const double rho = (double)pl->step_q32 / 4294967296.0;
    long long span_need = 0;
    const int tile_out = rs_pick_tile(rho, &span_need);
    RsParams p{pl->step_q32, (long long)src_len, (long long)j_end, ch, (long long)j_begin, rs_pick_rot(pl->step_q32), tile_out};
    const bool tiled = span_need <= kRsMaxSpan && !ctx->dbg_rs_direct;
    const int span_alloc = (int)((span_need + 3) & ~3ll);
    // stereo batches: 4 streams per workgroup share the per-output coefficients (if their staging fits LDS)
    const int group = (tiled && ch == 2 && n_streams >= 4 && span_alloc <= 1536 && !ctx->dbg_rs_single) ? 4 : 1;
    const size_t lds = ((NAE_RS_PHASES + 1) * kRsRow + (size_t)ch * span_alloc * group) * sizeof(float);
    const unsigned gx = tiled ? (unsigned)((count + tile_out - 1) / tile_out) : (unsigned)((count + 255) / 256);
    return for_stream_slices(n_streams, group, [&](size_t s0, size_t ns) {
        const SigViewD sv = at_stream(to_view(src), s0);
        const OutViewD ov = at_stream(to_out(out), s0);
        const dim3 grid(gx, (unsigned)((ns + group - 1) / group));
        if (!tiled) return nae_launch_grid(ctx, "resample_kernel", resample_kernel, grid, dim3(256), 0, sv, p, (long long)ns, d_tab, ov);
        auto tile = [&](auto kernel) {
            return nae_launch_grid(ctx, "resample_tile_kernel", kernel, grid, dim3(kRsThreads), lds, sv, p, d_tab, ov, span_alloc, (long long)ns);
        };
        return group == 4 ? tile(resample_tile_kernel<true, 4>) : ch == 2 ? tile(resample_tile_kernel<true, 1>) : tile(resample_tile_kernel<false, 1>);
    });
}

// mix(2) + transposer in one launch (see mix_resample_tile_kernel).  Returns 1 when the shapes do not fit the fused
// kernel (the caller then runs the two nodes separately), 0 on success, < 0 on error.
int nae_launch_mix_resample(nae_ctx* ctx, const nae_stretch_plan* pl, const nae_sig* a, const nae_sig* b, float va, float vb,
                            const nae_sig* mix_out, size_t S, size_t n_streams, const float* d_tab, const nae_sig* out)
{
    const double rho = (double)pl->step_q32 / 4294967296.0;
    long long span_need = 0;
    const int tile_out = rs_pick_tile(rho, &span_need);
    const int span_alloc = (int)((span_need + 3) & ~3ll);
    auto inter16 = [](const nae_sig* v) {
        return v->chan_stride == 1 && v->frame_stride == 2 && (reinterpret_cast<uintptr_t>(v->base) & 15) == 0 && (v->stream_stride & 3) == 0;
    };
    // planar mix output: 16-byte stores per plane; interleaved (or any other) layout: scalar stores
    const bool mix_ok = mix_out->frame_stride != 1 ||
                        ((reinterpret_cast<uintptr_t>(mix_out->base) & 15) == 0 && (mix_out->stream_stride & 3) == 0 &&
                         (mix_out->chan_stride & 3) == 0);
    if (ctx->dbg_no_mix_fuse || !inter16(a) || !inter16(b) || !mix_ok || span_need > kRsMaxSpan || span_alloc > 1536 || n_streams == 0 ||
        pl->mid_len == 0 || S == 0)
        return 1;
    RsParams p{pl->step_q32, (long long)S, (long long)pl->mid_len, 2, 0, rs_pick_rot(pl->step_q32), tile_out};
    const size_t lds = ((NAE_RS_PHASES + 1) * kRsRow + (size_t)2 * span_alloc * 4) * sizeof(float);
    const unsigned gx = (unsigned)((pl->mid_len + tile_out - 1) / tile_out);
    const MixFuseD f{static_cast<const float*>(a->base), (long long)a->stream_stride, static_cast<const float*>(b->base), (long long)b->stream_stride,
                     va, vb, static_cast<float*>(mix_out->base), (long long)mix_out->stream_stride, (long long)mix_out->chan_stride,
                     (long long)mix_out->frame_stride};
    return for_stream_slices(n_streams, 4, [&](size_t s0, size_t ns) {
        return nae_launch_grid(ctx, "mix_resample_tile_kernel", mix_resample_tile_kernel<4>, dim3(gx, (unsigned)((ns + 3) / 4)), dim3(kRsThreads), lds,
                               at_stream(f, s0), p, d_tab, at_stream(to_out(out), s0), span_alloc, (long long)ns);
    });
}
