// kernels_lim.hip — K22, the true-peak look-ahead limiter ("K22 limiter") for gfx950: K14's 4 x 12-tap oversampler as the level
// detector, K12's demand, sliding maximum and release scan, and an attack that is a moving sum of integers, so the gain is smooth and the
// sample ceiling holds for any release and look-ahead.
//
// One wave per detector walks its chunks of 64 lanes x 16 samples in order (chunk_stage.h).  A detector is a stream-channel, or with `link`
// a stereo stream: the wave then reads and writes both channels (DC = 2).  The walk is one chunk ahead with steps 1 and 2, as K12's is.
// Step 1 with `true_peak`: the stage holds the chunk between the 16 samples in front of it (row 0) and the 16 behind it (row 65), a lane
// reads the 6 samples to either side of its own 16 and runs the four phases at the 17 positions n + 5 ... n + 6 its samples need, so the
// demand of a chunk is whole when its level pass ends and steps 3 and 4 stand on aligned lanes.  That costs a seventeenth FIR position per
// lane and reads 6 samples past the chunk; a handle waits for them (the detector's reach D = 6) and its FIFO keeps the chunk in front.
// Steps 3 and 4 are K12's, the two functions dyn_walk runs them with (dyn_steps.h: dyn_lookahead_max, dyn_release_scan): lifting them left
// K12, K15, K19 and K20 at their `make resources` figures, line for line.  Step 5: a lane forms the prefix of its 16 q, the wave scans the
// lane totals in six steps of 64-bit integers, a running total is carried from chunk to chunk (all modulo 2^64: differences of prefix sums are exact), and the prefix sums of two chunks stand in
// a second LDS ring at the 17-to-a-lane stride; W[n] is the lane's own prefix less the ring's word at n - la - 1.  The hold of q[0] seeds the
// ring's other slot at chunk 0.  The carries (y1, the running total) stay in registers between chunks; a handle keeps them and the last
// chunk's 1024 prefix sums in device memory between launches.  Built with -ffp-contract=off: every step is one IEEE operation in the order of
// the CPU statement (tests/lim_ref/ref_lim.c).
#include "dyn_steps.h"
#include <array>
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kLimPhases = NAE_LOUD_TP_PHASES, kLimTaps = NAE_LOUD_TP_TAPS, kLimTapCount = kLimPhases * kLimTaps;
constexpr int kLimReach = NAE_LIM_TP_REACH;                 // D: samples behind n the level of n reads, and as many in front
constexpr int kLimXs = kChunkT + 2 * kLimReach;             // a lane's samples with the 6 to either side
constexpr int kLimPos = kChunkT + 1;                        // the FIR positions n + 5 ... n + 6 of a lane's 16 n
constexpr int kLimStage = (kChunkC / kChunkT + 2) * kChunkStride;   // rows 0 ... 65: the 16 in front, lane l's at row l + 1, the 16 behind
constexpr int kLimStateWords = 2 + kChunkC;                 // a detector's handle state: y1's bits, the running total, 1024 prefix sums
static_assert(kLimTaps - 1 == 2 * kLimReach - 1 && kLimReach <= kChunkT, "v_p[m] reads x[m - 11 ... m]; m = n + 5, n + 6");
static_assert(NAE_LIM_MAX_LOOKAHEAD + kLimReach <= kChunkC, "DESIGN.md §3, K22: la + D within one chunk");
static_assert(kLimStage >= kChunkStage, "the stage serves dyn_load too");

enum { kLimCeiling, kLimGain, kLimAr, kLimOmr, kLimDenom, kLimParams };
struct LimParams {
    long long in_len;      // samples of a signal: reads at or past in_len and below 0 give zero, samples past in_len are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_det;       // detectors: one wave each
    double v[kLimParams];  // kLimCeiling ... kLimDenom = (la + 1) 2^24
    float taps[kLimTapCount];   // K14's, [phase][k]
    int ch, la, tp;
};

// step 1 with true_peak: L[n] = max(|x[n]|, e[n + 5], e[n + 6]) of the lane's 16 samples of chunk ck, over DC channels at kp (cs apart)
template <int DC>
__device__ inline void lim_tp_level(float* stage, const float* taps, const float* kp, long long cs, long long fs, long long in_len, long long ck,
                                    int lane, float (&L)[kChunkT])
{
    const long long n0 = ck * kChunkC;
#pragma unroll
    for (int c = 0; c < DC; c++) {
        const float* cp = kp + c * cs;
        chunk_load<true, 4>(stage + kChunkStride, cp, fs, n0, in_len, lane);   // behind row 0
        if (lane < 2 * kChunkT) {
            // lanes 0 ... 15: the 16 samples in front of the chunk into row 0; lanes 16 ... 31: the 16 behind it into row 65
            const bool behind = lane >= kChunkT;
            const long long g = behind ? n0 + kChunkC + (lane - kChunkT) : n0 - kChunkT + lane;
            const bool in = g >= 0 && g < in_len;
            const float v = cp[(in ? g : in_len - 1) * fs];   // always a sample of the signal: no branch
            stage[behind ? (kChunkC / kChunkT + 1) * kChunkStride + (lane - kChunkT) : lane] = in ? v : 0.0f;
        }
        chunk_lds_sync();
        // xs[i]: sample 16 lane - 6 + i of the chunk, which stands at word 17 lane + 10 + i + (10 + i) / 16 of the rows
        float xs[kLimXs];
#pragma unroll
        for (int i = 0; i < kLimXs; i++) xs[i] = stage[lane * kChunkStride + (kChunkT - kLimReach) + i + ((kChunkT - kLimReach + i) >> 4)];
        chunk_lds_sync();                                  // the next use rewrites the stage
        // e[j]: the largest |v_p[m]| at m = 16 lane + 5 + j; v_p[m] = taps[p][0] x[m] + taps[p][1] x[m - 1] + ..., K14's order
        float e[kLimPos];
#pragma unroll
        for (int j = 0; j < kLimPos; j++) e[j] = 0.0f;
#pragma unroll 1
        for (int ph = 0; ph < kLimPhases; ph++) {
            float tp[kLimTaps];
#pragma unroll
            for (int t = 0; t < kLimTaps; t++) tp[t] = taps[ph * kLimTaps + t];
#pragma unroll
            for (int j = 0; j < kLimPos; j++) {
                float v = tp[0] * xs[j + kLimTaps - 1];
#pragma unroll
                for (int t = 1; t < kLimTaps; t++) v = v + tp[t] * xs[j + kLimTaps - 1 - t];
                const float av = fabsf(v);
                e[j] = av > e[j] ? av : e[j];
            }
        }
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            float m = fabsf(xs[kLimReach + k]);
            m = e[k] > m ? e[k] : m;
            m = e[k + 1] > m ? e[k + 1] : m;
            if (c == 0) L[k] = m;
            else L[k] = m > L[k] ? m : L[k];
        }
    }
}

// state: [n_det][kLimStateWords] words of 64 bits, the carries in front of chunk c_origin (y1 as its bits, the running total, the prefix sums
// of chunk c_origin - 1), replaced by the ones in front of chunk c_stop; null: the start of a stream, nothing kept (the block call)
template <int DC>
__global__ __launch_bounds__(64) void lim_kernel(SigViewD src, OutViewD out, LimParams p, unsigned long long* state)
{
    __shared__ float stage[kLimStage];
    __shared__ double ring[2 * kDynSlot];                  // r (la < 16) or P (la >= 16) of two chunks, chunk ck in slot ck & 1: K12's
    __shared__ double lane_max[128];                       // M of the same two chunks
    __shared__ unsigned long long psum[2 * kDynSlot];      // the prefix sums of q of two chunks, in the same layout
    __shared__ double coef[kDynCoefs];
    __shared__ double prm[kLimParams];
    __shared__ float taps[kLimTapCount];
    const int lane = threadIdx.x;
    const long long det = blockIdx.x;
    if (det >= p.n_det) return;
    // DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`
    const long long s_idx = DC == 2 ? det : det / p.ch;
    const int c0 = DC == 2 ? 0 : (int)(det % p.ch);
    const float* ip = src.base + s_idx * src.ss + c0 * src.cs;
    float* op = out.base + s_idx * out.ss + c0 * out.cs;
    if (lane < kDynCoefs) coef[lane] = kDynCoef[lane];
    if (lane < kLimParams) prm[lane] = p.v[lane];
    if (lane < kLimTapCount) taps[lane] = p.taps[lane];
    chunk_lds_sync();
    const bool wide = p.la >= kChunkT;

    // where the detector's carries stand, or null, and the output's address: as the compiler cannot follow them, so in VGPR pairs, not in four
    // SGPRs through the chunk loop (dyn_walk's kSpareSgprs)
    unsigned long long* carry = state ? state + det * kLimStateWords : nullptr;
    asm volatile("" : "+v"(carry), "+v"(op));
    double y1c = 0.0;
    unsigned long long tot = 0;                            // the sum of every q in front of the current chunk, modulo 2^64
    if (carry) {
        y1c = __longlong_as_double((long long)carry[0]);
        tot = carry[1];
        if (p.c_origin > 0) {
#pragma unroll
            for (int k = 0; k < kChunkT; k++)
                psum[chunk_word((int)((p.c_origin - 1) & 1) * kChunkC + lane * kChunkT + k)] = carry[2 + lane * kChunkT + k];
        }
    }
    double dc[kChunkT];     // what its look-ahead maximum starts from: r (la < 16) or the suffix maximum of the lane (la >= 16)

    // steps 1 and 2 of chunk ck: what its maximum starts from, and its part of the ring
    const auto level = [&](long long ck, double (&d0)[kChunkT]) {
        float x[kChunkT];
        if (p.tp) lim_tp_level<DC>(stage, taps, ip, src.cs, src.fs, p.in_len, ck, lane, x);
        else dyn_plain_level<DC>(stage, ip, src.cs, src.fs, p.in_len, ck, lane, x);
        const double ceiling = prm[kLimCeiling], gain = prm[kLimGain];
        double* slot = ring + (int)(ck & 1) * kDynSlot + lane * kChunkStride;
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const double a = (double)x[k];
            const double lg = kDynK * dyn_log2(a, coef);           // of zero too, and dropped: a select
            const double xg = a == 0.0 ? (double)NAE_DYN_FLOOR_DB : lg;
            const double u = (xg + gain) - ceiling;
            const double r = u > 0.0 ? u : 0.0;
            d0[k] = r;
            run = k == 0 ? r : dyn_max(run, r);
            slot[k] = wide ? run : r;
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four samples in flight, not sixteen
        }
        lane_max[(int)(ck & 1) * 64 + lane] = run;
        if (wide) {
#pragma unroll
            for (int k = kChunkT - 2; k >= 0; k--) d0[k] = dyn_max(d0[k], d0[k + 1]);
        }
    };

    // the same of a chunk whose demand is not needed or is known: wholly past in_len its input is zero, and the demand of zero is 0
    const auto quiet = [&](long long ck, double (&d0)[kChunkT]) {
        double* slot = ring + (int)(ck & 1) * kDynSlot + lane * kChunkStride;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            d0[k] = 0.0;
            slot[k] = 0.0;
        }
        lane_max[(int)(ck & 1) * 64 + lane] = 0.0;
    };

    level(p.c_origin, dc);
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        double dn[kChunkT];
        // the lane number the scans' masks are made of, as the compiler cannot follow it: the masks are made chunk by chunk and do not hold
        // their SGPRs through the level pass
        int sl = lane;
        asm volatile("" : "+v"(sl));
        // one chunk ahead — but not past the signal's end (6 samples in front of the chunk may still reach it: their level is that of the chunk
        // before), and not behind the launch's last chunk when nothing looks ahead
        if ((ck + 1) * kChunkC >= p.in_len + (p.tp ? kLimReach : 0) || (ck + 1 == p.c_stop && !p.la)) quiet(ck + 1, dn);
        else level(ck + 1, dn);
        chunk_lds_sync();
        // steps 3 and 4: d[n] = max(r[n] ... r[n + la]) and y1 = max(d, ar y1 + omr d): K12's (dyn_steps.h)
        const int la = p.la;
        const int m0 = (int)(ck & 1) * kChunkC + lane * kChunkT;
        dyn_lookahead_max(ring, lane_max, ck, lane, la, wide, dc);
        dyn_release_scan(prm[kLimAr], prm[kLimOmr], sl, y1c, dc);
        // step 5: q = ceil(y1 2^24) as an integer, its prefix sums, and the moving sum as a difference of two of them
        {
            unsigned long long pq[kChunkT];
            unsigned long long run = 0;
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                const double sc = dc[k] * NAE_LIM_Q_SCALE;
                const double cl = ceil(sc);
                const double fin = fabs(cl) < 9.0e18 ? cl : 0.0;   // not finite: 0, so the conversion is defined
                run += (unsigned long long)(long long)fin;
                pq[k] = run;
            }
            unsigned long long inc = run;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const unsigned long long u = __shfl_up(inc, 1u << j);
                if (sl >= (1 << j)) inc += u;
            }
            unsigned long long base = __shfl_up(inc, 1u);
            if (sl == 0) base = 0;
            base += tot;
            tot += __shfl(inc, 63);
            if (ck == 0) {
                // the hold: q[n] = q[0] for n < 0, so the prefix sum at n < 0 is (n + 1) q[0]; chunk -1 stands in slot 1
                const unsigned long long q0 = __shfl(pq[0], 0);
#pragma unroll
                for (int k = 0; k < kChunkT; k++)
                    psum[chunk_word(kChunkC + lane * kChunkT + k)] = (0ull - (unsigned long long)(kChunkC - 1 - lane * kChunkT - k)) * q0;
            }
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                pq[k] += base;
                psum[chunk_word(m0 + k)] = pq[k];
            }
            chunk_lds_sync();
            const double denom = prm[kLimDenom], gain = prm[kLimGain];
            // step 6: the gain, once per detector and sample
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                const int m = (m0 + k - la - 1) & (2 * kChunkC - 1);
                const unsigned long long W = pq[k] - psum[chunk_word(m)];
                const double s = (double)(long long)W / denom;
                dc[k] = dyn_exp2((gain - s) * kDynKInv, coef);
                if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the chunk's samples are read again (they came through the caches a chunk ago)
#pragma unroll
        for (int c = 0; c < DC; c++) {
            float x[kChunkT];
            dyn_load(stage, ip, c * src.cs, src.fs, p.in_len, ck, lane, x);
#pragma unroll
            for (int k = 0; k < kChunkT; k++) x[k] = (float)((double)x[k] * dc[k]);
            chunk_lane_write(stage, lane, x);
            chunk_lds_sync();
            chunk_store<4>(stage, op + c * out.cs, out.fs, n0, p.in_len, lane);
            chunk_lds_sync();                              // the next channel, or the next chunk, rewrites the stage
        }
#pragma unroll
        for (int k = 0; k < kChunkT; k++) dc[k] = dn[k];
    }
    if (carry) {
        if (lane == 0) {
            carry[0] = (unsigned long long)__double_as_longlong(y1c);
            carry[1] = tot;
        }
#pragma unroll
        for (int k = 0; k < kChunkT; k++)
            carry[2 + lane * kChunkT + k] = psum[chunk_word((int)((p.c_stop - 1) & 1) * kChunkC + lane * kChunkT + k)];
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_lim_block_f32 and nae_lim_create (ctx may be null: no message then)
int nae_lim_check(nae_ctx* ctx, const nae_lim_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->ceiling_db) || !isfinite(p->gain_db) || !isfinite(p->alpha_release)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: non-finite parameter");
    if (p->ceiling_db < NAE_LIM_MIN_CEILING_DB || p->ceiling_db > NAE_LIM_MAX_CEILING_DB)
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: ceiling_db outside -20 ... 0");
    if (p->gain_db < -NAE_LIM_MAX_GAIN_DB || p->gain_db > NAE_LIM_MAX_GAIN_DB) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: gain_db outside -24 ... 24");
    if (p->alpha_release < 0.0 || p->alpha_release >= 1.0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: alpha_release outside [0, 1)");
    if (p->lookahead < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: negative lookahead");
    if (p->true_peak != 0 && p->true_peak != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: true_peak must be 0 or 1");
    if (p->link != 0 && p->link != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "lim: link must be 0 or 1");
    if (p->lookahead > NAE_LIM_MAX_LOOKAHEAD) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "lim: lookahead above 1018 samples");
    return NAE_OK;
}

size_t nae_lim_detectors(const nae_lim_params* p, int ch, size_t n_streams) { return p->link && ch == 2 ? n_streams : n_streams * (size_t)ch; }
size_t nae_lim_state_words() { return kLimStateWords; }
size_t nae_lim_wait(const nae_lim_params* p) { return (size_t)p->lookahead + (p->true_peak ? kLimReach : 0); }

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_lim(nae_ctx* ctx, const nae_lim_params* lp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, unsigned long long* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    LimParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_det = (long long)nae_lim_detectors(lp, ch, n_streams);
    p.v[kLimCeiling] = lp->ceiling_db;
    p.v[kLimGain] = lp->gain_db;
    p.v[kLimAr] = lp->alpha_release;
    p.v[kLimOmr] = 1.0 - lp->alpha_release;
    p.v[kLimDenom] = (double)((long long)(lp->lookahead + 1) * (long long)NAE_LIM_Q_SCALE);
    static const std::array<float, kLimTapCount> taps = [] {   // K14's design, made once per process
        std::array<float, kLimTapCount> t;
        nae_loud_taps(t.data());
        return t;
    }();
    memcpy(p.taps, taps.data(), sizeof(p.taps));
    p.ch = ch;
    p.la = lp->lookahead;
    p.tp = lp->true_peak;
    // one wave per detector
    return with_flags(lp->link && ch == 2, [&](auto linked) {
        return nae_launch_tiles(ctx, "lim_kernel", "lim_kernel: grid too large", lim_kernel<linked.value ? 2 : 1>, p.n_det, 1, 64, 0, to_view(src),
                                to_out(dst), p, d_state);
    });
}

extern "C" {

int nae_lim_block_f32(nae_ctx* ctx, const nae_lim_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "lim: null pointer");
    const int rc = nae_lim_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "lim: null pointer");
    return nae_launch_lim(ctx, params, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr);
}

// DESIGN.md §3, "K22 limiter", "Design"
int nae_lim_design(int sample_rate, double ceiling_db, double gain_db, double release_s, double lookahead_s, int true_peak, int link,
                   nae_lim_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1) || (true_peak != 0 && true_peak != 1)) return NAE_ERR_INVALID;
    if (!isfinite(ceiling_db) || !isfinite(gain_db) || !isfinite(release_s) || !isfinite(lookahead_s)) return NAE_ERR_INVALID;
    if (ceiling_db < NAE_LIM_MIN_CEILING_DB || ceiling_db > NAE_LIM_MAX_CEILING_DB || gain_db < -NAE_LIM_MAX_GAIN_DB || gain_db > NAE_LIM_MAX_GAIN_DB ||
        release_s < NAE_DYN_MIN_RELEASE_S || release_s > NAE_DYN_MAX_RELEASE_S || lookahead_s < 0.0)
        return NAE_ERR_INVALID;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)NAE_LIM_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    const long n = lround(la);
    if (n > NAE_LIM_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    out->ceiling_db = ceiling_db;
    out->gain_db = gain_db;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->lookahead = (int)n;
    out->true_peak = true_peak;
    out->link = link;
    return NAE_OK;
}

} // extern "C"
