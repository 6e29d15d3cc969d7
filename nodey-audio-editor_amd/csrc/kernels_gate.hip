// kernels_gate.hip — K19, the noise gate and downward expander ("K19 gate") for gfx950: a hysteresis decision with a hold timer
// behind a look-ahead, made parallel in time in integers, and a smoother in the dB domain whose coefficient changes from sample to sample.
//
// One wave per detector walks its chunks of 64 lanes x 16 samples in order (chunk_stage.h).  A detector is a stream-channel, or with `link`
// a stereo stream: the wave then reads and writes both channels (DC = 2).  The walk is one chunk ahead with steps 1 and 2: a lane packs the
// set / clear / keep events of its 16 samples, takes its incoming state from the last event of the nearest lower lane (two ballots and a count
// of leading zeros; the chunk's carry where there is none) and leaves its 16 states as one word of an LDS ring of two chunks.  The ballots of
// the lanes that hold a set state stay in registers.  Step 3 is then two ring words, a mask and a count of leading zeros per sample, with the
// last set sample of an earlier lane, or of an earlier chunk (the carried index), where the lane's own words hold none.  Step 5 is scanned as
// DESIGN.md states it.  The carries (the state, the last set index, y) stay in registers between chunks; a handle keeps them in device
// memory between launches, as they stand in front of the chunk at which the launch stops.  Built with -ffp-contract=off: every step is one
// IEEE operation in the order of the CPU statement (tests/gate_ref/ref_gate.c).
#include "dyn_steps.h"
#include <math.h>
#include <string.h>

namespace nae {

struct GateParams {
    long long in_len;      // samples of a signal: reads at or past in_len give zero, samples there are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_det;       // detectors: one wave each
    double v[6];           // kGateThr ... kGateOmr
    float open_lin, close_lin;
    int ch, la, hold;
};
enum { kGateThr, kGateSlope, kGateRange, kGateAa, kGateAr, kGateOmr, kGateParams };

constexpr int kGateFar = -(1 << 23);   // "no set sample in reach", as a position relative to a chunk: below -NAE_GATE_MAX_HOLD
static_assert(NAE_GATE_MAX_HOLD + kChunkC < (1 << 23), "kGateFar lies below every n - hold of a chunk");

// m ? a : b for m all ones or zero, on the bits: sixteen selects by compare are sixteen SGPR pairs through a phase
__device__ __forceinline__ double gate_pick(unsigned m, double a, double b)
{
    const unsigned long long mm = ((unsigned long long)m << 32) | m;
    return __longlong_as_double((long long)(((unsigned long long)__double_as_longlong(a) & mm) | ((unsigned long long)__double_as_longlong(b) & ~mm)));
}
// bit k of the open mask as all ones or zero
__device__ __forceinline__ unsigned gate_bit(unsigned openm, int k) { return 0u - ((openm >> k) & 1u); }

// the highest set bit of a word that has one
__device__ __forceinline__ int gate_top(unsigned w) { return 31 - __clz((int)w); }
__device__ __forceinline__ int gate_top64(unsigned long long w) { return 63 - __clzll((long long)w); }

// state: [n_det][3] words of 64 bits, the carries in front of chunk c_origin (the hysteresis state, the last set sample or -1, y as its bits),
// replaced by the ones in front of chunk c_stop; null: (0, none, range_db) in, nothing out (the block call)
template <int DC, bool EXPAND>
__global__ __launch_bounds__(64) void gate_kernel(SigViewD src, OutViewD out, GateParams p, long long* state)
{
    __shared__ float stage[kChunkStage];
    __shared__ unsigned smask[128];                        // the 16 states of every lane of two chunks, chunk ck in words [(ck & 1) 64, +64)
    __shared__ double coef[kDynCoefs];
    __shared__ double prm[kGateParams];
    const int lane = threadIdx.x;
    const long long det = blockIdx.x;
    if (det >= p.n_det) return;
    // DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`
    const long long s_idx = DC == 2 ? det : det / p.ch;
    const int c0 = DC == 2 ? 0 : (int)(det % p.ch);
    const float* ip = src.base + s_idx * src.ss + c0 * src.cs;
    float* op = out.base + s_idx * out.ss + c0 * out.cs;
    if (lane < kDynCoefs) coef[lane] = kDynCoef[lane];
    if (lane < kGateParams) prm[lane] = p.v[lane];
    chunk_lds_sync();

    // where the detector's carries stand, or null, and the output's address: as the compiler cannot follow them, so in VGPR pairs, not in four
    // SGPRs through the chunk loop (dyn_walk's kSpareSgprs)
    long long* carry = state ? state + det * 3 : nullptr;
    asm volatile("" : "+v"(carry), "+v"(op));
    int s_front = 0;              // the hysteresis state in front of the chunk the level pass does next
    long long last = -1;          // the last set sample in front of the current chunk, or -1
    double yc = p.v[kGateRange];
    if (carry) {
        s_front = (int)carry[0];
        last = carry[1];
        yc = __longlong_as_double(carry[2]);
    }

    // steps 1 and 2 of chunk c from the state s_in in front of it: the lanes' states into the ring, the state behind the chunk into s_out;
    // returns the lanes that hold a set state
    const auto level = [&](long long c, int s_in, int& s_out) -> unsigned long long {
        float x[kChunkT];
        dyn_plain_level<DC>(stage, ip, src.cs, src.fs, p.in_len, c, lane, x);
        unsigned setm = 0, clrm = 0;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            setm |= (x[k] >= p.open_lin ? 1u : 0u) << k;   // a NaN fails both and keeps the state
            clrm |= (x[k] < p.close_lin ? 1u : 0u) << k;
        }
        const unsigned ev = setm | clrm;
        const bool last_set = ev != 0 && ((setm >> gate_top(ev | 1u)) & 1u) != 0;
        const unsigned long long b_ev = __ballot(ev != 0), b_set = __ballot(last_set);
        const unsigned long long lower = b_ev & ((1ull << lane) - 1ull);
        unsigned st = lower ? (unsigned)((b_set >> gate_top64(lower)) & 1ull) : (unsigned)s_in;
        s_out = b_ev ? (int)((b_set >> gate_top64(b_ev)) & 1ull) : s_in;
        unsigned m = 0;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            st = ((setm >> k) & 1u) | (st & ~(clrm >> k) & 1u);
            m |= st << k;
        }
        smask[(int)(c & 1) * 64 + lane] = m;
        return __ballot(m != 0);
    };

    int s_next = s_front;
    unsigned long long any_c = level(p.c_origin, s_front, s_next);
    s_front = s_next;             // in front of chunk c_origin + 1
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        // one chunk ahead — but not past the signal's end (zero is below close_lin: no set state there), and not behind the launch's last
        // chunk when nothing looks ahead
        unsigned long long any_n = 0;
        if ((ck + 1) * kChunkC >= p.in_len || (ck + 1 == p.c_stop && !p.la)) smask[(int)((ck + 1) & 1) * 64 + lane] = 0;
        else any_n = level(ck + 1, s_front, s_next);
        chunk_lds_sync();

        // step 3: the last set sample at or below n + la, as a position relative to n0; samples of the two chunks stand in lanes 0 ... 127
        const int rb = (int)(ck & 1) * 64;
        const int la = p.la, q = la >> 4, rem = la & 15, hold = p.hold;
        const int l0 = lane + q;                           // the lane of sample n + la, or the one below it
        const unsigned ww = smask[(rb + l0) & 127] | (smask[(rb + l0 + 1) & 127] << 16);   // lanes l0 and l0 + 1: bit k + rem is sample n + la
        const long long back = n0 - last;
        const int far = last < 0 || back > -(long long)kGateFar ? kGateFar : (int)-back;
        int f0 = far;                                      // below lane l0
        {
            const unsigned long long hi = l0 > 64 ? any_n & ((1ull << (l0 - 64)) - 1ull) : 0ull;
            const unsigned long long lo = l0 >= 64 ? any_c : any_c & ((1ull << l0) - 1ull);
            const int j = hi ? 64 + gate_top64(hi) : (lo ? gate_top64(lo) : -1);
            if (j >= 0) f0 = j * kChunkT + gate_top(smask[(rb + j) & 127] | 1u);
        }
        unsigned openm = 0;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const unsigned w = ww & ((2u << (k + rem)) - 1u);
            const int pos = w ? l0 * kChunkT + gate_top(w) : f0;
            openm |= (pos >= lane * kChunkT + k - hold ? 1u : 0u) << k;
        }
        if (any_c) {
            const int j = gate_top64(any_c);
            last = n0 + j * kChunkT + gate_top(smask[rb + j] | 1u);
        }

        // the lane number the scan's masks are made of, as the compiler cannot follow it: the seven masks are made chunk by chunk and do not
        // hold fourteen SGPRs through the level pass
        int sl = lane;
        asm volatile("" : "+v"(sl));
        // steps 4 and 5: the chunk's samples, the depth, and y = (alpha y) + b as the map y -> A y + B
        float x0[kChunkT], x1[DC == 2 ? kChunkT : 1];
        dyn_load(stage, ip, 0, src.fs, p.in_len, ck, lane, x0);
        if constexpr (DC == 2) dyn_load(stage, ip, src.cs, src.fs, p.in_len, ck, lane, x1);
        const double aa = prm[kGateAa], ar = prm[kGateAr], omr = prm[kGateOmr], range = prm[kGateRange];
        double d[kChunkT];
        if constexpr (EXPAND) {
            const double thr = prm[kGateThr], slope = prm[kGateSlope];
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                float af = fabsf(x0[k]);
                if constexpr (DC == 2) {
                    const float bf = fabsf(x1[k]);
                    af = bf > af ? bf : af;
                }
                const double a = (double)af;
                const double lg = kDynK * dyn_log2(a, coef);   // of zero too, and dropped: a select
                const double xg = a == 0.0 ? (double)NAE_DYN_FLOOR_DB : lg;
                const double u = thr - xg;
                const double v = slope * u;
                const double depth = u <= 0.0 ? 0.0 : (v < range ? v : range);
                d[k] = gate_pick(gate_bit(openm, k), 0.0, omr * depth);
                if (k & 1) __builtin_amdgcn_sched_barrier(0);   // two logarithms in flight, not sixteen: each holds a division's registers
            }
        } else {
            const double b = omr * range;
#pragma unroll
            for (int k = 0; k < kChunkT; k++) d[k] = gate_pick(gate_bit(openm, k), 0.0, b);
        }
        {
            double A = gate_pick(gate_bit(openm, 0), aa, ar), B = d[0];
#pragma unroll
            for (int k = 1; k < kChunkT; k++) {
                const double ak = gate_pick(gate_bit(openm, k), aa, ar);
                A = ak * A;
                B = (ak * B) + d[k];
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double uA = __shfl_up(A, 1u << j), uB = __shfl_up(B, 1u << j);
                const double nA = A * uA;
                const double nB = (A * uB) + B;
                if (sl >= (1 << j)) {
                    A = nA;
                    B = nB;
                }
            }
            const double pA = __shfl_up(A, 1u), pB = __shfl_up(B, 1u);
            double s = (pA * yc) + pB;
            if (sl == 0) s = yc;
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                const double ak = gate_pick(gate_bit(openm, k), aa, ar);
                s = (ak * s) + d[k];
                d[k] = s;
            }
            yc = __shfl(s, 63);
        }
        // step 6: the gain, once per detector and sample
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            d[k] = dyn_exp2((0.0 - d[k]) * kDynKInv, coef);
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int c = 0; c < DC; c++) {
            float y[kChunkT];
#pragma unroll
            for (int k = 0; k < kChunkT; k++) y[k] = (float)((double)(c == 0 ? x0[k] : x1[DC == 2 ? k : 0]) * d[k]);
            chunk_lane_write(stage, lane, y);
            chunk_lds_sync();
            chunk_store<4>(stage, op + c * out.cs, out.fs, n0, p.in_len, lane);
            chunk_lds_sync();                              // the next channel, or the next chunk, rewrites the stage
        }
        any_c = any_n;
        if (ck + 1 < p.c_stop) s_front = s_next;           // at the end: the state in front of chunk c_stop, not behind it
    }
    if (carry && lane == 0) {
        carry[0] = s_front;
        carry[1] = last;
        carry[2] = __double_as_longlong(yc);
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_gate_block_f32 and nae_gate_create (ctx may be null: no message then)
int nae_gate_check(nae_ctx* ctx, const nae_gate_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->open_lin) || !isfinite(p->close_lin) || !isfinite(p->threshold_db) || !isfinite(p->slope) || !isfinite(p->range_db) ||
        !isfinite(p->alpha_attack) || !isfinite(p->alpha_release))
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: non-finite parameter");
    if (!(p->close_lin > 0.0f) || p->close_lin > p->open_lin) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: thresholds outside 0 < close_lin <= open_lin");
    if (p->threshold_db < NAE_GATE_MIN_THRESHOLD_DB || p->threshold_db > NAE_GATE_MAX_THRESHOLD_DB)
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: threshold_db outside -90 ... 0");
    if (p->slope < 0.0 || p->slope > NAE_GATE_MAX_SLOPE) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: slope outside 0 ... 99");
    if (p->range_db < 0.0 || p->range_db > NAE_GATE_MAX_RANGE_DB) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: range_db outside 0 ... 120");
    if (p->alpha_attack < 0.0 || p->alpha_attack >= 1.0 || p->alpha_release < 0.0 || p->alpha_release >= 1.0)
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: alpha outside [0, 1)");
    if (p->hold < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: negative hold");
    if (p->lookahead < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: negative lookahead");
    if (p->expand != 0 && p->expand != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: expand must be 0 or 1");
    if (p->link != 0 && p->link != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "gate: link must be 0 or 1");
    if (p->lookahead > NAE_DYN_MAX_LOOKAHEAD) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "gate: lookahead above 1024 samples");
    if (p->hold > NAE_GATE_MAX_HOLD) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "gate: hold above 2097152 samples");
    return NAE_OK;
}

size_t nae_gate_detectors(const nae_gate_params* p, int ch, size_t n_streams) { return p->link && ch == 2 ? n_streams : n_streams * (size_t)ch; }

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_gate(nae_ctx* ctx, const nae_gate_params* gp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                    size_t c_origin, size_t c_stop, long long* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    GateParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_det = (long long)nae_gate_detectors(gp, ch, n_streams);
    p.v[kGateThr] = gp->threshold_db;
    p.v[kGateSlope] = gp->slope;
    p.v[kGateRange] = gp->range_db;
    p.v[kGateAa] = gp->alpha_attack;
    p.v[kGateAr] = gp->alpha_release;
    p.v[kGateOmr] = 1.0 - gp->alpha_release;
    p.open_lin = gp->open_lin;
    p.close_lin = gp->close_lin;
    p.ch = ch;
    p.la = gp->lookahead;
    p.hold = gp->hold;
    // one wave per detector
    return with_flags(gp->link && ch == 2, gp->expand != 0, [&](auto linked, auto expand) {
        return nae_launch_tiles(ctx, "gate_kernel", "gate_kernel: grid too large", gate_kernel<linked.value ? 2 : 1, expand.value>, p.n_det, 1, 64,
                                0, to_view(src), to_out(dst), p, d_state);
    });
}

extern "C" {

int nae_gate_block_f32(nae_ctx* ctx, const nae_gate_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "gate: null pointer");
    const int rc = nae_gate_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "gate: null pointer");
    return nae_launch_gate(ctx, params, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr);
}

// DESIGN.md §3, "K19 gate", "Design"
int nae_gate_design(int sample_rate, int mode, double threshold_db, double hysteresis_db, double range_db, double ratio, double attack_s,
                    double hold_s, double release_s, double lookahead_s, int link, nae_gate_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1) || (mode != NAE_GATE_MODE_GATE && mode != NAE_GATE_MODE_EXPANDER)) return NAE_ERR_INVALID;
    if (!isfinite(threshold_db) || !isfinite(hysteresis_db) || !isfinite(range_db) || !isfinite(ratio) || !isfinite(attack_s) || !isfinite(hold_s) ||
        !isfinite(release_s) || !isfinite(lookahead_s))
        return NAE_ERR_INVALID;
    if (threshold_db < NAE_GATE_MIN_THRESHOLD_DB || threshold_db > NAE_GATE_MAX_THRESHOLD_DB || hysteresis_db < 0.0 ||
        hysteresis_db > NAE_GATE_MAX_HYSTERESIS_DB || range_db < 0.0 || range_db > NAE_GATE_MAX_RANGE_DB || ratio < 1.0 || ratio > NAE_GATE_MAX_RATIO ||
        attack_s < 0.0 || attack_s > NAE_DYN_MAX_ATTACK_S || hold_s < 0.0 || hold_s > NAE_GATE_MAX_HOLD_S || release_s < NAE_DYN_MIN_RELEASE_S ||
        release_s > NAE_DYN_MAX_RELEASE_S || lookahead_s < 0.0)
        return NAE_ERR_INVALID;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    const long n = lround(la);
    if (n > NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    const double hd = hold_s * (double)sample_rate;
    if (hd > 2.0 * (double)NAE_GATE_MAX_HOLD) return NAE_ERR_UNSUPPORTED;
    const long nh = lround(hd);
    if (nh > NAE_GATE_MAX_HOLD) return NAE_ERR_UNSUPPORTED;
    out->open_lin = (float)pow(10.0, threshold_db / 20.0);
    out->close_lin = (float)pow(10.0, (threshold_db - hysteresis_db) / 20.0);
    out->threshold_db = threshold_db;
    out->slope = ratio - 1.0;
    out->range_db = range_db;
    out->alpha_attack = attack_s > 0.0 ? exp(-1.0 / (attack_s * (double)sample_rate)) : 0.0;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->hold = (int)nh;
    out->lookahead = (int)n;
    out->expand = mode == NAE_GATE_MODE_EXPANDER ? 1 : 0;
    out->link = link;
    return NAE_OK;
}

} // extern "C"
