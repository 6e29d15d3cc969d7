// dyn_steps.h — what the dynamics processor (kernels_dyn.hip, K12) and the keyed dynamics (kernels_dynkey.hip, K15) share: the launch record,
// the two functions of the specification, the static curve, the staged load, and the walk of one wave over its detector's chunks (DESIGN.md
// §3, "K12 dynamics", steps 1 to 6).  Steps 3 and 4 stand as functions of their own (dyn_lookahead_max, dyn_release_scan): the limiter
// (kernels_lim.hip, K22) runs them too.  The two kernels differ in where the magnitude of steps 1 and 2 comes from; the walk takes that as a
// `Mag`, and states every other step once.  Both translation units are built with -ffp-contract=off: every step is one IEEE operation in
// the order of the CPU statement (tests/dyn_ref/ref_dyn.c).
//
// One wave per detector walks its chunks of C = 64 T samples (T = NAE_DYN_LANE = 16) in order, as eq_cascade_kernel walks its stream-channel.
// A chunk is loaded coalesced (64 consecutive samples per load) into an LDS stage, where lane l reads its own T consecutive samples at a stride
// of T + 1 words, odd, so the 32 lanes of a ds_read_b32 group fall on 32 banks: the tiling, the stage and the wave's LDS ordering stand in
// chunk_stage.h.  The look-ahead needs the demand r of `la` samples past the chunk:
// the loop is one chunk ahead with steps 1 and 2 and keeps what the sliding maximum needs of two chunks in an LDS ring — r itself for
// la < 16, where a lane reads the la words behind each of its samples, and for la >= 16 the running maximum P of every lane's 16 samples from
// its first on, with the 128 lane maxima M: a window that leaves its lane is the rest of that lane (a suffix maximum, in registers), the whole
// lanes between (M) and P at its last sample.  The ring's doubles stand 17 to a lane, 34 words, so the 32 lanes of a ds_read_b64 group fall on
// the 64 banks in pairs.  Steps 4 and 5 are scanned as DESIGN.md states them: a lane composes its 16 steps, the wave scans the 64 maps in six
// Kogge-Stone steps with __shfl_up of doubles, every lane takes its start state from the scanned map of the lanes below it and the chunk's
// carry-in and runs its 16 samples as the plain recurrence.  The carries (y1, yl) stay in registers between chunks; a handle keeps them in
// device memory between launches.
#pragma once
#include "chunk_stage.h"

namespace nae {

constexpr int kDynSlot = 64 * kChunkStride;          // a chunk of the ring: chunk_word's layout, in doubles
static_assert(NAE_DYN_MAX_LOOKAHEAD <= kChunkC, "DESIGN.md §3, K12: a look-ahead of at most one chunk");

constexpr double kDynK = 6.020599913279624;      // 20 log10(2)
constexpr double kDynKInv = 0.1660964047443681;  // 1 / K

struct DynParams {
    long long in_len;      // samples of a signal: reads at or past in_len give zero, samples there are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_det;       // detectors: one wave each
    double v[10];          // kDynThr ... kDynMakeup
    int ch, la;
};
// DynParams::v.  The kernel keeps these ten in LDS with the polynomials' coefficients and reads them where a phase starts, as broadcasts into
// VGPRs: as kernel arguments they are 20 SGPRs through the whole chunk loop, which with the views and the loop's own then spill.
enum { kDynThr, kDynSlope, kDynKnee, kDynHalfKnee, kDynInv2Knee, kDynAa, kDynOma, kDynAr, kDynOmr, kDynMakeup, kDynParams };
struct DynCurve { double thr, slope, knee, half_knee, inv_2knee; };

__device__ __forceinline__ double dyn_max(double a, double b) { return __builtin_fmax(a, b); }

// the coefficients of the two polynomials, lowest degree first: 2 / ((2 i + 1) ln 2), i < 9, and (ln 2)^i / i!, i < 12.  The kernel copies them
// into LDS once per launch and reads them there at wave-uniform addresses (broadcasts): as literals they are 40 SGPR pairs that live through
// the whole chunk loop, and spilled.
constexpr int kDynLogTerms = 9, kDynExpTerms = 12, kDynCoefs = kDynLogTerms + kDynExpTerms;
__device__ const double kDynCoef[kDynCoefs] = {
    2.8853900817779268, 0.9617966939259757, 0.5770780163555853, 0.41219858311113244, 0.3205988979753252, 0.2623081892525388,
    0.2219530832136867, 0.19235933878519512, 0.16972882833987804,
    1.0, 0.6931471805599453, 0.2402265069591007, 0.055504108664821576, 0.009618129107628477, 0.0013333558146428441, 0.00015403530393381606,
    1.5252733804059838e-05, 1.3215486790144305e-06, 1.0178086009239696e-07, 7.054911620801121e-09, 4.44553827187081e-10};

// DESIGN.md §3, "K12 dynamics", dyn_log2: a positive, normal double; cf: the coefficients in LDS
__device__ __forceinline__ double dyn_log2(double a, const double* cf)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(a);
    int e = (int)((bits >> 52) & 0x7ff) - 1023;
    const unsigned long long mant = bits & 0xfffffffffffffull;
    const bool up = mant > 0x6a09e667f3bcdull;
    const unsigned long long mbits = mant | ((up ? 1022ull : 1023ull) << 52);
    e += up ? 1 : 0;
    const double m = __longlong_as_double((long long)mbits);
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = cf[kDynLogTerms - 1];
#pragma unroll
    for (int i = kDynLogTerms - 2; i >= 0; i--) p = p * z + cf[i];
    return (double)e + s * p;
}

// DESIGN.md §3, "K12 dynamics", dyn_exp2: |t| < 1000
__device__ __forceinline__ double dyn_exp2(double t, const double* cf)
{
    const double big = 6755399441055744.0;   // 1.5 * 2^52
    const double tt = t + big;
    const int n = (int)(unsigned)(unsigned long long)__double_as_longlong(tt);
    const double f = t - (tt - big);
    double p = cf[kDynCoefs - 1];
#pragma unroll
    for (int i = kDynExpTerms - 2; i >= 0; i--) p = p * f + cf[kDynLogTerms + i];
    const unsigned long long sbits = (unsigned long long)(unsigned)(n + 1023) << 52;
    return p * __longlong_as_double((long long)sbits);
}

// steps 1 and 2: the gain-reduction demand of the magnitude af
__device__ __forceinline__ double dyn_demand(const DynCurve& p, float af, const double* cf)
{
    const double a = (double)af;
    const double lg = kDynK * dyn_log2(a, cf);             // of zero too, and dropped: a select, no branch around the division
    const double xg = a == 0.0 ? (double)NAE_DYN_FLOOR_DB : lg;
    const double u = xg - p.thr;
    const double tu = 2.0 * u;
    const double h = u + p.half_knee;
    const double soft = (p.slope * (h * h)) * p.inv_2knee;
    const double hard = p.slope * u;
    return tu < -p.knee ? 0.0 : (p.knee > 0.0 && fabs(tu) <= p.knee ? soft : hard);
}

// the staged load: chunk ck of the channel at cp + ofs (frames fs apart, in_len of them, zero behind) through the stage; lane l gets its
// samples [l T, l T + T)
__device__ inline void dyn_load(float* stage, const float* cp, long long ofs, long long fs, long long in_len, long long ck, int lane,
                                         float (&x)[kChunkT])
{
    chunk_load<true, 4>(stage, cp + ofs, fs, ck * kChunkC, in_len, lane);   // four loads together, not 16: sixteen bounds masks are 32 SGPRs
    chunk_lds_sync();
    chunk_lane_read(stage, lane, x);
    chunk_lds_sync();                                      // the next use rewrites the stage
}

// the magnitude of steps 1 and 2 where nothing is filtered: |.| of KC channels at kp (cs apart), the larger of two
template <int KC>
__device__ inline void dyn_plain_level(float* stage, const float* kp, long long cs, long long fs, long long in_len, long long ck, int lane,
                                       float (&x)[kChunkT])
{
    dyn_load(stage, kp, 0, fs, in_len, ck, lane, x);
#pragma unroll
    for (int k = 0; k < kChunkT; k++) x[k] = fabsf(x[k]);
    if constexpr (KC == 2) {
        float x1[kChunkT];
        dyn_load(stage, kp, cs, fs, in_len, ck, lane, x1);
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const float b = fabsf(x1[k]);
            x[k] = b > x[k] ? b : x[k];
        }
    }
}

// K12's source of that magnitude: the signal is its own key.  A Mag has level(stage, ck, x), the magnitudes of chunk ck into the lane's x,
// skip(), which the walk calls where it leaves a chunk's level out, and kSpareSgprs: its level needs SGPRs the walk would hold through it, so the
// walk keeps two addresses in VGPRs and makes its scans' lane masks chunk by chunk.
template <int KC>
struct DynPlainKey {
    const float* kp;
    const SigViewD& v;
    const DynParams& p;
    int lane;
    __device__ void level(float* stage, long long ck, float (&x)[kChunkT]) { dyn_plain_level<KC>(stage, kp, v.cs, v.fs, p.in_len, ck, lane, x); }
    __device__ void skip() {}
    static constexpr bool kSpareSgprs = false;
};

// step 3 of chunk ck: d[n] = max(r[n] ... r[n + la]) on dc, which holds what the maximum starts from: r (la < 16) or the lane's suffix maximum
// (la >= 16).  ring: r or P of two chunks, sample m of the two, m < 2048 counted from an even chunk's first, at chunk_word(m); lane_max: M of
// the same two chunks.  K12's, K15's and K22's.
__device__ __forceinline__ void dyn_lookahead_max(const double* ring, const double* lane_max, long long ck, int lane, int la, bool wide,
                                                  double (&dc)[kChunkT])
{
    const int q = la >> 4, rem = la & 15;
    const int m0 = (int)(ck & 1) * kChunkC + lane * kChunkT;
    if (!wide) {
#pragma unroll 1
        for (int t = 1; t <= la; t++) {
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                const int m = (m0 + k + t) & (2 * kChunkC - 1);
                dc[k] = dyn_max(dc[k], ring[chunk_word(m)]);
            }
        }
    } else {
        // the whole lanes between: l + 1 ... l + q - 1, and l + q too where the window ends in lane l + q + 1
        const int l0 = (int)(ck & 1) * 64 + lane;
        double r1 = 0.0;
#pragma unroll 1
        for (int t = 1; t < q; t++) r1 = dyn_max(r1, lane_max[(l0 + t) & 127]);
        const double r2 = dyn_max(r1, lane_max[(l0 + q) & 127]);
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const int m = (m0 + k + la) & (2 * kChunkC - 1);
            dc[k] = dyn_max(dc[k], dyn_max(k + rem >= kChunkT ? r2 : r1, ring[chunk_word(m)]));
        }
    }
}

// step 4 of a chunk: y1 = max(d, ar y1 + omr d) on dc, the step as the map y -> max(c, a y + b); sl: the lane number the scan's masks are made
// of; y1c: the carry in front of the chunk, replaced by the one behind it
__device__ __forceinline__ void dyn_release_scan(double ar, double omr, int sl, double& y1c, double (&dc)[kChunkT])
{
    double A = ar, B = omr * dc[0], M = dc[0];
#pragma unroll
    for (int k = 1; k < kChunkT; k++) {
        const double bk = omr * dc[k];
        A = ar * A;
        B = (ar * B) + bk;
        M = dyn_max(dc[k], (ar * M) + bk);
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double uA = __shfl_up(A, 1u << j), uB = __shfl_up(B, 1u << j), uM = __shfl_up(M, 1u << j);
        const double nA = A * uA;
        const double nB = (A * uB) + B;
        const double nM = dyn_max(M, (A * uM) + B);
        if (sl >= (1 << j)) {
            A = nA;
            B = nB;
            M = nM;
        }
    }
    const double pA = __shfl_up(A, 1u), pB = __shfl_up(B, 1u), pM = __shfl_up(M, 1u);
    double s = dyn_max(pM, (pA * y1c) + pB);
    if (sl == 0) s = y1c;
#pragma unroll
    for (int k = 0; k < kChunkT; k++) {
        s = dyn_max(dc[k], (ar * s) + (omr * dc[k]));
        dc[k] = s;
    }
    y1c = __shfl(s, 63);
}

// The walk of detector `det`'s wave over chunks [c_origin, c_stop): ip, op: the detector's first signal channel in and out (DC of them, src.cs
// and out.cs apart).  state: [n_det][2] doubles, the carries (y1, yl) in front of chunk c_origin, replaced by the ones behind chunk
// c_stop - 1; null: zero in, nothing out (the block call).  mag.level runs one chunk ahead of the rest: chunk c_origin first, and chunk c_stop
// at the end where something looks ahead and the signal reaches it.
template <int DC, class Mag>
__device__ inline void dyn_walk(const float* ip, float* op, const SigViewD& src, const OutViewD& out, const DynParams& p, double* state,
                                         long long det, int lane, Mag& mag)
{
    __shared__ float stage[kChunkStage];
    __shared__ double ring[2 * kDynSlot];                  // r (la < 16) or P (la >= 16) of two chunks, chunk ck in slot ck & 1
    __shared__ double lane_max[128];                       // M of the same two chunks
    __shared__ double coef[kDynCoefs];
    __shared__ double prm[kDynParams];
    __shared__ int la_lds;
    if (lane < kDynCoefs) coef[lane] = kDynCoef[lane];
    if (lane < kDynParams) prm[lane] = p.v[lane];
    if (lane == 0) la_lds = p.la;
    chunk_lds_sync();
    const bool wide = p.la >= kChunkT;

    // where the detector's carries stand, or null; with kSpareSgprs as the compiler cannot follow it, so in a VGPR pair, not in two SGPRs
    // through the chunk loop
    double* carry = state ? state + det * 2 : nullptr;
    if constexpr (Mag::kSpareSgprs) asm volatile("" : "+v"(carry), "+v"(op));   // and the output's address with it
    double y1c = 0.0, ylc = 0.0;
    if (carry) {
        y1c = carry[0];
        ylc = carry[1];
    }
    double dc[kChunkT];     // what its look-ahead maximum starts from: r (la < 16) or the suffix maximum of the lane (la >= 16)

    // steps 1 and 2 of chunk ck: what its maximum starts from, and its part of the ring
    const auto level = [&](long long ck, double (&d0)[kChunkT]) {
        float x[kChunkT];
        mag.level(stage, ck, x);
        const DynCurve cv{prm[kDynThr], prm[kDynSlope], prm[kDynKnee], prm[kDynHalfKnee], prm[kDynInv2Knee]};
        double* slot = ring + (int)(ck & 1) * kDynSlot + lane * kChunkStride;   // sample m of an even chunk and its successor at chunk_word(m)
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const double r = dyn_demand(cv, x[k], coef);
            d0[k] = r;
            run = k == 0 ? r : dyn_max(run, r);
            slot[k] = wide ? run : r;
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four samples in flight, not sixteen: the registers of twelve more polynomials
        }
        lane_max[(int)(ck & 1) * 64 + lane] = run;
        if (wide) {
#pragma unroll
            for (int k = kChunkT - 2; k >= 0; k--) d0[k] = dyn_max(d0[k], d0[k + 1]);
        }
    };

    // the same of a chunk whose demand is not needed or is known: wholly past in_len its input is zero, and the demand of zero is 0
    const auto quiet = [&](long long ck, double (&d0)[kChunkT]) {
        mag.skip();
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
        // the lane number the scans' masks are made of: where a Mag asks for it, one the compiler cannot follow, so the seven masks are made
        // chunk by chunk and do not hold fourteen SGPRs through the Mag's level
        int sl = lane;
        if constexpr (Mag::kSpareSgprs) asm volatile("" : "+v"(sl));
        // one chunk ahead — but not past the signal's end, and not behind the launch's last chunk when nothing looks ahead: steps 1 and 2 are
        // the costliest stage
        if ((ck + 1) * kChunkC >= p.in_len || (ck + 1 == p.c_stop && !p.la)) quiet(ck + 1, dn);
        else level(ck + 1, dn);
        chunk_lds_sync();
        // step 3: d[n] = max(r[n] ... r[n + la]); sample m of the two chunks, m < 2048 counted from an even chunk's first, stands at chunk_word(m).
        // The look-ahead is read from LDS here, behind the fence: what depends on it and on k is then made where it is used, sixteen compares,
        // not carried through the whole chunk loop as sixteen masks and sixteen addresses.
        const int la = la_lds;
        const double ar = prm[kDynAr], omr = prm[kDynOmr], aa = prm[kDynAa], oma = prm[kDynOma], makeup = prm[kDynMakeup];
        dyn_lookahead_max(ring, lane_max, ck, lane, la, wide, dc);
        dyn_release_scan(ar, omr, sl, y1c, dc);
        // step 5: yl = aa yl + oma y1, the step as the map y -> a y + b
        {
            double A = aa, B = oma * dc[0];
#pragma unroll
            for (int k = 1; k < kChunkT; k++) {
                const double bk = oma * dc[k];
                A = aa * A;
                B = (aa * B) + bk;
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
            double s = (pA * ylc) + pB;
            if (sl == 0) s = ylc;
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                s = (aa * s) + (oma * dc[k]);
                dc[k] = s;
            }
            ylc = __shfl(s, 63);
        }
        // step 6: the gain, once per detector and sample; the chunk's samples are read again (they came through the caches a chunk ago)
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            dc[k] = dyn_exp2((makeup - dc[k]) * kDynKInv, coef);
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
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
    if (carry && lane == 0) {
        carry[0] = y1c;
        carry[1] = ylc;
    }
}

} // namespace nae

// kernels_dyn.hip: the launch record of chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples
nae::DynParams nae_dyn_launch_params(const nae_dyn_params* dp, size_t in_len, int ch, size_t n_streams, size_t c_origin, size_t c_stop);
