// kernels_dyn.hip — K12, the dynamics processor ("K12 dynamics") for gfx950: a feed-forward compressor / look-ahead limiter in the
// dB domain, its two recurrences computed parallel in time.
//
// One wave per detector walks its chunks of C = 64 T samples (T = NAE_DYN_LANE = 16) in order, as eq_cascade_kernel walks its stream-channel.
// A detector is a stream-channel, or with `link` a stereo stream: the wave then reads and writes both channels (DC = 2).  A chunk is loaded
// coalesced (64 consecutive samples per load) into an LDS stage, where lane l reads its own T consecutive samples at a stride of T + 1 words,
// odd, so the 32 lanes of a ds_read_b32 group fall on 32 banks.  The look-ahead needs the demand r of `la` samples past the chunk: the loop is
// one chunk ahead with steps 1 and 2 and keeps what the sliding maximum needs of two chunks in an LDS ring — r itself for la < 16, where a lane
// reads the la words behind each of its samples, and for la >= 16 the running maximum P of every lane's 16 samples from its first on, with the
// 128 lane maxima M: a window that leaves its lane is the rest of that lane (a suffix maximum, in registers), the whole lanes between (M) and
// P at its last sample.  The ring's doubles stand 17 to a lane, 34 words, so the 32 lanes of a ds_read_b64 group fall on the 64 banks in pairs.
// Steps 4 and 5 are scanned as DESIGN.md states them: a lane composes its 16 steps, the wave scans the 64 maps in six Kogge-Stone steps with
// __shfl_up of doubles, every lane takes its start state from the scanned map of the lanes below it and the chunk's carry-in and runs its 16
// samples as the plain recurrence.  The carries (y1, yl) stay in registers between chunks; a handle keeps them in device memory between
// launches.  Built with -ffp-contract=off: every step is one IEEE operation in the order of the CPU statement (tests/dyn_ref/ref_dyn.c).
#include "launch.h"
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kDynT = NAE_DYN_LANE, kDynC = NAE_DYN_CHUNK, kDynStride = kDynT + 1, kDynSlot = 64 * kDynStride;
static_assert(kDynT == 16 && kDynC == 1024 && NAE_DYN_MAX_LOOKAHEAD <= kDynC, "DESIGN.md §3, K12: chunks of 1024 samples, a look-ahead of at most one chunk");

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

__device__ __forceinline__ void dyn_lds_sync()
{
    // this wave's LDS writes before its following LDS reads of other lanes' words: DS operations of one wave execute in issue order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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

// state: [n_det][2] doubles, the carries (y1, yl) in front of chunk c_origin, replaced by the ones behind chunk c_stop - 1; null: zero in,
// nothing out (the block call)
template <int DC>
__global__ __launch_bounds__(64) void dyn_kernel(SigViewD src, OutViewD out, DynParams p, double* state)
{
    __shared__ float stage[kDynC + 64];
    __shared__ double ring[2 * kDynSlot];                  // r (la < 16) or P (la >= 16) of two chunks, chunk ck in slot ck & 1
    __shared__ double lane_max[128];                       // M of the same two chunks
    __shared__ double coef[kDynCoefs];
    __shared__ double prm[kDynParams];
    __shared__ int la_lds;
    const int lane = threadIdx.x;
    const long long det = blockIdx.x;
    if (det >= p.n_det) return;
    if (lane < kDynCoefs) coef[lane] = kDynCoef[lane];
    if (lane < kDynParams) prm[lane] = p.v[lane];
    if (lane == 0) la_lds = p.la;
    dyn_lds_sync();
    // DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`
    const long long s_idx = DC == 2 ? det : det / p.ch;
    const int c0 = DC == 2 ? 0 : (int)(det % p.ch);
    const float* ip = src.base + s_idx * src.ss + c0 * src.cs;
    float* op = out.base + s_idx * out.ss + c0 * out.cs;
    const bool wide = p.la >= kDynT;

    double y1c = 0.0, ylc = 0.0;
    if (state) {
        y1c = state[det * 2];
        ylc = state[det * 2 + 1];
    }
    double dc[kDynT];       // what its look-ahead maximum starts from: r (la < 16) or the suffix maximum of the lane (la >= 16)

    // channel c of chunk ck through the stage: lane l gets its samples [l T, l T + T)
    const auto load = [&](long long ck, int c, float (&x)[kDynT]) {
#pragma unroll 4                                           // not 16: sixteen bounds masks are 32 SGPRs
        for (int j = 0; j < kDynT; j++) {
            const int n = j * 64 + lane;
            const long long g = ck * kDynC + n;
            const float v = ip[c * src.cs + (g < p.in_len ? g : p.in_len - 1) * src.fs];   // always a sample of the signal: no branch
            stage[n + (n >> 4)] = g < p.in_len ? v : 0.0f;
        }
        dyn_lds_sync();
#pragma unroll
        for (int k = 0; k < kDynT; k++) x[k] = stage[lane * kDynStride + k];
        dyn_lds_sync();                                    // the next use rewrites the stage
    };
    // steps 1 and 2 of chunk ck: what its maximum starts from, and its part of the ring
    const auto level = [&](long long ck, double (&d0)[kDynT]) {
        float x[kDynT];
        load(ck, 0, x);
#pragma unroll
        for (int k = 0; k < kDynT; k++) x[k] = fabsf(x[k]);
        if constexpr (DC == 2) {
            float x1[kDynT];
            load(ck, 1, x1);
#pragma unroll
            for (int k = 0; k < kDynT; k++) {
                const float b = fabsf(x1[k]);
                x[k] = b > x[k] ? b : x[k];
            }
        }
        const DynCurve cv{prm[kDynThr], prm[kDynSlope], prm[kDynKnee], prm[kDynHalfKnee], prm[kDynInv2Knee]};
        double* slot = ring + (int)(ck & 1) * kDynSlot + lane * kDynStride;   // sample m of an even chunk and its successor at m + (m >> 4)
        double run = 0.0;
#pragma unroll
        for (int k = 0; k < kDynT; k++) {
            const double r = dyn_demand(cv, x[k], coef);
            d0[k] = r;
            run = k == 0 ? r : dyn_max(run, r);
            slot[k] = wide ? run : r;
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four samples in flight, not sixteen: the registers of twelve more polynomials
        }
        lane_max[(int)(ck & 1) * 64 + lane] = run;
        if (wide) {
#pragma unroll
            for (int k = kDynT - 2; k >= 0; k--) d0[k] = dyn_max(d0[k], d0[k + 1]);
        }
    };

    // the same of a chunk whose demand is not needed or is known: wholly past in_len its input is zero, and the demand of zero is 0
    const auto quiet = [&](long long ck, double (&d0)[kDynT]) {
        double* slot = ring + (int)(ck & 1) * kDynSlot + lane * kDynStride;
#pragma unroll
        for (int k = 0; k < kDynT; k++) {
            d0[k] = 0.0;
            slot[k] = 0.0;
        }
        lane_max[(int)(ck & 1) * 64 + lane] = 0.0;
    };

    level(p.c_origin, dc);
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kDynC;
        double dn[kDynT];
        // one chunk ahead — but not past the signal's end, and not behind the launch's last chunk when nothing looks ahead: steps 1 and 2 are
        // the costliest stage
        if ((ck + 1) * kDynC >= p.in_len || (ck + 1 == p.c_stop && !p.la)) quiet(ck + 1, dn);
        else level(ck + 1, dn);
        dyn_lds_sync();
        // step 3: d[n] = max(r[n] ... r[n + la]); sample m of the two chunks, m < 2048 counted from an even chunk's first, stands at m + (m >> 4).
        // The look-ahead is read from LDS here, behind the fence: what depends on it and on k is then made where it is used, sixteen compares,
        // not carried through the whole chunk loop as sixteen masks and sixteen addresses.
        const int la = la_lds, q = la >> 4, rem = la & 15;
        const double ar = prm[kDynAr], omr = prm[kDynOmr], aa = prm[kDynAa], oma = prm[kDynOma], makeup = prm[kDynMakeup];
        const int m0 = (int)(ck & 1) * kDynC + lane * kDynT;
        if (!wide) {
#pragma unroll 1
            for (int t = 1; t <= la; t++) {
#pragma unroll
                for (int k = 0; k < kDynT; k++) {
                    const int m = (m0 + k + t) & (2 * kDynC - 1);
                    dc[k] = dyn_max(dc[k], ring[m + (m >> 4)]);
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
            for (int k = 0; k < kDynT; k++) {
                const int m = (m0 + k + la) & (2 * kDynC - 1);
                dc[k] = dyn_max(dc[k], dyn_max(k + rem >= kDynT ? r2 : r1, ring[m + (m >> 4)]));
            }
        }
        // step 4: y1 = max(d, ar y1 + omr d), the step as the map y -> max(c, a y + b)
        {
            double A = ar, B = omr * dc[0], M = dc[0];
#pragma unroll
            for (int k = 1; k < kDynT; k++) {
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
                if (lane >= (1 << j)) {
                    A = nA;
                    B = nB;
                    M = nM;
                }
            }
            const double pA = __shfl_up(A, 1u), pB = __shfl_up(B, 1u), pM = __shfl_up(M, 1u);
            double s = dyn_max(pM, (pA * y1c) + pB);
            if (lane == 0) s = y1c;
#pragma unroll
            for (int k = 0; k < kDynT; k++) {
                s = dyn_max(dc[k], (ar * s) + (omr * dc[k]));
                dc[k] = s;
            }
            y1c = __shfl(s, 63);
        }
        // step 5: yl = aa yl + oma y1, the step as the map y -> a y + b
        {
            double A = aa, B = oma * dc[0];
#pragma unroll
            for (int k = 1; k < kDynT; k++) {
                const double bk = oma * dc[k];
                A = aa * A;
                B = (aa * B) + bk;
            }
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const double uA = __shfl_up(A, 1u << j), uB = __shfl_up(B, 1u << j);
                const double nA = A * uA;
                const double nB = (A * uB) + B;
                if (lane >= (1 << j)) {
                    A = nA;
                    B = nB;
                }
            }
            const double pA = __shfl_up(A, 1u), pB = __shfl_up(B, 1u);
            double s = (pA * ylc) + pB;
            if (lane == 0) s = ylc;
#pragma unroll
            for (int k = 0; k < kDynT; k++) {
                s = (aa * s) + (oma * dc[k]);
                dc[k] = s;
            }
            ylc = __shfl(s, 63);
        }
        // step 6: the gain, once per detector and sample; the chunk's samples are read again (they came through the caches a chunk ago)
#pragma unroll
        for (int k = 0; k < kDynT; k++) {
            dc[k] = dyn_exp2((makeup - dc[k]) * kDynKInv, coef);
            if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int c = 0; c < DC; c++) {
            float x[kDynT];
            load(ck, c, x);
#pragma unroll
            for (int k = 0; k < kDynT; k++) stage[lane * kDynStride + k] = (float)((double)x[k] * dc[k]);
            dyn_lds_sync();
#pragma unroll 4
            for (int j = 0; j < kDynT; j++) {
                const int n = j * 64 + lane;
                const long long g = n0 + n;
                if (g < p.in_len) op[c * out.cs + g * out.fs] = stage[n + (n >> 4)];
            }
            dyn_lds_sync();                                // the next channel, or the next chunk, rewrites the stage
        }
#pragma unroll
        for (int k = 0; k < kDynT; k++) dc[k] = dn[k];
    }
    if (state && lane == 0) {
        state[det * 2] = y1c;
        state[det * 2 + 1] = ylc;
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_dyn_block_f32 and nae_dyn_create (ctx may be null: no message then)
int nae_dyn_check(nae_ctx* ctx, const nae_dyn_params* p, int ch)
{
    const auto fail = [&](int code, const char* what) { return ctx ? nae_fail(ctx, code, what) : code; };
    if (!p) return fail(NAE_ERR_INVALID, "dyn: null pointer");
    if (ch != 1 && ch != 2) return fail(NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->threshold_db) || !isfinite(p->slope) || !isfinite(p->knee_db) || !isfinite(p->alpha_attack) || !isfinite(p->alpha_release) ||
        !isfinite(p->makeup_db))
        return fail(NAE_ERR_INVALID, "dyn: non-finite parameter");
    if (p->threshold_db < NAE_DYN_MIN_THRESHOLD_DB || p->threshold_db > NAE_DYN_MAX_THRESHOLD_DB) return fail(NAE_ERR_INVALID, "dyn: threshold_db outside -60 ... 0");
    if (p->slope < 0.0 || p->slope > 1.0) return fail(NAE_ERR_INVALID, "dyn: slope outside 0 ... 1");
    if (p->knee_db < 0.0 || p->knee_db > NAE_DYN_MAX_KNEE_DB) return fail(NAE_ERR_INVALID, "dyn: knee_db outside 0 ... 24");
    if (p->alpha_attack < 0.0 || p->alpha_attack >= 1.0 || p->alpha_release < 0.0 || p->alpha_release >= 1.0)
        return fail(NAE_ERR_INVALID, "dyn: alpha outside [0, 1)");
    if (p->makeup_db < -NAE_DYN_MAX_MAKEUP_DB || p->makeup_db > NAE_DYN_MAX_MAKEUP_DB) return fail(NAE_ERR_INVALID, "dyn: makeup_db outside -24 ... 24");
    if (p->lookahead < 0) return fail(NAE_ERR_INVALID, "dyn: negative lookahead");
    if (p->link != 0 && p->link != 1) return fail(NAE_ERR_INVALID, "dyn: link must be 0 or 1");
    if (p->lookahead > NAE_DYN_MAX_LOOKAHEAD) return fail(NAE_ERR_UNSUPPORTED, "dyn: lookahead above 1024 samples");
    return NAE_OK;
}

size_t nae_dyn_detectors(const nae_dyn_params* p, int ch, size_t n_streams) { return p->link && ch == 2 ? n_streams : n_streams * (size_t)ch; }

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_dyn(nae_ctx* ctx, const nae_dyn_params* dp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, double* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    const size_t n_det = nae_dyn_detectors(dp, ch, n_streams);
    DynParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_det = (long long)n_det;
    p.v[kDynThr] = dp->threshold_db;
    p.v[kDynSlope] = dp->slope;
    p.v[kDynKnee] = dp->knee_db;
    p.v[kDynHalfKnee] = dp->knee_db / 2.0;
    p.v[kDynInv2Knee] = dp->knee_db > 0.0 ? 1.0 / (2.0 * dp->knee_db) : 0.0;
    p.v[kDynAa] = dp->alpha_attack;
    p.v[kDynOma] = 1.0 - dp->alpha_attack;
    p.v[kDynAr] = dp->alpha_release;
    p.v[kDynOmr] = 1.0 - dp->alpha_release;
    p.v[kDynMakeup] = dp->makeup_db;
    p.ch = ch;
    p.la = dp->lookahead;
    // one wave per detector
    return with_flags(dp->link && ch == 2, [&](auto linked) {
        return nae_launch_tiles(ctx, "dyn_kernel", "dyn_kernel: grid too large", dyn_kernel<linked.value ? 2 : 1>, p.n_det, 1, 64, 0, to_view(src),
                                to_out(dst), p, d_state);
    });
}

extern "C" {

int nae_dyn_block_f32(nae_ctx* ctx, const nae_dyn_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "dyn: null pointer");
    const int rc = nae_dyn_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "dyn: null pointer");
    return nae_launch_dyn(ctx, params, src, in_len, ch, n_streams, dst, 0, (in_len + kDynC - 1) / kDynC, nullptr);
}

// DESIGN.md §3, "K12 dynamics", "Design"
int nae_dyn_design(int sample_rate, double threshold_db, double ratio, double knee_db, double attack_s, double release_s, double lookahead_s,
                   double makeup_db, int link, nae_dyn_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1)) return NAE_ERR_INVALID;
    if (!isfinite(threshold_db) || isnan(ratio) || !isfinite(knee_db) || !isfinite(attack_s) || !isfinite(release_s) || !isfinite(lookahead_s) ||
        !isfinite(makeup_db))
        return NAE_ERR_INVALID;
    if (threshold_db < NAE_DYN_MIN_THRESHOLD_DB || threshold_db > NAE_DYN_MAX_THRESHOLD_DB || ratio < 1.0 || knee_db < 0.0 || knee_db > NAE_DYN_MAX_KNEE_DB ||
        attack_s < 0.0 || attack_s > NAE_DYN_MAX_ATTACK_S || release_s < NAE_DYN_MIN_RELEASE_S || release_s > NAE_DYN_MAX_RELEASE_S ||
        makeup_db < -NAE_DYN_MAX_MAKEUP_DB || makeup_db > NAE_DYN_MAX_MAKEUP_DB || lookahead_s < 0.0)
        return NAE_ERR_INVALID;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    const long n = lround(la);
    if (n > NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    out->threshold_db = threshold_db;
    out->slope = isinf(ratio) ? 1.0 : 1.0 - 1.0 / ratio;
    out->knee_db = knee_db;
    out->alpha_attack = attack_s > 0.0 ? exp(-1.0 / (attack_s * (double)sample_rate)) : 0.0;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->makeup_db = makeup_db;
    out->lookahead = (int)n;
    out->link = link;
    return NAE_OK;
}

} // extern "C"
