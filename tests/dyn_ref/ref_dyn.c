/* ref_dyn.c — the CPU statement of K12, the dynamics processor ("K12 dynamics"): the tiled form the GPU computes, bit for bit
 * (ref_dyn_run), the plain sequential double recurrence it is measured against (ref_dyn_sequential), the two functions of the
 * specification (ref_dyn_log2, ref_dyn_exp2) and the design (ref_dyn_design).
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written here. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define T 16              /* NAE_DYN_LANE */
#define LANES 64
#define C (LANES * T)     /* NAE_DYN_CHUNK */
#define MAX_LOOKAHEAD 1024 /* NAE_DYN_MAX_LOOKAHEAD */
#define FLOOR_DB (-1000.0) /* NAE_DYN_FLOOR_DB */

typedef struct ref_dyn_params {   /* nae_dyn_params of include/nae_gpu.h */
    double threshold_db, slope, knee_db, alpha_attack, alpha_release, makeup_db;
    int lookahead, link;
} ref_dyn_params;

static const double K = 6.020599913279624;      /* 20 log10(2) */
static const double KINV = 0.1660964047443681;  /* 1 / K */

/* the larger of two doubles that are no NaNs and no zeros of different sign */
static double dmax(double a, double b) { return a > b ? a : b; }

/* log2 of a positive, normal double: the exponent by bit operations, the mantissa folded into [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1),
 * log2 m = s P(s^2) with P the first nine terms of 2 atanh(s) / ln 2 in Horner form */
double ref_dyn_log2(double a)
{
    static const double L[9] = {2.8853900817779268, 0.9617966939259757, 0.5770780163555853, 0.41219858311113244, 0.3205988979753252,
                                0.2623081892525388, 0.2219530832136867, 0.19235933878519512, 0.16972882833987804};
    uint64_t bits;
    memcpy(&bits, &a, 8);
    int e = (int)((bits >> 52) & 0x7ff) - 1023;
    const uint64_t mant = bits & 0xfffffffffffffull;
    uint64_t mbits = mant | (1023ull << 52);
    if (mant > 0x6a09e667f3bcdull) {
        mbits = mant | (1022ull << 52);
        e += 1;
    }
    double m;
    memcpy(&m, &mbits, 8);
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = L[8];
    for (int i = 7; i >= 0; i--) p = p * z + L[i];
    return (double)e + s * p;
}

/* 2^t, |t| < 1000: n = the nearest integer by the 1.5 * 2^52 addition, f = t - n in [-1/2, 1/2], 2^f by the terms up to degree 11 of
 * exp(f ln 2) in Horner form, times 2^n made by bit operations */
double ref_dyn_exp2(double t)
{
    static const double E[12] = {1.0, 0.6931471805599453, 0.2402265069591007, 0.055504108664821576, 0.009618129107628477,
                                 0.0013333558146428441, 0.00015403530393381606, 1.5252733804059838e-05, 1.3215486790144305e-06,
                                 1.0178086009239696e-07, 7.054911620801121e-09, 4.44553827187081e-10};
    const double big = 6755399441055744.0;   /* 1.5 * 2^52 */
    const double tt = t + big;
    uint64_t bits;
    memcpy(&bits, &tt, 8);
    const int n = (int)(uint32_t)bits;
    const double f = t - (tt - big);
    double p = E[11];
    for (int i = 10; i >= 0; i--) p = p * f + E[i];
    const uint64_t sbits = (uint64_t)(uint32_t)(n + 1023) << 52;
    double sc;
    memcpy(&sc, &sbits, 8);
    return p * sc;
}

void ref_dyn_log2_v(const double* a, size_t n, double* out) { for (size_t i = 0; i < n; i++) out[i] = ref_dyn_log2(a[i]); }
void ref_dyn_exp2_v(const double* t, size_t n, double* out) { for (size_t i = 0; i < n; i++) out[i] = ref_dyn_exp2(t[i]); }

/* 0 when the parameters are acceptable, -1 invalid, -2 a look-ahead above the maximum */
int ref_dyn_check(const ref_dyn_params* p)
{
    if (!p) return -1;
    if (!isfinite(p->threshold_db) || !isfinite(p->slope) || !isfinite(p->knee_db) || !isfinite(p->alpha_attack) ||
        !isfinite(p->alpha_release) || !isfinite(p->makeup_db))
        return -1;
    if (p->threshold_db < -60.0 || p->threshold_db > 0.0 || p->slope < 0.0 || p->slope > 1.0 || p->knee_db < 0.0 || p->knee_db > 24.0) return -1;
    if (p->alpha_attack < 0.0 || p->alpha_attack >= 1.0 || p->alpha_release < 0.0 || p->alpha_release >= 1.0) return -1;
    if (p->makeup_db < -24.0 || p->makeup_db > 24.0 || p->lookahead < 0 || (p->link != 0 && p->link != 1)) return -1;
    if (p->lookahead > MAX_LOOKAHEAD) return -2;
    return 0;
}

/* steps 1 and 2: the gain-reduction demand of the magnitude a (f32, widened) */
static double demand(const ref_dyn_params* p, double half_knee, double inv_2knee, float af)
{
    const double a = (double)af;
    const double xg = a == 0.0 ? FLOOR_DB : K * ref_dyn_log2(a);
    const double u = xg - p->threshold_db;
    const double tu = 2.0 * u;
    if (tu < -p->knee_db) return 0.0;
    if (p->knee_db > 0.0 && fabs(tu) <= p->knee_db) {
        const double h = u + half_knee;
        return (p->slope * (h * h)) * inv_2knee;
    }
    return p->slope * u;
}

/* x: interleaved [in_len][ch]; one detector per stream (link = 1 and ch = 2) or per channel.  tiled != 0: steps 4 and 5 parallel in time,
 * as the GPU computes them; else the plain recurrences.  y (f32, rounded once), yd (the same in double, not rounded) and yl (the smoothed
 * reduction [in_len][detectors]) are each optional. */
static int run(const ref_dyn_params* p, const float* x, size_t in_len, int ch, int tiled, float* y, double* yd, double* yl_out)
{
    if (ref_dyn_check(p) || (ch != 1 && ch != 2) || (in_len && !x)) return -1;
    const int linked = p->link && ch == 2;
    const int n_det = linked ? 1 : ch, dc = linked ? 2 : 1;
    const size_t la = (size_t)p->lookahead;
    const double ar = p->alpha_release, aa = p->alpha_attack;
    const double omr = 1.0 - ar, oma = 1.0 - aa;
    const double half_knee = p->knee_db / 2.0, inv_2knee = p->knee_db > 0.0 ? 1.0 / (2.0 * p->knee_db) : 0.0;
    const size_t chunks = (in_len + C - 1) / C, padded = chunks * C;
    if (padded == 0) return 0;
    double* r = (double*)malloc((padded + la) * sizeof(double));
    double* d = (double*)malloc(padded * sizeof(double));
    if (!r || !d) { free(r); free(d); return -3; }
    for (int det = 0; det < n_det; det++) {
        const int c0 = linked ? 0 : det;
        /* 1, 2: level and static curve; input past in_len is zero */
        for (size_t n = 0; n < padded + la; n++) {
            float a = 0.0f;
            if (n < in_len)
                for (int c = 0; c < dc; c++) {
                    const float v = fabsf(x[n * ch + c0 + c]);
                    a = c == 0 ? v : (v > a ? v : a);
                }
            r[n] = demand(p, half_knee, inv_2knee, a);
        }
        /* 3: the look-ahead, an exact maximum */
        for (size_t n = 0; n < padded; n++) {
            double m = r[n];
            for (size_t t = 1; t <= la; t++) m = dmax(m, r[n + t]);
            d[n] = m;
        }
        double y1c = 0.0, ylc = 0.0;
        if (!tiled) {
            for (size_t n = 0; n < padded; n++) {
                y1c = dmax(d[n], (ar * y1c) + (omr * d[n]));
                ylc = (aa * ylc) + (oma * y1c);
                d[n] = ylc;
            }
        } else {
            double A[LANES], B[LANES], M[LANES], PA[LANES], PB[LANES], PM[LANES];
            for (size_t n0 = 0; n0 < padded; n0 += C) {
                double* v = d + n0;
                /* 4: every lane composes its steps from its first one; a step is y -> max(c, a y + b) with (a, b, c) = (ar, omr d, d) */
                for (int l = 0; l < LANES; l++) {
                    double a = ar, b = omr * v[l * T], m = v[l * T];
                    for (int k = 1; k < T; k++) {
                        const double bk = omr * v[l * T + k];
                        a = ar * a;
                        b = (ar * b) + bk;
                        m = dmax(v[l * T + k], (ar * m) + bk);
                    }
                    A[l] = a; B[l] = b; M[l] = m;
                }
                for (int j = 0; j < 6; j++) {
                    memcpy(PA, A, sizeof(A)); memcpy(PB, B, sizeof(B)); memcpy(PM, M, sizeof(M));
                    for (int l = 1 << j; l < LANES; l++) {
                        const int e = l - (1 << j);   /* the earlier map */
                        A[l] = PA[l] * PA[e];
                        B[l] = (PA[l] * PB[e]) + PB[l];
                        M[l] = dmax(PM[l], (PA[l] * PM[e]) + PB[l]);
                    }
                }
                const double in1 = y1c;
                for (int l = 0; l < LANES; l++) {
                    double s = l == 0 ? in1 : dmax(M[l - 1], (A[l - 1] * in1) + B[l - 1]);
                    for (int k = 0; k < T; k++) {
                        s = dmax(v[l * T + k], (ar * s) + (omr * v[l * T + k]));
                        v[l * T + k] = s;
                    }
                    if (l == LANES - 1) y1c = s;
                }
                /* 5: the same scheme with (a, b) = (aa, oma y1) */
                for (int l = 0; l < LANES; l++) {
                    double a = aa, b = oma * v[l * T];
                    for (int k = 1; k < T; k++) {
                        const double bk = oma * v[l * T + k];
                        a = aa * a;
                        b = (aa * b) + bk;
                    }
                    A[l] = a; B[l] = b;
                }
                for (int j = 0; j < 6; j++) {
                    memcpy(PA, A, sizeof(A)); memcpy(PB, B, sizeof(B));
                    for (int l = 1 << j; l < LANES; l++) {
                        const int e = l - (1 << j);
                        A[l] = PA[l] * PA[e];
                        B[l] = (PA[l] * PB[e]) + PB[l];
                    }
                }
                const double in2 = ylc;
                for (int l = 0; l < LANES; l++) {
                    double s = l == 0 ? in2 : (A[l - 1] * in2) + B[l - 1];
                    for (int k = 0; k < T; k++) {
                        s = (aa * s) + (oma * v[l * T + k]);
                        v[l * T + k] = s;
                    }
                    if (l == LANES - 1) ylc = s;
                }
            }
        }
        /* 6: the gain */
        for (size_t n = 0; n < in_len; n++) {
            const double g = ref_dyn_exp2((p->makeup_db - d[n]) * KINV);
            if (yl_out) yl_out[n * n_det + det] = d[n];
            for (int c = 0; c < dc; c++) {
                const double v = (double)x[n * ch + c0 + c] * g;
                if (y) y[n * ch + c0 + c] = (float)v;
                if (yd) yd[n * ch + c0 + c] = v;
            }
        }
    }
    free(r);
    free(d);
    return 0;
}

/* the tiled statement: what the GPU computes, bit for bit */
int ref_dyn_run(const ref_dyn_params* p, const float* x, size_t in_len, int ch, float* y) { return y ? run(p, x, in_len, ch, 1, y, NULL, NULL) : -1; }

/* the tiled statement in front of its final rounding */
int ref_dyn_run_f64(const ref_dyn_params* p, const float* x, size_t in_len, int ch, double* yd) { return yd ? run(p, x, in_len, ch, 1, NULL, yd, NULL) : -1; }

/* the plain sequential recurrence, not rounded; yl (optional): the smoothed reduction [in_len][detectors] */
int ref_dyn_sequential(const ref_dyn_params* p, const float* x, size_t in_len, int ch, double* yd, double* yl)
{
    return yd ? run(p, x, in_len, ch, 0, NULL, yd, yl) : -1;
}

/* nae_dyn_design of include/nae_gpu.h */
int ref_dyn_design(int sample_rate, double threshold_db, double ratio, double knee_db, double attack_s, double release_s, double lookahead_s,
                   double makeup_db, int link, ref_dyn_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1)) return -1;
    if (!isfinite(threshold_db) || isnan(ratio) || !isfinite(knee_db) || !isfinite(attack_s) || !isfinite(release_s) || !isfinite(lookahead_s) ||
        !isfinite(makeup_db))
        return -1;
    if (threshold_db < -60.0 || threshold_db > 0.0 || ratio < 1.0 || knee_db < 0.0 || knee_db > 24.0 || attack_s < 0.0 || attack_s > 0.5 ||
        release_s < 0.001 || release_s > 5.0 || makeup_db < -24.0 || makeup_db > 24.0 || lookahead_s < 0.0)
        return -1;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)MAX_LOOKAHEAD) return -2;
    const long n = lround(la);
    if (n > MAX_LOOKAHEAD) return -2;
    out->threshold_db = threshold_db;
    out->slope = isinf(ratio) ? 1.0 : 1.0 - 1.0 / ratio;
    out->knee_db = knee_db;
    out->alpha_attack = attack_s > 0.0 ? exp(-1.0 / (attack_s * (double)sample_rate)) : 0.0;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->makeup_db = makeup_db;
    out->lookahead = (int)n;
    out->link = link;
    return 0;
}
