/* ref_gate.c — the CPU statement of K19, the noise gate and downward expander ("K19 gate"): the tiled form the GPU computes,
 * bit for bit (ref_gate_run), the plain sequential form it is measured against (ref_gate_sequential: step 3 a brute-force search of the
 * window, step 5 the plain recurrence), the parameter rules (ref_gate_check) and the design (ref_gate_design).
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written here. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define T 16               /* NAE_DYN_LANE */
#define LANES 64
#define C (LANES * T)      /* NAE_DYN_CHUNK */
#define MAX_LOOKAHEAD 1024 /* NAE_DYN_MAX_LOOKAHEAD */
#define MAX_HOLD (1 << 21) /* NAE_GATE_MAX_HOLD */
#define FLOOR_DB (-1000.0) /* NAE_DYN_FLOOR_DB */

typedef struct ref_gate_params {   /* nae_gate_params of include/nae_gpu.h */
    float open_lin, close_lin;
    double threshold_db, slope, range_db, alpha_attack, alpha_release;
    int hold, lookahead, expand, link;
} ref_gate_params;

static const double K = 6.020599913279624;      /* 20 log10(2) */
static const double KINV = 0.1660964047443681;  /* 1 / K */

/* K12's dyn_log2 ("K12 dynamics") */
static double gate_log2(double a)
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

/* K12's dyn_exp2 */
static double gate_exp2(double t)
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

/* 0 when the parameters are acceptable, -1 invalid, -2 a look-ahead or a hold above its maximum */
int ref_gate_check(const ref_gate_params* p)
{
    if (!p) return -1;
    if (!isfinite(p->open_lin) || !isfinite(p->close_lin) || !isfinite(p->threshold_db) || !isfinite(p->slope) || !isfinite(p->range_db) ||
        !isfinite(p->alpha_attack) || !isfinite(p->alpha_release))
        return -1;
    if (!(p->close_lin > 0.0f) || p->close_lin > p->open_lin) return -1;
    if (p->threshold_db < -90.0 || p->threshold_db > 0.0 || p->slope < 0.0 || p->slope > 99.0 || p->range_db < 0.0 || p->range_db > 120.0) return -1;
    if (p->alpha_attack < 0.0 || p->alpha_attack >= 1.0 || p->alpha_release < 0.0 || p->alpha_release >= 1.0) return -1;
    if (p->hold < 0 || p->lookahead < 0 || (p->expand != 0 && p->expand != 1) || (p->link != 0 && p->link != 1)) return -1;
    if (p->lookahead > MAX_LOOKAHEAD || p->hold > MAX_HOLD) return -2;
    return 0;
}

/* step 4 */
static double depth_of(const ref_gate_params* p, float af)
{
    if (!p->expand) return p->range_db;
    const double a = (double)af;
    const double xg = a == 0.0 ? FLOOR_DB : K * gate_log2(a);
    const double u = p->threshold_db - xg;
    const double v = p->slope * u;
    return u <= 0.0 ? 0.0 : (v < p->range_db ? v : p->range_db);
}

/* x: interleaved [in_len][ch]; one detector per stream (link = 1 and ch = 2) or per channel.  tiled != 0: step 3 by the last set index and
 * step 5 parallel in time, as the GPU computes them; else the window searched sample by sample and the plain recurrence.  y (f32, rounded
 * once), yd (the same in double, not rounded), sm (the smoothed depth y[n], [in_len][detectors]), s_out and open_out (steps 2 and 3 as
 * bytes, [in_len][detectors]) are each optional. */
static int run(const ref_gate_params* p, const float* x, size_t in_len, int ch, int tiled, float* y, double* yd, double* sm, unsigned char* s_out,
               unsigned char* open_out)
{
    if (ref_gate_check(p) || (ch != 1 && ch != 2) || (in_len && !x)) return -1;
    const int linked = p->link && ch == 2;
    const int n_det = linked ? 1 : ch, dc = linked ? 2 : 1;
    const size_t la = (size_t)p->lookahead, hold = (size_t)p->hold;
    const double ar = p->alpha_release, aa = p->alpha_attack;
    const double omr = 1.0 - ar;
    const size_t chunks = (in_len + C - 1) / C, padded = chunks * C;
    if (padded == 0) return 0;
    float* a = (float*)malloc((padded + la) * sizeof(float));
    unsigned char* s = (unsigned char*)malloc(padded + la);
    unsigned char* open = (unsigned char*)malloc(padded);
    double* d = (double*)malloc(padded * sizeof(double));
    if (!a || !s || !open || !d) { free(a); free(s); free(open); free(d); return -3; }
    for (int det = 0; det < n_det; det++) {
        const int c0 = linked ? 0 : det;
        /* 1, 2: level and hysteresis; input past in_len is zero */
        unsigned char st = 0;
        for (size_t n = 0; n < padded + la; n++) {
            float v = 0.0f;
            if (n < in_len)
                for (int c = 0; c < dc; c++) {
                    const float b = fabsf(x[n * ch + c0 + c]);
                    v = c == 0 ? b : (b > v ? b : v);
                }
            a[n] = v;
            if (v >= p->open_lin) st = 1;
            else if (v < p->close_lin) st = 0;
            s[n] = st;
        }
        /* 3: hold and look-ahead */
        if (tiled) {
            size_t k = 0;
            long long last = -1;   /* the largest m <= n + la with s[m] = 1 */
            for (size_t n = 0; n < padded; n++) {
                for (; k <= n + la; k++)
                    if (s[k]) last = (long long)k;
                open[n] = last >= 0 && last >= (long long)n - (long long)hold;
            }
        } else {
            for (size_t n = 0; n < padded; n++) {
                const size_t lo = n > hold ? n - hold : 0;
                unsigned char o = 0;
                for (size_t m = n + la + 1; m-- > lo;)
                    if (s[m]) { o = 1; break; }
                open[n] = o;
            }
        }
        /* 4: the map of every sample: y -> (alpha y) + b; d holds b */
        for (size_t n = 0; n < padded; n++) d[n] = open[n] ? 0.0 : omr * depth_of(p, a[n]);
        /* 5 */
        double yc = p->range_db;
        if (!tiled) {
            for (size_t n = 0; n < padded; n++) {
                yc = ((open[n] ? aa : ar) * yc) + d[n];
                d[n] = yc;
            }
        } else {
            double A[LANES], B[LANES], PA[LANES], PB[LANES];
            for (size_t n0 = 0; n0 < padded; n0 += C) {
                double* v = d + n0;
                const unsigned char* o = open + n0;
                for (int l = 0; l < LANES; l++) {
                    double am = o[l * T] ? aa : ar, bm = v[l * T];
                    for (int k = 1; k < T; k++) {
                        const double ak = o[l * T + k] ? aa : ar;
                        am = ak * am;
                        bm = (ak * bm) + v[l * T + k];
                    }
                    A[l] = am; B[l] = bm;
                }
                for (int j = 0; j < 6; j++) {
                    memcpy(PA, A, sizeof(A)); memcpy(PB, B, sizeof(B));
                    for (int l = 1 << j; l < LANES; l++) {
                        const int e = l - (1 << j);   /* the earlier map */
                        A[l] = PA[l] * PA[e];
                        B[l] = (PA[l] * PB[e]) + PB[l];
                    }
                }
                const double in = yc;
                for (int l = 0; l < LANES; l++) {
                    double t = l == 0 ? in : (A[l - 1] * in) + B[l - 1];
                    for (int k = 0; k < T; k++) {
                        t = ((o[l * T + k] ? aa : ar) * t) + v[l * T + k];
                        v[l * T + k] = t;
                    }
                    if (l == LANES - 1) yc = t;
                }
            }
        }
        /* 6: the gain */
        for (size_t n = 0; n < in_len; n++) {
            const double g = gate_exp2((0.0 - d[n]) * KINV);
            if (sm) sm[n * n_det + det] = d[n];
            if (s_out) s_out[n * n_det + det] = s[n];
            if (open_out) open_out[n * n_det + det] = open[n];
            for (int c = 0; c < dc; c++) {
                const double v = (double)x[n * ch + c0 + c] * g;
                if (y) y[n * ch + c0 + c] = (float)v;
                if (yd) yd[n * ch + c0 + c] = v;
            }
        }
    }
    free(a); free(s); free(open); free(d);
    return 0;
}

/* the tiled statement: what the GPU computes, bit for bit */
int ref_gate_run(const ref_gate_params* p, const float* x, size_t in_len, int ch, float* y) { return y ? run(p, x, in_len, ch, 1, y, NULL, NULL, NULL, NULL) : -1; }

/* either form with everything it makes: yd not rounded, sm the smoothed depth, s and open the integer decisions (each optional) */
int ref_gate_full(const ref_gate_params* p, const float* x, size_t in_len, int ch, int tiled, float* y, double* yd, double* sm, unsigned char* s,
                  unsigned char* open)
{
    return run(p, x, in_len, ch, tiled, y, yd, sm, s, open);
}

/* nae_gate_design of include/nae_gpu.h */
int ref_gate_design(int sample_rate, int mode, double threshold_db, double hysteresis_db, double range_db, double ratio, double attack_s,
                    double hold_s, double release_s, double lookahead_s, int link, ref_gate_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1) || (mode != 0 && mode != 1)) return -1;
    if (!isfinite(threshold_db) || !isfinite(hysteresis_db) || !isfinite(range_db) || !isfinite(ratio) || !isfinite(attack_s) || !isfinite(hold_s) ||
        !isfinite(release_s) || !isfinite(lookahead_s))
        return -1;
    if (threshold_db < -90.0 || threshold_db > 0.0 || hysteresis_db < 0.0 || hysteresis_db > 24.0 || range_db < 0.0 || range_db > 120.0 ||
        ratio < 1.0 || ratio > 100.0 || attack_s < 0.0 || attack_s > 0.5 || hold_s < 0.0 || hold_s > 10.0 || release_s < 0.001 || release_s > 5.0 ||
        lookahead_s < 0.0)
        return -1;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)MAX_LOOKAHEAD) return -2;
    const long n = lround(la);
    if (n > MAX_LOOKAHEAD) return -2;
    const double hd = hold_s * (double)sample_rate;
    if (hd > 2.0 * (double)MAX_HOLD) return -2;
    const long nh = lround(hd);
    if (nh > MAX_HOLD) return -2;
    out->open_lin = (float)pow(10.0, threshold_db / 20.0);
    out->close_lin = (float)pow(10.0, (threshold_db - hysteresis_db) / 20.0);
    out->threshold_db = threshold_db;
    out->slope = ratio - 1.0;
    out->range_db = range_db;
    out->alpha_attack = attack_s > 0.0 ? exp(-1.0 / (attack_s * (double)sample_rate)) : 0.0;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->hold = (int)nh;
    out->lookahead = (int)n;
    out->expand = mode;
    out->link = link;
    return 0;
}
