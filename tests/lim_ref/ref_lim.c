/* ref_lim.c — the CPU statement of K22, the true-peak look-ahead limiter ("K22 limiter"): the tiled form the GPU computes, bit
 * for bit (ref_lim_run), the plain sequential form it is measured against (step 3 and step 5 brute-force searches and sums of the window,
 * step 4 the plain recurrence), the parameter rules (ref_lim_check) and the design (ref_lim_design).  It stands on K12's statement
 * (dyn_ref/ref_dyn.c: ref_dyn_log2, ref_dyn_exp2, the tiling) and on K14's true-peak taps (loud_ref/ref_loud.c: ref_loud_taps).
 * Built with -ffp-contract=off: every step is one IEEE operation in the order written here. */
#include "../loud_ref/ref_loud.c"
#include "../dyn_ref/ref_dyn.c"

#define REACH 6                        /* NAE_LIM_TP_REACH */
#define LIM_MAX_LOOKAHEAD (C - REACH)  /* NAE_LIM_MAX_LOOKAHEAD */
#define Q_SCALE 16777216.0             /* NAE_LIM_Q_SCALE */

typedef struct ref_lim_params {   /* nae_lim_params of include/nae_gpu.h */
    double ceiling_db, gain_db, alpha_release;
    int lookahead, true_peak, link;
} ref_lim_params;

/* 0 when the parameters are acceptable, -1 invalid, -2 a look-ahead above its maximum */
int ref_lim_check(const ref_lim_params* p)
{
    if (!p) return -1;
    if (!isfinite(p->ceiling_db) || !isfinite(p->gain_db) || !isfinite(p->alpha_release)) return -1;
    if (p->ceiling_db < -20.0 || p->ceiling_db > 0.0 || p->gain_db < -24.0 || p->gain_db > 24.0) return -1;
    if (p->alpha_release < 0.0 || p->alpha_release >= 1.0) return -1;
    if (p->lookahead < 0 || (p->true_peak != 0 && p->true_peak != 1) || (p->link != 0 && p->link != 1)) return -1;
    if (p->lookahead > LIM_MAX_LOOKAHEAD) return -2;
    return 0;
}

/* sample n of channel c, zero outside [0, in_len) */
static float lim_x(const float* x, size_t in_len, int ch, int c, long long n) { return n >= 0 && (size_t)n < in_len ? x[(size_t)n * ch + c] : 0.0f; }

/* x: interleaved [in_len][ch]; one detector per stream (link = 1 and ch = 2) or per channel.  tiled != 0: step 3 by a monotonic queue, step 4
 * parallel in time and step 5 by wrapping prefix sums, as the GPU computes them; else the windows searched and summed sample by sample and the
 * plain recurrence.  y (f32, rounded once), yd (the same in double, not rounded), and per detector [in_len][detectors] r_out (the demand),
 * s_out (the smoothed reduction), y1_out (the release's output) and w_out (the integer sums W) are each optional. */
static int lim_run(const ref_lim_params* p, const float* x, size_t in_len, int ch, int tiled, float* y, double* yd, double* r_out, double* s_out,
                   double* y1_out, int64_t* w_out)
{
    if (ref_lim_check(p) || (ch != 1 && ch != 2) || (in_len && !x)) return -1;
    const int linked = p->link && ch == 2;
    const int n_det = linked ? 1 : ch, dc = linked ? 2 : 1;
    const size_t la = (size_t)p->lookahead;
    const double ar = p->alpha_release;
    const double omr = 1.0 - ar;
    const double denom = (double)((int64_t)(la + 1) * (int64_t)Q_SCALE);
    const size_t chunks = (in_len + C - 1) / C, padded = chunks * C;
    if (padded == 0) return 0;
    float taps[PHASES * TAPS];
    ref_loud_taps(taps);
    float* e = (float*)malloc((padded + la + REACH + 1) * sizeof(float));
    double* r = (double*)malloc((padded + la) * sizeof(double));
    double* d = (double*)malloc(padded * sizeof(double));
    int64_t* q = (int64_t*)malloc(padded * sizeof(int64_t));
    uint64_t* S = (uint64_t*)malloc(padded * sizeof(uint64_t));
    uint64_t* Wv = (uint64_t*)malloc(padded * sizeof(uint64_t));
    size_t* dq = (size_t*)malloc((padded + la) * sizeof(size_t));
    if (!e || !r || !d || !q || !S || !Wv || !dq) { free(e); free(r); free(d); free(q); free(S); free(Wv); free(dq); return -3; }
    for (int det = 0; det < n_det; det++) {
        const int c0 = linked ? 0 : det;
        /* 1, 2: level and demand */
        float* L = (float*)malloc((padded + la) * sizeof(float));
        if (!L) { free(e); free(r); free(d); free(q); free(S); free(Wv); free(dq); return -3; }
        for (int c = 0; c < dc; c++) {
            if (p->true_peak)
                for (size_t m = 0; m < padded + la + REACH + 1; m++) {
                    float em = 0.0f;
                    for (int ph = 0; ph < PHASES; ph++) {
                        float v = taps[ph * TAPS] * lim_x(x, in_len, ch, c0 + c, (long long)m);
                        for (int t = 1; t < TAPS; t++) v = v + taps[ph * TAPS + t] * lim_x(x, in_len, ch, c0 + c, (long long)m - t);
                        const float av = fabsf(v);
                        em = av > em ? av : em;
                    }
                    e[m] = em;
                }
            for (size_t n = 0; n < padded + la; n++) {
                float m = fabsf(lim_x(x, in_len, ch, c0 + c, (long long)n));
                if (p->true_peak) {
                    m = e[n + 5] > m ? e[n + 5] : m;
                    m = e[n + 6] > m ? e[n + 6] : m;
                }
                L[n] = c == 0 ? m : (m > L[n] ? m : L[n]);
            }
        }
        for (size_t n = 0; n < padded + la; n++) {
            const double a = (double)L[n];
            const double lg = K * ref_dyn_log2(a);
            const double xg = a == 0.0 ? FLOOR_DB : lg;
            const double u = (xg + p->gain_db) - p->ceiling_db;
            r[n] = u > 0.0 ? u : 0.0;
        }
        free(L);
        /* 3: the look-ahead, an exact maximum */
        if (tiled) {
            size_t head = 0, tail = 0, k = 0;   /* dq[head ... tail): indices of falling r */
            for (size_t n = 0; n < padded; n++) {
                for (; k <= n + la; k++) {
                    while (tail > head && !(r[dq[tail - 1]] > r[k])) tail--;
                    dq[tail++] = k;
                }
                while (dq[head] < n) head++;
                d[n] = r[dq[head]];
            }
        } else {
            for (size_t n = 0; n < padded; n++) {
                double m = r[n];
                for (size_t t = 1; t <= la; t++) m = dmax(m, r[n + t]);
                d[n] = m;
            }
        }
        /* 4: the release */
        double y1c = 0.0;
        if (!tiled) {
            for (size_t n = 0; n < padded; n++) {
                y1c = dmax(d[n], (ar * y1c) + (omr * d[n]));
                d[n] = y1c;
            }
        } else {
            double A[LANES], B[LANES], M[LANES], PA[LANES], PB[LANES], PM[LANES];
            for (size_t n0 = 0; n0 < padded; n0 += C) {
                double* v = d + n0;
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
                        const int f = l - (1 << j);   /* the earlier map */
                        A[l] = PA[l] * PA[f];
                        B[l] = (PA[l] * PB[f]) + PB[l];
                        M[l] = dmax(PM[l], (PA[l] * PM[f]) + PB[l]);
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
            }
        }
        /* 5: the attack, in integers; q[n] = q[0] for n < 0 */
        for (size_t n = 0; n < padded; n++) {
            const double sc = d[n] * Q_SCALE;
            const double cl = ceil(sc);
            const double fin = fabs(cl) < 9.0e18 ? cl : 0.0;   /* not finite: 0, so the conversion is defined */
            q[n] = (int64_t)fin;
        }
        if (tiled) {
            uint64_t run = 0;
            for (size_t n = 0; n < padded; n++) {
                run += (uint64_t)q[n];
                S[n] = run;
            }
            for (size_t n = 0; n < padded; n++) {
                /* the prefix sum at n - la - 1; below 0 it is (m + 1) q[0], modulo 2^64 */
                const long long m = (long long)n - (long long)la - 1;
                const uint64_t below = m >= 0 ? S[m] : (0ull - (uint64_t)(-(m + 1))) * (uint64_t)q[0];
                Wv[n] = S[n] - below;
            }
        } else {
            for (size_t n = 0; n < padded; n++) {
                int64_t w = 0;
                for (size_t t = 0; t <= la; t++) w += t <= n ? q[n - t] : q[0];
                Wv[n] = (uint64_t)w;
            }
        }
        /* 6: the gain */
        for (size_t n = 0; n < in_len; n++) {
            const int64_t W = (int64_t)Wv[n];
            const double s = (double)W / denom;
            const double g = ref_dyn_exp2((p->gain_db - s) * KINV);
            if (r_out) r_out[n * n_det + det] = r[n];
            if (s_out) s_out[n * n_det + det] = s;
            if (y1_out) y1_out[n * n_det + det] = d[n];
            if (w_out) w_out[n * n_det + det] = W;
            for (int c = 0; c < dc; c++) {
                const double v = (double)x[n * ch + c0 + c] * g;
                if (y) y[n * ch + c0 + c] = (float)v;
                if (yd) yd[n * ch + c0 + c] = v;
            }
        }
    }
    free(e); free(r); free(d); free(q); free(S); free(Wv); free(dq);
    return 0;
}

/* the tiled statement: what the GPU computes, bit for bit */
int ref_lim_run(const ref_lim_params* p, const float* x, size_t in_len, int ch, float* y) { return y ? lim_run(p, x, in_len, ch, 1, y, NULL, NULL, NULL, NULL, NULL) : -1; }

/* either form with everything it makes (each optional) */
int ref_lim_full(const ref_lim_params* p, const float* x, size_t in_len, int ch, int tiled, float* y, double* yd, double* r, double* s, double* y1,
                 int64_t* w)
{
    return lim_run(p, x, in_len, ch, tiled, y, yd, r, s, y1, w);
}

/* nae_lim_design of include/nae_gpu.h */
int ref_lim_design(int sample_rate, double ceiling_db, double gain_db, double release_s, double lookahead_s, int true_peak, int link,
                   ref_lim_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1) || (true_peak != 0 && true_peak != 1)) return -1;
    if (!isfinite(ceiling_db) || !isfinite(gain_db) || !isfinite(release_s) || !isfinite(lookahead_s)) return -1;
    if (ceiling_db < -20.0 || ceiling_db > 0.0 || gain_db < -24.0 || gain_db > 24.0 || release_s < 0.001 || release_s > 5.0 || lookahead_s < 0.0) return -1;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)LIM_MAX_LOOKAHEAD) return -2;
    const long n = lround(la);
    if (n > LIM_MAX_LOOKAHEAD) return -2;
    out->ceiling_db = ceiling_db;
    out->gain_db = gain_db;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->lookahead = (int)n;
    out->true_peak = true_peak;
    out->link = link;
    return 0;
}
