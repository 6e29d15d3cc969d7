/* ref_pv_formant.c — CPU statement of the K7 phase vocoder with formant preservation ("Formant preservation").
 *
 * One statement with the frame size N, the phase lock and the lifter q as parameters.  The loops restate tests/pv_sizes/ref_pv_sizes.c
 * (every size, the canonical FFT written plainly) and, with lock = 1 (N = 1024 only), the locked Qs recurrence of tests/pv_lock/ref_pv_lock.c.
 * With q = 0 it is those two statements bit for bit (tests/test_pv_formant_cpu.py).  With q > 0 and both stages on (pv_on and rs_on), every
 * synthesis frame's magnitudes are multiplied by G[k] of the frame's cepstral envelope; everything else is unchanged.  The atan2 and the
 * transposer's table are the oracle's own (linked from oracle/libnae_oracle.so).  Built by its tests with gcc -ffp-contract=off.
 */
#include "../../oracle/nae_oracle.h"
#include "../../include/nae_dsp_spec.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y; } cf;

static cf cadd(cf a, cf b) { cf r = {a.x + b.x, a.y + b.y}; return r; }
static cf csub(cf a, cf b) { cf r = {a.x - b.x, a.y - b.y}; return r; }
static cf mul_mi(cf a) { cf r = {a.y, -a.x}; return r; }
static cf cmul_tw(cf v, cf w)
{
    cf r;
    r.x = fmaf(-v.y, w.y, v.x * w.x);
    r.y = fmaf(v.y, w.x, v.x * w.y);
    return r;
}

/* canonical DFT2 / DFT4 / DFT8: radix-2 DIF layers, natural-order output */
static void dft(int R, const cf* a, cf* b)
{
    if (R == 2) {
        b[0] = cadd(a[0], a[1]);
        b[1] = csub(a[0], a[1]);
    } else if (R == 4) {
        const cf s0 = cadd(a[0], a[2]), d0 = csub(a[0], a[2]), s1 = cadd(a[1], a[3]), d1 = mul_mi(csub(a[1], a[3]));
        b[0] = cadd(s0, s1); b[2] = csub(s0, s1); b[1] = cadd(d0, d1); b[3] = csub(d0, d1);
    } else {
        const float c = 0.70710678118654752440f;
        const cf s0 = cadd(a[0], a[4]), d0 = csub(a[0], a[4]);
        const cf s1 = cadd(a[1], a[5]), e1 = csub(a[1], a[5]);
        const cf s2 = cadd(a[2], a[6]), e2 = csub(a[2], a[6]);
        const cf s3 = cadd(a[3], a[7]), e3 = csub(a[3], a[7]);
        const cf d1 = {(e1.x + e1.y) * c, (e1.y - e1.x) * c};
        const cf d2 = mul_mi(e2);
        const cf d3 = {(e3.y - e3.x) * c, -((e3.x + e3.y) * c)};
        const cf t0 = cadd(s0, s2), t1 = csub(s0, s2), t2 = cadd(s1, s3), t3 = mul_mi(csub(s1, s3));
        b[0] = cadd(t0, t2); b[4] = csub(t0, t2); b[2] = cadd(t1, t3); b[6] = csub(t1, t3);
        const cf u0 = cadd(d0, d2), u1 = csub(d0, d2), u2 = cadd(d1, d3), u3 = mul_mi(csub(d1, d3));
        b[1] = cadd(u0, u2); b[5] = csub(u0, u2); b[3] = cadd(u1, u3); b[7] = csub(u1, u3);
    }
}

/* DIF FFT of MT points (a block of the M-point transform): first pass radix R1 (M = R1 * 8^s), every later pass radix 8; output q >= 1 of
 * butterfly l is multiplied by W_M[(M/MT) l q] unless MT == R.  Output q of butterfly l is point l of sub-transform q, whose bin k' is bin
 * q + R k' of this block. */
static void fft_dif(const cf* in, int MT, int M, int R1, const cf* WM, cf* out)
{
    const int R = MT == M ? R1 : 8, S = MT / R;
    cf* u = (cf*)malloc(sizeof(cf) * MT);
    cf* sub = (cf*)malloc(sizeof(cf) * S);
    cf a[8], b[8];
    for (int l = 0; l < S; l++) {
        for (int j = 0; j < R; j++) a[j] = in[l + S * j];
        dft(R, a, b);
        for (int q = 0; q < R; q++) u[q * S + l] = (q == 0 || MT == R) ? b[q] : cmul_tw(b[q], WM[(M / MT) * l * q]);
    }
    for (int q = 0; q < R; q++) {
        if (S == 1)
            sub[0] = u[q];
        else
            fft_dif(u + q * S, S, M, R1, WM, sub);
        for (int k = 0; k < S; k++) out[q + R * k] = sub[k];
    }
    free(sub);
    free(u);
}

static int size_ok(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

/* tables of one size, in double, rounded once to f32 */
typedef struct { int N, M, R1; float* hann; cf* TN; cf* WM; } tables;

static void tables_make(tables* t, int N)
{
    const double two_pi = 6.283185307179586476925286766559;
    const int M = N / 2;
    int lg = 0;
    while ((1 << lg) < M) lg++;
    t->N = N;
    t->M = M;
    t->R1 = lg % 3 == 0 ? 8 : (1 << (lg % 3));
    t->hann = (float*)malloc(sizeof(float) * N);
    t->TN = (cf*)malloc(sizeof(cf) * (M + 1));
    t->WM = (cf*)malloc(sizeof(cf) * M);
    for (int n = 0; n < N; n++) t->hann[n] = (float)(0.5 - 0.5 * cos(two_pi * n / (double)N));
    for (int k = 0; k <= M; k++) { t->TN[k].x = (float)cos(two_pi * k / (double)N); t->TN[k].y = (float)(-sin(two_pi * k / (double)N)); }
    for (int k = 0; k < M; k++) { t->WM[k].x = (float)cos(two_pi * k / (double)M); t->WM[k].y = (float)(-sin(two_pi * k / (double)M)); }
}

static void tables_free(tables* t) { free(t->hann); free(t->TN); free(t->WM); }

/* canonical r2c: pack pairs, M-point FFT, split */
static void rfft(const tables* t, const float* xw, cf* X)
{
    const int M = t->M;
    cf* Z = (cf*)malloc(sizeof(cf) * M);
    fft_dif((const cf*)xw, M, M, t->R1, t->WM, Z);
    for (int k = 0; k <= M; k++) {
        const cf A = Z[k & (M - 1)], B = Z[(M - k) & (M - 1)];
        const cf E = {0.5f * (A.x + B.x), 0.5f * (A.y - B.y)};
        const cf O = {0.5f * (A.x - B.x), 0.5f * (A.y + B.y)};
        const cf P = cmul_tw(O, t->TN[k]);
        X[k].x = E.x + P.y;
        X[k].y = E.y - P.x;
    }
    free(Z);
}

/* c2r, 1/N normalised: split with T_N, conjugate, forward FFT_M, scale (the oracle's irfft1024 at every size) */
static void irfft(const tables* t, const cf* X, float* y)
{
    const int M = t->M;
    cf* Zc = (cf*)malloc(sizeof(cf) * M);
    cf* z = (cf*)malloc(sizeof(cf) * M);
    for (int k = 0; k < M; k++) {
        cf Xk = X[k], Xm = X[M - k];
        if (k == 0) { Xk.y = 0.0f; Xm.y = 0.0f; }
        const cf E = {0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y - Xm.y)};
        const cf D = {0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y + Xm.y)};
        const cf T = t->TN[k];
        const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x}; /* conj(T) * D */
        Zc[k].x = E.x - Q.y;
        Zc[k].y = -(E.y + Q.x);
    }
    fft_dif(Zc, M, M, t->R1, t->WM, z);
    const float scale = 1.0f / (float)M;
    for (int m = 0; m < M; m++) {
        y[2 * m] = z[m].x * scale;
        y[2 * m + 1] = -z[m].y * scale;
    }
    free(Zc);
    free(z);
}

/* the plan at frame size N: the oracle's, with the hop, the ratios and the frame count of N */
int ref_formant_plan(double rate, double pitch, int N, size_t in_len, orc_stretch_plan* pl)
{
    if (!size_ok(N)) return -3;
    const int rc = orc_stretch_plan_make(rate, pitch, in_len, pl);
    if (rc) return rc;
    const int H = N / 4;
    pl->ha_q24 = (int64_t)llround((double)H * pl->tempo_eff * (double)(1 << NAE_HA_FRAC_BITS));
    pl->d0 = (int32_t)(pl->ha_q24 >> NAE_HA_FRAC_BITS);
    for (int i = 0; i < 2; i++) {
        const uint64_t d = (uint64_t)(pl->d0 + i);
        pl->r_q24[i] = (uint32_t)((((uint64_t)H << NAE_R_FRAC_BITS) + d / 2) / d);
    }
    const size_t pv_out = pl->rs_first ? pl->out_len : pl->mid_len;
    pl->frames = pl->pv_on ? (pv_out + N / 2 + H - 1) / H + 1 : 0;
    return 0;
}

static inline int64_t frame_start(const orc_stretch_plan* pl, int N, int64_t f)
{
    return (((f - 1) * pl->ha_q24 + ((int64_t)1 << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - N / 2;
}

/* phase locking, rules 2 and 3 of DESIGN.md §3 over BINS bins: sigma[k] = the nearest peak of P, a tie to the lower one; no peak: k */
static void regions(const float* P, int BINS, int* sigma)
{
    unsigned char* peak = (unsigned char*)malloc((size_t)BINS);
    int n = 0;
    for (int k = 0; k < BINS; k++) {
        int ok = P[k] > 0.0f;
        if (k >= 1) ok = ok && P[k] > P[k - 1];
        if (k >= 2) ok = ok && P[k] > P[k - 2];
        if (k + 1 < BINS) ok = ok && P[k] >= P[k + 1];
        if (k + 2 < BINS) ok = ok && P[k] >= P[k + 2];
        peak[k] = (unsigned char)ok;
        n += ok;
    }
    for (int k = 0; k < BINS; k++) {
        if (!n) { sigma[k] = k; continue; }
        int best = -1;
        for (int p = 0; p < BINS; p++)
            if (peak[p] && (best < 0 || abs(k - p) < abs(k - best))) best = p;
        sigma[k] = best;
    }
    free(peak);
}

/* formant preservation, steps 1-5: G[0..M] of one frame's analysis spectrum X, lifter q, transposer ratio g */
static void ref_formant_gain(const tables* t, const cf* X, int q, float g, float* G)
{
    const int N = t->N, M = t->M;
    cf* Lc = (cf*)malloc(sizeof(cf) * (M + 1));
    cf* E = (cf*)malloc(sizeof(cf) * (M + 1));
    float* c = (float*)malloc(sizeof(float) * N);
    float* Ls = (float*)malloc(sizeof(float) * (M + 1));
    for (int k = 0; k <= M; k++) {
        const float mag = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
        Lc[k].x = log2f(fmaxf(mag, 0x1p-40f));
        Lc[k].y = 0.0f;
    }
    irfft(t, Lc, c);
    for (int n = 0; n < N; n++)
        if (!(n < q || n > N - q)) c[n] = 0.0f;
    rfft(t, c, E);
    for (int k = 0; k <= M; k++) Ls[k] = E[k].x;
    for (int k = 0; k <= M; k++) {
        const float u = (float)k * g;
        if (u > (float)M) {
            G[k] = 0.0f;
            continue;
        }
        const int i = (int)u;
        const float tt = u - (float)i;
        const float lu = (i == M) ? Ls[M] : Ls[i] + tt * (Ls[i + 1] - Ls[i]);
        G[k] = fminf(exp2f(lu - Ls[k]), NAE_FORMANT_MAX_GAIN);
    }
    free(Lc); free(E); free(c); free(Ls);
}

/* one channel of the vocoder stage; v[0..Mlen) is overwritten.  q > 0: formant preservation with ratio g */
static void pv_channel(const tables* t, const float* src, size_t L, int ch, int c, const orc_stretch_plan* pl, size_t Mlen, float* v, int lock,
                       int q, float g)
{
    const int N = t->N, H = N / 4, BINS = N / 2 + 1, b = N == 512 ? 9 : N == 1024 ? 10 : N == 2048 ? 11 : 12;
    float* xw = (float*)malloc(sizeof(float) * N);
    float* y = (float*)malloc(sizeof(float) * N);
    float* P = (float*)malloc(sizeof(float) * BINS);
    float* G = (float*)malloc(sizeof(float) * BINS);
    cf* X = (cf*)malloc(sizeof(cf) * BINS);
    cf* Y = (cf*)malloc(sizeof(cf) * BINS);
    uint32_t* qa = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qa_prev = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qs = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qs_old = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* inc = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    int* sigma = (int*)malloc(sizeof(int) * BINS);
    const double two_pi = 6.283185307179586476925286766559;
    memset(v, 0, Mlen * sizeof(float));
    int64_t s_prev = 0;
    for (size_t f = 0; f < pl->frames; f++) {
        const int64_t s = frame_start(pl, N, (int64_t)f);
        for (int n = 0; n < N; n++) {
            const int64_t i = s + n;
            const float x = (i >= 0 && (uint64_t)i < L) ? src[(size_t)i * ch + c] : 0.0f;
            xw[n] = x * t->hann[n];
        }
        rfft(t, xw, X);
        for (int k = 0; k < BINS - 1; k++) qa[k] = (uint32_t)orc_atan2_q32(X[k].y, X[k].x);
        qa[BINS - 1] = (X[BINS - 1].x < 0.0f) ? 0x80000000u : 0u;
        if (f == 0)
            memcpy(qs, qa, sizeof(uint32_t) * BINS);
        else {
            const int64_t d = s - s_prev;
            const uint32_t R = pl->r_q24[d - pl->d0];
            for (int k = 0; k < BINS; k++) {
                const uint32_t e = (uint32_t)(((uint64_t)k * (uint64_t)d) & (uint64_t)(N - 1)) << (32 - b);
                const int32_t dw = (int32_t)(qa[k] - qa_prev[k] - e);
                const uint32_t adv = (uint32_t)(((uint64_t)k * (uint64_t)H) & (uint64_t)(N - 1)) << (32 - b);
                const int64_t scaled = ((int64_t)dw * (int64_t)R + ((int64_t)1 << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
                inc[k] = adv + (uint32_t)scaled;
            }
            if (!lock) {
                for (int k = 0; k < BINS; k++) qs[k] += inc[k];
            } else {
                for (int k = 0; k < BINS; k++) P[k] = X[k].x * X[k].x + X[k].y * X[k].y;
                regions(P, BINS, sigma);
                memcpy(qs_old, qs, sizeof(uint32_t) * BINS);
                for (int k = 0; k < BINS; k++) {
                    const int p = sigma[k];
                    qs[k] = qs_old[p] + (inc[p] + (qa[k] - qa[p]));
                }
            }
        }
        memcpy(qa_prev, qa, sizeof(uint32_t) * BINS);
        s_prev = s;
        if (q > 0) ref_formant_gain(t, X, q, g, G);
        for (int k = 0; k < BINS; k++) {
            float mag = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
            if (q > 0) mag = G[k] * mag;
            const double ph = two_pi * ((double)(int32_t)qs[k] * (1.0 / 4294967296.0));
            Y[k].x = mag * (float)cos(ph);
            Y[k].y = mag * (float)sin(ph);
        }
        irfft(t, Y, y);
        const int64_t o = ((int64_t)f - 1) * H - N / 2;
        for (int n = 0; n < N; n++) {
            const int64_t m = o + n;
            if (m >= 0 && (uint64_t)m < Mlen) v[m] += t->hann[n] * y[n];
        }
    }
    for (size_t m = 0; m < Mlen; m++) v[m] *= NAE_OLA_GAIN;
    free(xw); free(y); free(P); free(G); free(X); free(Y); free(qa); free(qa_prev); free(qs); free(qs_old); free(inc); free(sigma);
}

static void rs_channel(const float* v, size_t M, size_t vstride, const orc_stretch_plan* pl, size_t n_out, const float* tab,
                       float* dst, int ch, int c)
{
    for (size_t j = 0; j < n_out; j++) {
        const unsigned __int128 pos = (unsigned __int128)j * pl->step_q32;
        const int64_t idx = (int64_t)(pos >> 32);
        const uint32_t frac = (uint32_t)pos;
        const uint32_t ph = frac >> 25;
        const float alpha = (float)(frac & 0x1FFFFFFu) * (1.0f / 33554432.0f);
        const float* t0 = tab + ph * NAE_RS_TAPS;
        const float* t1 = t0 + NAE_RS_TAPS;
        float acc = 0.0f;
        for (int i = 0; i < NAE_RS_TAPS; i++) {
            const int64_t m = idx - (NAE_RS_TAPS / 2 - 1) + i;
            const float x = (m >= 0 && (uint64_t)m < M) ? v[(size_t)m * vstride] : 0.0f;
            const float coef = t0[i] + alpha * (t1[i] - t0[i]);
            acc += coef * x;
        }
        dst[j * (size_t)ch + c] = acc;
    }
}

/* the whole node at frame size N, phase lock `lock` (N = 1024 only), lifter q (0: off; it applies only with both stages on);
 * dst holds plan.out_len * ch floats */
int ref_formant_stretch(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, float* dst)
{
    orc_stretch_plan pl;
    const int rc = ref_formant_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (q < 0 || q > N / 4) return -1;
    if (!pl.pv_on && !pl.rs_on) {
        memmove(dst, src, L * (size_t)ch * sizeof(float));
        return 0;
    }
    if (!(pl.pv_on && pl.rs_on)) q = 0;
    const float g = (float)pl.rate_eff;
    tables t;
    tables_make(&t, N);
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    float* v = pl.pv_on ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
    float* w = pl.rs_first ? (float*)malloc((pl.out_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, v, 1, 0);
            pv_channel(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, w, lock, q, g);
            for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = w[m];
        } else if (pl.pv_on) {
            pv_channel(&t, src, L, ch, c, &pl, pl.mid_len, v, lock, q, g);
            if (pl.rs_on) rs_channel(v, pl.mid_len, 1, &pl, pl.out_len, tab, dst, ch, c);
            else
                for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = v[m];
        } else
            rs_channel(src + c, L, (size_t)ch, &pl, pl.out_len, tab, dst, ch, c);
    }
    free(v);
    free(w);
    tables_free(&t);
    return 0;
}
