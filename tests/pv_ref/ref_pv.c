/* ref_pv.c — CPU statement of the K7 phase vocoder ("Phase locking", "Formant preservation").
 *
 * The loops of oracle/orc_stft.c (plan, pv_channel, rs_channel, the stage order of orc_stretch_f32, orc_pv_synth_phase) with the frame size
 * N = 512 ... 4096 (hop H = N / 4), the phase lock (N = 1024 only) and the formant lifter q as parameters.  The FFT is the canonical one of
 * every size (tests/ref_fft.h); the inverse is the oracle's irfft1024 generalised (split with T_N, conjugate, forward FFT_{N/2}, scale).
 * lock = 1 replaces the Qs recurrence of frames f >= 1 by the locked one.  With q > 0 and both stages on (pv_on and rs_on), every synthesis
 * frame's magnitudes are multiplied by G[k] of the frame's cepstral envelope.  At N = 1024, unlocked, q = 0 it equals orc_stretch_f32 and
 * orc_pv_synth_phase bit for bit; its integer phases elsewhere are pinned by tests/golden/pv_synth_phase.json (tests/test_pv_formant_cpu.py).
 * The atan2 and the transposer's table are the oracle's own (linked from oracle/libnae_oracle.so).  Built by its tests with gcc
 * -ffp-contract=off.
 */
#include "../../oracle/nae_oracle.h"
#include "../../include/nae_dsp_spec.h"
#include "../ref_fft.h"
#include <string.h>

static int size_ok(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

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
int ref_pv_plan(double rate, double pitch, int N, size_t in_len, orc_stretch_plan* pl)
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

/* phase locking, rule 2 of DESIGN.md §3: the peaks of the power spectrum P[0..BINS); a neighbour outside 0..BINS-1 counts as satisfied, a
 * NaN compares false.  Returns the number of peaks. */
static int peaks(const float* P, int BINS, unsigned char* peak)
{
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
    return n;
}

/* rule 3: sigma[k] = the nearest peak of P, a tie to the lower one; no peak at all: k */
static void regions(const float* P, int BINS, int* sigma)
{
    unsigned char* peak = (unsigned char*)malloc((size_t)BINS);
    const int n = peaks(P, BINS, peak);
    for (int k = 0; k < BINS; k++) {
        if (!n) { sigma[k] = k; continue; }
        int best = -1;
        for (int p = 0; p < BINS; p++)
            if (peak[p] && (best < 0 || abs(k - p) < abs(k - best))) best = p;   /* ascending p: a tie keeps the lower peak */
        sigma[k] = best;
    }
    free(peak);
}

/* the rules at N = 1024 (513 bins), for tests/test_pv_lock_cpu.py */
void ref_pv_peaks(const float* P, unsigned char* peak) { peaks(P, NAE_FFT_BINS, peak); }
void ref_pv_regions(const float* P, int* sigma) { regions(P, NAE_FFT_BINS, sigma); }

/* formant preservation, steps 1-5: G[0..M] of one frame's analysis spectrum X, lifter q, transposer ratio g */
static void formant_gain(const tables* t, const cf* X, int q, float g, float* G)
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

/* one channel of the vocoder stage; v[0..Mlen) is overwritten unless v is NULL.  q > 0: formant preservation with ratio g.  qs_tap: every
 * frame's synthesis phase at qs_tap + f * tap_stride */
static void pv_channel(const tables* t, const float* src, size_t L, int ch, int c, const orc_stretch_plan* pl, size_t Mlen, float* v, int lock,
                       int q, float g, int32_t* qs_tap, size_t tap_stride)
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
    if (v) memset(v, 0, Mlen * sizeof(float));
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
        if (qs_tap) memcpy(qs_tap + f * tap_stride, qs, sizeof(uint32_t) * BINS);
        if (!v) continue;
        if (q > 0) formant_gain(t, X, q, g, G);
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
    if (v)
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
int ref_pv_stretch(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, float* dst)
{
    orc_stretch_plan pl;
    const int rc = ref_pv_plan(rate, pitch, N, L, &pl);
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
            pv_channel(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, w, lock, q, g, NULL, 0);
            for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = w[m];
        } else if (pl.pv_on) {
            pv_channel(&t, src, L, ch, c, &pl, pl.mid_len, v, lock, q, g, NULL, 0);
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

/* synthesis phase of every frame, [frames][ch][N/2 + 1] (the lifter does not touch it); with the transposer first its input is the transposed
 * signal */
int ref_pv_synth_phase(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int32_t* qs)
{
    orc_stretch_plan pl;
    const int rc = ref_pv_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (!pl.pv_on) return -1;
    const size_t bins = (size_t)N / 2 + 1;
    tables t;
    tables_make(&t, N);
    float* v = pl.rs_first ? (float*)malloc((pl.mid_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        int32_t* tap = qs + (size_t)c * bins;
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, orc_rs_table(pl.rate_eff), v, 1, 0);
            pv_channel(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, NULL, lock, 0, 0.0f, tap, (size_t)ch * bins);
        } else
            pv_channel(&t, src, L, ch, c, &pl, pl.mid_len, NULL, lock, 0, 0.0f, tap, (size_t)ch * bins);
    }
    free(v);
    tables_free(&t);
    return 0;
}
