/* ref_hpss.c — the CPU statement of the harmonic/percussive separation ("K21 separation") on the canonical FFT of every size
 * (tests/ref_fft.h), written from the specification text: a whole signal, frame after frame, no tiling, the medians by sorting.  Compile
 * with -ffp-contract=off.
 *
 *   N = 512, 1024, 2048 or 4096, H = N / 4, M = N / 2; x is zero outside [0, L); B = ceil(L / H) blocks; frames f = 0 .. B + 2, frame f
 *   starts at sample (f - 3) H
 *   1  X_f = r2c_N(hann x_f), bins 0 .. M;  p_f[k] = X.x X.x + X.y X.y
 *   2  q_f[k] = (uint16)(bits(p_f[k]) >> 16); q_f = 0 for f outside [0, B + 2]; value(q) = the float with the bits q << 16
 *   3  Hq_f[k] = median_{|j| <= Tn} q_{f+j}[k];  Pq_f[k] = median_{|i| <= Fn} q_f[mir(k + i)], mir(k) = |k| for k <= M and 2 M - k above; the
 *      median of an odd count is the element of rank (count - 1) / 2
 *   4  hard: m = 1 if Hq >= Pq else 0;  soft: h = value(Hq), p = value(Pq), s = (double)h + (double)p, m = 0.5 if s == 0 else (float)((double)h / s)
 *   5  G = g_p + d m, d = (float)((double)g_h - (double)g_p);  Y = {G X.x, G X.y};  y_f = hann c2r_N(Y);
 *      block b = ((y_b[3 H ..] + y_{b+1}[2 H ..]) + y_{b+2}[H ..]) + y_{b+3}[0 ..], times NAE_OLA_GAIN
 */
#include "../ref_fft.h"
#include "../../include/nae_dsp_spec.h"
#include <stddef.h>
#include <stdint.h>
#include <string.h>

static int size_ok(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

/* c2r of the vocoder's synthesis: Zc[k] = conj(E + i conj(T_N[k]) D), z = FFT_M(Zc), v[2m] = Re z[m] / M, v[2m + 1] = -Im z[m] / M */
static void c2r(const tables* t, const cf* Y, float* v)
{
    const int M = t->M;
    cf* Zc = (cf*)malloc(sizeof(cf) * M);
    cf* z = (cf*)malloc(sizeof(cf) * M);
    for (int k = 0; k < M; k++) {
        cf a = Y[k], b = Y[M - k];
        if (k == 0) { a.y = 0.0f; b.y = 0.0f; }
        const cf E = {0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
        const cf D = {0.5f * (a.x - b.x), 0.5f * (a.y + b.y)};
        const cf T = t->TN[k];
        const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};
        Zc[k].x = E.x - Q.y;
        Zc[k].y = -(E.y + Q.x);
    }
    fft_dif(Zc, M, M, t->R1, t->WM, z);
    const float scale = 1.0f / (float)M;
    for (int m = 0; m < M; m++) {
        v[2 * m] = z[m].x * scale;
        v[2 * m + 1] = -z[m].y * scale;
    }
    free(Zc);
    free(z);
}

/* the windowed spectrum of the N samples from `start` on (zero outside [0, len)) */
static void analyse(const tables* t, const float* x, size_t len, size_t stride, long long start, float* xw, cf* X)
{
    for (int n = 0; n < t->N; n++) {
        const long long i = start + n;
        const float s = (i >= 0 && i < (long long)len) ? x[(size_t)i * stride] : 0.0f;
        xw[n] = s * t->hann[n];
    }
    rfft(t, xw, X);
}

static int mir(int k, int M) { return k < 0 ? -k : (k > M ? 2 * M - k : k); }

static uint16_t key_of(float p)
{
    uint32_t u;
    memcpy(&u, &p, sizeof u);
    return (uint16_t)(u >> 16);
}

static float value_of(uint16_t q)
{
    const uint32_t u = (uint32_t)q << 16;
    float v;
    memcpy(&v, &u, sizeof v);
    return v;
}

/* the element of rank (n - 1) / 2 of v[0 .. n), n odd and at most 17: insertion sort */
static uint16_t median(uint16_t* v, int n)
{
    for (int i = 1; i < n; i++) {
        const uint16_t e = v[i];
        int j = i;
        while (j > 0 && v[j - 1] > e) { v[j] = v[j - 1]; j--; }
        v[j] = e;
    }
    return v[(n - 1) / 2];
}

/* one channel: x[i * stride], i < L, to y[i * stride].  q_out, hq_out, pq_out (or null) receive the keys and the two medians [B + 3][M + 1],
 * m_out (or null) the mask [B + 3][M + 1].  0, or -1 for parameters outside the specification */
int ref_hpss_run(int N, int Tn, int Fn, int hard, float gain_h, float gain_p, const float* x, size_t L, size_t stride, float* y, uint16_t* q_out,
                 uint16_t* hq_out, uint16_t* pq_out, float* m_out)
{
    if (!size_ok(N) || Tn < 0 || Tn > NAE_HPSS_MAX_SPAN || Fn < 0 || Fn > NAE_HPSS_MAX_SPAN || (hard != 0 && hard != 1)) return -1;
    if (L == 0) return 0;
    const int H = N / 4, M = N / 2, K = M + 1;
    const long long B = (long long)((L + H - 1) / H), F = B + 3;
    tables t;
    tables_make(&t, N);
    float* xw = (float*)malloc(sizeof(float) * N);
    float* v = (float*)malloc(sizeof(float) * N);
    cf* X = (cf*)malloc(sizeof(cf) * (size_t)F * K);
    uint16_t* q = (uint16_t*)malloc(sizeof(uint16_t) * (size_t)F * K);
    float* yw = (float*)malloc(sizeof(float) * (size_t)F * N);
    /* 1, 2 */
    for (long long f = 0; f < F; f++) {
        analyse(&t, x, L, stride, (f - 3) * H, xw, X + f * K);
        for (int k = 0; k < K; k++) {
            const cf a = X[f * K + k];
            q[f * K + k] = key_of(a.x * a.x + a.y * a.y);
        }
    }
    if (q_out) memcpy(q_out, q, sizeof(uint16_t) * (size_t)F * K);
    /* 3, 4, 5 */
    const float d = (float)((double)gain_h - (double)gain_p);
    cf* Y = (cf*)malloc(sizeof(cf) * K);
    uint16_t w[2 * NAE_HPSS_MAX_SPAN + 1];
    for (long long f = 0; f < F; f++) {
        for (int k = 0; k < K; k++) {
            for (int j = -Tn; j <= Tn; j++) w[j + Tn] = (f + j >= 0 && f + j < F) ? q[(f + j) * K + k] : 0;
            const uint16_t hq = median(w, 2 * Tn + 1);
            for (int i = -Fn; i <= Fn; i++) w[i + Fn] = q[f * K + mir(k + i, M)];
            const uint16_t pq = median(w, 2 * Fn + 1);
            float m;
            if (hard) m = hq >= pq ? 1.0f : 0.0f;
            else {
                const double h = (double)value_of(hq), s = h + (double)value_of(pq);
                m = s == 0.0 ? 0.5f : (float)(h / s);
            }
            if (hq_out) hq_out[f * K + k] = hq;
            if (pq_out) pq_out[f * K + k] = pq;
            if (m_out) m_out[f * K + k] = m;
            const float G = gain_p + d * m;
            Y[k].x = G * X[f * K + k].x;
            Y[k].y = G * X[f * K + k].y;
        }
        c2r(&t, Y, v);
        for (int n = 0; n < N; n++) yw[f * N + n] = t.hann[n] * v[n];
    }
    for (long long b = 0; b < B; b++)
        for (int n = 0; n < H; n++) {
            const size_t i = (size_t)b * H + n;
            if (i >= L) break;
            float acc = yw[b * N + 3 * H + n];
            acc = acc + yw[(b + 1) * N + 2 * H + n];
            acc = acc + yw[(b + 2) * N + H + n];
            y[i * stride] = (acc + yw[(b + 3) * N + n]) * NAE_OLA_GAIN;
        }
    free(xw); free(v); free(X); free(q); free(yw); free(Y);
    tables_free(&t);
    return 0;
}

/* nae_hpss_design's formula for one level */
float ref_hpss_gain(double db) { return db <= NAE_HPSS_MIN_DB ? 0.0f : (float)pow(10.0, db / 20.0); }
