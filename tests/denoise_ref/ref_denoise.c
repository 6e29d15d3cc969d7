/* ref_denoise.c — the CPU statement of the spectral gate ("K13 spectral gate") on the canonical FFT of every size
 * (tests/ref_fft.h), written from the specification text: a whole signal, frame after frame, no tiling.  Compile with -ffp-contract=off.
 *
 *   N = 512, 1024, 2048 or 4096, H = N / 4, M = N / 2; x is zero outside [0, L); B = ceil(L / H) blocks; frames f = 0 .. B + 2, frame f
 *   starts at sample (f - 3) H
 *   1  X_f = r2c_N(hann x_f), bins 0 .. M;  p_f[k] = X.x X.x + X.y X.y
 *   2  d_f[k] = p_f[k] > profile[k] thr_scale (one f32 product); d_f = 0 for f outside [0, B + 2]
 *   3  v_f[k] = sum_{|j| <= Tn} (Tn + 1 - |j|) d_{f+j}[k];  c_f[k] = sum_{|i| <= Fn} (Fn + 1 - |i|) v_f[mir(k + i)], mir(k) = |k| for k <= M and
 *      2 M - k above;  C = (Tn + 1)^2 (Fn + 1)^2
 *   4  G = 1 if c = C, else floor_gain + span ((float)c inv_c), span = (float)(1 - floor_gain), inv_c = (float)(1 / C), both from double
 *   5  Y = {G X.x, G X.y};  y_f = hann c2r_N(Y);  block b = ((y_b[3 H ..] + y_{b+1}[2 H ..]) + y_{b+2}[H ..]) + y_{b+3}[0 ..], times NAE_OLA_GAIN
 */
#include "../ref_fft.h"
#include "../../include/nae_dsp_spec.h"
#include <stddef.h>
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

/* one channel: x[i * stride], i < L, to y[i * stride].  d_out (or null) receives the decisions [B + 3][M + 1] as bytes, c_out (or null) the
 * counts [B + 3][M + 1].  d_in (or null): decisions to use instead of the statement's own (the restatement's output check).  0, or -1 for
 * parameters outside the specification */
int ref_denoise_run(int N, int Tn, int Fn, float thr_scale, float floor_gain, const float* profile, const float* x, size_t L, size_t stride, float* y,
                    unsigned char* d_out, int* c_out, const unsigned char* d_in)
{
    if (!size_ok(N) || Tn < 0 || Tn > NAE_DENOISE_MAX_TIME || Fn < 0 || Fn > NAE_DENOISE_MAX_FREQ) return -1;
    if (L == 0) return 0;
    const int H = N / 4, M = N / 2, K = M + 1;
    const long long B = (long long)((L + H - 1) / H), F = B + 3;
    tables t;
    tables_make(&t, N);
    float* xw = (float*)malloc(sizeof(float) * N);
    float* v = (float*)malloc(sizeof(float) * N);
    cf* X = (cf*)malloc(sizeof(cf) * (size_t)F * K);
    unsigned char* d = (unsigned char*)malloc((size_t)F * K);
    int* vt = (int*)malloc(sizeof(int) * K);
    float* yw = (float*)malloc(sizeof(float) * (size_t)F * N);
    /* 1, 2 */
    for (long long f = 0; f < F; f++) {
        analyse(&t, x, L, stride, (f - 3) * H, xw, X + f * K);
        for (int k = 0; k < K; k++) {
            const cf a = X[f * K + k];
            const float p = a.x * a.x + a.y * a.y;
            d[f * K + k] = d_in ? d_in[f * K + k] : (p > profile[k] * thr_scale ? 1 : 0);
        }
    }
    if (d_out) memcpy(d_out, d, (size_t)F * K);
    /* 3, 4, 5 */
    const int C = (Tn + 1) * (Tn + 1) * (Fn + 1) * (Fn + 1);
    const float span = (float)(1.0 - (double)floor_gain), inv_c = (float)(1.0 / (double)C);
    cf* Y = (cf*)malloc(sizeof(cf) * K);
    for (long long f = 0; f < F; f++) {
        for (int k = 0; k < K; k++) {
            int s = 0;
            for (int j = -Tn; j <= Tn; j++)
                if (f + j >= 0 && f + j < F) s += (Tn + 1 - abs(j)) * d[(f + j) * K + k];
            vt[k] = s;
        }
        for (int k = 0; k < K; k++) {
            int c = 0;
            for (int i = -Fn; i <= Fn; i++) c += (Fn + 1 - abs(i)) * vt[mir(k + i, M)];
            if (c_out) c_out[f * K + k] = c;
            const float G = c == C ? 1.0f : floor_gain + span * ((float)c * inv_c);
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
    free(xw); free(v); free(X); free(d); free(vt); free(yw); free(Y);
    tables_free(&t);
    return 0;
}

/* the noise profile of one channel's excerpt x[i * stride], i < len: frames at 0, H, 2 H, ... while start + N <= len (n of them; n = 0: -1);
 * profile[k] = (float)(sum_f (double)p_f[k] / (double)n), summed in frame order */
int ref_denoise_profile(int N, const float* x, size_t len, size_t stride, float* profile)
{
    if (!size_ok(N) || len < (size_t)N) return -1;
    const int H = N / 4, M = N / 2, K = M + 1;
    const size_t n = (len - N) / H + 1;
    tables t;
    tables_make(&t, N);
    float* xw = (float*)malloc(sizeof(float) * N);
    cf* X = (cf*)malloc(sizeof(cf) * K);
    double* acc = (double*)calloc(K, sizeof(double));
    for (size_t f = 0; f < n; f++) {
        analyse(&t, x, len, stride, (long long)(f * H), xw, X);
        for (int k = 0; k < K; k++) acc[k] += (double)(X[k].x * X[k].x + X[k].y * X[k].y);
    }
    for (int k = 0; k < K; k++) profile[k] = (float)(acc[k] / (double)n);
    free(xw); free(X); free(acc);
    tables_free(&t);
    return 0;
}

/* nae_denoise_design's formulas */
int ref_denoise_design(double reduction_db, double sensitivity_db, float* thr_scale, float* floor_gain)
{
    *thr_scale = (float)pow(10.0, sensitivity_db / 10.0);
    *floor_gain = (float)pow(10.0, -reduction_db / 20.0);
    return 0;
}
