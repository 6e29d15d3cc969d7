/* ref_fir.c — the CPU statement of the FIR filter ("K9 FIR filter"): overlap-save on the canonical FFT of every size
 * (tests/ref_fft.h), written from the specification text.  Compile with -ffp-contract=off.
 *
 *   taps h[0 .. L-1], frame size N = 512, 1024, 2048 or 4096, M = B = N / 2, 1 <= L <= B + 1
 *   1  H = r2c_N(h zero-padded to N), no window, bins 0 .. M
 *   2  block b = 0 .. ceil(in_len / B) - 1: u[n] = x[b B - B + n], n < N, zero outside [0, in_len); U = r2c_N(u), no window
 *   3  Y[k].x = U.x H.x - U.y H.y, Y[k].y = U.x H.y + U.y H.x (four products, one subtract, one add)
 *   4  v = c2r_N(Y): split with T_N, conjugate, forward FFT_M, scale by 1 / M; the imaginary parts of bins 0 and M are dropped
 *   5  y[b B + n] = v[B + n], n < B, wherever b B + n < in_len
 */
#include "../ref_fft.h"
#include <stddef.h>
#include <string.h>

static int size_ok(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

/* c2r: Zc[k] = conj(E + i conj(T_N[k]) D) with E, D the even and odd parts of (Y[k], conj Y[M - k]); z = FFT_M(Zc);
 * v[2m] = Re z[m] / M, v[2m + 1] = -Im z[m] / M */
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

int ref_fir_pick_n_fft(int n_taps)
{
    if (n_taps < 1) return 0;
    for (int n = 512; n <= 4096; n *= 2)
        if (n / 2 + 1 >= n_taps) return n;
    return 0;
}

/* one channel: x[i * stride], i < in_len, to y[i * stride]; 0, or -1 for parameters outside the specification */
int ref_fir_run(const float* h, int L, int N, const float* x, size_t in_len, size_t stride, float* y)
{
    if (!size_ok(N) || L < 1 || L > N / 2 + 1) return -1;
    const int M = N / 2, B = N / 2;
    tables t;
    tables_make(&t, N);
    float* u = (float*)malloc(sizeof(float) * N);
    float* v = (float*)malloc(sizeof(float) * N);
    cf* H = (cf*)malloc(sizeof(cf) * (M + 1));
    cf* U = (cf*)malloc(sizeof(cf) * (M + 1));
    cf* Y = (cf*)malloc(sizeof(cf) * (M + 1));
    memset(u, 0, sizeof(float) * N);
    memcpy(u, h, sizeof(float) * L);
    rfft(&t, u, H);
    const size_t blocks = (in_len + B - 1) / B;
    for (size_t b = 0; b < blocks; b++) {
        for (int n = 0; n < N; n++) {
            const long long i = (long long)(b * B) - B + n;
            u[n] = (i >= 0 && i < (long long)in_len) ? x[(size_t)i * stride] : 0.0f;
        }
        rfft(&t, u, U);
        for (int k = 0; k <= M; k++) {
            Y[k].x = U[k].x * H[k].x - U[k].y * H[k].y;
            Y[k].y = U[k].x * H[k].y + U[k].y * H[k].x;
        }
        c2r(&t, Y, v);
        for (int n = 0; n < B; n++)
            if (b * B + n < in_len) y[(b * B + n) * stride] = v[B + n];
    }
    free(u); free(v); free(H); free(U); free(Y);
    tables_free(&t);
    return 0;
}
