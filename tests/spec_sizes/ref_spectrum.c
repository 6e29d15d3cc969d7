/* ref_spectrum.c — CPU restatement of the K8 spectrum at every size ("K8 spectrum, every size").
 * Test code: the GPU kernels must equal it bit for bit.  The canonical FFT is tests/ref_fft.h's; the magnitude of each bin of its r2c output.
 * Compile with -ffp-contract=off (fused multiply-adds appear only where fmaf() is written). */
#include "../ref_fft.h"
#include <stddef.h>

static int size_ok(int n) { return n >= 256 && n <= 4096 && (n & (n - 1)) == 0; }

size_t ref_frames(size_t T, int n_fft, int hop)
{
    if (!size_ok(n_fft) || hop < 1 || hop > n_fft) return 0;
    return T < (size_t)n_fft ? 0 : (T - (size_t)n_fft) / (size_t)hop + 1;
}

/* src: interleaved [T][ch]; dst: [frame][ch][n_fft/2 + 1] */
int ref_spectrum_f32(const float* src, size_t T, int ch, int n_fft, int hop, float* dst)
{
    if (!size_ok(n_fft) || hop < 1 || hop > n_fft || ch < 1 || ch > 2) return -1;
    const int M = n_fft / 2;
    tables t;
    tables_make(&t, n_fft);
    float* xw = (float*)malloc(sizeof(float) * n_fft);
    cf* X = (cf*)malloc(sizeof(cf) * (M + 1));
    const size_t F = ref_frames(T, n_fft, hop);
    for (size_t f = 0; f < F; f++)
        for (int c = 0; c < ch; c++) {
            const float* s = src + f * (size_t)hop * ch + c;
            for (int n = 0; n < n_fft; n++) xw[n] = s[(size_t)n * ch] * t.hann[n];
            rfft(&t, xw, X);
            float* o = dst + (f * ch + c) * (size_t)(M + 1);
            for (int k = 0; k <= M; k++) o[k] = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
        }
    free(xw); free(X);
    tables_free(&t);
    return 0;
}
