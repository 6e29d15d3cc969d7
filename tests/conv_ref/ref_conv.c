/* ref_conv.c — the CPU statement of the long convolution ("K10 long convolution"): uniformly partitioned overlap-save on the
 * canonical FFT of every size (tests/ref_fft.h), written from the specification text.  Compile with -ffp-contract=off.
 *
 *   taps h[0 .. L-1], frame size N = 512, 1024, 2048 or 4096, M = B = N / 2, P = ceil(L / B) partitions, 1 <= L <= 262144, P <= 512
 *   1  H_p = r2c_N(h[p B .. p B + B - 1] zero-padded to N), p < P, no window, bins 0 .. M (the last partition zero-padded too)
 *   2  block b = 0 .. ceil(in_len / B) - 1: u_b[n] = x[b B - B + n], n < N, zero outside [0, in_len); U_b = r2c_N(u_b), no window
 *   3  Y_b[k] = sum over p = 0 .. min(b, P - 1), in increasing p, of U_{b-p}[k] H_p[k]: each product .x = U.x H.x - U.y H.y,
 *      .y = U.x H.y + U.y H.x; the accumulator starts as the p = 0 product and grows by one add per component and term
 *   4  v = c2r_N(Y_b) (the FIR filter's: ref_fir.c)
 *   5  y[b B + n] = v[B + n], n < B, wherever b B + n < in_len
 * and the float64 restatement of the reverb design (include/nae_gpu.h, nae_conv_design_reverb), not rounded.
 */
#include "../fir_ref/ref_fir.c"
#include <math.h>
#include <stdint.h>

#define CONV_MAX_TAPS 262144
#define CONV_MAX_PARTS 512

int ref_conv_pick_n_fft(int n_taps)
{
    if (n_taps < 1 || n_taps > CONV_MAX_TAPS) return 0;
    for (int n = 512; n <= 4096; n *= 2)
        if ((n_taps + n / 2 - 1) / (n / 2) <= 16) return n;
    return (n_taps + 2047) / 2048 <= CONV_MAX_PARTS ? 4096 : 0;
}

/* one channel: x[i * stride], i < in_len, to y[i * stride]; 0, or -1 for parameters outside the specification */
int ref_conv_run(const float* h, int L, int N, const float* x, size_t in_len, size_t stride, float* y)
{
    if (!size_ok(N) || L < 1 || L > CONV_MAX_TAPS) return -1;
    const int M = N / 2, B = N / 2, P = (L + B - 1) / B;
    if (P > CONV_MAX_PARTS) return -1;
    tables t;
    tables_make(&t, N);
    const size_t blocks = (in_len + B - 1) / B, bins = (size_t)M + 1;
    float* u = (float*)malloc(sizeof(float) * N);
    float* v = (float*)malloc(sizeof(float) * N);
    cf* H = (cf*)malloc(sizeof(cf) * bins * P);
    cf* U = (cf*)malloc(sizeof(cf) * bins * (blocks ? blocks : 1));
    cf* Y = (cf*)malloc(sizeof(cf) * bins);
    for (int p = 0; p < P; p++) {
        memset(u, 0, sizeof(float) * N);
        const int n = L - p * B < B ? L - p * B : B;
        memcpy(u, h + (size_t)p * B, sizeof(float) * n);
        rfft(&t, u, H + bins * p);
    }
    for (size_t b = 0; b < blocks; b++) {
        for (int n = 0; n < N; n++) {
            const long long i = (long long)(b * B) - B + n;
            u[n] = (i >= 0 && i < (long long)in_len) ? x[(size_t)i * stride] : 0.0f;
        }
        rfft(&t, u, U + bins * b);
        const int last = b < (size_t)(P - 1) ? (int)b : P - 1;
        for (int k = 0; k <= M; k++) {
            cf acc = {0.0f, 0.0f};
            for (int p = 0; p <= last; p++) {
                const cf a = U[bins * (b - p) + k], w = H[bins * p + k];
                const cf term = {a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x};
                if (p == 0) acc = term;
                else {
                    acc.x = acc.x + term.x;
                    acc.y = acc.y + term.y;
                }
            }
            Y[k] = acc;
        }
        c2r(&t, Y, v);
        for (int n = 0; n < B; n++)
            if (b * B + n < in_len) y[(b * B + n) * stride] = v[B + n];
    }
    free(u); free(v); free(H); free(U); free(Y);
    tables_free(&t);
    return 0;
}

/* the reverb design in double: d = round(predelay sr) silent taps, noise from splitmix64's output function under exp(-ln(1000) (n - d) / (rt60 sr)),
 * scaled to unit energy (summed in increasing n), h = wet r + dry delta */
int ref_conv_reverb_taps(int sample_rate, double rt60_s, double predelay_s)
{
    return (int)(round(predelay_s * (double)sample_rate) + ceil(rt60_s * (double)sample_rate));
}

void ref_conv_design_reverb(int sample_rate, double rt60_s, double predelay_s, double dry, double wet, uint64_t seed, int n_taps, double* h)
{
    const long long d = (long long)round(predelay_s * (double)sample_rate);
    double sum = 0.0;
    for (long long n = 0; n < n_taps; n++) {
        uint64_t z = seed + (uint64_t)(n + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const double g = 2.0 * ((double)(z >> 11) * 0x1p-53) - 1.0;
        h[n] = n >= d ? g * exp(-log(1000.0) * (double)(n - d) / (rt60_s * (double)sample_rate)) : 0.0;
        sum += h[n] * h[n];
    }
    const double norm = sqrt(sum);
    for (long long n = 0; n < n_taps; n++) h[n] = wet * (h[n] / norm) + (n == 0 ? dry : 0.0);
}
