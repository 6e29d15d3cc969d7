/* ref_sat.c — the CPU statement of the saturation ("K18 saturation"): the plain sequential form of the specification in
 * include/nae_gpu.h, every step one IEEE f32 operation in the order written there.  Built by tests/cstatement.py (-ffp-contract=off: fmaf is
 * the only fused operation).  The whole oversampled signals u and v are formed first and filtered afterwards: nothing is tiled, staged or
 * shared with the library. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define K 16           /* NAE_SAT_HALF */
#define MAX_OS 8       /* NAE_SAT_MAX_OS */
#define SOFT 0
#define HARD 1
#define BETA 8.0       /* NAE_FIR_KAISER_BETA */

typedef struct ref_sat_params { int oversample; int curve; float drive; float bias; float wet; float dry; } ref_sat_params;

static int os_ok(int m) { return m == 1 || m == 2 || m == 4 || m == 8; }

int ref_sat_latency(int m) { return m == 1 ? 0 : (os_ok(m) ? 2 * K : -1); }

/* the modified Bessel function I0 by its power series, as the library's Kaiser windows use it */
static double bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 64; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

/* hd: the Kaiser-windowed sinc low-pass of 2 K M + 1 taps at cutoff c = 1 / M (nae_fir_design(0, 2 M, -, 1.0, 2 K M + 1)), in double, normalised
 * to unit sum, rounded once; returns the count, 0 for M = 1 */
int ref_sat_taps(int m, float* hd)
{
    if (!hd || !os_ok(m) || m == 1) return 0;
    const int L = 2 * K * m + 1;
    const double pi = 3.14159265358979323846;
    const double c = 2.0 * 1.0 / (double)(2 * m), half = 0.5 * (double)(L - 1), i0b = bessel_i0(BETA);
    double h[2 * K * MAX_OS + 1], sum = 0.0;
    for (int n = 0; n < L; n++) {
        const double t = (double)n - half;
        const double a = t / half;
        const double r = 1.0 - a * a;
        const double w = bessel_i0(BETA * sqrt(r > 0.0 ? r : 0.0)) / i0b;
        const double arg = pi * c * t;
        const double sinc = arg == 0.0 ? 1.0 : sin(arg) / arg;
        h[n] = c * sinc * w;
        sum += h[n];
    }
    for (int n = 0; n < L; n++) hd[n] = (float)(h[n] / sum);
    return L;
}

int ref_sat_check(const ref_sat_params* p, int ch)
{
    if (!p) return -1;
    if (ch != 1 && ch != 2) return -1;
    if (!isfinite(p->drive) || !isfinite(p->bias) || !isfinite(p->wet) || !isfinite(p->dry)) return -1;
    if (p->curve != SOFT && p->curve != HARD) return -1;
    if (!os_ok(p->oversample)) return -2;
    return 0;
}

int ref_sat_design(double drive_db, double bias, int curve, int oversample, double output_db, double mix, ref_sat_params* out)
{
    if (!out) return -1;
    if (!isfinite(drive_db) || !isfinite(bias) || !isfinite(output_db) || !isfinite(mix)) return -1;
    if (drive_db < 0.0 || drive_db > 48.0 || bias < 0.0 || bias > 1.0 || output_db < -24.0 || output_db > 24.0 || mix < 0.0 || mix > 1.0) return -1;
    if (curve != SOFT && curve != HARD) return -1;
    if (!os_ok(oversample)) return -2;
    memset(out, 0, sizeof(*out));
    out->oversample = oversample;
    out->curve = curve;
    out->drive = (float)pow(10.0, drive_db / 20.0);
    out->bias = (float)bias;
    out->wet = (float)(mix * pow(10.0, output_db / 20.0));
    out->dry = (float)(1.0 - mix);
    return 0;
}

float ref_sat_curve(int curve, float t)
{
    if (curve == SOFT) {
        const float c = t > 3.0f ? 3.0f : (t < -3.0f ? -3.0f : t);
        const float q = c * c;
        return (c * (27.0f + q)) / (27.0f + (9.0f * q));
    }
    return t > 1.0f ? 1.0f : (t < -1.0f ? -1.0f : t);
}

/* one channel: x[i * ch] -> y[i * ch], i = 0 ... n - 1 */
static int run_channel(const ref_sat_params* p, const float* x, size_t n, int ch, float* y)
{
    const int M = p->oversample;
    const float g = p->drive, b = p->bias, wet = p->wet, dry = p->dry;
    const float fb = ref_sat_curve(p->curve, b);
    if (M == 1) {
        for (size_t i = 0; i < n; i++) y[i * ch] = (dry * x[i * ch]) + (wet * (ref_sat_curve(p->curve, fmaf(g, x[i * ch], b)) - fb));
        return 0;
    }
    float hd[2 * K * MAX_OS + 1], hu[2 * K * MAX_OS + 1];
    const int L = ref_sat_taps(M, hd);
    for (int j = 0; j < L; j++) hu[j] = (float)M * hd[j];
    float* v = (float*)malloc(n * (size_t)M * sizeof(float));
    if (!v) return -4;
#define X(i) ((i) < 0 ? 0.0f : x[(size_t)(i) * ch])
    for (long long i = 0; i < (long long)n; i++)
        for (int ph = 0; ph < M; ph++) {
            float a = hu[ph] * X(i);
            for (int k = 1; ph + k * M <= 2 * K * M; k++) a = fmaf(hu[ph + k * M], X(i - k), a);
            const float t = fmaf(g, a, b);
            v[i * M + ph] = ref_sat_curve(p->curve, t) - fb;
        }
#define V(m) ((m) < 0 ? 0.0f : v[m])
    for (long long i = 0; i < (long long)n; i++) {
        float s = hd[0] * V(i * M);
        for (int j = 1; j <= 2 * K * M; j++) s = fmaf(hd[j], V(i * M - j), s);
        y[(size_t)i * ch] = (dry * X(i - 2 * K)) + (wet * s);
    }
#undef X
#undef V
    free(v);
    return 0;
}

/* x[n][ch] interleaved -> y[n][ch] */
int ref_sat_run(const ref_sat_params* p, const float* x, size_t n, int ch, float* y)
{
    const int rc = ref_sat_check(p, ch);
    if (rc) return rc;
    for (int c = 0; c < ch; c++) {
        const int r = run_channel(p, x + c, n, ch, y + c);
        if (r) return r;
    }
    return 0;
}
