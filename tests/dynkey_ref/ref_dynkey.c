/* ref_dynkey.c — the CPU statement of K15, the keyed dynamics ("K15 keyed dynamics"): K12 whose detector reads a key.  The key
 * path is K11's statement (ref_eq_run_f64 of ../eq_ref/ref_eq.c), the detector K12's (run() of ../dyn_ref/ref_dyn.c on the f32 magnitudes),
 * the gain ref_dyn_exp2 on the signal.  The tiled form is what the GPU computes, bit for bit (ref_dynkey_run); the sequential form runs the
 * plain recurrences in both (ref_dynkey_sequential); ref_dynkey_magnitude exports m.
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written in the two statements included here.
 * With -DREF_DYNKEY_MAIN the file is a program that runs every form once on a small case (for a sanitizer build). */
#include "../eq_ref/ref_eq.c"
#include "../dyn_ref/ref_dyn.c"

#define DYNKEY_MAX_SECTIONS 4 /* NAE_DYNKEY_MAX_SECTIONS */

typedef struct ref_dynkey_params {   /* nae_dynkey_params of include/nae_gpu.h */
    ref_dyn_params dyn;
    int key_ch, n_sections;
    double coef[DYNKEY_MAX_SECTIONS][5];
} ref_dynkey_params;

/* 0 when the parameters are acceptable for `ch` channels, -1 invalid, -2 unsupported (the look-ahead, or more than four sections) */
int ref_dynkey_check(const ref_dynkey_params* p, int ch)
{
    if (!p || (ch != 1 && ch != 2)) return -1;
    const int rc = ref_dyn_check(&p->dyn);
    if (rc) return rc;
    if (p->key_ch != 0 && p->key_ch != 1 && p->key_ch != ch) return -1;
    if (p->n_sections < 0) return -1;
    if (p->n_sections > DYNKEY_MAX_SECTIONS) return -2;
    return p->n_sections ? ref_eq_check(&p->coef[0][0], p->n_sections) : 0;
}

/* step 2 of K15: m[in_len][kc] = (float)|w|, w the key's channel through the sections (tiled: K11's tiled form, else the plain recurrence) */
static int magnitude(const ref_dynkey_params* p, const float* key, size_t in_len, int kc, int tiled, float* m)
{
    float* xc = (float*)malloc(in_len * sizeof(float));
    double* w = (double*)malloc(in_len * sizeof(double));
    int rc = xc && w ? 0 : -3;
    for (int c = 0; c < kc && !rc; c++) {
        for (size_t n = 0; n < in_len; n++) xc[n] = key[n * kc + c];
        if (p->n_sections == 0)
            for (size_t n = 0; n < in_len; n++) w[n] = (double)xc[n];
        else
            rc = tiled ? ref_eq_run_f64(&p->coef[0][0], p->n_sections, xc, in_len, 1, w) : ref_eq_sequential(&p->coef[0][0], p->n_sections, xc, in_len, 1, w);
        for (size_t n = 0; n < in_len && !rc; n++) m[n * kc + c] = (float)fabs(w[n]);
    }
    free(xc);
    free(w);
    return rc;
}

/* x: interleaved [in_len][ch]; key: interleaved [in_len][key_ch], or null with key_ch = 0 (the signal is its own key).  The detectors are
 * K12's on m: linked, one on the larger m of the key's channels; unlinked, detector c on key channel c, or on channel 0 of a mono key.
 * y (f32, rounded once), yd (the same in double, not rounded) and m_out ([in_len][key channels]) are each optional. */
static int keyed(const ref_dynkey_params* p, const float* x, const float* key, size_t in_len, int ch, int tiled, float* y, double* yd, float* m_out)
{
    if (ref_dynkey_check(p, ch) || (in_len && !x) || (p->key_ch == 0) != (key == NULL)) return -1;
    if (in_len == 0) return 0;
    const int kc = p->key_ch ? p->key_ch : ch;
    const int n_det = p->dyn.link && kc == 2 ? 1 : kc;         /* the detectors run() makes of m */
    float* m = (float*)malloc(in_len * kc * sizeof(float));
    double* yl = (double*)malloc(in_len * n_det * sizeof(double));
    int rc = m && yl ? 0 : -3;
    if (!rc) rc = magnitude(p, p->key_ch ? key : x, in_len, kc, tiled, m);
    /* the demand is zero from in_len on: run() reads zeros there, as K12's statement does of its own signal */
    if (!rc) rc = run(&p->dyn, m, in_len, kc, tiled, NULL, NULL, yl);
    for (size_t n = 0; n < in_len && !rc; n++)
        for (int c = 0; c < ch; c++) {
            const double g = ref_dyn_exp2((p->dyn.makeup_db - yl[n * n_det + (n_det == 1 ? 0 : c)]) * KINV);
            const double v = (double)x[n * ch + c] * g;
            if (y) y[n * ch + c] = (float)v;
            if (yd) yd[n * ch + c] = v;
        }
    if (!rc && m_out) memcpy(m_out, m, in_len * kc * sizeof(float));
    free(m);
    free(yl);
    return rc;
}

/* the tiled statement: what the GPU computes, bit for bit */
int ref_dynkey_run(const ref_dynkey_params* p, const float* x, const float* key, size_t in_len, int ch, float* y)
{
    return y ? keyed(p, x, key, in_len, ch, 1, y, NULL, NULL) : -1;
}

/* the tiled statement in front of its final rounding */
int ref_dynkey_run_f64(const ref_dynkey_params* p, const float* x, const float* key, size_t in_len, int ch, double* yd)
{
    return yd ? keyed(p, x, key, in_len, ch, 1, NULL, yd, NULL) : -1;
}

/* the plain sequential recurrences in the key filter and in the detector, not rounded */
int ref_dynkey_sequential(const ref_dynkey_params* p, const float* x, const float* key, size_t in_len, int ch, double* yd)
{
    return yd ? keyed(p, x, key, in_len, ch, 0, NULL, yd, NULL) : -1;
}

/* m of the tiled statement, [in_len][key_ch, or ch with key_ch = 0] */
int ref_dynkey_magnitude(const ref_dynkey_params* p, const float* x, const float* key, size_t in_len, int ch, float* m)
{
    if (!m) return -1;
    double* yd = (double*)malloc((in_len ? in_len : 1) * ch * sizeof(double));
    const int rc = yd ? keyed(p, x, key, in_len, ch, 1, NULL, yd, m) : -3;
    free(yd);
    return rc;
}

#ifdef REF_DYNKEY_MAIN
#include <stdio.h>
int main(void)
{
    enum { N = 3 * C + 7 };
    static float x[N * 2], key[N * 2], y[N * 2], m[N * 2];
    static double yd[N * 2];
    unsigned s = 1u;
    for (int i = 0; i < N * 2; i++) {
        s = s * 1664525u + 1013904223u;
        x[i] = (float)(s >> 8) / 8388608.0f - 1.0f;
        s = s * 1664525u + 1013904223u;
        key[i] = ((i / 2) % 700 < 90 ? 0.9f : 0.003f) * ((float)(s >> 8) / 8388608.0f - 1.0f);
    }
    ref_dynkey_params p = {{-30.0, 0.75, 6.0, 0.9, 0.999, 3.0, 17, 1}, 2, 0, {{0}}};
    int bad = 0;
    for (int sections = 0; sections <= DYNKEY_MAX_SECTIONS; sections += 2)
        for (int key_ch = 0; key_ch <= 2; key_ch++)
            for (int ch = 1; ch <= 2; ch++)
                for (int link = 0; link <= 1; link++) {
                    if (key_ch > ch) continue;
                    p.key_ch = key_ch;
                    p.n_sections = sections;
                    p.dyn.link = link;
                    for (int i = 0; i < sections; i++)
                        if (ref_eq_design(i & 1 ? 4 : 0, 48000, 200.0 * (i + 1), 6.0, 0.7, p.coef[i])) bad++;
                    const float* k = key_ch ? key : NULL;
                    bad += ref_dynkey_run(&p, x, k, N, ch, y) != 0;
                    bad += ref_dynkey_run_f64(&p, x, k, N, ch, yd) != 0;
                    bad += ref_dynkey_sequential(&p, x, k, N, ch, yd) != 0;
                    bad += ref_dynkey_magnitude(&p, x, k, N, ch, m) != 0;
                    bad += ref_dynkey_run(&p, x, k, 1, ch, y) != 0;
                }
    printf("ref_dynkey: %d failures\n", bad);
    return bad != 0;
}
#endif
