/* ref_mb.c — the CPU statement of K20, the multiband compressor ("K20 multiband"): a crossover tree of K11 sections, K12 on every
 * band, and the bands' sum.  A band's signal is K11's statement on the sections of the band's path (ref_eq_run of ../eq_ref/ref_eq.c: the
 * signal stays double between the sections of a path and is rounded once), a band's compressor K12's (ref_dyn_run of ../dyn_ref/ref_dyn.c),
 * the sum a double addition in band order, rounded once.  This file holds the tree, the parameter rules and the design.  ref_mb_run is what
 * the GPU computes, bit for bit; ref_mb_split_f64 exports the band signals in front of their rounding, tiled or by the plain recurrence.
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written in the two statements included here.
 * With -DREF_MB_MAIN the file is a program that runs every form once on a small case (for a sanitizer build). */
#include "../eq_ref/ref_eq.c"
#include "../dyn_ref/ref_dyn.c"

#define MB_MAX_BANDS 4     /* NAE_MB_MAX_BANDS */
#define MB_MAX_SECTIONS 14 /* NAE_MB_MAX_SECTIONS */
#define MB_MAX_PATH 5

typedef struct ref_mb_params {   /* nae_mb_params of include/nae_gpu.h */
    int n_bands, n_sections;
    double coef[MB_MAX_SECTIONS][5];
    ref_dyn_params band[MB_MAX_BANDS];
    unsigned mute_mask, bypass_mask;
} ref_mb_params;

/* the tree: the slots of band b's path from the input on, ended by -1 ("K20 multiband", the table) */
static const signed char mb_path[3][MB_MAX_BANDS][MB_MAX_PATH + 1] = {
    {{0, 1, -1}, {2, 3, -1}},
    {{0, 1, 2, -1}, {3, 4, 5, 6, -1}, {3, 4, 7, 8, -1}},
    {{0, 1, 2, 3, 4, -1}, {0, 1, 2, 5, 6, -1}, {7, 8, 9, 10, 11, -1}, {7, 8, 9, 12, 13, -1}}};

int ref_mb_sections(int n_bands) { return n_bands == 2 ? 4 : n_bands == 3 ? 9 : n_bands == 4 ? 14 : 0; }

/* the slots of band b's path into slots[MB_MAX_PATH]; returns how many */
int ref_mb_path(int n_bands, int b, int* slots)
{
    if (n_bands < 2 || n_bands > MB_MAX_BANDS || b < 0 || b >= n_bands) return 0;
    int n = 0;
    while (mb_path[n_bands - 2][b][n] >= 0) {
        slots[n] = mb_path[n_bands - 2][b][n];
        n++;
    }
    return n;
}

/* 0 when the parameters are acceptable for `ch` channels, -1 invalid, -2 unsupported (more than four bands, or the look-ahead) */
int ref_mb_check(const ref_mb_params* p, int ch)
{
    if (!p || (ch != 1 && ch != 2)) return -1;
    if (p->n_bands < 2) return -1;
    if (p->n_bands > MB_MAX_BANDS) return -2;
    if (p->n_sections != ref_mb_sections(p->n_bands)) return -1;
    if (ref_eq_check(&p->coef[0][0], p->n_sections)) return -1;
    for (int b = 0; b < p->n_bands; b++) {
        const int rc = ref_dyn_check(&p->band[b]);
        if (rc) return rc;
        if (p->band[b].lookahead != p->band[0].lookahead || p->band[b].link != p->band[0].link) return -1;
    }
    if ((p->mute_mask | p->bypass_mask) >> p->n_bands) return -1;
    return 0;
}

/* the sections of band b's path, in a row */
static int path_coef(const ref_mb_params* p, int b, double* coef)
{
    int slots[MB_MAX_PATH];
    const int n = ref_mb_path(p->n_bands, b, slots);
    for (int i = 0; i < n; i++) memcpy(coef + 5 * i, p->coef[slots[i]], 5 * sizeof(double));
    return n;
}

/* x: interleaved [in_len][ch].  xb (optional): the band signals [n_bands][in_len][ch]; y (optional): the output [in_len][ch] */
static int multiband(const ref_mb_params* p, const float* x, size_t in_len, int ch, float* xb_out, float* y)
{
    if (ref_mb_check(p, ch) || (in_len && !x)) return -1;
    if (in_len == 0) return 0;
    const size_t plane = in_len * (size_t)ch;
    float* xb = (float*)malloc(plane * sizeof(float));
    float* yb = (float*)malloc(plane * sizeof(float));
    double* acc = (double*)malloc(plane * sizeof(double));
    int rc = xb && yb && acc ? 0 : -3;
    int first = 1;
    for (int b = 0; b < p->n_bands && !rc; b++) {
        double coef[MB_MAX_PATH * 5];
        const int n = path_coef(p, b, coef);
        for (int c = 0; c < ch && !rc; c++) rc = ref_eq_run(coef, n, x + c, in_len, (size_t)ch, xb + c);
        if (rc) break;
        if (xb_out) memcpy(xb_out + (size_t)b * plane, xb, plane * sizeof(float));
        if (p->bypass_mask >> b & 1u) memcpy(yb, xb, plane * sizeof(float));
        else rc = ref_dyn_run(&p->band[b], xb, in_len, ch, yb);
        if (rc || (p->mute_mask >> b & 1u)) continue;
        for (size_t i = 0; i < plane; i++) acc[i] = first ? (double)yb[i] : acc[i] + (double)yb[i];
        first = 0;
    }
    if (!rc && y)
        for (size_t i = 0; i < plane; i++) y[i] = first ? 0.0f : (float)acc[i];
    free(xb);
    free(yb);
    free(acc);
    return rc;
}

/* the statement: what the GPU computes, bit for bit */
int ref_mb_run(const ref_mb_params* p, const float* x, size_t in_len, int ch, float* y) { return y ? multiband(p, x, in_len, ch, NULL, y) : -1; }

/* the band signals xb[n_bands][in_len][ch] of the statement */
int ref_mb_bands(const ref_mb_params* p, const float* x, size_t in_len, int ch, float* xb) { return xb ? multiband(p, x, in_len, ch, xb, NULL) : -1; }

/* one channel x[in_len]: the band signals w[n_bands][in_len] in front of their rounding; tiled != 0: K11's tiled form, else the plain recurrence */
int ref_mb_split_f64(const ref_mb_params* p, const float* x, size_t in_len, int tiled_form, double* w)
{
    if (ref_mb_check(p, 1) || !x || !w) return -1;
    for (int b = 0; b < p->n_bands; b++) {
        double coef[MB_MAX_PATH * 5];
        const int n = path_coef(p, b, coef);
        const int rc = tiled_form ? ref_eq_run_f64(coef, n, x, in_len, 1, w + (size_t)b * in_len) : ref_eq_sequential(coef, n, x, in_len, 1, w + (size_t)b * in_len);
        if (rc) return rc;
    }
    return 0;
}

/* the cookbook's all-pass at the w0, alpha and q of ref_eq_design's low-pass and high-pass */
static void allpass(int sample_rate, double freq, double q, double* coef)
{
    const double pi = 3.14159265358979323846;
    const double w0 = 2.0 * pi * freq / (double)sample_rate;
    const double cs = cos(w0), alpha = sin(w0) / (2.0 * q);
    const double a0 = 1.0 + alpha;
    coef[0] = (1.0 - alpha) / a0;
    coef[1] = (-2.0 * cs) / a0;
    coef[2] = (1.0 + alpha) / a0;
    coef[3] = (-2.0 * cs) / a0;
    coef[4] = (1.0 - alpha) / a0;
}

/* nae_mb_design of include/nae_gpu.h: -1 for everything it refuses */
int ref_mb_design(int sample_rate, int n_bands, const double* crossover_hz, const ref_dyn_params* bands, unsigned mute_mask, unsigned bypass_mask,
                  ref_mb_params* out)
{
    if (!out || !crossover_hz || !bands || sample_rate <= 0 || n_bands < 2 || n_bands > MB_MAX_BANDS) return -1;
    if ((mute_mask | bypass_mask) >> n_bands) return -1;
    /* (kind, crossover) per slot; kind 0 LP, 1 HP, 2 AP */
    static const signed char tree[3][MB_MAX_SECTIONS][2] = {
        {{0, 0}, {0, 0}, {1, 0}, {1, 0}},
        {{0, 0}, {0, 0}, {2, 1}, {1, 0}, {1, 0}, {0, 1}, {0, 1}, {1, 1}, {1, 1}},
        {{0, 1}, {0, 1}, {2, 2}, {0, 0}, {0, 0}, {1, 0}, {1, 0}, {1, 1}, {1, 1}, {2, 0}, {0, 2}, {0, 2}, {1, 2}, {1, 2}}};
    const double q = 0.7071067811865476;
    ref_mb_params p;
    memset(&p, 0, sizeof(p));
    p.n_bands = n_bands;
    p.n_sections = ref_mb_sections(n_bands);
    for (int i = 0; i < n_bands - 1; i++)
        if (!isfinite(crossover_hz[i]) || (i && !(crossover_hz[i] > crossover_hz[i - 1]))) return -1;
    for (int s = 0; s < p.n_sections; s++) {
        const int kind = tree[n_bands - 2][s][0];
        const double f = crossover_hz[tree[n_bands - 2][s][1]];
        if (ref_eq_design(3, sample_rate, f, 0.0, q, p.coef[s])) return -1;     /* the crossover's own check */
        if (kind == 1 && ref_eq_design(4, sample_rate, f, 0.0, q, p.coef[s])) return -1;
        if (kind == 2) allpass(sample_rate, f, q, p.coef[s]);
    }
    for (int b = 0; b < n_bands; b++) p.band[b] = bands[b];
    p.mute_mask = mute_mask;
    p.bypass_mask = bypass_mask;
    if (ref_mb_check(&p, 1)) return -1;
    *out = p;
    return 0;
}

#ifdef REF_MB_MAIN
#include <stdio.h>
int main(void)
{
    enum { N = 3 * C + 7 };
    static float x[N * 2], y[N * 2], xb[MB_MAX_BANDS * N * 2];
    static double w[MB_MAX_BANDS * N];
    unsigned s = 1u;
    for (int i = 0; i < N * 2; i++) {
        s = s * 1664525u + 1013904223u;
        x[i] = ((i / 2) % 700 < 90 ? 0.9f : 0.03f) * ((float)(s >> 8) / 8388608.0f - 1.0f);
    }
    const double xs[3] = {120.0, 1000.0, 6000.0};
    int bad = 0;
    for (int nb = 2; nb <= MB_MAX_BANDS; nb++)
        for (int ch = 1; ch <= 2; ch++)
            for (int link = 0; link <= 1; link++)
                for (unsigned mask = 0; mask < 4; mask++) {
                    ref_dyn_params bands[MB_MAX_BANDS];
                    for (int b = 0; b < nb; b++)
                        if (ref_dyn_design(48000, -30.0 + 3.0 * b, 4.0, 6.0, 0.002, 0.05, 17.0 / 48000.0, 2.0, link, &bands[b])) bad++;
                    ref_mb_params p;
                    if (ref_mb_design(48000, nb, xs, bands, mask & 1u, mask & 2u, &p)) { bad++; continue; }
                    bad += ref_mb_run(&p, x, N, ch, y) != 0;
                    bad += ref_mb_bands(&p, x, N, ch, xb) != 0;
                    bad += ref_mb_split_f64(&p, x, N, 1, w) != 0;
                    bad += ref_mb_split_f64(&p, x, N, 0, w) != 0;
                    bad += ref_mb_run(&p, x, 1, ch, y) != 0;
                }
    printf("ref_mb: %d failures\n", bad);
    return bad != 0;
}
#endif
