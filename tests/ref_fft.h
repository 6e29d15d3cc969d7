/* ref_fft.h — the canonical FFT of every size ("K8 spectrum, every size"), shared by the CPU statements
 * tests/spec_sizes/ref_spectrum.c and tests/pv_ref/ref_pv.c.  Written from the specification text, as plainly as possible: one recursive
 * decimation-in-frequency FFT, tables in double rounded once to f32.  Compile with -ffp-contract=off (fused multiply-adds appear only where
 * fmaf() is written). */
#ifndef REF_FFT_H
#define REF_FFT_H
#include <math.h>
#include <stdlib.h>

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

#endif
