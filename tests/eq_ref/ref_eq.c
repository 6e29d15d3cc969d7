/* ref_eq.c — the CPU statement of K11, the biquad cascade ("K11 biquad cascade"): the tiled form the GPU computes, bit for bit
 * (ref_eq_run), the plain sequential double recurrence it is measured against (ref_eq_sequential), the same recurrence in long double that
 * both are measured against at steady state (ref_eq_sequential_ld), the tables of one section (ref_eq_tables), and the design (ref_eq_design).
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written here. */
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#define T 16            /* NAE_EQ_LANE */
#define LANES 64
#define C (LANES * T)   /* NAE_EQ_CHUNK */
#define MAX_SECTIONS 16 /* NAE_EQ_MAX_SECTIONS */

/* 0 when the cascade is acceptable: 1 ... 16 sections, finite, strictly stable */
int ref_eq_check(const double* coef, int n_sections)
{
    if (!coef || n_sections < 1 || n_sections > MAX_SECTIONS) return -1;
    for (int s = 0; s < n_sections; s++) {
        const double* c = coef + 5 * s;
        for (int i = 0; i < 5; i++)
            if (!isfinite(c[i])) return -1;
        if (!(fabs(c[4]) < 1.0 && fabs(c[3]) < 1.0 + c[4])) return -1;
    }
    return 0;
}

/* Double-double arithmetic for step 2: a value is hi + lo with |lo| <= ulp(hi) / 2, about 106 bits.  Every line is plain IEEE double
 * arithmetic (two-sum, and a two-product by fma()), written operation for operation as in eq_make_tables (kernels_eq.hip): the two must
 * give the same bits. */
typedef struct { double hi, lo; } dd;

static dd dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    const dd r = { s, (a - (s - bb)) + (b - bb) };
    return r;
}

/* |a| >= |b| or a == 0 */
static dd dd_quick_sum(double a, double b)
{
    const double s = a + b;
    const dd r = { s, b - (s - a) };
    return r;
}

static dd dd_two_prod(double a, double b)
{
    const double p = a * b;
    const dd r = { p, fma(a, b, -p) };
    return r;
}

static dd dd_add(dd x, dd y)
{
    dd s = dd_two_sum(x.hi, y.hi);
    const dd t = dd_two_sum(x.lo, y.lo);
    s = dd_quick_sum(s.hi, s.lo + t.hi);
    return dd_quick_sum(s.hi, s.lo + t.lo);
}

static dd dd_mul(dd x, dd y)
{
    const dd p = dd_two_prod(x.hi, y.hi);
    return dd_quick_sum(p.hi, p.lo + ((x.hi * y.lo) + (x.lo * y.hi)));
}

/* step 2: p, q and Phi_0 ... Phi_5 (m00 m01 m10 m11) of one section by the zero-input recurrence in its literal order and five squarings, all in
 * double-double; every entry is rounded to double once, at the end */
static void tables(double a1, double a2, double* p, double* q, double phi[6][4])
{
    const dd na1 = { -a1, 0.0 }, na2 = { -a2, 0.0 };
    dd m[4], r[4];
    for (int col = 0; col < 2; col++) {
        dd z1 = { col == 0 ? 1.0 : 0.0, 0.0 }, z2 = { col == 0 ? 0.0 : 1.0, 0.0 };
        double* out = col == 0 ? p : q;
        for (int n = 0; n < T; n++) {
            const dd y = z1;
            z1 = dd_add(dd_mul(na1, y), z2);
            z2 = dd_mul(na2, y);
            out[n] = y.hi + y.lo;
        }
        m[col] = z1;
        m[2 + col] = z2;
    }
    for (int j = 0; j < 6; j++) {
        for (int i = 0; i < 4; i++) phi[j][i] = m[i].hi + m[i].lo;
        r[0] = dd_add(dd_mul(m[0], m[0]), dd_mul(m[1], m[2]));
        r[1] = dd_add(dd_mul(m[0], m[1]), dd_mul(m[1], m[3]));
        r[2] = dd_add(dd_mul(m[2], m[0]), dd_mul(m[3], m[2]));
        r[3] = dd_add(dd_mul(m[2], m[1]), dd_mul(m[3], m[3]));
        for (int i = 0; i < 4; i++) m[i] = r[i];
    }
}

/* the statement's tables of one section in the library's block order: p[16] q[16] Phi_0 ... Phi_5, each m00 m01 m10 m11 */
void ref_eq_tables(double a1, double a2, double* out)
{
    double phi[6][4];
    tables(a1, a2, out, out + T, phi);
    memcpy(out + 2 * T, phi, sizeof(phi));
}

/* one channel: x[n * stride], n < in_len, through the cascade: y[n * stride] rounded to f32 and / or yd[n] as it stands in double */
static int tiled(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, float* y, double* yd)
{
    if (ref_eq_check(coef, n_sections) || !x || (!y && !yd)) return -1;
    double p[MAX_SECTIONS][T], q[MAX_SECTIONS][T], phi[MAX_SECTIONS][6][4];
    double carry[MAX_SECTIONS][2];
    for (int s = 0; s < n_sections; s++) {
        tables(coef[5 * s + 3], coef[5 * s + 4], p[s], q[s], phi[s]);
        carry[s][0] = carry[s][1] = 0.0;
    }
    double v[C];
    double E[LANES][2], P[LANES][2], st[LANES][2];
    for (size_t n0 = 0; n0 < in_len; n0 += C) {
        for (int n = 0; n < C; n++) v[n] = n0 + n < in_len ? (double)x[(n0 + n) * stride] : 0.0;
        for (int s = 0; s < n_sections; s++) {
            const double b0 = coef[5 * s], b1 = coef[5 * s + 1], b2 = coef[5 * s + 2], a1 = coef[5 * s + 3], a2 = coef[5 * s + 4];
            /* 1: the zero-state pass of every lane */
            for (int l = 0; l < LANES; l++) {
                double z1 = 0.0, z2 = 0.0;
                for (int k = 0; k < T; k++) {
                    const double xv = v[l * T + k];
                    const double yv = b0 * xv + z1;
                    z1 = (b1 * xv - a1 * yv) + z2;
                    z2 = b2 * xv - a2 * yv;
                    v[l * T + k] = yv;
                }
                E[l][0] = z1;
                E[l][1] = z2;
            }
            /* 3: the carry */
            const double in1 = carry[s][0], in2 = carry[s][1];
            {
                const double* m = phi[s][0];
                const double e1 = E[0][0] + ((m[0] * in1) + (m[1] * in2));
                const double e2 = E[0][1] + ((m[2] * in1) + (m[3] * in2));
                E[0][0] = e1;
                E[0][1] = e2;
            }
            for (int j = 0; j < 6; j++) {
                const double* m = phi[s][j];
                memcpy(P, E, sizeof(E));
                for (int l = 1 << j; l < LANES; l++) {
                    const double u1 = P[l - (1 << j)][0], u2 = P[l - (1 << j)][1];
                    E[l][0] = P[l][0] + ((m[0] * u1) + (m[1] * u2));
                    E[l][1] = P[l][1] + ((m[2] * u1) + (m[3] * u2));
                }
            }
            st[0][0] = in1;
            st[0][1] = in2;
            for (int l = 1; l < LANES; l++) {
                st[l][0] = E[l - 1][0];
                st[l][1] = E[l - 1][1];
            }
            carry[s][0] = E[LANES - 1][0];
            carry[s][1] = E[LANES - 1][1];
            /* 4: the correction */
            for (int l = 0; l < LANES; l++)
                for (int k = 0; k < T; k++) v[l * T + k] = v[l * T + k] + ((p[s][k] * st[l][0]) + (q[s][k] * st[l][1]));
        }
        for (int n = 0; n < C && n0 + n < in_len; n++) {
            if (y) y[(n0 + n) * stride] = (float)v[n];
            if (yd) yd[n0 + n] = v[n];
        }
    }
    return 0;
}

/* the tiled statement: what the GPU computes, bit for bit */
int ref_eq_run(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, float* y)
{
    return tiled(coef, n_sections, x, in_len, stride, y, NULL);
}

/* the tiled statement in front of its final rounding, for measuring it against ref_eq_sequential */
int ref_eq_run_f64(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, double* y)
{
    return tiled(coef, n_sections, x, in_len, stride, NULL, y);
}

/* the plain sequential recurrence in double, section after section, not rounded */
int ref_eq_sequential(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, double* y)
{
    if (ref_eq_check(coef, n_sections) || !x || !y) return -1;
    for (size_t n = 0; n < in_len; n++) y[n] = (double)x[n * stride];
    for (int s = 0; s < n_sections; s++) {
        const double b0 = coef[5 * s], b1 = coef[5 * s + 1], b2 = coef[5 * s + 2], a1 = coef[5 * s + 3], a2 = coef[5 * s + 4];
        double z1 = 0.0, z2 = 0.0;
        for (size_t n = 0; n < in_len; n++) {
            const double xv = y[n];
            const double yv = b0 * xv + z1;
            z1 = (b1 * xv - a1 * yv) + z2;
            z2 = b2 * xv - a2 * yv;
            y[n] = yv;
        }
    }
    return 0;
}

/* the same recurrence with every value and operation in long double (64 bits of significand or more: ref_eq_ldbl_mant_dig), returned as
 * double: what the two forms above are measured against at steady state */
int ref_eq_sequential_ld(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, double* y)
{
    if (ref_eq_check(coef, n_sections) || !x || !y) return -1;
    long double* v = malloc((in_len ? in_len : 1) * sizeof(long double));
    if (!v) return -1;
    for (size_t n = 0; n < in_len; n++) v[n] = (long double)x[n * stride];
    for (int s = 0; s < n_sections; s++) {
        const long double b0 = coef[5 * s], b1 = coef[5 * s + 1], b2 = coef[5 * s + 2], a1 = coef[5 * s + 3], a2 = coef[5 * s + 4];
        long double z1 = 0.0L, z2 = 0.0L;
        for (size_t n = 0; n < in_len; n++) {
            const long double xv = v[n];
            const long double yv = b0 * xv + z1;
            z1 = (b1 * xv - a1 * yv) + z2;
            z2 = b2 * xv - a2 * yv;
            v[n] = yv;
        }
    }
    for (size_t n = 0; n < in_len; n++) y[n] = (double)v[n];
    free(v);
    return 0;
}

int ref_eq_ldbl_mant_dig(void) { return LDBL_MANT_DIG; }

/* the same recurrence with every value and operation in f32: what the choice of double is measured against */
int ref_eq_sequential_f32(const double* coef, int n_sections, const float* x, size_t in_len, size_t stride, float* y)
{
    if (ref_eq_check(coef, n_sections) || !x || !y) return -1;
    for (size_t n = 0; n < in_len; n++) y[n] = x[n * stride];
    for (int s = 0; s < n_sections; s++) {
        const float b0 = (float)coef[5 * s], b1 = (float)coef[5 * s + 1], b2 = (float)coef[5 * s + 2], a1 = (float)coef[5 * s + 3],
                    a2 = (float)coef[5 * s + 4];
        float z1 = 0.0f, z2 = 0.0f;
        for (size_t n = 0; n < in_len; n++) {
            const float xv = y[n];
            const float yv = b0 * xv + z1;
            z1 = (b1 * xv - a1 * yv) + z2;
            z2 = b2 * xv - a2 * yv;
            y[n] = yv;
        }
    }
    return 0;
}

/* the Audio EQ Cookbook's forms (kinds 0 ... 5: peak, low shelf, high shelf, low-pass, high-pass, notch), divided through by a0 */
int ref_eq_design(int kind, int sample_rate, double freq, double gain_db, double q, double* coef)
{
    if (!coef || kind < 0 || kind > 5 || sample_rate <= 0) return -1;
    if (!(freq > 0.0 && freq < 0.5 * (double)sample_rate) || !(q >= 0.1 && q <= 40.0) || !(fabs(gain_db) <= 24.0)) return -1;
    const double pi = 3.14159265358979323846;
    const double A = pow(10.0, gain_db / 40.0), w0 = 2.0 * pi * freq / (double)sample_rate;
    const double cs = cos(w0), alpha = sin(w0) / (2.0 * q), r = 2.0 * sqrt(A) * alpha;
    double b0, b1, b2, a0, a1, a2;
    switch (kind) {
    case 0:
        b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A; a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
        break;
    case 1:
        b0 = A * ((A + 1.0) - (A - 1.0) * cs + r); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs); b2 = A * ((A + 1.0) - (A - 1.0) * cs - r);
        a0 = (A + 1.0) + (A - 1.0) * cs + r; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - r;
        break;
    case 2:
        b0 = A * ((A + 1.0) + (A - 1.0) * cs + r); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs); b2 = A * ((A + 1.0) + (A - 1.0) * cs - r);
        a0 = (A + 1.0) - (A - 1.0) * cs + r; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - r;
        break;
    default:
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        if (kind == 3) { b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = (1.0 - cs) / 2.0; }
        else if (kind == 4) { b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = (1.0 + cs) / 2.0; }
        else { b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0; }
    }
    coef[0] = b0 / a0; coef[1] = b1 / a0; coef[2] = b2 / a0; coef[3] = a1 / a0; coef[4] = a2 / a0;
    return 0;
}
