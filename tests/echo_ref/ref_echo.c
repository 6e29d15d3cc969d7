/* ref_echo.c — the CPU statement of K16, the echo ("K16 echo"): the tiled form the GPU computes, bit for bit, and the plain
 * sequential form it is measured against (ref_echo_run with tiled = 1 and 0), the parameter rules (ref_echo_check) and the design
 * (ref_echo_design).  The loop's damping filter is the equalizer's statement (eq_ref/ref_eq.c): its tables and its design are used as they
 * stand; its tiled steps 1, 3 and 4 are restated here for ONE chunk with the carry handed in and out, because the loop feeds a chunk's output
 * back into a later chunk's input (ref_eq.c's own tiled() walks a whole signal).  tests/test_echo_cpu.py ties the restatement to ref_eq_run.
 * Built with -ffp-contract=off: every step is one IEEE double operation in the order written here. */
#include "../eq_ref/ref_eq.c"

#define ECHO_MAX_SECTIONS 4     /* NAE_ECHO_MAX_SECTIONS */
#define ECHO_MIN_DELAY C        /* NAE_ECHO_MIN_DELAY = NAE_EQ_CHUNK */
#define ECHO_MAX_DELAY (1 << 20) /* NAE_ECHO_MAX_DELAY */
#define ECHO_MAX_FEEDBACK 0.99  /* NAE_ECHO_MAX_FEEDBACK */

/* nae_echo_params (include/nae_gpu.h), field for field */
typedef struct {
    int delay[2];
    double feedback;
    int cross;
    double wet, dry;
    int n_sections;
    double coef[5 * ECHO_MAX_SECTIONS];
} echo_params;

/* 0, -1 (NAE_ERR_INVALID) or -2 (NAE_ERR_UNSUPPORTED), as the library's entries, in their order */
int ref_echo_check(const echo_params* p, int ch)
{
    if (!p || (ch != 1 && ch != 2)) return -1;
    if (!isfinite(p->feedback) || !isfinite(p->wet) || !isfinite(p->dry)) return -1;
    if (!(fabs(p->feedback) <= ECHO_MAX_FEEDBACK)) return -1;
    if (p->cross != 0 && p->cross != 1) return -1;
    if (p->n_sections < 0) return -1;
    if (p->n_sections > ECHO_MAX_SECTIONS) return -2;
    for (int c = 0; c < ch; c++)
        if (p->delay[c] < ECHO_MIN_DELAY || p->delay[c] > ECHO_MAX_DELAY) return -2;
    return p->n_sections ? ref_eq_check(p->coef, p->n_sections) : 0;
}

/* 0 or -1, as nae_echo_design */
int ref_echo_design(int sample_rate, double delay_s_left, double delay_s_right, double feedback, double damp_hz, double lowcut_hz, double wet,
                    double dry, int cross, echo_params* out)
{
    if (!out || sample_rate <= 0 || (cross != 0 && cross != 1)) return -1;
    if (!isfinite(delay_s_left) || !isfinite(delay_s_right) || !isfinite(feedback) || !isfinite(damp_hz) || !isfinite(lowcut_hz) || !isfinite(wet) ||
        !isfinite(dry))
        return -1;
    if (!(fabs(feedback) <= ECHO_MAX_FEEDBACK) || damp_hz < 0.0 || lowcut_hz < 0.0) return -1;
    echo_params p;
    memset(&p, 0, sizeof(p));
    const double d[2] = { delay_s_left * (double)sample_rate, delay_s_right * (double)sample_rate };
    for (int c = 0; c < 2; c++) {
        if (!(d[c] >= (double)ECHO_MIN_DELAY - 0.5 && d[c] <= (double)ECHO_MAX_DELAY + 0.5)) return -1;
        const long r = lround(d[c]);
        if (r < ECHO_MIN_DELAY || r > ECHO_MAX_DELAY) return -1;
        p.delay[c] = (int)r;
    }
    p.feedback = feedback;
    p.cross = cross;
    p.wet = wet;
    p.dry = dry;
    const double q = sqrt(0.5);
    if (damp_hz > 0.0 && ref_eq_design(3, sample_rate, damp_hz, 0.0, q, p.coef + 5 * p.n_sections++)) return -1;
    if (lowcut_hz > 0.0 && ref_eq_design(4, sample_rate, lowcut_hz, 0.0, q, p.coef + 5 * p.n_sections++)) return -1;
    *out = p;
    return 0;
}

/* what a channel's loop keeps between chunks: the tables of its sections and their carries */
typedef struct {
    double p[ECHO_MAX_SECTIONS][T], q[ECHO_MAX_SECTIONS][T], phi[ECHO_MAX_SECTIONS][6][4];
    double carry[ECHO_MAX_SECTIONS][2];
} echo_filter;

/* K11's steps 1, 3 and 4 (ref_eq.c, tiled()) on one chunk v[C] in place, section after section, the carries in f */
static void cascade_chunk(const double* coef, int n_sections, echo_filter* f, double* v)
{
    double E[LANES][2], P[LANES][2], st[LANES][2];
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
        const double in1 = f->carry[s][0], in2 = f->carry[s][1];
        {
            const double* m = f->phi[s][0];
            const double e1 = E[0][0] + ((m[0] * in1) + (m[1] * in2));
            const double e2 = E[0][1] + ((m[2] * in1) + (m[3] * in2));
            E[0][0] = e1;
            E[0][1] = e2;
        }
        for (int j = 0; j < 6; j++) {
            const double* m = f->phi[s][j];
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
        f->carry[s][0] = E[LANES - 1][0];
        f->carry[s][1] = E[LANES - 1][1];
        /* 4: the correction */
        for (int l = 0; l < LANES; l++)
            for (int k = 0; k < T; k++) v[l * T + k] = v[l * T + k] + ((f->p[s][k] * st[l][0]) + (f->q[s][k] * st[l][1]));
    }
}

/* x, y: interleaved [in_len][ch] (y may be x).  tiled = 1: what the GPU computes, bit for bit; tiled = 0: the same formulas with the sections'
 * direct-form recurrence sample by sample; the line is f32 in both.  line: if not null, receives w, [in_len][ch]. */
int ref_echo_run(const echo_params* p, const float* x, size_t in_len, int ch, float* y, int tiled, float* line)
{
    if (ref_echo_check(p, ch) || !x || !y) return -1;
    const int S = p->n_sections;
    const double g = p->feedback, wet = p->wet, dry = p->dry;
    float* w = malloc((in_len ? in_len : 1) * (size_t)ch * sizeof(float));    /* w_c[n] at w[n * ch + c] */
    echo_filter* f = calloc((size_t)ch, sizeof(echo_filter));
    if (!w || !f) { free(w); free(f); return -1; }
    size_t D[2];
    int from[2];
    for (int c = 0; c < ch; c++) {
        D[c] = (size_t)p->delay[c];
        from[c] = p->cross && ch == 2 ? 1 - c : c;
        for (int s = 0; s < S; s++) tables(p->coef[5 * s + 3], p->coef[5 * s + 4], f[c].p[s], f[c].q[s], f[c].phi[s]);
    }
    if (tiled) {
        double v[C];
        for (size_t n0 = 0; n0 < in_len; n0 += C) {
            for (int c = 0; c < ch; c++) {
                /* the delayed samples lie in earlier chunks of either channel: D >= C */
                for (int n = 0; n < C; n++) {
                    const size_t i = n0 + (size_t)n;
                    v[n] = i < in_len && i >= D[c] ? (double)w[(i - D[c]) * ch + from[c]] : 0.0;
                }
                cascade_chunk(p->coef, S, &f[c], v);
                for (int n = 0; n < C && n0 + n < in_len; n++) {
                    const size_t i = n0 + (size_t)n;
                    const double xd = (double)x[i * ch + c];
                    w[i * ch + c] = (float)(xd + (g * v[n]));
                    y[i * ch + c] = (float)((dry * xd) + (wet * v[n]));
                }
            }
        }
    } else {
        /* carry[s] is the section's (z1, z2) */
        for (size_t i = 0; i < in_len; i++)
            for (int c = 0; c < ch; c++) {
                double fv = i >= D[c] ? (double)w[(i - D[c]) * ch + from[c]] : 0.0;
                for (int s = 0; s < S; s++) {
                    const double b0 = p->coef[5 * s], b1 = p->coef[5 * s + 1], b2 = p->coef[5 * s + 2], a1 = p->coef[5 * s + 3], a2 = p->coef[5 * s + 4];
                    const double yv = b0 * fv + f[c].carry[s][0];
                    f[c].carry[s][0] = (b1 * fv - a1 * yv) + f[c].carry[s][1];
                    f[c].carry[s][1] = b2 * fv - a2 * yv;
                    fv = yv;
                }
                const double xd = (double)x[i * ch + c];
                w[i * ch + c] = (float)(xd + (g * fv));
                y[i * ch + c] = (float)((dry * xd) + (wet * fv));
            }
    }
    if (line) memcpy(line, w, in_len * (size_t)ch * sizeof(float));
    free(w);
    free(f);
    return 0;
}
