/* ref_loud.c — the CPU statement of K14, the loudness meter ("K14 loudness"): the tiled form the GPU computes, bit for bit, and
 * the plain sequential form it is measured against (ref_loud_measure with tiled = 1 and 0), the design (ref_loud_design) and the true-peak taps
 * (ref_loud_taps).  The K-weighting is the equalizer's statement with two sections (eq_ref/ref_eq.c: its tiled form and its sequential
 * recurrence, unrounded).  Built with -ffp-contract=off: every step is one IEEE operation in the order written here. */
#include "../eq_ref/ref_eq.c"

#define SECTIONS 2      /* NAE_LOUD_SECTIONS */
#define PHASES 4        /* NAE_LOUD_TP_PHASES */
#define TAPS 12         /* NAE_LOUD_TP_TAPS */
#define KAISER_BETA 8.0 /* NAE_FIR_KAISER_BETA */

/* nae_loud_params and nae_loud_result (include/nae_gpu.h), field for field */
typedef struct {
    int sample_rate, sub_block;
    double coef[5 * SECTIONS];
    double gate_abs, target, ceiling_lin, max_gain_lin;
} loud_params;

typedef struct {
    double mean2, momentary_max, gain;
    float gain_f32, true_peak[2], sample_peak[2];
    unsigned blocks_total, blocks_abs, blocks_rel;
} loud_result;

/* the library's power series of I0 (the Kaiser windows of the transposer and the FIR designs) */
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

/* the 4x oversampler: h[i] = sinc((i - 23.5) / 4) w[i], a 48-tap Kaiser-windowed sinc; phase p takes h[p + 4 k], divided by its own sum and
 * rounded once: out[p][k] */
void ref_loud_taps(float* out)
{
    const double pi = 3.14159265358979323846;
    const double half = 0.5 * (double)(PHASES * TAPS - 1), i0b = bessel_i0(KAISER_BETA);
    double h[PHASES * TAPS];
    for (int i = 0; i < PHASES * TAPS; i++) {
        const double t = (double)i - half;
        const double a = t / half;
        const double r = 1.0 - a * a;
        const double w = bessel_i0(KAISER_BETA * sqrt(r > 0.0 ? r : 0.0)) / i0b;
        const double arg = pi * (t / (double)PHASES);
        h[i] = sin(arg) / arg * w;
    }
    for (int p = 0; p < PHASES; p++) {
        double sum = 0.0;
        for (int k = 0; k < TAPS; k++) sum += h[p + PHASES * k];
        for (int k = 0; k < TAPS; k++) out[p * TAPS + k] = (float)(h[p + PHASES * k] / sum);
    }
}

/* 0, -1 (NAE_ERR_INVALID) or -2 (NAE_ERR_UNSUPPORTED), as nae_loud_design */
int ref_loud_design(int sample_rate, double target_lufs, double ceiling_dbtp, double max_gain_db, loud_params* out)
{
    if (!out) return -1;
    if (!(target_lufs >= -70.0 && target_lufs <= -5.0) || !(ceiling_dbtp >= -20.0 && ceiling_dbtp <= 0.0) || !(max_gain_db >= 0.0 && max_gain_db <= 40.0))
        return -1;
    if (sample_rate < 8000 || sample_rate > 192000 || sample_rate % 10 != 0) return -2;
    const double pi = 3.14159265358979323846;
    memset(out, 0, sizeof(*out));
    out->sample_rate = sample_rate;
    out->sub_block = sample_rate / 10;
    {
        const double K = tan(pi * 1681.974450955533 / (double)sample_rate);
        const double Vh = pow(10.0, 3.999843853973347 / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double kq = K / 0.7071752369554196, kk = K * K;
        const double a0 = 1.0 + kq + kk;
        out->coef[0] = (Vh + Vb * kq + kk) / a0;
        out->coef[1] = 2.0 * (kk - Vh) / a0;
        out->coef[2] = (Vh - Vb * kq + kk) / a0;
        out->coef[3] = 2.0 * (kk - 1.0) / a0;
        out->coef[4] = (1.0 - kq + kk) / a0;
    }
    {
        const double K = tan(pi * 38.13547087602444 / (double)sample_rate);
        const double kq = K / 0.5003270373238773, kk = K * K;
        const double a0 = 1.0 + kq + kk;
        out->coef[5] = 1.0;
        out->coef[6] = -2.0;
        out->coef[7] = 1.0;
        out->coef[8] = 2.0 * (kk - 1.0) / a0;
        out->coef[9] = (1.0 - kq + kk) / a0;
    }
    out->gate_abs = pow(10.0, (-70.0 + 0.691) / 10.0);
    out->target = pow(10.0, (target_lufs + 0.691) / 10.0);
    out->ceiling_lin = pow(10.0, ceiling_dbtp / 20.0);
    out->max_gain_lin = pow(10.0, max_gain_db / 20.0);
    return 0;
}

/* E[u], u < U, of one channel's weighted signal w in the GPU's order: per chunk of 1024 every lane adds its own samples of the sub-block in
 * index order from 0.0, the 64 sums go through a butterfly over the distances 32 ... 1, and the chunk's sum is added to E[u] in chunk order */
static void energies_tiled(const double* w, size_t in_len, size_t B, size_t U, double* E, size_t stride)
{
    for (size_t u = 0; u < U; u++) E[u * stride] = 0.0;
    for (size_t n0 = 0; n0 < in_len; n0 += C) {
        for (size_t u = n0 / B; u <= (n0 + C - 1) / B && u < U; u++) {
            double lane[LANES], next[LANES];
            for (int l = 0; l < LANES; l++) {
                double sum = 0.0;
                for (int k = 0; k < T; k++) {
                    const size_t n = n0 + (size_t)(l * T + k);
                    const double sq = n < in_len ? w[n] * w[n] : 0.0;   /* u < U: every sample of the sub-block lies below in_len */
                    if (n >= u * B && n < (u + 1) * B) sum = sum + sq;
                }
                lane[l] = sum;
            }
            for (int d = 32; d >= 1; d >>= 1) {
                for (int l = 0; l < LANES; l++) next[l] = lane[l] + lane[l ^ d];
                memcpy(lane, next, sizeof(lane));
            }
            E[u * stride] = E[u * stride] + lane[0];
        }
    }
}

/* the plain form: every sub-block summed in index order */
static void energies_sequential(const double* w, size_t B, size_t U, double* E, size_t stride)
{
    for (size_t u = 0; u < U; u++) {
        double sum = 0.0;
        for (size_t n = u * B; n < (u + 1) * B; n++) sum = sum + w[n] * w[n];
        E[u * stride] = sum;
    }
}

/* One stream: x interleaved [in_len][ch] -> the record; E_out (may be null) receives the sub-block energies [in_len / B][ch].
 * tiled = 1: the K-weighting and the energies in the GPU's tiling (what the GPU computes, bit for bit); 0: the sequential recurrence and plain
 * sums.  The gates, the true peak and the gain are the same in both. */
int ref_loud_measure(const loud_params* p, const float* x, size_t in_len, int ch, int tiled_form, loud_result* out, double* E_out)
{
    if (!p || !x || !out || (ch != 1 && ch != 2) || in_len == 0) return -1;
    const size_t B = (size_t)p->sub_block, U = in_len / B, blocks = U >= 4 ? U - 3 : 0;
    double* w = malloc(in_len * sizeof(double));
    double* E = calloc((U ? U : 1) * (size_t)ch, sizeof(double));
    if (!w || !E) { free(w); free(E); return -1; }
    float taps[PHASES * TAPS];
    ref_loud_taps(taps);
    memset(out, 0, sizeof(*out));
    for (int c = 0; c < ch; c++) {
        const int rc = tiled_form ? tiled(p->coef, SECTIONS, x + c, in_len, (size_t)ch, NULL, w) : ref_eq_sequential(p->coef, SECTIONS, x + c, in_len, (size_t)ch, w);
        if (rc) { free(w); free(E); return rc; }
        if (tiled_form) energies_tiled(w, in_len, B, U, E + c, (size_t)ch);
        else energies_sequential(w, B, U, E + c, (size_t)ch);
        /* the peaks: v_p[n] = sum over k, in order, of t_p[k] x[n - k], n = 0 ... in_len + 10 */
        float tp = 0.0f, sp = 0.0f;
        for (size_t n = 0; n < in_len + TAPS - 1; n++) {
            if (n < in_len) {
                const float ax = fabsf(x[n * ch + c]);
                sp = ax > sp ? ax : sp;
            }
            for (int ph = 0; ph < PHASES; ph++) {
                float v = 0.0f;
                for (int k = 0; k < TAPS; k++) {
                    const float xv = n >= (size_t)k && n - k < in_len ? x[(n - k) * ch + c] : 0.0f;
                    const float prod = taps[ph * TAPS + k] * xv;
                    v = k == 0 ? prod : v + prod;
                }
                const float av = fabsf(v);
                tp = av > tp ? av : tp;
            }
        }
        out->true_peak[c] = tp;
        out->sample_peak[c] = sp;
    }
    if (E_out) memcpy(E_out, E, U * (size_t)ch * sizeof(double));
    /* the gates, in energy */
    const double d4b = (double)(4 * B);
    double sum1 = 0.0, sum2 = 0.0, mx = 0.0;
    unsigned n_abs = 0, n_rel = 0;
    for (int pass = 0; pass < 2; pass++) {
        const double gate_rel = n_abs ? 0.1 * (sum1 / (double)n_abs) : 0.0;
        for (size_t j = 0; j < blocks; j++) {
            double pw = 0.0;
            for (int c = 0; c < ch; c++) {
                const double* e = E + j * ch + c;
                const double z = ((e[0] + e[ch]) + (e[2 * ch] + e[3 * ch])) / d4b;
                pw = c == 0 ? z : pw + z;
            }
            if (pass == 0) {
                mx = pw > mx ? pw : mx;
                if (pw > p->gate_abs) { sum1 = sum1 + pw; n_abs++; }
            } else if (pw > p->gate_abs && pw > gate_rel) { sum2 = sum2 + pw; n_rel++; }
        }
    }
    out->mean2 = n_rel ? sum2 / (double)n_rel : 0.0;
    out->momentary_max = mx;
    out->blocks_total = (unsigned)blocks;
    out->blocks_abs = n_abs;
    out->blocks_rel = n_rel;
    /* the gain */
    float peak = 0.0f;
    for (int c = 0; c < ch; c++) {
        peak = out->true_peak[c] > peak ? out->true_peak[c] : peak;
        peak = out->sample_peak[c] > peak ? out->sample_peak[c] : peak;
    }
    double g = 1.0;
    if (n_rel) {
        g = sqrt(p->target / out->mean2);
        if (g * (double)peak > p->ceiling_lin) g = p->ceiling_lin / (double)peak;
        g = g > p->max_gain_lin ? p->max_gain_lin : g;
    }
    out->gain = g;
    out->gain_f32 = (float)g;
    free(w);
    free(E);
    return 0;
}

/* -0.691 + 10 log10(energy) */
double ref_loud_lufs(double energy) { return -0.691 + 10.0 * log10(energy); }
