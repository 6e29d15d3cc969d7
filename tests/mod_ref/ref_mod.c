/* ref_mod.c — the CPU statement of K17, the modulated delay ("K17 modulated delay"): the plain sequential form, sample after
 * sample (ref_mod_run), the LFO alone (ref_mod_lfo), the parameter rules (ref_mod_check) and the design (ref_mod_design).  The GPU computes
 * runs of up to 64 samples in parallel; no sample's arithmetic depends on that, so this form is the statement and every run length must
 * give its bits.  Built with -ffp-contract=off: every step is one IEEE double operation in the order written here. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MOD_MIN_DELAY 2.0       /* NAE_MOD_MIN_DELAY */
#define MOD_MAX_DELAY 3070.0    /* NAE_MOD_MAX_DELAY */
#define MOD_MAX_VOICES 4        /* NAE_MOD_MAX_VOICES */
#define MOD_MAX_FEEDBACK 0.95   /* NAE_MOD_MAX_FEEDBACK */
#define MOD_SINE 0              /* NAE_MOD_SINE */
#define MOD_TRIANGLE 1          /* NAE_MOD_TRIANGLE */

/* nae_mod_params (include/nae_gpu.h), field for field */
typedef struct {
    double delay, depth, feedback, wet, dry;
    uint32_t rate_inc, phase0, phase_ch;
    int n_voices;
    uint32_t voice_phase[MOD_MAX_VOICES];
    int shape;
} mod_params;

/* 0, -1 (NAE_ERR_INVALID) or -2 (NAE_ERR_UNSUPPORTED), as the library's entries, in their order */
int ref_mod_check(const mod_params* p, int ch)
{
    if (!p || (ch != 1 && ch != 2)) return -1;
    if (!isfinite(p->delay) || !isfinite(p->depth) || !isfinite(p->feedback) || !isfinite(p->wet) || !isfinite(p->dry)) return -1;
    if (!(fabs(p->feedback) <= MOD_MAX_FEEDBACK)) return -1;
    if (p->depth < 0.0) return -1;
    if (p->n_voices < 1) return -1;
    if (p->shape != MOD_SINE && p->shape != MOD_TRIANGLE) return -1;
    if (p->n_voices > MOD_MAX_VOICES) return -2;
    if (!(p->delay - p->depth >= MOD_MIN_DELAY) || !(p->delay + p->depth <= MOD_MAX_DELAY)) return -2;
    return 0;
}

/* 0 or -1, as nae_mod_design */
int ref_mod_design(int sample_rate, double rate_hz, double delay_ms, double depth_ms, double feedback, int voices, double spread, int shape,
                   double wet, double dry, mod_params* out)
{
    if (!out || sample_rate <= 0) return -1;
    if (!isfinite(rate_hz) || !isfinite(delay_ms) || !isfinite(depth_ms) || !isfinite(feedback) || !isfinite(spread) || !isfinite(wet) || !isfinite(dry))
        return -1;
    if (rate_hz < 0.0 || rate_hz > 20.0 || depth_ms < 0.0 || !(fabs(feedback) <= MOD_MAX_FEEDBACK) || spread < 0.0 || spread > 1.0) return -1;
    if (voices < 1 || voices > MOD_MAX_VOICES || (shape != MOD_SINE && shape != MOD_TRIANGLE)) return -1;
    mod_params p;
    memset(&p, 0, sizeof(p));
    p.delay = (delay_ms * 1e-3) * (double)sample_rate;
    p.depth = (depth_ms * 1e-3) * (double)sample_rate;
    if (!(p.delay - p.depth >= MOD_MIN_DELAY) || !(p.delay + p.depth <= MOD_MAX_DELAY)) return -1;
    p.feedback = feedback;
    p.wet = wet;
    p.dry = dry;
    p.rate_inc = (uint32_t)(uint64_t)llround((rate_hz / (double)sample_rate) * 4294967296.0);
    p.phase0 = 0;
    p.phase_ch = (uint32_t)llround(spread * 2147483648.0);
    p.n_voices = voices;
    for (int v = 0; v < voices; v++) p.voice_phase[v] = (uint32_t)(((uint64_t)v << 32) / (uint64_t)voices);
    p.shape = shape;
    *out = p;
    return 0;
}

/* the LFO at phase phi, in turns 2^32: t = phi as a signed number of half turns, in [-1, 1); the sine form is the parabola 4 t (1 - |t|) with
 * one correction, the triangle is exact */
double ref_mod_lfo(int shape, uint32_t phi)
{
    const double t = (double)(int32_t)phi * 0x1p-31;
    if (shape == MOD_SINE) {
        const double y = (4.0 * t) * (1.0 - fabs(t));
        return (0.225 * ((y * fabs(y)) - y)) + y;
    }
    return (2.0 * fabs(t)) - 1.0;
}

/* x, y: interleaved [in_len][ch] (y may be x).  line: if not null, receives w, [in_len][ch]. */
int ref_mod_run(const mod_params* p, const float* x, size_t in_len, int ch, float* y, float* line)
{
    if (ref_mod_check(p, ch) || !x || !y) return -1;
    const double g = p->feedback, wet = p->wet, dry = p->dry;
    const double inv = 1.0 / (double)p->n_voices;
    float* w = malloc((in_len ? in_len : 1) * (size_t)ch * sizeof(float));    /* w_c[n] at w[n * ch + c] */
    if (!w) return -1;
    for (size_t i = 0; i < in_len; i++)
        for (int c = 0; c < ch; c++) {
            const uint64_t n = (uint64_t)i;
            double v = 0.0;
            for (int vc = 0; vc < p->n_voices; vc++) {
                const uint32_t phi = p->phase0 + p->voice_phase[vc] + (c == 1 ? p->phase_ch : 0u) + (uint32_t)(n * (uint64_t)p->rate_inc);
                const double l = ref_mod_lfo(p->shape, phi);
                const double d = p->delay + (p->depth * l);
                const long k = (long)floor(d);
                const double f = d - (double)k;
                const long at = (long)i - k;
                const double a = at + 1 >= 0 ? (double)w[(at + 1) * ch + c] : 0.0;
                const double b = at >= 0 ? (double)w[at * ch + c] : 0.0;
                const double c2 = at - 1 >= 0 ? (double)w[(at - 1) * ch + c] : 0.0;
                const double e = at - 2 >= 0 ? (double)w[(at - 2) * ch + c] : 0.0;
                const double fm1 = f - 1.0, fm2 = f - 2.0, fp1 = f + 1.0;
                const double ca = ((-(f * fm1)) * fm2) * (1.0 / 6.0);
                const double cb = ((fp1 * fm1) * fm2) * 0.5;
                const double cc = ((-(fp1 * f)) * fm2) * 0.5;
                const double ce = ((fp1 * f) * fm1) * (1.0 / 6.0);
                const double tap = (((ca * a) + (cb * b)) + (cc * c2)) + (ce * e);
                v = vc == 0 ? tap : v + tap;
            }
            const double u = v * inv;
            const double xd = (double)x[i * ch + c];
            w[i * ch + c] = g == 0.0 ? x[i * ch + c] : (float)(xd + (g * u));
            y[i * ch + c] = (float)((dry * xd) + (wet * u));
        }
    if (line) memcpy(line, w, in_len * (size_t)ch * sizeof(float));
    free(w);
    return 0;
}
