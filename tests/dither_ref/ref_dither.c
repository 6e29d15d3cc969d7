// ref_dither.c — the CPU statement of the dither ("K23 dither"): the plain sequential form, one stream-channel after the other,
// every step in double in the order the specification writes it.  "fused" steps are fma() (one rounding); every other step is one IEEE
// operation (built with -ffp-contract=off).  The state (position and error history) is a record the caller keeps, so a signal can be run in
// pieces; ref_dither_r12 exports the random source, ref_dither_check the parameter rules, ref_dither_design the presets.
// `after_clamp` plants the mistake the clamp test is there to catch (the error taken behind the clamp) and is 0 everywhere else.
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAX_TAPS 12
#define MAX_TAP_SUM 64.0
enum { KIND_NONE, KIND_RECTANGULAR, KIND_TRIANGULAR, KIND_HIGHPASS };

typedef struct {
    int bits, kind, n_taps;
    double taps[MAX_TAPS];
    uint64_t seed;
} params_t;

// per stream-channel: the next sample's index and e[n - 1], e[n - 2], ...
typedef struct {
    uint64_t n;
    double e[MAX_TAPS];
} state_t;

static const uint64_t G = 0x9E3779B97F4A7C15ull;

static uint64_t fin(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint64_t ref_dither_key(uint64_t seed, uint64_t stream, uint64_t channel) { return fin(fin(fin(seed + G) + stream) + channel); }

static double half(uint32_t w) { return (double)(int32_t)w * 0x1p-32; }

void ref_dither_r12(uint64_t key, uint64_t n, double* r1, double* r2)
{
    const uint64_t h = fin(key + G * n);
    *r1 = half((uint32_t)(h >> 32));
    *r2 = half((uint32_t)h);
}

double ref_dither_d(uint64_t key, uint64_t n, int kind)
{
    double r1, r2, b1 = 0.0, b2;
    if (kind == KIND_NONE) return 0.0;
    ref_dither_r12(key, n, &r1, &r2);
    if (kind == KIND_RECTANGULAR) return r1;
    if (kind == KIND_TRIANGULAR) return r1 + r2;
    if (n) ref_dither_r12(key, n - 1, &b1, &b2);
    return r1 - b1;
}

int ref_dither_check(const params_t* p, int ch)
{
    if (!p || (ch != 1 && ch != 2)) return -1;
    if (p->bits < 8 || p->bits > 24 || p->kind < KIND_NONE || p->kind > KIND_HIGHPASS || p->n_taps < 0 || p->n_taps > MAX_TAPS) return -1;
    double sum = 0.0;
    for (int k = 0; k < p->n_taps; k++) {
        if (!isfinite(p->taps[k])) return -1;
        sum += fabs(p->taps[k]);
    }
    return sum <= MAX_TAP_SUM ? 0 : -1;
}

int ref_dither_design(int bits, int kind, int shaping, uint64_t seed, params_t* out)
{
    static const double first[] = {1.0}, second[] = {2.0, -1.0}, lipshitz[] = {2.033, -2.165, 1.959, -1.590, 0.6149};
    static const double* const taps[] = {0, first, second, lipshitz};
    static const int count[] = {0, 1, 2, 5};
    if (!out || bits < 8 || bits > 24 || kind < KIND_NONE || kind > KIND_HIGHPASS || shaping < 0 || shaping > 3) return -1;
    memset(out, 0, sizeof(*out));
    out->bits = bits;
    out->kind = kind;
    out->n_taps = count[shaping];
    for (int k = 0; k < count[shaping]; k++) out->taps[k] = taps[shaping][k];
    out->seed = seed;
    return 0;
}

// x[n_frames][ch] -> y[n_frames][ch] as stream `stream` of a call; st[ch] carries on from where the last piece stopped (all zero: sample 0).
// e_out (may be null): e[n] per sample, [n_frames][ch]
int ref_dither_run(const params_t* p, uint64_t stream, const float* x, size_t n_frames, int ch, state_t* st, float* y, double* e_out, int after_clamp)
{
    if (ref_dither_check(p, ch)) return -1;
    const double S = ldexp(1.0, p->bits - 1);
    const int K = p->n_taps;
    for (int c = 0; c < ch; c++) {
        const uint64_t key = ref_dither_key(p->seed, stream, (uint64_t)c);
        state_t* s = &st[c];
        for (size_t i = 0; i < n_frames; i++) {
            const float xi = x[i * ch + c];
            const double t = isfinite(xi) ? (double)xi * S : 0.0;          // exact; a sample that is not finite counts as zero
            double u = t;
            for (int k = K; k >= 1; k--) u = fma(-p->taps[k - 1], s->e[k - 1], u);   // fused, the oldest error first
            const double d = ref_dither_d(key, s->n, p->kind);
            const double q = rint(u + d);                                 // one add, one round to nearest even
            const double qc = q < -S ? -S : (q > S - 1.0 ? S - 1.0 : q);
            const double e = (after_clamp ? qc : q) - u;                  // one subtract, in front of the clamp
            for (int k = K - 1; k > 0; k--) s->e[k] = s->e[k - 1];
            if (K) s->e[0] = e;
            s->n++;
            y[i * ch + c] = (float)(qc / S);                              // exact
            if (e_out) e_out[i * ch + c] = e;
        }
    }
    return 0;
}
