/* ref_pv.c — CPU statement of the K7 phase vocoder ("Phase locking", "Formant preservation", "Transient preservation",
 * "Formant shift", "Channel link").
 *
 * The loops of oracle/orc_stft.c (plan, pv_channel, rs_channel, the stage order of orc_stretch_f32, orc_pv_synth_phase) with every option of
 * the vocoder as a parameter of one frame loop (pv_stream) and one node driver (ref_pv_run):
 *   N           the frame size, 512 ... 4096 (hop H = N / 4).  The FFT is the canonical one of every size (tests/ref_fft.h); the inverse is the
 *               oracle's irfft1024 generalised (split with T_N, conjugate, forward FFT_{N/2}, scale).
 *   lock        (N = 1024 only) replaces the Qs recurrence of frames f >= 1 by the locked one.
 *   q, g        lifter q > 0: every synthesis frame's magnitudes are multiplied by G[k] of the frame's cepstral envelope, transposer ratio g.
 *   transients  frame f >= 2 is an onset when the count of rising bins crosses NUM/DEN of the bins upwards, and an onset frame takes
 *               Qs_f = Qa_f in place of the recurrence, unlocked and locked alike.
 *   forced      the plan of the formant shift where the envelope stage runs without a tempo change: the vocoder stage on at tempo 1 (ha = H,
 *               d0 = H, r = 2^24).  A frame of the forced stage is Y = G X; its phase recurrence is still walked and leaves Qs = Qa.
 *   link        the onset rule and the lock's peaks and regions read Pl = 0.5f (P^0 + P^1) — one add with channel 0 first, one product — in
 *               place of each channel's P, so onset(f) and sigma_f are one decision per stream; Qa, inc, the magnitudes, the formant gain and
 *               Qs stay each channel's own.
 * With every option off at N = 1024 it equals orc_stretch_f32 and orc_pv_synth_phase bit for bit; its integer phases elsewhere are pinned by
 * tests/golden/pv_synth_phase.json and tests/golden/pv_option_phase.json.  The atan2 and the transposer's table are the oracle's own (linked
 * from oracle/libnae_oracle.so).  Built by tests/pv_ref.py with gcc -ffp-contract=off.
 */
#include "../../oracle/nae_oracle.h"
#include "../../include/nae_dsp_spec.h"
#include "../ref_fft.h"
#include <string.h>

static int size_ok(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

/* c2r, 1/N normalised: split with T_N, conjugate, forward FFT_M, scale (the oracle's irfft1024 at every size) */
static void irfft(const tables* t, const cf* X, float* y)
{
    const int M = t->M;
    cf* Zc = (cf*)malloc(sizeof(cf) * M);
    cf* z = (cf*)malloc(sizeof(cf) * M);
    for (int k = 0; k < M; k++) {
        cf Xk = X[k], Xm = X[M - k];
        if (k == 0) { Xk.y = 0.0f; Xm.y = 0.0f; }
        const cf E = {0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y - Xm.y)};
        const cf D = {0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y + Xm.y)};
        const cf T = t->TN[k];
        const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x}; /* conj(T) * D */
        Zc[k].x = E.x - Q.y;
        Zc[k].y = -(E.y + Q.x);
    }
    fft_dif(Zc, M, M, t->R1, t->WM, z);
    const float scale = 1.0f / (float)M;
    for (int m = 0; m < M; m++) {
        y[2 * m] = z[m].x * scale;
        y[2 * m + 1] = -z[m].y * scale;
    }
    free(Zc);
    free(z);
}

/* the plan at frame size N: the oracle's, with the hop, the ratios and the frame count of N */
int ref_pv_plan(double rate, double pitch, int N, size_t in_len, orc_stretch_plan* pl)
{
    if (!size_ok(N)) return -3;
    const int rc = orc_stretch_plan_make(rate, pitch, in_len, pl);
    if (rc) return rc;
    const int H = N / 4;
    pl->ha_q24 = (int64_t)llround((double)H * pl->tempo_eff * (double)(1 << NAE_HA_FRAC_BITS));
    pl->d0 = (int32_t)(pl->ha_q24 >> NAE_HA_FRAC_BITS);
    for (int i = 0; i < 2; i++) {
        const uint64_t d = (uint64_t)(pl->d0 + i);
        pl->r_q24[i] = (uint32_t)((((uint64_t)H << NAE_R_FRAC_BITS) + d / 2) / d);
    }
    const size_t pv_out = pl->rs_first ? pl->out_len : pl->mid_len;
    pl->frames = pl->pv_on ? (pv_out + N / 2 + H - 1) / H + 1 : 0;
    return 0;
}

static inline int64_t frame_start(const orc_stretch_plan* pl, int N, int64_t f)
{
    return (((f - 1) * pl->ha_q24 + ((int64_t)1 << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - N / 2;
}

/* phase locking, rule 2 of DESIGN.md §3: the peaks of the power spectrum P[0..BINS); a neighbour outside 0..BINS-1 counts as satisfied, a
 * NaN compares false.  Returns the number of peaks. */
static int peaks(const float* P, int BINS, unsigned char* peak)
{
    int n = 0;
    for (int k = 0; k < BINS; k++) {
        int ok = P[k] > 0.0f;
        if (k >= 1) ok = ok && P[k] > P[k - 1];
        if (k >= 2) ok = ok && P[k] > P[k - 2];
        if (k + 1 < BINS) ok = ok && P[k] >= P[k + 1];
        if (k + 2 < BINS) ok = ok && P[k] >= P[k + 2];
        peak[k] = (unsigned char)ok;
        n += ok;
    }
    return n;
}

/* rule 3: sigma[k] = the nearest peak of P, a tie to the lower one; no peak at all: k */
static void regions(const float* P, int BINS, int* sigma)
{
    unsigned char* peak = (unsigned char*)malloc((size_t)BINS);
    const int n = peaks(P, BINS, peak);
    for (int k = 0; k < BINS; k++) {
        if (!n) { sigma[k] = k; continue; }
        int best = -1;
        for (int p = 0; p < BINS; p++)
            if (peak[p] && (best < 0 || abs(k - p) < abs(k - best))) best = p;   /* ascending p: a tie keeps the lower peak */
        sigma[k] = best;
    }
    free(peak);
}

/* the rules at N = 1024 (513 bins), for tests/test_pv_lock_cpu.py */
void ref_pv_peaks(const float* P, unsigned char* peak) { peaks(P, NAE_FFT_BINS, peak); }
void ref_pv_regions(const float* P, int* sigma) { regions(P, NAE_FFT_BINS, sigma); }

/* formant preservation, steps 1-5: G[0..M] of one frame's analysis spectrum X, lifter q, transposer ratio g */
static void formant_gain(const tables* t, const cf* X, int q, float g, float* G)
{
    const int N = t->N, M = t->M;
    cf* Lc = (cf*)malloc(sizeof(cf) * (M + 1));
    cf* E = (cf*)malloc(sizeof(cf) * (M + 1));
    float* c = (float*)malloc(sizeof(float) * N);
    float* Ls = (float*)malloc(sizeof(float) * (M + 1));
    for (int k = 0; k <= M; k++) {
        const float mag = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
        Lc[k].x = log2f(fmaxf(mag, 0x1p-40f));
        Lc[k].y = 0.0f;
    }
    irfft(t, Lc, c);
    for (int n = 0; n < N; n++)
        if (!(n < q || n > N - q)) c[n] = 0.0f;
    rfft(t, c, E);
    for (int k = 0; k <= M; k++) Ls[k] = E[k].x;
    for (int k = 0; k <= M; k++) {
        const float u = (float)k * g;
        if (u > (float)M) {
            G[k] = 0.0f;
            continue;
        }
        const int i = (int)u;
        const float tt = u - (float)i;
        const float lu = (i == M) ? Ls[M] : Ls[i] + tt * (Ls[i + 1] - Ls[i]);
        G[k] = fminf(exp2f(lu - Ls[k]), NAE_FORMANT_MAX_GAIN);
    }
    free(Lc); free(E); free(c); free(Ls);
}

static void rs_channel(const float* v, size_t M, size_t vstride, const orc_stretch_plan* pl, size_t n_out, const float* tab,
                       float* dst, int ch, int c)
{
    for (size_t j = 0; j < n_out; j++) {
        const unsigned __int128 pos = (unsigned __int128)j * pl->step_q32;
        const int64_t idx = (int64_t)(pos >> 32);
        const uint32_t frac = (uint32_t)pos;
        const uint32_t ph = frac >> 25;
        const float alpha = (float)(frac & 0x1FFFFFFu) * (1.0f / 33554432.0f);
        const float* t0 = tab + ph * NAE_RS_TAPS;
        const float* t1 = t0 + NAE_RS_TAPS;
        float acc = 0.0f;
        for (int i = 0; i < NAE_RS_TAPS; i++) {
            const int64_t m = idx - (NAE_RS_TAPS / 2 - 1) + i;
            const float x = (m >= 0 && (uint64_t)m < M) ? v[(size_t)m * vstride] : 0.0f;
            const float coef = t0[i] + alpha * (t1[i] - t0[i]);
            acc += coef * x;
        }
        dst[j * (size_t)ch + c] = acc;
    }
}


/* rules 1-3: the number of bins of P (this frame) that rise over Pp (the previous frame); a NaN compares false */
static int rising_bins(const float* P, const float* Pp, int BINS, int N)
{
    const float floor_ = NAE_TRANSIENT_FLOOR * (float)N;
    int c = 0;
    for (int k = 0; k < BINS; k++) c += (P[k] > NAE_TRANSIENT_RISE * Pp[k]) && (P[k] > floor_);
    return c;
}

static int is_high(int c, int BINS) { return NAE_TRANSIENT_DEN * c >= NAE_TRANSIENT_NUM * BINS; }


/* rule 4: frame f's verdict from its power P and the previous frame's Pp; *high_prev carries high(f - 1) */
static int onset_at(const float* P, const float* Pp, int BINS, int N, size_t f, int* high_prev)
{
    if (f == 0) return 0;
    const int high = is_high(rising_bins(P, Pp, BINS, N), BINS);
    const int onset = f >= 2 && high && !*high_prev;
    *high_prev = high;
    return onset;
}

/* rule 4 on a sequence of power spectra P[frames][BINS] of a frame size N: on[f] = 1 at an onset */
void ref_pv_onset_rule(const float* P, int frames, int BINS, int N, unsigned char* on)
{
    int high_prev = 0;
    for (int f = 0; f < frames; f++) on[f] = (unsigned char)onset_at(P + (size_t)f * BINS, P + (size_t)(f ? f - 1 : 0) * BINS, BINS, N, (size_t)f, &high_prev);
}

static int stage_on(double rate_eff, int q, double phi) { return q > 0 && fabs(rate_eff / phi - 1.0) >= 1e-6; }

static int plan_forced(const orc_stretch_plan* pl) { return pl->pv_on && pl->tempo_eff == 1.0; }

/* the plan of the formant shift: ref_pv_plan's, with the vocoder stage forced on when the envelope stage runs at tempo 1.
 * -1: an argument that is not valid (phi not finite or <= 0, q outside [0, N / 4]); -2: phi outside [0.25, 4] */
int ref_pv_fs_plan(double rate, double pitch, double phi, int q, int N, size_t in_len, orc_stretch_plan* pl)
{
    if (!size_ok(N)) return -2;
    if (!(rate > 0.0) || !(pitch > 0.0)) return -1;
    if (!isfinite(phi) || !(phi > 0.0) || q < 0 || q > N / 4) return -1;
    if (phi < NAE_FORMANT_SHIFT_MIN || phi > NAE_FORMANT_SHIFT_MAX) return -2;
    const int rc = ref_pv_plan(rate, pitch, N, in_len, pl);
    if (rc) return rc;
    if (pl->pv_on || !stage_on(pl->rate_eff, q, phi)) return 0;
    const int H = N / 4;
    pl->pv_on = 1;                               /* tempo_eff is 1 already: the plan was made without the stage */
    pl->ha_q24 = (int64_t)H << NAE_HA_FRAC_BITS;
    pl->d0 = H;
    pl->r_q24[0] = 1u << NAE_R_FRAC_BITS;
    pl->r_q24[1] = (uint32_t)((((uint64_t)H << NAE_R_FRAC_BITS) + (uint64_t)(H + 1) / 2) / (uint64_t)(H + 1));
    pl->rs_first = pl->rs_on && pl->rate_eff > 1.0;
    if (pl->rs_first) pl->mid_len = (size_t)floor((double)in_len / pl->rate_eff + 0.5);   /* the transposer runs first: mid_len is its output */
    const size_t pv_out = pl->rs_first ? pl->out_len : pl->mid_len;
    pl->frames = (pv_out + N / 2 + H - 1) / H + 1;
    return 0;
}

/* per frame and channel, frame-major with the channel next; each may be NULL: qs [frames][ch][BINS] the synthesis phase, on [frames][ch] the
 * onset verdict the channel acts on (linked: the stream's) whatever `transients` says, sig [frames][ch][BINS] sigma_f as the channel applies
 * it (the identity where no map is taken: unlocked, frame 0 and, with transients, an onset frame), *qdiff the (frame, channel, bin) triples with
 * Qs != Qa (a forced stage: 0) */
typedef struct {
    int32_t* qs;
    unsigned char* on;
    int32_t* sig;
    long long* qdiff;
} pv_taps;

typedef struct {
    const float* src; size_t stride;       /* the channel's input, sample i at src[i * stride] */
    float *P, *Pp, *G;
    cf *X;
    uint32_t *qa, *qa_prev, *qs, *inc;
    int* sigma;
    int high_prev, onset;
    float* v;                              /* the channel's output (Mlen floats), or NULL */
} pv_chan;

static void chan_alloc(pv_chan* c, int BINS)
{
    c->P = (float*)calloc(BINS, sizeof(float));
    c->Pp = (float*)calloc(BINS, sizeof(float));
    c->G = (float*)calloc(BINS, sizeof(float));
    c->X = (cf*)calloc(BINS, sizeof(cf));
    c->qa = (uint32_t*)calloc(BINS, sizeof(uint32_t));
    c->qa_prev = (uint32_t*)calloc(BINS, sizeof(uint32_t));
    c->qs = (uint32_t*)calloc(BINS, sizeof(uint32_t));
    c->inc = (uint32_t*)calloc(BINS, sizeof(uint32_t));
    c->sigma = (int*)calloc(BINS, sizeof(int));
    c->high_prev = c->onset = 0;
}

static void chan_free(pv_chan* c)
{
    free(c->P); free(c->Pp); free(c->G); free(c->X); free(c->qa); free(c->qa_prev); free(c->qs); free(c->inc); free(c->sigma);
}

/* the vocoder stage of one stream: nch channels (1 or 2) of L samples each; cs[c].v[0..Mlen) is overwritten unless it is NULL.  q > 0: formant
 * preservation with ratio g.  link != 0 needs nch == 2.  forced: Y = G X (q > 0 there).  The stream's channels are channels c0 ... of the
 * taps' ch */
static void pv_stream(const tables* t, pv_chan* cs, int nch, size_t L, const orc_stretch_plan* pl, size_t Mlen, int lock, int q, float g,
                      int transients, int forced, int link, const pv_taps* tp, int ch, int c0)
{
    const int N = t->N, H = N / 4, BINS = N / 2 + 1, b = N == 512 ? 9 : N == 1024 ? 10 : N == 2048 ? 11 : 12;
    float* xw = (float*)malloc(sizeof(float) * N);
    float* y = (float*)malloc(sizeof(float) * N);
    float* Pl = (float*)malloc(sizeof(float) * BINS);
    float* Plp = (float*)calloc(BINS, sizeof(float));
    cf* Y = (cf*)malloc(sizeof(cf) * BINS);
    uint32_t* qs_old = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    const double two_pi = 6.283185307179586476925286766559;
    int high_prev_l = 0;
    for (int c = 0; c < nch; c++)
        if (cs[c].v) memset(cs[c].v, 0, Mlen * sizeof(float));
    int64_t s_prev = 0;
    for (size_t f = 0; f < pl->frames; f++) {
        const int64_t s = frame_start(pl, N, (int64_t)f);
        /* analysis and power of every channel */
        for (int c = 0; c < nch; c++) {
            pv_chan* C = &cs[c];
            for (int n = 0; n < N; n++) {
                const int64_t i = s + n;
                const float x = (i >= 0 && (uint64_t)i < L) ? C->src[(size_t)i * C->stride] : 0.0f;
                xw[n] = x * t->hann[n];
            }
            rfft(t, xw, C->X);
            for (int k = 0; k < BINS - 1; k++) C->qa[k] = (uint32_t)orc_atan2_q32(C->X[k].y, C->X[k].x);
            C->qa[BINS - 1] = (C->X[BINS - 1].x < 0.0f) ? 0x80000000u : 0u;
            for (int k = 0; k < BINS; k++) C->P[k] = C->X[k].x * C->X[k].x + C->X[k].y * C->X[k].y;
        }
        /* the decisions: linked, one per stream on Pl; else one per channel on its P */
        if (link) {
            for (int k = 0; k < BINS; k++) Pl[k] = 0.5f * (cs[0].P[k] + cs[1].P[k]);
            cs[0].onset = cs[1].onset = onset_at(Pl, Plp, BINS, N, f, &high_prev_l);
            if (lock) {
                regions(Pl, BINS, cs[0].sigma);
                memcpy(cs[1].sigma, cs[0].sigma, sizeof(int) * BINS);
            }
            memcpy(Plp, Pl, sizeof(float) * BINS);
        } else {
            for (int c = 0; c < nch; c++) {
                pv_chan* C = &cs[c];
                C->onset = onset_at(C->P, C->Pp, BINS, N, f, &C->high_prev);
                if (lock) regions(C->P, BINS, C->sigma);
            }
        }
        /* the recurrence, the taps and the synthesis: per channel */
        for (int c = 0; c < nch; c++) {
            pv_chan* C = &cs[c];
            int mapped = 0;
            if (f == 0 || (transients && C->onset))
                memcpy(C->qs, C->qa, sizeof(uint32_t) * BINS);
            else {
                const int64_t d = s - s_prev;
                const uint32_t R = pl->r_q24[d - pl->d0];
                for (int k = 0; k < BINS; k++) {
                    const uint32_t e = (uint32_t)(((uint64_t)k * (uint64_t)d) & (uint64_t)(N - 1)) << (32 - b);
                    const int32_t dw = (int32_t)(C->qa[k] - C->qa_prev[k] - e);
                    const uint32_t adv = (uint32_t)(((uint64_t)k * (uint64_t)H) & (uint64_t)(N - 1)) << (32 - b);
                    const int64_t scaled = ((int64_t)dw * (int64_t)R + ((int64_t)1 << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
                    C->inc[k] = adv + (uint32_t)scaled;
                }
                if (!lock) {
                    for (int k = 0; k < BINS; k++) C->qs[k] += C->inc[k];
                } else {
                    mapped = 1;
                    memcpy(qs_old, C->qs, sizeof(uint32_t) * BINS);
                    for (int k = 0; k < BINS; k++) {
                        const int p = C->sigma[k];
                        C->qs[k] = qs_old[p] + (C->inc[p] + (C->qa[k] - C->qa[p]));
                    }
                }
            }
            memcpy(C->qa_prev, C->qa, sizeof(uint32_t) * BINS);
            memcpy(C->Pp, C->P, sizeof(float) * BINS);
            const size_t row = f * (size_t)ch + (size_t)(c0 + c);
            if (tp->qs) memcpy(tp->qs + row * BINS, C->qs, sizeof(uint32_t) * BINS);
            if (tp->on) tp->on[row] = (unsigned char)C->onset;
            if (tp->sig)
                for (int k = 0; k < BINS; k++) tp->sig[row * BINS + k] = mapped ? C->sigma[k] : k;
            if (tp->qdiff)
                for (int k = 0; k < BINS; k++) *tp->qdiff += C->qs[k] != C->qa[k];
            if (!C->v) continue;
            if (q > 0) formant_gain(t, C->X, q, g, C->G);
            for (int k = 0; k < BINS; k++) {
                if (forced) {                    /* Qs = Qa: the frame keeps its own phases */
                    Y[k].x = C->G[k] * C->X[k].x;
                    Y[k].y = C->G[k] * C->X[k].y;
                    continue;
                }
                float mag = sqrtf(C->X[k].x * C->X[k].x + C->X[k].y * C->X[k].y);
                if (q > 0) mag = C->G[k] * mag;
                const double ph = two_pi * ((double)(int32_t)C->qs[k] * (1.0 / 4294967296.0));
                Y[k].x = mag * (float)cos(ph);
                Y[k].y = mag * (float)sin(ph);
            }
            irfft(t, Y, y);
            const int64_t o = ((int64_t)f - 1) * H - N / 2;
            for (int n = 0; n < N; n++) {
                const int64_t m = o + n;
                if (m >= 0 && (uint64_t)m < Mlen) C->v[m] += t->hann[n] * y[n];
            }
        }
        s_prev = s;
    }
    for (int c = 0; c < nch; c++)
        if (cs[c].v)
            for (size_t m = 0; m < Mlen; m++) cs[c].v[m] *= NAE_OLA_GAIN;
    free(xw); free(y); free(Pl); free(Plp); free(Y); free(qs_old);
}

/* the whole node at frame size N.  shift = 0: the rules of the _n / _formant entries (ref_pv_plan; the lifter q applies only with both stages
 * on; g = rate_eff; phi unused); shift = 1: those of the _formant_shift entries (ref_pv_fs_plan; q applies with the envelope stage on;
 * g = rate_eff / phi).  The link is effective with two channels, the vocoder stage on and not forced, and the lock or transients on.  A stereo
 * stream runs its channels side by side, linked or not; any other channel count runs channel by channel.  dst (plan.out_len * ch floats) may
 * be NULL when only taps are wanted; the taps (pv_taps; each may be NULL) need the vocoder stage (-1 without it).  -1 / -2 / -3: the codes of
 * the plans; the lock at a size other than 1024 -2; q outside [0, N / 4] -1 */
int ref_pv_run(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, int shift, double phi,
               int link, float* dst, int32_t* qs_tap, unsigned char* on_tap, int32_t* sig_tap, long long* qdiff)
{
    orc_stretch_plan pl;
    const int rc = shift ? ref_pv_fs_plan(rate, pitch, phi, q, N, L, &pl) : ref_pv_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (q < 0 || q > N / 4) return -1;
    if (ch < 1) return -1;
    const pv_taps tp = {qs_tap, on_tap, sig_tap, qdiff};
    if ((qs_tap || on_tap || sig_tap || qdiff) && !pl.pv_on) return -1;
    if (!pl.pv_on && !pl.rs_on) {
        if (dst) memmove(dst, src, L * (size_t)ch * sizeof(float));
        return 0;
    }
    float g;
    if (shift) {
        if (!(pl.pv_on && stage_on(pl.rate_eff, q, phi))) q = 0;
        g = (float)(pl.rate_eff / phi);
    } else {
        if (!(pl.pv_on && pl.rs_on)) q = 0;
        g = (float)pl.rate_eff;
    }
    const int forced = plan_forced(&pl);
    const int link_eff = link && ch == 2 && pl.pv_on && !forced && (lock || transients);
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    if (!pl.pv_on) {
        for (int c = 0; c < ch && dst; c++) rs_channel(src + c, L, (size_t)ch, &pl, pl.out_len, tab, dst, ch, c);
        return 0;
    }
    tables t;
    tables_make(&t, N);
    const int BINS = N / 2 + 1, nch = ch == 2 ? 2 : 1;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    const size_t in_len = pl.rs_first ? pl.mid_len : L;
    const size_t Mlen = pl.rs_first ? pl.out_len : pl.mid_len;
    for (int c0 = 0; c0 < ch; c0 += nch) {
        pv_chan cs[2];
        float* mid[2] = {NULL, NULL};
        for (int i = 0; i < nch; i++) {
            chan_alloc(&cs[i], BINS);
            if (pl.rs_first) {
                mid[i] = (float*)malloc((pl.mid_len + 1) * sizeof(float));
                rs_channel(src + c0 + i, L, (size_t)ch, &pl, pl.mid_len, tab, mid[i], 1, 0);
                cs[i].src = mid[i];
                cs[i].stride = 1;
            } else {
                cs[i].src = src + c0 + i;
                cs[i].stride = (size_t)ch;
            }
            cs[i].v = dst ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
        }
        pv_stream(&t, cs, nch, in_len, &pl, Mlen, lock, q, g, transients, forced, link_eff, &tp, ch, c0);
        for (int i = 0; i < nch; i++) {
            if (dst) {
                if (!pl.rs_first && pl.rs_on) rs_channel(cs[i].v, pl.mid_len, 1, &pl, pl.out_len, tab, dst, ch, c0 + i);
                else
                    for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c0 + i] = cs[i].v[m];
            }
            free(mid[i]);
            free(cs[i].v);
            chan_free(&cs[i]);
        }
    }
    tables_free(&t);
    return 0;
}
