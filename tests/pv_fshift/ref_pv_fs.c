/* ref_pv_fs.c — CPU statement of the K7 phase vocoder with the formant shift ("Formant shift").
 *
 * It includes the statement with transient preservation (tests/pv_transient/ref_pv_tr.c, which includes tests/pv_ref/ref_pv.c: the tables, the
 * FFTs, the plan, the region rule, the formant gain, the onset rule and the transposer) and restates its loops with two parameters: the ratio
 * g = (float)(rate_eff / phi) of the gain rule, and the forced plan — the vocoder stage on at tempo 1 (ha = H, d0 = H, r = 2^24) where the envelope
 * stage runs without a tempo change.  The envelope stage runs when q > 0 and |rate_eff / phi - 1| >= 1e-6.  A frame of the forced stage is
 * Y = G X; its phase recurrence is still walked (unlocked, locked, with onset resets), and ref_pv_fs_forced_phase_diff counts the bins where it
 * leaves Qs != Qa: none.  With phi = 1 and a plan that is not forced it is ref_pv_tr_stretch bit for bit (tests/test_pv_fshift_cpu.py).  Built
 * by its tests with gcc -ffp-contract=off against oracle/libnae_oracle.so.
 */
#include "../pv_transient/ref_pv_tr.c"

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

/* pv_channel_tr of ref_pv_tr.c with the forced stage: forced != 0 takes Y = G X (q > 0 there) and counts in *qdiff the (frame, bin) pairs whose
 * synthesis phase differs from the analysis phase */
static void pv_channel_fs(const tables* t, const float* src, size_t L, int ch, int c, const orc_stretch_plan* pl, size_t Mlen, float* v, int lock,
                          int q, float g, int transients, int forced, size_t* qdiff)
{
    const int N = t->N, H = N / 4, BINS = N / 2 + 1, b = N == 512 ? 9 : N == 1024 ? 10 : N == 2048 ? 11 : 12;
    float* xw = (float*)malloc(sizeof(float) * N);
    float* y = (float*)malloc(sizeof(float) * N);
    float* P = (float*)malloc(sizeof(float) * BINS);
    float* Pp = (float*)malloc(sizeof(float) * BINS);
    float* G = (float*)malloc(sizeof(float) * BINS);
    cf* X = (cf*)malloc(sizeof(cf) * BINS);
    cf* Y = (cf*)malloc(sizeof(cf) * BINS);
    uint32_t* qa = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qa_prev = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qs = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* qs_old = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    uint32_t* inc = (uint32_t*)malloc(sizeof(uint32_t) * BINS);
    int* sigma = (int*)malloc(sizeof(int) * BINS);
    const double two_pi = 6.283185307179586476925286766559;
    memset(v, 0, Mlen * sizeof(float));
    int64_t s_prev = 0;
    int high_prev = 0;
    for (size_t f = 0; f < pl->frames; f++) {
        const int64_t s = frame_start(pl, N, (int64_t)f);
        for (int n = 0; n < N; n++) {
            const int64_t i = s + n;
            const float x = (i >= 0 && (uint64_t)i < L) ? src[(size_t)i * ch + c] : 0.0f;
            xw[n] = x * t->hann[n];
        }
        rfft(t, xw, X);
        for (int k = 0; k < BINS - 1; k++) qa[k] = (uint32_t)orc_atan2_q32(X[k].y, X[k].x);
        qa[BINS - 1] = (X[BINS - 1].x < 0.0f) ? 0x80000000u : 0u;
        for (int k = 0; k < BINS; k++) P[k] = X[k].x * X[k].x + X[k].y * X[k].y;
        int onset = 0;
        if (f >= 1) {
            const int high = is_high(rising_bins(P, Pp, BINS, N), BINS);
            onset = f >= 2 && high && !high_prev;
            high_prev = high;
        }
        if (f == 0 || (transients && onset))
            memcpy(qs, qa, sizeof(uint32_t) * BINS);
        else {
            const int64_t d = s - s_prev;
            const uint32_t R = pl->r_q24[d - pl->d0];
            for (int k = 0; k < BINS; k++) {
                const uint32_t e = (uint32_t)(((uint64_t)k * (uint64_t)d) & (uint64_t)(N - 1)) << (32 - b);
                const int32_t dw = (int32_t)(qa[k] - qa_prev[k] - e);
                const uint32_t adv = (uint32_t)(((uint64_t)k * (uint64_t)H) & (uint64_t)(N - 1)) << (32 - b);
                const int64_t scaled = ((int64_t)dw * (int64_t)R + ((int64_t)1 << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
                inc[k] = adv + (uint32_t)scaled;
            }
            if (!lock) {
                for (int k = 0; k < BINS; k++) qs[k] += inc[k];
            } else {
                regions(P, BINS, sigma);
                memcpy(qs_old, qs, sizeof(uint32_t) * BINS);
                for (int k = 0; k < BINS; k++) {
                    const int p = sigma[k];
                    qs[k] = qs_old[p] + (inc[p] + (qa[k] - qa[p]));
                }
            }
        }
        memcpy(qa_prev, qa, sizeof(uint32_t) * BINS);
        memcpy(Pp, P, sizeof(float) * BINS);
        s_prev = s;
        if (qdiff)
            for (int k = 0; k < BINS; k++) *qdiff += qs[k] != qa[k];
        if (q > 0) formant_gain(t, X, q, g, G);
        for (int k = 0; k < BINS; k++) {
            if (forced) {                        /* Qs = Qa: the frame keeps its own phases */
                Y[k].x = G[k] * X[k].x;
                Y[k].y = G[k] * X[k].y;
                continue;
            }
            float mag = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
            if (q > 0) mag = G[k] * mag;
            const double ph = two_pi * ((double)(int32_t)qs[k] * (1.0 / 4294967296.0));
            Y[k].x = mag * (float)cos(ph);
            Y[k].y = mag * (float)sin(ph);
        }
        irfft(t, Y, y);
        const int64_t o = ((int64_t)f - 1) * H - N / 2;
        for (int n = 0; n < N; n++) {
            const int64_t m = o + n;
            if (m >= 0 && (uint64_t)m < Mlen) v[m] += t->hann[n] * y[n];
        }
    }
    for (size_t m = 0; m < Mlen; m++) v[m] *= NAE_OLA_GAIN;
    free(xw); free(y); free(P); free(Pp); free(G); free(X); free(Y); free(qa); free(qa_prev); free(qs); free(qs_old); free(inc);
    free(sigma);
}

static int stretch_fs(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, double phi,
                      float* dst, size_t* qdiff)
{
    orc_stretch_plan pl;
    const int rc = ref_pv_fs_plan(rate, pitch, phi, q, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (!pl.pv_on && !pl.rs_on) {
        memmove(dst, src, L * (size_t)ch * sizeof(float));
        return 0;
    }
    if (!(pl.pv_on && stage_on(pl.rate_eff, q, phi))) q = 0;
    const float g = (float)(pl.rate_eff / phi);
    const int forced = plan_forced(&pl);
    tables t;
    tables_make(&t, N);
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    float* v = pl.pv_on ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
    float* w = pl.rs_first ? (float*)malloc((pl.out_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, v, 1, 0);
            pv_channel_fs(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, w, lock, q, g, transients, forced, qdiff);
            for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = w[m];
        } else if (pl.pv_on) {
            pv_channel_fs(&t, src, L, ch, c, &pl, pl.mid_len, v, lock, q, g, transients, forced, qdiff);
            if (pl.rs_on) rs_channel(v, pl.mid_len, 1, &pl, pl.out_len, tab, dst, ch, c);
            else
                for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = v[m];
        } else
            rs_channel(src + c, L, (size_t)ch, &pl, pl.out_len, tab, dst, ch, c);
    }
    free(v);
    free(w);
    tables_free(&t);
    return 0;
}

/* the whole node with the formant shift phi and lifter q; dst holds plan.out_len * ch floats */
int ref_pv_fs_stretch(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, double phi, float* dst)
{
    return stretch_fs(src, L, ch, rate, pitch, N, lock, q, transients, phi, dst, NULL);
}

/* the (frame, bin) pairs of the vocoder stage whose synthesis phase differs from the analysis phase (a forced stage: 0); -1 without the stage */
long long ref_pv_fs_forced_phase_diff(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients,
                                      double phi)
{
    orc_stretch_plan pl;
    if (ref_pv_fs_plan(rate, pitch, phi, q, N, L, &pl) || !pl.pv_on) return -1;
    float* dst = (float*)malloc((pl.out_len + 1) * (size_t)ch * sizeof(float));
    size_t n = 0;
    const int rc = stretch_fs(src, L, ch, rate, pitch, N, lock, q, transients, phi, dst, &n);
    free(dst);
    return rc ? -1 : (long long)n;
}
