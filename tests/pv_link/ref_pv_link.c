/* ref_pv_link.c — CPU statement of the K7 phase vocoder with the channel link ("Channel link").
 *
 * It includes the statement with the formant shift (tests/pv_fshift/ref_pv_fs.c, which includes tests/pv_transient/ref_pv_tr.c and
 * tests/pv_ref/ref_pv.c: the tables, the FFTs, the plans, the region rule, the formant gain, the onset rule and the transposer) and restates the
 * loops of pv_channel_tr / pv_channel_fs for the two channels of a stream side by side, with a `link` argument: linked, the onset rule and the
 * lock's peaks and regions read Pl = 0.5f (P^0 + P^1) — one add with channel 0 first, one product — in place of each channel's P, so onset(f)
 * and sigma_f are one decision per stream; Qa, inc, the magnitudes, the formant gain and Qs stay each channel's own.  The link is effective with
 * two channels, the vocoder stage on and not forced, and the lock or transient preservation on; otherwise, and with link = 0, it is
 * ref_pv_tr_stretch / ref_pv_tr_synth_phase (shift = 0) or ref_pv_fs_stretch (shift = 1) bit for bit (tests/test_pv_link_cpu.py).  Built by its
 * tests with gcc -ffp-contract=off against oracle/libnae_oracle.so.
 */
#include "../pv_fshift/ref_pv_fs.c"

typedef struct {
    const float* src; size_t stride;       /* the channel's input, sample i at src[i * stride] */
    float *P, *Pp, *G;
    cf *X;
    uint32_t *qa, *qa_prev, *qs, *inc;
    int* sigma;
    int high_prev, onset;
    float* v;                              /* the channel's output (Mlen floats), or NULL */
} link_chan;

static void chan_alloc(link_chan* c, int BINS)
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

static void chan_free(link_chan* c)
{
    free(c->P); free(c->Pp); free(c->G); free(c->X); free(c->qa); free(c->qa_prev); free(c->qs); free(c->inc); free(c->sigma);
}

/* the vocoder stage of one stream: nch channels (1 or 2) of L samples each.  link != 0 needs nch == 2.  forced: Y = G X (ref_pv_fs.c).
 * Taps (each may be NULL), frame-major with the channel next: qs_tap [frames][nch][BINS], on_tap [frames][nch] (the verdict the channel acts
 * on: linked, the stream's), sig_tap [frames][nch][BINS] (locked: sigma_f as the channel applies it; the identity where no map is taken — frame
 * 0 and, with transients, an onset frame) */
static void pv_stream_link(const tables* t, link_chan* cs, int nch, size_t L, const orc_stretch_plan* pl, size_t Mlen, int lock, int q, float g,
                           int transients, int forced, int link, int32_t* qs_tap, unsigned char* on_tap, int32_t* sig_tap)
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
        /* analysis and power of every channel: rule 1, per channel */
        for (int c = 0; c < nch; c++) {
            link_chan* C = &cs[c];
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
            int onset = 0;
            if (f >= 1) {
                const int high = is_high(rising_bins(Pl, Plp, BINS, N), BINS);
                onset = f >= 2 && high && !high_prev_l;
                high_prev_l = high;
            }
            cs[0].onset = cs[1].onset = onset;
            if (lock) {
                regions(Pl, BINS, cs[0].sigma);
                memcpy(cs[1].sigma, cs[0].sigma, sizeof(int) * BINS);
            }
            memcpy(Plp, Pl, sizeof(float) * BINS);
        } else {
            for (int c = 0; c < nch; c++) {
                link_chan* C = &cs[c];
                C->onset = 0;
                if (f >= 1) {
                    const int high = is_high(rising_bins(C->P, C->Pp, BINS, N), BINS);
                    C->onset = f >= 2 && high && !C->high_prev;
                    C->high_prev = high;
                }
                if (lock) regions(C->P, BINS, C->sigma);
            }
        }
        /* the recurrence, the taps and the synthesis: per channel */
        for (int c = 0; c < nch; c++) {
            link_chan* C = &cs[c];
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
            if (qs_tap) memcpy(qs_tap + (f * nch + c) * (size_t)BINS, C->qs, sizeof(uint32_t) * BINS);
            if (on_tap) on_tap[f * nch + c] = (unsigned char)C->onset;
            if (sig_tap)
                for (int k = 0; k < BINS; k++) sig_tap[(f * nch + c) * (size_t)BINS + k] = mapped ? C->sigma[k] : k;
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

/* the whole node.  shift = 0: the _n / _formant entries (ref_pv_tr_stretch's rules; phi unused); shift = 1: the _formant_shift entries
 * (ref_pv_fs_stretch's).  dst (plan.out_len * ch floats) may be NULL when only taps are wanted; taps as pv_stream_link, and only with the vocoder
 * stage on (-1 without it).  -1 / -2: the codes of the plans; the lock at a size other than 1024 -2, with or without the link */
static int link_run(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, int shift, double phi,
                    int link, float* dst, int32_t* qs_tap, unsigned char* on_tap, int32_t* sig_tap)
{
    orc_stretch_plan pl;
    const int rc = shift ? ref_pv_fs_plan(rate, pitch, phi, q, N, L, &pl) : ref_pv_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (q < 0 || q > N / 4) return -1;
    if (ch < 1 || ch > 2) return -1;
    const int taps = qs_tap || on_tap || sig_tap;
    if (taps && !pl.pv_on) return -1;
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
    /* rule 4: when the link is effective */
    const int link_eff = link && ch == 2 && pl.pv_on && !forced && (lock || transients);
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    if (!pl.pv_on) {
        for (int c = 0; c < ch && dst; c++) rs_channel(src + c, L, (size_t)ch, &pl, pl.out_len, tab, dst, ch, c);
        return 0;
    }
    tables t;
    tables_make(&t, N);
    const int BINS = N / 2 + 1;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    link_chan cs[2];
    float* mid[2] = {NULL, NULL};
    float* out[2] = {NULL, NULL};
    for (int c = 0; c < ch; c++) {
        chan_alloc(&cs[c], BINS);
        if (pl.rs_first) {
            mid[c] = (float*)malloc((pl.mid_len + 1) * sizeof(float));
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, mid[c], 1, 0);
            cs[c].src = mid[c];
            cs[c].stride = 1;
        } else {
            cs[c].src = src + c;
            cs[c].stride = (size_t)ch;
        }
        out[c] = dst ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
        cs[c].v = out[c];
    }
    const size_t in_len = pl.rs_first ? pl.mid_len : L;
    const size_t Mlen = pl.rs_first ? pl.out_len : pl.mid_len;
    pv_stream_link(&t, cs, ch, in_len, &pl, Mlen, lock, q, g, transients, forced, link_eff, qs_tap, on_tap, sig_tap);
    for (int c = 0; c < ch; c++) {
        if (dst) {
            if (!pl.rs_first && pl.rs_on) rs_channel(out[c], pl.mid_len, 1, &pl, pl.out_len, tab, dst, ch, c);
            else
                for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = out[c][m];
        }
        free(mid[c]);
        free(out[c]);
        chan_free(&cs[c]);
    }
    tables_free(&t);
    return 0;
}

/* ref_pv_tr_stretch with the link (shift = 0) / ref_pv_fs_stretch with it (shift = 1) */
int ref_pv_link_stretch(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, int shift,
                        double phi, int link, float* dst)
{
    return link_run(src, L, ch, rate, pitch, N, lock, q, transients, shift, phi, link, dst, NULL, NULL, NULL);
}

/* per frame and channel: the synthesis phase qs [frames][ch][N/2 + 1], the onset verdict on [frames][ch] and, locked, sigma sig
 * [frames][ch][N/2 + 1]; each may be NULL */
int ref_pv_link_taps(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int transients, int link, int32_t* qs,
                     unsigned char* on, int32_t* sig)
{
    return link_run(src, L, ch, rate, pitch, N, lock, 0, transients, 0, 1.0, link, NULL, qs, on, sig);
}
