/* ref_pv_tr.c — CPU statement of the K7 phase vocoder with transient preservation ("Transient preservation").
 *
 * It includes the vocoder's statement (tests/pv_ref/ref_pv.c: the tables, the FFTs, the plan, the region rule, the formant gain and the
 * transposer) and restates its pv_channel with the onset rule: with `transients` on, frame f >= 2 is an onset when the count of rising bins
 * crosses NUM/DEN of the bins upwards, and an onset frame takes Qs_f = Qa_f in place of the recurrence, unlocked and locked alike.  With
 * `transients` off it is ref_pv_stretch / ref_pv_synth_phase bit for bit (tests/test_pv_transient_cpu.py).  Built by its tests with gcc
 * -ffp-contract=off against oracle/libnae_oracle.so.
 */
#include "../pv_ref/ref_pv.c"

/* rules 1-3: the number of bins of P (this frame) that rise over Pp (the previous frame); a NaN compares false */
static int rising_bins(const float* P, const float* Pp, int BINS, int N)
{
    const float floor_ = NAE_TRANSIENT_FLOOR * (float)N;
    int c = 0;
    for (int k = 0; k < BINS; k++) c += (P[k] > NAE_TRANSIENT_RISE * Pp[k]) && (P[k] > floor_);
    return c;
}

static int is_high(int c, int BINS) { return NAE_TRANSIENT_DEN * c >= NAE_TRANSIENT_NUM * BINS; }

/* rule 4 on a sequence of power spectra P[frames][BINS] of a frame size N: on[f] = 1 at an onset */
void ref_pv_tr_onset_rule(const float* P, int frames, int BINS, int N, unsigned char* on)
{
    int high_prev = 0;
    for (int f = 0; f < frames; f++) {
        on[f] = 0;
        if (f == 0) continue;
        const int high = is_high(rising_bins(P + (size_t)f * BINS, P + (size_t)(f - 1) * BINS, BINS, N), BINS);
        on[f] = (unsigned char)(f >= 2 && high && !high_prev);
        high_prev = high;
    }
}

/* pv_channel of ref_pv.c with the onset rule (transients != 0); on_tap: every frame's onset verdict at on_tap + f * on_stride, whatever
 * `transients` says */
static void pv_channel_tr(const tables* t, const float* src, size_t L, int ch, int c, const orc_stretch_plan* pl, size_t Mlen, float* v,
                          int lock, int q, float g, int transients, int32_t* qs_tap, size_t tap_stride, unsigned char* on_tap,
                          size_t on_stride)
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
    if (v) memset(v, 0, Mlen * sizeof(float));
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
        if (on_tap) on_tap[f * on_stride] = (unsigned char)onset;
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
        if (qs_tap) memcpy(qs_tap + f * tap_stride, qs, sizeof(uint32_t) * BINS);
        if (!v) continue;
        if (q > 0) formant_gain(t, X, q, g, G);
        for (int k = 0; k < BINS; k++) {
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
    if (v)
        for (size_t m = 0; m < Mlen; m++) v[m] *= NAE_OLA_GAIN;
    free(xw); free(y); free(P); free(Pp); free(G); free(X); free(Y); free(qa); free(qa_prev); free(qs); free(qs_old); free(inc);
    free(sigma);
}

/* ref_pv_stretch with the onset rule (transients: 0 or 1; it only acts where the vocoder runs) */
int ref_pv_tr_stretch(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int q, int transients, float* dst)
{
    orc_stretch_plan pl;
    const int rc = ref_pv_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (q < 0 || q > N / 4) return -1;
    if (!pl.pv_on && !pl.rs_on) {
        memmove(dst, src, L * (size_t)ch * sizeof(float));
        return 0;
    }
    if (!(pl.pv_on && pl.rs_on)) q = 0;
    const float g = (float)pl.rate_eff;
    tables t;
    tables_make(&t, N);
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    float* v = pl.pv_on ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
    float* w = pl.rs_first ? (float*)malloc((pl.out_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, v, 1, 0);
            pv_channel_tr(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, w, lock, q, g, transients, NULL, 0, NULL, 0);
            for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = w[m];
        } else if (pl.pv_on) {
            pv_channel_tr(&t, src, L, ch, c, &pl, pl.mid_len, v, lock, q, g, transients, NULL, 0, NULL, 0);
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

/* synthesis phase of every frame, [frames][ch][N/2 + 1] (qs may be NULL), and the onset verdict of every frame, [frames][ch] (on may be
 * NULL) */
static int synth_phase_tr(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int transients, int32_t* qs,
                          unsigned char* on)
{
    orc_stretch_plan pl;
    const int rc = ref_pv_plan(rate, pitch, N, L, &pl);
    if (rc) return rc;
    if (lock && N != 1024) return -2;
    if (!pl.pv_on) return -1;
    const size_t bins = (size_t)N / 2 + 1;
    tables t;
    tables_make(&t, N);
    float* v = pl.rs_first ? (float*)malloc((pl.mid_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        int32_t* tap = qs ? qs + (size_t)c * bins : NULL;
        unsigned char* otap = on ? on + c : NULL;
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, orc_rs_table(pl.rate_eff), v, 1, 0);
            pv_channel_tr(&t, v, pl.mid_len, 1, 0, &pl, pl.out_len, NULL, lock, 0, 0.0f, transients, tap, (size_t)ch * bins, otap, ch);
        } else
            pv_channel_tr(&t, src, L, ch, c, &pl, pl.mid_len, NULL, lock, 0, 0.0f, transients, tap, (size_t)ch * bins, otap, ch);
    }
    free(v);
    tables_free(&t);
    return 0;
}

/* ref_pv_synth_phase with the onset rule */
int ref_pv_tr_synth_phase(const float* src, size_t L, int ch, double rate, double pitch, int N, int lock, int transients, int32_t* qs)
{
    return synth_phase_tr(src, L, ch, rate, pitch, N, lock, transients, qs, NULL);
}

/* the onset verdict of every (frame, channel), [frames][ch]; it depends on neither the lock nor the flag */
int ref_pv_tr_onsets(const float* src, size_t L, int ch, double rate, double pitch, int N, unsigned char* on)
{
    return synth_phase_tr(src, L, ch, rate, pitch, N, 0, 0, NULL, on);
}
