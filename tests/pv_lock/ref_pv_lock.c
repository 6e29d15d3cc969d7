/* ref_pv_lock.c — CPU restatement of the K7 phase vocoder with identity phase locking ("Phase locking").
 *
 * The loops of oracle/orc_stft.c (pv_channel, rs_channel, orc_stretch_f32, orc_pv_synth_phase) restated with a `lock`
 * argument.  lock = 0 is the oracle's vocoder (tests/test_pv_lock_cpu.py pins it bit for bit); lock = 1 replaces the Qs
 * recurrence of frames f >= 1 by the locked one.  The FFTs, the atan2, the Hann window and the transposer's table are the
 * oracle's own (linked from oracle/libnae_oracle.so).  Built by its test with gcc -ffp-contract=off.
 */
#include "../../oracle/nae_oracle.h"
#include "../../include/nae_dsp_spec.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y; } cf;

/* rule 2: peaks of the power spectrum P[0..512]; a neighbour outside 0..512 counts as satisfied, a NaN compares false */
void ref_peaks(const float* P, unsigned char* peak)
{
    for (int k = 0; k < NAE_FFT_BINS; k++) {
        int ok = P[k] > 0.0f;
        if (k >= 1) ok = ok && P[k] > P[k - 1];
        if (k >= 2) ok = ok && P[k] > P[k - 2];
        if (k + 1 < NAE_FFT_BINS) ok = ok && P[k] >= P[k + 1];
        if (k + 2 < NAE_FFT_BINS) ok = ok && P[k] >= P[k + 2];
        peak[k] = (unsigned char)ok;
    }
}

/* rule 3: sigma[k] = the nearest peak, a tie to the lower one; no peak at all: sigma[k] = k.  Returns the number of peaks. */
int ref_regions(const float* P, unsigned short* sigma)
{
    unsigned char peak[NAE_FFT_BINS];
    ref_peaks(P, peak);
    int n = 0;
    for (int k = 0; k < NAE_FFT_BINS; k++) n += peak[k];
    for (int k = 0; k < NAE_FFT_BINS; k++) {
        if (!n) { sigma[k] = (unsigned short)k; continue; }
        int best = -1;
        for (int p = 0; p < NAE_FFT_BINS; p++)
            if (peak[p] && (best < 0 || abs(k - p) < abs(k - best))) best = p;   /* ascending p: a tie keeps the lower peak */
        sigma[k] = (unsigned short)best;
    }
    return n;
}

static inline int64_t frame_start(const orc_stretch_plan* pl, int64_t f)
{
    return (((f - 1) * pl->ha_q24 + ((int64_t)1 << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - NAE_FFT_N / 2;
}

static void pv_channel(const float* src, size_t L, int ch, int c, const orc_stretch_plan* pl, size_t M, float* v,
                       int32_t* qs_tap, size_t tap_stride, int lock)
{
    const float* HANN = orc_hann1024();
    float xw[NAE_FFT_N], y[NAE_FFT_N], P[NAE_FFT_BINS];
    cf X[NAE_FFT_BINS], Y[NAE_FFT_BINS];
    uint32_t qa[NAE_FFT_BINS], qa_prev[NAE_FFT_BINS], qs[NAE_FFT_BINS], qs_old[NAE_FFT_BINS], inc[NAE_FFT_BINS];
    unsigned short sigma[NAE_FFT_BINS];
    const double two_pi = 6.283185307179586476925286766559;
    if (v) memset(v, 0, M * sizeof(float));
    int64_t s_prev = 0;
    for (size_t f = 0; f < pl->frames; f++) {
        const int64_t s = frame_start(pl, (int64_t)f);
        for (int n = 0; n < NAE_FFT_N; n++) {
            const int64_t i = s + n;
            const float x = (i >= 0 && (uint64_t)i < L) ? src[(size_t)i * ch + c] : 0.0f;
            xw[n] = x * HANN[n];
        }
        orc_rfft1024(xw, (float*)X);
        for (int k = 0; k < NAE_FFT_BINS - 1; k++) qa[k] = (uint32_t)orc_atan2_q32(X[k].y, X[k].x);
        qa[NAE_FFT_BINS - 1] = (X[NAE_FFT_BINS - 1].x < 0.0f) ? 0x80000000u : 0u;
        if (f == 0)
            memcpy(qs, qa, sizeof qs);
        else {
            const int64_t d = s - s_prev;
            const uint32_t R = pl->r_q24[d - pl->d0];
            for (int k = 0; k < NAE_FFT_BINS; k++) {
                const uint32_t e = (uint32_t)(((uint64_t)k * (uint64_t)d) & (NAE_FFT_N - 1)) << 22;
                const int32_t dw = (int32_t)(qa[k] - qa_prev[k] - e);
                const uint32_t adv = (uint32_t)((k * NAE_HOP) & (NAE_FFT_N - 1)) << 22;
                const int64_t scaled = ((int64_t)dw * (int64_t)R + ((int64_t)1 << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
                inc[k] = adv + (uint32_t)scaled;
            }
            if (!lock) {
                for (int k = 0; k < NAE_FFT_BINS; k++) qs[k] += inc[k];
            } else {
                for (int k = 0; k < NAE_FFT_BINS; k++) P[k] = X[k].x * X[k].x + X[k].y * X[k].y;
                ref_regions(P, sigma);
                memcpy(qs_old, qs, sizeof qs);
                for (int k = 0; k < NAE_FFT_BINS; k++) {
                    const int p = sigma[k];
                    qs[k] = qs_old[p] + (inc[p] + (qa[k] - qa[p]));
                }
            }
        }
        memcpy(qa_prev, qa, sizeof qa);
        s_prev = s;
        if (qs_tap) memcpy(qs_tap + f * tap_stride, qs, sizeof qs);
        if (!v) continue;
        for (int k = 0; k < NAE_FFT_BINS; k++) {
            const float mag = sqrtf(X[k].x * X[k].x + X[k].y * X[k].y);
            const double ph = two_pi * ((double)(int32_t)qs[k] * (1.0 / 4294967296.0));
            Y[k].x = mag * (float)cos(ph);
            Y[k].y = mag * (float)sin(ph);
        }
        orc_irfft1024((const float*)Y, y);
        const int64_t o = ((int64_t)f - 1) * NAE_HOP - NAE_FFT_N / 2;
        for (int n = 0; n < NAE_FFT_N; n++) {
            const int64_t m = o + n;
            if (m >= 0 && (uint64_t)m < M) v[m] += HANN[n] * y[n];
        }
    }
    if (v)
        for (size_t m = 0; m < M; m++) v[m] *= NAE_OLA_GAIN;
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

/* the whole node; dst holds plan.out_len * ch floats */
int ref_stretch(const float* src, size_t L, int ch, double rate, double pitch, int lock, float* dst)
{
    orc_stretch_plan pl;
    const int rc = orc_stretch_plan_make(rate, pitch, L, &pl);
    if (rc) return rc;
    if (!pl.pv_on && !pl.rs_on) {
        memmove(dst, src, L * (size_t)ch * sizeof(float));
        return 0;
    }
    const float* tab = pl.rs_on ? orc_rs_table(pl.rate_eff) : NULL;
    const size_t vlen = pl.mid_len > pl.out_len ? pl.mid_len : pl.out_len;
    float* v = pl.pv_on ? (float*)malloc((vlen + 1) * sizeof(float)) : NULL;
    float* w = pl.rs_first ? (float*)malloc((pl.out_len + 1) * sizeof(float)) : NULL;
    for (int c = 0; c < ch; c++) {
        if (pl.rs_first) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, v, 1, 0);
            pv_channel(v, pl.mid_len, 1, 0, &pl, pl.out_len, w, NULL, 0, lock);
            for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = w[m];
        } else if (pl.pv_on) {
            pv_channel(src, L, ch, c, &pl, pl.mid_len, v, NULL, 0, lock);
            if (pl.rs_on) rs_channel(v, pl.mid_len, 1, &pl, pl.out_len, tab, dst, ch, c);
            else
                for (size_t m = 0; m < pl.out_len; m++) dst[m * (size_t)ch + c] = v[m];
        } else
            rs_channel(src + c, L, (size_t)ch, &pl, pl.out_len, tab, dst, ch, c);
    }
    free(v);
    free(w);
    return 0;
}

/* synthesis phase of every frame, [frames][ch][513]; with the transposer first its input is the transposed signal */
int ref_pv_synth_phase(const float* src, size_t L, int ch, double rate, double pitch, int lock, int32_t* qs)
{
    orc_stretch_plan pl;
    const int rc = orc_stretch_plan_make(rate, pitch, L, &pl);
    if (rc) return rc;
    if (!pl.pv_on) return -1;
    if (pl.rs_first) {
        const float* tab = orc_rs_table(pl.rate_eff);
        float* v = (float*)malloc((pl.mid_len + 1) * sizeof(float));
        for (int c = 0; c < ch; c++) {
            rs_channel(src + c, L, (size_t)ch, &pl, pl.mid_len, tab, v, 1, 0);
            pv_channel(v, pl.mid_len, 1, 0, &pl, pl.out_len, NULL, qs + (size_t)c * NAE_FFT_BINS, (size_t)ch * NAE_FFT_BINS, lock);
        }
        free(v);
        return 0;
    }
    for (int c = 0; c < ch; c++)
        pv_channel(src, L, ch, c, &pl, pl.mid_len, NULL, qs + (size_t)c * NAE_FFT_BINS, (size_t)ch * NAE_FFT_BINS, lock);
    return 0;
}
