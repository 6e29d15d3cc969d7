// nae_stream.hip — SoundTouch-shaped and spectrum streaming handles on top of the block kernels.
//
// nae_stretch mirrors the calls soundtouch_process_payload makes (/root/reference/src/processor/
// audio-velocity.cpp:369-428): putSamples / numSamples / receiveSamples / flush.
#include "nae_internal.h"
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stream_util.h"

struct nae_stretch {
    nae_ctx* ctx;
    int sample_rate, ch;
    double rate, pitch;
    nae_pv_opts opts;             // what the nae_stretch_create* entry asked for
    nae_stretch_plan pl{};        // parameters (in_len = 0)
    nae_pv_run run{};             // the options as this plan runs them (none of it depends on in_len)
    DevFifo in;                   // interleaved input, sample-frames
    // phase vocoder
    size_t blocks_done = 0;       // hop blocks produced == frames folded into the carried phase
    uint32_t* carry[2] = {nullptr, nullptr};
    int carry_cur = 0;
    DevFifo mid;                  // between the stages: planar when the vocoder runs first, else interleaved
    // output
    DevFifo out;                  // interleaved result, sample-frames
    size_t out_read = 0;
    bool flushed = false;
};

struct nae_spectrum {
    nae_ctx* ctx;
    int ch;
    int n_fft = NAE_FFT_N, hop = NAE_HOP;
    DevFifo pending;               // interleaved samples, from the first one the next frame needs
    DevFifo out;                   // frames of [ch][n_fft/2 + 1]
    size_t out_read = 0;           // frames handed out
};

// the FIR filter's handle ("K9 FIR filter"): whole blocks of n_fft / 2 samples are filtered as they become available
struct nae_fir {
    nae_ctx* ctx;
    int ch, n_fft, n_taps;
    float* d_spec = nullptr;       // the padded taps and their spectrum H (nae_fir_make_spec)
    DevFifo in;                    // interleaved input, from the half block in front of the next block on
    DevFifo out;                   // interleaved result
    size_t blocks_done = 0, out_read = 0;
    bool flushed = false;
};

// the long convolution's handle ("K10 long convolution"): nae_fir's, with the ring of spectra kept between puts
struct nae_conv {
    nae_ctx* ctx;
    int ch, n_fft, n_taps, taps_ch, parts;
    float* d_spec = nullptr;       // the padded taps and their spectra H (nae_conv_make_spec)
    float* d_ring = nullptr;       // [ch][ring] spectra: the last parts - 1 blocks stay in it between puts
    size_t ring = 0;
    DevFifo in;                    // interleaved input, from the half block in front of the next block on
    DevFifo out;                   // interleaved result
    size_t blocks_done = 0, out_read = 0;
    bool flushed = false;
};

// the biquad cascade's handle ("K11 biquad cascade"): whole chunks of NAE_EQ_CHUNK samples are filtered as they fill; the sections'
// carry between two launches stays on the device
struct nae_eq {
    nae_ctx* ctx;
    int ch, n_sections;
    double* d_block = nullptr;     // coefficients and tables (nae_eq_make_block)
    double* d_state = nullptr;     // [ch][NAE_EQ_MAX_SECTIONS][2]: every section's (z1, z2) behind the last chunk done
    DevFifo in;                    // interleaved input, from the first sample of the next chunk on
    DevFifo out;                   // interleaved result
    size_t chunks_done = 0, out_read = 0;
    bool flushed = false;
};

// the dynamics processor's handle ("K12 dynamics"): whole chunks of NAE_DYN_CHUNK samples are computed once the `lookahead` samples
// behind them are there; the detectors' carries between two launches stay on the device
struct nae_dyn {
    nae_ctx* ctx;
    int ch;
    nae_dyn_params params;
    double* d_state = nullptr;     // [detector][2]: (y1, yl) behind the last chunk done
    DevFifo in;                    // interleaved input, from the first sample of the next chunk on
    DevFifo out;                   // interleaved result
    size_t chunks_done = 0, out_read = 0;
    bool flushed = false;
};

namespace {

// the chunks that became computable: every whole chunk whose look-ahead is complete, and after the flush all the rest
int dyn_process(nae_dyn* h)
{
    nae_ctx* ctx = h->ctx;
    const size_t C = NAE_DYN_CHUNK, la = (size_t)h->params.lookahead;
    const size_t chunks = h->flushed ? (h->in.total + C - 1) / C : (h->in.total >= la ? (h->in.total - la) / C : 0);
    if (chunks <= h->chunks_done) return NAE_OK;
    const size_t produced = h->flushed ? h->in.total : chunks * C;
    int rc = h->out.reserve(ctx, produced);
    if (rc) return rc;
    const nae_sig src = h->in.view(), dst = h->out.view();
    rc = nae_launch_dyn(ctx, &h->params, &src, h->in.total, h->ch, 1, &dst, h->chunks_done, chunks, h->d_state);
    if (rc) return rc;
    h->out.total = produced;
    h->chunks_done = chunks;
    h->in.drop((long long)(chunks * C));
    return NAE_OK;
}

// the chunks that became computable: every whole chunk, and after the flush the partial one at the end
int eq_process(nae_eq* h)
{
    nae_ctx* ctx = h->ctx;
    const size_t C = NAE_EQ_CHUNK;
    const size_t chunks = h->flushed ? (h->in.total + C - 1) / C : h->in.total / C;
    if (chunks <= h->chunks_done) return NAE_OK;
    const size_t produced = h->flushed ? h->in.total : chunks * C;
    int rc = h->out.reserve(ctx, produced);
    if (rc) return rc;
    const nae_sig src = h->in.view(), dst = h->out.view();
    rc = nae_launch_eq(ctx, h->d_block, h->n_sections, &src, h->in.total, h->ch, 1, &dst, h->chunks_done, chunks, h->d_state);
    if (rc) return rc;
    h->out.total = produced;
    h->chunks_done = chunks;
    h->in.drop((long long)(chunks * C));
    return NAE_OK;
}

int conv_process(nae_conv* h)
{
    nae_ctx* ctx = h->ctx;
    const size_t B = (size_t)h->n_fft / 2;
    const size_t blocks = h->flushed ? (h->in.total + B - 1) / B : h->in.total / B;
    if (blocks <= h->blocks_done) return NAE_OK;
    const size_t produced = h->flushed ? h->in.total : blocks * B;
    int rc = h->out.reserve(ctx, produced);
    if (rc) return rc;
    const nae_sig src = h->in.view(), dst = h->out.view();
    rc = nae_launch_conv(ctx, h->n_fft, h->parts, h->taps_ch, h->d_spec, h->d_ring, h->ring, &src, h->in.total, h->ch, 1, &dst, h->blocks_done, blocks);
    if (rc) return rc;
    h->out.total = produced;
    h->blocks_done = blocks;
    h->in.drop((long long)((blocks - 1) * B));       // the next block's first half
    return NAE_OK;
}

// the blocks that became computable: every whole block, and after the flush the partial one at the end
int fir_process(nae_fir* h)
{
    nae_ctx* ctx = h->ctx;
    const size_t B = (size_t)h->n_fft / 2;
    const size_t blocks = h->flushed ? (h->in.total + B - 1) / B : h->in.total / B;
    if (blocks <= h->blocks_done) return NAE_OK;
    const size_t produced = h->flushed ? h->in.total : blocks * B;
    int rc = h->out.reserve(ctx, produced);
    if (rc) return rc;
    const nae_sig src = h->in.view(), dst = h->out.view();
    rc = nae_launch_fir(ctx, h->n_fft, h->d_spec, &src, h->in.total, h->ch, 1, &dst, h->blocks_done, blocks);
    if (rc) return rc;
    h->out.total = produced;
    h->blocks_done = blocks;
    h->in.drop((long long)((blocks - 1) * B));       // the next block's first half
    return NAE_OK;
}

inline long long frame_start_host(const nae_stretch_plan& pl, int n_fft, long long f)
{
    return (((f - 1) * pl.ha_q24 + (1ll << (NAE_HA_FRAC_BITS - 1))) >> NAE_HA_FRAC_BITS) - n_fft / 2;
}

// number of leading frames whose n_fft-sample window lies inside [.., in_total)
size_t frames_available(const nae_stretch_plan& pl, int n_fft, size_t in_total)
{
    if (in_total < (size_t)n_fft / 2) return 0;
    // estimate, then correct with the exact start formula
    long long f = (long long)(((double)in_total - 0.5 * n_fft) / ((double)pl.ha_q24 / (double)(1 << NAE_HA_FRAC_BITS))) + 2;
    if (f < 0) f = 0;
    while (f > 0 && frame_start_host(pl, n_fft, f - 1) + n_fft > (long long)in_total) f--;
    while (frame_start_host(pl, n_fft, f) + n_fft <= (long long)in_total) f++;
    return (size_t)f;
}

// the vocoder stage over the hop blocks [blocks_done, B_r) of `src` (absolute indexing, src_len samples-frames stored) into `dst`: frames >= F_r
// are not available, samples >= limit are not stored.  Carries the phase on and advances blocks_done.
int stretch_pv_stage(nae_stretch* h, const nae_stretch_plan& pl, const nae_sig& src, size_t src_len, size_t F_r, size_t B_r, long long limit,
                     const nae_sig& dst)
{
    nae_ctx* ctx = h->ctx;
    const int ch = h->ch;
    const size_t count = B_r - h->blocks_done;
    // a short segment (what a node's batch of waiting frames gives) is ONE tile run frame-interleaved — four consecutive
    // frames per step — and the pipeline itself hands the phase on: one launch instead of pass 1 + scan + pass 3.
    // Long segments (a whole file in one put) are cut into 64-frame tiles that run side by side.
    const bool one_tile = ctx->pv_tile <= 0 && count <= 256;
    const int tile = one_tile ? (int)count : (ctx->pv_tile > 0 ? ctx->pv_tile : 64);
    const int fps = one_tile ? 4 : 1;
    const bool forced = h->run.forced;            // the envelope pass: no phase workspace and nothing carried
    int rc = nae_pv_reserve_ws(ctx, h->run, count, ch, 1, tile);
    if (rc) return rc;
    for (int i = 0; i < 2 && !forced; i++)
        if (!h->carry[i] && hipMalloc((void**)&h->carry[i], (size_t)ch * nae_pv_record_pad(h->opts.n_fft) * sizeof(uint32_t)) != hipSuccess)
            return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(carry)");
    const nae_pv_segment seg{(long long)h->blocks_done, (long long)count, (long long)F_r, limit,
                             h->blocks_done && !forced ? h->carry[h->carry_cur] : nullptr, h->carry[h->carry_cur ^ 1], one_tile};
    rc = nae_launch_pv_phase(ctx, h->run, &pl, &src, src_len, ch, 1, tile, tile, static_cast<uint32_t*>(ctx->ws_phase), &seg);
    if (rc) return rc;
    rc = nae_launch_pv_synth(ctx, h->run, &pl, &src, src_len, ch, 1, tile, tile, static_cast<uint32_t*>(ctx->ws_phase), &dst, &seg, fps);
    if (rc) return rc;
    h->carry_cur ^= 1;
    h->blocks_done = B_r;
    return NAE_OK;
}

// frames in front of a segment that its passes re-analyse: 1, or 2 with transient preservation (onset(f) reads frames f - 2 .. f)
inline long long prime_frames(const nae_stretch* h) { return h->run.transients ? 2 : 1; }

int stretch_process(nae_stretch* h)
{
    nae_ctx* ctx = h->ctx;
    const int ch = h->ch;
    const nae_stretch_plan& pl = h->pl;
    const int n_fft = h->opts.n_fft;
    const size_t hop = (size_t)n_fft / 4;        // hop blocks of the vocoder stage
    DevFifo &in = h->in, &mid = h->mid, &out = h->out;
    nae_stretch_plan fin{};
    if (const int rc = h->flushed ? nae_pv_plan_make(ctx, h->opts, h->rate, h->pitch, in.total, &fin) : NAE_OK) return rc;
    // ---- neither stage: the node is a wire (a formant shift at tempo 1 has the vocoder stage forced on and does not come here)
    if (!pl.pv_on && !pl.rs_on) {
        if (in.total == out.total) return NAE_OK;
        const int rc = out.push(ctx, in.at(out.total), in.total - out.total, false);
        if (!rc) in.drop((long long)in.total);
        return rc;
    }
    // ---- transposer first (rate_eff > 1): in -> [RS] -> mid (interleaved FIFO) -> [PV] -> out
    if (pl.rs_first) {
        size_t J_r;
        if (h->flushed) J_r = fin.mid_len;
        else if (in.total <= NAE_RS_TAPS / 2) J_r = 0;
        else {
            const unsigned __int128 lim = ((unsigned __int128)(in.total - NAE_RS_TAPS / 2) << 32) - 1;
            J_r = (size_t)(lim / pl.step_q32) + 1;
        }
        if (J_r > mid.total) {
            int rc = nae_ensure_rs_table(ctx, pl.rate_eff);
            if (!rc) rc = mid.reserve(ctx, J_r);
            if (rc) return rc;
            const nae_sig src = in.view(), dst = mid.view();
            rc = nae_launch_resample(ctx, &pl, &src, in.total, ch, 1, ctx->d_rs_tab, &dst, mid.total, J_r);
            if (rc) return rc;
            mid.total = J_r;
            const unsigned __int128 pos = (unsigned __int128)J_r * pl.step_q32;
            in.drop(((long long)(pos >> 32) - (NAE_RS_TAPS / 2 - 1)) & ~3ll);
        }
        size_t F_r, B_r;
        long long out_limit;
        if (h->flushed) {
            F_r = fin.frames;
            B_r = (fin.out_len + hop - 1) / hop;
            out_limit = (long long)fin.out_len;
        } else {
            F_r = frames_available(pl, n_fft, mid.total);
            B_r = F_r >= 3 ? F_r - 3 : 0;
            out_limit = (long long)1 << 60;
        }
        if (B_r > h->blocks_done) {
            const size_t produced_total = h->flushed ? fin.out_len : B_r * hop;
            int rc = out.reserve(ctx, produced_total);
            if (rc) return rc;
            rc = stretch_pv_stage(h, pl, mid.view(), mid.total, F_r, B_r, out_limit, out.view());
            if (rc) return rc;
            out.total = produced_total;
            mid.drop(frame_start_host(pl, n_fft, (long long)B_r - prime_frames(h)));
        }
        return NAE_OK;
    }
    // ---- vocoder first: in -> [PV] -> mid (planar FIFO) -> [RS] -> out
    // ---- stage 1: phase vocoder over the hop blocks that became computable
    if (pl.pv_on) {
        size_t F_r, B_r;
        long long mid_limit;
        if (h->flushed) {
            F_r = fin.frames;
            B_r = (fin.mid_len + hop - 1) / hop;
            mid_limit = (long long)fin.mid_len;
        } else {
            F_r = frames_available(pl, n_fft, in.total);
            B_r = F_r >= 3 ? F_r - 3 : 0;
            mid_limit = (long long)1 << 60;
        }
        if (B_r > h->blocks_done) {
            size_t produced_total = h->flushed ? fin.mid_len : B_r * hop;
            DevFifo& dst = pl.rs_on ? mid : out;
            if (!pl.rs_on && h->flushed) {
                if (produced_total > fin.out_len) produced_total = fin.out_len;
                mid_limit = (long long)fin.out_len;
            }
            int rc = dst.reserve(ctx, produced_total);
            if (rc) return rc;
            rc = stretch_pv_stage(h, pl, in.view(), in.total, F_r, B_r, mid_limit, dst.view());
            if (rc) return rc;
            dst.total = produced_total;
            // input still needed: from the start of frame B_r - 1 (it primes the next call's phase difference; with transients also
            // frame B_r - 2, which primes its onset rule)
            in.drop(frame_start_host(pl, n_fft, (long long)B_r - prime_frames(h)));
        }
    }
    // ---- stage 2: rate transposer over the outputs whose 16 taps are known
    if (pl.rs_on) {
        DevFifo& src = pl.pv_on ? mid : in;
        size_t J_r;
        if (h->flushed) J_r = fin.out_len;
        else if (src.total <= NAE_RS_TAPS / 2) J_r = 0;
        else {
            const unsigned __int128 lim = ((unsigned __int128)(src.total - NAE_RS_TAPS / 2) << 32) - 1;
            J_r = (size_t)(lim / pl.step_q32) + 1;
        }
        if (J_r > out.total) {
            int rc = nae_ensure_rs_table(ctx, pl.rate_eff);
            if (!rc) rc = out.reserve(ctx, J_r);
            if (rc) return rc;
            const nae_sig sv = src.view(), dv = out.view();
            const size_t src_len = h->flushed && pl.pv_on ? fin.mid_len : src.total;
            rc = nae_launch_resample(ctx, &pl, &sv, src_len, ch, 1, ctx->d_rs_tab, &dv, out.total, J_r);
            if (rc) return rc;
            out.total = J_r;
            // source still needed: from idx(J_r) - 7, rounded DOWN to a multiple of 4 samples as the tiled kernel stages it
            const unsigned __int128 pos = (unsigned __int128)J_r * pl.step_q32;
            src.drop(((long long)(pos >> 32) - (NAE_RS_TAPS / 2 - 1)) & ~3ll);
        }
    }
    return NAE_OK;
}

} // namespace

extern "C" {

static int stretch_create(nae_ctx* ctx, const nae_pv_opts& o, int sample_rate, int channels, float rate, float pitch, nae_stretch** h)
{
    (void)nae_use_device(ctx);
    *h = nullptr;
    // audio-velocity.cpp:371-379 rejects rates outside 8..48 kHz for SoundTouch; the vocoder has no such
    // limit, but the drop-in keeps the reference's envelope (lift it with sample_rate = 0).
    if (sample_rate != 0 && (sample_rate < 8000 || sample_rate > 48000)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "Unsupported sample rate: requires 8000..48000 Hz");
    if (channels != 1 && channels != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    nae_stretch_plan pl;
    if (const int rc = nae_pv_plan_make(ctx, o, rate, pitch, 0, &pl)) return rc;
    nae_stretch* s = new (std::nothrow) nae_stretch();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->sample_rate = sample_rate;
    s->ch = channels;
    s->rate = rate;
    s->pitch = pitch;
    s->opts = o;
    s->pl = pl;
    s->run = nae_pv_resolve(o, pl, channels);
    s->in.width = s->mid.width = s->out.width = (size_t)channels;
    s->mid.planar = !pl.rs_first;
    *h = s;
    return NAE_OK;
}

// the create entries: a null handle pointer NAE_ERR_INVALID first, the options checked into a record (nae_pv_opts_check), then the one implementation
int nae_stretch_create(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, nae_stretch** h)
{
    return nae_stretch_create_ex(ctx, sample_rate, channels, rate, pitch, 0u, h);
}

int nae_stretch_create_ex(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, nae_stretch** h)
{
    nae_pv_opts o;
    const int rc = h ? nae_pv_opts_check(ctx, flags, NAE_STRETCH_PHASE_LOCK, NAE_FFT_N, 0, nullptr, &o) : NAE_ERR_INVALID;
    return rc ? rc : stretch_create(ctx, o, sample_rate, channels, rate, pitch, h);
}

int nae_stretch_create_n(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, int n_fft, nae_stretch** h)
{
    return nae_stretch_create_formant(ctx, sample_rate, channels, rate, pitch, flags, n_fft, 0, h);
}

int nae_stretch_create_formant(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, int n_fft, int lifter,
                               nae_stretch** h)
{
    nae_pv_opts o;
    const int rc = h ? nae_pv_opts_check(ctx, flags, kPvFlagsN, n_fft, lifter, nullptr, &o) : NAE_ERR_INVALID;
    return rc ? rc : stretch_create(ctx, o, sample_rate, channels, rate, pitch, h);
}

int nae_stretch_create_formant_shift(nae_ctx* ctx, int sample_rate, int channels, float rate, float pitch, unsigned flags, int n_fft, int lifter,
                                     double formant_ratio, nae_stretch** h)
{
    nae_pv_opts o;
    const int rc = h ? nae_pv_opts_check(ctx, flags, kPvFlagsN, n_fft, lifter, &formant_ratio, &o) : NAE_ERR_INVALID;
    return rc ? rc : stretch_create(ctx, o, sample_rate, channels, rate, pitch, h);
}

static int stretch_append(nae_stretch* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : stretch_process(h);
}

int nae_stretch_put(nae_stretch* h, const float* interleaved, size_t S) { return stretch_append(h, interleaved, S, false); }
int nae_stretch_put_host(nae_stretch* h, const float* interleaved, size_t S) { return stretch_append(h, interleaved, S, true); }

// everything still buffered is transformed as if the input ended here (zero padding behind the last sample);
// the samples delivered over the handle's life equal nae_stretch_block_f32 on the whole input, bit for bit
int nae_stretch_flush(nae_stretch* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    h->flushed = true;
    return stretch_process(h);
}

size_t nae_stretch_available(nae_stretch* h) { return h ? h->out.total - h->out_read : 0; }

static int stretch_take(nae_stretch* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_stretch_receive(nae_stretch* h, float* dst, size_t max_frames, size_t* got) { return stretch_take(h, dst, max_frames, got, false); }
int nae_stretch_receive_host(nae_stretch* h, float* dst, size_t max_frames, size_t* got) { return stretch_take(h, dst, max_frames, got, true); }

int nae_stretch_destroy(nae_stretch* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->in.free();
    h->mid.free();
    h->out.free();
    for (int i = 0; i < 2; i++)
        if (h->carry[i]) (void)hipFree(h->carry[i]);
    delete h;
    return NAE_OK;
}

// ------------------------------------------------------------------------------------------------ spectrum
int nae_spectrum_create(nae_ctx* ctx, int n_fft, int hop, int channels, nae_spectrum** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    *h = nullptr;
    const int chk = nae_spectrum_check(n_fft, hop);
    if (chk != NAE_OK)
        return nae_fail(ctx, chk, chk == NAE_ERR_UNSUPPORTED ? "spectrum: n_fft must be a power of two in [256, 4096]" : "spectrum: hop must be in [1, n_fft]");
    if (channels != 1 && channels != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    nae_spectrum* s = new (std::nothrow) nae_spectrum();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->ch = channels;
    s->n_fft = n_fft;
    s->hop = hop;
    s->pending.width = (size_t)channels;
    s->out.width = (size_t)channels * (size_t)(n_fft / 2 + 1);
    *h = s;
    return NAE_OK;
}

int nae_spectrum_put(nae_spectrum* h, const float* interleaved, size_t S)
{
    if (!h || (S && !interleaved)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (S == 0) return NAE_OK;
    nae_ctx* ctx = h->ctx;
    int rc = h->pending.push(ctx, interleaved, S, false);
    if (rc) return rc;
    const size_t start = h->out.total * (size_t)h->hop;     // first sample of the next frame
    const size_t T = h->pending.total - start;
    const size_t F = nae_spectrum_frames_ex(T, h->n_fft, h->hop);
    if (F == 0) return NAE_OK;
    if ((rc = h->out.reserve(ctx, h->out.total + F))) return rc;
    const nae_sig src{h->pending.at(start), 0, 1, (size_t)h->ch};
    rc = nae_spectrum_block_ex_f32(ctx, h->n_fft, h->hop, &src, T, h->ch, 1, h->out.at(h->out.total), 0);
    if (rc) return rc;
    h->out.total += F;
    // keep the samples the next frame still needs: everything from its start on
    h->pending.drop((long long)(h->out.total * (size_t)h->hop));
    return NAE_OK;
}

size_t nae_spectrum_available(nae_spectrum* h) { return h ? h->out.total - h->out_read : 0; }

int nae_spectrum_receive(nae_spectrum* h, float* dst, size_t max_frames, size_t* got)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, false);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_spectrum_destroy(nae_spectrum* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->pending.free();
    h->out.free();
    delete h;
    return NAE_OK;
}

// ------------------------------------------------------------------------------------------------ FIR filter
int nae_fir_create(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, int channels, nae_fir** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    if (!taps_host) return nae_fail(ctx, NAE_ERR_INVALID, "fir: null pointer");
    int rc = nae_fir_check(ctx, n_taps, channels, &n_fft);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_fir* s = new (std::nothrow) nae_fir();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->ch = channels;
    s->n_fft = n_fft;
    s->n_taps = n_taps;
    s->in.width = s->out.width = (size_t)channels;
    if (hipMalloc((void**)&s->d_spec, nae_fir_spec_floats(n_fft) * sizeof(float)) != hipSuccess) {
        delete s;
        return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(fir spectrum)");
    }
    if ((rc = nae_fir_make_spec(ctx, taps_host, n_taps, n_fft, s->d_spec))) {
        (void)hipFree(s->d_spec);
        delete s;
        return rc;
    }
    *h = s;
    return NAE_OK;
}

static int fir_append(nae_fir* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : fir_process(h);
}

int nae_fir_put(nae_fir* h, const float* interleaved, size_t S) { return fir_append(h, interleaved, S, false); }
int nae_fir_put_host(nae_fir* h, const float* interleaved_host, size_t S) { return fir_append(h, interleaved_host, S, true); }

// n_taps - 1 zero frames behind the input: the tail of the convolution comes out, in_len + n_taps - 1 frames over the handle's life
int nae_fir_flush(nae_fir* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    const size_t tail = (size_t)h->n_taps - 1;
    if (tail) {
        const int rc = h->in.reserve(h->ctx, h->in.total + tail);
        if (rc) return rc;
        const hipError_t e = hipMemsetAsync(h->in.at(h->in.total), 0, tail * h->in.width * sizeof(float), h->ctx->stream);
        if (e != hipSuccess) return nae_check(h->ctx, e, "hipMemsetAsync(fir flush)");
        h->in.total += tail;
    }
    h->flushed = true;
    return fir_process(h);
}

size_t nae_fir_available(nae_fir* h) { return h ? h->out.total - h->out_read : 0; }

static int fir_take(nae_fir* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_fir_receive(nae_fir* h, float* dst, size_t max_frames, size_t* got) { return fir_take(h, dst, max_frames, got, false); }
int nae_fir_receive_host(nae_fir* h, float* dst_host, size_t max_frames, size_t* got) { return fir_take(h, dst_host, max_frames, got, true); }

int nae_fir_destroy(nae_fir* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->in.free();
    h->out.free();
    if (h->d_spec) (void)hipFree(h->d_spec);
    delete h;
    return NAE_OK;
}

// ------------------------------------------------------------------------------------------------ long convolution
int nae_conv_create(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, int channels, nae_conv** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    if (!taps_host) return nae_fail(ctx, NAE_ERR_INVALID, "conv: null pointer");
    int rc = nae_conv_check(ctx, n_taps, taps_ch, channels, &n_fft);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_conv* s = new (std::nothrow) nae_conv();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->ch = channels;
    s->n_fft = n_fft;
    s->n_taps = n_taps;
    s->taps_ch = taps_ch;
    s->parts = nae_conv_parts(n_taps, n_fft);
    s->ring = nae_pick_conv_ring(ctx, n_fft, s->parts, NAE_CONV_HANDLE_SLAB, (size_t)channels);
    s->in.width = s->out.width = (size_t)channels;
    if (hipMalloc((void**)&s->d_spec, nae_conv_spec_floats(n_fft, s->parts, taps_ch) * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&s->d_ring, nae_conv_ring_floats(n_fft, (size_t)channels, s->ring) * sizeof(float)) != hipSuccess) {
        if (s->d_spec) (void)hipFree(s->d_spec);
        delete s;
        return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(conv spectra)");
    }
    if ((rc = nae_conv_make_spec(ctx, taps_host, n_taps, taps_ch, n_fft, s->d_spec))) {
        (void)hipFree(s->d_spec);
        (void)hipFree(s->d_ring);
        delete s;
        return rc;
    }
    *h = s;
    return NAE_OK;
}

static int conv_append(nae_conv* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : conv_process(h);
}

int nae_conv_put(nae_conv* h, const float* interleaved, size_t S) { return conv_append(h, interleaved, S, false); }
int nae_conv_put_host(nae_conv* h, const float* interleaved_host, size_t S) { return conv_append(h, interleaved_host, S, true); }

// n_taps - 1 zero frames behind the input: the tail of the convolution comes out, in_len + n_taps - 1 frames over the handle's life
int nae_conv_flush(nae_conv* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    const size_t tail = (size_t)h->n_taps - 1;
    if (tail) {
        const int rc = h->in.reserve(h->ctx, h->in.total + tail);
        if (rc) return rc;
        const hipError_t e = hipMemsetAsync(h->in.at(h->in.total), 0, tail * h->in.width * sizeof(float), h->ctx->stream);
        if (e != hipSuccess) return nae_check(h->ctx, e, "hipMemsetAsync(conv flush)");
        h->in.total += tail;
    }
    h->flushed = true;
    return conv_process(h);
}

size_t nae_conv_available(nae_conv* h) { return h ? h->out.total - h->out_read : 0; }

static int conv_take(nae_conv* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_conv_receive(nae_conv* h, float* dst, size_t max_frames, size_t* got) { return conv_take(h, dst, max_frames, got, false); }
int nae_conv_receive_host(nae_conv* h, float* dst_host, size_t max_frames, size_t* got) { return conv_take(h, dst_host, max_frames, got, true); }

int nae_conv_destroy(nae_conv* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->in.free();
    h->out.free();
    if (h->d_spec) (void)hipFree(h->d_spec);
    if (h->d_ring) (void)hipFree(h->d_ring);
    delete h;
    return NAE_OK;
}

// ------------------------------------------------------------------------------------------------ biquad cascade
int nae_eq_create(nae_ctx* ctx, const double* coef_host, int n_sections, int channels, nae_eq** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_eq_check(ctx, coef_host, n_sections, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_eq* s = new (std::nothrow) nae_eq();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->ch = channels;
    s->n_sections = n_sections;
    s->in.width = s->out.width = (size_t)channels;
    const size_t state_bytes = (size_t)channels * NAE_EQ_MAX_SECTIONS * 2 * sizeof(double);
    if (hipMalloc((void**)&s->d_block, nae_eq_block_doubles() * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&s->d_state, state_bytes) != hipSuccess) {
        if (s->d_block) (void)hipFree(s->d_block);
        delete s;
        return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(eq tables)");
    }
    const hipError_t e = hipMemsetAsync(s->d_state, 0, state_bytes, ctx->stream);
    rc = e != hipSuccess ? nae_check(ctx, e, "hipMemsetAsync(eq state)") : nae_eq_make_block(ctx, coef_host, n_sections, s->d_block);
    if (rc) {
        (void)hipFree(s->d_block);
        (void)hipFree(s->d_state);
        delete s;
        return rc;
    }
    *h = s;
    return NAE_OK;
}

static int eq_append(nae_eq* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : eq_process(h);
}

int nae_eq_put(nae_eq* h, const float* interleaved, size_t S) { return eq_append(h, interleaved, S, false); }
int nae_eq_put_host(nae_eq* h, const float* interleaved_host, size_t S) { return eq_append(h, interleaved_host, S, true); }

// the partial last chunk comes out: as many frames as were put over the handle's life (an IIR has no tail to append)
int nae_eq_flush(nae_eq* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    h->flushed = true;
    return eq_process(h);
}

size_t nae_eq_available(nae_eq* h) { return h ? h->out.total - h->out_read : 0; }

static int eq_take(nae_eq* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_eq_receive(nae_eq* h, float* dst, size_t max_frames, size_t* got) { return eq_take(h, dst, max_frames, got, false); }
int nae_eq_receive_host(nae_eq* h, float* dst_host, size_t max_frames, size_t* got) { return eq_take(h, dst_host, max_frames, got, true); }

int nae_eq_destroy(nae_eq* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->in.free();
    h->out.free();
    if (h->d_block) (void)hipFree(h->d_block);
    if (h->d_state) (void)hipFree(h->d_state);
    delete h;
    return NAE_OK;
}

// ------------------------------------------------------------------------------------------------ dynamics
int nae_dyn_create(nae_ctx* ctx, const nae_dyn_params* params, int channels, nae_dyn** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_dyn_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_dyn* s = new (std::nothrow) nae_dyn();
    if (!s) return NAE_ERR_NOMEM;
    s->ctx = ctx;
    s->ch = channels;
    s->params = *params;
    s->in.width = s->out.width = (size_t)channels;
    const size_t state_bytes = nae_dyn_detectors(params, channels, 1) * 2 * sizeof(double);
    if (hipMalloc((void**)&s->d_state, state_bytes) != hipSuccess) {
        delete s;
        return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(dyn state)");
    }
    const hipError_t e = hipMemsetAsync(s->d_state, 0, state_bytes, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(s->d_state);
        delete s;
        return nae_check(ctx, e, "hipMemsetAsync(dyn state)");
    }
    *h = s;
    return NAE_OK;
}

static int dyn_append(nae_dyn* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : dyn_process(h);
}

int nae_dyn_put(nae_dyn* h, const float* interleaved, size_t S) { return dyn_append(h, interleaved, S, false); }
int nae_dyn_put_host(nae_dyn* h, const float* interleaved_host, size_t S) { return dyn_append(h, interleaved_host, S, true); }

// the chunks that waited for their look-ahead and the partial last one come out: as many frames as were put over the handle's life
int nae_dyn_flush(nae_dyn* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    h->flushed = true;
    return dyn_process(h);
}

size_t nae_dyn_available(nae_dyn* h) { return h ? h->out.total - h->out_read : 0; }

static int dyn_take(nae_dyn* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}

int nae_dyn_receive(nae_dyn* h, float* dst, size_t max_frames, size_t* got) { return dyn_take(h, dst, max_frames, got, false); }
int nae_dyn_receive_host(nae_dyn* h, float* dst_host, size_t max_frames, size_t* got) { return dyn_take(h, dst_host, max_frames, got, true); }

int nae_dyn_destroy(nae_dyn* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    h->in.free();
    h->out.free();
    if (h->d_state) (void)hipFree(h->d_state);
    delete h;
    return NAE_OK;
}

} // extern "C"
