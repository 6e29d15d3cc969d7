// nae_wsola.hip — host side of K7 option A (SoundTouch-shaped WSOLA chain): parameters, the scalar bookkeeping of
// st_chain.h, the block entry point and the streaming handle (nae_wsola, on stream_util.h's handle core).  Device work is in
// kernels_wsola.hip.
//
// Replaces soundtouch::SoundTouch as used by /root/reference/src/processor/audio-velocity.cpp:369-428.
#include "st_chain.h"
#include "stream_util.h"
#include <math.h>
#include <new>
#include <string.h>
#include <vector>

namespace nae {

int st_cfg_make(StCfg& c, int sample_rate, int channels, double rate, double pitch)
{
    if (channels != 1 && channels != 2) return NAE_ERR_INVALID;
    if (sample_rate < 8000 || sample_rate > 48000) return NAE_ERR_UNSUPPORTED;   // audio-velocity.cpp:371-379
    if (!(rate > 0.0) || !(pitch > 0.0)) return NAE_ERR_INVALID;
    c.sr = sample_rate;
    c.ch = channels;
    c.tempo = 1.0 / pitch;
    c.rate = pitch * rate;
    if (!(c.tempo >= NAE_TEMPO_MIN && c.tempo <= NAE_TEMPO_MAX) || !(c.rate >= NAE_RATE_MIN && c.rate <= NAE_RATE_MAX))
        return NAE_ERR_UNSUPPORTED;
    c.order = (c.rate > 1.0) ? 0 : (c.rate < 1.0 ? 2 : 1);
    // sequence 90..40 ms and seek window 20..15 ms, linear in tempo over [0.5, 2], whole milliseconds; overlap 8 ms
    const double seq_k = (40.0 - 90.0) / (2.0 - 0.5), seq_c = 90.0 - seq_k * 0.5;
    const double seek_k = (15.0 - 20.0) / (2.0 - 0.5), seek_c = 20.0 - seek_k * 0.5;
    double seq = seq_c + seq_k * c.tempo;
    seq = seq < 40.0 ? 40.0 : (seq > 90.0 ? 90.0 : seq);
    double seek = seek_c + seek_k * c.tempo;
    seek = seek < 15.0 ? 15.0 : (seek > 20.0 ? 20.0 : seek);
    const int seq_ms = (int)(seq + 0.5), seek_ms = (int)(seek + 0.5);
    int ovl = (sample_rate * 8) / 1000;
    if (ovl < 16) ovl = 16;
    ovl -= ovl % 8;
    c.ovl = ovl;
    c.swl = (sample_rate * seq_ms) / 1000;
    if (c.swl < 2 * ovl) c.swl = 2 * ovl;
    c.seekl = (sample_rate * seek_ms) / 1000;
    c.body = c.swl - 2 * ovl;
    c.nominal_skip = c.tempo * (double)(c.swl - ovl);
    const int intskip = (int)(c.nominal_skip + 0.5);
    const int a = intskip + ovl, b = c.swl;
    c.sample_req = (a > b ? a : b) + c.seekl;
    c.first_skip = (int)(c.tempo * (double)ovl + 0.5 * (double)c.seekl + 0.5);
    // anti-alias filter: Hamming-windowed sinc, cutoff 0.5/rate above unity and 0.5*rate below; scaled to a 2^14
    // grid with the library's rounding half left in (float build)
    const double cutoff = c.rate > 1.0 ? 0.5 / c.rate : 0.5 * c.rate;
    const double pi = 3.14159265358979323846;
    double work[kAaLen], sum = 0.0;
    const double wc = 2.0 * pi * cutoff, tc = (2.0 * pi) / (double)kAaLen;
    for (int i = 0; i < kAaLen; i++) {
        const double t = (double)i - (double)(kAaLen / 2);
        const double arg = t * wc;
        const double h = (arg != 0.0) ? sin(arg) / arg : 1.0;
        work[i] = (0.54 + 0.46 * cos(tc * t)) * h;
        sum += work[i];
    }
    const double scale = 16384.0 / sum;
    for (int i = 0; i < kAaLen; i++) {
        double v = work[i] * scale;
        v += (v >= 0.0) ? 0.5 : -0.5;
        c.aa[i] = (float)v / 16384.0f;
    }
    return NAE_OK;
}

static void sim_td(const StCfg& c, StState& s)
{
    while (s.td_in - s.td_ip >= c.sample_req) {
        if (!s.td_begin) {
            s.td_out += c.ovl;
        } else {
            s.td_begin = false;
            s.td_skip -= (double)c.first_skip;
            if (s.td_skip <= -c.nominal_skip) s.td_skip = -c.nominal_skip;
        }
        s.td_out += c.body;
        s.td_nseq++;
        s.td_skip += c.nominal_skip;
        const int adv = (int)s.td_skip;
        s.td_skip -= (double)adv;
        s.td_ip += adv;
    }
}

static void sim_aa(const StCfg& c, StState& s)
{
    const long long n = s.aa_in - s.aa_out;
    if (n < kAaLen) return;
    long long count = n - kAaLen;
    if (c.ch == 2) {
        count &= ~1ll;
        if (count < 2) return;
    }
    s.aa_out += count;
}

static void sim_cu(const StCfg& c, StState& s, CuTable* tab)
{
    const long long n = s.cu_in - s.cu_pos, end = n - 4;
    long long used = 0;
    while (used < end) {
        if (tab) {
            tab->pos.push_back(s.cu_pos + used);
            tab->fract.push_back((float)s.cu_fract);
        }
        s.cu_out++;
        s.cu_fract += c.rate;
        const int whole = (int)s.cu_fract;
        s.cu_fract -= (double)whole;
        used += whole;
    }
    s.cu_pos += used;
}

void st_sim_put(const StCfg& c, StState& s, long long n, CuTable* tab)
{
    if (n <= 0) return;
    s.expected += (double)n / (c.rate * c.tempo);
    switch (c.order) {
    case 0:
        s.td_in += n;
        sim_td(c, s);
        if (s.td_out > s.aa_in) {
            s.aa_in = s.td_out;
            sim_aa(c, s);
            s.cu_in = s.aa_out;
            sim_cu(c, s, tab);
        }
        break;
    case 1:
        s.aa_in += n;
        sim_aa(c, s);
        s.cu_in = s.aa_out;
        sim_cu(c, s, tab);
        s.td_in = s.cu_out;
        sim_td(c, s);
        break;
    default:
        s.cu_in += n;
        sim_cu(c, s, tab);
        s.aa_in = s.cu_out;
        sim_aa(c, s);
        s.td_in = s.aa_out;
        sim_td(c, s);
        break;
    }
}

long long st_final_out(const StCfg& c, const StState& s) { return c.order == 0 ? s.cu_out : s.td_out; }

// the zero puts of SoundTouch::flush: 128 frames at a time until `still` frames are available, at most 200 times
static long long sim_flush(const StCfg& c, StState& s, long long received, CuTable* tab, long long* zeros_fed)
{
    long long still = (long long)(s.expected + 0.5) - received;
    if (still < 0) still = 0;
    long long fed = 0;
    for (int i = 0; still > st_final_out(c, s) - received && i < 200; i++) {
        st_sim_put(c, s, 128, tab);
        fed += 128;
    }
    if (zeros_fed) *zeros_fed = fed;
    const long long avail = st_final_out(c, s) - received;
    return avail < still ? avail : still;
}

static int upload_cu(nae_ctx* ctx, const CuTable& tab, size_t first, size_t count, long long* d_pos, float* d_fract)
{
    if (!count) return NAE_OK;
    hipError_t e = hipMemcpyAsync(d_pos + first, tab.pos.data() + first, count * sizeof(long long), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_fract + first, tab.fract.data() + first, count * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // the host vectors may move after this call
    return nae_check(ctx, e, "hipMemcpyAsync(cubic table)");
}

} // namespace nae

using namespace nae;

// the cubic stage's table on the device: the source position and the fraction of every output (CuTable's two columns).  Each column knows its
// own capacity, so a grow that fails at the second one leaves nothing to put right
struct CuDevTable {
    CtxBuf pos, fract;

    int reserve(nae_ctx* ctx, size_t want)
    {
        const int rc = pos.reserve(ctx, want * sizeof(long long), "cubic table");
        return rc ? rc : fract.reserve(ctx, want * sizeof(float), "cubic table");
    }
    long long* d_pos() const { return pos.as<long long>(); }
    float* d_fract() const { return fract.as<float>(); }
};

// plan cache of the block entry point (one entry: the bench and batch jobs repeat one parameter set)
struct nae_wsola_cache {
    bool valid = false;
    int sr = 0, ch = 0;
    double rate = 0, pitch = 0;
    size_t in_len = 0;
    StCfg cfg;
    StState fin;
    long long out_len = 0;
    CuDevTable tab;
    CtxBuf tile_n;                  // first cubic output of every fused filter+cubic tile (orders 0 and 1), ints
    size_t n_tiles = 0;
    CtxBuf ws_a, ws_b;              // the signals between the stages
};

void nae_wsola_cache_free(nae_wsola_cache* c) { delete c; }

static int plan_fill(const StCfg& cfg, const StState& fin, long long out_len, size_t in_len, long long zeros, nae_wsola_plan* pl)
{
    memset(pl, 0, sizeof *pl);
    pl->sample_rate = cfg.sr;
    pl->channels = cfg.ch;
    pl->rate_eff = cfg.rate;
    pl->tempo_eff = cfg.tempo;
    pl->order = cfg.order;
    pl->overlap_len = cfg.ovl;
    pl->seq_len = cfg.swl;
    pl->seek_len = cfg.seekl;
    pl->sample_req = cfg.sample_req;
    pl->nominal_skip = cfg.nominal_skip;
    pl->in_len = in_len;
    pl->flush_zeros = (size_t)zeros;
    pl->n_seq = (size_t)fin.td_nseq;
    pl->td_out_len = (size_t)fin.td_out;
    pl->aa_out_len = (size_t)fin.aa_out;
    pl->cu_out_len = (size_t)fin.cu_out;
    pl->out_len = (size_t)out_len;
    return NAE_OK;
}

extern "C" {

int nae_wsola_plan_make(int sample_rate, int channels, double rate, double pitch, size_t in_len, nae_wsola_plan* plan)
{
    if (!plan) return NAE_ERR_INVALID;
    StCfg cfg;
    int rc = st_cfg_make(cfg, sample_rate, channels, rate, pitch);
    if (rc) return rc;
    StState s;
    st_sim_put(cfg, s, (long long)in_len, nullptr);
    long long zeros = 0;
    const long long out_len = sim_flush(cfg, s, 0, nullptr, &zeros);
    return plan_fill(cfg, s, out_len, in_len, zeros, plan);
}

int nae_wsola_block_f32(nae_ctx* ctx, int sample_rate, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                        size_t n_streams, const nae_sig* dst, int32_t* offsets_dbg)
{
    if (!ctx) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    if (!src || !dst || !src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "nae_wsola_block_f32: null signal");
    if (!ctx->wsola_cache) ctx->wsola_cache.reset(new (std::nothrow) nae_wsola_cache());
    nae_wsola_cache* wc = ctx->wsola_cache.get();
    if (!wc) return nae_fail(ctx, NAE_ERR_NOMEM, "plan cache");
    int rc;
    if (!(wc->valid && wc->sr == sample_rate && wc->ch == ch && wc->rate == rate && wc->pitch == pitch && wc->in_len == in_len)) {
        wc->valid = false;
        rc = st_cfg_make(wc->cfg, sample_rate, ch, rate, pitch);
        if (rc) return nae_fail(ctx, rc, "nae_wsola_block_f32: parameters");
        CuTable tab;
        StState s;
        st_sim_put(wc->cfg, s, (long long)in_len, &tab);
        wc->out_len = sim_flush(wc->cfg, s, 0, &tab, nullptr);
        wc->fin = s;
        rc = wc->tab.reserve(ctx, tab.pos.size());
        if (!rc) rc = upload_cu(ctx, tab, 0, tab.pos.size(), wc->tab.d_pos(), wc->tab.d_fract());
        if (rc) return rc;
        wc->n_tiles = 0;
        if (wc->cfg.order != 2) {
            // filter and cubic stage are adjacent: they run as one launch, tile by tile
            std::vector<int> tile_n;
            st_tile_starts(tab, wc->cfg.order == 0 ? wc->out_len : s.cu_out, tile_n);
            rc = wc->tile_n.reserve(ctx, tile_n.size() * sizeof(int), "tile table");
            if (rc) return rc;
            if (!tile_n.empty()) {
                hipError_t e = hipMemcpyAsync(wc->tile_n.as<int>(), tile_n.data(), tile_n.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) return nae_check(ctx, e, "hipMemcpyAsync(tile table)");
                wc->n_tiles = tile_n.size() - 1;
            }
        }
        wc->sr = sample_rate; wc->ch = ch; wc->rate = rate; wc->pitch = pitch; wc->in_len = in_len;
        wc->valid = true;
    }
    if (n_streams == 0 || wc->out_len == 0) return NAE_OK;
    const StCfg& cfg = wc->cfg;
    const StState& fin = wc->fin;
    // intermediate signals: interleaved [n][ch] per stream
    const size_t w = (size_t)ch;
    size_t len1, len2;     // outputs of the first and the second stage
    switch (cfg.order) {
    case 0: len1 = (size_t)fin.td_out; len2 = (size_t)fin.aa_out; break;
    case 1: len1 = (size_t)fin.aa_out; len2 = (size_t)fin.cu_out; break;
    default: len1 = (size_t)fin.cu_out; len2 = (size_t)fin.aa_out; break;
    }
    const size_t stride1 = (len1 + 8) * w, stride2 = (len2 + 8) * w;
    rc = wc->ws_a.reserve(ctx, n_streams * stride1 * sizeof(float), "workspace");
    if (!rc) rc = wc->ws_b.reserve(ctx, n_streams * stride2 * sizeof(float), "workspace");
    if (rc) return rc;
    const StView v_src{(const float*)src->base, (long long)src->stream_stride, (long long)src->chan_stride,
                       (long long)src->frame_stride, 0, (long long)in_len};
    const StOut o_a{wc->ws_a.as<float>(), (long long)stride1, 1, (long long)w, 0};
    const StOut o_b{wc->ws_b.as<float>(), (long long)stride2, 1, (long long)w, 0};
    const StView v_a{wc->ws_a.as<float>(), (long long)stride1, 1, (long long)w, 0, (long long)len1};
    const StView v_b{wc->ws_b.as<float>(), (long long)stride2, 1, (long long)w, 0, (long long)len2};
    const StOut o_dst{(float*)dst->base, (long long)dst->stream_stride, (long long)dst->chan_stride, (long long)dst->frame_stride, 0};
    const TdRange all{0, 0, fin.td_nseq, 0.0, 1, cfg.order == 0 ? (long long)len1 : wc->out_len};
    const long long n_offs = fin.td_nseq > 0 ? fin.td_nseq - 1 : 0;
    const long long* d_pos = wc->tab.d_pos();
    const float* d_fract = wc->tab.d_fract();
    switch (cfg.order) {
    case 0:
        rc = st_launch_td(ctx, cfg, v_src, all, o_a, n_streams, nullptr, offsets_dbg, n_offs);
        if (!rc && !ctx->dbg_st_unfused)
            rc = st_launch_aa_cu(ctx, cfg, v_a, d_pos, d_fract, wc->tile_n.as<int>(), wc->n_tiles, wc->out_len, o_dst, n_streams);
        else {
            if (!rc) rc = st_launch_aa(ctx, cfg, v_a, 0, fin.aa_out, o_b, n_streams);
            if (!rc) rc = st_launch_cu(ctx, cfg, v_b, d_pos, d_fract, 0, 0, wc->out_len, o_dst, n_streams);
        }
        break;
    case 1:
        if (!ctx->dbg_st_unfused)
            rc = st_launch_aa_cu(ctx, cfg, v_src, d_pos, d_fract, wc->tile_n.as<int>(), wc->n_tiles, fin.cu_out, o_b, n_streams);
        else {
            rc = st_launch_aa(ctx, cfg, v_src, 0, fin.aa_out, o_a, n_streams);
            if (!rc) rc = st_launch_cu(ctx, cfg, v_a, d_pos, d_fract, 0, 0, fin.cu_out, o_b, n_streams);
        }
        if (!rc) rc = st_launch_td(ctx, cfg, v_b, all, o_dst, n_streams, nullptr, offsets_dbg, n_offs);
        break;
    default:
        if (!ctx->dbg_st_unfused)
            rc = st_launch_cu_aa(ctx, cfg, v_src, d_pos, d_fract, fin.cu_out, fin.aa_out, o_b, n_streams);
        else {
            rc = st_launch_cu(ctx, cfg, v_src, d_pos, d_fract, 0, 0, fin.cu_out, o_a, n_streams);
            if (!rc) rc = st_launch_aa(ctx, cfg, v_a, 0, fin.aa_out, o_b, n_streams);
        }
        if (!rc) rc = st_launch_td(ctx, cfg, v_b, all, o_dst, n_streams, nullptr, offsets_dbg, n_offs);
        break;
    }
    return rc;
}

} // extern "C"

// ------------------------------------------------------------------ streaming handle
// SoundTouch-shaped calls (audio-velocity.cpp:403 putSamples, :399 numSamples, :298 receiveSamples, :427 flush) on
// one stream.  Every put advances the scalar bookkeeping, then each stage is launched once for the index range
// that became computable; the FIFOs between the stages are addressed by absolute frame index.  The handle stands on stream_util.h's core:
// `in` holds the frames really put (the flush's zeros are virtual), and put, flush, available, receive and destroy are the core's.
struct nae_wsola : StreamHandle {
    StCfg cfg;
    StState st;                  // everything up to this state has been computed on the device
    size_t fed = 0;              // frames of `in` that `st` has seen
    CuDevTable tab;              // the cubic outputs of one step
    DevFifo a, b;                // stage 1 -> 2, stage 2 -> 3
    float* d_mid = nullptr;      // stretcher tail carried between calls
    int process() override;
    ~nae_wsola() override
    {
        a.free();
        b.free();
    }
};

namespace {

int wsola_run(nae_wsola* h, const StState& before)
{
    nae_ctx* ctx = h->ctx;
    const StCfg& c = h->cfg;
    const StState& now = h->st;
    int rc;
    // table entries for the new cubic outputs: generated on the device from the state in front of them (no host copy,
    // so a put never blocks)
    const long long cu_new = now.cu_out - before.cu_out;
    if (cu_new > 0) {
        rc = h->tab.reserve(ctx, (size_t)cu_new);
        if (!rc) rc = st_launch_cu_table(ctx, before.cu_pos, before.cu_fract, c.rate, cu_new, h->tab.d_pos(), h->tab.d_fract());
        if (rc) return rc;
    }
    DevFifo* chain[4] = {&h->in, &h->a, &h->b, &h->out};
    const int kinds[3][3] = {{0, 1, 2}, {1, 2, 0}, {2, 1, 0}};   // 0 TD, 1 AA, 2 CU per stage slot
    for (int slot = 0; slot < 3; slot++) {
        const int kind = kinds[c.order][slot];
        DevFifo& src = *chain[slot];
        DevFifo& dst = *chain[slot + 1];
        const long long out_before = kind == 0 ? before.td_out : (kind == 1 ? before.aa_out : before.cu_out);
        const long long out_now = kind == 0 ? now.td_out : (kind == 1 ? now.aa_out : now.cu_out);
        if (out_now > out_before) {
            rc = dst.reserve(ctx, (size_t)out_now);
            if (rc) return rc;
            const long long w = (long long)src.width;
            const StView vin{src.p, 0, 1, w, (long long)src.base, (long long)src.total};
            const StOut vout{dst.p, 0, 1, w, (long long)dst.base};
            if (kind == 0) {
                const TdRange r{before.td_ip, before.td_out, now.td_nseq - before.td_nseq, before.td_skip, before.td_begin ? 1 : 0,
                                out_now};
                rc = st_launch_td(ctx, c, vin, r, vout, 1, h->d_mid, nullptr, 0);
            } else if (kind == 1) {
                rc = st_launch_aa(ctx, c, vin, out_before, out_now, vout, 1);
            } else {
                rc = st_launch_cu(ctx, c, vin, h->tab.d_pos(), h->tab.d_fract(), before.cu_out, out_before, out_now, vout, 1);
            }
            if (rc) return rc;
            dst.total = (size_t)out_now;
        }
        // what this stage will never read again
        const long long keep_from = kind == 0 ? now.td_ip : (kind == 1 ? now.aa_out : now.cu_pos);
        src.drop(keep_from);
    }
    return NAE_OK;
}

} // namespace

// the one step behind a put and the flush: the bookkeeping takes the frames that arrived, or the flush's zero puts, and the stages run
int nae_wsola::process()
{
    const StState before = st;
    long long release = 0;
    if (flushed) {
        release = sim_flush(cfg, st, (long long)out_read, nullptr, nullptr);
    } else {
        st_sim_put(cfg, st, (long long)(in.total - fed), nullptr);
        fed = in.total;
    }
    const int rc = wsola_run(this, before);
    if (rc) return rc;
    // the flush releases `release` frames and no more; nothing runs after it, so cutting the FIFO's end short says so once and for all
    if (flushed && out_read + (size_t)release < out.total) out.total = out_read + (size_t)release;
    return NAE_OK;
}

extern "C" {

int nae_wsola_create(nae_ctx* ctx, int sample_rate, int channels, double rate, double pitch, nae_wsola** out)
{
    if (!ctx || !out) return NAE_ERR_INVALID;
    *out = nullptr;
    (void)nae_use_device(ctx);
    StCfg cfg;
    int rc = st_cfg_make(cfg, sample_rate, channels, rate, pitch);
    if (rc)
        return nae_fail(ctx, rc, rc == NAE_ERR_UNSUPPORTED ? "nae_wsola_create: sample rate outside 8000..48000 Hz or ratio out of range"
                                                           : "nae_wsola_create: bad parameters");
    nae_wsola* h = handle_new<nae_wsola>(ctx, channels);
    if (!h) return NAE_ERR_NOMEM;
    h->cfg = cfg;
    h->a.width = h->b.width = (size_t)channels;
    rc = h->dev_alloc(&h->d_mid, (size_t)cfg.ovl * (size_t)channels, "hipMalloc(stretcher tail)");
    return handle_created(h, rc, out);
}

int nae_wsola_put(nae_wsola* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_wsola_put_host(nae_wsola* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the zero puts of SoundTouch::flush (sim_flush); what it releases is counted from the frames received so far
int nae_wsola_flush(nae_wsola* h) { return handle_flush(h); }
size_t nae_wsola_available(const nae_wsola* h) { return handle_available(h); }
int nae_wsola_receive(nae_wsola* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_wsola_receive_host(nae_wsola* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_wsola_destroy(nae_wsola* h) { return handle_destroy(h); }

} // extern "C"
