// nae_stream.hip — SoundTouch-shaped and spectrum streaming handles on top of the block kernels.
//
// nae_stretch mirrors the calls soundtouch_process_payload makes (/root/reference/src/processor/
// audio-velocity.cpp:369-428): putSamples / numSamples / receiveSamples / flush.
//
// Every handle stands on stream_util.h's core (StreamHandle / BlockHandle): put, flush, available, receive and destroy are written there
// once.  A handle adds its own fields, its create entry and process(), the step that computes what became computable.  nae_wsola
// (nae_wsola.hip) and nae_swr (nae_swr.hip) stand on the same core beside their own host code.
#include "nae_internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stream_util.h"

struct nae_stretch : StreamHandle {
    int sample_rate;
    double rate, pitch;
    nae_pv_opts opts;             // what the nae_stretch_create* entry asked for
    nae_stretch_plan pl{};        // parameters (in_len = 0)
    nae_pv_run run{};             // the options as this plan runs them (none of it depends on in_len)
    // phase vocoder
    size_t blocks_done = 0;       // hop blocks produced == frames folded into the carried phase
    uint32_t* carry[2] = {nullptr, nullptr};
    int carry_cur = 0;
    DevFifo mid;                  // between the stages: planar when the vocoder runs first, else interleaved
    int process() override;
    ~nae_stretch() override { mid.free(); }
};

// `in` holds the interleaved samples from the first one the next frame needs; `out` frames of [ch][n_fft/2 + 1]
struct nae_spectrum : StreamHandle {
    int n_fft = NAE_FFT_N, hop = NAE_HOP;
    int process() override;
};

// the FIR filter's handle ("K9 FIR filter"): whole blocks of n_fft / 2 samples are filtered as they become available; the input
// stays from the half block in front of the next block on
struct nae_fir : BlockHandle {
    int n_fft;
    float* d_spec = nullptr;       // the padded taps and their spectrum H (nae_fir_make_spec)
    int process() override;
};

// the long convolution's handle ("K10 long convolution"): nae_fir's, with the ring of spectra kept between puts
struct nae_conv : BlockHandle {
    int n_fft, taps_ch, parts;
    float* d_spec = nullptr;       // the padded taps and their spectra H (nae_conv_make_spec)
    float* d_ring = nullptr;       // [ch][ring] spectra: the last parts - 1 blocks stay in it between puts
    size_t ring = 0;
    int process() override;
};

// the biquad cascade's handle ("K11 biquad cascade"): whole chunks of NAE_EQ_CHUNK samples are filtered as they fill; the sections'
// carry between two launches stays on the device
struct nae_eq : BlockHandle {
    int n_sections;
    double* d_block = nullptr;     // coefficients and tables (nae_eq_make_block)
    double* d_state = nullptr;     // [ch][NAE_EQ_MAX_SECTIONS][2]: every section's (z1, z2) behind the last chunk done
    int process() override;
};

// the dynamics processor's handle ("K12 dynamics"): whole chunks of NAE_DYN_CHUNK samples are computed once the `lookahead` samples
// behind them are there; the detectors' carries between two launches stay on the device
struct nae_dyn : BlockHandle {
    nae_dyn_params params;
    double* d_state = nullptr;     // [detector][2]: (y1, yl) behind the last chunk done
    int process() override;
};

// the keyed dynamics' handle ("K15 keyed dynamics"): nae_dyn's, with an input FIFO of ch + key_ch floats per frame — the signal's
// channels, then the key's — and the key filter's carries in front of the next chunk beside the detectors'
struct nae_dynkey : BlockHandle {
    nae_dynkey_params params;
    double* d_block = nullptr;     // the key filter's coefficients and tables (nae_eq_make_block); null with no section
    double* d_state = nullptr;     // [detector][2]: (y1, yl) behind the last chunk done
    double* d_fstate = nullptr;    // nae_dynkey_filter_doubles(): the filter's (z1, z2) behind the last chunk done
    int process() override;
};

// the echo's handle ("K16 echo"): whole chunks of NAE_EQ_CHUNK samples are computed as they fill; the delay lines and the sections' carry
// between two launches stay on the device.  Chunks are counted from the stream's first sample, so any cut into puts gives the block call's bits
struct nae_echo : BlockHandle {
    nae_echo_params params;
    double* d_block = nullptr;     // the sections' coefficients and tables (nae_eq_make_block); null with no section
    float* d_line = nullptr;       // [ch][nae_echo_ring()]: the lines' last samples, by absolute index mod the ring
    double* d_state = nullptr;     // [ch][NAE_ECHO_MAX_SECTIONS][2]: every section's (z1, z2) behind the last chunk done
    int process() override;
};

// the modulated delay's handle ("K17 modulated delay"): whole chunks of NAE_EQ_CHUNK samples are computed as they fill; every channel's
// last NAE_MOD_KEEP line samples between two launches stay on the device, and `done` is the sample count.  Phases and runs are counted from the
// stream's first sample, so any cut into puts gives the block call's bits
struct nae_mod : BlockHandle {
    nae_mod_params params;
    float* d_state = nullptr;      // [ch][NAE_MOD_KEEP]: the lines' samples in front of the next chunk (zero in front of the first)
    int process() override;
};

// the saturation's handle ("K18 saturation"): whole chunks of NAE_EQ_CHUNK samples are computed as they fill; the kernel keeps nothing
// between launches and reads the 64 samples in front of a chunk from the input itself, so the last chunk of input stays in the FIFO; the flush puts
// the latency's zero frames behind the input (flush_tail)
struct nae_sat : BlockHandle {
    nae_sat_params params;
    int process() override;
};

// the gate's handle ("K19 gate"): whole chunks of NAE_DYN_CHUNK samples are computed once the `lookahead` samples behind them are
// there; the detectors' carries in front of the next chunk stay on the device between two launches
struct nae_gate : BlockHandle {
    nae_gate_params params;
    long long* d_state = nullptr;  // [detector][3]: the hysteresis state, the last set sample or -1, and y's bits in front of the next chunk
    int process() override;
};

// the multiband compressor's handle ("K20 multiband"): whole chunks of NAE_DYN_CHUNK samples are computed once the `lookahead`
// samples behind them are there, in slabs through the handle's own band planes; the sections' and the detectors' carries in front of the next
// chunk stay on the device between two launches
struct nae_mb : BlockHandle {
    nae_mb_params params;
    double* d_block = nullptr;     // the tree's coefficients and tables (nae_eq_make_block)
    float* d_planes = nullptr;     // nae_mb_plane_floats(): the band signals of a slab and the chunk behind it
    double* d_state = nullptr;     // nae_mb_state_doubles(): the carries in front of the next chunk
    size_t slab = 0;               // chunks per slab (nae_mb_handle_slab at the create)
    int process() override;
};

// the spectral gate's handle ("K13 spectral gate"): whole hop blocks of n_fft / 4 samples are computed once the time_smooth + 3
// blocks behind them are there; the input stays from time_smooth + 3 blocks in front of the next block on, and nothing else is kept
struct nae_denoise : BlockHandle {
    nae_denoise_params params;
    int profile_ch = 1;
    float* d_profile = nullptr;    // [profile_ch][n_fft / 2 + 1], the handle's own copy
    int process() override;
};

// the separation's handle ("K21 separation"): whole hop blocks of n_fft / 4 samples are computed once the time_span + 3 blocks behind
// them are there; the input stays from time_span + 3 blocks in front of the next block on, and nothing else is kept
struct nae_hpss : BlockHandle {
    nae_hpss_params params;
    int process() override;
};

// the limiter's handle ("K22 limiter"): whole chunks of NAE_DYN_CHUNK samples are computed once the `lookahead` samples behind them
// and the detector's reach are there; the chunk in front of the next one stays in the FIFO (the true-peak FIR reads its last samples), and the
// detectors' carries stay on the device between two launches
struct nae_lim : BlockHandle {
    nae_lim_params params;
    unsigned long long* d_state = nullptr;  // [detector][nae_lim_state_words()]: y1's bits, the running total of q, the last chunk's prefix sums
    int process() override;
};

// the dither's handle ("K23 dither"): a unit is one frame and nothing is waited for or kept, so every put is computed at once
// from the position it reached; the K errors per channel stay on the device between two launches
struct nae_dither : BlockHandle {
    nae_dither_params params;
    double* d_state = nullptr;  // [channel][NAE_DITHER_MAX_TAPS]: e[n - 1], e[n - 2], ... in front of the next frame
    int process() override;
};

// the loudness meter's handle ("K14 loudness"): whole chunks of NAE_EQ_CHUNK samples are measured as they fill and leave the FIFO
// (the state carries the 11 samples the true peak reads in front of a chunk); the sub-block energies grow on the device; the flush measures the
// rest and runs the gates.  Nothing comes out of it but the record.
struct nae_loud : StreamHandle {
    nae_loud_params params;
    void* d_block = nullptr;       // the K-weighting's tables and the true-peak taps (nae_loud_make_block)
    void* d_state = nullptr;       // [ch] records of nae_loud_state_bytes() bytes
    nae_loud_result* d_result = nullptr;
    double* d_E = nullptr;         // [e_cap][ch] sub-block energies; grown by doubling, the new part zero
    size_t e_cap = 0, done = 0;    // sub-blocks d_E holds; chunks measured
    int reserve_E(size_t want);
    int process() override;
    ~nae_loud() override { if (d_E) (void)hipFree(d_E); }
};

namespace {

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
        if (!h->carry[i] && (rc = h->dev_alloc(&h->carry[i], (size_t)ch * nae_pv_record_pad(h->opts.n_fft), "hipMalloc(carry)"))) return rc;
    const nae_pv_segment seg{(long long)h->blocks_done, (long long)count, (long long)F_r, limit,
                             h->blocks_done && !forced ? h->carry[h->carry_cur] : nullptr, h->carry[h->carry_cur ^ 1], one_tile};
    rc = nae_launch_pv_phase(ctx, h->run, &pl, &src, src_len, ch, 1, tile, tile, ctx->ws_phase.as<uint32_t>(), &seg);
    if (rc) return rc;
    rc = nae_launch_pv_synth(ctx, h->run, &pl, &src, src_len, ch, 1, tile, tile, ctx->ws_phase.as<uint32_t>(), &dst, &seg, fps);
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
            rc = nae_launch_resample(ctx, &pl, &src, in.total, ch, 1, ctx->rs_tab.as<float>(), &dst, mid.total, J_r);
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
            rc = nae_launch_resample(ctx, &pl, &sv, src_len, ch, 1, ctx->rs_tab.as<float>(), &dv, out.total, J_r);
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

int nae_stretch::process() { return stretch_process(this); }

// the frames that became computable, from the first sample of the next frame on
int nae_spectrum::process()
{
    const size_t start = out.total * (size_t)hop;
    const size_t T = in.total - start;
    const size_t F = nae_spectrum_frames_ex(T, n_fft, hop);
    if (F == 0) return NAE_OK;
    int rc = out.reserve(ctx, out.total + F);
    if (rc) return rc;
    const nae_sig src{in.at(start), 0, 1, (size_t)ch};
    rc = nae_spectrum_block_ex_f32(ctx, n_fft, hop, &src, T, ch, 1, out.at(out.total), 0);
    if (rc) return rc;
    out.total += F;
    // keep the samples the next frame still needs: everything from its start on
    in.drop((long long)(out.total * (size_t)hop));
    return NAE_OK;
}

// the block handles: the unit, the frames that must lie behind a unit, the units of input kept (an overlap-save block's first half), the launch
int nae_fir::process()
{
    return run_units((size_t)n_fft / 2, 0, 1, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_fir(ctx, n_fft, d_spec, &src, in.total, ch, 1, &dst, from, to);
    });
}

int nae_conv::process()
{
    return run_units((size_t)n_fft / 2, 0, 1, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_conv(ctx, n_fft, parts, taps_ch, d_spec, d_ring, ring, &src, in.total, ch, 1, &dst, from, to);
    });
}

int nae_eq::process()
{
    return run_units(NAE_EQ_CHUNK, 0, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_eq(ctx, d_block, n_sections, &src, in.total, ch, 1, &dst, from, to, d_state);
    });
}

int nae_dyn::process()
{
    return run_units(NAE_DYN_CHUNK, (size_t)params.lookahead, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_dyn(ctx, &params, &src, in.total, ch, 1, &dst, from, to, d_state);
    });
}

int nae_dynkey::process()
{
    return run_units(NAE_DYN_CHUNK, (size_t)params.dyn.lookahead, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        // the key's channels stand behind the signal's in every frame
        const nae_sig key{static_cast<float*>(src.base) + ch, src.stream_stride, src.chan_stride, src.frame_stride};
        return nae_launch_dynkey(ctx, &params, d_block, &src, &key, in.total, ch, 1, &dst, from, to, d_state, d_fstate);
    });
}

int nae_echo::process()
{
    return run_units(NAE_EQ_CHUNK, 0, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_echo(ctx, &params, d_block, &src, in.total, ch, 1, &dst, from, to, d_line, d_state);
    });
}

int nae_mod::process()
{
    return run_units(NAE_EQ_CHUNK, 0, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_mod(ctx, &params, &src, in.total, ch, 1, &dst, from, to, d_state);
    });
}

int nae_sat::process()
{
    return run_units(NAE_EQ_CHUNK, 0, 1, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_sat(ctx, &params, &src, in.total, ch, 1, &dst, from, to);
    });
}

int nae_gate::process()
{
    return run_units(NAE_DYN_CHUNK, (size_t)params.lookahead, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_gate(ctx, &params, &src, in.total, ch, 1, &dst, from, to, d_state);
    });
}

int nae_mb::process()
{
    return run_units(NAE_DYN_CHUNK, (size_t)params.band[0].lookahead, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_mb_run(ctx, &params, d_block, &src, in.total, ch, 1, &dst, from, to, d_planes, slab, d_state);
    });
}

int nae_denoise::process()
{
    const size_t H = (size_t)params.n_fft / 4, reach = (size_t)params.time_smooth + 3;
    return run_units(H, reach * H, reach, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_denoise(ctx, &params, d_profile, profile_ch, &src, in.total, ch, 1, &dst, from, to);
    });
}

int nae_lim::process()
{
    return run_units(NAE_DYN_CHUNK, nae_lim_wait(&params), 1, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_lim(ctx, &params, &src, in.total, ch, 1, &dst, from, to, d_state);
    });
}

int nae_dither::process()
{
    return run_units(1, 0, 0, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_dither(ctx, &params, &src, ch, 1, &dst, from, to, d_state);
    });
}

int nae_hpss::process()
{
    const size_t H = (size_t)params.n_fft / 4, reach = (size_t)params.time_span + 3;
    return run_units(H, reach * H, reach, [&](const nae_sig& src, const nae_sig& dst, size_t from, size_t to) {
        return nae_launch_hpss(ctx, &params, &src, in.total, ch, 1, &dst, from, to);
    });
}

int nae_loud::reserve_E(size_t want)
{
    if (want <= e_cap) return NAE_OK;
    size_t cap = e_cap ? e_cap : 1024;
    while (cap < want) cap *= 2;
    double* np = nullptr;
    if (hipMalloc((void**)&np, cap * ch * sizeof(double)) != hipSuccess) return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(loud sub-blocks)");
    hipError_t e = hipMemsetAsync(np, 0, cap * ch * sizeof(double), ctx->stream);
    if (e == hipSuccess && d_E) e = hipMemcpyAsync(np, d_E, e_cap * ch * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(np);
        return nae_check(ctx, e, "loud: sub-block array");
    }
    if (d_E) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_E);
    }
    d_E = np;
    e_cap = cap;
    return NAE_OK;
}

int nae_loud::process()
{
    const size_t ready = nae_loud_chunks(in.total, flushed);
    if (ready > done) {
        // every sub-block the chunks up to `ready` meet has its entry
        int rc = reserve_E(ready * NAE_EQ_CHUNK / (size_t)params.sub_block + 1);
        if (rc) return rc;
        const nae_sig src = in.view();
        rc = nae_launch_loud_measure(ctx, &params, d_block, &src, in.total, ch, 1, done, ready, d_state, d_E, e_cap * ch, e_cap);
        if (rc) return rc;
        done = ready;
        in.drop((long long)(ready * NAE_EQ_CHUNK));
    }
    if (!flushed) return NAE_OK;
    const int rc = reserve_E(1);
    return rc ? rc : nae_launch_loud_gate(ctx, &params, in.total, ch, 1, d_state, d_E, e_cap * ch, d_result);
}

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
    nae_stretch* s = handle_new<nae_stretch>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->sample_rate = sample_rate;
    s->rate = rate;
    s->pitch = pitch;
    s->opts = o;
    s->pl = pl;
    s->run = nae_pv_resolve(o, pl, channels);
    s->mid.width = (size_t)channels;
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

int nae_stretch_put(nae_stretch* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_stretch_put_host(nae_stretch* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, true); }
// flush: everything still buffered is transformed as if the input ended here (zero padding behind the last sample);
// the samples delivered over the handle's life equal nae_stretch_block_f32 on the whole input, bit for bit
int nae_stretch_flush(nae_stretch* h) { return handle_flush(h); }
size_t nae_stretch_available(nae_stretch* h) { return handle_available(h); }
int nae_stretch_receive(nae_stretch* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_stretch_receive_host(nae_stretch* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, true); }
int nae_stretch_destroy(nae_stretch* h) { return handle_destroy(h); }

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
    nae_spectrum* s = handle_new<nae_spectrum>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->n_fft = n_fft;
    s->hop = hop;
    s->out.width = (size_t)channels * (size_t)(n_fft / 2 + 1);
    *h = s;
    return NAE_OK;
}

int nae_spectrum_put(nae_spectrum* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
size_t nae_spectrum_available(nae_spectrum* h) { return handle_available(h); }
int nae_spectrum_receive(nae_spectrum* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_spectrum_destroy(nae_spectrum* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ FIR filter
int nae_fir_create(nae_ctx* ctx, const float* taps_host, int n_taps, int n_fft, int channels, nae_fir** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    if (!taps_host) return nae_fail(ctx, NAE_ERR_INVALID, "fir: null pointer");
    int rc = nae_fir_check(ctx, n_taps, channels, &n_fft);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_fir* s = handle_new<nae_fir>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->n_fft = n_fft;
    s->flush_tail = (size_t)n_taps - 1;
    rc = s->dev_alloc(&s->d_spec, nae_fir_spec_floats(n_fft), "hipMalloc(fir spectrum)");
    if (!rc) rc = nae_fir_make_spec(ctx, taps_host, n_taps, n_fft, s->d_spec);
    return handle_created(s, rc, h);
}

int nae_fir_put(nae_fir* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_fir_put_host(nae_fir* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: n_taps - 1 zero frames behind the input: the tail of the convolution comes out, in_len + n_taps - 1 frames over the handle's life
int nae_fir_flush(nae_fir* h) { return handle_flush(h); }
size_t nae_fir_available(nae_fir* h) { return handle_available(h); }
int nae_fir_receive(nae_fir* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_fir_receive_host(nae_fir* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_fir_destroy(nae_fir* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ long convolution
int nae_conv_create(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, int channels, nae_conv** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    if (!taps_host) return nae_fail(ctx, NAE_ERR_INVALID, "conv: null pointer");
    int rc = nae_conv_check(ctx, n_taps, taps_ch, channels, &n_fft);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_conv* s = handle_new<nae_conv>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->n_fft = n_fft;
    s->flush_tail = (size_t)n_taps - 1;
    s->taps_ch = taps_ch;
    s->parts = nae_conv_parts(n_taps, n_fft);
    s->ring = nae_pick_conv_ring(ctx, n_fft, s->parts, NAE_CONV_HANDLE_SLAB, (size_t)channels);
    rc = s->dev_alloc(&s->d_spec, nae_conv_spec_floats(n_fft, s->parts, taps_ch), "hipMalloc(conv spectra)");
    if (!rc) rc = s->dev_alloc(&s->d_ring, nae_conv_ring_floats(n_fft, (size_t)channels, s->ring), "hipMalloc(conv spectra)");
    if (!rc) rc = nae_conv_make_spec(ctx, taps_host, n_taps, taps_ch, n_fft, s->d_spec);
    return handle_created(s, rc, h);
}

int nae_conv_put(nae_conv* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_conv_put_host(nae_conv* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: as the FIR filter's
int nae_conv_flush(nae_conv* h) { return handle_flush(h); }
size_t nae_conv_available(nae_conv* h) { return handle_available(h); }
int nae_conv_receive(nae_conv* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_conv_receive_host(nae_conv* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_conv_destroy(nae_conv* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ biquad cascade
int nae_eq_create(nae_ctx* ctx, const double* coef_host, int n_sections, int channels, nae_eq** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_eq_check(ctx, coef_host, n_sections, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_eq* s = handle_new<nae_eq>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->n_sections = n_sections;
    const size_t state_doubles = (size_t)channels * NAE_EQ_MAX_SECTIONS * 2;
    rc = s->dev_alloc(&s->d_block, nae_eq_block_doubles(), "hipMalloc(eq tables)");
    if (!rc) rc = s->dev_alloc(&s->d_state, state_doubles, "hipMalloc(eq tables)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(eq state)");
    if (!rc) rc = nae_eq_make_block(ctx, coef_host, n_sections, s->d_block);
    return handle_created(s, rc, h);
}

int nae_eq_put(nae_eq* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_eq_put_host(nae_eq* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the partial last chunk comes out: as many frames as were put over the handle's life (an IIR has no tail to append)
int nae_eq_flush(nae_eq* h) { return handle_flush(h); }
size_t nae_eq_available(nae_eq* h) { return handle_available(h); }
int nae_eq_receive(nae_eq* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_eq_receive_host(nae_eq* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_eq_destroy(nae_eq* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ dynamics
int nae_dyn_create(nae_ctx* ctx, const nae_dyn_params* params, int channels, nae_dyn** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_dyn_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_dyn* s = handle_new<nae_dyn>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    const size_t state_doubles = nae_dyn_detectors(params, channels, 1) * 2;
    rc = s->dev_alloc(&s->d_state, state_doubles, "hipMalloc(dyn state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(dyn state)");
    return handle_created(s, rc, h);
}

int nae_dyn_put(nae_dyn* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_dyn_put_host(nae_dyn* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the chunks that waited for their look-ahead and the partial last one come out: as many frames as were put over the handle's life
int nae_dyn_flush(nae_dyn* h) { return handle_flush(h); }
size_t nae_dyn_available(nae_dyn* h) { return handle_available(h); }
int nae_dyn_receive(nae_dyn* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_dyn_receive_host(nae_dyn* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_dyn_destroy(nae_dyn* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ keyed dynamics
int nae_dynkey_create(nae_ctx* ctx, const nae_dynkey_params* params, int channels, nae_dynkey** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_dynkey_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_dynkey* s = handle_new<nae_dynkey>(ctx, channels, params->key_ch);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    const size_t state_doubles = nae_dyn_detectors(&params->dyn, channels, 1) * 2, filter_doubles = nae_dynkey_filter_doubles(params, channels, 1);
    rc = s->dev_alloc(&s->d_state, state_doubles, "hipMalloc(dynkey state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(dynkey state)");
    if (!rc && params->n_sections) {
        rc = s->dev_alloc(&s->d_fstate, filter_doubles, "hipMalloc(dynkey state)");
        if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_fstate, 0, filter_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(dynkey state)");
        if (!rc) rc = s->dev_alloc(&s->d_block, nae_eq_block_doubles(), "hipMalloc(dynkey tables)");
        if (!rc) rc = nae_eq_make_block(ctx, &params->coef[0][0], params->n_sections, s->d_block);
    }
    return handle_created(s, rc, h);
}

int nae_dynkey_put(nae_dynkey* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_dynkey_put_host(nae_dynkey* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: as nae_dyn's
int nae_dynkey_flush(nae_dynkey* h) { return handle_flush(h); }
size_t nae_dynkey_available(nae_dynkey* h) { return handle_available(h); }
int nae_dynkey_receive(nae_dynkey* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_dynkey_receive_host(nae_dynkey* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_dynkey_destroy(nae_dynkey* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ echo
int nae_echo_create(nae_ctx* ctx, const nae_echo_params* params, int channels, nae_echo** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_echo_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_echo* s = handle_new<nae_echo>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    const size_t state_doubles = (size_t)channels * NAE_ECHO_MAX_SECTIONS * 2;
    // the lines are not cleared: sample n - D of a line is read only once it has been written
    rc = s->dev_alloc(&s->d_line, (size_t)channels * nae_echo_ring(params, channels), "hipMalloc(echo lines)");
    if (!rc) rc = s->dev_alloc(&s->d_state, state_doubles, "hipMalloc(echo state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(echo state)");
    if (!rc && params->n_sections) {
        rc = s->dev_alloc(&s->d_block, nae_eq_block_doubles(), "hipMalloc(echo tables)");
        if (!rc) rc = nae_eq_make_block(ctx, &params->coef[0][0], params->n_sections, s->d_block);
    }
    return handle_created(s, rc, h);
}

int nae_echo_put(nae_echo* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_echo_put_host(nae_echo* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the partial last chunk comes out: as many frames as were put over the handle's life (the echoes' tail is dropped: flush_tail = 0)
int nae_echo_flush(nae_echo* h) { return handle_flush(h); }
size_t nae_echo_available(nae_echo* h) { return handle_available(h); }
int nae_echo_receive(nae_echo* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_echo_receive_host(nae_echo* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_echo_destroy(nae_echo* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ modulated delay
int nae_mod_create(nae_ctx* ctx, const nae_mod_params* params, int channels, nae_mod** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_mod_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_mod* s = handle_new<nae_mod>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    // the line in front of the stream's first sample is zero
    const size_t state_floats = (size_t)channels * NAE_MOD_KEEP;
    rc = s->dev_alloc(&s->d_state, state_floats, "hipMalloc(mod lines)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_floats * sizeof(float), ctx->stream), "hipMemsetAsync(mod lines)");
    return handle_created(s, rc, h);
}

int nae_mod_put(nae_mod* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_mod_put_host(nae_mod* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the partial last chunk comes out: as many frames as were put over the handle's life (the tail is dropped: flush_tail = 0)
int nae_mod_flush(nae_mod* h) { return handle_flush(h); }
size_t nae_mod_available(nae_mod* h) { return handle_available(h); }
int nae_mod_receive(nae_mod* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_mod_receive_host(nae_mod* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_mod_destroy(nae_mod* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ saturation
int nae_sat_create(nae_ctx* ctx, const nae_sat_params* params, int channels, nae_sat** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    const int rc = nae_sat_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_sat* s = handle_new<nae_sat>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    s->flush_tail = (size_t)nae_sat_latency(params->oversample);
    return handle_created(s, NAE_OK, h);
}

int nae_sat_put(nae_sat* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_sat_put_host(nae_sat* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the latency's zero frames go in behind the input and the partial last chunk comes out: in_len + D frames over the handle's life
int nae_sat_flush(nae_sat* h) { return handle_flush(h); }
size_t nae_sat_available(nae_sat* h) { return handle_available(h); }
int nae_sat_receive(nae_sat* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_sat_receive_host(nae_sat* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_sat_destroy(nae_sat* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ gate
int nae_gate_create(nae_ctx* ctx, const nae_gate_params* params, int channels, nae_gate** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_gate_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_gate* s = handle_new<nae_gate>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    // in front of sample 0: closed, no set sample, and the y an endless silence leaves
    long long first[2][3];
    const size_t n_det = nae_gate_detectors(params, channels, 1);
    for (size_t d = 0; d < n_det; d++) {
        first[d][0] = 0;
        first[d][1] = -1;
        memcpy(&first[d][2], &params->range_db, sizeof(double));
    }
    rc = s->dev_alloc(&s->d_state, n_det * 3, "hipMalloc(gate state)");
    if (!rc) rc = nae_check(ctx, hipMemcpyAsync(s->d_state, first, n_det * 3 * sizeof(long long), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(gate state)");
    if (!rc) rc = nae_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(gate state)");   // `first` is this call's
    return handle_created(s, rc, h);
}

int nae_gate_put(nae_gate* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_gate_put_host(nae_gate* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the chunks that waited for their look-ahead and the partial last one come out: as many frames as were put over the handle's life
int nae_gate_flush(nae_gate* h) { return handle_flush(h); }
size_t nae_gate_available(nae_gate* h) { return handle_available(h); }
int nae_gate_receive(nae_gate* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_gate_receive_host(nae_gate* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_gate_destroy(nae_gate* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ multiband
int nae_mb_create(nae_ctx* ctx, const nae_mb_params* params, int channels, nae_mb** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_mb_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_mb* s = handle_new<nae_mb>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    s->slab = nae_mb_handle_slab(ctx);
    // in front of sample 0 every carry is zero; the planes are written before they are read
    const size_t state_doubles = nae_mb_state_doubles(params, channels, 1);
    rc = s->dev_alloc(&s->d_state, state_doubles, "hipMalloc(mb state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_doubles * sizeof(double), ctx->stream), "hipMemsetAsync(mb state)");
    if (!rc) rc = s->dev_alloc(&s->d_planes, nae_mb_plane_floats(params, channels, 1, s->slab), "hipMalloc(mb planes)");
    if (!rc) rc = s->dev_alloc(&s->d_block, nae_eq_block_doubles(), "hipMalloc(mb tables)");
    if (!rc) rc = nae_eq_make_block(ctx, &params->coef[0][0], params->n_sections, s->d_block);
    return handle_created(s, rc, h);
}

int nae_mb_put(nae_mb* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_mb_put_host(nae_mb* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the chunks that waited for their look-ahead and the partial last one come out: as many frames as were put over the handle's life
int nae_mb_flush(nae_mb* h) { return handle_flush(h); }
size_t nae_mb_available(nae_mb* h) { return handle_available(h); }
int nae_mb_receive(nae_mb* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_mb_receive_host(nae_mb* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_mb_destroy(nae_mb* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ spectral gate
int nae_denoise_create(nae_ctx* ctx, const nae_denoise_params* params, const float* profile_dev, int profile_ch, int channels, nae_denoise** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_denoise_check(ctx, params, profile_dev, profile_ch, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_denoise* s = handle_new<nae_denoise>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    s->profile_ch = profile_ch;
    const size_t floats = (size_t)profile_ch * ((size_t)params->n_fft / 2 + 1);
    rc = s->dev_alloc(&s->d_profile, floats, "hipMalloc(denoise profile)");
    if (!rc) rc = nae_check(ctx, hipMemcpyAsync(s->d_profile, profile_dev, floats * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream),
                            "hipMemcpyAsync(denoise profile)");
    return handle_created(s, rc, h);
}

int nae_denoise_put(nae_denoise* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_denoise_put_host(nae_denoise* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
int nae_denoise_flush(nae_denoise* h) { return handle_flush(h); }
size_t nae_denoise_available(nae_denoise* h) { return handle_available(h); }
int nae_denoise_receive(nae_denoise* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_denoise_receive_host(nae_denoise* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_denoise_destroy(nae_denoise* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ separation
int nae_hpss_create(nae_ctx* ctx, const nae_hpss_params* params, int channels, nae_hpss** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    const int rc = nae_hpss_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_hpss* s = handle_new<nae_hpss>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    return handle_created(s, NAE_OK, h);
}

int nae_hpss_put(nae_hpss* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_hpss_put_host(nae_hpss* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
int nae_hpss_flush(nae_hpss* h) { return handle_flush(h); }
size_t nae_hpss_available(nae_hpss* h) { return handle_available(h); }
int nae_hpss_receive(nae_hpss* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_hpss_receive_host(nae_hpss* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_hpss_destroy(nae_hpss* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ limiter
int nae_lim_create(nae_ctx* ctx, const nae_lim_params* params, int channels, nae_lim** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_lim_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_lim* s = handle_new<nae_lim>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    // in front of sample 0: y1 = 0 and nothing summed; the prefix sums are made at chunk 0
    const size_t words = nae_lim_detectors(params, channels, 1) * nae_lim_state_words();
    rc = s->dev_alloc(&s->d_state, words, "hipMalloc(lim state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, words * sizeof(unsigned long long), ctx->stream), "hipMemsetAsync(lim state)");
    return handle_created(s, rc, h);
}

int nae_lim_put(nae_lim* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_lim_put_host(nae_lim* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the chunks that waited for their look-ahead and the partial last one come out: as many frames as were put over the handle's life
int nae_lim_flush(nae_lim* h) { return handle_flush(h); }
size_t nae_lim_available(nae_lim* h) { return handle_available(h); }
int nae_lim_receive(nae_lim* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_lim_receive_host(nae_lim* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_lim_destroy(nae_lim* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ dither
int nae_dither_create(nae_ctx* ctx, const nae_dither_params* params, int channels, nae_dither** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_dither_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_dither* s = handle_new<nae_dither>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    // in front of sample 0 every error is zero
    const size_t words = (size_t)channels * NAE_DITHER_MAX_TAPS;
    rc = s->dev_alloc(&s->d_state, words, "hipMalloc(dither state)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, words * sizeof(double), ctx->stream), "hipMemsetAsync(dither state)");
    return handle_created(s, rc, h);
}

int nae_dither_put(nae_dither* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_dither_put_host(nae_dither* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: nothing was held back; from here on a put is refused
int nae_dither_flush(nae_dither* h) { return handle_flush(h); }
size_t nae_dither_available(nae_dither* h) { return handle_available(h); }
int nae_dither_receive(nae_dither* h, float* dst, size_t max_frames, size_t* got) { return handle_take(h, dst, max_frames, got, false); }
int nae_dither_receive_host(nae_dither* h, float* dst_host, size_t max_frames, size_t* got) { return handle_take(h, dst_host, max_frames, got, true); }
int nae_dither_destroy(nae_dither* h) { return handle_destroy(h); }

// ------------------------------------------------------------------------------------------------ loudness
int nae_loud_create(nae_ctx* ctx, const nae_loud_params* params, int channels, nae_loud** h)
{
    if (!ctx || !h) return NAE_ERR_INVALID;
    *h = nullptr;
    int rc = nae_loud_check(ctx, params, channels);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    nae_loud* s = handle_new<nae_loud>(ctx, channels);
    if (!s) return NAE_ERR_NOMEM;
    s->params = *params;
    const size_t state_bytes = (size_t)channels * nae_loud_state_bytes();
    rc = s->dev_alloc((char**)&s->d_block, nae_loud_block_bytes(), "hipMalloc(loud tables)");
    if (!rc) rc = s->dev_alloc((char**)&s->d_state, state_bytes, "hipMalloc(loud state)");
    if (!rc) rc = s->dev_alloc(&s->d_result, 1, "hipMalloc(loud record)");
    if (!rc) rc = nae_check(ctx, hipMemsetAsync(s->d_state, 0, state_bytes, ctx->stream), "hipMemsetAsync(loud state)");
    if (!rc) rc = nae_loud_make_block(ctx, params, s->d_block);
    return handle_created(s, rc, h);
}

int nae_loud_put(nae_loud* h, const float* interleaved, size_t S) { return handle_append(h, interleaved, S, false); }
int nae_loud_put_host(nae_loud* h, const float* interleaved_host, size_t S) { return handle_append(h, interleaved_host, S, true); }
// flush: the partial last chunk, and one more where the true peak's tail reaches past it, are measured; the gates run
int nae_loud_flush(nae_loud* h) { return handle_flush(h); }
int nae_loud_destroy(nae_loud* h) { return handle_destroy(h); }

int nae_loud_get_result(nae_loud* h, nae_loud_result* out_host)
{
    if (!h || !out_host) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (!h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "result before flush");
    hipError_t e = hipMemcpyAsync(out_host, h->d_result, sizeof(nae_loud_result), hipMemcpyDeviceToHost, h->ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->ctx->stream);
    return e == hipSuccess ? NAE_OK : nae_check(h->ctx, e, "loud: result download");
}

} // extern "C"
