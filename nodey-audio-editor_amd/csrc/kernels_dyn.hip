// kernels_dyn.hip — K12, the dynamics processor ("K12 dynamics") for gfx950: a feed-forward compressor / look-ahead limiter in the
// dB domain, its two recurrences computed parallel in time.
//
// One wave per detector walks its chunks in order.  A detector is a stream-channel, or with `link` a stereo stream: the wave then reads and
// writes both channels (DC = 2).  The walk and every step of it stand in dyn_steps.h, which the keyed dynamics (kernels_dynkey.hip) run too:
// here the magnitude the detector reads is the signal's own.  Built with -ffp-contract=off: every step is one IEEE operation in the order of
// the CPU statement (tests/dyn_ref/ref_dyn.c).
#include "dyn_steps.h"
#include <math.h>
#include <string.h>

namespace nae {

// state: [n_det][2] doubles, the carries (y1, yl) in front of chunk c_origin, replaced by the ones behind chunk c_stop - 1; null: zero in,
// nothing out (the block call)
template <int DC>
__global__ __launch_bounds__(64) void dyn_kernel(SigViewD src, OutViewD out, DynParams p, double* state)
{
    const int lane = threadIdx.x;
    const long long det = blockIdx.x;
    if (det >= p.n_det) return;
    // DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`
    const long long s_idx = DC == 2 ? det : det / p.ch;
    const int c0 = DC == 2 ? 0 : (int)(det % p.ch);
    const float* ip = src.base + s_idx * src.ss + c0 * src.cs;
    float* op = out.base + s_idx * out.ss + c0 * out.cs;
    DynPlainKey<DC> mag{ip, src, p, lane};
    dyn_walk<DC>(ip, op, src, out, p, state, det, lane, mag);
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_dyn_block_f32 and nae_dyn_create (ctx may be null: no message then)
int nae_dyn_check(nae_ctx* ctx, const nae_dyn_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->threshold_db) || !isfinite(p->slope) || !isfinite(p->knee_db) || !isfinite(p->alpha_attack) || !isfinite(p->alpha_release) ||
        !isfinite(p->makeup_db))
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: non-finite parameter");
    if (p->threshold_db < NAE_DYN_MIN_THRESHOLD_DB || p->threshold_db > NAE_DYN_MAX_THRESHOLD_DB)
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: threshold_db outside -60 ... 0");
    if (p->slope < 0.0 || p->slope > 1.0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: slope outside 0 ... 1");
    if (p->knee_db < 0.0 || p->knee_db > NAE_DYN_MAX_KNEE_DB) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: knee_db outside 0 ... 24");
    if (p->alpha_attack < 0.0 || p->alpha_attack >= 1.0 || p->alpha_release < 0.0 || p->alpha_release >= 1.0)
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: alpha outside [0, 1)");
    if (p->makeup_db < -NAE_DYN_MAX_MAKEUP_DB || p->makeup_db > NAE_DYN_MAX_MAKEUP_DB) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: makeup_db outside -24 ... 24");
    if (p->lookahead < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: negative lookahead");
    if (p->link != 0 && p->link != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dyn: link must be 0 or 1");
    if (p->lookahead > NAE_DYN_MAX_LOOKAHEAD) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "dyn: lookahead above 1024 samples");
    return NAE_OK;
}

size_t nae_dyn_detectors(const nae_dyn_params* p, int ch, size_t n_streams) { return p->link && ch == 2 ? n_streams : n_streams * (size_t)ch; }

// the launch record of chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples: K12's, and K15's
DynParams nae_dyn_launch_params(const nae_dyn_params* dp, size_t in_len, int ch, size_t n_streams, size_t c_origin, size_t c_stop)
{
    DynParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_det = (long long)nae_dyn_detectors(dp, ch, n_streams);
    p.v[kDynThr] = dp->threshold_db;
    p.v[kDynSlope] = dp->slope;
    p.v[kDynKnee] = dp->knee_db;
    p.v[kDynHalfKnee] = dp->knee_db / 2.0;
    p.v[kDynInv2Knee] = dp->knee_db > 0.0 ? 1.0 / (2.0 * dp->knee_db) : 0.0;
    p.v[kDynAa] = dp->alpha_attack;
    p.v[kDynOma] = 1.0 - dp->alpha_attack;
    p.v[kDynAr] = dp->alpha_release;
    p.v[kDynOmr] = 1.0 - dp->alpha_release;
    p.v[kDynMakeup] = dp->makeup_db;
    p.ch = ch;
    p.la = dp->lookahead;
    return p;
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_dyn(nae_ctx* ctx, const nae_dyn_params* dp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, double* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    const DynParams p = nae_dyn_launch_params(dp, in_len, ch, n_streams, c_origin, c_stop);
    // one wave per detector
    return with_flags(dp->link && ch == 2, [&](auto linked) {
        return nae_launch_tiles(ctx, "dyn_kernel", "dyn_kernel: grid too large", dyn_kernel<linked.value ? 2 : 1>, p.n_det, 1, 64, 0, to_view(src),
                                to_out(dst), p, d_state);
    });
}

extern "C" {

int nae_dyn_block_f32(nae_ctx* ctx, const nae_dyn_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "dyn: null pointer");
    const int rc = nae_dyn_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "dyn: null pointer");
    return nae_launch_dyn(ctx, params, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr);
}

// DESIGN.md §3, "K12 dynamics", "Design"
int nae_dyn_design(int sample_rate, double threshold_db, double ratio, double knee_db, double attack_s, double release_s, double lookahead_s,
                   double makeup_db, int link, nae_dyn_params* out)
{
    if (!out || sample_rate <= 0 || (link != 0 && link != 1)) return NAE_ERR_INVALID;
    if (!isfinite(threshold_db) || isnan(ratio) || !isfinite(knee_db) || !isfinite(attack_s) || !isfinite(release_s) || !isfinite(lookahead_s) ||
        !isfinite(makeup_db))
        return NAE_ERR_INVALID;
    if (threshold_db < NAE_DYN_MIN_THRESHOLD_DB || threshold_db > NAE_DYN_MAX_THRESHOLD_DB || ratio < 1.0 || knee_db < 0.0 || knee_db > NAE_DYN_MAX_KNEE_DB ||
        attack_s < 0.0 || attack_s > NAE_DYN_MAX_ATTACK_S || release_s < NAE_DYN_MIN_RELEASE_S || release_s > NAE_DYN_MAX_RELEASE_S ||
        makeup_db < -NAE_DYN_MAX_MAKEUP_DB || makeup_db > NAE_DYN_MAX_MAKEUP_DB || lookahead_s < 0.0)
        return NAE_ERR_INVALID;
    const double la = lookahead_s * (double)sample_rate;
    if (la > 2.0 * (double)NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    const long n = lround(la);
    if (n > NAE_DYN_MAX_LOOKAHEAD) return NAE_ERR_UNSUPPORTED;
    out->threshold_db = threshold_db;
    out->slope = isinf(ratio) ? 1.0 : 1.0 - 1.0 / ratio;
    out->knee_db = knee_db;
    out->alpha_attack = attack_s > 0.0 ? exp(-1.0 / (attack_s * (double)sample_rate)) : 0.0;
    out->alpha_release = exp(-1.0 / (release_s * (double)sample_rate));
    out->makeup_db = makeup_db;
    out->lookahead = (int)n;
    out->link = link;
    return NAE_OK;
}

} // extern "C"
