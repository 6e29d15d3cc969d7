// kernels_mod.hip — K17, the modulated delay ("K17 modulated delay") for gfx950: chorus, flanger and vibrato.  One short delay
// d(n) = delay + depth l(n) whose length an LFO sweeps, read between samples by 4-point Lagrange interpolation, up to four voices of the one
// LFO at different phases, and feedback into the line.
//
// The shortest delay is floor(delay - depth) = kmin >= 2, and the newest line sample a tap of sample n reads is n - k + 1: a run of
// L = kmin - 1 consecutive samples reads only line samples in front of the run.  So the loop needs no scan: L lanes compute L samples in
// parallel, and the runs go in order.  Without feedback the line is the input and any L holds (64).  No sample's arithmetic depends on L.
// One wave per stream-channel (the channels do not interact: no workgroup barrier).  The line lives in LDS as a ring of 4096 floats addressed
// by the absolute sample index mod 4096: one chunk of 1024 samples and the deepest reach, floor(d) + 2 <= 3072, in front of it.  Per chunk the
// wave issues its 16 coalesced input loads together, from addresses clamped into the signal, into the ring at the samples' own places — where
// the line's samples [n0 - 4096, n0 - 3072) stood, which no tap reads any more — and walks the chunk in runs of L: lane j < L computes the
// voices' phases and delays, reads four ring words per voice, forms the tap, writes w over its own x in the ring (with feedback only: without,
// w is x) and stores y, the run's lanes together (an LDS stage of one chunk in front of 16 coalesced stores was measured too:
// profiles/r23_mod.md).  Between two runs the wave's LDS writes are ordered in front of its next reads (chunk_lds_sync).
// Samples in front of the stream's first read as zero: the 3072 ring words in front of the first chunk are filled from the handle's state, or
// with zeros, before the first load.
// The translation unit is built with -ffp-contract=off: every step is one IEEE operation, in the order of tests/mod_ref/ref_mod.c.
#include "chunk_stage.h"
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kModRing = 4096, kModKeep = (int)NAE_MOD_KEEP;
// LDS words behind the ring that no lane touches: 20 KiB per wave hold a CU's 160 KiB to eight waves.  With the ring alone a CU admits ten,
// 2048 waves (1024 stereo streams) then land ten on some CUs and fewer on others, and the launch ends with the fullest: the default chorus
// measured 9.3 ms in most rounds and 7.4 in some, against 7.2 ... 7.3 in all with eight (profiles/r23_mod.md)
constexpr int kModHold = 1024;
static_assert(kModKeep + kChunkC == kModRing && (double)kModKeep == NAE_MOD_MAX_DELAY + 2.0, "the ring holds one chunk and the deepest reach, floor(d) + 2");

struct ModParams {
    long long in_len;      // samples of a stream-channel: samples at or past in_len are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_waves;     // stream-channels: one wave each
    double delay, depth, g, wet, dry, inv;
    unsigned rate_inc, phase0, phase_ch;
    unsigned voice_phase[NAE_MOD_MAX_VOICES];
    int ch, n_voices, shape;
    int sub;               // L: samples of a run, 1 ... 64
};

// the LFO at phase phi (turns 2^32): the corrected parabola, or the triangle
__device__ __forceinline__ double mod_lfo(int shape, unsigned phi)
{
    const double t = (double)(int)phi * 0x1p-31;
    if (shape == NAE_MOD_SINE) {
        const double y = (4.0 * t) * (1.0 - fabs(t));
        return (0.225 * ((y * fabs(y)) - y)) + y;
    }
    return (2.0 * fabs(t)) - 1.0;
}

// state: [n_waves][kModKeep] floats, the line's samples [1024 c_origin - 3072, 1024 c_origin), replaced by those in front of chunk c_stop;
// null: zero in, nothing out (the block call)
__global__ __launch_bounds__(64) void mod_kernel(SigViewD src, OutViewD out, ModParams p, float* state)
{
    __shared__ float ring[kModRing + kModHold];
    const int lane = threadIdx.x;
    const long long sc = blockIdx.x;
    if (sc >= p.n_waves) return;
    const long long s_idx = sc / p.ch;
    const int c = (int)(sc - s_idx * p.ch);
    const float* ip = src.base + s_idx * src.ss + c * src.cs;
    float* op = out.base + s_idx * out.ss + c * out.cs;
    const double g = p.g, wet = p.wet, dry = p.dry, inv = p.inv;
    const bool loop = g != 0.0;
    const int L = p.sub, nv = p.n_voices, shape = p.shape;
    const unsigned rate_inc = p.rate_inc;
    unsigned vph[NAE_MOD_MAX_VOICES];
#pragma unroll
    for (int v = 0; v < NAE_MOD_MAX_VOICES; v++) vph[v] = p.phase0 + p.voice_phase[v] + (c == 1 ? p.phase_ch : 0u);

    // the line in front of the first chunk (its indices may be negative: the mask is the index mod 4096 all the same)
    {
        const long long first = p.c_origin * kChunkC - kModKeep;
        for (int j = lane; j < kModKeep; j += 64) ring[(int)((first + j) & (kModRing - 1))] = state ? state[sc * kModKeep + j] : 0.0f;
    }
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        const int slot0 = (int)(n0 & (kModRing - 1));              // a multiple of the chunk: [slot0, slot0 + 1024) does not wrap
        // every load is issued whatever the sample's place, from an address inside the signal, and what lies past in_len is dropped behind it:
        // 16 loads in flight, not 16 branches that each wait for their own
#pragma unroll
        for (int j = 0; j < kChunkT; j++) {
            const int i = j * 64 + lane;
            const long long gi = n0 + i;
            const bool in = gi < p.in_len;
            const float xv = ip[(in ? gi : p.in_len - 1) * src.fs];
            ring[slot0 + i] = in ? xv : 0.0f;
        }
        chunk_lds_sync();
#pragma unroll 1
        for (int r = 0; r < kChunkC; r += L) {
            const int i = r + lane;
            if (lane < L && i < kChunkC) {
                const long long gi = n0 + i;
                const double xd = (double)ring[slot0 + i];
                const unsigned turn = (unsigned)gi * rate_inc;     // the low 32 bits of n rate_inc
                double sum = 0.0;
#pragma unroll
                for (int v = 0; v < NAE_MOD_MAX_VOICES; v++) {
                    if (v < nv) {
                        const double l = mod_lfo(shape, vph[v] + turn);
                        const double d = p.delay + (p.depth * l);
                        const double kf = floor(d);
                        const double f = d - kf;
                        const unsigned at = (unsigned)gi - (unsigned)(int)kf;   // n - k mod 2^32: its low 12 bits are the ring's address
                        const double a = (double)ring[(at + 1u) & (kModRing - 1)], b = (double)ring[at & (kModRing - 1)];
                        const double c2 = (double)ring[(at - 1u) & (kModRing - 1)], e = (double)ring[(at - 2u) & (kModRing - 1)];
                        const double fm1 = f - 1.0, fm2 = f - 2.0, fp1 = f + 1.0;
                        const double ca = ((-(f * fm1)) * fm2) * (1.0 / 6.0);
                        const double cb = ((fp1 * fm1) * fm2) * 0.5;
                        const double cc = ((-(fp1 * f)) * fm2) * 0.5;
                        const double ce = ((fp1 * f) * fm1) * (1.0 / 6.0);
                        const double tap = (((ca * a) + (cb * b)) + (cc * c2)) + (ce * e);
                        sum = v == 0 ? tap : sum + tap;
                    }
                }
                const double u = sum * inv;
                if (loop) ring[slot0 + i] = (float)(xd + (g * u));
                const float y = (float)((dry * xd) + (wet * u));
                if (gi < p.in_len) op[gi * out.fs] = y;
            }
            // this run's line samples before the next run's taps; without feedback the ring holds the input and no run writes it
            if (loop) chunk_lds_sync();
        }
    }
    if (state) {
        chunk_lds_sync();
        const long long first = p.c_stop * kChunkC - kModKeep;
        for (int j = lane; j < kModKeep; j += 64) state[sc * kModKeep + j] = ring[(int)((first + j) & (kModRing - 1))];
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_mod_block_f32 and nae_mod_create (ctx may be null: no message then)
int nae_mod_check(nae_ctx* ctx, const nae_mod_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->delay) || !isfinite(p->depth) || !isfinite(p->feedback) || !isfinite(p->wet) || !isfinite(p->dry))
        return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: non-finite parameter");
    if (!(fabs(p->feedback) <= NAE_MOD_MAX_FEEDBACK)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: |feedback| above 0.95");
    if (p->depth < 0.0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: negative depth");
    if (p->n_voices < 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: n_voices below 1");
    if (p->shape != NAE_MOD_SINE && p->shape != NAE_MOD_TRIANGLE) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mod: unknown shape");
    if (p->n_voices > NAE_MOD_MAX_VOICES) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "mod: at most 4 voices");
    if (!(p->delay - p->depth >= NAE_MOD_MIN_DELAY) || !(p->delay + p->depth <= NAE_MOD_MAX_DELAY))
        return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "mod: delay - depth must be at least 2 and delay + depth at most 3070 samples");
    return NAE_OK;
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_mod(nae_ctx* ctx, const nae_mod_params* mp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop, float* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    ModParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_waves = (long long)n_streams * ch;
    p.delay = mp->delay;
    p.depth = mp->depth;
    p.g = mp->feedback;
    p.wet = mp->wet;
    p.dry = mp->dry;
    p.inv = 1.0 / (double)mp->n_voices;
    p.rate_inc = mp->rate_inc;
    p.phase0 = mp->phase0;
    p.phase_ch = mp->phase_ch;
    for (int v = 0; v < NAE_MOD_MAX_VOICES; v++) p.voice_phase[v] = mp->voice_phase[v];
    p.ch = ch;
    p.n_voices = mp->n_voices;
    p.shape = mp->shape;
    // the sub-block rule: 64 without feedback, else min(64, kmin - 1) with kmin = floor(delay - depth) >= 2; mod_sub caps it
    const long long kmin = (long long)floor(mp->delay - mp->depth);
    int sub = mp->feedback == 0.0 ? 64 : (int)(kmin - 1 < 64 ? kmin - 1 : 64);
    if (ctx->mod_sub > 0 && ctx->mod_sub < sub) sub = ctx->mod_sub;
    p.sub = sub < 1 ? 1 : sub;
    // one workgroup of one wave per stream-channel
    return nae_launch_tiles(ctx, "mod_kernel", "mod_kernel: grid too large", mod_kernel, p.n_waves, 1, 64, 0, to_view(src), to_out(dst), p,
                            d_state);
}

extern "C" {

int nae_mod_block_f32(nae_ctx* ctx, const nae_mod_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "mod: null pointer");
    const int rc = nae_mod_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "mod: null pointer");
    return nae_launch_mod(ctx, params, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr);
}

// DESIGN.md §3, "K17 modulated delay", "Design"
int nae_mod_design(int sample_rate, double rate_hz, double delay_ms, double depth_ms, double feedback, int voices, double spread, int shape,
                   double wet, double dry, nae_mod_params* out)
{
    if (!out || sample_rate <= 0) return NAE_ERR_INVALID;
    if (!isfinite(rate_hz) || !isfinite(delay_ms) || !isfinite(depth_ms) || !isfinite(feedback) || !isfinite(spread) || !isfinite(wet) || !isfinite(dry))
        return NAE_ERR_INVALID;
    if (rate_hz < 0.0 || rate_hz > 20.0 || depth_ms < 0.0 || !(fabs(feedback) <= NAE_MOD_MAX_FEEDBACK) || spread < 0.0 || spread > 1.0) return NAE_ERR_INVALID;
    if (voices < 1 || voices > NAE_MOD_MAX_VOICES || (shape != NAE_MOD_SINE && shape != NAE_MOD_TRIANGLE)) return NAE_ERR_INVALID;
    nae_mod_params p;
    memset(&p, 0, sizeof(p));
    p.delay = (delay_ms * 1e-3) * (double)sample_rate;
    p.depth = (depth_ms * 1e-3) * (double)sample_rate;
    if (!(p.delay - p.depth >= NAE_MOD_MIN_DELAY) || !(p.delay + p.depth <= NAE_MOD_MAX_DELAY)) return NAE_ERR_INVALID;
    p.feedback = feedback;
    p.wet = wet;
    p.dry = dry;
    p.rate_inc = (uint32_t)(uint64_t)llround((rate_hz / (double)sample_rate) * 4294967296.0);
    p.phase0 = 0;
    p.phase_ch = (uint32_t)llround(spread * 2147483648.0);
    p.n_voices = voices;
    for (int v = 0; v < voices; v++) p.voice_phase[v] = (uint32_t)(((uint64_t)v << 32) / (uint64_t)voices);
    p.shape = shape;
    *out = p;
    return NAE_OK;
}

} // extern "C"
