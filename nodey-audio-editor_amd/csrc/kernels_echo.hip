// kernels_echo.hip — K16, the echo ("K16 echo") for gfx950: a feedback delay whose loop runs K11's cascade as its damping filter.
//
// The delay is at least one K11 chunk (NAE_ECHO_MIN_DELAY = NAE_EQ_CHUNK), so when a chunk starts, all of its delayed input has been written:
// a chunk of the loop is one K11 cascade over known samples, and the recurrence over the delay needs no scan.  One workgroup per stream, one
// wave per channel; every wave walks the chunks in order.  Per chunk a wave loads its 1024 input samples and the 1024 delayed samples of the
// line it listens to (its own, or with `cross` the other channel's) coalesced into two LDS stages in K11's lane order (chunk_stage.h), runs
// eq_section per section on the delayed samples, forms the line's new samples w and the output y in registers, and stores both coalesced
// through the same stages.  The line is a ring of R samples per stream-channel in device memory, R the smallest multiple of the chunk with
// R >= max(D_0, D_1) + 1024, addressed by the absolute sample index mod R: a chunk's store never wraps (its load may, at any sample), and the
// samples it overwrites, [n0 - R, n0 - R + 1024), lie in front of everything either channel of the stream reads in this chunk or later
// (reads reach back to n0 - max D >= n0 - R + 1024).  At D = 1024 a chunk reads exactly what the previous iteration stored — with `cross`
// what the OTHER wave stored — so one __syncthreads() stands between a chunk's line stores and the next chunk's line loads, behind
// every wave's own wait for its stores (s_waitcnt vmcnt(0): the barrier itself waits for no counter): a workgroup-scope release / acquire.
// Both waves sit on one CU and share its vector L1, which is why both channels of a stream stay in one workgroup.  The same barrier keeps a
// wave from overwriting, one chunk ahead, samples its sibling still has to read.  The line is never read for n < D, so no workspace needs
// clearing.
// The translation unit is built with -ffp-contract=off: every step is one IEEE operation, in the order of tests/echo_ref/ref_echo.c.
#include "eq_cascade.h"
#include <math.h>
#include <string.h>

namespace nae {

struct EchoParams {
    long long in_len;      // samples of a stream-channel: reads at or past in_len give zero, samples there are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_streams;   // one workgroup each
    long long ring;        // R: samples of a stream-channel's line
    double g, wet, dry;
    int ch, n_sections, cross;
    int delay[2];
};

// line: [n_streams][ch][R] floats; state: [n_streams][ch][NAE_ECHO_MAX_SECTIONS][2] doubles, the carry (z1, z2) of every section in front of
// chunk c_origin, replaced by the one behind chunk c_stop - 1; null: zero in, nothing out (the block call)
__global__ __launch_bounds__(128) void echo_kernel(SigViewD src, OutViewD out, EchoParams p, const double* __restrict__ tab, float* line, double* state)
{
    __shared__ float stage[2][2][kChunkStage];                   // [wave][x / y | v / w]
    __shared__ double pq[NAE_ECHO_MAX_SECTIONS * 2 * kChunkT];   // p and q of every section: read at wave-uniform addresses (a broadcast)
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    const long long s_idx = blockIdx.x;
    if (s_idx >= p.n_streams) return;                            // the whole workgroup: no wave is left alone at a barrier
    eq_stage_pq(pq, tab, p.n_sections, threadIdx.x, blockDim.x);
    __syncthreads();
    float* sx = stage[c][0];
    float* sv = stage[c][1];
    const float* ip = src.base + s_idx * src.ss + c * src.cs;
    float* op = out.base + s_idx * out.ss + c * out.cs;
    const int S = p.n_sections;
    const long long R = p.ring, D = p.delay[c];
    const long long sc = s_idx * p.ch + c;
    const float* rline = line + (s_idx * p.ch + (p.cross && p.ch == 2 ? 1 - c : c)) * R;   // the line this channel's loop listens to
    float* wline = line + sc * R;
    const double g = p.g, wet = p.wet, dry = p.dry;

    double st1, st2;                                             // lane s: the carry of section s
    eq_carry_load(state, sc, NAE_ECHO_MAX_SECTIONS, lane, S, st1, st2);
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        // sample n0 - D of the listened line stands at rpos (n0 - D may be negative: such samples are not read)
        long long rpos = (n0 - D) % R;
        if (rpos < 0) rpos += R;
        const long long wpos = n0 % R;                           // R is a multiple of the chunk: [wpos, wpos + 1024) does not wrap
#pragma unroll
        for (int j = 0; j < kChunkT; j++) {
            const int n = j * 64 + lane;
            const long long gi = n0 + n;
            long long r = rpos + n;
            if (r >= R) r -= R;
            // both loads are issued whatever the sample's place, from an address inside the signal and inside the ring, and what does not count
            // is dropped behind them: 32 loads in flight, not 32 branches that each wait for their own
            const bool in = gi < p.in_len;
            const float xv = ip[(in ? gi : p.in_len - 1) * src.fs], lv = rline[r];
            sx[chunk_word(n)] = in ? xv : 0.0f;
            sv[chunk_word(n)] = in && gi >= D ? lv : 0.0f;
        }
        chunk_lds_sync();
        float xs[kChunkT];
        double f[kChunkT];
        // the two stages word by word, not one chunk_lane_read after the other: that order measured 5 ... 10 % slower at 8 streams
        // (profiles/r24_chunk_stage.md)
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            xs[k] = sx[lane * kChunkStride + k];
            f[k] = (double)sv[lane * kChunkStride + k];
        }
#pragma unroll 1
        for (int s = 0; s < S; s++) {
            eq_section(f, s, lane, tab, pq, st1, st2);
        }
        // the lanes read their own words above and write only them here; the coalesced reads below need the other lanes' words
        double y[kChunkT];
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const double xd = (double)xs[k];
            y[k] = (dry * xd) + (wet * f[k]);
            f[k] = xd + (g * f[k]);                              // w, the line's new sample
        }
        chunk_lane_write(sv, lane, f);
        chunk_lane_write(sx, lane, y);
        chunk_lds_sync();
#pragma unroll
        for (int j = 0; j < kChunkT; j++) {
            const int n = j * 64 + lane;
            const long long gi = n0 + n;
            if (gi < p.in_len) {
                op[gi * out.fs] = sx[chunk_word(n)];
                wline[wpos + n] = sv[chunk_word(n)];
            }
        }
        // this chunk's line stores, of both waves, before the next chunk's line loads (and the stages' reads before they are rewritten).
        // s_barrier waits for no counter, and the workgroup-scope release of __syncthreads() compiles to no wait for vector stores on this
        // target (a CU's L1 takes its waves' accesses in issue order), so every storing wave drains its own stores in front of the barrier:
        // the hand-off then holds whatever the order in which the L1 takes them
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    eq_carry_store(state, sc, NAE_ECHO_MAX_SECTIONS, lane, S, st1, st2);
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_echo_block_f32 and nae_echo_create (ctx may be null: no message then)
int nae_echo_check(nae_ctx* ctx, const nae_echo_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "echo: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->feedback) || !isfinite(p->wet) || !isfinite(p->dry)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "echo: non-finite parameter");
    if (!(fabs(p->feedback) <= NAE_ECHO_MAX_FEEDBACK)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "echo: |feedback| above 0.99");
    if (p->cross != 0 && p->cross != 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "echo: cross must be 0 or 1");
    if (p->n_sections < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "echo: negative n_sections");
    if (p->n_sections > NAE_ECHO_MAX_SECTIONS) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "echo: at most 4 sections");
    for (int c = 0; c < ch; c++)
        if (p->delay[c] < NAE_ECHO_MIN_DELAY || p->delay[c] > NAE_ECHO_MAX_DELAY)
            return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "echo: the delay must be 1024 ... 1048576 samples");
    return p->n_sections ? nae_eq_check(ctx, &p->coef[0][0], p->n_sections, ch) : NAE_OK;
}

// R: samples of a stream-channel's line, the smallest multiple of the chunk that holds the longest delay of the call's channels and one chunk
size_t nae_echo_ring(const nae_echo_params* p, int ch)
{
    const size_t d = (size_t)(ch == 2 && p->delay[1] > p->delay[0] ? p->delay[1] : p->delay[0]);
    return nae_chunks(d + kChunkC) * kChunkC;
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_block: the sections' K11 constant block, unused
// with no section; d_line: n_streams x ch rings of nae_echo_ring() floats; d_state as the kernel's
int nae_launch_echo(nae_ctx* ctx, const nae_echo_params* ep, const double* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                    const nae_sig* dst, size_t c_origin, size_t c_stop, float* d_line, double* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    EchoParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_streams = (long long)n_streams;
    p.ring = (long long)nae_echo_ring(ep, ch);
    p.g = ep->feedback;
    p.wet = ep->wet;
    p.dry = ep->dry;
    p.ch = ch;
    p.n_sections = ep->n_sections;
    p.cross = ep->cross;
    p.delay[0] = ep->delay[0];
    p.delay[1] = ch == 2 ? ep->delay[1] : ep->delay[0];
    // one workgroup per stream, one wave per channel
    return nae_launch_tiles(ctx, "echo_kernel", "echo_kernel: grid too large", echo_kernel, p.n_streams, 1, 64 * ch, 0, to_view(src), to_out(dst), p,
                            d_block, d_line, d_state);
}

extern "C" {

int nae_echo_block_f32(nae_ctx* ctx, const nae_echo_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "echo: null pointer");
    int rc = nae_echo_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "echo: null pointer");
    // the sections' tables are the context's, with nae_eq_block_f32's: a call with the coefficients of the last one uploads nothing
    double* d_block = nullptr;
    if (params->n_sections && (rc = nae_eq_cached_block(ctx, &params->coef[0][0], params->n_sections, &d_block))) return rc;
    // streams per launch: as many as keep the lines inside the workspace cap, or echo_group
    const size_t line_bytes = nae_echo_ring(params, ch) * (size_t)ch * sizeof(float);
    size_t group = ctx->echo_group > 0 ? (size_t)ctx->echo_group : NAE_CONV_WS_BYTES / line_bytes;
    group = group < 1 ? 1 : group < n_streams ? group : n_streams;
    rc = ctx->ws_echo.reserve(ctx, group * line_bytes, "workspace");
    if (rc) return rc;
    const size_t chunks = nae_chunks(in_len);
    return nae_for_stream_groups(src, dst, n_streams, group, [&](const nae_sig& gs, const nae_sig& gd, size_t n) {
        return nae_launch_echo(ctx, params, d_block, &gs, in_len, ch, n, &gd, 0, chunks, ctx->ws_echo.as<float>(), nullptr);
    });
}

// DESIGN.md §3, "K16 echo", "Design": the delays to the nearest sample, the loop's low-pass and high-pass by nae_eq_design at q = 1 / sqrt 2
int nae_echo_design(int sample_rate, double delay_s_left, double delay_s_right, double feedback, double damp_hz, double lowcut_hz, double wet,
                    double dry, int cross, nae_echo_params* out)
{
    if (!out || sample_rate <= 0 || (cross != 0 && cross != 1)) return NAE_ERR_INVALID;
    if (!isfinite(delay_s_left) || !isfinite(delay_s_right) || !isfinite(feedback) || !isfinite(damp_hz) || !isfinite(lowcut_hz) || !isfinite(wet) ||
        !isfinite(dry))
        return NAE_ERR_INVALID;
    if (!(fabs(feedback) <= NAE_ECHO_MAX_FEEDBACK) || damp_hz < 0.0 || lowcut_hz < 0.0) return NAE_ERR_INVALID;
    nae_echo_params p;
    memset(&p, 0, sizeof(p));
    const double d[2] = {delay_s_left * (double)sample_rate, delay_s_right * (double)sample_rate};
    for (int c = 0; c < 2; c++) {
        if (!(d[c] >= (double)NAE_ECHO_MIN_DELAY - 0.5 && d[c] <= (double)NAE_ECHO_MAX_DELAY + 0.5)) return NAE_ERR_INVALID;
        const long r = lround(d[c]);
        if (r < NAE_ECHO_MIN_DELAY || r > NAE_ECHO_MAX_DELAY) return NAE_ERR_INVALID;
        p.delay[c] = (int)r;
    }
    p.feedback = feedback;
    p.cross = cross;
    p.wet = wet;
    p.dry = dry;
    const double q = sqrt(0.5);
    if (damp_hz > 0.0 && nae_eq_design(NAE_EQ_LOWPASS, sample_rate, damp_hz, 0.0, q, p.coef[p.n_sections++]) != NAE_OK) return NAE_ERR_INVALID;
    if (lowcut_hz > 0.0 && nae_eq_design(NAE_EQ_HIGHPASS, sample_rate, lowcut_hz, 0.0, q, p.coef[p.n_sections++]) != NAE_OK) return NAE_ERR_INVALID;
    *out = p;
    return NAE_OK;
}

} // extern "C"
