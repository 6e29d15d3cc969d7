// kernels_mb.hip — K20, the multiband compressor ("K20 multiband") for gfx950: a Linkwitz-Riley crossover tree of K11 sections, K12
// on every band, and the bands' sum.  Three kernels per slab of chunks, with the band signals in planes of a device workspace between them:
//
//   mb_split_kernel<B>   one wave per stream-channel walks its chunks as eq_cascade_kernel does.  A chunk is loaded once; the tree's 4, 9 or 14
//                        sections run on it with eq_section (eq_cascade.h), lane s keeping slot s's carry, the signal double from section to
//                        section of a path; every band is rounded once and stored coalesced into its plane.  Beside the working array the
//                        input and one branch point (l, then h) are live: three arrays of 16 doubles.
//   mb_band_kernel<DC>   one wave per (detector, band that is not bypassed) runs dyn_walk (dyn_steps.h) with the band's own record on the band's
//                        plane, in place.  The walk levels one chunk ahead, so a slab's planes hold chunks [c0, c1] while it runs [c0, c1).
//   mb_sum_kernel        the unmuted planes, added in double in band order and rounded once, into the caller's view.
//
// The planes stay inside NAE_CONV_WS_BYTES: a batch runs in groups of streams and slabs of chunks (debug keys mb_group, mb_slab), the carries of
// the sections and of the detectors on the device between slabs exactly as a handle keeps them between puts: one slab routine (nae_mb_run)
// serves the block call and the handle.  The split stores its carries in front of chunk c1 and the next slab computes that chunk again.
// Built with -ffp-contract=off: every step is one IEEE operation in the order of the CPU statement (tests/mb_ref/ref_mb.c), which is the
// composition of tests/eq_ref/ref_eq.c and tests/dyn_ref/ref_dyn.c.
#include "eq_cascade.h"
#include "dyn_steps.h"
#include <math.h>
#include <string.h>

namespace nae {

static_assert(NAE_MB_MAX_SECTIONS <= NAE_EQ_MAX_SECTIONS, "DESIGN.md §3, K20: the tree fits K11's constant block, lane s keeps slot s");

struct MbSplitParams {
    long long in_len;      // samples of a stream-channel: reads at or past in_len give zero, samples there are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed: the planes' first chunk is c_origin
    long long c_stop;
    long long c_keep;      // the carries in front of this chunk are the ones kept (c_origin <= c_keep <= c_stop)
    long long n_sc;        // stream-channels: one wave each
    long long plane_len;   // samples of a stream-channel's plane
    long long band_stride; // floats from a band's planes to the next band's
    int ch;
};

// state: [n_sc][NAE_EQ_MAX_SECTIONS][2] doubles, the carry (z1, z2) of every slot in front of chunk c_origin, replaced by the one in front of chunk
// c_keep
template <int B>
__global__ __launch_bounds__(64) void mb_split_kernel(SigViewD src, float* planes, MbSplitParams p, const double* __restrict__ tab, double* state)
{
    constexpr int S = B == 2 ? 4 : B == 3 ? 9 : 14;
    __shared__ float stage[kChunkStage];
    __shared__ double pq[NAE_EQ_MAX_SECTIONS * 2 * kChunkT];
    const int lane = threadIdx.x;
    const long long sc = blockIdx.x;
    if (sc >= p.n_sc) return;
    eq_stage_pq(pq, tab, S, lane, 64);
    chunk_lds_sync();
    const float* ip = src.base + (sc / p.ch) * src.ss + (sc % p.ch) * src.cs;
    float* pp = planes + sc * p.plane_len - p.c_origin * kChunkC;   // sample n of band b at pp[b * band_stride + n]

    double st1, st2;                                       // lane s: the carry of slot s
    eq_carry_load(state, sc, NAE_EQ_MAX_SECTIONS, lane, S, st1, st2);
    double k1 = st1, k2 = st2;
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        if (ck == p.c_keep) {
            k1 = st1;
            k2 = st2;
        }
        const long long n0 = ck * kChunkC;
        chunk_load<false, kChunkT>(stage, ip, src.fs, n0, p.in_len, lane);
        chunk_lds_sync();
        double x[kChunkT], w[kChunkT];
        chunk_lane_read(stage, lane, x);
        // slots [a, e) on w, in slot order
        const auto run = [&](int a, int e) {
#pragma unroll 1
            for (int s = a; s < e; s++) eq_section(w, s, lane, tab, pq, st1, st2);
        };
        // w, rounded once, is band b: the lanes write their own words, which nothing reads until the fence; the coalesced store reads the others'
        const auto emit = [&](int b) {
            chunk_lane_write(stage, lane, w);
            chunk_lds_sync();
            chunk_store<kChunkT>(stage, pp + b * p.band_stride, 1, n0, p.in_len, lane);
            chunk_lds_sync();
        };
        const auto copy = [&](double (&d)[kChunkT], const double (&s)[kChunkT]) {
#pragma unroll
            for (int k = 0; k < kChunkT; k++) d[k] = s[k];
        };
        copy(w, x);
        if constexpr (B == 2) {
            run(0, 2); emit(0);
            copy(w, x); run(2, 4); emit(1);
        } else if constexpr (B == 3) {
            run(0, 3); emit(0);
            copy(w, x); run(3, 5);
            copy(x, w);                                    // h
            run(5, 7); emit(1);
            copy(w, x); run(7, 9); emit(2);
        } else {
            double t[kChunkT];
            run(0, 3);
            copy(t, w);                                    // l
            run(3, 5); emit(0);
            copy(w, t); run(5, 7); emit(1);
            copy(w, x); run(7, 10);
            copy(t, w);                                    // h
            run(10, 12); emit(2);
            copy(w, t); run(12, 14); emit(3);
        }
    }
    if (p.c_keep >= p.c_stop) {
        k1 = st1;
        k2 = st2;
    }
    eq_carry_store(state, sc, NAE_EQ_MAX_SECTIONS, lane, S, k1, k2);
}

struct MbBandRec {
    DynParams p[NAE_MB_MAX_BANDS];   // the bands' launch records: in_len, chunks, detectors and look-ahead are the same in all
    int band_of[NAE_MB_MAX_BANDS];   // the bands that run, in band order
    long long plane_len, band_stride, c_origin;   // as MbSplitParams'
};

// state: [band][n_det][2] doubles, K12's carries (y1, yl) of every band's detectors
template <int DC>
__global__ __launch_bounds__(64) void mb_band_kernel(float* planes, MbBandRec r, double* state)
{
    const int lane = threadIdx.x;
    const long long n_det = r.p[0].n_det;
    const long long det = blockIdx.x % n_det;
    const int band = r.band_of[blockIdx.x / n_det];
    const DynParams& p = r.p[band];
    // the band's planes as an absolutely indexed planar view: DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`
    const long long sc0 = DC == 2 ? det * 2 : det;
    float* bp = planes + band * r.band_stride + sc0 * r.plane_len - r.c_origin * kChunkC;
    const SigViewD src{bp, 0, r.plane_len, 1};
    const OutViewD out{bp, 0, r.plane_len, 1};
    DynPlainKey<DC> mag{bp, src, p, lane};
    dyn_walk<DC>(bp, bp, src, out, p, state + band * n_det * 2, det, lane, mag);
}

struct MbSumParams {
    long long n0, n1;                  // samples [n0, n1) of every stream-channel, n1 at most the signal's length
    long long n_sc, plane_len, band_stride, plane_origin;
    int ch, n_sum;
    int band_of[NAE_MB_MAX_BANDS];     // the unmuted bands, in band order
};

constexpr int kMbSumThreads = 256;

// memory-bound: one workgroup per (stream-channel, chunk), four samples a thread, each read and each write of a wave 64 consecutive samples
__global__ __launch_bounds__(kMbSumThreads) void mb_sum_kernel(const float* __restrict__ planes, OutViewD out, MbSumParams p)
{
    const long long tiles = (p.n1 - p.n0 + kChunkC - 1) / kChunkC;
    const long long sc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    if (sc >= p.n_sc) return;
    const float* pp = planes + sc * p.plane_len - p.plane_origin;
    float* op = out.base + (sc / p.ch) * out.ss + (sc % p.ch) * out.cs;
#pragma unroll
    for (int j = 0; j < kChunkC / kMbSumThreads; j++) {
        const long long n = p.n0 + tile * kChunkC + j * kMbSumThreads + threadIdx.x;
        if (n >= p.n1) continue;
        float y = 0.0f;
        if (p.n_sum > 0) {
            double acc = (double)pp[p.band_of[0] * p.band_stride + n];
            for (int i = 1; i < p.n_sum; i++) acc = acc + (double)pp[p.band_of[i] * p.band_stride + n];
            y = (float)acc;
        }
        op[n * out.fs] = y;
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the tree's sections for B bands, 0 where there is no tree
static int nae_mb_sections(int n_bands) { return n_bands == 2 ? 4 : n_bands == 3 ? 9 : n_bands == 4 ? 14 : 0; }

// the one statement of the parameter rules of nae_mb_block_f32 and nae_mb_create (ctx may be null: no message then)
int nae_mb_check(nae_ctx* ctx, const nae_mb_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mb: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (p->n_bands < 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mb: n_bands must be at least 2");
    if (p->n_bands > NAE_MB_MAX_BANDS) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "mb: at most 4 bands");
    if (p->n_sections != nae_mb_sections(p->n_bands)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mb: n_sections must be 4, 9 or 14 for 2, 3 or 4 bands");
    int rc = nae_eq_check(ctx, &p->coef[0][0], p->n_sections, ch);
    if (rc) return rc;
    for (int b = 0; b < p->n_bands; b++) {
        if ((rc = nae_dyn_check(ctx, &p->band[b], ch))) return rc;
        if (p->band[b].lookahead != p->band[0].lookahead || p->band[b].link != p->band[0].link)
            return nae_fail_opt(ctx, NAE_ERR_INVALID, "mb: lookahead and link must be equal in all bands");
    }
    if ((p->mute_mask | p->bypass_mask) >> p->n_bands) return nae_fail_opt(ctx, NAE_ERR_INVALID, "mb: mask bit at or above n_bands");
    return NAE_OK;
}

// floats of the planes of n_streams x ch signals that hold `slab` chunks and the one the walk levels ahead; doubles of the two carries
size_t nae_mb_plane_floats(const nae_mb_params* p, int ch, size_t n_streams, size_t slab)
{
    return (size_t)p->n_bands * n_streams * (size_t)ch * (slab + 1) * kChunkC;
}
size_t nae_mb_state_doubles(const nae_mb_params* p, int ch, size_t n_streams)
{
    return n_streams * (size_t)ch * NAE_EQ_MAX_SECTIONS * 2 + (size_t)NAE_MB_MAX_BANDS * nae_dyn_detectors(&p->band[0], ch, n_streams) * 2;
}

// Chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing) in slabs of at most `slab` chunks through d_planes
// (nae_mb_plane_floats).  d_state (nae_mb_state_doubles): the sections' carries [stream-channel][16][2], then the detectors' [band][detector][2],
// in front of chunk c_origin; they are replaced by the ones in front of chunk c_stop.
int nae_mb_run(nae_ctx* ctx, const nae_mb_params* mp, const double* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
               const nae_sig* dst, size_t c_origin, size_t c_stop, float* d_planes, size_t slab, double* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    const size_t n_sc = n_streams * (size_t)ch;
    const size_t n_det = nae_dyn_detectors(&mp->band[0], ch, n_streams);
    double* d_dyn_state = d_state + n_sc * NAE_EQ_MAX_SECTIONS * 2;
    const long long plane_len = (long long)(slab + 1) * kChunkC, band_stride = (long long)n_sc * plane_len;
    const bool linked = mp->band[0].link && ch == 2;
    for (size_t c0 = c_origin; c0 < c_stop; c0 += slab) {
        const size_t c1 = c0 + slab < c_stop ? c0 + slab : c_stop;
        // the walk levels chunk c1 where something looks ahead and the signal reaches it: the split computes it, and keeps the carries in front of it
        const bool ahead = mp->band[0].lookahead > 0 && c1 * kChunkC < in_len;
        MbSplitParams sp;
        sp.in_len = (long long)in_len;
        sp.c_origin = (long long)c0;
        sp.c_stop = (long long)(c1 + (ahead ? 1 : 0));
        sp.c_keep = (long long)c1;
        sp.n_sc = (long long)n_sc;
        sp.plane_len = plane_len;
        sp.band_stride = band_stride;
        sp.ch = ch;
        int rc = pick_value<2, 3, 4>(ctx, mp->n_bands, "mb: n_bands must be 2, 3 or 4", [&](auto nb) {
            return nae_launch_tiles(ctx, "mb_split_kernel", "mb_split_kernel: grid too large", mb_split_kernel<nb.value>, sp.n_sc, 1, 64, 0, to_view(src),
                                    d_planes, sp, d_block, d_state);
        });
        if (rc) return rc;
        MbBandRec br;
        int n_run = 0;
        for (int b = 0; b < NAE_MB_MAX_BANDS; b++) {
            br.p[b] = nae_dyn_launch_params(&mp->band[b < mp->n_bands ? b : 0], in_len, ch, n_streams, c0, c1);
            br.band_of[b] = 0;
        }
        for (int b = 0; b < mp->n_bands; b++)
            if (!(mp->bypass_mask >> b & 1u)) br.band_of[n_run++] = b;
        br.plane_len = plane_len;
        br.band_stride = band_stride;
        br.c_origin = (long long)c0;
        if (n_run) {
            rc = with_flags(linked, [&](auto lk) {
                return nae_launch_tiles(ctx, "mb_band_kernel", "mb_band_kernel: grid too large", mb_band_kernel<lk.value ? 2 : 1>,
                                        (long long)n_det * n_run, 1, 64, 0, d_planes, br, d_dyn_state);
            });
            if (rc) return rc;
        }
        MbSumParams up;
        up.n0 = (long long)(c0 * kChunkC);
        up.n1 = (long long)(c1 * kChunkC < in_len ? c1 * kChunkC : in_len);
        up.n_sc = (long long)n_sc;
        up.plane_len = plane_len;
        up.band_stride = band_stride;
        up.plane_origin = (long long)(c0 * kChunkC);
        up.ch = ch;
        up.n_sum = 0;
        for (int b = 0; b < NAE_MB_MAX_BANDS; b++) up.band_of[b] = 0;
        for (int b = 0; b < mp->n_bands; b++)
            if (!(mp->mute_mask >> b & 1u)) up.band_of[up.n_sum++] = b;
        if (up.n1 > up.n0) {
            rc = nae_launch_tiles(ctx, "mb_sum_kernel", "mb_sum_kernel: grid too large", mb_sum_kernel, up.n_sc * (long long)(c1 - c0), 1, kMbSumThreads, 0,
                                  static_cast<const float*>(d_planes), to_out(dst), up);
            if (rc) return rc;
        }
    }
    return NAE_OK;
}

// the slab of a handle, which holds one stream: mb_slab, else 64 chunks
size_t nae_mb_handle_slab(const nae_ctx* ctx) { return ctx->mb_slab > 0 ? (size_t)ctx->mb_slab : 64; }

extern "C" {

int nae_mb_block_f32(nae_ctx* ctx, const nae_mb_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "mb: null pointer");
    int rc = nae_mb_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "mb: null pointer");
    // the sections' tables are the context's, with nae_eq_block_f32's: a call with the coefficients of the last one uploads nothing
    double* d_block = nullptr;
    if ((rc = nae_eq_cached_block(ctx, &params->coef[0][0], params->n_sections, &d_block))) return rc;
    // streams per group: as many as leave the planes room for a chunk and the one ahead of it inside the cap, or mb_group; chunks per slab: as
    // many as the cap then holds, or mb_slab
    const size_t chunks = nae_chunks(in_len);
    const size_t chunk_bytes = (size_t)params->n_bands * (size_t)ch * kChunkC * sizeof(float);   // of one stream
    size_t group = ctx->mb_group > 0 ? (size_t)ctx->mb_group : NAE_CONV_WS_BYTES / (2 * chunk_bytes);
    group = group < 1 ? 1 : group < n_streams ? group : n_streams;
    size_t slab = ctx->mb_slab > 0 ? (size_t)ctx->mb_slab : NAE_CONV_WS_BYTES / (group * chunk_bytes) - 1;
    slab = slab < 1 ? 1 : slab < chunks ? slab : chunks;
    // the carries stand in front of the planes, on a 256-byte boundary
    const size_t state_bytes = (nae_mb_state_doubles(params, ch, group) * sizeof(double) + 255) / 256 * 256;
    rc = ctx->ws_mb.reserve(ctx, state_bytes + nae_mb_plane_floats(params, ch, group, slab) * sizeof(float), "workspace");
    if (rc) return rc;
    double* d_state = ctx->ws_mb.as<double>();
    float* d_planes = reinterpret_cast<float*>(ctx->ws_mb.as<char>() + state_bytes);
    return nae_for_stream_groups(src, dst, n_streams, group, [&](const nae_sig& gs, const nae_sig& gd, size_t n) {
        (void)nae_use_device(ctx);
        const hipError_t e = hipMemsetAsync(d_state, 0, nae_mb_state_doubles(params, ch, n) * sizeof(double), ctx->stream);
        if (e != hipSuccess) return nae_check(ctx, e, "hipMemsetAsync(mb state)");
        return nae_mb_run(ctx, params, d_block, &gs, in_len, ch, n, &gd, 0, chunks, d_planes, slab, d_state);
    });
}

// DESIGN.md §3, "K20 multiband", "Design": the tree's slots from the crossovers, LR4 halves by nae_eq_design at q = 1 / sqrt 2 and the cookbook's
// all-pass of the same w0, alpha and q
int nae_mb_design(int sample_rate, int n_bands, const double* crossover_hz, const nae_dyn_params* bands, unsigned mute_mask, unsigned bypass_mask,
                  nae_mb_params* out)
{
    if (!out || !crossover_hz || !bands || sample_rate <= 0 || n_bands < 2 || n_bands > NAE_MB_MAX_BANDS) return NAE_ERR_INVALID;
    if ((mute_mask | bypass_mask) >> n_bands) return NAE_ERR_INVALID;
    const double q = 0.7071067811865476;
    double lp[NAE_MB_MAX_BANDS - 1][5], hp[NAE_MB_MAX_BANDS - 1][5], ap[NAE_MB_MAX_BANDS - 1][5];
    for (int i = 0; i < n_bands - 1; i++) {
        const double f = crossover_hz[i];
        if (!isfinite(f) || (i && !(f > crossover_hz[i - 1]))) return NAE_ERR_INVALID;
        if (nae_eq_design(NAE_EQ_LOWPASS, sample_rate, f, 0.0, q, lp[i]) != NAE_OK || nae_eq_design(NAE_EQ_HIGHPASS, sample_rate, f, 0.0, q, hp[i]) != NAE_OK)
            return NAE_ERR_INVALID;
        const double pi = 3.14159265358979323846;
        const double w0 = 2.0 * pi * f / (double)sample_rate;
        const double cs = cos(w0), alpha = sin(w0) / (2.0 * q);
        const double a0 = 1.0 + alpha;
        ap[i][0] = (1.0 - alpha) / a0;
        ap[i][1] = (-2.0 * cs) / a0;
        ap[i][2] = (1.0 + alpha) / a0;
        ap[i][3] = (-2.0 * cs) / a0;
        ap[i][4] = (1.0 - alpha) / a0;
    }
    nae_mb_params p;
    memset(&p, 0, sizeof(p));
    p.n_bands = n_bands;
    p.n_sections = nae_mb_sections(n_bands);
    // the slots of DESIGN.md's table: (kind, crossover) per slot; kind 0 LP, 1 HP, 2 AP
    static const signed char tree[3][NAE_MB_MAX_SECTIONS][2] = {
        {{0, 0}, {0, 0}, {1, 0}, {1, 0}},
        {{0, 0}, {0, 0}, {2, 1}, {1, 0}, {1, 0}, {0, 1}, {0, 1}, {1, 1}, {1, 1}},
        {{0, 1}, {0, 1}, {2, 2}, {0, 0}, {0, 0}, {1, 0}, {1, 0}, {1, 1}, {1, 1}, {2, 0}, {0, 2}, {0, 2}, {1, 2}, {1, 2}}};
    for (int s = 0; s < p.n_sections; s++) {
        const int kind = tree[n_bands - 2][s][0], x = tree[n_bands - 2][s][1];
        memcpy(p.coef[s], kind == 0 ? lp[x] : kind == 1 ? hp[x] : ap[x], 5 * sizeof(double));
    }
    for (int b = 0; b < n_bands; b++) p.band[b] = bands[b];
    p.mute_mask = mute_mask;
    p.bypass_mask = bypass_mask;
    if (nae_mb_check(nullptr, &p, 1) != NAE_OK) return NAE_ERR_INVALID;
    *out = p;
    return NAE_OK;
}

} // extern "C"
