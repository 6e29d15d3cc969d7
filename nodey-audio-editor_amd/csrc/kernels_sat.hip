// kernels_sat.hip — K18, the saturation ("K18 saturation") for gfx950: a static waveshaper run oversampled.  Per sample n of a
// stream-channel: the input goes up by M through a polyphase FIR (u), through the curve (v = f(g u + b) - f(b)), down again through the same
// prototype (s), and is mixed with the input delayed by the latency D = 2 K = 32.  The kernel is feed-forward: y[n] reads x[n - 64 ... n] and
// nothing it wrote, so time tiles freely: one wave per (stream-channel, tile of chunks), and a lone stream fills the chip.
//
// A wave walks its tile in pieces of P = 2048 / M samples (1024, 512, 256 at M = 2, 4, 8: the oversampled stage is 2048 + 32 M samples, and
// with its padding and the x stage a wave has 13 ... 16 KiB: a CU holds ten to twelve waves).  Two stages in LDS: xs, the piece's input with the 64 samples in front of it (clamped loads, zero below sample 0 and from
// in_len on), and vs, the shaped oversampled signal of the piece and of the 32 base samples in front of it, one row per phase: vs[p][i] is
// v[M (n0 - 32 + i) + p].  A lane owns four consecutive base samples in both phases of a piece, and slot i of a stage stands at word
// i + i / 4: a lane's four words are consecutive and two lanes' are five apart, which is odd: the 32 lanes of a ds_read_b32 group fall on 32
// different banks (chunk_word's pattern at four samples per lane).  chunk_stage.h's chunk_load, chunk_store and chunk_word are not used: they
// move one whole chunk of 1024 samples at 16 samples a lane (stride 17), and here a stage is a piece of 256 ... 1024 samples with a halo of
// 64 in front of it, read at four samples a lane (stride 5) so that a lane's register window and the taps it meets stay small; the
// clamped-load and guarded-store forms and chunk_lds_sync are chunk_stage.h's.  Only the lanes' own reads and writes (five words apart) are
// free of bank conflicts: the coalesced fill and drain of xs touch words k + k / 4 for 64 consecutive k, 40 words a half wave, and meet a
// few two-way conflicts per instruction, as chunk_load's do at stride 17.
//   Phase A  the lane reads x[n - 32 ... n + 3], 36 words, into a register window and forms the M phases of its four samples, each one chain
//            of 32 or 33 FMAs over taps that are wave-uniform (scalar loads), shapes them and writes them to vs.
//   Phase B  the lane forms its four outputs: per block of 32 / M base samples back it reads 32 / M + 3 words of every phase, 32 + 3 M words for 128 FMAs,
//            each output's chain in the one order of the specification; then the mix with x[n - 32] out of xs, and y goes back into xs where
//            that x stood, which no other lane reads.
//   Store    the wave stores the piece out of xs, 64 consecutive samples a store.
// The v halo of a tile's first piece is computed (eight lanes, once per tile); between pieces the last 32 base samples of every phase row move
// to its front: 40 M words, against 12.5 % more of phase A at M = 8 for computing them again.
// M = 1 has no filter: a streaming map of its own (sat_map_kernel), 16 bytes per lane where both views are interleaved or mono and aligned.
// The translation unit is built with -ffp-contract=off: every step is one IEEE f32 operation, in the order of tests/sat_ref/ref_sat.c.
#include "chunk_stage.h"
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kSatK = NAE_SAT_HALF, kSatD = 2 * kSatK;
static_assert(kSatK == 16 && NAE_SAT_MAX_OS == 8, "the window sizes below are written for K = 16 and M up to 8");
constexpr int kSatTapRow = 264;                                  // floats of one tap row on the device (hd, then hu): 2 K M + 1 = 257 at most, 16-byte multiples
constexpr int kSatSlot = 2 * kSatTapRow;                         // floats of one oversampling factor's slot: [hd | hu]

struct SatParams {
    long long in_len;      // samples of a stream-channel: samples at or past in_len are not stored and read as zero
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_tiles;     // tiles of `tile` chunks per stream-channel: one wave each
    long long n_items;     // stream-channels x tiles
    int tile, ch;
    float g, b, wet, dry;
};

// the curve ("K18 saturation", step 2): compare-select, so a NaN stays a NaN
template <int CURVE>
__device__ __forceinline__ float sat_curve(float t)
{
    if constexpr (CURVE == NAE_SAT_SOFT) {
        const float c = t > 3.0f ? 3.0f : (t < -3.0f ? -3.0f : t);
        const float q = c * c;
        return (c * (27.0f + q)) / (27.0f + (9.0f * q));
    } else {
        return t > 1.0f ? 1.0f : (t < -1.0f ? -1.0f : t);
    }
}

// slot i of a stage (four samples per lane)
__device__ __forceinline__ int sat_word(int i) { return i + (i >> 2); }

template <int M>
struct Sat {
    static constexpr int P = 2048 / M;                    // base samples of a piece
    static constexpr int kPasses = P / 256;               // rounds of 64 lanes x 4 samples
    static constexpr int XS = P + 2 * kSatD;              // slots of xs: x[n0 - 64 ... n0 + P)
    static constexpr int XW = XS + XS / 4;
    static constexpr int VS = P + kSatD;                  // slots of a phase row: base samples [n0 - 32, n0 + P)
    static constexpr int VW = VS + VS / 4;
    static constexpr int kLds = XW + M * VW;              // words
    static constexpr int kBack = 32 / M;                  // base samples back a block of phase B reads: 32 taps in SGPRs, (kBack + 3) M words in VGPRs, 128 FMAs
    static_assert(kChunkC % P == 0 && P % 256 == 0, "pieces tile a chunk, lanes x 4 tile a piece");
};

// phase A for the four base samples of slot group q (v slots 4 q ... 4 q + 3, base samples n0 - 32 + 4 q + r): reads x slots 4 q ... 4 q + 35
template <int M, int CURVE>
__device__ __forceinline__ void sat_up(const float* xs, float* vs, const float* __restrict__ hu, int q, float g, float b, float fb)
{
    using S = Sat<M>;
    float w[36];
#pragma unroll
    for (int k = 0; k < 36; k++) w[k] = xs[5 * q + k + (k >> 2)];
    // one phase a trip: its 32 taps (33 in phase 0) are read where they are used, wave-uniform, and do not outlive the trip
#pragma unroll 1
    for (int p = 0; p < M; p++) {
        const float* __restrict__ hp = hu + p;
        float a[4];
#pragma unroll
        for (int r = 0; r < 4; r++) a[r] = hp[0] * w[32 + r];
#pragma unroll
        for (int i = 1; i < 2 * kSatK; i++) {
            const float h = hp[i * M];
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] = __builtin_fmaf(h, w[32 + r - i], a[r]);
        }
        if (p == 0) {
            const float h = hp[2 * kSatK * M];
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] = __builtin_fmaf(h, w[r], a[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float t = __builtin_fmaf(g, a[r], b);
            vs[p * S::VW + 5 * q + r] = sat_curve<CURVE>(t) - fb;
        }
    }
}

// taps: the slot of this M, [hd | hu] (wave-uniform reads)
template <int M, int CURVE>
__global__ __launch_bounds__(64) void sat_kernel(SigViewD src, OutViewD out, SatParams p, const float* __restrict__ taps)
{
    using S = Sat<M>;
    constexpr int TB = S::kBack;
    __shared__ float lds[S::kLds];
    float* xs = lds;
    float* vs = lds + S::XW;
    const int lane = threadIdx.x;
    const long long item = blockIdx.x;
    if (item >= p.n_items) return;
    const long long sc = item / p.n_tiles;
    const long long tl = item - sc * p.n_tiles;
    const long long s_idx = sc / p.ch;
    const int c = (int)(sc - s_idx * p.ch);
    const float* __restrict__ ip = src.base + s_idx * src.ss + c * src.cs;
    float* __restrict__ op = out.base + s_idx * out.ss + c * out.cs;
    const float* __restrict__ hd = taps;
    const float* __restrict__ hu = taps + kSatTapRow;
    const float g = p.g, b = p.b, wet = p.wet, dry = p.dry;
    const float fb = sat_curve<CURVE>(b);
    const long long in_len = p.in_len;

    const long long c_first = p.c_origin + tl * p.tile;
    long long c_last = c_first + p.tile;
    if (c_last > p.c_stop) c_last = p.c_stop;
    long long n_end = c_last * kChunkC;
    if (n_end > in_len) n_end = in_len;
    bool first = true;
#pragma unroll 1
    for (long long n0 = c_first * kChunkC; n0 < n_end; n0 += S::P) {
        // xs: x[n0 - 64 ... n0 + P): every load is issued, from an address inside the signal, and what lies outside it is dropped behind it
#pragma unroll
        for (int j = 0; j < S::XS / 64; j++) {
            const int k = j * 64 + lane;
            const long long gi = n0 - 2 * kSatD + k;
            const bool in = gi >= 0 && gi < in_len;
            const float xv = ip[(gi < 0 ? 0 : (gi < in_len ? gi : in_len - 1)) * src.fs];
            xs[sat_word(k)] = in ? xv : 0.0f;
        }
        chunk_lds_sync();
        // phase A: the v halo of the tile's first piece, then the piece
        if (first) {
            if (lane < kSatD / 4) sat_up<M, CURVE>(xs, vs, hu, lane, g, b, fb);
            first = false;
        }
#pragma unroll 1
        for (int ps = 0; ps < S::kPasses; ps++) sat_up<M, CURVE>(xs, vs, hu, kSatD / 4 + ps * 64 + lane, g, b, fb);
        chunk_lds_sync();
        // phase B: outputs o = 4 qo + r of the piece; the v slot of base sample n0 + o is o + 32.  s = hd[0] v[M n], then for t = 0 ... 31 the
        // M taps hd[t M + 1 ... t M + M] meet phases M - 1 ... 0 of base sample n - 1 - t, slot o + 31 - t
#pragma unroll 1
        for (int ps = 0; ps < S::kPasses; ps++) {
            const int qo = ps * 64 + lane;
            float s[4];
#pragma unroll
            for (int r = 0; r < 4; r++) s[r] = hd[0] * vs[5 * (qo + kSatD / 4) + r];
#pragma unroll 1
            for (int tb = 0; tb < 2 * kSatK / TB; tb++) {
                // t = TB tb + tt: slot o + 31 - t = 4 (qo - TB / 4 tb) + e, e = r + 31 - tt in [32 - TB, 34]
                const int at = 5 * (qo - TB / 4 * tb);
                const float* __restrict__ hb = hd + tb * TB * M;
                float win[M][TB + 3];
#pragma unroll
                for (int ph = 0; ph < M; ph++)
#pragma unroll
                    for (int e = 0; e < TB + 3; e++) win[ph][e] = vs[ph * S::VW + at + (e + 32 - TB) + ((e + 32 - TB) >> 2)];
#pragma unroll
                for (int tt = 0; tt < TB; tt++)
#pragma unroll
                    for (int q = 1; q <= M; q++) {
                        const float h = hb[tt * M + q];
#pragma unroll
                        for (int r = 0; r < 4; r++) s[r] = __builtin_fmaf(h, win[(M - q) % M][r + TB - 1 - tt], s[r]);
                    }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int wd = 5 * (qo + kSatD / 4) + r;       // x[n - 32]: x slot o + 32
                xs[wd] = (dry * xs[wd]) + (wet * s[r]);
            }
        }
        chunk_lds_sync();
#pragma unroll
        for (int j = 0; j < S::P / 64; j++) {
            const int o = j * 64 + lane;
            const long long gi = n0 + o;
            if (gi < n_end) op[gi * out.fs] = xs[sat_word(o + kSatD)];
        }
        // the last 32 base samples of every phase row become the next piece's halo
        float keep[(M * 40 + 63) / 64];
#pragma unroll
        for (int j = 0; j < (M * 40 + 63) / 64; j++) {
            const int k = j * 64 + lane;
            const int ph = k / 40, wd = k - ph * 40;
            keep[j] = k < M * 40 ? vs[ph * S::VW + 5 * (S::P / 4) + wd] : 0.0f;
        }
        chunk_lds_sync();
#pragma unroll
        for (int j = 0; j < (M * 40 + 63) / 64; j++) {
            const int k = j * 64 + lane;
            const int ph = k / 40, wd = k - ph * 40;
            if (k < M * 40) vs[ph * S::VW + wd] = keep[j];
        }
        chunk_lds_sync();
    }
}

constexpr int kSatMapBlock = 256, kSatMapPer = 4;          // threads of a workgroup of the M = 1 map, 16-byte pieces per thread

template <int CURVE>
__device__ __forceinline__ float sat_map(float x, float g, float b, float fb, float wet, float dry)
{
    return (dry * x) + (wet * (sat_curve<CURVE>(__builtin_fmaf(g, x, b)) - fb));
}

// M = 1, both views interleaved (or mono) and 16-byte aligned: elements [e0, e1) of every stream, e0 a multiple of 4; `per` workgroups a stream
template <int CURVE>
__global__ __launch_bounds__(kSatMapBlock) void sat_map_flat_kernel(SigViewD src, OutViewD out, long long e0, long long e1, long long per, float g,
                                                                    float b, float wet, float dry)
{
    const long long s = blockIdx.x / per, blk = blockIdx.x - s * per;
    const float* __restrict__ in = src.base + s * src.ss;
    float* __restrict__ o = out.base + s * out.ss;
    const float fb = sat_curve<CURVE>(b);
    const long long first = e0 + (blk * kSatMapBlock * kSatMapPer) * 4;
    float4 v[kSatMapPer];
#pragma unroll
    for (int j = 0; j < kSatMapPer; j++) {
        const long long e = first + ((long long)j * kSatMapBlock + threadIdx.x) * 4;
        if (e + 4 <= e1) v[j] = *reinterpret_cast<const float4*>(in + e);
    }
#pragma unroll
    for (int j = 0; j < kSatMapPer; j++) {
        const long long e = first + ((long long)j * kSatMapBlock + threadIdx.x) * 4;
        if (e + 4 <= e1) {
            float4 y;
            y.x = sat_map<CURVE>(v[j].x, g, b, fb, wet, dry);
            y.y = sat_map<CURVE>(v[j].y, g, b, fb, wet, dry);
            y.z = sat_map<CURVE>(v[j].z, g, b, fb, wet, dry);
            y.w = sat_map<CURVE>(v[j].w, g, b, fb, wet, dry);
            *reinterpret_cast<float4*>(o + e) = y;
        } else {
            for (long long k = e; k < e1; k++) o[k] = sat_map<CURVE>(in[k], g, b, fb, wet, dry);
        }
    }
}

// M = 1, any view: samples [n_from, n_to) of every stream-channel
template <int CURVE>
__global__ __launch_bounds__(kSatMapBlock) void sat_map_kernel(SigViewD src, OutViewD out, long long n_from, long long n_to, long long per, int ch,
                                                               float g, float b, float wet, float dry)
{
    const long long s = blockIdx.x / per, blk = blockIdx.x - s * per;
    const float fb = sat_curve<CURVE>(b);
    const long long n = (n_to - n_from) * ch;
    const long long first = blk * kSatMapBlock * kSatMapPer;
#pragma unroll
    for (int j = 0; j < kSatMapPer; j++) {
        const long long e = first + (long long)j * kSatMapBlock + threadIdx.x;
        if (e < n) {
            const long long i = n_from + e / ch;
            const int c = (int)(e % ch);
            out.base[s * out.ss + c * out.cs + i * out.fs] = sat_map<CURVE>(src.base[s * src.ss + c * src.cs + i * src.fs], g, b, fb, wet, dry);
        }
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

static inline bool sat_os_ok(int m) { return m == 1 || m == 2 || m == 4 || m == 8; }

// the one statement of the parameter rules of nae_sat_block_f32 and nae_sat_create (ctx may be null: no message then)
int nae_sat_check(nae_ctx* ctx, const nae_sat_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "sat: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!isfinite(p->drive) || !isfinite(p->bias) || !isfinite(p->wet) || !isfinite(p->dry)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "sat: non-finite parameter");
    if (p->curve != NAE_SAT_SOFT && p->curve != NAE_SAT_HARD) return nae_fail_opt(ctx, NAE_ERR_INVALID, "sat: unknown curve");
    if (!sat_os_ok(p->oversample)) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "sat: oversample must be 1, 2, 4 or 8");
    return NAE_OK;
}

// Chunks per wave of a launch over `chunks` chunks of n_sc stream-channels: the one tile rule (nae_pick_tile) for the eight waves a CU holds, so
// a small batch is cut until the CUs are full, and never more than kSatTileMax chunks: at 1024 stereo streams x 10 s whole streams (469
// chunks a wave, one round of waves that load and compute in step) measured 9.4 / 12.6 / 23.4 ms at M = 2 / 4 / 8, tiles of 59 chunks
// 7.3 / 11.0 / 20.5 ms and tiles of 8 chunks 6.8 / 10.4 / 19.2 ms; tiles of 16, 4 and 2 chunks lie behind 8 (profiles/r26_sat.md); a tile's
// first piece pays one pass of eight lanes for its halo.  sat_tile forces the tile.  Every tile gives the same bits.
constexpr int kSatTileMax = 8;
int nae_pick_sat_tile(nae_ctx* ctx, size_t chunks, size_t n_sc)
{
    const int tile = nae_pick_tile(ctx, ctx->sat_tile, chunks, n_sc, 8, 1, false);
    return ctx->sat_tile > 0 || tile < kSatTileMax ? tile : kSatTileMax;
}

// the device taps of oversampling factor M = 2, 4, 8 (slot 0, 1, 2 of the context's table: [hd | hu] each), uploaded at M's first call; the
// slots stay, so changing M between calls neither waits nor uploads again
static int sat_taps_dev(nae_ctx* ctx, int M, const float** d_taps)
{
    const int slot = M == 2 ? 0 : M == 4 ? 1 : 2;
    (void)nae_use_device(ctx);
    if (!ctx->sat_taps.p) {
        ctx->sat_taps_have = 0;
        const int rc = ctx->sat_taps.reserve(ctx, 3 * kSatSlot * sizeof(float), "sat taps");
        if (rc) return rc;
    }
    float* d_slot = ctx->sat_taps.as<float>() + slot * kSatSlot;
    if (!(ctx->sat_taps_have & (1 << slot))) {
        float h[kSatSlot] = {};
        const int n = nae_sat_taps(M, h);
        if (n != 2 * kSatK * M + 1) return nae_fail(ctx, NAE_ERR_INVALID, "sat: tap design failed");
        for (int j = 0; j < n; j++) h[kSatTapRow + j] = (float)M * h[j];          // exact: M is a power of two
        hipError_t e = hipMemcpyAsync(d_slot, h, kSatSlot * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return nae_check(ctx, e, "sat: taps upload");
        ctx->sat_taps_have |= 1 << slot;
    }
    *d_taps = d_slot;
    return NAE_OK;
}

static inline bool sat_flat_view(const void* base, long long ss, long long cs, long long fs, int ch)
{
    return ((uintptr_t)base & 15) == 0 && ss % 4 == 0 && fs == ch && (ch == 1 || cs == 1);
}

template <int CURVE>
static int launch_sat_curve(nae_ctx* ctx, const nae_sat_params* sp, const SigViewD& s, const OutViewD& d, size_t in_len, int ch, size_t n_streams,
                            size_t c_origin, size_t c_stop)
{
    const int M = sp->oversample;
    if (M == 1) {
        const long long n_from = (long long)c_origin * kChunkC;
        long long n_to = (long long)c_stop * kChunkC;
        if (n_to > (long long)in_len) n_to = (long long)in_len;
        if (n_to <= n_from) return NAE_OK;
        const long long n = (n_to - n_from) * ch, per_wg = (long long)kSatMapBlock * kSatMapPer;
        if (sat_flat_view(s.base, s.ss, s.cs, s.fs, ch) && sat_flat_view(d.base, d.ss, d.cs, d.fs, ch)) {
            const long long per = (n + 4 * per_wg - 1) / (4 * per_wg);
            return nae_launch_tiles(ctx, "sat_map_flat_kernel", "sat_map_flat_kernel: grid too large", sat_map_flat_kernel<CURVE>, per * (long long)n_streams, 1,
                                    kSatMapBlock, 0, s, d, n_from * ch, n_to * ch, per, sp->drive, sp->bias, sp->wet, sp->dry);
        }
        const long long per = (n + per_wg - 1) / per_wg;
        return nae_launch_tiles(ctx, "sat_map_kernel", "sat_map_kernel: grid too large", sat_map_kernel<CURVE>, per * (long long)n_streams, 1, kSatMapBlock, 0,
                                s, d, n_from, n_to, per, ch, sp->drive, sp->bias, sp->wet, sp->dry);
    }
    const float* d_taps = nullptr;
    const int rc = sat_taps_dev(ctx, M, &d_taps);
    if (rc) return rc;
    const size_t chunks = c_stop - c_origin, n_sc = n_streams * (size_t)ch;
    SatParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.tile = nae_pick_sat_tile(ctx, chunks, n_sc);
    p.n_tiles = (long long)((chunks + (size_t)p.tile - 1) / (size_t)p.tile);
    p.n_items = (long long)n_sc * p.n_tiles;
    p.ch = ch;
    p.g = sp->drive;
    p.b = sp->bias;
    p.wet = sp->wet;
    p.dry = sp->dry;
    // one workgroup of one wave per (stream-channel, tile)
    if (M == 2) return nae_launch_tiles(ctx, "sat_kernel", "sat_kernel: grid too large", sat_kernel<2, CURVE>, p.n_items, 1, 64, 0, s, d, p, d_taps);
    if (M == 4) return nae_launch_tiles(ctx, "sat_kernel", "sat_kernel: grid too large", sat_kernel<4, CURVE>, p.n_items, 1, 64, 0, s, d, p, d_taps);
    return nae_launch_tiles(ctx, "sat_kernel", "sat_kernel: grid too large", sat_kernel<8, CURVE>, p.n_items, 1, 64, 0, s, d, p, d_taps);
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); reads from 64 samples in front of c_origin on
int nae_launch_sat(nae_ctx* ctx, const nae_sat_params* sp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                   size_t c_origin, size_t c_stop)
{
    if (c_stop <= c_origin || n_streams == 0 || in_len == 0) return NAE_OK;
    if (sp->curve == NAE_SAT_SOFT) return launch_sat_curve<NAE_SAT_SOFT>(ctx, sp, to_view(src), to_out(dst), in_len, ch, n_streams, c_origin, c_stop);
    return launch_sat_curve<NAE_SAT_HARD>(ctx, sp, to_view(src), to_out(dst), in_len, ch, n_streams, c_origin, c_stop);
}

extern "C" {

int nae_sat_latency(int oversample) { return oversample == 1 ? 0 : (sat_os_ok(oversample) ? kSatD : -1); }

int nae_sat_taps(int oversample, float* hd_host)
{
    if (!hd_host || !sat_os_ok(oversample) || oversample == 1) return 0;
    const int n = 2 * kSatK * oversample + 1;
    return nae_fir_design(0, 2 * oversample, 0.0, 1.0, n, hd_host) == NAE_OK ? n : 0;
}

// DESIGN.md §3, "K18 saturation", "Design"
int nae_sat_design(double drive_db, double bias, int curve, int oversample, double output_db, double mix, nae_sat_params* out)
{
    if (!out) return NAE_ERR_INVALID;
    if (!isfinite(drive_db) || !isfinite(bias) || !isfinite(output_db) || !isfinite(mix)) return NAE_ERR_INVALID;
    if (drive_db < 0.0 || drive_db > 48.0 || bias < 0.0 || bias > 1.0 || output_db < -24.0 || output_db > 24.0 || mix < 0.0 || mix > 1.0) return NAE_ERR_INVALID;
    if (curve != NAE_SAT_SOFT && curve != NAE_SAT_HARD) return NAE_ERR_INVALID;
    if (!sat_os_ok(oversample)) return NAE_ERR_UNSUPPORTED;
    nae_sat_params p;
    memset(&p, 0, sizeof(p));
    p.oversample = oversample;
    p.curve = curve;
    p.drive = (float)pow(10.0, drive_db / 20.0);
    p.bias = (float)bias;
    p.wet = (float)(mix * pow(10.0, output_db / 20.0));
    p.dry = (float)(1.0 - mix);
    *out = p;
    return NAE_OK;
}

int nae_sat_block_f32(nae_ctx* ctx, const nae_sat_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "sat: null pointer");
    const int rc = nae_sat_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "sat: null pointer");
    // a tile's halo is read after a neighbouring wave may have written it: not in place
    if (src->base == dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "sat: dst must not overlap src");
    return nae_launch_sat(ctx, params, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len));
}

} // extern "C"
