// kernels_loud.hip — K14, the loudness meter and normalizer ("K14 loudness") for gfx950: ITU-R BS.1770-4 / EBU R 128.
//
// loud_measure_kernel: one wave per stream-channel walks its chunks of 1024 samples in order, as K11 does (chunk_stage.h): a chunk is loaded
// coalesced into LDS and lane l reads its own 16 samples at a stride of 17 words.  In one pass over the chunk the lane runs the four phases of
// the true-peak oversampler on the staged f32 samples (its own 16 and the 11 in front of them, which are the lane before's; the 11 in front of
// the chunk stand in the stage's first row, where lane 63 leaves its samples for the next chunk), the K-weighting — K11's cascade with two
// sections, kept in double — and the squares: per 100 ms sub-block the chunk meets (up to three at 8 kHz; a boundary may fall inside a lane's
// samples) the lane's sum, a butterfly over the wave, and the sum onto the open sub-block, which is wave-uniform in a register pair and goes
// to the sub-block array when the next one opens.  What a handle needs to continue — the sections' carries, the peaks, the 11 samples — is in
// one LoudState per stream-channel; the open sub-block's sum is its entry of the array.
// loud_gate_kernel: one lane per stream runs the 400 ms blocks in order, twice: the absolute gate and the mean behind it, then the relative
// gate; compared in energy, so there is no logarithm on the device.  It writes the stream's nae_loud_result.
// loud_apply_kernel: y = x gain_f32 of the stream's record, through any view.
// The translation unit is built with -ffp-contract=off: every step is one IEEE operation, in the order of the CPU statement
// (tests/loud_ref/ref_loud.c).
#include "eq_cascade.h"
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kLdS = NAE_LOUD_SECTIONS, kLdPhases = NAE_LOUD_TP_PHASES, kLdTaps = NAE_LOUD_TP_TAPS, kLdHist = kLdTaps - 1;
constexpr int kLdTapCount = kLdPhases * kLdTaps;
// the stage: row r = 0 ... 64 of 16 samples at 17 r; row 0 is the 16 samples in front of the chunk, row l + 1 lane l's
constexpr int kLdStage = (kChunkC + kChunkT) + (kChunkC + kChunkT) / kChunkT;
// the constant block: K11's block of the two sections, then the 48 taps [phase][k] as f32
constexpr size_t kLdBlockBytes = kEqBlockDoubles * sizeof(double) + kLdTapCount * sizeof(float);
static_assert(kLdHist <= kChunkT && kLdS <= NAE_EQ_MAX_SECTIONS, "the history is part of one lane's samples");

// what a stream-channel carries between two launches; all zero in front of sample 0
struct LoudState {
    double z[kLdS][2];     // the sections' carries (z1, z2)
    float true_peak, sample_peak;
    float hist[kChunkT];   // the 16 samples in front of the next chunk (the last 11 are read)
};

struct LoudParams {
    long long in_len;      // samples of a stream-channel: reads at or past in_len give zero; the true peak runs to sample in_len + 10
    long long c_origin;    // chunks [c_origin, c_stop) are measured (a handle continues where it stopped)
    long long c_stop;
    long long n_sc;        // stream-channels: one wave each
    long long e_ss;        // doubles between two streams' sub-block energies; sub-block u of channel c at [u * ch + c]
    long long n_sub;       // sub-blocks per stream-channel the array has room for: sums of later ones are dropped
    int ch, B;             // B: samples per sub-block
};

__global__ __launch_bounds__(64) void loud_measure_kernel(SigViewD src, LoudParams p, const double* __restrict__ tab, LoudState* state, double* E)
{
    __shared__ float stage[kLdStage];
    __shared__ double pq[kLdS * 2 * kChunkT];
    const int lane = threadIdx.x;
    const long long sc = blockIdx.x;
    if (sc >= p.n_sc) return;
    const float* __restrict__ taps = reinterpret_cast<const float*>(tab + kEqBlockDoubles);
    LoudState* st = state + sc;
    eq_stage_pq(pq, tab, kLdS, lane, 64);
    if (lane < kChunkT) stage[lane] = st->hist[lane];
    const long long s_idx = sc / p.ch;
    const int c = (int)(sc % p.ch);
    const float* ip = src.base + s_idx * src.ss + c * src.cs;
    double* Esc = E + s_idx * p.e_ss + c;

    double st1 = 0.0, st2 = 0.0;                           // lane s: the carry of section s
    if (lane < kLdS) {
        st1 = st->z[lane][0];
        st2 = st->z[lane][1];
    }
    float tp = 0.0f, sp = 0.0f;                            // this lane's peaks over the launch
    long long u_open = p.c_origin * kChunkC / p.B;         // the open sub-block and its sum so far (wave-uniform)
    double e_open = u_open < p.n_sub ? Esc[u_open * p.ch] : 0.0;
    const long long tp_stop = p.in_len + kLdHist;          // v_p[n] counts for n < tp_stop
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        chunk_load<false, kChunkT>(stage + kChunkStride, ip, src.fs, n0, p.in_len, lane);   // behind row 0
        chunk_lds_sync();
        // xs[i]: sample 16 lane - 11 + i of the chunk: the last 11 of the row above, then the lane's own
        float xs[kLdHist + kChunkT];
#pragma unroll
        for (int i = 0; i < kLdHist; i++) xs[i] = stage[lane * kChunkStride + (kChunkT - kLdHist) + i];
        chunk_lane_read(stage + kChunkStride, lane, xs + kLdHist);
        // every lane has read the row above it; lane 63's samples are the next chunk's row 0
        if (lane == 63) {
#pragma unroll
            for (int k = 0; k < kChunkT; k++) stage[k] = xs[kLdHist + k];
        }
        // the peaks
        const long long n_lane = n0 + lane * kChunkT;
#pragma unroll
        for (int k = 0; k < kChunkT; k++) {
            const float ax = fabsf(xs[kLdHist + k]);
            sp = ax > sp ? ax : sp;
            const bool counts = n_lane + k < tp_stop;
#pragma unroll
            for (int ph = 0; ph < kLdPhases; ph++) {
                float v = taps[ph * kLdTaps] * xs[kLdHist + k];
#pragma unroll
                for (int t = 1; t < kLdTaps; t++) v = v + taps[ph * kLdTaps + t] * xs[kLdHist + k - t];
                const float av = fabsf(v);
                tp = counts && av > tp ? av : tp;
            }
        }
        // the K-weighting
        double x[kChunkT];
#pragma unroll
        for (int k = 0; k < kChunkT; k++) x[k] = (double)xs[kLdHist + k];
#pragma unroll 1
        for (int s = 0; s < kLdS; s++) eq_section(x, s, lane, tab, pq, st1, st2);
        // the sub-blocks the chunk meets
        const long long u_last = (n0 + kChunkC - 1) / p.B;
#pragma unroll 1
        for (long long u = n0 / p.B; u <= u_last; u++) {
            // the lane's samples k of [lo, hi) lie in sub-block u
            const long long first = u * p.B - n_lane;
            const int lo = (int)(first < 0 ? 0 : first > kChunkT ? kChunkT : first), hi = (int)(first + p.B < 0 ? 0 : first + p.B > kChunkT ? kChunkT : first + p.B);
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < kChunkT; k++) {
                const double sq = x[k] * x[k];
                sum = (k >= lo && k < hi) ? sum + sq : sum;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum = sum + __shfl_xor(sum, d);
            if (u != u_open) {
                if (lane == 0 && u_open < p.n_sub) Esc[u_open * p.ch] = e_open;
                u_open = u;
                e_open = 0.0;
            }
            e_open = e_open + sum;
        }
        chunk_lds_sync();                                  // the next chunk rewrites the stage
    }
    if (lane == 0 && u_open < p.n_sub) Esc[u_open * p.ch] = e_open;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ot = __shfl_xor(tp, d), os = __shfl_xor(sp, d);
        tp = ot > tp ? ot : tp;
        sp = os > sp ? os : sp;
    }
    if (lane == 0) {
        const float t0 = st->true_peak, s0 = st->sample_peak;
        st->true_peak = tp > t0 ? tp : t0;
        st->sample_peak = sp > s0 ? sp : s0;
    }
    if (lane < kLdS) {
        st->z[lane][0] = st1;
        st->z[lane][1] = st2;
    }
    if (lane < kChunkT) st->hist[lane] = stage[lane];
}

struct LoudGateParams {
    long long n_streams, in_len, e_ss;
    int ch, B;
    double gate_abs, target, ceiling_lin, max_gain_lin;
};

// p[j] of one stream: e points at its channel 0, sub-block j
__device__ __forceinline__ double loud_block_power(const double* e, int ch, double d4b)
{
    double pw = 0.0;
    for (int c = 0; c < ch; c++) {
        const double z = ((e[c] + e[ch + c]) + (e[2 * ch + c] + e[3 * ch + c])) / d4b;
        pw = c == 0 ? z : pw + z;
    }
    return pw;
}

__global__ __launch_bounds__(64) void loud_gate_kernel(LoudGateParams p, const double* __restrict__ E, const LoudState* __restrict__ state, nae_loud_result* out)
{
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= p.n_streams) return;
    const double* e = E + s * p.e_ss;
    const long long U = p.in_len / p.B, blocks = U >= NAE_LOUD_BLOCK_SUBS ? U - (NAE_LOUD_BLOCK_SUBS - 1) : 0;
    const double d4b = (double)(NAE_LOUD_BLOCK_SUBS * (long long)p.B);
    double sum1 = 0.0, mx = 0.0;
    unsigned n_abs = 0, n_rel = 0;
#pragma unroll 1
    for (long long j = 0; j < blocks; j++) {
        const double pw = loud_block_power(e + j * p.ch, p.ch, d4b);
        mx = pw > mx ? pw : mx;
        if (pw > p.gate_abs) {
            sum1 = sum1 + pw;
            n_abs++;
        }
    }
    const double gate_rel = n_abs ? NAE_LOUD_REL_GATE * (sum1 / (double)n_abs) : 0.0;
    double sum2 = 0.0;
#pragma unroll 1
    for (long long j = 0; j < blocks; j++) {
        const double pw = loud_block_power(e + j * p.ch, p.ch, d4b);
        if (pw > p.gate_abs && pw > gate_rel) {
            sum2 = sum2 + pw;
            n_rel++;
        }
    }
    const double mean2 = n_rel ? sum2 / (double)n_rel : 0.0;
    float tpk[2] = {0.0f, 0.0f}, spk[2] = {0.0f, 0.0f};
    float peak = 0.0f;
    for (int c = 0; c < p.ch; c++) {
        tpk[c] = state[s * p.ch + c].true_peak;
        spk[c] = state[s * p.ch + c].sample_peak;
        peak = tpk[c] > peak ? tpk[c] : peak;
        peak = spk[c] > peak ? spk[c] : peak;
    }
    double g = 1.0;
    if (n_rel) {
        g = sqrt(p.target / mean2);
        if (g * (double)peak > p.ceiling_lin) g = p.ceiling_lin / (double)peak;
        g = g > p.max_gain_lin ? p.max_gain_lin : g;
    }
    nae_loud_result r;
    r.mean2 = mean2;
    r.momentary_max = mx;
    r.gain = g;
    r.gain_f32 = (float)g;
    r.true_peak[0] = tpk[0];
    r.true_peak[1] = tpk[1];
    r.sample_peak[0] = spk[0];
    r.sample_peak[1] = spk[1];
    r.blocks_total = (unsigned)blocks;
    r.blocks_abs = n_abs;
    r.blocks_rel = n_rel;
    out[s] = r;
}

constexpr int kLdApplyTile = 1024;   // samples of one stream-channel per workgroup of 256 threads

__global__ __launch_bounds__(256) void loud_apply_kernel(SigViewD src, OutViewD out, const nae_loud_result* __restrict__ res, long long in_len, long long tiles,
                                                          int ch)
{
    const long long sc = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const long long s_idx = sc / ch;
    const int c = (int)(sc % ch);
    const float g = res[s_idx].gain_f32;
    const float* ip = src.base + s_idx * src.ss + c * src.cs;
    float* op = out.base + s_idx * out.ss + c * out.cs;
#pragma unroll
    for (int j = 0; j < kLdApplyTile / 256; j++) {
        const long long i = tile * kLdApplyTile + j * 256 + threadIdx.x;
        if (i < in_len) op[i * out.fs] = ip[i * src.fs] * g;
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

size_t nae_loud_block_bytes() { return kLdBlockBytes; }
size_t nae_loud_state_bytes() { return sizeof(LoudState); }

// DESIGN.md §3, "K14 loudness", "True peak": the 48-tap Kaiser-windowed sinc in double, split into four phases of twelve taps, every phase
// divided by its own sum and rounded once: out[phase][k]
void nae_loud_taps(float* out)
{
    const double pi = 3.14159265358979323846;
    const double half = 0.5 * (double)(kLdTapCount - 1), i0b = nae_bessel_i0(NAE_FIR_KAISER_BETA);
    double h[kLdTapCount];
    for (int i = 0; i < kLdTapCount; i++) {
        const double t = (double)i - half;
        const double a = t / half;
        const double r = 1.0 - a * a;
        const double w = nae_bessel_i0(NAE_FIR_KAISER_BETA * sqrt(r > 0.0 ? r : 0.0)) / i0b;
        const double arg = pi * (t / (double)kLdPhases);
        h[i] = sin(arg) / arg * w;
    }
    for (int ph = 0; ph < kLdPhases; ph++) {
        double sum = 0.0;
        for (int k = 0; k < kLdTaps; k++) sum += h[ph + kLdPhases * k];
        for (int k = 0; k < kLdTaps; k++) out[ph * kLdTaps + k] = (float)(h[ph + kLdPhases * k] / sum);
    }
}

static bool loud_rate_ok(int sample_rate)
{
    return sample_rate >= NAE_LOUD_MIN_RATE && sample_rate <= NAE_LOUD_MAX_RATE && sample_rate % NAE_LOUD_SUBS_PER_S == 0;
}

// the one statement of the parameter rules of the block entries and nae_loud_create (ctx may be null: no message then)
int nae_loud_check(nae_ctx* ctx, const nae_loud_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "loud: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (!loud_rate_ok(p->sample_rate)) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "loud: the sample rate must be 8000 ... 192000 and a multiple of 10");
    if (p->sub_block != p->sample_rate / NAE_LOUD_SUBS_PER_S) return nae_fail_opt(ctx, NAE_ERR_INVALID, "loud: sub_block is not sample_rate / 10");
    const int rc = nae_eq_check(ctx, p->coef, kLdS, ch);
    if (rc) return rc;
    for (const double v : {p->gate_abs, p->target, p->ceiling_lin, p->max_gain_lin})
        if (!(isfinite(v) && v > 0.0)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "loud: a level is not positive and finite");
    return NAE_OK;
}

// the constant block of checked parameters into d_block (nae_loud_block_bytes() bytes); waits for the upload
int nae_loud_make_block(nae_ctx* ctx, const nae_loud_params* p, void* d_block)
{
    std::vector<double> blk(kLdBlockBytes / sizeof(double));
    eq_make_tables(p->coef, kLdS, blk.data());
    nae_loud_taps(reinterpret_cast<float*>(blk.data() + kEqBlockDoubles));
    (void)nae_use_device(ctx);
    hipError_t e = hipMemcpyAsync(d_block, blk.data(), kLdBlockBytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? NAE_OK : nae_check(ctx, e, "loud: table upload");
}

size_t nae_loud_chunks(size_t in_len, bool flushed)
{
    return flushed ? (in_len ? nae_chunks(in_len + kLdHist) : 0) : in_len / kChunkC;
}

int nae_launch_loud_measure(nae_ctx* ctx, const nae_loud_params* p, const void* d_block, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                            size_t c_origin, size_t c_stop, void* d_state, double* d_E, size_t e_ss, size_t n_sub)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    LoudParams q;
    q.in_len = (long long)in_len;
    q.c_origin = (long long)c_origin;
    q.c_stop = (long long)c_stop;
    q.n_sc = (long long)(n_streams * (size_t)ch);
    q.e_ss = (long long)e_ss;
    q.n_sub = (long long)n_sub;
    q.ch = ch;
    q.B = p->sub_block;
    // one wave per stream-channel
    return nae_launch_tiles(ctx, "loud_measure_kernel", "loud_measure_kernel: grid too large", loud_measure_kernel, q.n_sc, 1, 64, 0, to_view(src), q,
                            static_cast<const double*>(d_block), static_cast<LoudState*>(d_state), d_E);
}

int nae_launch_loud_gate(nae_ctx* ctx, const nae_loud_params* p, size_t in_len, int ch, size_t n_streams, const void* d_state, const double* d_E,
                         size_t e_ss, nae_loud_result* d_results)
{
    if (n_streams == 0) return NAE_OK;
    LoudGateParams q;
    q.n_streams = (long long)n_streams;
    q.in_len = (long long)in_len;
    q.e_ss = (long long)e_ss;
    q.ch = ch;
    q.B = p->sub_block;
    q.gate_abs = p->gate_abs;
    q.target = p->target;
    q.ceiling_lin = p->ceiling_lin;
    q.max_gain_lin = p->max_gain_lin;
    // one lane per stream
    return nae_launch_tiles(ctx, "loud_gate_kernel", "loud_gate_kernel: grid too large", loud_gate_kernel, q.n_streams, 64, 64, 0, q, d_E,
                            static_cast<const LoudState*>(d_state), d_results);
}

// measure into `results` (device; null: the records in the context's workspace), which *used receives
static int loud_measure(nae_ctx* ctx, const nae_loud_params* p, const nae_sig* src, size_t in_len, int ch, size_t n_streams, nae_loud_result* results,
                        nae_loud_result** used)
{
    (void)nae_use_device(ctx);
    // the tables are kept with the context: a call with the coefficients of the last one uploads nothing
    int rc = ctx->loud_block.get(ctx, {}, p->coef, sizeof(p->coef), kLdBlockBytes, "loud tables",
                                 [&] { return nae_loud_make_block(ctx, p, ctx->loud_block.dev.p); });
    if (rc) return rc;
    // the workspace: [stream-channel] LoudState | [stream][sub-block][channel] doubles | [stream] records
    const size_t n_sc = n_streams * (size_t)ch;
    const size_t U = in_len / (size_t)p->sub_block, n_sub = U ? U : 1, e_ss = n_sub * (size_t)ch;
    const size_t state_bytes = n_sc * sizeof(LoudState), e_bytes = n_streams * e_ss * sizeof(double);
    rc = ctx->ws_loud.reserve(ctx, state_bytes + e_bytes + n_streams * sizeof(nae_loud_result), "workspace");
    if (rc) return rc;
    char* ws = ctx->ws_loud.as<char>();
    double* d_E = reinterpret_cast<double*>(ws + state_bytes);
    *used = results ? results : reinterpret_cast<nae_loud_result*>(ws + state_bytes + e_bytes);
    rc = nae_check(ctx, hipMemsetAsync(ws, 0, state_bytes + e_bytes, ctx->stream), "hipMemsetAsync(loud workspace)");
    if (!rc) rc = nae_launch_loud_measure(ctx, p, ctx->loud_block.dev.p, src, in_len, ch, n_streams, 0, nae_loud_chunks(in_len, true), ws, d_E, e_ss, U);
    if (!rc) rc = nae_launch_loud_gate(ctx, p, in_len, ch, n_streams, ws, d_E, e_ss, *used);
    return rc;
}

static int loud_apply(nae_ctx* ctx, const nae_loud_result* results, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    const long long tiles = (long long)((in_len + kLdApplyTile - 1) / kLdApplyTile);
    return nae_launch_tiles(ctx, "loud_apply_kernel", "loud_apply_kernel: grid too large", loud_apply_kernel, (long long)(n_streams * (size_t)ch) * tiles, 1,
                            256, 0, to_view(src), to_out(dst), results, (long long)in_len, tiles, ch);
}

extern "C" {

int nae_loud_measure_f32(nae_ctx* ctx, const nae_loud_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                         nae_loud_result* results_dev)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !results_dev) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    const int rc = nae_loud_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    nae_loud_result* used = nullptr;
    return loud_measure(ctx, params, src, in_len, ch, n_streams, results_dev, &used);
}

int nae_loud_apply_f32(nae_ctx* ctx, const nae_loud_result* results_dev, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!results_dev || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    return loud_apply(ctx, results_dev, src, in_len, ch, n_streams, dst);
}

int nae_loud_normalize_f32(nae_ctx* ctx, const nae_loud_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                           const nae_sig* dst, nae_loud_result* results_dev)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    int rc = nae_loud_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "loud: null pointer");
    nae_loud_result* used = nullptr;
    rc = loud_measure(ctx, params, src, in_len, ch, n_streams, results_dev, &used);
    return rc ? rc : loud_apply(ctx, used, src, in_len, ch, n_streams, dst);
}

// DESIGN.md §3, "K14 loudness", "Design"
int nae_loud_design(int sample_rate, double target_lufs, double ceiling_dbtp, double max_gain_db, nae_loud_params* out)
{
    if (!out) return NAE_ERR_INVALID;
    if (!(target_lufs >= NAE_LOUD_MIN_TARGET_LUFS && target_lufs <= NAE_LOUD_MAX_TARGET_LUFS)) return NAE_ERR_INVALID;
    if (!(ceiling_dbtp >= NAE_LOUD_MIN_CEILING_DBTP && ceiling_dbtp <= 0.0)) return NAE_ERR_INVALID;
    if (!(max_gain_db >= 0.0 && max_gain_db <= NAE_LOUD_MAX_GAIN_DB)) return NAE_ERR_INVALID;
    if (!loud_rate_ok(sample_rate)) return NAE_ERR_UNSUPPORTED;
    const double pi = 3.14159265358979323846;
    nae_loud_params p;
    memset(&p, 0, sizeof(p));
    p.sample_rate = sample_rate;
    p.sub_block = sample_rate / NAE_LOUD_SUBS_PER_S;
    {
        const double K = tan(pi * NAE_LOUD_SHELF_F0 / (double)sample_rate);
        const double Vh = pow(10.0, NAE_LOUD_SHELF_GAIN_DB / 20.0), Vb = pow(Vh, NAE_LOUD_SHELF_VB_EXP);
        const double kq = K / NAE_LOUD_SHELF_Q, kk = K * K;
        const double a0 = 1.0 + kq + kk;
        p.coef[0] = (Vh + Vb * kq + kk) / a0;
        p.coef[1] = 2.0 * (kk - Vh) / a0;
        p.coef[2] = (Vh - Vb * kq + kk) / a0;
        p.coef[3] = 2.0 * (kk - 1.0) / a0;
        p.coef[4] = (1.0 - kq + kk) / a0;
    }
    {
        const double K = tan(pi * NAE_LOUD_HP_F0 / (double)sample_rate);
        const double kq = K / NAE_LOUD_HP_Q, kk = K * K;
        const double a0 = 1.0 + kq + kk;
        p.coef[5] = 1.0;
        p.coef[6] = -2.0;
        p.coef[7] = 1.0;
        p.coef[8] = 2.0 * (kk - 1.0) / a0;
        p.coef[9] = (1.0 - kq + kk) / a0;
    }
    p.gate_abs = pow(10.0, (NAE_LOUD_ABS_GATE_LUFS + NAE_LOUD_OFFSET) / 10.0);
    p.target = pow(10.0, (target_lufs + NAE_LOUD_OFFSET) / 10.0);
    p.ceiling_lin = pow(10.0, ceiling_dbtp / 20.0);
    p.max_gain_lin = pow(10.0, max_gain_db / 20.0);
    *out = p;
    return NAE_OK;
}

double nae_loud_lufs(double energy) { return -NAE_LOUD_OFFSET + 10.0 * log10(energy); }

} // extern "C"
