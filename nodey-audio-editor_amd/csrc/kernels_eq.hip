// kernels_eq.hip — K11, the biquad cascade ("K11 biquad cascade") for gfx950: a recurrence computed parallel in time.
//
// One wave per stream-channel walks its chunks of C = 64 T samples (T = NAE_EQ_LANE = 16) in order.  A chunk is loaded coalesced (64
// consecutive samples per load, 4 KiB of f32 per chunk) into LDS; lane l then reads its own T consecutive samples with a stride of T + 1
// words between lanes, which is odd, so the 32 lanes of a ds_read_b32 group fall on 32 different banks.  Per section the lane runs the
// recurrence from the zero state over its samples (y0 and the end state e_l), the wave scans the 64 end states in six Kogge-Stone steps with
// the powers Phi^(2^j) of the T-step state map — the cross-lane moves are __shfl_up of a double, two 32-bit moves each —, and every sample gets
// the zero-input response of the state its lane starts from: y = y0 + ((p[k] z1) + (q[k] z2)).  The samples stay in registers as doubles from
// section to section and are rounded once behind the last.  The carry state of section s between chunks is kept by lane s: (z1, z2) in two
// register pairs, read by a broadcast and replaced by the scan's last value; a handle keeps it in device memory between launches.  Everything
// that depends on the coefficients — p, q and the six maps — is made on the host in double-double (eq_make_tables) into a constant block of
// 16 x (5 + 56) doubles.  The coefficients and the maps are read from it at wave-uniform addresses; p and q of the call's sections are copied
// into LDS once per launch and read there as broadcasts (read from the block they cost 28 SGPR spills).
// The translation unit is built with -ffp-contract=off: every step is one IEEE operation, in the order of the CPU statement
// (tests/eq_ref/ref_eq.c).  The tiling and the LDS stage stand in chunk_stage.h, which every chunked kernel shares; the section's steps, the copy
// of p and q and the carries' way in and out in eq_cascade.h, which the loudness meter, the keyed dynamics and the echo run too.
#include "eq_cascade.h"
#include <math.h>
#include <string.h>

namespace nae {

struct EqParams {
    long long in_len;      // samples of a stream-channel: reads at or past in_len give zero, samples there are not stored
    long long c_origin;    // chunks [c_origin, c_stop) are computed (a handle continues where it stopped)
    long long c_stop;
    long long n_sc;        // stream-channels: one wave each
    int ch, n_sections;
};

// state: [n_sc][NAE_EQ_MAX_SECTIONS][2] doubles, the carry (z1, z2) of every section in front of chunk c_origin, replaced by the one behind chunk
// c_stop - 1; null: zero in, nothing out (the block call)
__global__ __launch_bounds__(64) void eq_cascade_kernel(SigViewD src, OutViewD out, EqParams p, const double* __restrict__ tab, double* state)
{
    __shared__ float stage[kChunkStage];
    __shared__ double pq[NAE_EQ_MAX_SECTIONS * 2 * kChunkT];   // p and q of every section: read at wave-uniform addresses (a broadcast)
    const int lane = threadIdx.x;
    const long long sc = blockIdx.x;
    if (sc >= p.n_sc) return;
    eq_stage_pq(pq, tab, p.n_sections, lane, 64);
    chunk_lds_sync();
    const long long s_idx = sc / p.ch;
    const int c = (int)(sc % p.ch);
    const float* ip = src.base + s_idx * src.ss + c * src.cs;
    float* op = out.base + s_idx * out.ss + c * out.cs;
    const int S = p.n_sections;

    double st1, st2;                                       // lane s: the carry of section s
    eq_carry_load(state, sc, NAE_EQ_MAX_SECTIONS, lane, S, st1, st2);
#pragma unroll 1
    for (long long ck = p.c_origin; ck < p.c_stop; ck++) {
        const long long n0 = ck * kChunkC;
        chunk_load<false, kChunkT>(stage, ip, src.fs, n0, p.in_len, lane);
        chunk_lds_sync();
        double x[kChunkT];
        chunk_lane_read(stage, lane, x);
#pragma unroll 1
        for (int s = 0; s < S; s++) {
            eq_section(x, s, lane, tab, pq, st1, st2);
        }
        // the lanes read their own words above and write only them here; the coalesced read below needs the other lanes' words
        chunk_lane_write(stage, lane, x);
        chunk_lds_sync();
        chunk_store<kChunkT>(stage, op, out.fs, n0, p.in_len, lane);
        chunk_lds_sync();                                  // the next chunk rewrites the stage
    }
    eq_carry_store(state, sc, NAE_EQ_MAX_SECTIONS, lane, S, st1, st2);
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

size_t nae_eq_block_doubles() { return kEqBlockDoubles; }

// the one statement of the parameter rules of nae_eq_block_f32 and nae_eq_create (ctx may be null: no message then)
int nae_eq_check(nae_ctx* ctx, const double* coef, int n_sections, int ch)
{
    if (!coef) return nae_fail_opt(ctx, NAE_ERR_INVALID, "eq: null pointer");
    if (n_sections < 1) return nae_fail_opt(ctx, NAE_ERR_INVALID, "eq: n_sections must be at least 1");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (n_sections > NAE_EQ_MAX_SECTIONS) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "eq: at most 16 sections");
    for (int s = 0; s < n_sections; s++) {
        const double* c = coef + 5 * s;
        for (int i = 0; i < 5; i++)
            if (!isfinite(c[i])) return nae_fail_opt(ctx, NAE_ERR_INVALID, "eq: non-finite coefficient");
        if (!(fabs(c[4]) < 1.0 && fabs(c[3]) < 1.0 + c[4])) return nae_fail_opt(ctx, NAE_ERR_INVALID, "eq: section is not strictly stable");
    }
    return NAE_OK;
}

// Double-double arithmetic for the tables: a value is hi + lo with |lo| <= ulp(hi) / 2, about 106 bits.  Every line is plain IEEE double
// arithmetic (two-sum, and a two-product by fma()), written operation for operation as in tests/eq_ref/ref_eq.c: the two must give the same bits.
struct EqDD { double hi, lo; };

static EqDD dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return EqDD{s, (a - (s - bb)) + (b - bb)};
}

// |a| >= |b| or a == 0
static EqDD dd_quick_sum(double a, double b)
{
    const double s = a + b;
    return EqDD{s, b - (s - a)};
}

static EqDD dd_two_prod(double a, double b)
{
    const double p = a * b;
    return EqDD{p, fma(a, b, -p)};
}

static EqDD dd_add(EqDD x, EqDD y)
{
    EqDD s = dd_two_sum(x.hi, y.hi);
    const EqDD t = dd_two_sum(x.lo, y.lo);
    s = dd_quick_sum(s.hi, s.lo + t.hi);
    return dd_quick_sum(s.hi, s.lo + t.lo);
}

static EqDD dd_mul(EqDD x, EqDD y)
{
    const EqDD p = dd_two_prod(x.hi, y.hi);
    return dd_quick_sum(p.hi, p.lo + ((x.hi * y.lo) + (x.lo * y.hi)));
}

// DESIGN.md §3, "K11 biquad cascade", step 2: the constant block of a cascade.  p, q and the six maps by the zero-input recurrence in its literal
// order and five squarings, all in double-double; every entry is rounded to double once, at the end
void eq_make_tables(const double* coef, int n_sections, double* blk)
{
    memset(blk, 0, kEqBlockDoubles * sizeof(double));
    for (int s = 0; s < n_sections; s++) {
        const EqDD na1 = {-coef[5 * s + 3], 0.0}, na2 = {-coef[5 * s + 4], 0.0};
        memcpy(blk + s * kEqCoefs, coef + 5 * s, 5 * sizeof(double));
        double* t = blk + kEqTabOfs + s * kEqTab;
        double* ph = t + 2 * kChunkT;
        EqDD m[4], r[4];
        for (int col = 0; col < 2; col++) {
            EqDD z1 = {col == 0 ? 1.0 : 0.0, 0.0}, z2 = {col == 0 ? 0.0 : 1.0, 0.0};
            for (int n = 0; n < kChunkT; n++) {
                const EqDD y = z1;
                z1 = dd_add(dd_mul(na1, y), z2);
                z2 = dd_mul(na2, y);
                t[col * kChunkT + n] = y.hi + y.lo;
            }
            m[col] = z1;           // Phi: the two end states as columns, stored m00 m01 m10 m11
            m[2 + col] = z2;
        }
        for (int j = 0; j < 6; j++) {
            for (int i = 0; i < 4; i++) ph[4 * j + i] = m[i].hi + m[i].lo;
            r[0] = dd_add(dd_mul(m[0], m[0]), dd_mul(m[1], m[2]));
            r[1] = dd_add(dd_mul(m[0], m[1]), dd_mul(m[1], m[3]));
            r[2] = dd_add(dd_mul(m[2], m[0]), dd_mul(m[3], m[2]));
            r[3] = dd_add(dd_mul(m[2], m[1]), dd_mul(m[3], m[3]));
            for (int i = 0; i < 4; i++) m[i] = r[i];
        }
    }
}

// the constant block of checked coefficients into d_block (nae_eq_block_doubles() doubles); waits for the upload
int nae_eq_make_block(nae_ctx* ctx, const double* coef, int n_sections, double* d_block)
{
    std::vector<double> blk(kEqBlockDoubles);
    eq_make_tables(coef, n_sections, blk.data());
    (void)nae_use_device(ctx);
    hipError_t e = hipMemcpyAsync(d_block, blk.data(), kEqBlockDoubles * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e == hipSuccess ? NAE_OK : nae_check(ctx, e, "eq: table upload");
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples (absolute indexing); d_state as the kernel's
int nae_launch_eq(nae_ctx* ctx, const double* d_block, int n_sections, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                  const nae_sig* dst, size_t c_origin, size_t c_stop, double* d_state)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    const size_t n_sc = n_streams * (size_t)ch;
    EqParams p;
    p.in_len = (long long)in_len;
    p.c_origin = (long long)c_origin;
    p.c_stop = (long long)c_stop;
    p.n_sc = (long long)n_sc;
    p.ch = ch;
    p.n_sections = n_sections;
    // one wave per stream-channel
    return nae_launch_tiles(ctx, "eq_cascade_kernel", "eq_cascade_kernel: grid too large", eq_cascade_kernel, p.n_sc, 1, 64, 0, to_view(src), to_out(dst),
                            p, d_block, d_state);
}

// the context's constant block of checked coefficients: the tables are kept with the context, so a call with the coefficients of the last one
// uploads nothing (nae_eq_block_f32, and the key filter of nae_dynkey_block_f32)
int nae_eq_cached_block(nae_ctx* ctx, const double* coef_host, int n_sections, double** d_block)
{
    (void)nae_use_device(ctx);
    const size_t n_coef = (size_t)n_sections * 5;
    const int rc = ctx->eq_block.get(ctx, {}, coef_host, n_coef * sizeof(double), kEqBlockDoubles * sizeof(double), "eq tables",
                                     [&] { return nae_eq_make_block(ctx, coef_host, n_sections, ctx->eq_block.as<double>()); });
    *d_block = ctx->eq_block.as<double>();
    return rc;
}

extern "C" {

int nae_eq_block_f32(nae_ctx* ctx, const double* coef_host, int n_sections, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                     const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!coef_host || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "eq: null pointer");
    int rc = nae_eq_check(ctx, coef_host, n_sections, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "eq: null pointer");
    double* d_block = nullptr;
    if ((rc = nae_eq_cached_block(ctx, coef_host, n_sections, &d_block))) return rc;
    return nae_launch_eq(ctx, d_block, n_sections, src, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr);
}

// DESIGN.md §3, "K11 biquad cascade", "Design": the Audio EQ Cookbook's forms in double, divided through by a0
int nae_eq_design(int kind, int sample_rate, double freq, double gain_db, double q, double coef_host[5])
{
    if (!coef_host || kind < NAE_EQ_PEAK || kind > NAE_EQ_NOTCH || sample_rate <= 0) return NAE_ERR_INVALID;
    if (!(freq > 0.0 && freq < 0.5 * (double)sample_rate)) return NAE_ERR_INVALID;
    if (!(q >= NAE_EQ_MIN_Q && q <= NAE_EQ_MAX_Q)) return NAE_ERR_INVALID;
    if (!(fabs(gain_db) <= NAE_EQ_MAX_GAIN_DB)) return NAE_ERR_INVALID;
    const double pi = 3.14159265358979323846;
    const double A = pow(10.0, gain_db / 40.0);
    const double w0 = 2.0 * pi * freq / (double)sample_rate;
    const double cs = cos(w0), alpha = sin(w0) / (2.0 * q);
    double b0, b1, b2, a0, a1, a2;
    if (kind == NAE_EQ_PEAK) {
        b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
    } else if (kind == NAE_EQ_LOWSHELF) {
        const double r = 2.0 * sqrt(A) * alpha;
        b0 = A * ((A + 1.0) - (A - 1.0) * cs + r); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs); b2 = A * ((A + 1.0) - (A - 1.0) * cs - r);
        a0 = (A + 1.0) + (A - 1.0) * cs + r; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - r;
    } else if (kind == NAE_EQ_HIGHSHELF) {
        const double r = 2.0 * sqrt(A) * alpha;
        b0 = A * ((A + 1.0) + (A - 1.0) * cs + r); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs); b2 = A * ((A + 1.0) + (A - 1.0) * cs - r);
        a0 = (A + 1.0) - (A - 1.0) * cs + r; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - r;
    } else {
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        if (kind == NAE_EQ_LOWPASS) { b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = (1.0 - cs) / 2.0; }
        else if (kind == NAE_EQ_HIGHPASS) { b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = (1.0 + cs) / 2.0; }
        else { b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0; }
    }
    coef_host[0] = b0 / a0;
    coef_host[1] = b1 / a0;
    coef_host[2] = b2 / a0;
    coef_host[3] = a1 / a0;
    coef_host[4] = a2 / a0;
    return NAE_OK;
}

} // extern "C"
