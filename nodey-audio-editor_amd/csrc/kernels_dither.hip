// kernels_dither.hip — K23, word-length reduction with TPDF dither and noise shaping ("K23 dither") for gfx950.
//
// Two kernels.  With no taps the quantiser is feed-forward: dither_flat_kernel takes four neighbouring samples per lane in 16-byte pieces
// wherever both views are dense and aligned (interleaved or planar), single ones otherwise, and is a grid over (row, tile of the row).
// With K >= 1 taps the error feedback is a non-linear recurrence: nothing scans it, only stream-channels run side by side.
// dither_ef_kernel<K, ROLES> gives a workgroup 64 stream-channels, one per lane of its walking wave (wave 0), stereo pairs in neighbouring
// lanes.  Tiles of kDitherT samples pass through LDS: an input stage of {t, d} pairs and an output stage of q, a row per stream-channel at
// an odd stride, so the walking wave's column reads (ds_read_b128) and the producers' row writes meet no bank twice.  With ROLES the four
// other waves of the workgroup are producers: in the interval in which wave 0 walks tile i they hash, scale and write {t, d} of tile i + 1
// from samples they loaded an interval earlier, issue the loads of tile i + 2, and clamp, scale and store tile i - 1; one barrier per tile,
// which orders LDS alone, so the loads stay in flight across it.
// The walking wave runs, per sample, one LDS read, K fused multiply-adds from the oldest error to the newest, one add, one round to
// nearest even, one subtract and one LDS write; the taps are kernel arguments (SGPRs), the error history K doubles in registers.
// Without ROLES (debug key dither_roles = 2) one wave does the three steps of a tile one after the other: the same bits, the price of the
// roles' absence on show.  Built with -ffp-contract=off; the fused steps are written as __builtin_fma, as the CPU statement writes fma()
// (tests/dither_ref/ref_dither.c).
#include "launch.h"
#include <math.h>
#include <string.h>

namespace nae {

constexpr int kDitherT = 16;                       // samples of a tile
constexpr int kDitherRows = 64;                    // stream-channels of a workgroup: the lanes of the walking wave
constexpr int kDitherStride = kDitherT + 1;        // row stride of both stages, in elements: odd
constexpr int kDitherProducers = 256;              // lanes of the four producer waves
// A tile is 16 slots of 64 neighbouring elements.  Waves 1 ... 3 take kDitherHeavy slots each; wave 4, which shares its SIMD with the walking
// wave, takes the one that is left
constexpr int kDitherHeavy = 5, kDitherLightWave = 4;
static_assert(3 * kDitherHeavy + 1 == kDitherRows * kDitherT / 64, "the producers' slots cover the tile");
constexpr unsigned long long kDitherGamma = 0x9E3779B97F4A7C15ull;

struct DitherParams {
    long long first, stop;     // frames [first, stop) of absolutely indexed views are computed; frame i is sample n = i of its stream
    long long n_sc;            // stream-channels
    unsigned long long seed;
    double scale, inv_scale;   // S = 2^(bits - 1) and 1 / S
    double nc[NAE_DITHER_MAX_TAPS];   // -c_1 ... -c_K
    int ch, kind;
};

// the splitmix64 finaliser (as fill_uniform_kernel's)
__device__ inline unsigned long long dither_fin(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the key of stream s, channel c under `seed`: three finalisers in a chain
__device__ inline unsigned long long dither_key(unsigned long long seed, unsigned long long s, unsigned long long c)
{
    return dither_fin(dither_fin(dither_fin(seed + kDitherGamma) + s) + c);
}
__device__ inline double dither_half(unsigned int w) { return (double)(int)w * 0x1p-32; }   // [-0.5, 0.5), exact
// d[n] in LSB
__device__ inline double dither_value(unsigned long long key, unsigned long long n, int kind)
{
    if (kind == NAE_DITHER_NONE) return 0.0;
    const unsigned long long h = dither_fin(key + kDitherGamma * n);
    const double r1 = dither_half((unsigned int)(h >> 32));
    if (kind == NAE_DITHER_RECTANGULAR) return r1;
    if (kind == NAE_DITHER_TRIANGULAR) return r1 + dither_half((unsigned int)h);
    const double before = n ? dither_half((unsigned int)(dither_fin(key + kDitherGamma * (n - 1)) >> 32)) : 0.0;
    return r1 - before;
}
// t[n]: exact; a sample that is not finite counts as zero
__device__ inline double dither_scaled(float x, double scale) { return isfinite(x) ? (double)x * scale : 0.0; }
// y[n] from q[n]: the clamp, then an exact scale and an exact rounding
__device__ inline float dither_out(double q, double scale, double inv_scale)
{
    return (float)(fmin(fmax(q, -scale), scale - 1.0) * inv_scale);      // q is never NaN
}

// ------------------------------------------------------------------------------------------------ K = 0
// Rows of `row_len` elements: with `ilv` a row is a stream and element j is frame j / ch of channel j % ch (element stride 1), else a row is
// a stream-channel and element j is frame j at stride fs.  vec: both views have element stride 1 and 16-byte aligned rows.  A workgroup
// takes 1024 elements of a row from element 4 * floor(j_first / 4) on.
__global__ __launch_bounds__(256) void dither_flat_kernel(SigViewD src, OutViewD dst, DitherParams p, long long tiles_per_row, int ilv, int vec)
{
    const long long row = blockIdx.x / tiles_per_row, tile = blockIdx.x % tiles_per_row;
    const long long per = ilv ? p.ch : 1;
    const long long j_first = p.first * per, j_stop = p.stop * per;
    const long long j0 = (j_first & ~3ll) + tile * 1024 + (long long)threadIdx.x * 4;
    if (j0 >= j_stop) return;
    const long long s = ilv ? row : row / p.ch, c0 = ilv ? 0 : row % p.ch;
    const float* ip = src.base + s * src.ss + c0 * src.cs;
    float* op = dst.base + s * dst.ss + c0 * dst.cs;
    const long long ifs = ilv ? 1 : src.fs, ofs = ilv ? 1 : dst.fs;
    const bool whole = j0 >= j_first && j0 + 4 <= j_stop;
    float x[4];
    if (vec && whole) {
        const float4 v = *reinterpret_cast<const float4*>(ip + j0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long j = j0 + k;
            x[k] = (j >= j_first && j < j_stop) ? ip[j * ifs] : 0.0f;
        }
    }
    const unsigned long long key0 = dither_key(p.seed, (unsigned long long)s, (unsigned long long)c0);
    const unsigned long long key1 = ilv && p.ch == 2 ? dither_key(p.seed, (unsigned long long)s, 1ull) : key0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long j = j0 + k;
        const bool odd = ilv && p.ch == 2 && (j & 1);
        const unsigned long long n = (unsigned long long)(ilv ? j / p.ch : j);
        const double t = dither_scaled(x[k], p.scale);
        const double q = __builtin_rint(t + dither_value(odd ? key1 : key0, n, p.kind));
        x[k] = dither_out(q, p.scale, p.inv_scale);
    }
    if (vec && whole) {
        *reinterpret_cast<float4*>(op + j0) = float4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const long long j = j0 + k;
            if (j >= j_first && j < j_stop) op[j * ofs] = x[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ K >= 1
// Element e = 0 ... 1023 of a tile as (row, column): with interleaved channels the ch rows of a stream lie side by side in memory, so
// neighbouring e are the channels of one frame, then the next frame; else neighbouring e are neighbouring frames of one row.  ch is 1 or 2.
__device__ inline void dither_element(int e, int ch, bool ilv, int& row, int& col)
{
    const int lg = ilv ? ch - 1 : 0;               // log2 of the rows that share a line
    row = ((e >> (4 + lg)) << lg) + (e & ((1 << lg) - 1));
    col = (e & ((kDitherT << lg) - 1)) >> lg;
}
static_assert(kDitherT == 16, "dither_element's shifts");

// what the workgroup keeps about its 64 rows: the key, and where the row's frame 0 lies in both views (elements from the base)
struct DitherRows {
    unsigned long long key[kDitherRows];
    long long src[kDitherRows], dst[kDitherRows];
};

// What a lane keeps about each of its PER elements of every tile, so that a tile costs it additions and no multiplication by an index: the
// element in the source's order (where it stands in the input stage, its column, its hash counter key + G n and its offset in the source)
// and the element in the destination's order (the same for the output stage and the destination).  The two orders differ where one view is
// interleaved and the other is not.  Loads, makes and stores each run over the tiles in order, and each moves its own state one tile on.
template <int PER>
struct DitherLane {
    unsigned long long ctr[PER];
    long long src[PER], dst[PER];
    int in_at[PER], q_at[PER];
    int col_in[PER], col_q[PER];       // a column of kDitherT where the row is not live
};

// the lane's elements are e = (slot0 + m) 64 + lane, m < PER: 64 neighbouring elements per instruction
template <int PER>
__device__ inline void dither_lane_init(DitherLane<PER>& L, const DitherRows& R, const SigViewD& src, const OutViewD& dst, const DitherParams& p, int slot0,
                                        int lane)
{
    const long long live_rows = p.n_sc - (long long)blockIdx.x * kDitherRows;
#pragma unroll
    for (int m = 0; m < PER; m++) {
        int row, col;
        dither_element((slot0 + m) * 64 + lane, p.ch, src.cs == 1, row, col);
        L.in_at[m] = row * kDitherStride + col;
        L.col_in[m] = row < live_rows ? col : kDitherT;
        L.ctr[m] = R.key[row] + kDitherGamma * (unsigned long long)(p.first + col);
        L.src[m] = R.src[row] + (p.first + col) * src.fs;
        dither_element((slot0 + m) * 64 + lane, p.ch, dst.cs == 1, row, col);
        L.q_at[m] = row * kDitherStride + col;
        L.col_q[m] = row < live_rows ? col : kDitherT;
        L.dst[m] = R.dst[row] + (p.first + col) * dst.fs;
    }
}
// the samples of the next tile, `left` frames of which lie inside the launch (zero outside them and the live rows)
template <int PER>
__device__ inline void dither_tile_load(DitherLane<PER>& L, const SigViewD& src, int left, float (&x)[PER])
{
#pragma unroll
    for (int m = 0; m < PER; m++) {
        x[m] = L.col_in[m] < left ? src.base[L.src[m]] : 0.0f;
        L.src[m] += kDitherT * src.fs;
    }
}
// {t, d} of the next tile into the input stage; start: the tile begins at sample 0 of the stream (the highpass dither's r1[-1] = 0)
template <int PER>
__device__ inline void dither_tile_make(DitherLane<PER>& L, const DitherParams& p, bool start, const float (&x)[PER], double2* in)
{
#pragma unroll
    for (int m = 0; m < PER; m++) {
        double d = 0.0;
        if (p.kind != NAE_DITHER_NONE) {
            const unsigned long long h = dither_fin(L.ctr[m]);
            d = dither_half((unsigned int)(h >> 32));
            if (p.kind == NAE_DITHER_TRIANGULAR) d += dither_half((unsigned int)h);
            if (p.kind == NAE_DITHER_HIGHPASS && !(start && L.col_in[m] == 0)) d -= dither_half((unsigned int)(dither_fin(L.ctr[m] - kDitherGamma) >> 32));
        }
        in[L.in_at[m]] = double2{dither_scaled(x[m], p.scale), d};
        L.ctr[m] += kDitherGamma * kDitherT;
    }
}
// the next tile from the output stage into the destination
template <int PER>
__device__ inline void dither_tile_store(DitherLane<PER>& L, const OutViewD& dst, const DitherParams& p, int left, const double* qs)
{
#pragma unroll
    for (int m = 0; m < PER; m++) {
        if (L.col_q[m] < left) dst.base[L.dst[m]] = dither_out(qs[L.q_at[m]], p.scale, p.inv_scale);
        L.dst[m] += kDitherT * dst.fs;
    }
}

// the recurrence over `count` samples of a tile (a whole tile: count = kDitherT, unrolled; the last one: a uniform bound)
template <int K>
__device__ inline void dither_walk(const double2* in, double* qs, const DitherParams& p, int lane, int count, double (&e)[K])
{
    const double2* row = in + lane * kDitherStride;
    double* out = qs + lane * kDitherStride;
#pragma unroll
    for (int j = 0; j < kDitherT; j++) {
        if (j < count) {
            const double2 td = row[j];
            double u = td.x;
#pragma unroll
            for (int k = K - 1; k >= 0; k--) u = __builtin_fma(p.nc[k], e[k], u);     // e[k] is e[n - 1 - k]: the oldest first
            const double q = __builtin_rint(u + td.y);
#pragma unroll
            for (int k = K - 1; k > 0; k--) e[k] = e[k - 1];
            e[0] = q - u;
            out[j] = q;
        }
    }
}

// The barrier between two intervals orders LDS only: every wave waits for its own LDS accesses and arrives.  __syncthreads() would also wait
// for the global loads of the tile after next, which are there to stay in flight across the walk, and for the stores of the tile before
__device__ __forceinline__ void dither_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A producer wave's whole life: tile 0 made and tile 1 loaded in front of the first barrier; then, in the interval in which the walking wave
// walks tile `it`, tile it + 1 made from the samples loaded an interval ago, tile it + 2 loaded, tile it - 1 stored; the last tile stored
// behind the last barrier.  As many barriers as the walking wave's: one and one per tile.
template <int PER>
__device__ inline void dither_produce(const SigViewD& src, const OutViewD& dst, const DitherParams& p, const DitherRows& R, long long tiles, int slot0,
                                      int lane, double2 (*in)[kDitherRows * kDitherStride], double (*qs)[kDitherRows * kDitherStride])
{
    const auto left = [&](long long it) { const long long n = p.stop - p.first - it * kDitherT; return n >= kDitherT ? kDitherT : (int)n; };
    DitherLane<PER> L;
    float x[PER];
    dither_lane_init(L, R, src, dst, p, slot0, lane);
    dither_tile_load(L, src, left(0), x);
    dither_tile_make(L, p, p.first == 0, x, in[0]);
    if (tiles > 1) dither_tile_load(L, src, left(1), x);
    dither_barrier();
    for (long long it = 0; it < tiles; it++) {
        if (it + 1 < tiles) dither_tile_make(L, p, false, x, in[(it + 1) & 1]);
        if (it + 2 < tiles) dither_tile_load(L, src, left(it + 2), x);
        if (it >= 1) dither_tile_store(L, dst, p, kDitherT, qs[(it - 1) & 1]);
        dither_barrier();
    }
    dither_tile_store(L, dst, p, left(tiles - 1), qs[(tiles - 1) & 1]);
}

// d_state: K doubles per stream-channel, e[n - 1] first, in front of frame `first` on entry and in front of `stop` on exit; null: zero, and
// nothing kept
template <int K, bool ROLES>
__global__ __launch_bounds__(ROLES ? 64 + kDitherProducers : 64) void dither_ef_kernel(SigViewD src, OutViewD dst, DitherParams p, double* d_state)
{
    __shared__ double2 in[2][kDitherRows * kDitherStride];
    __shared__ double qs[2][kDitherRows * kDitherStride];
    __shared__ DitherRows R;
    const long long tiles = (p.stop - p.first + kDitherT - 1) / kDitherT;
    const int tid = threadIdx.x;
    const bool walker = tid < 64;
    const long long g = (long long)blockIdx.x * kDitherRows + tid;
    double e[K];
#pragma unroll
    for (int k = 0; k < K; k++) e[k] = (walker && d_state && g < p.n_sc) ? d_state[g * NAE_DITHER_MAX_TAPS + k] : 0.0;
    if (walker) {
        const long long s = g < p.n_sc ? g / p.ch : 0, c = g < p.n_sc ? g % p.ch : 0;
        R.key[tid] = dither_key(p.seed, (unsigned long long)s, (unsigned long long)c);
        R.src[tid] = s * src.ss + c * src.cs;
        R.dst[tid] = s * dst.ss + c * dst.cs;
    }
    __syncthreads();

    // frames of tile `it` inside the launch, at most a tile
    const auto left = [&](long long it) { const long long n = p.stop - p.first - it * kDitherT; return n >= kDitherT ? kDitherT : (int)n; };
    if constexpr (ROLES) {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        if (wave == 0) {
            __builtin_amdgcn_s_setprio(3);
            dither_barrier();
            for (long long it = 0; it < tiles; it++) {
                if (left(it) == kDitherT) dither_walk<K>(in[it & 1], qs[it & 1], p, tid, kDitherT, e);     // unrolled, no bound in it
                else dither_walk<K>(in[it & 1], qs[it & 1], p, tid, left(it), e);
                dither_barrier();
            }
        } else if (wave == kDitherLightWave) {
            dither_produce<1>(src, dst, p, R, tiles, (kDitherLightWave - 1) * kDitherHeavy, tid & 63, in, qs);
        } else {
            dither_produce<kDitherHeavy>(src, dst, p, R, tiles, (wave - 1) * kDitherHeavy, tid & 63, in, qs);
        }
    } else {
        constexpr int PER = kDitherT;
        DitherLane<PER> L;
        float x[PER];
        dither_lane_init(L, R, src, dst, p, 0, tid);
        for (long long it = 0; it < tiles; it++) {
            dither_tile_load(L, src, left(it), x);
            dither_tile_make(L, p, p.first + it * kDitherT == 0, x, in[0]);
            __syncthreads();
            if (left(it) == kDitherT) dither_walk<K>(in[0], qs[0], p, tid, kDitherT, e);
            else dither_walk<K>(in[0], qs[0], p, tid, left(it), e);
            __syncthreads();
            dither_tile_store(L, dst, p, left(it), qs[0]);
            __syncthreads();
        }
    }
    if (walker && d_state && g < p.n_sc) {
#pragma unroll
        for (int k = 0; k < K; k++) d_state[g * NAE_DITHER_MAX_TAPS + k] = e[k];
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_dither_block_f32 and nae_dither_create (ctx may be null: no message then)
int nae_dither_check(nae_ctx* ctx, const nae_dither_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: null pointer");
    if (ch != 1 && ch != 2) return nae_fail_opt(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (p->bits < NAE_DITHER_MIN_BITS || p->bits > NAE_DITHER_MAX_BITS) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: bits outside 8 ... 24");
    if (p->kind < NAE_DITHER_NONE || p->kind > NAE_DITHER_HIGHPASS) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: unknown kind");
    if (p->n_taps < 0 || p->n_taps > NAE_DITHER_MAX_TAPS) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: n_taps outside 0 ... 12");
    double sum = 0.0;
    for (int k = 0; k < p->n_taps; k++) {
        if (!isfinite(p->taps[k])) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: non-finite tap");
        sum += fabs(p->taps[k]);
    }
    if (!(sum <= NAE_DITHER_MAX_TAP_SUM)) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dither: the taps' absolute sum exceeds 64");
    return NAE_OK;
}

// frames [first, stop) of n_streams x ch absolutely indexed signals; d_state as dither_ef_kernel's (unused without taps)
int nae_launch_dither(nae_ctx* ctx, const nae_dither_params* dp, const nae_sig* src, int ch, size_t n_streams, const nae_sig* dst, size_t first,
                      size_t stop, double* d_state)
{
    if (stop <= first || n_streams == 0) return NAE_OK;
    DitherParams p;
    memset(&p, 0, sizeof(p));
    p.first = (long long)first;
    p.stop = (long long)stop;
    p.n_sc = (long long)(n_streams * (size_t)ch);
    p.seed = dp->seed;
    p.scale = ldexp(1.0, dp->bits - 1);
    p.inv_scale = ldexp(1.0, 1 - dp->bits);
    for (int k = 0; k < dp->n_taps; k++) p.nc[k] = -dp->taps[k];
    p.ch = ch;
    p.kind = dp->kind;
    const SigViewD sv = to_view(src);
    const OutViewD ov = to_out(dst);
    if (dp->n_taps == 0) {
        // interleaved on both sides: a row per stream; else a row per stream-channel.  16-byte pieces where every row of both views starts
        // on one and neighbouring elements are neighbours in memory
        const bool ilv = sv.cs == 1 && sv.fs == ch && ov.cs == 1 && ov.fs == ch;
        const auto dense = [&](const void* base, long long ss, long long cs, long long fs) {
            return ((uintptr_t)base & 15) == 0 && (ss & 3) == 0 && (ilv || (fs == 1 && (cs & 3) == 0));
        };
        const bool vec = dense(sv.base, sv.ss, sv.cs, sv.fs) && dense(ov.base, ov.ss, ov.cs, ov.fs);
        const long long per = ilv ? ch : 1, rows = ilv ? (long long)n_streams : p.n_sc;
        const long long span = p.stop * per - ((p.first * per) & ~3ll);
        const long long tiles_per_row = (span + 1023) / 1024;
        if (rows > 0x7fffffffll / tiles_per_row) return nae_fail(ctx, NAE_ERR_INVALID, "dither_flat_kernel: grid too large");
        return nae_launch_tiles(ctx, "dither_flat_kernel", "dither_flat_kernel: grid too large", dither_flat_kernel, rows * tiles_per_row, 1, 256, 0, sv,
                                ov, p, tiles_per_row, (int)ilv, (int)vec);
    }
    const bool roles = ctx->dither_roles != 2;
    return pick_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(ctx, dp->n_taps, "dither: n_taps outside 0 ... 12", [&](auto k) {
        return with_flags(roles, [&](auto r) {
            return nae_launch_tiles(ctx, "dither_ef_kernel", "dither_ef_kernel: grid too large", dither_ef_kernel<k.value, r.value>, p.n_sc, kDitherRows,
                                    r.value ? 64 + kDitherProducers : 64, 0, sv, ov, p, d_state);
        });
    });
}

extern "C" {

int nae_dither_block_f32(nae_ctx* ctx, const nae_dither_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                         const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "dither: null pointer");
    const int rc = nae_dither_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "dither: null pointer");
    return nae_launch_dither(ctx, params, src, ch, n_streams, dst, 0, in_len, nullptr);
}

// DESIGN.md §3, "K23 dither", "Presets"
int nae_dither_design(int bits, int kind, int shaping, unsigned long long seed, nae_dither_params* out)
{
    static const double first[] = {1.0}, second[] = {2.0, -1.0}, lipshitz[] = {2.033, -2.165, 1.959, -1.590, 0.6149};
    static const struct { const double* taps; int n; } presets[] = {{nullptr, 0}, {first, 1}, {second, 2}, {lipshitz, 5}};
    if (!out || bits < NAE_DITHER_MIN_BITS || bits > NAE_DITHER_MAX_BITS || kind < NAE_DITHER_NONE || kind > NAE_DITHER_HIGHPASS ||
        shaping < NAE_DITHER_SHAPE_NONE || shaping > NAE_DITHER_SHAPE_LIPSHITZ)
        return NAE_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->bits = bits;
    out->kind = kind;
    out->n_taps = presets[shaping].n;
    for (int k = 0; k < out->n_taps; k++) out->taps[k] = presets[shaping].taps[k];
    out->seed = seed;
    return NAE_OK;
}

} // extern "C"
