// kernels_hpss.hip — K21, the harmonic/percussive separation ("K21 separation") at frame sizes N = 512, 1024, 2048, 4096 for gfx950.
//
// The spectral gate's STFT pass (kernels_denoise.hip) with another gain: analysis, a gain per bin, c2r, window, overlap-add, from the same helpers
// (pv_any.h).  The gain comes from two medians of 16-bit keys q_f[k], the upper half of the f32 power p_f[k]: Hq over 2 Tn + 1 frames at one
// bin, Pq over 2 Fn + 1 bins of one frame, and a mask between the two.  hpss_kernel is one wave per (stream-channel, tile of hop blocks) and
// starts cold: for the tile [b0, b_end) it takes the keys of frames b0 - Tn ... b_end + 2 + Tn and synthesises frames b0 ... b_end + 2, so the key
// front runs Tn frames ahead of the synthesis and a frame is analysed twice (Tn = 0: once) — three FFTs per frame.
// The keys of the last 2 Tn + 1 frames stand in an LDS ring of rows of 16-bit words.  A row holds bins -8 ... M + 8 with the mirror already
// applied (bin k at half word 8 + k), so neither median computes an index per element.  In both medians lane l takes the bin pairs
// 2 (l + 64 r) + {0, 1}: one aligned dword per row for the time median, nine consecutive dwords of the centre row for the frequency median (an odd
// offset is one v_alignbit of two of them) — consecutive lanes read consecutive dwords, no bank is asked twice.  Two bins ride in one register
// through a selection of fixed length 17 (hp_median17) on v_pk_min_u16 / v_pk_max_u16; a narrower span pads with as many 0x0000 as 0xFFFF, which
// leaves the median where it was (over time the padding stands in the ring's unused rows, written once).  Every key and every median is an integer: any selection method gives the same bits, and so do every tiling
// and the streaming handle.  A wave's FFT scratch, the frame's spectrum Y and the ring live in LDS (Hp<N>), the three open overlap-add blocks in
// registers.
// Built with -ffp-contract=off: every f32 step is one IEEE operation in the order of the CPU statement (tests/hpss_ref/ref_hpss.c).
#include "pv_any.h"
#include <math.h>

namespace nae {

constexpr int kHpRing = 2 * NAE_HPSS_MAX_SPAN + 1;        // frames of keys a wave keeps
constexpr int kHpEdge = NAE_HPSS_MAX_SPAN;                // mirrored bins in front of bin 0 and behind bin M

// A wave's LDS: the FFT scratch and Y as PvEnv<N>, and the ring of keys, sized for Tn = 8 at every size: 9.3 / 17.8 / 34.8 / 68.8 KB
template <int N>
struct Hp {
    using A = PvAny<N>;
    static constexpr int M = A::M, NB = A::NB;
    static constexpr int NP = M / 128 + 1;                // bin pairs per lane: k0 = 2 (lane + 64 r)
    // half words per row: bins -8 ... M + 8 and the one behind them that the pair of bin M reads (and drops), a whole number of 16-byte slots
    static constexpr int ROW = (M + 2 * kHpEdge + 2 + 7) & ~7;
    static constexpr size_t kWave = A::Gm::SCR * sizeof(cf) + A::PAD * sizeof(cf) + (size_t)kHpRing * ROW * sizeof(uint16_t);
    static constexpr int kMaxWaves = (int)((160 * 1024 - 512 * sizeof(cf)) / kWave);
    static constexpr int kWaves = kMaxWaves < 8 ? kMaxWaves : 8;      // 8, 5, 3, 1 waves per workgroup at N = 512 ... 4096
    // waves a CU holds: whole workgroups by LDS (8, 5, 3, 1), and the registers hold as many (`make resources`, profiles/r33_hpss.md)
    static constexpr int kResident = (int)((160 * 1024) / (512 * sizeof(cf) + kWaves * kWave)) * kWaves;
    static_assert(ROW % 2 == 0 && ROW >= M + 2 * kHpEdge + 2, "a row holds the mirrored bins in whole dwords");
    static_assert(kWaves >= 1, "one wave's state fits a CU's LDS");
};

struct HpGain {
    float gain_p, d;       // G = gain_p + d m, d = (float)((double)gain_h - (double)gain_p)
    int tn, fn;
};

typedef unsigned short hp_u16x2 __attribute__((ext_vector_type(2)));

// two compare-exchanges at once, one per half word: a = min, b = max
__device__ __forceinline__ void hp_cx(uint32_t& a, uint32_t& b)
{
    const hp_u16x2 x = __builtin_bit_cast(hp_u16x2, a), y = __builtin_bit_cast(hp_u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
}

// the smallest of w[0 .. m) to w[0] and the largest to w[m - 1]: pairs across the middle first, so the smallest is in the lower half and the
// largest in the upper; floor(m / 2) + 2 ceil(m / 2) - 2 exchanges
template <int m>
__device__ __forceinline__ void hp_ends(uint32_t (&w)[10])
{
#pragma unroll
    for (int i = 0; i < m / 2; i++) hp_cx(w[i], w[m - 1 - i]);
#pragma unroll
    for (int i = 1; i < (m + 1) / 2; i++) hp_cx(w[0], w[i]);
#pragma unroll
    for (int i = m / 2; i < m - 1; i++) hp_cx(w[i], w[m - 1]);
}

// the element of rank 8 of 17, per half word.  Among any 10 of the 17 the smallest has 9 above it and the largest 9 below: neither is the
// median (or it has an equal that stays), so both go and the next input comes in; 10, 9, ... 4 elements, then the median of the last three —
// 61 exchanges and 4 single operations
__device__ __forceinline__ uint32_t hp_median17(const uint32_t (&a)[kHpRing])
{
    uint32_t w[10];
#pragma unroll
    for (int i = 0; i < 10; i++) w[i] = a[i];
    hp_ends<10>(w); w[0] = a[10];
    hp_ends<9>(w);  w[0] = a[11];
    hp_ends<8>(w);  w[0] = a[12];
    hp_ends<7>(w);  w[0] = a[13];
    hp_ends<6>(w);  w[0] = a[14];
    hp_ends<5>(w);  w[0] = a[15];
    hp_ends<4>(w);  w[0] = a[16];
    hp_cx(w[0], w[1]);
    const hp_u16x2 lo = __builtin_bit_cast(hp_u16x2, w[0]), hi = __builtin_bit_cast(hp_u16x2, w[1]), c = __builtin_bit_cast(hp_u16x2, w[2]);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(lo, __builtin_elementwise_min(hi, c)));
}

// q = (uint16)(bits(p) >> 16) of p = X.x X.x + X.y X.y: two products and one add
__device__ __forceinline__ uint16_t hp_key(cf x) { return (uint16_t)(__float_as_uint(x.x * x.x + x.y * x.y) >> 16); }

// bin k's key into a row, and into the places that mirror it: bin -k for k = 1 ... 8, bin 2 M - k for k = M - 8 ... M - 1
template <int N>
__device__ __forceinline__ void hp_put_key(uint16_t* row, int k, uint16_t q)
{
    constexpr int M = Hp<N>::M;
    row[kHpEdge + k] = q;
    if (k >= 1 && k <= kHpEdge) row[kHpEdge - k] = q;
    if (k >= M - kHpEdge && k < M) row[kHpEdge + 2 * M - k] = q;
}

// the keys of frame g into `row`: a frame outside [0, frames) is silence, all zero and not analysed
template <int N, bool kUnit>
__device__ __forceinline__ void hp_keys(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in, const PvParams& p, uint16_t* row, long long g,
                                        int lane)
{
    using H = Hp<N>;
    using Gm = typename H::A::Gm;
    if (g < 0 || g >= p.frames) {                          // wave-uniform
        uint32_t* r32 = reinterpret_cast<uint32_t*>(row);
        for (int i = lane; i < H::ROW / 2; i += 64) r32[i] = 0;
        wave_lds_sync();
        return;
    }
    pva_analyse<N, kUnit>(scr, w512l, tb, in, pva_frame_start<N>(p, g), lane);
#pragma unroll 2
    for (int r = 0; r < H::NB; r++) {
        const int k = lane + 64 * r;
        if (k <= H::M) hp_put_key<N>(row, k, hp_key(any_rfft_bin<Gm>(scr, tb.tn, k)));
    }
    wave_lds_sync();                                       // the next analysis rewrites the scratch; the ring is read by every lane
}

// the mask between the medians Hq and Pq of one bin
template <bool kHard>
__device__ __forceinline__ float hp_mask(uint32_t hq, uint32_t pq)
{
    if (kHard) return hq >= pq ? 1.0f : 0.0f;
    const double h = (double)__uint_as_float(hq << 16), s = h + (double)__uint_as_float(pq << 16);
    return s == 0.0 ? 0.5f : (float)(h / s);
}

template <int N, bool kUnit, bool kHard>
__global__ __launch_bounds__(64 * (Hp<N>::kWaves)) void hpss_kernel(SigViewD src, PvParams p, long long n_items, OutViewD out, SpecAnyTables tb, HpGain gn)
{
    using P = PvAny<N>;
    using H = Hp<N>;
    using Gm = typename P::Gm;
    constexpr int M = P::M;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[H::kWaves * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[H::kWaves * P::PAD];
    __shared__ __attribute__((aligned(16))) uint16_t ringbuf[H::kWaves * kHpRing * H::ROW];
    for (int i = threadIdx.x; i < 512; i += 64 * H::kWaves) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * H::kWaves + wave_id();
    if (item >= n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * P::PAD;
    uint16_t* ring = ringbuf + wave_id() * (kHpRing * H::ROW);
    const uint32_t* ring32 = reinterpret_cast<const uint32_t*>(ring);
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    const ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const long long b0 = p.f_origin + (long long)tile * p.tile;
    const long long b_end = b0 + p.tile < p.f_stop ? b0 + p.tile : p.f_stop;
    long long f_end = b_end + 3;                           // frames b0 .. b_end+2 feed blocks b0 .. b_end-1
    if (f_end > p.frames) f_end = p.frames;
    float* optr = out.base + s_idx * out.ss + c * out.cs;
    const int tn = gn.tn, fn = gn.fn, nring = 2 * tn + 1;

    // the rows behind the 2 Tn + 1 slots are the selection's padding, as many of 0x0000 as of 0xFFFF: the median of all 17 rows is the slots'
#pragma unroll 1
    for (int t = nring; t < kHpRing; t++) {
        uint32_t* r32 = reinterpret_cast<uint32_t*>(ring + t * H::ROW);
        const uint32_t fill = t < tn + kHpEdge + 1 ? 0u : 0xFFFFFFFFu;
        for (int i = lane; i < H::ROW / 2; i += 64) r32[i] = fill;
    }
    // the key front: frames b0 - Tn ... b0 + Tn - 1 before the first synthesis; frame g sits in slot (g - (b0 - Tn)) mod (2 Tn + 1)
    int head = 0;                                          // the slot of frame f - Tn, the oldest one frame f reads
#pragma unroll 1
    for (int j = 0; j < 2 * tn; j++) hp_keys<N, kUnit>(scr, w512l, tb, in, p, ring + j * H::ROW, b0 - tn + j, lane);

    float r0[P::K], r1[P::K], r2[P::K];
#pragma unroll
    for (int i = 0; i < P::K; i++) r0[i] = r1[i] = r2[i] = 0.0f;
#pragma unroll 1
    for (long long f = b0; f < f_end; f++) {
        const int newest = head == 0 ? nring - 1 : head - 1;   // the slot of frame f + Tn: the one frame f - Tn - 1 had
        int centre = head + tn;                                 // the slot of frame f
        centre = centre >= nring ? centre - nring : centre;
        if (tn > 0) hp_keys<N, kUnit>(scr, w512l, tb, in, p, ring + newest * H::ROW, f + tn, lane);
        pva_analyse<N, kUnit>(scr, w512l, tb, in, pva_frame_start<N>(p, f), lane);
        // Y = X; with Tn = 0 the frame's own keys come from this analysis: no second one
#pragma unroll 2
        for (int r = 0; r < H::NB; r++) {
            const int k = lane + 64 * r;
            if (k <= M) {
                const cf x = any_rfft_bin<Gm>(scr, tb.tn, k);
                lds_st(ys + k, x);
                if (tn == 0) hp_put_key<N>(ring, k, hp_key(x));
            }
        }
        wave_lds_sync();
        // the two medians, the mask and the gain of this lane's bin pairs
#pragma unroll 1
        for (int r = 0; r < H::NP; r++) {
            const int j = lane + 64 * r, k0 = 2 * j;
            if (k0 <= M) {
                uint32_t v[kHpRing];
                // Hq: all 17 rows in the order they stand in (a median asks for no order): the 2 Tn + 1 slots, then the padding
#pragma unroll
                for (int t = 0; t < kHpRing; t++) v[t] = ring32[t * (H::ROW / 2) + kHpEdge / 2 + j];
                const uint32_t hq = hp_median17(v);
                // Pq: half words 2 j ... 2 j + 17 of the centre row are bins k0 - 8 ... k0 + 9; offset i of the pair is half words e, e + 1, e = i + 8
                uint32_t d[kHpEdge + 1];
#pragma unroll
                for (int t = 0; t <= kHpEdge; t++) d[t] = ring32[centre * (H::ROW / 2) + j + t];
#pragma unroll
                for (int e = 0; e < kHpRing; e++) {
                    const uint32_t pair = (e & 1) ? __builtin_amdgcn_alignbit(d[(e + 1) / 2], d[(e - 1) / 2], 16) : d[e / 2];
                    v[e] = e < kHpEdge - fn ? 0u : (e > kHpEdge + fn ? 0xFFFFFFFFu : pair);
                }
                const uint32_t pq = hp_median17(v);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int k = k0 + h;
                    if (k <= M) {
                        const float m = hp_mask<kHard>((hq >> (16 * h)) & 0xFFFFu, (pq >> (16 * h)) & 0xFFFFu);
                        const float G = gn.gain_p + gn.d * m;
                        const cf y = ys[k];
                        ys[k] = cf{G * y.x, G * y.y};
                    }
                }
            }
        }
        wave_lds_sync();
        float o[P::K];
        pva_synth_frame<N>(scr, w512l, tb, ys, r0, r1, r2, o, lane);
        pva_store_block<N>(p, b0, b_end, optr, out.fs, f - 3, o, lane);
        head = head + 1 == nring ? 0 : head + 1;
    }
    pva_drain<N>(p, b0, b_end, f_end, optr, out.fs, r0, r1, r2, lane);
}

template <int N>
static int launch_hpss(nae_ctx* ctx, const SigViewD& src, const OutViewD& out, const PvParams& p, long long n_sc, const HpGain& gn, bool hard,
                       const SpecAnyTables& tb)
{
    using H = Hp<N>;
    const long long items = n_sc * p.n_tiles;
    if (items == 0) return NAE_OK;
    return with_flags(src.fs == 1 && out.fs == 1, hard, [&](auto unit, auto khard) {
        return nae_launch_tiles(ctx, "hpss_kernel", "hpss_kernel: grid too large", hpss_kernel<N, unit.value, khard.value>, items, H::kWaves, 64 * H::kWaves,
                                0, src, p, items, out, tb, gn);
    });
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// Hop blocks per tile of a launch over `blocks` blocks of n_sc stream-channels: the one tile rule (nae_pick_tile) for the waves a CU holds
// (Hp<N>::kResident), never shorter than NAE_HPSS_MIN_TILE blocks (a tile pays 2 Tn key analyses and three whole frames beyond its own — at
// Tn = 8 sixteen single FFTs and three frames against one frame per block: about a tenth of its work at 64 blocks), the number of tiles
// rounded down.  hpss_tile forces the tile.
int nae_pick_hpss_tile(nae_ctx* ctx, int n_fft, size_t blocks, size_t n_sc)
{
    const size_t resident = n_fft == 512 ? Hp<512>::kResident : n_fft == 1024 ? Hp<1024>::kResident : n_fft == 2048 ? Hp<2048>::kResident
                                                                                                                     : Hp<4096>::kResident;
    return nae_pick_tile(ctx, ctx->hpss_tile, blocks, n_sc, resident, NAE_HPSS_MIN_TILE, true);
}

// a gain nae_hpss_design can give: 0 ... (float)10^(NAE_HPSS_MAX_DB / 20)
static bool hpss_gain_ok(float g) { return isfinite(g) && g >= 0.0f && g <= (float)pow(10.0, NAE_HPSS_MAX_DB / 20.0); }

// the one statement of the parameter rules of nae_hpss_block_f32 and nae_hpss_create
int nae_hpss_check(nae_ctx* ctx, const nae_hpss_params* p, int ch)
{
    if (!p) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: null pointer");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (p->time_span < 0 || p->time_span > NAE_HPSS_MAX_SPAN) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: time_span outside 0 ... 8");
    if (p->freq_span < 0 || p->freq_span > NAE_HPSS_MAX_SPAN) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: freq_span outside 0 ... 8");
    if (p->hard != 0 && p->hard != 1) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: hard must be 0 or 1");
    if (!hpss_gain_ok(p->gain_h)) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: gain_h outside 0 ... 10^(12/20) or not finite");
    if (!hpss_gain_ok(p->gain_p)) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: gain_p outside 0 ... 10^(12/20) or not finite");
    if (!nae_size_ok(p->n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "hpss: n_fft must be 512, 1024, 2048 or 4096");
    return NAE_OK;
}

// hop blocks [b_origin, b_stop) of n_streams x ch signals of in_len samples (absolute indexing)
int nae_launch_hpss(nae_ctx* ctx, const nae_hpss_params* hp, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst,
                    size_t b_origin, size_t b_stop)
{
    if (b_stop <= b_origin || n_streams == 0) return NAE_OK;
    const int n_fft = hp->n_fft, H = n_fft / 4;
    SpecAnyTables tb;
    const int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    const size_t blocks = b_stop - b_origin, n_sc = n_streams * (size_t)ch;
    const int tile = nae_pick_hpss_tile(ctx, n_fft, blocks, n_sc);
    const size_t n_tiles = (blocks + (size_t)tile - 1) / (size_t)tile;
    if (n_tiles > 0x7fffffffull) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: too many tiles");
    PvParams p{};
    p.ha_q24 = (long long)H << NAE_HA_FRAC_BITS;           // tempo 1: frame f starts at (f - 3) H
    p.in_len = (long long)in_len;
    p.frames = (long long)((in_len + (size_t)H - 1) / (size_t)H) + 3;
    p.mid_len = (long long)in_len;
    p.ch = ch;
    p.tile = tile;
    p.n_tiles = (int)n_tiles;
    p.f_origin = (long long)b_origin;
    p.f_stop = (long long)b_stop;
    const HpGain gn{hp->gain_p, (float)((double)hp->gain_h - (double)hp->gain_p), hp->time_span, hp->freq_span};
    return at_size(ctx, n_fft, [&](auto n) {
        return launch_hpss<decltype(n)::value>(ctx, to_view(src), to_out(dst), p, (long long)n_sc, gn, hp->hard != 0, tb);
    });
}

extern "C" {

int nae_hpss_design(double harmonic_db, double percussive_db, int n_fft, int time_span, int freq_span, int hard, nae_hpss_params* out)
{
    if (!out || !isfinite(harmonic_db) || !isfinite(percussive_db)) return NAE_ERR_INVALID;
    if (harmonic_db < NAE_HPSS_MIN_DB || harmonic_db > NAE_HPSS_MAX_DB || percussive_db < NAE_HPSS_MIN_DB || percussive_db > NAE_HPSS_MAX_DB ||
        time_span < 0 || time_span > NAE_HPSS_MAX_SPAN || freq_span < 0 || freq_span > NAE_HPSS_MAX_SPAN || (hard != 0 && hard != 1))
        return NAE_ERR_INVALID;
    if (!nae_size_ok(n_fft)) return NAE_ERR_UNSUPPORTED;
    out->n_fft = n_fft;
    out->time_span = time_span;
    out->freq_span = freq_span;
    out->hard = hard;
    out->gain_h = harmonic_db <= NAE_HPSS_MIN_DB ? 0.0f : (float)pow(10.0, harmonic_db / 20.0);
    out->gain_p = percussive_db <= NAE_HPSS_MIN_DB ? 0.0f : (float)pow(10.0, percussive_db / 20.0);
    return NAE_OK;
}

int nae_hpss_block_f32(nae_ctx* ctx, const nae_hpss_params* params, const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: null pointer");
    const int rc = nae_hpss_check(ctx, params, ch);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "hpss: null pointer");
    const size_t H = (size_t)params->n_fft / 4;
    return nae_launch_hpss(ctx, params, src, in_len, ch, n_streams, dst, 0, (in_len + H - 1) / H);
}

} // extern "C"
