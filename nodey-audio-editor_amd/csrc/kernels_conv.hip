// kernels_conv.hip — K10, the long convolution by uniformly partitioned overlap-save ("K10 long convolution") at frame sizes
// N = 512, 1024, 2048, 4096 for gfx950: up to NAE_CONV_MAX_TAPS taps in P = ceil(L / B) partitions of B = N / 2 taps, one set for every channel or
// one per channel.
//
// Three kernels on the block code of the FIR filter (fir_block.h).  conv_taps_kernel: H_{c,p} = r2c_N(partition p of channel c's taps), one wave
// each.  conv_spectra_kernel: the first half of fir_block_kernel — tile head, carried half block, r2c — storing U_b, bins 0 ... M, into a ring of R
// spectrum slots per stream-channel (block j in slot j mod R).  conv_mac_kernel: Y_b = sum_p U_{b-p} H_{c,p} in increasing p, then the c2r and the
// store of fir_block_kernel's second half.  A launch is cut into slabs of at most R - (P - 1) blocks: spectra of the slab, then its sums, which
// reach back over the P - 1 spectra in front of it that the ring still holds.
//
// The sums are the hot path: unreused, a complex multiply-accumulate loads 16 bytes for 8 flops.  A wave therefore owns kT consecutive output
// blocks and a lane its bins k = lane + 64 r, walked in chunks of kC: the kT x kC accumulators stay in registers, a loaded U_j[k] feeds up to kT
// sums (block b0 + t takes it with p = b0 + t - j) and the kT spectra H_p a step needs are a window that moves by one H per step.  Walking j
// downwards gives every accumulator its terms in increasing p.  Y of the kT blocks is collected in LDS, as fir_block_kernel collects one.
#include "fir_block.h"
#include <string.h>
#include <math.h>
#include <new>
#include <vector>

namespace nae {

template <int N>
struct Conv {
    using F = Fir<N>;
    using Gm = typename F::Gm;
    static constexpr int M = F::M, B = F::B, PAD = F::PAD;
    static constexpr int kT = N == 4096 ? 2 : 4;          // output blocks whose accumulators a wave holds (their Y must fit LDS: 4 x 16 KiB at 4096 would leave one wave per CU)
    static constexpr int kC = 4;                          // bins per lane and chunk; F::NB - 1 = 4, 8, 16, 32 of them, then bin M on lane 0
    static_assert((F::NB - 1) % kC == 0, "whole chunks");
    // spectra: scratch and the carried half block per wave — 8, 8, 8, 5 waves per workgroup (six at 4096 would take the 160 KiB to the last byte)
    static constexpr size_t kWaveS = (Gm::SCR + M / 2) * sizeof(cf);
    static constexpr int kMaxWavesS = (int)((159 * 1024 - 512 * sizeof(cf)) / kWaveS);
    static constexpr int kWavesS = kMaxWavesS < 8 ? kMaxWavesS : 8;
    // sums: scratch and Y of kT blocks per wave — 7, 7, 3, 3 waves per workgroup (two workgroups of 7 fit a CU at 512)
    static constexpr size_t kWaveM = (Gm::SCR + kT * PAD) * sizeof(cf);
    static constexpr int kMaxWavesM = (int)((160 * 1024 - 512 * sizeof(cf)) / kWaveM);
    static constexpr int kWavesM = kMaxWavesM < 7 ? kMaxWavesM : 7;
    static_assert(kWavesS >= 1 && kWavesM >= 1, "a wave's state fits a CU's LDS");
};

struct ConvParams {
    long long in_len;      // samples of a stream-channel: reads outside [0, in_len) give zero, samples >= in_len are not stored
    long long b_origin;    // blocks [b_origin, b_stop) of this slab
    long long b_stop;
    long long n_items;     // (stream-channel, tile) pairs
    int tile, n_tiles, ch;
    int taps_ch, parts, ring;   // H is [taps_ch][parts][PAD]; the workspace [stream-channel][ring][PAD]
};

template <int N>
__global__ __launch_bounds__(64) void conv_taps_kernel(const float* __restrict__ hpad, cf* __restrict__ hspec, SpecAnyTables tb)
{
    using F = Fir<N>;
    using Gm = typename F::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scr[Gm::SCR];
    for (int i = threadIdx.x; i < 512; i += 64) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // partition blockIdx.x of the [taps_ch][parts B] padded taps: B reals, then zeros up to N
    fir_taps_r2c<N>(scr, w512l, tb, hpad + (size_t)blockIdx.x * F::B, F::B, hspec + (size_t)blockIdx.x * F::PAD, lane);
}

template <int N, bool kUnit>
__global__ __launch_bounds__(64 * (Conv<N>::kWavesS)) void conv_spectra_kernel(SigViewD src, ConvParams p, cf* __restrict__ ws, SpecAnyTables tb)
{
    using V = Conv<N>;
    using F = Fir<N>;
    using Gm = typename F::Gm;
    constexpr int M = F::M, B = F::B;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[V::kWavesS * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf carry[V::kWavesS * (M / 2)];
    for (int i = threadIdx.x; i < 512; i += 64 * V::kWavesS) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * V::kWavesS + wave_id();
    if (item >= p.n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* cw = carry + wave_id() * (M / 2);
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const float* ip = src.base + w.s_idx * src.ss + w.c * src.cs;
    cf* us = ws + w.sc * p.ring * F::PAD;
    const long long b0 = p.b_origin + (long long)w.tile * p.tile;
    const long long b_end = b0 + p.tile < p.b_stop ? b0 + p.tile : p.b_stop;
    int slot = (int)(b0 % p.ring);

    fir_tile_head<N, kUnit>(cw, ip, src.fs, p.in_len, b0, lane);
#pragma unroll 1
    for (long long b = b0; b < b_end; b++) {
        const long long n0 = b * B;
        const bool full = n0 + B <= p.in_len;              // wave-uniform
        fir_block_r2c<N, kUnit>(scr, cw, w512l, tb, ip, src.fs, p.in_len, n0, full, lane);
        cf* u = us + (long long)slot * F::PAD;
        // lane k mod 64 writes bin k: a wave stores contiguous runs of 512 bytes
#pragma unroll 2
        for (int r = 0; r < F::NB; r++) {
            const int k = lane + 64 * r;
            if (k <= M) u[k] = any_rfft_bin<Gm>(scr, tb.tn, k);
        }
        slot = slot + 1 == p.ring ? 0 : slot + 1;
        wave_lds_sync();                                   // the next block rewrites the scratch
    }
}

// acc (+)= u h in K9's form: four products, one subtract, one add, then one plain add per component (-ffp-contract=off: nothing fuses)
__device__ __forceinline__ void conv_term(cf& acc, cf u, cf h, bool first)
{
    const cf t = cf{u.x * h.x - u.y * h.y, u.x * h.y + u.y * h.x};
    acc = first ? t : cf{acc.x + t.x, acc.y + t.y};
}

// Y of blocks bg ... bg + nblk - 1 (nblk <= kT) at the kC bins k0 + 64 i, into ys[t PAD + k].  us: the stream-channel's ring, hc: the channel's H.
// store: this lane's bins exist (the chunk of bin M: lane 0 alone; the others compute a copy of it).
template <int N, int kC>
__device__ __forceinline__ void conv_accumulate(const cf* __restrict__ us, const cf* __restrict__ hc, cf* ys, long long bg, int nblk, int parts,
                                                int ring, int k0, bool store)
{
    using V = Conv<N>;
    constexpr int kT = V::kT, PAD = V::PAD;
    cf acc[kT][kC];
#pragma unroll
    for (int t = 0; t < kT; t++)
#pragma unroll
        for (int i = 0; i < kC; i++) acc[t][i] = cf{0.0f, 0.0f};
    auto load = [&](const cf* s, cf (&v)[kC]) {
#pragma unroll
        for (int i = 0; i < kC; i++) v[i] = s[k0 + 64 * i];
    };
    // U_j, j = bg + nblk - 1 downwards, q = bg - j: block bg + t takes it with p = q + t where 0 <= p < parts, and p = 0 starts its accumulator
    int slot = (int)((bg + nblk) % ring);                  // one past the first U; block j - 1 sits one slot back
    auto checked = [&](int q) {
        slot = slot == 0 ? ring - 1 : slot - 1;
        cf u[kC];
        load(us + (long long)slot * PAD, u);
#pragma unroll
        for (int t = 0; t < kT; t++) {
            const int pp = q + t;
            if (t < nblk && pp >= 0 && pp < parts) {       // wave-uniform
                cf h[kC];
                load(hc + (long long)pp * PAD, h);
#pragma unroll
                for (int i = 0; i < kC; i++) conv_term(acc[t][i], u[i], h[i], pp == 0);
            }
        }
    };
    const int q_max = bg < parts - 1 ? (int)bg : parts - 1;               // j >= 0, and the last block's p < parts
    const int q_body = q_max < parts - kT ? q_max : parts - kT;           // up to here every block of the group has 1 <= p < parts
    // head: the group's own blocks
#pragma unroll 1
    for (int q = 1 - nblk; q <= 0; q++) checked(q);
    // body: the window hw[t] = H_{q + t} moves by one spectrum per step
    int q = 1;
    if (q <= q_body) {
        cf hw[kT][kC];
#pragma unroll
        for (int t = 0; t + 1 < kT; t++) load(hc + (long long)(1 + t) * PAD, hw[t]);
        const cf* hn = hc + (long long)kT * PAD;           // H_{q + kT - 1}
#pragma unroll 4
        for (; q <= q_body; q++) {
            slot = slot == 0 ? ring - 1 : slot - 1;
            cf u[kC];
            load(us + (long long)slot * PAD, u);
            load(hn, hw[kT - 1]);
            hn += PAD;
#pragma unroll
            for (int t = 0; t < kT; t++)
#pragma unroll
                for (int i = 0; i < kC; i++) conv_term(acc[t][i], u[i], hw[t][i], false);
#pragma unroll
            for (int t = 0; t + 1 < kT; t++)
#pragma unroll
                for (int i = 0; i < kC; i++) hw[t][i] = hw[t + 1][i];
        }
    }
    // tail: the blocks whose p has not yet reached parts - 1
#pragma unroll 1
    for (; q <= q_max; q++) checked(q);
    if (store) {
#pragma unroll
        for (int t = 0; t < kT; t++) {
            if (t < nblk) {
#pragma unroll
                for (int i = 0; i < kC; i++) lds_st(ys + t * PAD + k0 + 64 * i, acc[t][i]);
            }
        }
    }
}

template <int N, bool kUnit>
__global__ __launch_bounds__(64 * (Conv<N>::kWavesM)) void conv_mac_kernel(OutViewD out, ConvParams p, const cf* __restrict__ ws,
                                                                          const cf* __restrict__ hspec, SpecAnyTables tb)
{
    using V = Conv<N>;
    using F = Fir<N>;
    using Gm = typename F::Gm;
    constexpr int M = F::M, B = F::B, kT = V::kT;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[V::kWavesM * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[V::kWavesM * kT * F::PAD];
    for (int i = threadIdx.x; i < 512; i += 64 * V::kWavesM) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * V::kWavesM + wave_id();
    if (item >= p.n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * (kT * F::PAD);
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    float* op = out.base + w.s_idx * out.ss + w.c * out.cs;
    const cf* us = ws + w.sc * p.ring * F::PAD;
    const cf* hc = hspec + (long long)(p.taps_ch == 1 ? 0 : w.c) * p.parts * F::PAD;
    const long long b0 = p.b_origin + (long long)w.tile * p.tile;
    const long long b_end = b0 + p.tile < p.b_stop ? b0 + p.tile : p.b_stop;

#pragma unroll 1
    for (long long bg = b0; bg < b_end; bg += kT) {
        const int nblk = b_end - bg < kT ? (int)(b_end - bg) : kT;
#pragma unroll 1
        for (int r0 = 0; r0 < F::NB - 1; r0 += V::kC) conv_accumulate<N, V::kC>(us, hc, ys, bg, nblk, p.parts, p.ring, lane + 64 * r0, true);
        conv_accumulate<N, 1>(us, hc, ys, bg, nblk, p.parts, p.ring, M, lane == 0);
        wave_lds_sync();
#pragma unroll 1
        for (int t = 0; t < nblk; t++) {
            const long long n0 = (bg + t) * B;
            const bool full = n0 + B <= p.in_len;          // wave-uniform
            fir_block_c2r_store<N, kUnit>(scr, ys + t * F::PAD, w512l, tb, op, out.fs, p.in_len, n0, full, lane);
            wave_lds_sync();                               // the next block rewrites the scratch, the next group Y
        }
    }
}

template <int N>
static int launch_conv_taps(nae_ctx* ctx, const float* hpad, cf* hspec, int n, const SpecAnyTables& tb)
{
    return nae_launch_grid(ctx, "conv_taps_kernel", conv_taps_kernel<N>, dim3((unsigned)n), dim3(64), 0, hpad, hspec, tb);
}

template <int N>
static int launch_conv_slab(nae_ctx* ctx, const SigViewD& src, const OutViewD& out, ConvParams p, size_t n_sc, cf* ws, const cf* hspec,
                            const SpecAnyTables& tb)
{
    using V = Conv<N>;
    const bool unit_in = src.fs == 1, unit_out = out.fs == 1;
    const size_t blocks = (size_t)(p.b_stop - p.b_origin);
    // spectra: the FIR filter's tiling (a tile re-reads half a block at its head)
    p.tile = nae_pick_fir_tile(ctx, N, blocks, n_sc);
    size_t n_tiles = (blocks + (size_t)p.tile - 1) / (size_t)p.tile;
    p.n_tiles = (int)n_tiles;
    p.n_items = (long long)(n_sc * n_tiles);
    // (a tile count past int32 cannot be a kernel argument: the launch's own refusal, in front of it)
    static const char kSpectraGrid[] = "conv_spectra_kernel: grid too large", kMacGrid[] = "conv_mac_kernel: grid too large";
    if (n_tiles > 0x7fffffffull) return nae_fail(ctx, NAE_ERR_INVALID, kSpectraGrid);
    const int rc = with_flags(unit_in, [&](auto unit) {
        return nae_launch_tiles(ctx, "conv_spectra_kernel", kSpectraGrid, conv_spectra_kernel<N, unit.value>, p.n_items, V::kWavesS, 64 * V::kWavesS, 0,
                                src, p, ws, tb);
    });
    if (rc) return rc;
    // sums
    p.tile = nae_pick_conv_tile(ctx, N);
    n_tiles = (blocks + (size_t)p.tile - 1) / (size_t)p.tile;
    p.n_tiles = (int)n_tiles;
    p.n_items = (long long)(n_sc * n_tiles);
    if (n_tiles > 0x7fffffffull) return nae_fail(ctx, NAE_ERR_INVALID, kMacGrid);
    return with_flags(unit_out, [&](auto unit) {
        return nae_launch_tiles(ctx, "conv_mac_kernel", kMacGrid, conv_mac_kernel<N, unit.value>, p.n_items, V::kWavesM, 64 * V::kWavesM, 0, out, p, ws,
                                hspec, tb);
    });
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

static size_t conv_pad(int n_fft) { return (size_t)n_fft / 2 + 8; }   // Fir<N>::PAD

int nae_conv_parts(int n_taps, int n_fft) { return (int)(((long long)n_taps + n_fft / 2 - 1) / (n_fft / 2)); }

// [taps_ch][parts B] padded taps, then H [taps_ch][parts][PAD] complex
size_t nae_conv_spec_floats(int n_fft, int parts, int taps_ch)
{
    return (size_t)taps_ch * (size_t)parts * ((size_t)n_fft / 2 + 2 * conv_pad(n_fft));
}

size_t nae_conv_ring_floats(int n_fft, size_t n_sc, size_t ring) { return n_sc * ring * conv_pad(n_fft) * 2; }

// Blocks per wave of the accumulate kernel.  Unlike a tile of the FIR filter, a longer one shares nothing: a wave's groups of Conv<N>::kT blocks
// are independent, so the choice is the register tile itself, which gives a launch the most waves; conv_tile forces another.
int nae_pick_conv_tile(nae_ctx* ctx, int n_fft)
{
    if (ctx->conv_tile > 0) return ctx->conv_tile;
    return n_fft == 4096 ? Conv<4096>::kT : Conv<512>::kT;
}

// the ring of a launch group of n_sc stream-channels that has `blocks` blocks to run behind `behind` spectra already kept: conv_ring if set (at
// least parts), else what the blocks need, at most what NAE_CONV_WS_BYTES holds and at least parts
size_t nae_pick_conv_ring(nae_ctx* ctx, int n_fft, int parts, size_t blocks, size_t n_sc)
{
    size_t ring;
    if (ctx->conv_ring > 0) ring = (size_t)ctx->conv_ring;
    else {
        ring = blocks + (size_t)parts - 1;
        const size_t cap = NAE_CONV_WS_BYTES / (n_sc * conv_pad(n_fft) * sizeof(cf));
        if (ring > cap) ring = cap;
    }
    if (ring < (size_t)parts) ring = (size_t)parts;
    return ring < 0x40000000 ? ring : 0x40000000;
}

// H of the [taps_ch][n_taps] host taps into d_spec (nae_conv_spec_floats floats); waits for the upload
int nae_conv_make_spec(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, float* d_spec)
{
    SpecAnyTables tb;
    int rc = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    (void)nae_use_device(ctx);
    const int parts = nae_conv_parts(n_taps, n_fft);
    const size_t row = (size_t)parts * ((size_t)n_fft / 2);
    hipError_t e = hipMemsetAsync(d_spec, 0, (size_t)taps_ch * row * sizeof(float), ctx->stream);
    for (int c = 0; c < taps_ch && e == hipSuccess; c++)
        e = hipMemcpyAsync(d_spec + (size_t)c * row, taps_host + (size_t)c * (size_t)n_taps, (size_t)n_taps * sizeof(float), hipMemcpyHostToDevice,
                           ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);            // the caller may reuse its taps
    if (e != hipSuccess) return nae_check(ctx, e, "conv: taps upload");
    cf* hspec = reinterpret_cast<cf*>(d_spec + (size_t)taps_ch * row);
    return at_size(ctx, n_fft, [&](auto n) { return launch_conv_taps<decltype(n)::value>(ctx, d_spec, hspec, taps_ch * parts, tb); });
}

// blocks [b_origin, b_stop) of n_streams x ch signals of in_len samples (absolute indexing), in slabs of at most ring - (parts - 1) blocks; the ring
// [n_streams ch][ring][PAD] holds the spectra of the parts - 1 blocks in front of b_origin (where they exist) and keeps those in front of b_stop
int nae_launch_conv(nae_ctx* ctx, int n_fft, int parts, int taps_ch, const float* d_spec, float* d_ring, size_t ring, const nae_sig* src,
                    size_t in_len, int ch, size_t n_streams, const nae_sig* dst, size_t b_origin, size_t b_stop)
{
    if (b_stop <= b_origin || n_streams == 0) return NAE_OK;
    if (ring < (size_t)parts) return nae_fail(ctx, NAE_ERR_INVALID, "conv: the ring is shorter than the response");
    SpecAnyTables tb;
    const int rc0 = nae_spec_any_tables(ctx, n_fft, &tb);
    if (rc0) return rc0;
    ConvParams p{};
    p.in_len = (long long)in_len;
    p.ch = ch;
    p.taps_ch = taps_ch;
    p.parts = parts;
    p.ring = (int)ring;
    const SigViewD sv = to_view(src);
    const OutViewD ov = to_out(dst);
    const cf* hspec = reinterpret_cast<const cf*>(d_spec + (size_t)taps_ch * (size_t)parts * ((size_t)n_fft / 2));
    const size_t slab = ring - ((size_t)parts - 1);
    for (size_t b = b_origin; b < b_stop; b += slab) {
        p.b_origin = (long long)b;
        p.b_stop = (long long)(b + slab < b_stop ? b + slab : b_stop);
        const int rc = at_size(ctx, n_fft, [&](auto n) {
            return launch_conv_slab<decltype(n)::value>(ctx, sv, ov, p, n_streams * (size_t)ch, reinterpret_cast<cf*>(d_ring), hspec, tb);
        });
        if (rc) return rc;
    }
    return NAE_OK;
}

// the one statement of the parameter rules of nae_conv_block_f32 and nae_conv_create; *n_fft 0 becomes the library's pick
int nae_conv_check(nae_ctx* ctx, int n_taps, int taps_ch, int ch, int* n_fft)
{
    if (n_taps < 1) return nae_fail(ctx, NAE_ERR_INVALID, "conv: n_taps must be at least 1");
    if (ch != 1 && ch != 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    if (taps_ch != 1 && taps_ch != ch) return nae_fail(ctx, NAE_ERR_INVALID, "conv: taps_ch must be 1 or the channel count");
    if (n_taps > NAE_CONV_MAX_TAPS) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "conv: at most NAE_CONV_MAX_TAPS taps");
    if (*n_fft == 0) *n_fft = nae_conv_pick_n_fft(n_taps);
    if (!nae_size_ok(*n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "conv: n_fft must be 512, 1024, 2048 or 4096");
    if (nae_conv_parts(n_taps, *n_fft) > NAE_CONV_MAX_PARTS) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "conv: at most NAE_CONV_MAX_PARTS partitions");
    return NAE_OK;
}

extern "C" {

int nae_conv_pick_n_fft(int n_taps)
{
    if (n_taps < 1 || n_taps > NAE_CONV_MAX_TAPS) return 0;
    for (int n = 512; n <= 4096; n *= 2)
        if (nae_conv_parts(n_taps, n) <= NAE_CONV_PICK_PARTS) return n;
    return nae_conv_parts(n_taps, 4096) <= NAE_CONV_MAX_PARTS ? 4096 : 0;
}

int nae_conv_block_f32(nae_ctx* ctx, const float* taps_host, int n_taps, int taps_ch, int n_fft, const nae_sig* src, size_t in_len, int ch,
                       size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!taps_host || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "conv: null pointer");
    int rc = nae_conv_check(ctx, n_taps, taps_ch, ch, &n_fft);
    if (rc) return rc;
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base) return nae_fail(ctx, NAE_ERR_INVALID, "conv: null pointer");
    (void)nae_use_device(ctx);
    const int parts = nae_conv_parts(n_taps, n_fft);
    const size_t all = (size_t)taps_ch * (size_t)n_taps;
    // H is kept with the context: a call with the taps, the channel layout and the size of the last one computes nothing again
    rc = ctx->conv_spec.get(ctx, {n_fft, taps_ch}, taps_host, all * sizeof(float), nae_conv_spec_floats(n_fft, parts, taps_ch) * sizeof(float),
                            "conv spectra", [&] { return nae_conv_make_spec(ctx, taps_host, n_taps, taps_ch, n_fft, ctx->conv_spec.as<float>()); });
    if (rc) return rc;
    const size_t B = (size_t)n_fft / 2, blocks = (in_len + B - 1) / B;
    // streams per launch group: as many as leave the ring room for slabs of NAE_CONV_MIN_SLAB blocks inside the workspace cap (every stream with
    // conv_ring set)
    size_t group = n_streams;
    if (ctx->conv_ring <= 0) {
        const size_t want_ring = blocks < NAE_CONV_MIN_SLAB ? blocks + (size_t)parts - 1 : (size_t)NAE_CONV_MIN_SLAB + (size_t)parts - 1;
        const size_t fit = NAE_CONV_WS_BYTES / (want_ring * (size_t)ch * conv_pad(n_fft) * sizeof(cf));
        group = fit < 1 ? 1 : fit < n_streams ? fit : n_streams;
    }
    const size_t ring = nae_pick_conv_ring(ctx, n_fft, parts, blocks, group * (size_t)ch);
    rc = ctx->ws_conv.reserve(ctx, nae_conv_ring_floats(n_fft, group * (size_t)ch, ring) * sizeof(float), "workspace");
    if (rc) return rc;
    return nae_for_stream_groups(src, dst, n_streams, group, [&](const nae_sig& gs, const nae_sig& gd, size_t n) {
        return nae_launch_conv(ctx, n_fft, parts, taps_ch, ctx->conv_spec.as<float>(), ctx->ws_conv.as<float>(), ring, &gs, in_len, ch, n, &gd, 0, blocks);
    });
}

// DESIGN.md §3, "K10 long convolution", "Reverb design": exponentially decaying noise in double, rounded once
static double conv_noise(uint64_t seed, long long n)
{
    uint64_t z = seed + (uint64_t)(n + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return 2.0 * ((double)(z >> 11) * 0x1p-53) - 1.0;
}

static bool conv_reverb_ok(int sample_rate, double rt60_s, double predelay_s)
{
    return sample_rate > 0 && rt60_s > 0.0 && rt60_s <= 10.0 && predelay_s >= 0.0 && predelay_s <= 1.0;   // a NaN fails a comparison
}

int nae_conv_reverb_taps(int sample_rate, double rt60_s, double predelay_s)
{
    if (!conv_reverb_ok(sample_rate, rt60_s, predelay_s)) return NAE_ERR_INVALID;
    const double n = round(predelay_s * (double)sample_rate) + ceil(rt60_s * (double)sample_rate);
    return (int)n;
}

int nae_conv_design_reverb(int sample_rate, double rt60_s, double predelay_s, double dry, double wet, uint64_t seed, int n_taps, float* taps_host)
{
    if (!taps_host || !conv_reverb_ok(sample_rate, rt60_s, predelay_s) || !isfinite(dry) || !isfinite(wet)) return NAE_ERR_INVALID;
    const long long d = (long long)round(predelay_s * (double)sample_rate);
    if ((long long)n_taps < d + 1) return NAE_ERR_INVALID;
    double* e = new (std::nothrow) double[(size_t)n_taps];
    if (!e) return NAE_ERR_NOMEM;
    const double tau = rt60_s * (double)sample_rate, ln1000 = log(1000.0);
    double sum = 0.0;
    for (long long n = 0; n < n_taps; n++) {
        e[n] = n >= d ? conv_noise(seed, n) * exp(-ln1000 * (double)(n - d) / tau) : 0.0;
        sum += e[n] * e[n];
    }
    const double norm = sqrt(sum);
    for (long long n = 0; n < n_taps; n++) taps_host[n] = (float)(wet * (e[n] / norm) + (n == 0 ? dry : 0.0));
    delete[] e;
    return NAE_OK;
}

} // extern "C"
