// kernels_pv_any.hip — the K7 phase vocoder at frame sizes N = 512, 1024, 2048, 4096 (hop N/4) for gfx950.
//
// The three passes of the 1024-point vocoder (kernels_stft.hip, kernels_pvpipe.hip) restated with N as a template parameter, on the
// size-generic canonical FFT of fft_any.h:
//   pass 1 (pv_any_phase_kernel)  one wave per (stream-channel, tile): analysis of each frame, sum of its integer phase increments;
//   pass 2 (pv_scan_kernel, pv_scan_chunked_kernel)  per (stream-channel, bin) the exclusive prefix over the tiles, in 16 chunks side by side
//                                 from 256 tiles on, with carry-in and carry-out — the one scan of the unlocked vocoder, at 1024 after the
//                                 shipped pass 1 too;
//   pass 3 (pv_any_synth_kernel)  one wave per synthesis tile: from its record it walks its frames forward — re-analysis, Qs update, rotation,
//                                 c2r transform, window, overlap-add in increasing frame order, gain — and stores its hop blocks.
// Every integer is exact, so every tiling gives the same bits, and the integer phases are the CPU statement's (tests/pv_ref/ref_pv.c);
// the samples follow the tolerance path.  A wave owns one frame at a time: its FFT scratch (9/8 M complex), the phases Qa_{f-1} and (pass 1) the
// tile's sum or (pass 3) Qs, [r][lane] for bin lane + 64 r, and in pass 3 the synthesis spectrum (B = N/2 + 1 complex, padded) live in LDS; the
// three open overlap-add blocks of pass 3 in registers.  (Phases in registers, 2 x (M/64 + 1) per lane, with the bin loop unrolled, spill from
// N = 2048 on.)
// kTransient (NAE_STRETCH_TRANSIENTS; DESIGN.md §3, "Transient preservation"): passes 1 and 3 also keep P_{f-1} (ST floats per wave) in LDS,
// count the rising bins of each row with a ballot, and at an onset restart the sum / Qs from Qa; pass 1 flags the record in slot B and pass 2 is
// the segmented scan.  Waves per workgroup: pass 1 8 / 8 / 7 / 3 at N = 512 ... 4096, pass 3 8 / 8 / 5 / 2 (with formants 8 / 8 / 4 / 2).
// kLink (NAE_STRETCH_LINK_CHANNELS with kTransient; DESIGN.md §3, "Channel link"): the wave of channel c also analyses channel c ^ 1 of its stream in
// front of each frame — a second pva_analyse into the same scratch, of which it keeps the power row (ST floats per wave in LDS) — and the onset rule
// reads Pl = 0.5 (P^0 + P^1) in place of P, so both channels' waves take the same decisions; pass 2 is unchanged.  Waves per workgroup: pass 1
// 8 / 8 / 6 / 3, pass 3 8 / 8 / 4 / 2 (with formants 8 / 7 / 4 / 2).
// N = 1024 runs the shipped passes 1 and 3 unless the debug key pv_any (or, pass 3, a lifter; or transients) asks for these: nae_pv_route_of.  The host
// decisions (records needed, base records, synthesis fields, workspace) are kernels_stft.hip's nae_launch_pv_phase / nae_launch_pv_synth.
#include "pv_any.h"

namespace nae {

// canonical phase of bin k: atan2_q32 below N/2, the sign of the real part at N/2
template <int N>
__device__ __forceinline__ uint32_t pva_phase(cf x, int k)
{
    return k < N / 2 ? atan2_q32(x.y, x.x) : ((x.x < 0.0f) ? 0x80000000u : 0u);
}

// exact phase increment of one hop for bin k: ((k H) mod N) 2^SH + round(int32(Qa - Qp - ((k d) mod N) 2^SH) R / 2^24)
template <int N>
__device__ __forceinline__ uint32_t pva_inc(uint32_t qa, uint32_t qp, unsigned k, unsigned d, unsigned R)
{
    using P = PvAny<N>;
    const uint32_t e = ((k * d) & (N - 1)) << P::SH;
    const int32_t dw = (int32_t)(qa - qp - e);
    const uint32_t adv = ((k * (unsigned)P::H) & (N - 1)) << P::SH;
    // R <= 2^30 at every N (it depends on the tempo only): a positive int32
    const long long scaled = ((long long)dw * (long long)(int32_t)R + (1ll << (NAE_R_FRAC_BITS - 1))) >> NAE_R_FRAC_BITS;
    return adv + (uint32_t)scaled;
}

// transient preservation ("Transient preservation"), rules 1-3 for bin k (k < B) of a row: does P = |X|^2 (two products and an
// add, never fused) rise over the previous frame's P in pp?  pp takes P.  The wave's count of rising bins of the row is the popcount of the ballot.
template <int N>
__device__ __forceinline__ int pva_rises(cf x, int k, float* pp, bool counted)
{
    const float P = x.x * x.x + x.y * x.y;
    const bool rise = counted && k < N / 2 + 1 && P > NAE_TRANSIENT_RISE * *pp && P > NAE_TRANSIENT_FLOOR * (float)N;
    *pp = P;
    return __popcll(__ballot(rise));
}

// channel link ("Channel link"): the power row of the stream's other channel for frame start s — its analysis into the wave's scratch,
// P of bin lane + 64 r into po[64 r] (read back by the same lane only) — after which the scratch is free for the wave's own frame
template <int N, bool kUnit>
__device__ __forceinline__ void pva_other_power(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in2, long long s, float* po, int lane)
{
    using P = PvAny<N>;
    using Gm = typename P::Gm;
    pva_analyse<N, kUnit>(scr, w512l, tb, in2, s, lane);
#pragma unroll 2
    for (int r = 0; r < P::NB; r++) {
        const int k = lane + 64 * r;
        const cf x = any_rfft_bin<Gm>(scr, tb.tn, k < P::B ? k : P::M);
        po[64 * r] = x.x * x.x + x.y * x.y;
    }
    wave_lds_sync();
}

// pva_rises on the linked power Pl = 0.5 (P^0 + P^1): own is this channel's P, other the other channel's (one IEEE add — it commutes, so either
// channel's wave gets the bits of P^0 + P^1 — then one product); pp keeps Pl_{f-1}
template <int N>
__device__ __forceinline__ int pva_rises_linked(cf x, int k, float* pp, float other, bool counted)
{
    const float own = x.x * x.x + x.y * x.y;
    const float P = 0.5f * (own + other);
    const bool rise = counted && k < N / 2 + 1 && P > NAE_TRANSIENT_RISE * *pp && P > NAE_TRANSIENT_FLOOR * (float)N;
    *pp = P;
    return __popcll(__ballot(rise));
}

// rule 4: frame f is an onset iff f >= 2, it is high and the frame before is not (high: DEN * count >= NUM * B)
template <int N>
__device__ __forceinline__ bool pva_high(int count)
{
    return NAE_TRANSIENT_DEN * count >= NAE_TRANSIENT_NUM * (N / 2 + 1);
}

// ------------------------------------------------------------------------------------------------ pass 1
// sums[(sc * n_tiles + tile) * PAD + k].  kTransient: an onset frame of the tile restarts the sum at its Qa, and the record's slot B is 1 when the
// tile holds an onset (the summary (r, S) of DESIGN.md §3); frames f0 - 2 and f0 - 1 prime P and "high"
template <int N, bool kUnit, bool kTransient = false, bool kLink = false>
__global__ __launch_bounds__(64 * (PvAny<N, false, kTransient, kLink>::kWaves1)) void pv_any_phase_kernel(SigViewD src, PvParams p, long long n_items,
                                                                             uint32_t* __restrict__ sums, SpecAnyTables tb)
{
    static_assert(kTransient || !kLink, "unlocked, the link acts on the onset rule only");
    using P = PvAny<N, false, kTransient, kLink>;
    using Gm = typename P::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[P::kWaves1 * Gm::SCR];
    __shared__ uint32_t state[P::kWaves1 * 2 * P::ST];
    __shared__ float pprev[kTransient ? P::kWaves1 * P::ST : 1];   // transients: P_{f-1} of bin lane + 64 r
    __shared__ float pother[kLink ? P::kWaves1 * P::ST : 1];       // link: the other channel's P_f
    for (int i = threadIdx.x; i < 512; i += 64 * P::kWaves1) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * P::kWaves1 + wave_id();
    if (item >= n_items) return;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    if (tile >= p.skip_from) return;                    // wave-uniform
    cf* scr = scratch + wave_id() * Gm::SCR;
    uint32_t* qp = state + wave_id() * 2 * P::ST + lane;  // [r * 64]: Qa_{f-1} of bin lane + 64 r
    uint32_t* acc = qp + P::ST;                          //           the tile's sum of increments
    float* pp = pprev + (kTransient ? wave_id() * P::ST + lane : 0);
    float* po = pother + (kLink ? wave_id() * P::ST + lane : 0);
    const ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const ChanView in2{src.base + s_idx * src.ss + (c ^ 1) * src.cs, src.fs, p.in_len};   // link (ch == 2): the stream's other channel
    const long long f0 = p.f_origin + (long long)tile * p.tile;
    long long f1 = f0 + p.tile;
    if (f1 > p.f_stop) f1 = p.f_stop;

    for (int r = 0; r < P::NB; r++) { acc[64 * r] = 0; qp[64 * r] = 0; }
    long long s_prev = 0;
    const long long f_first = kTransient ? (f0 > 2 ? f0 - 2 : 0) : (f0 > 0 ? f0 - 1 : 0);
    bool high_prev = false;                                // transients: high(f - 1), wave-uniform
    uint32_t reset = 0;                                    //             an onset in [f0, f1)
    // frames before f0 only prime qp (their increments belong to the previous tile) and, with transients, P and high
#pragma unroll 1
    for (long long f = f_first; f < f1; f++) {
        const long long s = pva_frame_start<N>(p, f);
        if constexpr (kLink) pva_other_power<N, kUnit>(scr, w512l, tb, in2, s, po, lane);
        pva_analyse<N, kUnit>(scr, w512l, tb, in, s, lane);
        const unsigned d = (unsigned)(s - s_prev);
        const unsigned R = (d == (unsigned)p.d0) ? p.r_q24_0 : p.r_q24_1;
        int rising = 0;
#pragma unroll 2
        for (int r = 0; r < P::NB; r++) {
            const int k = lane + 64 * r;
            const int kc = k < P::B ? k : P::M;            // lanes past bin M (last row) compute bin M and store nothing
            const cf x = any_rfft_bin<Gm>(scr, tb.tn, kc);
            const uint32_t qa = pva_phase<N>(x, kc);
            // frame f0 - 1 only primes; the "increment" of frame 0 is its analysis phase
            if (f >= f0) acc[64 * r] = (f == 0) ? qa : acc[64 * r] + pva_inc<N>(qa, qp[64 * r], (unsigned)kc, d, R);
            qp[64 * r] = qa;
            if constexpr (kLink) rising += pva_rises_linked<N>(x, k, pp + 64 * r, po[64 * r], f > f_first);
            else if constexpr (kTransient) rising += pva_rises<N>(x, k, pp + 64 * r, f > f_first);
        }
        if constexpr (kTransient) {
            const bool high = f > f_first && pva_high<N>(rising);
            if (f >= f0 && f >= 2 && high && !high_prev) {     // an onset: the sum restarts at Qa_f (wave-uniform)
#pragma unroll 1
                for (int r = 0; r < P::NB; r++) acc[64 * r] = qp[64 * r];
                reset = 1;
            }
            high_prev = high;
        }
        wave_lds_sync();                                   // the next frame rewrites the scratch
        s_prev = s;
    }
    uint32_t* o = sums + item * P::PAD;
    for (int r = 0; r < P::NB; r++) {
        const int k = lane + 64 * r;
        if (k < P::B) o[k] = acc[64 * r];
    }
    if (kTransient && lane == 0) o[P::B] = reset;          // slot B of the padding (PAD - B = 7 at every N)
}

// ------------------------------------------------------------------------------------------------ pass 2
// the one scan of the unlocked vocoder (after pv_phase_kernel or pv_any_phase_kernel): exclusive prefix over tiles, in place; one thread per
// (stream-channel, bin).  carry_in (optional): the phase in front of tile 0, [n_sc][PAD]; carry_out (optional): the phase behind the last tile.
// Records at or beyond n_read count as zero.  kSeg (transients): the segmented scan — a record whose slot B is set restarts the running value at
// its own sum, (r1, S1) then (r2, S2) = r2 ? (1, S2) : (r1, S1 + S2); the carried phase does not cross a reset.
template <int N, bool kSeg = false>
__global__ void pv_scan_kernel(uint32_t* __restrict__ sums, long long n_sc, int n_tiles, const uint32_t* __restrict__ carry_in,
                               uint32_t* __restrict__ carry_out, int n_read)
{
    using P = PvAny<N>;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long sc = t / P::PAD;
    const int k = (int)(t % P::PAD);
    if (sc >= n_sc || k >= P::B) return;
    uint32_t* p = sums + sc * n_tiles * (long long)P::PAD + k;
    const uint32_t* fl = sums + sc * n_tiles * (long long)P::PAD + P::B;   // kSeg: the tiles' reset flags (read only)
    uint32_t run = carry_in ? carry_in[sc * P::PAD + k] : 0u;
    int j = 0;
    // the loads do not depend on the running sum: fetch 8 tiles ahead, then prefix them
    for (; j + 8 <= n_read; j += 8) {
        uint32_t v[8], r[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            v[u] = p[(long long)(j + u) * P::PAD];
            if constexpr (kSeg) r[u] = fl[(long long)(j + u) * P::PAD];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            p[(long long)(j + u) * P::PAD] = run;
            if constexpr (kSeg) run = r[u] ? v[u] : run + v[u];
            else run += v[u];
        }
    }
    for (; j < n_tiles; j++) {
        const uint32_t v = (j < n_read) ? p[(long long)j * P::PAD] : 0u;
        p[(long long)j * P::PAD] = run;
        if constexpr (kSeg) run = (j < n_read && fl[(long long)j * P::PAD]) ? v : run + v;
        else run += v;
    }
    if (carry_out) carry_out[sc * P::PAD + k] = run;
}

// the same for many tiles per stream-channel (a long lone stream: thousands of tiles on a few stream-channels, where one thread per bin walks them
// one after the other): 16 threads per bin take a sixteenth of the tiles each — sum it, exchange the 16 sums through LDS, prefix the own part
// (modular integer sums: the split changes no bit).  One workgroup per (stream-channel, 64 bins).  kSeg: the segmented scan, each sixteenth's
// summary a (reset seen, sum since the last reset) pair.
constexpr int kScanChunks = 16;
template <int N, bool kSeg = false>
__global__ __launch_bounds__(64 * kScanChunks) void pv_scan_chunked_kernel(uint32_t* __restrict__ sums, long long n_sc, int n_tiles,
                                                                          const uint32_t* __restrict__ carry_in, uint32_t* __restrict__ carry_out, int n_read)
{
    using P = PvAny<N>;
    __shared__ uint32_t part[kScanChunks][64];
    __shared__ uint32_t pflag[kSeg ? kScanChunks : 1][64];
    const int kb = threadIdx.x & 63, ck = threadIdx.x >> 6;
    const long long sc = blockIdx.x / P::NB;
    const int k = (int)(blockIdx.x % P::NB) * 64 + kb;
    const bool valid = k < P::B;
    const int per = (n_tiles + kScanChunks - 1) / kScanChunks;
    const int j0 = ck * per, j1 = (j0 + per < n_tiles) ? j0 + per : n_tiles;
    const int r1 = j1 < n_read ? j1 : n_read;                       // tiles at or beyond n_read count as zero
    uint32_t* p = sums + sc * n_tiles * (long long)P::PAD + (valid ? k : 0);
    const uint32_t* fl = sums + sc * n_tiles * (long long)P::PAD + P::B;   // kSeg: the tiles' reset flags (read only)
    uint32_t sum = 0, seen = 0;
    if (valid) {
        int j = j0;
        for (; j + 8 <= r1; j += 8) {
            uint32_t v[8], r[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                v[u] = p[(long long)(j + u) * P::PAD];
                if constexpr (kSeg) r[u] = fl[(long long)(j + u) * P::PAD];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                if constexpr (kSeg) { sum = r[u] ? v[u] : sum + v[u]; seen |= r[u]; }
                else sum += v[u];
            }
        }
        for (; j < r1; j++) {
            if constexpr (kSeg) {
                const uint32_t r = fl[(long long)j * P::PAD];
                sum = r ? p[(long long)j * P::PAD] : sum + p[(long long)j * P::PAD];
                seen |= r;
            } else sum += p[(long long)j * P::PAD];
        }
    }
    part[ck][kb] = sum;
    if constexpr (kSeg) pflag[ck][kb] = seen;
    __syncthreads();
    uint32_t run = (valid && carry_in) ? carry_in[sc * P::PAD + k] : 0u;
    for (int c2 = 0; c2 < ck; c2++) {
        if constexpr (kSeg) run = pflag[c2][kb] ? part[c2][kb] : run + part[c2][kb];
        else run += part[c2][kb];
    }
    if (!valid) return;
    int j = j0;
    for (; j + 8 <= r1; j += 8) {
        uint32_t v[8], r[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            v[u] = p[(long long)(j + u) * P::PAD];
            if constexpr (kSeg) r[u] = fl[(long long)(j + u) * P::PAD];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            p[(long long)(j + u) * P::PAD] = run;
            if constexpr (kSeg) run = r[u] ? v[u] : run + v[u];
            else run += v[u];
        }
    }
    for (; j < j1; j++) {
        const uint32_t v = (j < n_read) ? p[(long long)j * P::PAD] : 0u;
        p[(long long)j * P::PAD] = run;
        if constexpr (kSeg) run = (j < n_read && fl[(long long)j * P::PAD]) ? v : run + v;
        else run += v;
    }
    if (carry_out && ck == kScanChunks - 1) carry_out[sc * P::PAD + k] = run;
}

// ------------------------------------------------------------------------------------------------ pass 3
// kFormant: formant preservation with lifter `lifter` and transposer ratio g (nae_stretch_block_formant_f32); off, both are unused.
// kTransient: an onset frame takes Qs = Qa ("Transient preservation"); frames b0 - 2 and b0 - 1 prime P and "high".
template <int N, bool kUnit, bool kFormant, bool kTransient = false, bool kLink = false>
__global__ __launch_bounds__(64 * (PvAny<N, kFormant, kTransient, kLink>::kWaves3)) void pv_any_synth_kernel(SigViewD src, PvParams p, long long n_items,
                                                                                       const uint32_t* __restrict__ phase_ws, OutViewD out,
                                                                                       SpecAnyTables tb, int lifter, float g)
{
    static_assert(kTransient || !kLink, "unlocked, the link acts on the onset rule only");
    using P = PvAny<N, kFormant, kTransient, kLink>;
    using Gm = typename P::Gm;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[P::kWaves3 * Gm::SCR];
    __shared__ __attribute__((aligned(16))) cf yspec[P::kWaves3 * P::PAD];
    __shared__ uint32_t state[P::kWaves3 * 2 * P::ST];
    __shared__ float lbuf[kFormant ? P::kWaves3 * P::PAD : 1];   // formant: L, then c', then Ls
    __shared__ float pprev[kTransient ? P::kWaves3 * P::ST : 1];  // transients: P_{f-1} of bin lane + 64 r
    __shared__ float pother[kLink ? P::kWaves3 * P::ST : 1];      // link: the other channel's P_f
    for (int i = threadIdx.x; i < 512; i += 64 * P::kWaves3) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * P::kWaves3 + wave_id();
    if (item >= n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    cf* ys = yspec + wave_id() * P::PAD;
    float* lb = lbuf + (kFormant ? wave_id() * P::PAD : 0);
    uint32_t* qp = state + wave_id() * 2 * P::ST + lane;  // [r * 64]: Qa_{f-1} of bin lane + 64 r
    uint32_t* qs = qp + P::ST;                           //           Qs
    float* pp = pprev + (kTransient ? wave_id() * P::ST + lane : 0);
    float* po = pother + (kLink ? wave_id() * P::ST + lane : 0);
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long sc = w.sc, s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    const ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const ChanView in2{src.base + s_idx * src.ss + (c ^ 1) * src.cs, src.fs, p.in_len};   // link (ch == 2): the stream's other channel
    const long long b0 = p.f_origin + (long long)tile * p.tile;
    const long long b_end = b0 + p.tile < p.f_stop ? b0 + p.tile : p.f_stop;
    long long f_end = b_end + 3;                           // frames b0 .. b_end+2 feed blocks b0 .. b_end-1
    if (f_end > p.frames) f_end = p.frames;
    // b0 - 1 only primes Qa_{f-1}; with transients b0 - 2 and b0 - 1 also prime P and "high"
    const long long f_first = kTransient ? (b0 > 2 ? b0 - 2 : 0) : (b0 > 0 ? b0 - 1 : 0);
    float* optr = out.base + s_idx * out.ss + c * out.cs;

    // Qs in front of the tile: pass 2's record (or zero)
    const uint32_t* rec = phase_ws + (sc * p.phase_tiles + (long long)tile * p.phase_step) * P::PAD;
    for (int r = 0; r < P::NB; r++) {
        const int k = lane + 64 * r;
        qs[64 * r] = (p.base_zero || k >= P::B) ? 0u : rec[k];
        qp[64 * r] = 0;
    }
    float r0[P::K], r1[P::K], r2[P::K];
#pragma unroll
    for (int i = 0; i < P::K; i++) r0[i] = r1[i] = r2[i] = 0.0f;
    long long s_prev = 0;
    bool high_prev = false;                                // transients: high(f - 1), wave-uniform
#pragma unroll 1
    for (long long f = f_first; f < f_end; f++) {
        const long long s = pva_frame_start<N>(p, f);
        if constexpr (kLink) pva_other_power<N, kUnit>(scr, w512l, tb, in2, s, po, lane);
        pva_analyse<N, kUnit>(scr, w512l, tb, in, s, lane);
        const unsigned d = (unsigned)(s - s_prev);
        const unsigned R = (d == (unsigned)p.d0) ? p.r_q24_0 : p.r_q24_1;
        const bool live = f >= b0;                         // wave-uniform
        int rising = 0;
#pragma unroll 2
        for (int r = 0; r < P::NB; r++) {
            const int k = lane + 64 * r;
            const int kc = k < P::B ? k : P::M;
            const cf x = any_rfft_bin<Gm>(scr, tb.tn, kc);
            const uint32_t qa = pva_phase<N>(x, kc);
            if (live) {
                const uint32_t q = qs[64 * r] + ((f == 0) ? qa : pva_inc<N>(qa, qp[64 * r], (unsigned)kc, d, R));
                qs[64 * r] = q;
                if (k < P::B) ys[k] = pipe_rotate(x, q, qa);         // Y = X e^{i (Qs - Qa)}
                if constexpr (kFormant)
                    if (k < P::B) lb[k] = __builtin_amdgcn_logf(fmaxf(sqrt_rn(x.x * x.x + x.y * x.y), 0x1p-40f));   // L = log2 max(|X|, 2^-40)
            }
            qp[64 * r] = qa;
            if constexpr (kLink) rising += pva_rises_linked<N>(x, k, pp + 64 * r, po[64 * r], f > f_first);
            else if constexpr (kTransient) rising += pva_rises<N>(x, k, pp + 64 * r, f > f_first);
        }
        if constexpr (kTransient) {
            const bool high = f > f_first && pva_high<N>(rising);
            if (live && f >= 2 && high && !high_prev) {        // an onset: Qs = Qa_f, Y = X (wave-uniform)
#pragma unroll 1
                for (int r = 0; r < P::NB; r++) {
                    const int k = lane + 64 * r;
                    const int kc = k < P::B ? k : P::M;
                    const uint32_t qa = qp[64 * r];
                    qs[64 * r] = qa;
                    if (k < P::B) ys[k] = pipe_rotate(any_rfft_bin<Gm>(scr, tb.tn, kc), qa, qa);
                }
            }
            high_prev = high;
        }
        s_prev = s;
        if (!live) {
            wave_lds_sync();
            continue;
        }
        if (f == p.carry_frame) {
            for (int r = 0; r < P::NB; r++) {
                const int k = lane + 64 * r;
                if (k < P::B) p.carry_out[sc * P::PAD + k] = qs[64 * r];
            }
        }
        wave_lds_sync();
        if constexpr (kFormant) pva_formant<N>(scr, w512l, tb, ys, lb, lifter, g, lane);
        // c2r: split with T_N, conjugate, forward FFT_M (the first pass builds its inputs from Y), scale by 1/M and conjugate back
        auto zc = [&](int m) -> cf {
            cf xk = ys[m], xm = ys[P::M - m];
            if (m == 0) { xk.y = 0.0f; xm.y = 0.0f; }
            const cf E = {0.5f * (xk.x + xm.x), 0.5f * (xk.y - xm.y)};
            const cf D = {0.5f * (xk.x - xm.x), 0.5f * (xk.y + xm.y)};
            const cf T = tb.tn[m];
            const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};   // conj(T) D
            return cf{E.x - Q.y, -(E.y + Q.x)};
        };
        any_first_pass_from<Gm>(scr, w512l, tb.wm, lane, zc);
        any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
        wave_lds_sync();
        // windowed samples 2m, 2m + 1 (m = lane + 64 j) of quarter q = j / JQ, overlap-added in increasing frame order: block f - 3 is complete
        float o[P::K];
#pragma unroll 1
        for (int q = 0; q < 4; q++) {
            float y[P::K];
#pragma unroll
            for (int jj = 0; jj < P::JQ; jj++) {
                const int m = lane + 64 * (q * P::JQ + jj);
                const cf z = lds_ld(scr + padx(zpos<Gm>(m)));
                const float2 w = *reinterpret_cast<const float2*>(tb.hann + 2 * m);
                y[2 * jj] = w.x * (z.x * (1.0f / P::M));
                y[2 * jj + 1] = w.y * (-z.y * (1.0f / P::M));
            }
#pragma unroll
            for (int i = 0; i < P::K; i++) {
                if (q == 0) o[i] = (r0[i] + y[i]) * NAE_OLA_GAIN;
                else if (q == 1) r0[i] = r1[i] + y[i];
                else if (q == 2) r1[i] = r2[i] + y[i];
                else r2[i] = y[i];
            }
        }
        wave_lds_sync();                                   // the next frame rewrites the scratch and Y
        pva_store_block<N>(p, b0, b_end, optr, out.fs, f - 3, o, lane);
    }
    // frames past the last one do not exist: the blocks they would have completed get nothing more
#pragma unroll 1
    for (long long f = f_end > b0 ? f_end : b0; f < b_end + 3; f++) {
        float o[P::K];
#pragma unroll
        for (int i = 0; i < P::K; i++) {
            o[i] = r0[i] * NAE_OLA_GAIN;
            r0[i] = r1[i];
            r1[i] = r2[i];
            r2[i] = 0.0f;
        }
        pva_store_block<N>(p, b0, b_end, optr, out.fs, f - 3, o, lane);
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// (unlocked, the link acts on the onset rule only: a linked kernel without transients does not exist, and nae_pv_resolve asks for none)
template <int N, bool kUnit, bool kTransient, bool kLink>
static int launch_phase(nae_ctx* ctx, const PvJob& j, const SpecAnyTables& tb)
{
    if constexpr (kLink && !kTransient) return nae_fail(ctx, NAE_ERR_INVALID, "pv_any_phase_kernel: the link needs transients");
    else {
        using P = PvAny<N, false, kTransient, kLink>;
        const char* name = kLink ? "pv_any_phase_link_kernel" : kTransient ? "pv_any_phase_transient_kernel" : "pv_any_phase_kernel";
        const long long items = j.n_sc * j.p.n_tiles;
        return nae_launch_tiles(ctx, name, "pv_any_phase_kernel: grid too large", pv_any_phase_kernel<N, kUnit, kTransient, kLink>, items, P::kWaves1,
                                64 * P::kWaves1, 0, j.src, j.p, items, j.phase_ws, tb);
    }
}

// from 256 tiles per stream-channel on, 16 threads per bin (pv_scan_chunked_kernel, one workgroup per (stream-channel, 64 bins)); else one
// (pv_scan_kernel, 256 threads per workgroup)
template <int N, bool kSeg>
static int launch_scan(nae_ctx* ctx, const char* name, uint32_t* phase_ws, long long n_sc, int n_tiles, const uint32_t* carry_in,
                       uint32_t* carry_out, int n_read)
{
    using P = PvAny<N>;
    const char* grid_err = "pv_scan_kernel: grid too large";
    if (n_tiles >= 256 && n_sc * P::NB <= 0x7fffffffll) {
        if (kSeg) name = "pv_any_scan_chunked_transient_kernel";   // the segmented scans have profile names of their own
        return nae_launch_tiles(ctx, name, grid_err, pv_scan_chunked_kernel<N, kSeg>, n_sc * P::NB, 1, 64 * kScanChunks, 0, phase_ws, n_sc, n_tiles,
                                carry_in, carry_out, n_read);
    }
    if (kSeg) name = "pv_any_scan_transient_kernel";
    return nae_launch_tiles(ctx, name, grid_err, pv_scan_kernel<N, kSeg>, n_sc * P::PAD, 256, 256, 0, phase_ws, n_sc, n_tiles, carry_in, carry_out,
                            n_read);
}

template <int N, bool kUnit, bool kFormant, bool kTransient, bool kLink>
static int launch_synth(nae_ctx* ctx, const PvJob& j, const SpecAnyTables& tb)
{
    if constexpr (kLink && !kTransient) return nae_fail(ctx, NAE_ERR_INVALID, "pv_any_synth_kernel: the link needs transients");
    else {
        using P = PvAny<N, kFormant, kTransient, kLink>;
        const char* name = kLink      ? (kFormant ? "pv_any_synth_formant_link_kernel" : "pv_any_synth_link_kernel")
                         : kTransient ? (kFormant ? "pv_any_synth_formant_transient_kernel" : "pv_any_synth_transient_kernel")
                                      : (kFormant ? "pv_any_synth_formant_kernel" : "pv_any_synth_kernel");
        const long long items = j.n_sc * j.p.n_tiles;
        if (items == 0) return NAE_OK;
        return nae_launch_tiles(ctx, name, "pv_any_synth_kernel: grid too large", pv_any_synth_kernel<N, kUnit, kFormant, kTransient, kLink>, items,
                                P::kWaves3, 64 * P::kWaves3, 0, j.src, j.p, items, j.phase_ws, j.out, tb, j.lifter, j.g);
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

size_t nae_pv_record_pad(int n_fft) { return (size_t)((n_fft / 2 + 1 + 7) & ~7); }

int nae_pv_resident(nae_ctx* ctx, const nae_pv_run& r, PvKernels pass3)
{
    if (pass3 == PvKernels::kLock) return 16;
    return at_size(ctx, r.n_fft, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if (pass3 == PvKernels::kEnv) return PvEnv<N>::kResident;
        return with_flags(r.lifter > 0, r.transients, r.link, [&](auto f, auto t, auto l) { return PvAny<N, f.value, t.value, t.value && l.value>::kResident3; });
    });
}

int nae_launch_pvany_phase(nae_ctx* ctx, const PvJob& j)
{
    SpecAnyTables tb;
    int rc = nae_spec_any_tables(ctx, j.n_fft, &tb);
    if (rc) return rc;
    return at_size(ctx, j.n_fft, [&](auto n) {
        return with_flags(j.unit_stride, j.transients, j.link,
                          [&](auto u, auto t, auto l) { return launch_phase<decltype(n)::value, u.value, t.value, l.value>(ctx, j, tb); });
    });
}

int nae_launch_pv_scan(nae_ctx* ctx, int n_fft, const char* name, uint32_t* phase_ws, long long n_sc, int n_tiles, const uint32_t* carry_in,
                       uint32_t* carry_out, int n_read, bool segmented)
{
    return at_size(ctx, n_fft, [&](auto n) {
        return with_flags(segmented, [&](auto seg) {
            return launch_scan<decltype(n)::value, seg.value>(ctx, name, phase_ws, n_sc, n_tiles, carry_in, carry_out, n_read);
        });
    });
}

int nae_launch_pvany_synth(nae_ctx* ctx, const PvJob& j)
{
    SpecAnyTables tb;
    int rc = nae_spec_any_tables(ctx, j.n_fft, &tb);
    if (rc) return rc;
    return at_size(ctx, j.n_fft, [&](auto n) {
        return with_flags(j.unit_stride, j.lifter > 0, j.transients, j.link, [&](auto u, auto f, auto t, auto l) {
            return launch_synth<decltype(n)::value, u.value, f.value, t.value, l.value>(ctx, j, tb);
        });
    });
}
