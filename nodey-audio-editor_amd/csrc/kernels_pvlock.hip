// kernels_pvlock.hip — K7 phase vocoder with identity phase locking (NAE_STRETCH_PHASE_LOCK; DESIGN.md §3, "Phase locking") for gfx950.
//
// The locked Qs recurrence of frame f is a map M_f = (sigma_f, c_f): Qs_f[k] = Qs_{f-1}[sigma_f[k]] + c_f[k] (uint32, wrapping).  Maps compose
// exactly — (sigma_b, c_b) o (sigma_a, c_a) = (sigma_a[sigma_b], c_a[sigma_b] + c_b), a first — so the three passes of the unlocked vocoder
// (kernels_stft.hip) keep their shape, with a map where they had a sum:
//   pass L1 (pvlock_map_kernel)   one wave per (stream-channel, pass-1 tile): analysis, power, peaks, regions and M_f of each frame, composed into
//                                 the tile's map (sigma uint16, c uint32);
//   pass L2 (pvlock_scan_kernel)  per stream-channel, the tile maps applied in order: Qs in front of every tile (the record format of the
//                                 unlocked scan), carry_in / carry_out as there.  Many tiles: 16 chunks composed side by side, then prefixed;
//   pass L3 (pvlock_synth_kernel) one wave per synthesis tile: from the recorded Qs it walks its frames forward — re-analysis, M_f applied to the
//                                 Qs vector in LDS, rotation, inverse FFT, window, overlap-add in increasing frame order — and stores its blocks.
// Every integer is exact, so any tiling gives the same bits; the samples follow the oracle's tolerance path (|X| e^{i Qs}, inverse FFT, overlap-add).
// kLink (NAE_STRETCH_LINK_CHANNELS; DESIGN.md §3, "Channel link"): the wave of channel c also analyses channel c ^ 1 of its stream in front of each
// frame and keeps its power (9 registers); peaks, regions and the onset rule read Pl = 0.5 (P^0 + P^1), so sigma_f and the resets are the same in
// both channels' waves.  B, Qa, inc and Qs stay the channel's own; pass L2 is unchanged.
// The default (unlocked) path runs none of these kernels.  The host decisions of both modes (parameters, records needed, base records, synthesis
// fields, workspace layout) are kernels_stft.hip's nae_launch_pv_phase / nae_launch_pv_synth; the launchers here only launch.
#include "pv_roles.h"

namespace nae {

// ------------------------------------------------------------------------------------------------ per-frame lock step
// Per-wave LDS of the lock step: the FFT scratch (576 complex = 1152 words) doubles, once the spectrum is in registers, as
//   words [0, 520):    P[k] (float bits), then sigma_f[k]
//   words [520, 1040): B[k] = inc[k] - Qa[k]   (c_f[k] = B[sigma_f[k]] + Qa[k]: the same integer as inc[p] + (Qa[k] - Qa[p]))
constexpr int kLockB = kT1024Pad;
constexpr int kNoPeakHi = 4096;                   // "no peak to the right" (any index above 512)
static_assert(2 * kT1024Pad <= 2 * kPadScratchCf, "P / sigma and B fit the FFT scratch");

// one frame's analysis: canonical X (v[r] = X[lane + 64 r], nyq = X[512] in every lane) and its phases
template <bool kUnit>
__device__ __forceinline__ void lock_analyse(cf (&v)[8], cf& nyq, uint32_t (&qa)[9], const ChanView& in, long long s, const float* hann, cf* scratch,
                                             const cf* twa, const cf* w64, const cf* t1024, int lane)
{
    load_frame_windowed<kUnit>(v, in, s, hann, lane);
    fft512_pad(v, make_fft_lds(scratch, twa, w64, lane));
    nyq = rfft_split<false>(v, scratch, t1024, lane);
    phases_of(v, nyq, qa);
}

// channel link: P of the stream's other channel for frame start s, for this lane's bins (the analysis of lock_analyse without the phases)
template <bool kUnit>
__device__ __forceinline__ void lock_other_power(float (&po)[9], const ChanView& in2, long long s, const float* hann, cf* scratch, const cf* twa,
                                                 const cf* w64, const cf* t1024, int lane)
{
    cf v[8];
    load_frame_windowed<kUnit>(v, in2, s, hann, lane);
    fft512_pad(v, make_fft_lds(scratch, twa, w64, lane));
    const cf nyq = rfft_split<false>(v, scratch, t1024, lane);
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const cf x = r < 8 ? v[r] : nyq;
        po[r] = x.x * x.x + x.y * x.y;
    }
}

// the linked power Pl = 0.5 (P^0 + P^1) of this lane's bins, in place over the other channel's P: one IEEE add (it commutes, so either channel's
// wave gets the bits of P^0 + P^1), one product
__device__ __forceinline__ void lock_linked_power(const cf (&v)[8], cf nyq, float (&pl)[9])
{
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const cf x = r < 8 ? v[r] : nyq;
        pl[r] = 0.5f * ((x.x * x.x + x.y * x.y) + pl[r]);
    }
}

// M_f of frame f >= 1 for this lane's bins k = lane + 64 r (r = 8: k = 512, meaningful in lane 0).  qp: Qa_{f-1}.
// Power (two products, one add, never fused), peaks, nearest-peak regions: DESIGN.md §3, rules 1-3.  kLink: peaks and regions on the linked power pl.
template <bool kLink = false>
__device__ __forceinline__ void lock_map_of_frame(const cf (&v)[8], cf nyq, const uint32_t (&qa)[9], const uint32_t (&qp)[9], unsigned d, unsigned R,
                                                  cf* scratch, int lane, uint32_t (&sig)[9], uint32_t (&c)[9], const float* pl = nullptr)
{
    uint32_t* w = reinterpret_cast<uint32_t*>(scratch);
    float* P = reinterpret_cast<float*>(scratch);
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const unsigned k = r < 8 ? (unsigned)(lane + 64 * r) : 512u;
        const cf x = r < 8 ? v[r] : nyq;
        const uint32_t inc = pipe_inc(qa[r], qp[r], k, d, R);
        if (r < 8 || lane == 0) {
            if constexpr (kLink) P[k] = pl[r];
            else P[k] = x.x * x.x + x.y * x.y;
            w[kLockB + k] = inc - qa[r];
        }
    }
    wave_lds_sync();
    // contiguous bins: lane l owns k0 .. k0 + 7 (lane 63 also 512); it reads P[k0 - 2 .. k0 + 10]
    const int k0 = 8 * lane;
    const int nb = lane == 63 ? 9 : 8;
    float pw[13];
#pragma unroll
    for (int j = 0; j < 13; j++) {
        const int i = k0 - 2 + j;
        pw[j] = (i >= 0 && i < NAE_FFT_BINS) ? P[i] : 0.0f;
    }
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const int k = k0 + j;
        bool ok = pw[j + 2] > 0.0f;
        ok = ok && (k < 1 || pw[j + 2] > pw[j + 1]);
        ok = ok && (k < 2 || pw[j + 2] > pw[j]);
        ok = ok && (k + 1 >= NAE_FFT_BINS || pw[j + 2] >= pw[j + 3]);
        ok = ok && (k + 2 >= NAE_FFT_BINS || pw[j + 2] >= pw[j + 4]);
        if (ok && j < nb) pk |= 1u << j;
    }
    // nearest peak to the left (prefix max of peak indices) and to the right (suffix min), across the wave
    const int last = pk ? k0 + 31 - __builtin_clz(pk) : -1;
    const int first = pk ? k0 + __builtin_ctz(pk) : kNoPeakHi;
    int lmax = last, rmin = first;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(lmax, o, 64), b = __shfl_down(rmin, o, 64);
        if (lane >= o) lmax = a > lmax ? a : lmax;
        if (lane + o < 64) rmin = b < rmin ? b : rmin;
    }
    int left = __shfl_up(lmax, 1, 64), right = __shfl_down(rmin, 1, 64);
    if (lane == 0) left = -1;
    if (lane == 63) right = kNoPeakHi;
    int lft[9], rgt[9];
#pragma unroll
    for (int j = 0; j < 9; j++) {
        if (pk & (1u << j)) left = k0 + j;
        lft[j] = left;
    }
#pragma unroll
    for (int j = 8; j >= 0; j--) {
        if (pk & (1u << j)) right = k0 + j;
        rgt[j] = right;
    }
    wave_lds_sync();                              // every lane's P reads are done: sigma_f replaces P
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const int k = k0 + j;
        int s;
        if (lft[j] < 0 && rgt[j] >= kNoPeakHi) s = k;                 // no peak in the frame: unlocked
        else if (lft[j] < 0) s = rgt[j];
        else if (rgt[j] >= kNoPeakHi) s = lft[j];
        else s = (k - lft[j] <= rgt[j] - k) ? lft[j] : rgt[j];        // a tie goes to the lower peak
        if (j < nb) w[k] = (uint32_t)s;
    }
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = r < 8 ? lane + 64 * r : 512;
        sig[r] = w[k];
        c[r] = w[kLockB + sig[r]] + qa[r];
    }
    wave_lds_sync();                              // the scratch is free again
}

// transient preservation ("Transient preservation"), rules 1-4 for this lane's bins k = lane + 64 r (r = 8: k = 512, lane 0):
// P = |X|^2 (two products and an add, never fused) against the previous frame's P in pp (registers), counted across the wave with a ballot; pp
// takes P.  Returns high(f); counted = false (the first frame of a walk) counts nothing.
__device__ __forceinline__ bool lock_high(const cf (&v)[8], cf nyq, float (&pp)[9], bool counted, int lane)
{
    int rising = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const cf x = r < 8 ? v[r] : nyq;
        const float P = x.x * x.x + x.y * x.y;
        const bool mine = r < 8 || lane == 0;
        const bool rise = counted && mine && P > NAE_TRANSIENT_RISE * pp[r] && P > NAE_TRANSIENT_FLOOR * (float)NAE_FFT_N;
        rising += __popcll(__ballot(rise));
        pp[r] = P;
    }
    return counted && NAE_TRANSIENT_DEN * rising >= NAE_TRANSIENT_NUM * NAE_FFT_BINS;
}

// lock_high on the linked power pl ("Channel link"); pp keeps Pl_{f-1}
__device__ __forceinline__ bool lock_high_linked(const float (&pl)[9], float (&pp)[9], bool counted, int lane)
{
    int rising = 0;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const float P = pl[r];
        const bool mine = r < 8 || lane == 0;
        const bool rise = counted && mine && P > NAE_TRANSIENT_RISE * pp[r] && P > NAE_TRANSIENT_FLOOR * (float)NAE_FFT_N;
        rising += __popcll(__ballot(rise));
        pp[r] = P;
    }
    return counted && NAE_TRANSIENT_DEN * rising >= NAE_TRANSIENT_NUM * NAE_FFT_BINS;
}

// ------------------------------------------------------------------------------------------------ pass L1
// tile maps: c at maps[rec * 520 + k] (uint32), sigma at sig16[rec * 520 + k] (uint16), rec = sc * n_tiles + tile.  kTransient: an onset frame's
// map is the reset map (Qs = Qa: it ignores its input), the running map becomes it, and maps[rec * 520 + 513] (a padding slot) is 1 when the tile
// holds an onset — the map (sigma, c, r) of DESIGN.md §3; frames f0 - 2 and f0 - 1 prime P and "high" 
constexpr size_t kLockMapWave = kPadScratchCf * sizeof(cf) + kT1024Pad * (sizeof(uint16_t) + sizeof(uint32_t));
constexpr size_t kLdsLockMap = kLdsTablesPad + kWaves * kLockMapWave;
static_assert(2 * kLdsLockMap <= 160 * 1024, "two workgroups per CU");

template <bool kUnit, bool kTransient = false, bool kLink = false>
__global__ __launch_bounds__(kThreads, 4) void pvlock_map_kernel(SigViewD src, PvParams p, long long n_items, uint32_t* __restrict__ maps,
                                                                 uint16_t* __restrict__ sig16, Tables tb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* hann; cf *t1024, *w64, *twa;
    stage_tables(smem, tb, blockDim.x, hann, t1024, w64, twa);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned char* mine = smem + kLdsTablesPad + (size_t)wave_id() * kLockMapWave;
    cf* scratch = reinterpret_cast<cf*>(mine);
    uint32_t* mc = reinterpret_cast<uint32_t*>(mine + kPadScratchCf * sizeof(cf));
    uint16_t* ms = reinterpret_cast<uint16_t*>(mc + kT1024Pad);
    const long long item = (long long)blockIdx.x * kWaves + wave_id();
    if (item >= n_items) return;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    if (tile >= p.skip_from) return;                    // wave-uniform
    ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const ChanView in2{src.base + s_idx * src.ss + (c ^ 1) * src.cs, src.fs, p.in_len};   // link (ch == 2): the stream's other channel

    const long long f0 = p.f_origin + (long long)tile * p.tile;
    long long f1 = f0 + p.tile;
    if (f1 > p.f_stop) f1 = p.f_stop;
    // the running map starts as the identity
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = lane + 64 * r;
        if (k < NAE_FFT_BINS) { mc[k] = 0u; ms[k] = (uint16_t)k; }
    }
    uint32_t qp[9], qa[9];
#pragma unroll
    for (int r = 0; r < 9; r++) qp[r] = 0;
    cf v[8], nyq;
    long long s_prev = 0;
    const long long f_first = kTransient ? (f0 > 2 ? f0 - 2 : 0) : (f0 > 0 ? f0 - 1 : 0);
    float pp[9];                                        // transients: P_{f-1} of this lane's bins
    bool high_prev = false;                             //             high(f - 1), wave-uniform
    uint32_t reset = 0;                                 //             an onset in [f0, f1)
    float pl[9];                                        // link: Pl_f of this lane's bins
#pragma unroll 1
    for (long long f = f_first; f < f1; f++) {
        const long long s = frame_start(p, f);
        if constexpr (kLink) lock_other_power<kUnit>(pl, in2, s, hann, scratch, twa, w64, t1024, lane);
        lock_analyse<kUnit>(v, nyq, qa, in, s, hann, scratch, twa, w64, t1024, lane);
        if constexpr (kLink) lock_linked_power(v, nyq, pl);
        bool onset = false;
        if constexpr (kTransient) {
            const bool high = kLink ? lock_high_linked(pl, pp, f > f_first, lane) : lock_high(v, nyq, pp, f > f_first, lane);
            onset = f >= 2 && high && !high_prev;
            high_prev = high;
        }
        if (f >= f0) {
            uint32_t sg[9], cc[9];
            if (f == 0 || onset) {
                // Qs_0 = Qa_0: the map (identity, Qa_0) applied to the zero phase in front of the stream; an onset's reset map is the same,
                // and whatever ran before it no longer matters
                if (onset) reset = 1;
#pragma unroll
                for (int r = 0; r < 9; r++) { sg[r] = r < 8 ? (uint32_t)(lane + 64 * r) : 512u; cc[r] = qa[r]; }
            } else {
                const unsigned d = (unsigned)(s - s_prev);
                const unsigned R = (d == (unsigned)p.d0) ? p.r_q24_0 : p.r_q24_1;
                lock_map_of_frame<kLink>(v, nyq, qa, qp, d, R, scratch, lane, sg, cc, pl);
            }
            // running map, then this frame: (ms[sg], mc[sg] + cc), or after a reset map the reset map; all gathers land before the first write
            uint32_t ns[9], nc[9];
#pragma unroll
            for (int r = 0; r < 9; r++) {
                if (onset) { ns[r] = sg[r]; nc[r] = cc[r]; }
                else { ns[r] = ms[sg[r]]; nc[r] = mc[sg[r]] + cc[r]; }
            }
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int k = lane + 64 * r;
                if (k < NAE_FFT_BINS) { ms[k] = (uint16_t)ns[r]; mc[k] = nc[r]; }
            }
            wave_lds_sync();
        }
#pragma unroll
        for (int r = 0; r < 9; r++) qp[r] = qa[r];
        s_prev = s;
    }
    uint32_t* oc = maps + item * kT1024Pad;
    uint16_t* os = sig16 + item * kT1024Pad;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = lane + 64 * r;
        if (k < NAE_FFT_BINS) { oc[k] = mc[k]; os[k] = ms[k]; }
    }
    if (kTransient && lane == 0) oc[NAE_FFT_BINS] = reset;   // slot 513 of the c record (padded to 520)
}

// ------------------------------------------------------------------------------------------------ pass L2
// One workgroup per stream-channel, one wave per chunk of tiles (1 chunk, or kLockChunks from 256 tiles on).  Tiles >= n_read are the identity
// (their maps were not computed); record t = Qs in front of tile t, carry_out = Qs behind the last tile.  kTransient: a tile map with slot 513 set
// is a reset map — composed after anything it is itself (sigma_b, c_b, 1), applied it gives c_b — and a chunk's map carries the flag in the same
// slot of its c array; the carried phase does not cross a reset.
constexpr int kLockChunks = 16;
constexpr size_t kLockScanWave = 3 * kT1024Pad * sizeof(uint32_t);      // chunk map (sigma, c) and the wave's running Qs

template <bool kTransient = false>
__global__ __launch_bounds__(64 * kLockChunks) void pvlock_scan_kernel(uint32_t* __restrict__ rec, const uint32_t* __restrict__ maps,
                                                                      const uint16_t* __restrict__ sig16, int n_tiles, const uint32_t* __restrict__ carry_in,
                                                                      uint32_t* __restrict__ carry_out, int n_read)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, ck = wave_id(), nch = (int)(blockDim.x >> 6);
    const long long sc = blockIdx.x;
    uint32_t* base = reinterpret_cast<uint32_t*>(smem);
    auto chunk_s = [&](int w) { return base + (size_t)w * 3 * kT1024Pad; };
    auto chunk_c = [&](int w) { return base + (size_t)w * 3 * kT1024Pad + kT1024Pad; };
    uint32_t* qs = base + (size_t)ck * 3 * kT1024Pad + 2 * kT1024Pad;
    const int per = (n_tiles + nch - 1) / nch;
    const int j0 = ck * per < n_tiles ? ck * per : n_tiles;
    const int j1 = j0 + per < n_tiles ? j0 + per : n_tiles;
    const int r1 = j1 < n_read ? j1 : n_read;
    const long long rec0 = sc * (long long)n_tiles;
    uint32_t* ms = chunk_s(ck);
    uint32_t* mc = chunk_c(ck);
    uint32_t chunk_reset = 0;                           // kTransient: a reset map among the chunk's tiles
    if (nch > 1) {
        // the chunk's map: its tiles composed in order
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) { ms[k] = (uint32_t)k; mc[k] = 0u; }
        }
        wave_lds_sync();
        for (int j = j0; j < r1; j++) {
            const uint32_t* tc = maps + (rec0 + j) * kT1024Pad;
            const uint16_t* ts = sig16 + (rec0 + j) * kT1024Pad;
            const bool rb = kTransient && tc[NAE_FFT_BINS] != 0u;   // wave-uniform
            if (rb) chunk_reset = 1;
            uint32_t ns[9], nc[9];
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int k = lane + 64 * r;
                if (k < NAE_FFT_BINS) {
                    const uint32_t sb = ts[k];
                    if (rb) { ns[r] = sb; nc[r] = tc[k]; }
                    else { ns[r] = ms[sb]; nc[r] = mc[sb] + tc[k]; }
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int k = lane + 64 * r;
                if (k < NAE_FFT_BINS) { ms[k] = ns[r]; mc[k] = nc[r]; }
            }
            wave_lds_sync();
        }
    }
    // Qs in front of the chunk: the carried phase (or zero), then the maps of the chunks before this one
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = lane + 64 * r;
        if (k < NAE_FFT_BINS) qs[k] = carry_in ? carry_in[sc * kT1024Pad + k] : 0u;
    }
    if (kTransient && nch > 1 && lane == 0) mc[NAE_FFT_BINS] = chunk_reset;   // the chunk map's flag, in slot 513 of its c array
    __syncthreads();
    for (int w = 0; w < ck; w++) {
        const uint32_t* ws = chunk_s(w);
        const uint32_t* wc = chunk_c(w);
        const bool rw = kTransient && wc[NAE_FFT_BINS] != 0u;      // wave-uniform
        uint32_t nq[9];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) nq[r] = rw ? wc[k] : qs[ws[k]] + wc[k];
        }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) qs[k] = nq[r];
        }
        wave_lds_sync();
    }
    // the chunk's own tiles: record, then apply
    for (int j = j0; j < j1; j++) {
        uint32_t* o = rec + (rec0 + j) * kT1024Pad;
        const uint32_t* tc = maps + (rec0 + j) * kT1024Pad;
        const uint16_t* ts = sig16 + (rec0 + j) * kT1024Pad;
        const bool rb = kTransient && j < n_read && tc[NAE_FFT_BINS] != 0u;   // wave-uniform
        uint32_t nq[9];
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) {
                o[k] = qs[k];
                nq[r] = rb ? tc[k] : j < n_read ? qs[ts[k]] + tc[k] : qs[k];
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) qs[k] = nq[r];
        }
        wave_lds_sync();
    }
    if (carry_out && ck == nch - 1) {
#pragma unroll
        for (int r = 0; r < 9; r++) {
            const int k = lane + 64 * r;
            if (k < NAE_FFT_BINS) carry_out[sc * kT1024Pad + k] = qs[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------ pass L3
constexpr size_t kLockSynthWave = kPadScratchCf * sizeof(cf) + kT1024Pad * sizeof(uint32_t);
constexpr size_t kLdsLockSynth = kLdsTablesPad + kWaves * kLockSynthWave;
static_assert(2 * kLdsLockSynth <= 160 * 1024, "two workgroups per CU");

// formant preservation ("Formant preservation") of one frame, in two steps around the rotation.  lock_formant_log: L = log2
// max(|X|, 2^-40) from this lane's bins k = lane + 64 r (r = 8: k = 512) into the FFT scratch, as floats.  lock_formant_apply: the cepstrum of L
// (in registers: n = 2 (lane + 64 r) + {0, 1}), lifted, its r2c Ls (into the scratch), and Y[k] *= G[k].
__device__ __forceinline__ void lock_formant_log(const cf (&v)[8], cf nyq, cf* scratch, int lane)
{
    float* lf = reinterpret_cast<float*>(scratch);
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const cf x = r < 8 ? v[r] : nyq;
        if (r < 8 || lane == 0) lf[r < 8 ? lane + 64 * r : 512] = __builtin_amdgcn_logf(fmaxf(sqrt_rn(x.x * x.x + x.y * x.y), 0x1p-40f));
    }
    wave_lds_sync();
}

__device__ __forceinline__ void lock_formant_apply(cf (&y)[8], cf& ynyq, cf* scratch, const cf* twa, const cf* w64, const cf* t1024, int q, float g,
                                                   int lane)
{
    float* lf = reinterpret_cast<float*>(scratch);
    // cepstrum c = c2r_N(L + 0i): the synthesis's split, FFT and 1/512
    cf u[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int k = lane + 64 * r;
        const cf Xk = {lf[k], 0.0f}, Xm = {lf[512 - k], 0.0f};
        const cf E = {0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y - Xm.y)};
        const cf D = {0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y + Xm.y)};
        const cf T = t1024[k];
        const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};
        u[r] = cf{E.x - Q.y, -(E.y + Q.x)};
    }
    wave_lds_sync();
    fft512_pad(u, make_fft_lds(scratch, twa, w64, lane));
    // lifter, then the envelope Ls = Re r2c_N(c') (packed pairs, no window)
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int n = 2 * (lane + 64 * r);
        const float c0 = u[r].x * (1.0f / 512.0f), c1 = -u[r].y * (1.0f / 512.0f);
        u[r] = cf{(n < q || n > NAE_FFT_N - q) ? c0 : 0.0f, (n + 1 < q || n + 1 > NAE_FFT_N - q) ? c1 : 0.0f};
    }
    fft512_pad(u, make_fft_lds(scratch, twa, w64, lane));
    const cf ls512 = rfft_split<false>(u, scratch, t1024, lane);
#pragma unroll
    for (int r = 0; r < 8; r++) lf[lane + 64 * r] = u[r].x;
    if (lane == 0) lf[512] = ls512.x;
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = r < 8 ? lane + 64 * r : 512;
        const float uk = (float)k * g;
        float G = 0.0f;
        if (uk <= 512.0f) {
            const int i = (int)uk;
            const float t = uk - (float)i;
            const float lu = i == 512 ? lf[512] : lf[i] + t * (lf[i + 1] - lf[i]);
            G = fminf(__builtin_amdgcn_exp2f(lu - lf[k]), NAE_FORMANT_MAX_GAIN);
        }
        cf& yk = r < 8 ? y[r] : ynyq;
        yk = cf{G * yk.x, G * yk.y};
    }
    wave_lds_sync();                              // Y replaces Ls in the scratch
}

// kFormant: formant preservation with lifter `lifter` and transposer ratio g; off, both are unused.  kTransient: an onset frame takes Qs = Qa
// ("Transient preservation"); frames b0 - 2 and b0 - 1 prime P and "high".
template <bool kUnit, bool kFormant, bool kTransient = false, bool kLink = false>
__global__ __launch_bounds__(kThreads, 4) void pvlock_synth_kernel(SigViewD src, PvParams p, long long n_items, const uint32_t* __restrict__ phase_ws,
                                                                   OutViewD out, Tables tb, int lifter, float g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* hann; cf *t1024, *w64, *twa;
    stage_tables(smem, tb, blockDim.x, hann, t1024, w64, twa);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned char* mine = smem + kLdsTablesPad + (size_t)wave_id() * kLockSynthWave;
    cf* scratch = reinterpret_cast<cf*>(mine);
    uint32_t* qs = reinterpret_cast<uint32_t*>(mine + kPadScratchCf * sizeof(cf));
    const long long item = (long long)blockIdx.x * kWaves + wave_id();
    if (item >= n_items) return;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long sc = w.sc, s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const ChanView in2{src.base + s_idx * src.ss + (c ^ 1) * src.cs, src.fs, p.in_len};   // link (ch == 2): the stream's other channel
    PipeItem it;
    it.sc = sc; it.s_idx = s_idx; it.c = c; it.tile = tile;
    it.b0 = p.f_origin + (long long)tile * p.tile;
    it.b_end = it.b0 + p.tile < p.f_stop ? it.b0 + p.tile : p.f_stop;
    long long f_end = it.b_end + 3;                              // frames b0 .. b_end+2 feed blocks b0 .. b_end-1
    if (f_end > p.frames) f_end = p.frames;
    // b0 - 1 only primes Qa_{f-1}; with transients b0 - 2 and b0 - 1 also prime P and "high"
    const long long f_first = kTransient ? (it.b0 > 2 ? it.b0 - 2 : 0) : (it.b0 > 0 ? it.b0 - 1 : 0);
    float* optr = out.base + s_idx * out.ss + c * out.cs;
    const BlockOut bo{optr, out.fs, (out.fs == 1) && ((reinterpret_cast<uintptr_t>(optr) & 15) == 0)};

    // Qs in front of the tile: pass L2's record (or zero)
    const uint32_t* b = phase_ws + (sc * p.phase_tiles + (long long)tile * p.phase_step) * kT1024Pad;
#pragma unroll
    for (int r = 0; r < 9; r++) {
        const int k = lane + 64 * r;
        if (k < NAE_FFT_BINS) qs[k] = p.base_zero ? 0u : b[k];
    }
    uint32_t qp[9], qa[9];
#pragma unroll
    for (int r = 0; r < 9; r++) qp[r] = 0;
    float r0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, r1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, r2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    cf v[8], nyq;
    long long s_prev = 0;
    float pp[9];                                                // transients: P_{f-1} of this lane's bins
    bool high_prev = false;                                     //             high(f - 1), wave-uniform
    float pl[9];                                                // link: Pl_f of this lane's bins
#pragma unroll 1
    for (long long f = f_first; f < f_end; f++) {
        const long long s = frame_start(p, f);
        if constexpr (kLink) lock_other_power<kUnit>(pl, in2, s, hann, scratch, twa, w64, t1024, lane);
        lock_analyse<kUnit>(v, nyq, qa, in, s, hann, scratch, twa, w64, t1024, lane);
        if constexpr (kLink) lock_linked_power(v, nyq, pl);
        bool onset = false;
        if constexpr (kTransient) {
            const bool high = kLink ? lock_high_linked(pl, pp, f > f_first, lane) : lock_high(v, nyq, pp, f > f_first, lane);
            onset = f >= 2 && high && !high_prev;
            high_prev = high;
        }
        if (f >= it.b0) {
            uint32_t sg[9], cc[9];
            if (f == 0 || onset) {                              // Qs_0 = Qa_0; an onset's Qs_f = Qa_f (applied to Qs_{f-1} = 0 below)
#pragma unroll
                for (int r = 0; r < 9; r++) { sg[r] = r < 8 ? (uint32_t)(lane + 64 * r) : 512u; cc[r] = qa[r]; }
            } else {
                const unsigned d = (unsigned)(s - s_prev);
                const unsigned R = (d == (unsigned)p.d0) ? p.r_q24_0 : p.r_q24_1;
                lock_map_of_frame<kLink>(v, nyq, qa, qp, d, R, scratch, lane, sg, cc, pl);
            }
            uint32_t nq[9];
#pragma unroll
            for (int r = 0; r < 9; r++) nq[r] = onset ? cc[r] : qs[sg[r]] + cc[r];
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const int k = lane + 64 * r;
                if (k < NAE_FFT_BINS) qs[k] = nq[r];
            }
            if (f == p.carry_frame) {
#pragma unroll
                for (int r = 0; r < 9; r++) {
                    const int k = lane + 64 * r;
                    if (k < NAE_FFT_BINS) p.carry_out[sc * kT1024Pad + k] = nq[r];
                }
            }
            // synthesis spectrum Y = X e^{i (Qs - Qa)} (formant: G X e^{i (Qs - Qa)}) in natural order, then the c2r pre-twiddle of the oracle's
            // irfft (conjugated: inverse = conj(FFT(conj Z)) / 512)
            if constexpr (kFormant) {
                lock_formant_log(v, nyq, scratch, lane);
#pragma unroll
                for (int r = 0; r < 8; r++) v[r] = pipe_rotate(v[r], nq[r], qa[r]);
                nyq = pipe_rotate(nyq, nq[8], qa[8]);
                lock_formant_apply(v, nyq, scratch, twa, w64, t1024, lifter, g, lane);
#pragma unroll
                for (int r = 0; r < 8; r++) scratch[lane + 64 * r] = v[r];
                if (lane == 0) scratch[512] = nyq;
            } else {
#pragma unroll
                for (int r = 0; r < 8; r++) scratch[lane + 64 * r] = pipe_rotate(v[r], nq[r], qa[r]);
                if (lane == 0) scratch[512] = pipe_rotate(nyq, nq[8], qa[8]);
            }
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int k = lane + 64 * r;
                cf Xk = scratch[k], Xm = scratch[512 - k];
                if (k == 0) { Xk.y = 0.0f; Xm.y = 0.0f; }
                const cf E = {0.5f * (Xk.x + Xm.x), 0.5f * (Xk.y - Xm.y)};
                const cf D = {0.5f * (Xk.x - Xm.x), 0.5f * (Xk.y + Xm.y)};
                const cf T = t1024[k];
                const cf Q = {T.x * D.x + T.y * D.y, T.x * D.y - T.y * D.x};
                v[r] = cf{E.x - Q.y, -(E.y + Q.x)};
            }
            wave_lds_sync();
            fft512_pad(v, make_fft_lds(scratch, twa, w64, lane));
            // time samples 2n, 2n+1 (n = lane + 64 r), windowed: quarter r >> 1 of the frame, offsets 2 lane + 128 (r & 1) + {0, 1}
            float y[4][4];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const float2 w = *reinterpret_cast<const float2*>(hann + 2 * (lane + 64 * r));
                y[r >> 1][2 * (r & 1)] = w.x * (v[r].x * (1.0f / 512.0f));
                y[r >> 1][2 * (r & 1) + 1] = w.y * (-v[r].y * (1.0f / 512.0f));
            }
            // block f - 3 is complete: its four contributions in increasing frame order, then the gain
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                o[i] = (r0[i] + y[0][i]) * NAE_OLA_GAIN;
                r0[i] = r1[i] + y[1][i];
                r1[i] = r2[i] + y[2][i];
                r2[i] = y[3][i];
            }
            r3_store_block(p, it, bo, f - 3, o, lane);
        }
#pragma unroll
        for (int r = 0; r < 9; r++) qp[r] = qa[r];
        s_prev = s;
    }
    // frames past the last one do not exist: the blocks they would have completed get nothing more
#pragma unroll 1
    for (long long f = f_end > it.b0 ? f_end : it.b0; f < it.b_end + 3; f++) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            o[i] = r0[i] * NAE_OLA_GAIN;
            r0[i] = r1[i];
            r1[i] = r2[i];
            r2[i] = 0.0f;
        }
        r3_store_block(p, it, bo, f - 3, o, lane);
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the kernels here take more than 64 KiB of dynamic LDS (the scan from 256 tiles on): the one launch path sets the attribute, as for the vocoder pipeline

// transients: the kTransient instantiations (reset maps, the segmented scan; profile names pvlock_map_transient_kernel and
// pvlock_scan_transient_kernel)
// link: the kLink instantiations of the map kernel (pvlock_map_link_kernel, pvlock_map_transient_link_kernel); the scan does not change
template <bool kUnit, bool kTransient, bool kLink>
static int launch_lock_map(nae_ctx* ctx, const PvJob& j, uint32_t* maps, uint16_t* sig16)
{
    const char* name = kLink ? (kTransient ? "pvlock_map_transient_link_kernel" : "pvlock_map_link_kernel")
                             : (kTransient ? "pvlock_map_transient_kernel" : "pvlock_map_kernel");
    const Tables tb = tables_1024(ctx);
    const long long items = j.n_sc * j.p.n_tiles;
    return nae_launch_tiles(ctx, name, "pvlock_map_kernel: grid too large", pvlock_map_kernel<kUnit, kTransient, kLink>, items, kWaves, kThreads, kLdsLockMap,
                            j.src, j.p, items, maps, sig16, tb);
}

// one workgroup per stream-channel, of one wave or (many tiles) of kLockChunks
template <bool kTransient>
static int launch_lock_scan(nae_ctx* ctx, const PvJob& j, int n_needed, const uint32_t* maps, const uint16_t* sig16, const uint32_t* carry_in,
                            uint32_t* carry_out)
{
    const char* name = kTransient ? "pvlock_scan_transient_kernel" : "pvlock_scan_kernel";
    const int nch = j.p.n_tiles >= 256 ? kLockChunks : 1;
    return nae_launch_tiles(ctx, name, "pvlock_scan_kernel: grid too large", pvlock_scan_kernel<kTransient>, j.n_sc, 1, 64 * nch, nch * kLockScanWave,
                            j.phase_ws, maps, sig16, j.p.n_tiles, carry_in, carry_out, n_needed);
}

int nae_launch_pvlock_phase(nae_ctx* ctx, const PvJob& j, int n_needed, uint32_t* maps, uint16_t* sig16, const uint32_t* carry_in, uint32_t* carry_out)
{
    const int rc = with_flags(j.unit_stride, j.transients, j.link,
                              [&](auto u, auto t, auto l) { return launch_lock_map<u.value, t.value, l.value>(ctx, j, maps, sig16); });
    if (rc) return rc;
    return with_flags(j.transients, [&](auto t) { return launch_lock_scan<t.value>(ctx, j, n_needed, maps, sig16, carry_in, carry_out); });
}

// kFormant: formant preservation (pvlock_synth_formant_kernel); kTransient: onsets reset Qs (the *_transient_kernel instantiations); kLink: the
// kLink instantiations (*_link_kernel)
template <bool kUnit, bool kFormant, bool kTransient, bool kLink>
static int launch_lock_synth(nae_ctx* ctx, const PvJob& j)
{
    const char* name = kLink ? (kTransient ? (kFormant ? "pvlock_synth_formant_transient_link_kernel" : "pvlock_synth_transient_link_kernel")
                                           : (kFormant ? "pvlock_synth_formant_link_kernel" : "pvlock_synth_link_kernel"))
                             : (kTransient ? (kFormant ? "pvlock_synth_formant_transient_kernel" : "pvlock_synth_transient_kernel")
                                           : (kFormant ? "pvlock_synth_formant_kernel" : "pvlock_synth_kernel"));
    const Tables tb = tables_1024(ctx);
    const long long items = j.n_sc * j.p.n_tiles;
    return nae_launch_tiles(ctx, name, "pvlock_synth_kernel: grid too large", pvlock_synth_kernel<kUnit, kFormant, kTransient, kLink>, items, kWaves, kThreads,
                            kLdsLockSynth, j.src, j.p, items, j.phase_ws, j.out, tb, j.lifter, j.g);
}

int nae_launch_pvlock_synth(nae_ctx* ctx, const PvJob& j)
{
    if (j.n_sc * j.p.n_tiles == 0) return NAE_OK;
    return with_flags(j.unit_stride, j.lifter > 0, j.transients, j.link,
                      [&](auto u, auto f, auto t, auto l) { return launch_lock_synth<u.value, f.value, t.value, l.value>(ctx, j); });
}
