// kernels_spectrum.hip — K8 magnitude spectrum for gfx950: n_fft = 256 ... 4096 (powers of two), any hop 1 <= hop <= n_fft.
//
// Three kernels behind one launcher (nae_launch_spectrum, at the end of this file):
//   spectrum_stereo_kernel<kWide>  1024 / 256, interleaved stereo with a 16-byte aligned stream base and an even stream stride
//   spectrum_kernel<kUnit>         1024 / 256, every other layout (debug key spec_generic: interleaved stereo too)
//   spectrum_any_kernel<N, kLoad>  every other size and hop (debug key spec_any: 1024 / 256 too)
// The two 1024-point kernels run the padded FFT512 of stft_device.h; all three give the canonical spectrum of DESIGN.md §3.
// Replaces the FFTW-based spectrum the reference declares but never implements.
#include "stft_common.h"
#include "fft_any.h"
#include <math.h>

namespace nae {

// ------------------------------------------------------------------------------------------------ 1024 / 256
constexpr size_t kLdsSpec = kLdsTablesPad + kWaves * kPadScratchCf * sizeof(cf);   // both 1024-point kernels
static_assert(3 * kLdsSpec <= 160 * 1024, "three workgroups per CU");

// one wave per (stream, frame); channels looped so an interleaved source is fetched by one wave.  54 / 84 VGPRs (kUnit true / false):
// six / five waves per SIMD (a minimum of 6 in the launch bounds makes the strided form spill)
template <bool kUnit>
__global__ __launch_bounds__(kThreads, 4) void spectrum_kernel(SigViewD src, long long T, int ch, long long n_frames,
                                                           long long n_items, float* __restrict__ dst,
                                                           long long dst_ss, Tables tb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* hann; cf *t1024, *w64, *twa;
    stage_tables(smem, tb, kThreads, hann, t1024, w64, twa);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    cf* scratch = reinterpret_cast<cf*>(smem + kLdsTablesPad) + wave_id() * kPadScratchCf;
    const long long item = (long long)blockIdx.x * kWaves + wave_id();
    if (item >= n_items) return;
    const long long s = item / n_frames, f = item % n_frames;
    const int kl = kl_of_lane(lane);
    for (int c = 0; c < ch; c++) {
        ChanView in{src.base + s * src.ss + c * src.cs, src.fs, T};
        cf v[8];
        load_frame_windowed<kUnit>(v, in, f * NAE_HOP, hann, lane);
        fft512_pad(v, make_fft_lds(scratch, twa, w64, lane));
        const cf nyq = rfft_split(v, scratch, t1024, lane);
        float* o = dst + s * dst_ss + (f * ch + c) * NAE_FFT_BINS;
#pragma unroll
        for (int r = 0; r < 8; r++) o[kl + 64 * r] = __builtin_sqrtf(v[r].x * v[r].x + v[r].y * v[r].y);
        if (lane == 0) o[512] = __builtin_sqrtf(nyq.x * nyq.x + nyq.y * nyq.y);
    }
}

// interleaved-stereo fast path: one 16-byte load per lane and row fetches (L0 R0 L1 R1), so a frame is read once for both
// channels and the window is applied once; requires a 16-byte aligned stream base and an even stream stride.
// A wave walks kSpecChunk consecutive frames of one stream; both channels run FFT -> r2c split -> magnitude on the padded low-register FFT (stft_device.h).
// Loop order:  window(f) -> stores(f-1) -> loads(f+1) -> FFT / split / magnitudes of frame f.  Vector-memory operations of a
// wave retire in issue order and share one counter, so a load issued behind its own frame's 18 stores can only be waited
// for together with them — and a store takes microseconds to be acknowledged.  Here the wait in front of window(f) covers
// the loads of frame f and, older than them, only the stores of frame f-2.  The magnitudes of the previous frame ride along
// in 18 registers.  (tools/ubench/spec_abl.hip, profiles/r02_spectrum_ablation.md: 3.43 -> 3.16 ms on the C5 signal; stores
// that bypass L2 allocation — they are never read again by this kernel — another 0.1-0.3 ms.)
constexpr int kSpecChunk = 32;         // frames one wave walks when the launch has many rounds of waves (16 / 64 / 128 measured
                                       // within 1 %: profiles/r02_spectrum_ablation.md); small batches: spec_pick_chunk
constexpr int kSpecChunkLarge = 16;    // frames per chunk of a large (persistent, chunk-drawing) launch: 12-16 measured 1.8 % faster than 32 at C5, 8 5 % slower
                                       // (round 6, gpurun_out: 2.70-2.73 against 2.76-2.78 and 2.92 ms; a chunk's head re-reads 3/4 of a frame)
constexpr int kSpecChunkFine = 8;      // frames of the short chunks at the end of a large launch's work list
constexpr int kSpecStoreAux = 2;       // cache policy bits of the spectrum stores (2 = nt)

// kWide (dst 16-byte aligned, even stream stride): a frame's two spectra are 4104 CONTIGUOUS bytes of the output; the wave drops its
// magnitudes into its FFT scratch in output order (the scratch is idle between two frames) and writes them back with 16 bytes
// per lane on 16-byte boundaries — four whole-wave 1-KiB pieces per frame instead of eighteen 256-byte dword pieces at every
// 4-byte phase of a line (the shape tools/ubench/rw_mix.hip measures the chip's streaming rate with).  4104 = 8 mod 16: the 8
// bytes by which a frame overhangs its last piece are carried in a register and go out with the next frame's first piece.
// Work distribution.  The launch is PERSISTENT: at most two workgroups per CU (what fits), and every wave draws its next chunk of
// consecutive frames from a device counter until the list is empty.  Round 5 measured why (tools/experiments/r05_spec_stamps.*): with
// one chunk per wave and 14.75 rounds of workgroups per CU, the waves of a workgroup left its slot up to 20 % apart — 10 % of all
// wave-slot time idle behind waves that had finished, 6 % more between workgroups.  The list is GUIDED: chunks of `chunk_c` frames for
// the first `coarse_streams` streams, then chunks of `chunk_f` (short: a quarter of the re-read at a chunk's head, but the launch's tail is
// one SHORT chunk long) for the rest.  Which wave computes which chunk does not touch any result.
// A wave's FIRST item is the one of its position in the grid (no atomic: 4096 waves drawing from one address at the same moment cost a
// small batch 0.15 ms); item n_waves + counter++ comes next.  The host zeroes the counter on the launch's stream in front of every launch
// that draws (a 4-byte fill: ~3 us; an earlier form let the launch's last wave reset it — one launch that dies would have left every later
// one on the context with a stale count).
struct SpecWork {
    int chunk_c, chunk_f;
    unsigned cps_c, cps_f;         // chunks per stream, coarse / fine
    unsigned coarse_streams;
    unsigned n_coarse;             // coarse items = coarse_streams * cps_c
    unsigned n_items;
    unsigned n_waves;              // waves of the launch
    unsigned dynamic;              // 0: no more items than waves — every wave works on the item of its position and nobody touches the counters
    unsigned* counters;
};

template <bool kWide>
__global__ __launch_bounds__(kThreads, 4) void spectrum_stereo_kernel(const float* __restrict__ src, long long src_ss, long long n_frames, SpecWork work,
                                                                     float* __restrict__ dst, long long dst_ss, Tables tb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* hann; cf *t1024, *w64, *twa;
    stage_tables(smem, tb, kThreads, hann, t1024, w64, twa);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    cf* scratch = reinterpret_cast<cf*>(smem + kLdsTablesPad) + wave_id() * kPadScratchCf;
    const FftLds L = make_fft_lds(scratch, twa, w64, lane);
    const cf* hw = reinterpret_cast<const cf*>(hann) + lane;
    const cf* tsp = t1024 + lane;
    const cf* tspm = t1024 + 512 - lane;                       // split twiddles of the mirrors, [-64 r]
    // the chunk this wave works on (wave-uniform; set per drawn item)
    int s = 0, f0 = 0, f1 = 0;
    const float* sbase = src;
    float* obase = dst;
    long long gbase = 0;
    unsigned drawn = 0;                                        // lane 0: what the counter handed out
    auto draw = [&]() { if (lane == 0) drawn = atomicAdd(&work.counters[0], 1u); };
    unsigned item = blockIdx.x * kWaves + (unsigned)wave_id();
    // magnitudes of one channel: [0..3] bins lane + 64 r, [4..7] their mirrors 512 - lane - 64 r, [8] bin 256 (lane 0)
    float ma[9], mb[9];
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    float carry = 0.0f;                  // kWide: mb[4] of the frame staged last = bin 512 (lane 0) / 511 (lane 1) of its second channel
    // LDS byte offset of the wave's scratch (wave-uniform) for ds_write_addtid_b32: address = M0 + offset + 4 * lane without an address
    // VGPR — half the cycles of ds_write_b32 on gfx950 (MI355X_MICROARCH.md, LDS).  The lane-ascending halves go that way.
    const unsigned scratch_off = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)scratch);
    // stage_frame: behind a frame's second channel the scratch is idle — the magnitudes go in, in output order.
    // emit_frame: one iteration later, in the LDS round trip that fetches the window, they come back 16 bytes per lane and leave.
    auto stage_frame = [&](int fs) {
        const int phase = (int)((gbase + (long long)fs * (2 * NAE_FFT_BINS)) & 3);    // of the frame's first float, counted from dst: 0 or 2 (wave-uniform)
        float* st = reinterpret_cast<float*>(scratch) + phase;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\t"           // (an SALU write of M0 needs one wait state before an add-TID store reads it)
                     "ds_write_addtid_b32 %1\n\tds_write_addtid_b32 %2 offset:256\n\t"
                     "ds_write_addtid_b32 %3 offset:512\n\tds_write_addtid_b32 %4 offset:768\n\t"
                     "ds_write_addtid_b32 %5 offset:2052\n\tds_write_addtid_b32 %6 offset:2308\n\t"
                     "ds_write_addtid_b32 %7 offset:2564\n\tds_write_addtid_b32 %8 offset:2820"
                     :: "s"(scratch_off + 4u * (unsigned)phase), "v"(ma[0]), "v"(ma[1]), "v"(ma[2]), "v"(ma[3]),
                        "v"(mb[0]), "v"(mb[1]), "v"(mb[2]), "v"(mb[3]) : "m0", "memory");
        float* sm = st + 512 - lane;                                          // bin 512 - lane - 64 r at [-64 r]
#pragma unroll
        for (int r = 0; r < 4; r++) { sm[-64 * r] = ma[4 + r]; sm[NAE_FFT_BINS - 64 * r] = mb[4 + r]; }
        if (lane == 0) { st[256] = ma[8]; st[NAE_FFT_BINS + 256] = mb[8]; }
        if (phase != 0 && lane < 2) reinterpret_cast<float*>(scratch)[1 - lane] = carry;    // the previous frame's last 8 bytes
        carry = mb[4];
        wave_lds_sync();
    };
    auto emit_frame = [&](int fs, const u32x4 (&q)[5], bool first, bool last) {
        const int phase = (int)((gbase + (long long)fs * (2 * NAE_FFT_BINS)) & 3);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(obase + (long long)fs * (2 * NAE_FFT_BINS) - phase, 0, -1, 0x00020000);
        if (phase != 0 && first) {
            // no frame in front of this one in the wave's chunk: its first piece is only the upper 8 bytes
            if (lane == 0) __builtin_amdgcn_raw_buffer_store_b64(u32x2{q[0].z, q[0].w}, rs, 8, 0, kSpecStoreAux);
            else __builtin_amdgcn_raw_buffer_store_b128(q[0], rs, 16 * lane, 0, kSpecStoreAux);
        } else {
            __builtin_amdgcn_raw_buffer_store_b128(q[0], rs, 16 * lane, 0, kSpecStoreAux);
        }
#pragma unroll
        for (int i = 1; i < 4; i++) __builtin_amdgcn_raw_buffer_store_b128(q[i], rs, 16 * lane, 1024 * i, kSpecStoreAux);
        if (phase != 0) {
            if (lane == 0) __builtin_amdgcn_raw_buffer_store_b128(q[4], rs, 0, 4096, kSpecStoreAux);
        } else if (last) {
            if (lane == 0) __builtin_amdgcn_raw_buffer_store_b64(u32x2{q[4].x, q[4].y}, rs, 0, 4096, kSpecStoreAux);
        }
    };
    const u32x4* stq = reinterpret_cast<const u32x4*>(scratch) + lane;   // staged pieces [64 i] per lane; floats 1024..1027 lie at piece 256 of the scratch (read with a lane-independent address)
    auto store_frame = [&](int fs) {
        // buffer stores: scalar descriptor of the frame's two spectra + one lane offset (no 64-bit per-lane addresses)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(obase + ((long long)fs * 2) * NAE_FFT_BINS, 0, -1, 0x00020000);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float (&m)[9] = c == 0 ? ma : mb;
            const int co = c * NAE_FFT_BINS * 4;
#pragma unroll
            for (int r = 0; r < 4; r++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m[r]), rs, 4 * lane, co + 256 * r, kSpecStoreAux);
#pragma unroll
            for (int r = 0; r < 4; r++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m[4 + r]), rs, 1280 - 4 * lane, co + 768 - 256 * r, kSpecStoreAux);   // bin 512 - lane - 64 r
            if (lane == 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m[8]), rs, 1024, co, kSpecStoreAux);
        }
    };
    // one channel: FFT, r2c split delivering 2 X (no 1/2 factors: |2 X|^2 = 4 |X|^2 and sqrt(4 a) = 2 sqrt(a) are exact
    // scalings, so 0.5 * sqrt(.) is the canonical magnitude bit for bit, for |X| above ~1e-18), magnitudes.
    // Bins in mirror pairs: a lane computes X[k] and X[512 - k], k = lane + 64 r, r < 4, from A = Z[k] (its own register) and
    // B = Z[512 - k] (the upper half of Z, handed over through LDS: 4 + 1 writes and 4 reads instead of 8 + 1 and 8) — the
    // mirror's E and O are (Ex, -Ey) and (-Ox, Oy), exact negations and commuted sums of the canonical formula.
    auto channel = [&](cf (&v)[8], float (&mc)[9]) {
        fft512_pad(v, L);
#pragma unroll
        for (int r = 4; r < 8; r++) lds_st(L.nat + 64 * r, v[r]);
        if (lane == 0) scratch[512] = v[0];                  // the mirror of bin 0 is read like any other
        wave_lds_sync();
        cf B[4], tk[4], tm[4];
#pragma unroll
        for (int r = 0; r < 4; r++) B[r] = lds_ld(L.mir + 448 - 64 * r);
#pragma unroll
        for (int r = 0; r < 4; r++) { tk[r] = lds_ld(tsp + 64 * r); tm[r] = lds_ld(tspm - 64 * r); }
        {
            // bin 256 = its own mirror: A = B = Z[256], held by lane 0 in v[4]
            const cf z = v[4];
            const cf E = cf{z.x + z.x, z.y - z.y};
            const cf O = cf{z.x - z.x, z.y + z.y};
            const cf P = cmul_tw(O, t1024[256]);
            const cf X = cf{E.x + P.y, E.y - P.x};
            mc[8] = 0.5f * sqrt_rn(X.x * X.x + X.y * X.y);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const cf A = v[r];
            const cf E = cf{A.x + B[r].x, A.y - B[r].y};
            const cf O = cf{A.x - B[r].x, A.y + B[r].y};
            const cf P = cmul_tw(O, tk[r]);
            const cf X = cf{E.x + P.y, E.y - P.x};
            mc[r] = 0.5f * sqrt_rn(X.x * X.x + X.y * X.y);
            const cf Pm = cmul_tw(cf{-O.x, O.y}, tm[r]);
            const cf Xm = cf{E.x + Pm.y, -E.y - Pm.x};
            mc[4 + r] = 0.5f * sqrt_rn(Xm.x * Xm.x + Xm.y * Xm.y);
        }
        wave_lds_sync();
    };
    // consecutive frames overlap by 768 of 1024 sample-frames = 6 of the 8 rows of the FFT input layout (pair index
    // n = lane + 64 j, hop = 128 pairs = 2 rows): the raw samples stay in registers and a frame loads only its last 2 rows,
    // so every input byte is read once
#pragma unroll 1
    for (;;) {
    if (item >= work.n_items) break;
    {
        // (the divisions run on the vector ALU once per chunk: bring the wave-uniform results back to scalar registers)
        unsigned sv, kv;
        int ck;
        if (item < work.n_coarse) { sv = item / work.cps_c; kv = item - sv * work.cps_c; ck = work.chunk_c; }
        else { const unsigned j = item - work.n_coarse; const unsigned q = j / work.cps_f; sv = work.coarse_streams + q; kv = j - q * work.cps_f; ck = work.chunk_f; }
        s = __builtin_amdgcn_readfirstlane((int)sv);
        const int chunk = __builtin_amdgcn_readfirstlane(ck);
        f0 = __builtin_amdgcn_readfirstlane((int)kv) * chunk;
        f1 = f0 + chunk > (int)n_frames ? (int)n_frames : f0 + chunk;
        sbase = src + (long long)s * src_ss + 4 * lane;            // frames lie fully inside [0, T) by construction
        obase = dst + (long long)s * dst_ss;
        gbase = (long long)s * dst_ss;
    }
    float4 raw[8], pre[2];
    if (f0 < f1) {
        const float* base = sbase + 2 * ((long long)f0 * NAE_HOP);
#pragma unroll
        for (int j = 0; j < 8; j++) raw[j] = *reinterpret_cast<const float4*>(base + 256 * j);
    }
    if (work.dynamic) draw();                                      // the next item: its latency hides behind this chunk
#pragma unroll 1
    for (int f = f0; f < f1; f++) {
        cf v0[8], v1[8];
        u32x4 q[5];
        if (kWide && f > f0) {
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = stq[64 * i];
            q[4] = reinterpret_cast<const u32x4*>(scratch)[256];   // every lane reads the SAME 16 bytes (inside the wave's scratch); lane 0's copy is stored
        }
        if (kWide && f > f0) {
            emit_frame(f - 1, q, f - 1 == f0, false);
            __builtin_amdgcn_sched_barrier(0);
        }
        cf w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = lds_ld(hw + 64 * j);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            v0[j] = cf{raw[j].x * w[j].x, raw[j].z * w[j].y};
            v1[j] = cf{raw[j].y * w[j].x, raw[j].w * w[j].y};
        }
        if (!kWide && f > f0) store_frame(f - 1);
        if (f + 1 < f1) {
            const float* base = sbase + 2 * ((long long)(f + 1) * NAE_HOP);
            pre[0] = *reinterpret_cast<const float4*>(base + 256 * 6);
            pre[1] = *reinterpret_cast<const float4*>(base + 256 * 7);
        }
        channel(v0, ma);
        __builtin_amdgcn_sched_barrier(0);      // keep the two channels apart: interleaved, their live values exceed the register budget
        channel(v1, mb);
        __builtin_amdgcn_sched_barrier(0);
        if (kWide) stage_frame(f);
#pragma unroll
        for (int j = 0; j < 6; j++) raw[j] = raw[j + 2];
        raw[6] = pre[0];
        raw[7] = pre[1];
    }
    if (f1 > f0) {
        if (kWide) {
            u32x4 q[5];
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] = stq[64 * i];
            q[4] = reinterpret_cast<const u32x4*>(scratch)[256];   // every lane reads the SAME 16 bytes (inside the wave's scratch); lane 0's copy is stored
            emit_frame(f1 - 1, q, f1 - 1 == f0, true);
            wave_lds_sync();
        }
        else store_frame(f1 - 1);
    }
    if (!work.dynamic) break;
    item = work.n_waves + (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
    }   // next chunk
}

// ------------------------------------------------------------------------------------------------ every size
// The canonical FFT of DESIGN.md §3 ("K8 spectrum, every size"): fft_any.h.
//
// Mapping: one wave = G = max(1, 512/M) consecutive frames of one (stream, channel); a 512-thread workgroup is 8 such waves that
// share only the W512 table in LDS; the first pass reads the windowed samples from memory.  LDS: 4 KiB + 8 x 9/8 x 512 x 8 B (n_fft <= 1024) ... 8 x 18 KiB
// (4096): 151 552 B (148 KiB) at 4096 = one workgroup, 2 waves per SIMD.  Hann_N and the split twiddles T_N are read through the caches
// (each element once per frame, coalesced); the first pass of M = 1024 / 2048 reads W_M likewise.
// Input reuse: a wave reads each of its frames' samples once; consecutive frames of a stream sit in neighbouring waves of one
// workgroup, so with hop < n_fft the shared samples are served by L2, not HBM.

constexpr int kAnyWaves = 8;
constexpr int kAnyThreads = 64 * kAnyWaves;

// item = (stream, channel, group of G consecutive frames), one per wave; consecutive items = consecutive frame groups of one stream-channel
template <int N, int kLoad>
__global__ __launch_bounds__(kAnyThreads) void spectrum_any_kernel(SigViewD src, int ch, long long hop, long long n_frames,
                                                                   long long n_groups, long long item0, long long n_items,
                                                                   float* __restrict__ dst, long long dst_ss, SpecAnyTables tb)
{
    using Gm = SpecGeom<N>;
    __shared__ __attribute__((aligned(16))) cf w512l[512];
    __shared__ __attribute__((aligned(16))) cf scratch[kAnyWaves * Gm::SCR];
    for (int i = threadIdx.x; i < 512; i += kAnyThreads) w512l[i] = tb.w512[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long item = item0 + (long long)blockIdx.x * kAnyWaves + wave_id();
    if (item >= n_items) return;
    cf* scr = scratch + wave_id() * Gm::SCR;
    const long long sc = item / n_groups, grp = item - sc * n_groups;
    const long long s = sc / ch;
    const int c = (int)(sc - s * ch);
    const long long f0 = grp * Gm::G;
    const int nvalid = (int)((n_frames - f0) < Gm::G ? (n_frames - f0) : Gm::G);
    const ChanView in{src.base + s * src.ss + c * src.cs, src.fs, 0};

    any_first_pass<Gm, kLoad>(scr, w512l, tb, in, f0 * hop, hop, nvalid, lane);
    any_passes8<Gm, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();

    // r2c split and magnitudes: output element o = g (M+1) + k, consecutive lanes -> consecutive addresses of one record
    float* out = dst + s * dst_ss + (f0 * ch + c) * (long long)Gm::BINS;
    constexpr int kOut = Gm::G * Gm::BINS;
#pragma unroll 4
    for (int o = lane; o < kOut; o += 64) {
        const int g = o / Gm::BINS, k = o - g * Gm::BINS;
        if (g >= nvalid) break;
        const cf* zf = scr + g * Gm::M + ((g * Gm::M) >> 3);       // padx(g M + p) = padx(g M) + padx(p): M is a multiple of 8
        const cf X = any_rfft_bin<Gm>(zf, tb.tn, k);
        out[(unsigned)(g * ch * Gm::BINS + k)] = __builtin_sqrtf(X.x * X.x + X.y * X.y);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// frames per wave of the stereo spectrum kernel.  A CU holds 16 of its waves; with many rounds of waves the tail of the last
// round does not matter and 32 frames keep the waves short.  A small batch (an eighth of the C5 job is 1.8 rounds at 32) gets
// the chunk that fills a whole number of rounds: waves <= rounds x slots, the fewest frames per slot over the launch.
static int spec_pick_chunk(long long frames, long long n_streams, int n_cu)
{
    const long long slots = (long long)n_cu * 16;
    const long long waves32 = ((frames + kSpecChunk - 1) / kSpecChunk) * n_streams;
    if (waves32 >= 8 * slots || n_streams > slots) return kSpecChunk;
    long long best_chunk = kSpecChunk, best_cost = ((waves32 + slots - 1) / slots) * kSpecChunk;
    for (long long rounds = 1; rounds <= 8; rounds++) {
        const long long per_stream = rounds * slots / n_streams;            // chunks a stream may be cut into
        if (per_stream < 1) continue;
        long long chunk = (frames + per_stream - 1) / per_stream;
        if (chunk < 8) chunk = 8;
        if (chunk > 128) continue;                                           // (longer waves were not measured)
        const long long waves = ((frames + chunk - 1) / chunk) * n_streams;
        const long long cost = ((waves + slots - 1) / slots) * chunk;       // frames a slot walks over the launch
        if (cost < best_cost) { best_cost = cost; best_chunk = chunk; }
    }
    return (int)best_chunk;
}

// the tables of a size for the size-generic kernels (the spectrum's, the vocoder's, the filters'): built at the size's first call
int nae_spec_any_tables(nae_ctx* ctx, int n_fft, SpecAnyTables* tb)
{
    const int rc = nae_fft_tab_ensure(ctx, n_fft);
    if (rc) return rc;
    const nae_fft_tab t = nae_fft_tab_of(ctx, n_fft);
    *tb = SpecAnyTables{t.hann, t.tn, t.wm, nae_fft_tab_of(ctx, NAE_FFT_N).wm};
    return NAE_OK;
}

template <int N, int kLoad>
static int launch_any_as(nae_ctx* ctx, const SigViewD& v, int ch, long long hop, long long F, long long n_groups, long long items,
                         float* dst, size_t dst_stream_stride, const SpecAnyTables& tb)
{
    // one item per wave (measured faster than waves walking items from a grid of 8 workgroups per CU: profiles/r07_spec_sizes.md);
    // a launch holds at most 2^22 workgroups (grid x block < 2^32 work-items), longer jobs take several
    constexpr long long kMaxItems = (1ll << 22) * kAnyWaves;
    for (long long item0 = 0; item0 < items; item0 += kMaxItems) {
        const long long n = items - item0 < kMaxItems ? items - item0 : kMaxItems;
        const int rc = nae_launch_tiles(ctx, "spectrum_any_kernel", "spectrum_any_kernel: grid too large", spectrum_any_kernel<N, kLoad>, n, kAnyWaves,
                                        kAnyThreads, 0, v, ch, hop, F, n_groups, item0, items, dst, (long long)dst_stream_stride, tb);
        if (rc) return rc;
    }
    return NAE_OK;
}

template <int N>
static int launch_any(nae_ctx* ctx, const nae_sig* src, int ch, long long hop, long long F, size_t n_streams, float* dst,
                      size_t dst_stream_stride, const SpecAnyTables& tb)
{
    constexpr int G = SpecGeom<N>::G;
    const long long n_groups = (F + G - 1) / G;
    const long long items = n_groups * (long long)n_streams * ch;
    const SigViewD v = to_view(src);
    if (src->frame_stride == 1) return launch_any_as<N, kLoadUnit>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
    if ((unsigned long long)src->frame_stride * N < (1ull << 31))
        return launch_any_as<N, kLoadStride32>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
    return launch_any_as<N, kLoadStride64>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
}

} // namespace nae

using namespace nae;

// Hann_N, T_N and W_M of one size (the layout: nae_internal.h): double, one rounding to f32, one upload
int nae_fft_tab_ensure(nae_ctx* ctx, int n_fft)
{
    CtxBuf& t = ctx->fft_tab[ilog2c(n_fft) - 8];
    if (t.p) return NAE_OK;
    const int M = n_fft / 2;
    const double two_pi = 6.283185307179586476925286766559;
    std::vector<char> img(nae_fft_tab_bytes(n_fft), 0);
    float* hann = reinterpret_cast<float*>(img.data());
    cf* tn = reinterpret_cast<cf*>(img.data() + nae_fft_tab_tn(n_fft));
    cf* wm = reinterpret_cast<cf*>(img.data() + nae_fft_tab_wm(n_fft));
    for (int n = 0; n < n_fft; n++) hann[n] = (float)(0.5 - 0.5 * cos(two_pi * n / (double)n_fft));
    for (int k = 0; k <= M; k++) tn[k] = cf{(float)cos(two_pi * k / (double)n_fft), (float)(-sin(two_pi * k / (double)n_fft))};
    for (int k = 0; k < M; k++) wm[k] = cf{(float)cos(two_pi * k / (double)M), (float)(-sin(two_pi * k / (double)M))};
    int rc = t.reserve(ctx, img.size(), "spectrum tables");
    if (!rc) rc = nae_check(ctx, hipMemcpy(t.p, img.data(), img.size(), hipMemcpyHostToDevice), "hipMemcpy(spectrum tables)");
    if (rc) t.release();
    return rc;
}

// the one spectrum launcher (arguments checked by nae_spectrum_block_ex_f32): the size-generic kernel for every size and hop
// but 1024 / 256 (and for that under spec_any), else the stereo kernel for an aligned interleaved-stereo source (unless
// spec_generic), else the generic 1024-point kernel
int nae_launch_spectrum(nae_ctx* ctx, int n_fft, int hop, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                        size_t dst_stream_stride)
{
    const size_t F = nae_spectrum_frames_ex(T, n_fft, hop);
    if (F == 0 || n_streams == 0) return NAE_OK;
    if (n_fft != NAE_FFT_N || hop != NAE_HOP || ctx->dbg_spec_any) {
        SpecAnyTables tb;
        const int rc = nae_spec_any_tables(ctx, n_fft, &tb);
        if (rc) return rc;
        return pick_value<256, 512, 1024, 2048, 4096>(ctx, n_fft, "spectrum: n_fft must be a power of two in [256, 4096]", [&](auto n) {   // (callers check first)
            return launch_any<decltype(n)::value>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb);
        });
    }
    const long long items = (long long)(F * n_streams);
    const Tables tb = tables_1024(ctx);
    const bool stereo_fast = ch == 2 && src->chan_stride == 1 && src->frame_stride == 2 && src->stream_stride % 4 == 0 &&
                             (reinterpret_cast<uintptr_t>(src->base) & 15) == 0 && !ctx->dbg_spec_generic;
    if (stereo_fast) {
        const long long slots = (long long)ctx->n_cu * 16;                   // waves a launch keeps resident (two workgroups per CU)
        SpecWork w{};
        w.counters = ctx->spec_ctr.as<unsigned>();
        const long long coarse_all = (((long long)F + kSpecChunk - 1) / kSpecChunk) * (long long)n_streams;
        if (coarse_all < 6 * slots) {
            // small batch: one list of equal chunks, sized so that the waves fill a whole number of rounds
            w.chunk_c = ctx->dbg_spec_chunk > 0 ? ctx->dbg_spec_chunk : spec_pick_chunk((long long)F, (long long)n_streams, ctx->n_cu);
            w.cps_c = (unsigned)(((long long)F + w.chunk_c - 1) / w.chunk_c);
            w.coarse_streams = (unsigned)n_streams;
            w.chunk_f = w.chunk_c;
            w.cps_f = w.cps_c;
        } else {
            // large batch: 16-frame chunks, and 8-frame chunks for the last streams — about four short chunks per resident wave, at most an
            // eighth of the job — so that the launch ends within one short chunk
            w.chunk_c = ctx->dbg_spec_chunk > 0 ? ctx->dbg_spec_chunk : kSpecChunkLarge;
            w.cps_c = (unsigned)(((long long)F + w.chunk_c - 1) / w.chunk_c);
            w.chunk_f = ctx->dbg_spec_fine > 0 ? ctx->dbg_spec_fine : kSpecChunkFine;
            w.cps_f = (unsigned)(((long long)F + w.chunk_f - 1) / w.chunk_f);
            long long fine_streams = ((ctx->dbg_spec_fine_rounds > 0 ? ctx->dbg_spec_fine_rounds : 4) * slots + w.cps_f - 1) / w.cps_f;
            if (fine_streams > (long long)n_streams / 8) fine_streams = (long long)n_streams / 8;
            w.coarse_streams = (unsigned)((long long)n_streams - fine_streams);
        }
        const long long n_coarse = (long long)w.coarse_streams * w.cps_c;
        const long long items = n_coarse + ((long long)n_streams - w.coarse_streams) * w.cps_f;
        if (items > 0x7fffffffll) return nae_fail(ctx, NAE_ERR_INVALID, "spectrum_stereo_kernel: too many chunks");
        w.n_coarse = (unsigned)n_coarse;
        w.n_items = (unsigned)items;
        long long groups = (items + kWaves - 1) / kWaves;
        if (groups > 2ll * ctx->n_cu) groups = 2ll * ctx->n_cu;
        w.n_waves = (unsigned)(groups * kWaves);
        w.dynamic = items > groups * kWaves ? 1u : 0u;
        if (w.dynamic) {
            (void)nae_use_device(ctx);
            const hipError_t e = hipMemsetAsync(ctx->spec_ctr.p, 0, sizeof(unsigned), ctx->stream);
            if (e != hipSuccess) return nae_check(ctx, e, "hipMemsetAsync(spectrum work counter)");
        }
        const bool wide = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 && dst_stream_stride % 2 == 0 && !ctx->dbg_spec_narrow;
        return with_flags(wide, [&](auto wd) {
            return nae_launch_grid(ctx, "spectrum_stereo_kernel", spectrum_stereo_kernel<wd.value>, dim3((unsigned)groups), dim3(kThreads), kLdsSpec,
                                   static_cast<const float*>(src->base), (long long)src->stream_stride, (long long)F, w, dst,
                                   (long long)dst_stream_stride, tb);
        });
    }
    return with_flags(src->frame_stride == 1, [&](auto unit) {
        return nae_launch_tiles(ctx, "spectrum_kernel", "spectrum_kernel: grid too large", spectrum_kernel<unit.value>, items, kWaves, kThreads,
                                kLdsSpec, to_view(src), (long long)T, ch, (long long)F, items, dst, (long long)dst_stream_stride, tb);
    });
}
