// kernels_stft.hip — K7 tempo/pitch: the phase vocoder's pass 1 at 1024 points (pv_phase_kernel) and the vocoder's host driver (workspace, the
// job record, nae_launch_pv_phase, nae_launch_pv_synth) for gfx950.  The rate transposer is kernels_resample.hip, the K8 spectrum kernels_spectrum.hip.
//
// Mapping (MI355X: 256 CUs x 4 SIMD, wave64, 160 KiB LDS/CU):
//   * one wavefront = one (stream, channel, tile of frames); a 512-thread workgroup is 8 independent waves
//     that only share the read-only Hann / split-twiddle tables in LDS (one __syncthreads after the table
//     fill, none afterwards).
//   * the phase accumulator is Q0.32 integer, so the time recurrence of the vocoder is an exact prefix sum:
//     pass 1 (pv_phase_kernel) reduces each tile's phase increments, pass 2 (pv_scan_kernel, kernels_pv_any.hip) scans tiles,
//     pass 3 (kernels_pvpipe.hip) recomputes the tile with the right starting phase and overlap-adds in registers.
//     HBM traffic stays at the algorithmic 4 B in + 4 B out per sample per channel (+ one re-read in pass 1).
//
// Replaces: SoundTouch behind /root/reference/src/processor/audio-velocity.cpp:369-428 (algorithm differs,
// see DESIGN.md §3).
#include "stft_common.h"
#include <stdlib.h>

namespace nae {

// ------------------------------------------------------------------------------------------------ K7
// pass 1: per-tile sum of phase increments.  sums[(sc * n_tiles + tile) * 520 + k]
// One wave per tile on the padded low-register FFT (stft_device.h; round 5 — rounds 1-4 ran the 100-VGPR swizzled FFT at four waves per SIMD): 80 VGPRs,
// three 8-wave workgroups per CU = six waves per SIMD, which is what the LDS allows (12 KB of tables + 8 x 4.5 KB of scratch per workgroup).
constexpr size_t kLdsPhase = kLdsTablesPad + kWaves * kPadScratchCf * sizeof(cf);
static_assert(3 * kLdsPhase <= 160 * 1024, "three workgroups per CU");
template <bool kUnit>
__global__ __launch_bounds__(kThreads, 6) void pv_phase_kernel(SigViewD src, PvParams p, long long n_items,
                                                              uint32_t* __restrict__ sums, Tables tb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* hann; cf *t1024, *w64, *twa;
    stage_tables(smem, tb, kThreads, hann, t1024, w64, twa);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    cf* scratch = reinterpret_cast<cf*>(smem + kLdsTablesPad) + wave_id() * kPadScratchCf;
    const long long item = (long long)blockIdx.x * kWaves + wave_id();
    if (item >= n_items) return;
    const WaveTile w = wave_tile(item, p.n_tiles, p.ch);
    const long long s_idx = w.s_idx;
    const int tile = w.tile, c = w.c;
    if (tile >= p.skip_from) return;                    // wave-uniform
    ChanView in{src.base + s_idx * src.ss + c * src.cs, src.fs, p.in_len};
    const int kl = kl_of_lane(lane);

    const long long f0 = p.f_origin + (long long)tile * p.tile;
    long long f1 = f0 + p.tile;
    if (f1 > p.f_stop) f1 = p.f_stop;

    uint32_t acc[9], qp[9], qa[9];
#pragma unroll
    for (int r = 0; r < 9; r++) { acc[r] = 0; qp[r] = 0; }
    cf v[8];
    long long s_prev = 0;
    // one analysis call site: frame f0-1 only primes qp (its increment belongs to the previous tile)
#pragma unroll 1
    for (long long f = (f0 > 0 ? f0 - 1 : 0); f < f1; f++) {
        const long long s = frame_start(p, f);
        load_frame_windowed<kUnit>(v, in, s, hann, lane);
        fft512_pad(v, make_fft_lds(scratch, twa, w64, lane));
        const cf nyq = rfft_split<true>(v, scratch, t1024, lane);   // 2 X: only phases are taken from it
        phases_of(v, nyq, qa);
        if (f < f0) {
            // priming frame: its increment belongs to the previous tile / call
        } else if (f == 0) {
#pragma unroll
            for (int r = 0; r < 9; r++) acc[r] = qa[r]; // the "increment" of frame 0 is its analysis phase
        } else {
            const unsigned d = (unsigned)(s - s_prev);
            const unsigned R = (d == (unsigned)p.d0) ? p.r_q24_0 : p.r_q24_1;
            phase_inc(qa, qp, acc, kl, d, R);
        }
#pragma unroll
        for (int r = 0; r < 9; r++) qp[r] = qa[r];
        s_prev = s;
    }
    uint32_t* o = sums + item * kT1024Pad;
#pragma unroll
    for (int r = 0; r < 8; r++) o[kl + 64 * r] = acc[r];
    if (lane == 0) o[512] = acc[8];
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// records [n_sc][n_tiles][nae_pv_record_pad(n_fft)] uint32 (the exclusive tile-prefix phases; 520 per record at 1024); locked (1024 only), then
// the tile maps: c [n_sc][n_tiles][520] uint32, sigma [n_sc][n_tiles][520] uint16
size_t nae_pv_workspace_bytes(bool lock, int n_fft, size_t n_frames, int ch, size_t n_streams, int tile)
{
    const size_t recs = n_streams * ch * ((n_frames + tile - 1) / tile);
    return recs * nae_pv_record_pad(n_fft) * (lock ? 2 * sizeof(uint32_t) + sizeof(uint16_t) : sizeof(uint32_t));
}

// the context's phase workspace for a call of n_frames frames in pass-1 tiles of `tile`; the envelope pass (a forced plan) has none
int nae_pv_reserve_ws(nae_ctx* ctx, const nae_pv_run& r, size_t n_frames, int ch, size_t n_streams, int tile)
{
    if (r.forced) return NAE_OK;
    return ctx->ws_phase.reserve(ctx, nae_pv_workspace_bytes(r.lock, r.n_fft, n_frames, ch, n_streams, tile), "workspace");
}

// what both passes hand their leaf launchers (pass 1: no output)
static PvJob make_pv_job(const nae_pv_run& r, const nae_stretch_plan& pl, const nae_sig* src, size_t in_len, int ch, size_t n_streams, int tile,
                         const nae_pv_segment* seg, uint32_t* phase_ws, const nae_sig* out)
{
    return PvJob{r.n_fft, make_pv_params(pl, in_len, ch, tile, seg), to_view(src), out ? to_out(out) : OutViewD{}, (long long)n_streams * ch,
                 src->frame_stride == 1, phase_ws, r.lifter, r.g, r.transients, r.link};
}

// pass 1 + 2: leaves the exclusive tile-prefix phases in `phase_ws` (one record per pass-1 tile).
// Pass 1 may use shorter tiles than pass 3 (`synth_tile` = a multiple of `tile`): its waves are independent, so short
// tiles keep the chip full on small batches, while pass 3 wants few long tiles (each re-analyses its frames).
// Only the sums (locked: maps) in front of the last synthesis tile are needed, unless the phase behind the segment is carried on (a
// continued stream): nothing at all when the stream-channel is a single synthesis tile.
// Pass 1 as nae_pv_route_of says; unlocked, either pass 1 is followed by the one scan (pv_scan_kernel, kernels_pv_any.hip).
int nae_launch_pv_phase(nae_ctx* ctx, const nae_pv_run& r, const nae_stretch_plan* pl, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                        int tile, int synth_tile, uint32_t* phase_ws, const nae_pv_segment* seg)
{
    if (tile <= 0 || synth_tile < tile || synth_tile % tile) return nae_fail(ctx, NAE_ERR_INVALID, "phase tile must divide the synthesis tile");
    if (r.forced) return NAE_OK;   // the envelope pass carries no phase
    PvJob j = make_pv_job(r, *pl, src, in_len, ch, n_streams, tile, seg, phase_ws, nullptr);
    PvParams& p = j.p;
    const long long n_sc = j.n_sc;
    if (n_sc * p.n_tiles == 0) return NAE_OK;
    const bool need_last = seg && seg->carry_out && !seg->carry_by_synth;
    const int step = synth_tile / tile;
    const int n_synth = (p.n_tiles + step - 1) / step;
    const int n_needed = need_last ? p.n_tiles : (n_synth - 1) * step;      // sums (maps) of tiles [0, n_needed) are used
    const uint32_t* carry_in = seg ? seg->carry_in : nullptr;
    uint32_t* carry_out = seg ? seg->carry_out : nullptr;
    const size_t pad = nae_pv_record_pad(r.n_fft);
    if (n_needed == 0) {
        // base phase of the only synthesis tile (record 0 of each stream-channel): the carried phase, or zero
        hipError_t e = hipSuccess;
        if (!carry_in) {
            // nothing carried in and a single synthesis tile: pass 3 starts from zero by itself (PvParams::base_zero) — no memset launch
            if (p.n_tiles != 1) e = hipMemsetAsync(phase_ws, 0, (size_t)n_sc * p.n_tiles * pad * sizeof(uint32_t), ctx->stream);
        }
        else if (p.n_tiles == 1)
            e = hipMemcpyAsync(phase_ws, carry_in, (size_t)n_sc * pad * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream);
        else
            e = hipMemcpy2DAsync(phase_ws, (size_t)p.n_tiles * pad * sizeof(uint32_t), carry_in, pad * sizeof(uint32_t),
                                 pad * sizeof(uint32_t), (size_t)n_sc, hipMemcpyDeviceToDevice, ctx->stream);
        return nae_check(ctx, e, "phase base init");
    }
    p.skip_from = n_needed;                   // pass 1 skips the tiles whose sums are not needed
    const PvKernels pass1 = nae_pv_route_of(ctx, r).pass1;
    if (pass1 == PvKernels::kLock) {
        const size_t n_rec = (size_t)n_sc * p.n_tiles;
        uint32_t* maps = phase_ws + n_rec * kT1024Pad;
        uint16_t* sig16 = reinterpret_cast<uint16_t*>(maps + n_rec * kT1024Pad);
        return nae_launch_pvlock_phase(ctx, j, n_needed, maps, sig16, carry_in, carry_out);
    }
    if (pass1 == PvKernels::kAny) {
        const int rc = nae_launch_pvany_phase(ctx, j);
        if (rc) return rc;
    } else {
        // items are (stream-channel, tile) with tile fastest
        const long long items = n_sc * p.n_tiles;
        const Tables tb = tables_1024(ctx);
        const int rc = with_flags(j.unit_stride, [&](auto unit) {
            return nae_launch_tiles(ctx, "pv_phase_kernel", "pv_phase_kernel: grid too large", pv_phase_kernel<unit.value>, items, kWaves, kThreads,
                                    kLdsPhase, j.src, p, items, phase_ws, tb);
        });
        if (rc) return rc;
    }
    return nae_launch_pv_scan(ctx, r.n_fft, pass1 == PvKernels::kAny ? "pv_any_scan_kernel" : "pv_scan_kernel", phase_ws, n_sc, p.n_tiles, carry_in,
                              carry_out, n_needed, r.transients);
}

// pass 3 (locked: L3) from the records of pass 2 (or, one tile and nothing carried in, from zero), on the kernels nae_pv_route_of says; r.lifter > 0:
// formant preservation, or with a formant ratio other than 1 the formant shift; a forced plan runs the envelope pass alone
int nae_launch_pv_synth(nae_ctx* ctx, const nae_pv_run& r, const nae_stretch_plan* pl, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                        int tile, int phase_tile, uint32_t* phase_ws, const nae_sig* out, const nae_pv_segment* seg, int frames_per_step)
{
    if (phase_tile <= 0 || tile < phase_tile || tile % phase_tile) return nae_fail(ctx, NAE_ERR_INVALID, "phase tile must divide the synthesis tile");
    PvJob j = make_pv_job(r, *pl, src, in_len, ch, n_streams, tile, seg, phase_ws, out);
    PvParams& p = j.p;
    const long long cnt = p.f_stop - p.f_origin;
    p.phase_step = tile / phase_tile;
    p.phase_tiles = (int)((cnt + phase_tile - 1) / phase_tile);
    p.base_zero = (p.n_tiles == 1 && p.phase_tiles == 1 && !(seg && seg->carry_in)) ? 1 : 0;
    if (seg && seg->carry_by_synth && seg->carry_out) {
        if (p.n_tiles != 1) return nae_fail(ctx, NAE_ERR_INVALID, "carry_by_synth needs a single synthesis tile");
        p.carry_out = seg->carry_out;
        p.carry_frame = p.f_stop - 1;
    }
    const PvKernels pass3 = nae_pv_route_of(ctx, r).pass3;
    if (pass3 == PvKernels::kEnv) return nae_launch_pvenv(ctx, j);
    if (pass3 == PvKernels::kLock) return nae_launch_pvlock_synth(ctx, j);
    if (pass3 == PvKernels::kAny) return nae_launch_pvany_synth(ctx, j);
    return nae_launch_pv_pipe(ctx, j, frames_per_step);
}

