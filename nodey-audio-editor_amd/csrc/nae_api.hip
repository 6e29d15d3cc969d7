// nae_api.hip — context, plumbing, and the host-side orchestration of K7/K8 behind the C ABI (include/nae_gpu.h).
// No CPU compute path exists in this library: every transform is a HIP kernel launch; if HIP is unusable the
// entry points fail with NAE_ERR_HIP.
#include "nae_internal.h"
#include <string>
#include <initializer_list>
#include <cmath>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

int nae_fail(nae_ctx* ctx, int code, const char* what)
{
    if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s", what);
    return code;
}

int nae_check(nae_ctx* ctx, hipError_t e, const char* what)
{
    if (e == hipSuccess) return NAE_OK;
    if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, hipGetErrorString(e));
    return NAE_ERR_HIP;
}

NaeProfScope::NaeProfScope(nae_ctx* c, const char* name) : ctx(c), idx(-1)
{
    if (!c || !c->prof_on) return;
    int slot = -1;
    for (size_t i = 0; i < c->prof_slots.size(); i++)
        if (c->prof_slots[i].name == name || !strcmp(c->prof_slots[i].name, name)) { slot = (int)i; break; }
    if (slot < 0) { c->prof_slots.push_back({name, 0.0, 0}); slot = (int)c->prof_slots.size() - 1; }
    nae_ctx::ProfPair pp{slot, nullptr, nullptr};
    if (hipEventCreate(&pp.a) != hipSuccess || hipEventCreate(&pp.b) != hipSuccess) return;
    (void)hipEventRecord(pp.a, c->stream);
    c->prof_pairs.push_back(pp);
    idx = (int)c->prof_pairs.size() - 1;
}
NaeProfScope::~NaeProfScope()
{
    if (idx >= 0) (void)hipEventRecord(ctx->prof_pairs[idx].b, ctx->stream);
}

static void prof_collect(nae_ctx* ctx)
{
    if (ctx->prof_pairs.empty()) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& pp : ctx->prof_pairs) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, pp.a, pp.b) == hipSuccess) {
            ctx->prof_slots[pp.slot].total_ms += ms;
            ctx->prof_slots[pp.slot].launches += 1;
        }
        (void)hipEventDestroy(pp.a);
        (void)hipEventDestroy(pp.b);
    }
    ctx->prof_pairs.clear();
}

int nae_ctx_drain(nae_ctx* ctx)
{
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

double nae_bessel_i0(double x)
{
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 64; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static void build_rs_table(double rate_eff, std::vector<float>& tab)
{
    const double pi = 3.14159265358979323846;
    const double c = NAE_RS_CUTOFF * (rate_eff > 1.0 ? 1.0 / rate_eff : 1.0);
    const double half = NAE_RS_TAPS / 2.0;
    const double i0b = nae_bessel_i0(NAE_RS_KAISER_BETA);
    tab.resize((NAE_RS_PHASES + 1) * NAE_RS_TAPS);
    for (int p = 0; p <= NAE_RS_PHASES; p++) {
        double row[NAE_RS_TAPS], sum = 0.0;
        for (int i = 0; i < NAE_RS_TAPS; i++) {
            const double x = (double)(i - (NAE_RS_TAPS / 2 - 1)) - (double)p / NAE_RS_PHASES;
            const double a = x / half;
            double w = 0.0;
            if (a > -1.0 && a < 1.0) w = nae_bessel_i0(NAE_RS_KAISER_BETA * sqrt(1.0 - a * a)) / i0b;
            else if (a == 1.0 || a == -1.0) w = 1.0 / i0b;
            const double arg = pi * c * x;
            const double sinc = (fabs(arg) < 1e-12) ? 1.0 : sin(arg) / arg;
            row[i] = c * sinc * w;
            sum += row[i];
        }
        for (int i = 0; i < NAE_RS_TAPS; i++) tab[p * NAE_RS_TAPS + i] = (float)(row[i] / sum);
    }
}

int nae_ensure_rs_table(nae_ctx* ctx, double rate_eff)
{
    return ctx->rs_tab.get(ctx, {}, &rate_eff, sizeof rate_eff, (NAE_RS_PHASES + 1) * NAE_RS_TAPS * sizeof(float), "rs table", [&] {
        std::vector<float> tab;
        build_rs_table(rate_eff, tab);
        return nae_check(ctx, hipMemcpy(ctx->rs_tab.as<float>(), tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(rs table)");
    });
}

// Shape of the phase vocoder for a block call: frames per step of the pipeline (kernels_pvpipe.hip), synthesis tile, pass-1 tile.
//   * more than 3 stream-channels per CU (>= 1024 at 256 CUs, e.g. 512 stereo streams): four stream-channels per workgroup
//     (frames_per_step 1), ONE tile per stream-channel — no pass 1, nothing analysed twice; from 2048 stream-channels two
//     workgroups share a CU; up to 1024 stream-channels (one workgroup per CU) the launch runs the one-barrier schedule (pv_flow_kernel).
//     (2 to 3 per CU: the frame-interleaved shape below in three rounds, see the code.)
//   * fewer: the four slots of a workgroup work on 2 or 4 consecutive frames of one stream-channel (frame-interleaved), so
//     256 stream-channels (the 128 streams one rank of an 8-GPU job owns) still give every CU a workgroup without cutting
//     a stream into time tiles.  A workgroup of these modes fills a CU's LDS alone: 4 frames per step up to n_cu
//     stream-channels, 2 frames per step up to 2 n_cu.
//   * fewer stream-channels than CUs: time tiles on top (each tile but the last of a stream-channel is analysed twice: pass 1
//     sums its phase increments, pass 3 synthesises it), just enough of them for one workgroup per CU.  Pass 1 is one wave per
//     tile and wants 24 n_cu waves (six per SIMD): it runs on tiles `step` times shorter (*phase_tile), never shorter than 64 frames; the
//     synthesis tile is a multiple of it.
int nae_pick_pv_shape(nae_ctx* ctx, size_t frames, size_t n_sc, int* phase_tile, int* frames_per_step)
{
    const size_t n_cu = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    int fps = n_sc > 2 * n_cu ? 1 : n_sc > n_cu ? 2 : 4;
    // between 2 and 3 stream-channels per CU four stream-channels per workgroup leave a quarter to a half of the CUs without a
    // workgroup; three rounds of four-frames-per-step workgroups are faster there (profiles/r04_shape_sweep.md: 768 stream-channels
    // 3.28 against 3.65 ms, 520: 3.21 against 3.35; at 1024 stream-channels one full round of the first shape wins again)
    if (n_sc > 2 * n_cu && n_sc <= 3 * n_cu) fps = 4;
    if (ctx->pv_fps == 1 || ctx->pv_fps == 2 || ctx->pv_fps == 4) fps = ctx->pv_fps;
    *frames_per_step = fps;
    if (ctx->pv_tile > 0) { *phase_tile = ctx->pv_tile; return ctx->pv_tile; }
    *phase_tile = 64;
    if (frames == 0 || n_sc == 0) return 64;
    // Few LONG stream-channels — at most half as many as CUs, where the frame-interleaved shape below needs time tiles and pass 1 anyway: cut them into as
    // many tiles as the FULL-batch shape wants — one frame per step, 8 n_cu (stream-channel, tile) items = two workgroups per CU at eight waves per SIMD, 1.37x
    // the frames per second of the frame-interleaved shape — when a tile keeps >= 128 frames (its 4 priming / tail frames then cost <= 3 %).  One hour of stereo
    // (BASELINE configs[2]): 1023 tiles of 660 frames per channel.  Pass 1 runs on thirds of a tile (6138 waves: six per SIMD).  Never more than 8 n_cu items:
    // one workgroup beyond two per CU would run alone in a second round.  Between n_cu / 2 and n_cu stream-channels the frame-interleaved shape runs ONE tile
    // per stream-channel (no pass 1) and wins: 96 / 112 / 127 streams of 10 s 1.53 / 1.64 / 1.75 ms per graph step against 1.55 / 1.74 / 2.00 with tiles;
    // 40 and 80 streams tie (profiles/r06_shape_sweep.md).
    if (ctx->pv_fps == 0 && 2 * n_sc <= n_cu) {
        const size_t want = 8 * n_cu / n_sc;                          // tiles per stream-channel, rounded down
        if (want >= 2 && frames >= 128 * want) {
            size_t third = ((frames + want - 1) / want + 2) / 3;          // pass-1 tile: a third of a synthesis tile (6 n_cu x 4 waves), >= 43 frames
            if (third < 64) third = 64;
            *frames_per_step = 1;
            *phase_tile = (int)third;
            return (int)(3 * third);
        }
    }
    // a synthesis tile pays 4 priming / tail frames and keeps >= 64; a pass-1 tile pays one priming frame and may be as short as kMinPhase frames, so that
    // pass 1 still gets its 24 n_cu waves on short streams (40 streams of 10 s: 6160 waves of 29 frames instead of 2800 of 64: profiles/r06_pass1.md)
    const size_t kMinPhase = ctx->dbg_pv_min_ptile > 0 ? (size_t)ctx->dbg_pv_min_ptile : 16;
    const size_t max_synth = (frames + 63) / 64, max_phase = (frames + kMinPhase - 1) / kMinPhase;
    // workgroups wanted: one per CU (two from 2048 stream-channels, where no tiles are needed anyway)
    const size_t wg = (n_sc * (size_t)fps + 3) / 4;                      // workgroups of one tile per stream-channel
    size_t n_synth = wg >= n_cu ? 1 : n_cu / wg;
    if (n_synth > max_synth) n_synth = max_synth;
    size_t n_phase = n_synth == 1 ? 1 : (24 * n_cu + n_sc - 1) / n_sc;   // a single synthesis tile needs no pass 1; else six waves per SIMD
    if (n_phase > max_phase) n_phase = max_phase;
    size_t step = (n_phase + n_synth - 1) / n_synth;
    if (step < 1) step = 1;
    size_t pt = (frames + n_synth * step - 1) / (n_synth * step);
    if (pt < kMinPhase) pt = kMinPhase;
    if (pt * step < 64) pt = (64 + step - 1) / step;
    *phase_tile = (int)pt;
    return (int)(pt * step);
}

// The one tile rule (nae_internal.h).  For the vocoder: more tiles than one round of the resident pass-3 waves would not add occupancy, only
// re-analysis (a tile pays one priming and three tail frames); a single tile per stream-channel needs no pass 1.  For the FIR filter: a tile
// re-reads half a block at its head, at most 1 / 16 of its input, and a launch of fewer than min_tile blocks is one tile.
int nae_pick_tile(nae_ctx* ctx, int forced, size_t units, size_t n_sc, size_t resident, size_t min_tile, bool max_tiles_down)
{
    if (forced > 0) return forced;
    const size_t n_cu = (size_t)(ctx->n_cu > 0 ? ctx->n_cu : 256);
    if (units == 0 || n_sc == 0) return (int)min_tile;
    size_t n_tiles = (resident * n_cu + n_sc - 1) / n_sc;
    const size_t max_tiles = (units + (max_tiles_down ? 0 : min_tile - 1)) / min_tile;
    if (n_tiles > max_tiles) n_tiles = max_tiles;
    if (n_tiles < 1) n_tiles = 1;
    const size_t tile = (units + n_tiles - 1) / n_tiles;
    return (int)(tile < 0x40000000 ? tile : 0x40000000);
}

// Tiles of a block call on the kernels it runs, and the phase workspace for them: the pipeline's shape rule, else one tile per pass-3 wave
struct PvBlockShape { int tile, phase_tile, frames_per_step; };
static int pv_block_shape(nae_ctx* ctx, const nae_pv_run& r, size_t frames, int ch, size_t n_streams, PvBlockShape* s)
{
    const PvKernels pass3 = nae_pv_route_of(ctx, r).pass3;
    const size_t n_sc = n_streams * ch;
    s->frames_per_step = 1;
    if (pass3 == PvKernels::kShipped) s->tile = nae_pick_pv_shape(ctx, frames, n_sc, &s->phase_tile, &s->frames_per_step);
    else {
        // the kernel's own residency (locked: four waves per SIMD), tiles of at least 64 frames (pv_min_ptile does not apply to the locked route)
        const size_t min_tile = pass3 != PvKernels::kLock && ctx->dbg_pv_min_ptile > 0 ? (size_t)ctx->dbg_pv_min_ptile : 64;
        s->tile = s->phase_tile = nae_pick_tile(ctx, ctx->pv_tile, frames, n_sc, (size_t)nae_pv_resident(ctx, r, pass3), min_tile, false);
    }
    return nae_pv_reserve_ws(ctx, r, frames, ch, n_streams, s->phase_tile);
}

extern "C" {

int nae_abi_version(void) { return NAE_ABI_VERSION; }

int nae_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// Several GPUs per process: the reference runs every node of a graph in ONE process on ONE thread
// (/root/reference/src/infra/runner.cpp:65-83,142-154), so the drop-in must reach all devices of the node from there.  A context
// remembers its device; allocations and launches go to the calling thread's CURRENT device in HIP, so every entry point selects
// the context's device first when it differs (nae_use_device: one hipGetDevice on the fast path) and leaves it selected.
// No process-global state: launch attributes are tracked per context, so contexts may be created and driven from different
// threads as long as ONE thread at a time drives a given context and its handles (include/nae_gpu.h, "Threads").
int nae_debug_set(nae_ctx* ctx, const char* key, long long value)
{
    if (!ctx || !key) return NAE_ERR_INVALID;
    const std::string k(key);
    const bool flag = value == 0 || value == 1;
    const bool count = value >= 0 && value <= 0x7fffffffll;
    auto one_of = [&](std::initializer_list<long long> ok) { for (long long v : ok) if (v == value) return true; return false; };
    if (k == "pv_tile" && count) ctx->pv_tile = (int)value;
    else if (k == "fir_tile" && count) ctx->fir_tile = (int)value;
    else if (k == "dn_tile" && count) ctx->dn_tile = (int)value;
    else if (k == "hpss_tile" && count) ctx->hpss_tile = (int)value;
    else if (k == "conv_tile" && count) ctx->conv_tile = (int)value;
    else if (k == "conv_ring" && count) ctx->conv_ring = (int)value;
    else if (k == "dither_roles" && one_of({0, 1, 2})) ctx->dither_roles = (int)value;
    else if (k == "echo_group" && count) ctx->echo_group = (int)value;
    else if (k == "mod_sub" && value >= 0 && value <= 64) ctx->mod_sub = (int)value;
    else if (k == "sat_tile" && count) ctx->sat_tile = (int)value;
    else if (k == "mb_group" && count) ctx->mb_group = (int)value;
    else if (k == "mb_slab" && count) ctx->mb_slab = (int)value;
    else if (k == "pv_fps" && one_of({0, 1, 2, 4})) ctx->pv_fps = (int)value;
    else if (k == "pv_flow" && one_of({0, 1, 2})) ctx->pv_flow = (int)value;
    else if (k == "pv_lean" && flag) ctx->pv_lean = value != 0;
    else if (k == "pv_min_ptile" && count) ctx->dbg_pv_min_ptile = (int)value;
    else if (k == "rs_single" && flag) ctx->dbg_rs_single = value != 0;
    else if (k == "rs_direct" && flag) ctx->dbg_rs_direct = value != 0;
    else if (k == "no_mix_fuse" && flag) ctx->dbg_no_mix_fuse = value != 0;
    else if (k == "spec_generic" && flag) ctx->dbg_spec_generic = value != 0;
    else if (k == "spec_narrow" && flag) ctx->dbg_spec_narrow = value != 0;
    else if (k == "spec_chunk" && count) ctx->dbg_spec_chunk = (int)value;
    else if (k == "spec_any" && flag) ctx->dbg_spec_any = value != 0;
    else if (k == "pv_any" && flag) ctx->dbg_pv_any = value != 0;
    else if (k == "spec_fine" && count) ctx->dbg_spec_fine = (int)value;
    else if (k == "spec_fine_rounds" && count) ctx->dbg_spec_fine_rounds = (int)value;
    else if (k == "td_nc" && one_of({0, 1, 2, 4})) ctx->dbg_td_nc = (int)value;
    else if (k == "st_unfused" && flag) ctx->dbg_st_unfused = value != 0;
    else return nae_fail(ctx, NAE_ERR_INVALID, "nae_debug_set: unknown key or value out of range");
    return NAE_OK;
}

int nae_ctx_create(int device, nae_ctx** out)
{
    if (!out) return NAE_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return NAE_ERR_HIP;
    if (device < 0 || device >= n) return NAE_ERR_INVALID;          // no such device
    if (hipSetDevice(device) != hipSuccess) return NAE_ERR_HIP;
    nae_ctx* ctx = new (std::nothrow) nae_ctx();
    if (!ctx) return NAE_ERR_NOMEM;
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        snprintf(ctx->name, sizeof ctx->name, "%s (%s)", prop.name, prop.gcnArchName);
        if (prop.multiProcessorCount > 0) ctx->n_cu = prop.multiProcessorCount;
    }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return NAE_ERR_HIP; }
    ctx->own_stream = true;
    if (const char* e = getenv("NAE_DEBUG")) {
        // "key=value,key=value": the one environment hook of the switches of nae_debug_set
        std::string all(e);
        size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string kv = all.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (!kv.empty() && (eq == std::string::npos || nae_debug_set(ctx, kv.substr(0, eq).c_str(), atoll(kv.c_str() + eq + 1)) != NAE_OK)) {
                fprintf(stderr, "libnae_gpu: NAE_DEBUG: bad assignment '%s'\n", kv.c_str());
                (void)hipStreamDestroy(ctx->stream);
                delete ctx;
                return NAE_ERR_INVALID;
            }
            pos = end + 1;
        }
    }
    // the 1024-point tables up front (the first call of that size pays nothing; every size reads its W512), and the spectrum's work counter
    const bool ok = nae_fft_tab_ensure(ctx, NAE_FFT_N) == NAE_OK && ctx->spec_ctr.reserve(ctx, 64, "spectrum work counter") == NAE_OK &&
                    hipMemset(ctx->spec_ctr.p, 0, 64) == hipSuccess;
    if (!ok) { nae_ctx_destroy(ctx); return NAE_ERR_HIP; }
    *out = ctx;
    return NAE_OK;
}

int nae_ctx_destroy(nae_ctx* ctx)
{
    if (!ctx) return NAE_OK;
    (void)nae_use_device(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    prof_collect(ctx);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;                  // the device is selected and the stream drained: every CtxBuf of the context frees itself
    return NAE_OK;
}

int nae_ctx_set_stream(nae_ctx* ctx, void* hip_stream)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
    return NAE_OK;
}

void* nae_ctx_stream(nae_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int nae_sync(nae_ctx* ctx)
{
    return ctx ? nae_ctx_drain(ctx) : NAE_ERR_INVALID;
}

int nae_poll(nae_ctx* ctx)
{
    if (!ctx) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    hipError_t e = hipStreamQuery(ctx->stream);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return nae_check(ctx, e, "hipStreamQuery");
}

const char* nae_last_error(nae_ctx* ctx) { return ctx ? ctx->err : "null context"; }
const char* nae_device_name(nae_ctx* ctx) { return ctx ? ctx->name : ""; }

int nae_malloc(nae_ctx* ctx, size_t bytes, void** dptr)
{
    if (!ctx || !dptr) return NAE_ERR_INVALID;
    *dptr = nullptr;
    if (bytes == 0) bytes = 16;
    (void)nae_use_device(ctx);
    hipError_t e = hipMalloc(dptr, bytes);
    if (e != hipSuccess) { nae_check(ctx, e, "hipMalloc"); return NAE_ERR_NOMEM; }
    return NAE_OK;
}
int nae_free(nae_ctx* ctx, void* dptr)
{
    if (!dptr) return NAE_OK;
    if (ctx) (void)nae_use_device(ctx);
    return nae_check(ctx, hipFree(dptr), "hipFree");
}
int nae_malloc_host(nae_ctx* ctx, size_t bytes, void** hptr)
{
    if (!ctx || !hptr) return NAE_ERR_INVALID;
    *hptr = nullptr;
    if (bytes == 0) bytes = 16;
    (void)nae_use_device(ctx);
    hipError_t e = hipHostMalloc(hptr, bytes, hipHostMallocDefault);
    if (e != hipSuccess) { nae_check(ctx, e, "hipHostMalloc"); return NAE_ERR_NOMEM; }
    return NAE_OK;
}
int nae_free_host(nae_ctx* ctx, void* hptr)
{
    if (!hptr) return NAE_OK;
    if (ctx) (void)nae_use_device(ctx);
    return nae_check(ctx, hipHostFree(hptr), "hipHostFree");
}
int nae_memcpy_h2d(nae_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx || (bytes && (!dst || !src))) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(h2d)");
}
int nae_memcpy_d2h(nae_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx || (bytes && (!dst || !src))) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(d2h)");
}
int nae_memcpy_d2d(nae_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx || (bytes && (!dst || !src))) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(d2d)");
}
int nae_memset(nae_ctx* ctx, void* dst, int value, size_t bytes)
{
    if (!ctx || (bytes && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream), "hipMemsetAsync");
}

int nae_event_create(nae_ctx* ctx, nae_event** ev)
{
    if (!ctx || !ev) return NAE_ERR_INVALID;
    nae_event* e = new (std::nothrow) nae_event();
    if (!e) return NAE_ERR_NOMEM;
    (void)nae_use_device(ctx);
    if (hipEventCreate(&e->ev) != hipSuccess) { delete e; return NAE_ERR_HIP; }
    *ev = e;
    return NAE_OK;
}
int nae_event_record(nae_ctx* ctx, nae_event* ev)
{
    if (!ctx || !ev) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipEventRecord(ev->ev, ctx->stream), "hipEventRecord");
}
int nae_event_query(nae_event* ev)
{
    if (!ev) return NAE_ERR_INVALID;
    const hipError_t e = hipEventQuery(ev->ev);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return NAE_ERR_HIP;
}
int nae_ctx_wait_event(nae_ctx* ctx, nae_event* ev)
{
    if (!ctx || !ev) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return nae_check(ctx, hipStreamWaitEvent(ctx->stream, ev->ev, 0), "hipStreamWaitEvent");
}
int nae_event_elapsed_ms(nae_event* start, nae_event* stop, float* ms)
{
    if (!start || !stop || !ms) return NAE_ERR_INVALID;
    if (hipEventSynchronize(stop->ev) != hipSuccess) return NAE_ERR_HIP;
    return hipEventElapsedTime(ms, start->ev, stop->ev) == hipSuccess ? NAE_OK : NAE_ERR_HIP;
}
int nae_event_destroy(nae_event* ev)
{
    if (!ev) return NAE_OK;
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return NAE_OK;
}

int nae_prof_enable(nae_ctx* ctx, int on)
{
    if (!ctx) return NAE_ERR_INVALID;
    prof_collect(ctx);
    ctx->prof_on = on != 0;
    return NAE_OK;
}
int nae_prof_reset(nae_ctx* ctx)
{
    if (!ctx) return NAE_ERR_INVALID;
    prof_collect(ctx);
    ctx->prof_slots.clear();
    return NAE_OK;
}
int nae_prof_get(nae_ctx* ctx, int index, char* name, size_t name_cap, double* total_ms, uint64_t* launches)
{
    if (!ctx) return NAE_ERR_INVALID;
    prof_collect(ctx);
    if (index < 0 || index >= (int)ctx->prof_slots.size()) return (int)ctx->prof_slots.size();
    if (name && name_cap) snprintf(name, name_cap, "%s", ctx->prof_slots[index].name);
    if (total_ms) *total_ms = ctx->prof_slots[index].total_ms;
    if (launches) *launches = ctx->prof_slots[index].launches;
    return (int)ctx->prof_slots.size();
}

// ------------------------------------------------------------------------------------------------ K7 plan
// Parameter resolution, DESIGN.md §3.2.  SoundTouch mapping (audio-velocity.cpp:384-385): setRate(rate) and
// setPitch(pitch) give a time-stretch of 1/pitch followed by a resampling of rate*pitch.
int nae_stretch_plan_make(double rate, double pitch, size_t in_len, nae_stretch_plan* pl)
{
    return nae_stretch_plan_make_n(rate, pitch, NAE_FFT_N, in_len, pl);
}

// frame size n_fft, synthesis hop H = n_fft / 4: the hop, the phase-advance ratios and the frame count follow the size,
// everything else does not
int nae_stretch_plan_make_n(double rate, double pitch, int n_fft, size_t in_len, nae_stretch_plan* pl)
{
    return nae_stretch_plan_make_shift(rate, pitch, 1.0, 0, n_fft, in_len, pl);
}

// the plan of the _formant_shift entries ("Formant shift"): the _n plan, with the vocoder stage forced on (tempo_eff = 1: ha = H,
// d0 = H, r = 2^24) when the envelope stage runs (nae_formant_stage_on) and the tempo is 1.  lifter = 0 is the _n plan.
int nae_stretch_plan_make_shift(double rate, double pitch, double formant_ratio, int lifter, int n_fft, size_t in_len, nae_stretch_plan* pl)
{
    if (!pl) return NAE_ERR_INVALID;
    memset(pl, 0, sizeof *pl);
    if (!nae_size_ok(n_fft)) return NAE_ERR_UNSUPPORTED;
    const int hop = n_fft / 4;
    if (!(rate > 0.0) || !(pitch > 0.0)) return NAE_ERR_INVALID;
    if (!std::isfinite(formant_ratio) || !(formant_ratio > 0.0) || lifter < 0 || lifter > n_fft / 4) return NAE_ERR_INVALID;
    if (formant_ratio < NAE_FORMANT_SHIFT_MIN || formant_ratio > NAE_FORMANT_SHIFT_MAX) return NAE_ERR_UNSUPPORTED;
    double tempo = 1.0 / pitch, rho = rate * pitch;
    if (fabs(tempo - 1.0) < 1e-6) tempo = 1.0;
    if (fabs(rho - 1.0) < 1e-6) rho = 1.0;
    pl->pv_on = tempo != 1.0 || nae_formant_stage_on(rho, lifter, formant_ratio);
    pl->rs_on = rho != 1.0;
    if (pl->pv_on && (tempo < NAE_TEMPO_MIN || tempo > NAE_TEMPO_MAX)) return NAE_ERR_UNSUPPORTED;
    if (pl->rs_on && (rho < NAE_RATE_MIN || rho > NAE_RATE_MAX)) return NAE_ERR_UNSUPPORTED;
    pl->tempo_eff = tempo;
    pl->rate_eff = rho;
    pl->ha_q24 = (int64_t)llround((double)hop * tempo * (double)(1 << NAE_HA_FRAC_BITS));
    pl->d0 = (int32_t)(pl->ha_q24 >> NAE_HA_FRAC_BITS);
    for (int i = 0; i < 2; i++) {
        const uint64_t d = (uint64_t)(pl->d0 + i);
        pl->r_q24[i] = (uint32_t)((((uint64_t)hop << NAE_R_FRAC_BITS) + d / 2) / d);
    }
    pl->step_q32 = (uint64_t)llround(rho * 4294967296.0);
    pl->out_len = (size_t)floor((double)in_len / (tempo * rho) + 0.5);
    pl->rs_first = pl->pv_on && pl->rs_on && rho > 1.0;
    size_t pv_out;
    if (pl->rs_first) {
        pl->mid_len = (size_t)floor((double)in_len / rho + 0.5);
        pv_out = pl->out_len;
    } else if (pl->rs_on) {
        if (pl->out_len == 0) pl->mid_len = 0;
        else {
            const unsigned __int128 pos = (unsigned __int128)(pl->out_len - 1) * pl->step_q32;
            pl->mid_len = (size_t)(pos >> 32) + NAE_RS_TAPS / 2 + 1;
        }
        pv_out = pl->mid_len;
    } else {
        pl->mid_len = pl->out_len;
        pv_out = pl->out_len;
    }
    pl->frames = pl->pv_on ? (pv_out + n_fft / 2 + hop - 1) / hop + 1 : 0;
    return NAE_OK;
}

static int check_sig(nae_ctx* ctx, const nae_sig* s, const char* what)
{
    if (!s || !s->base) return nae_fail(ctx, NAE_ERR_INVALID, what);
    return NAE_OK;
}

} // extern "C"

// the signal between the transposer and the vocoder: planar in the context's workspace, rows padded to 4 frames (16-byte accesses on both sides)
static int reserve_mid(nae_ctx* ctx, const nae_stretch_plan& pl, int ch, size_t n_streams, nae_sig* mid)
{
    const size_t mid_stride = (pl.mid_len + 3) & ~(size_t)3;
    const int rc = ctx->ws_mid.reserve(ctx, n_streams * ch * mid_stride * sizeof(float), "workspace");
    if (rc) return rc;
    *mid = nae_sig{ctx->ws_mid.p, (size_t)ch * mid_stride, mid_stride, 1};
    return NAE_OK;
}

int nae_pv_opts_check(nae_ctx* ctx, unsigned flags, unsigned allowed, int n_fft, int lifter, const double* formant_ratio, nae_pv_opts* o)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (flags & ~allowed) return nae_fail(ctx, NAE_ERR_INVALID, "unknown stretch flag");
    if (!nae_size_ok(n_fft)) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "vocoder: n_fft must be 512, 1024, 2048 or 4096");
    if ((flags & NAE_STRETCH_PHASE_LOCK) && n_fft != NAE_FFT_N) return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "phase locking runs at n_fft = 1024 only");
    if (lifter < 0 || lifter > n_fft / 4) return nae_fail(ctx, NAE_ERR_INVALID, "formant lifter must be in [0, n_fft / 4]");
    *o = nae_pv_opts{n_fft, lifter, (flags & NAE_STRETCH_PHASE_LOCK) != 0, (flags & NAE_STRETCH_TRANSIENTS) != 0, formant_ratio != nullptr,
                     formant_ratio ? *formant_ratio : 1.0, (flags & NAE_STRETCH_LINK_CHANNELS) != 0};
    return NAE_OK;
}

int nae_pv_plan_make(nae_ctx* ctx, const nae_pv_opts& o, double rate, double pitch, size_t in_len, nae_stretch_plan* pl)
{
    const int rc = o.shift ? nae_stretch_plan_make_shift(rate, pitch, o.formant_ratio, o.lifter, o.n_fft, in_len, pl)
                           : nae_stretch_plan_make_n(rate, pitch, o.n_fft, in_len, pl);
    return rc ? nae_fail(ctx, rc, o.shift ? "rate/pitch/formant ratio outside the supported range" : "rate/pitch outside the supported range") : NAE_OK;
}

// a 2-input mix node in front of the stretch node (graph4): when the transposer runs first it can mix while staging
struct nae_mix_front {
    const nae_sig* a;
    const nae_sig* b;
    float va, vb;
};

// stages: bit 0 = the front stage (the mix node, and the transposer when it runs first), bit 1 = everything behind it
// (nae_debug_graph4_stages: scheduling experiments run the two from separate calls; the intermediate signal stays in the
// context's workspace between them).
static int stretch_block_impl(nae_ctx* ctx, const nae_pv_opts& o, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                              size_t n_streams, const nae_sig* dst, const nae_mix_front* front, int stages)
{
    int rc;
    if ((rc = check_sig(ctx, src, "null source view")) || (rc = check_sig(ctx, dst, "null destination view"))) return rc;
    if (ch < 1 || ch > 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    nae_stretch_plan pl;
    if ((rc = nae_pv_plan_make(ctx, o, rate, pitch, in_len, &pl))) return rc;
    // the mix node in front: fused into the transposer when that runs first, else its own launch (src = its output)
    bool mix_pending = front != nullptr && (stages & 1);
    auto run_mix = [&]() -> int {
        if (!mix_pending) return NAE_OK;
        mix_pending = false;
        const nae_sig ins[2] = {*front->a, *front->b};
        const float vol[2] = {front->va, front->vb};
        return nae_amix_sig_f32(ctx, ins, vol, 2, src, in_len, n_streams);
    };
    if (n_streams == 0 || pl.out_len == 0) return run_mix();
    if (!pl.pv_on && !pl.rs_on) {
        if ((rc = run_mix())) return rc;
        return (stages & 2) ? nae_launch_copy_sig(ctx, src, dst, in_len, ch, n_streams, false, 1.0f) : NAE_OK;
    }

    nae_sig mid{};
    if (pl.pv_on && pl.rs_on && (rc = reserve_mid(ctx, pl, ch, n_streams, &mid))) return rc;
    if (pl.rs_on) {
        rc = nae_ensure_rs_table(ctx, pl.rate_eff);
        if (rc) return rc;
    }
    // stage order: transposer first when it shrinks the signal (rate_eff > 1), else vocoder first
    const nae_sig* pv_src = src;
    size_t pv_in_len = in_len;
    const nae_sig* pv_dst = dst;
    long long pv_out_len = (long long)pl.out_len;
    if (pl.rs_first && !(stages & 1)) {
        pv_src = &mid;
        pv_in_len = pl.mid_len;
    } else if (pl.rs_first) {
        rc = 1;
        if (mix_pending && ch == 2) {
            rc = nae_launch_mix_resample(ctx, &pl, front->a, front->b, front->va, front->vb, src, in_len, n_streams, ctx->rs_tab.as<float>(), &mid);
            if (rc < 0) return rc;
            if (rc == 0) mix_pending = false;
        }
        if (rc == 1) {
            if ((rc = run_mix())) return rc;
            rc = nae_launch_resample(ctx, &pl, src, in_len, ch, n_streams, ctx->rs_tab.as<float>(), &mid, 0, pl.mid_len);
            if (rc) return rc;
        }
        pv_src = &mid;
        pv_in_len = pl.mid_len;
    } else if (pl.pv_on && pl.rs_on) {
        pv_dst = &mid;
        pv_out_len = (long long)pl.mid_len;
    }
    if ((rc = run_mix())) return rc;     // vocoder first / transposer only: the mix is a launch of its own
    if (!(stages & 2)) return NAE_OK;
    if (pl.pv_on) {
        const nae_pv_run run = nae_pv_resolve(o, pl, ch);
        PvBlockShape sh;
        if ((rc = pv_block_shape(ctx, run, pl.frames, ch, n_streams, &sh))) return rc;
        const nae_pv_segment seg{0, (long long)pl.frames, (long long)pl.frames, pv_out_len, nullptr, nullptr};
        rc = nae_launch_pv_phase(ctx, run, &pl, pv_src, pv_in_len, ch, n_streams, sh.phase_tile, sh.tile, ctx->ws_phase.as<uint32_t>(), &seg);
        if (rc) return rc;
        rc = nae_launch_pv_synth(ctx, run, &pl, pv_src, pv_in_len, ch, n_streams, sh.tile, sh.phase_tile, ctx->ws_phase.as<uint32_t>(),
                                 pv_dst, &seg, sh.frames_per_step);
        if (rc) return rc;
    }
    if (pl.rs_on && !pl.rs_first) {
        const nae_sig* rs_src = pl.pv_on ? &mid : src;
        const size_t rs_src_len = pl.pv_on ? pl.mid_len : in_len;
        rc = nae_launch_resample(ctx, &pl, rs_src, rs_src_len, ch, n_streams, ctx->rs_tab.as<float>(), dst, 0, pl.out_len);
        if (rc) return rc;
    }
    return NAE_OK;
}

extern "C" {

int nae_stretch_block_f32(nae_ctx* ctx, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                          size_t n_streams, const nae_sig* dst)
{
    return nae_stretch_block_ex_f32(ctx, rate, pitch, 0u, src, in_len, ch, n_streams, dst);
}

int nae_stretch_block_ex_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, const nae_sig* src, size_t in_len, int ch,
                             size_t n_streams, const nae_sig* dst)
{
    nae_pv_opts o;
    const int rc = nae_pv_opts_check(ctx, flags, NAE_STRETCH_PHASE_LOCK, NAE_FFT_N, 0, nullptr, &o);
    return rc ? rc : stretch_block_impl(ctx, o, rate, pitch, src, in_len, ch, n_streams, dst, nullptr, 3);
}

int nae_stretch_block_n_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, const nae_sig* src, size_t in_len, int ch,
                            size_t n_streams, const nae_sig* dst)
{
    return nae_stretch_block_formant_f32(ctx, rate, pitch, flags, n_fft, 0, src, in_len, ch, n_streams, dst);
}

int nae_stretch_formant_lifter(int sample_rate, int n_fft)
{
    if (!nae_size_ok(n_fft) || sample_rate <= 0) return 0;
    int q = sample_rate / 700;
    if (q < 1) q = 1;
    return q < n_fft / 4 ? q : n_fft / 4;
}

int nae_stretch_block_formant_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, int lifter, const nae_sig* src, size_t in_len,
                                  int ch, size_t n_streams, const nae_sig* dst)
{
    nae_pv_opts o;
    const int rc = nae_pv_opts_check(ctx, flags, kPvFlagsN, n_fft, lifter, nullptr, &o);
    return rc ? rc : stretch_block_impl(ctx, o, rate, pitch, src, in_len, ch, n_streams, dst, nullptr, 3);
}

int nae_stretch_block_formant_shift_f32(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, int lifter, double formant_ratio,
                                        const nae_sig* src, size_t in_len, int ch, size_t n_streams, const nae_sig* dst)
{
    nae_pv_opts o;
    const int rc = nae_pv_opts_check(ctx, flags, kPvFlagsN, n_fft, lifter, &formant_ratio, &o);
    return rc ? rc : stretch_block_impl(ctx, o, rate, pitch, src, in_len, ch, n_streams, dst, nullptr, 3);
}

// pass 1 + 2 of a block call in tiles of 64 frames (pv_tile), the records copied to the host
static int pv_tile_phase_impl(nae_ctx* ctx, const nae_pv_opts& o, double rate, double pitch, const nae_sig* src, size_t in_len, int ch, size_t n_streams,
                              int32_t* dst_host, size_t dst_capacity, size_t* n_tiles_out, size_t* tile_frames)
{
    if (!dst_host || !n_tiles_out || !tile_frames) return NAE_ERR_INVALID;
    int rc = check_sig(ctx, src, "null source view");
    if (rc) return rc;
    nae_stretch_plan pl;
    if ((rc = nae_pv_plan_make(ctx, o, rate, pitch, in_len, &pl))) return rc;
    if (!pl.pv_on) return nae_fail(ctx, NAE_ERR_STATE, "phase vocoder stage is bypassed for these parameters");
    const int tile = ctx->pv_tile > 0 ? ctx->pv_tile : 64;
    const size_t n_tiles = (pl.frames + tile - 1) / tile;
    *n_tiles_out = n_tiles;
    *tile_frames = (size_t)tile;
    const nae_pv_run run = nae_pv_resolve(o, pl, ch);   // an _n plan with the stage on: never forced, the transient flag as given
    const size_t bins = (size_t)o.n_fft / 2 + 1, pad = nae_pv_record_pad(o.n_fft);
    const size_t need = n_streams * ch * n_tiles * bins;
    if (dst_capacity < need) return nae_fail(ctx, NAE_ERR_INVALID, "destination too small");
    if (n_tiles == 1) {
        // a single tile: nae_launch_pv_phase writes no record (pass 3 starts from zero by itself, PvParams::base_zero), so the workspace holds
        // whatever an earlier call left; the phase in front of tile 0 is zero
        memset(dst_host, 0, need * sizeof(int32_t));
        return NAE_OK;
    }
    const size_t ws_bytes = nae_pv_workspace_bytes(false, o.n_fft, pl.frames, ch, n_streams, tile);   // the records (the locked workspace begins with them)
    if ((rc = nae_pv_reserve_ws(ctx, run, pl.frames, ch, n_streams, tile))) return rc;
    const nae_sig* pv_src = src;
    size_t pv_in_len = in_len;
    nae_sig mid{};
    if (pl.rs_first) {
        rc = reserve_mid(ctx, pl, ch, n_streams, &mid);
        if (rc) return rc;
        rc = nae_ensure_rs_table(ctx, pl.rate_eff);
        if (rc) return rc;
        rc = nae_launch_resample(ctx, &pl, src, in_len, ch, n_streams, ctx->rs_tab.as<float>(), &mid, 0, pl.mid_len);
        if (rc) return rc;
        pv_src = &mid;
        pv_in_len = pl.mid_len;
    }
    const nae_pv_segment seg{0, (long long)pl.frames, (long long)pl.frames, 0, nullptr, nullptr};
    rc = nae_launch_pv_phase(ctx, run, &pl, pv_src, pv_in_len, ch, n_streams, tile, tile, ctx->ws_phase.as<uint32_t>(), &seg);
    if (rc) return rc;
    std::vector<int32_t> tmp(ws_bytes / sizeof(int32_t));
    hipError_t e = hipMemcpyAsync(tmp.data(), ctx->ws_phase.p, ws_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return nae_check(ctx, e, "copy phase workspace");
    for (size_t rec = 0; rec < n_streams * ch * n_tiles; rec++)
        memcpy(dst_host + rec * bins, tmp.data() + rec * pad, bins * sizeof(int32_t));
    return NAE_OK;
}

int nae_debug_pv_tile_phase(nae_ctx* ctx, double rate, double pitch, const nae_sig* src, size_t in_len, int ch,
                            size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles_out,
                            size_t* tile_frames)
{
    return nae_debug_pv_tile_phase_ex(ctx, rate, pitch, 0u, src, in_len, ch, n_streams, dst_host, dst_capacity, n_tiles_out, tile_frames);
}

int nae_debug_pv_tile_phase_ex(nae_ctx* ctx, double rate, double pitch, unsigned flags, const nae_sig* src, size_t in_len, int ch,
                               size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles_out,
                               size_t* tile_frames)
{
    nae_pv_opts o;
    const int rc = nae_pv_opts_check(ctx, flags, NAE_STRETCH_PHASE_LOCK, NAE_FFT_N, 0, nullptr, &o);
    return rc ? rc : pv_tile_phase_impl(ctx, o, rate, pitch, src, in_len, ch, n_streams, dst_host, dst_capacity, n_tiles_out, tile_frames);
}

int nae_debug_pv_tile_phase_n(nae_ctx* ctx, double rate, double pitch, unsigned flags, int n_fft, const nae_sig* src, size_t in_len, int ch,
                              size_t n_streams, int32_t* dst_host, size_t dst_capacity, size_t* n_tiles_out, size_t* tile_frames)
{
    nae_pv_opts o;
    const int rc = nae_pv_opts_check(ctx, flags, kPvFlagsN, n_fft, 0, nullptr, &o);
    return rc ? rc : pv_tile_phase_impl(ctx, o, rate, pitch, src, in_len, ch, n_streams, dst_host, dst_capacity, n_tiles_out, tile_frames);
}

// ------------------------------------------------------------------------------------------------ K8
size_t nae_spectrum_frames(size_t T) { return nae_spectrum_frames_ex(T, NAE_FFT_N, NAE_HOP); }

int nae_spectrum_block_f32(nae_ctx* ctx, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                           size_t dst_stream_stride)
{
    return nae_spectrum_block_ex_f32(ctx, NAE_FFT_N, NAE_HOP, src, T, ch, n_streams, dst, dst_stream_stride);
}

size_t nae_spectrum_frames_ex(size_t T, int n_fft, int hop)
{
    if (nae_spectrum_check(n_fft, hop) != NAE_OK) return 0;
    return T < (size_t)n_fft ? 0 : (T - (size_t)n_fft) / (size_t)hop + 1;
}

int nae_spectrum_block_ex_f32(nae_ctx* ctx, int n_fft, int hop, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                              size_t dst_stream_stride)
{
    if (!ctx || !dst) return NAE_ERR_INVALID;
    const int chk = nae_spectrum_check(n_fft, hop);
    if (chk != NAE_OK)
        return nae_fail(ctx, chk, chk == NAE_ERR_UNSUPPORTED ? "spectrum: n_fft must be a power of two in [256, 4096]" : "spectrum: hop must be in [1, n_fft]");
    int rc = check_sig(ctx, src, "null source view");
    if (rc) return rc;
    if (ch < 1 || ch > 2) return nae_fail(ctx, NAE_ERR_INVALID, "channel count must be 1 or 2");
    return nae_launch_spectrum(ctx, n_fft, hop, src, T, ch, n_streams, dst, dst_stream_stride);
}

// ------------------------------------------------------------------------------------------------ graph
// mask: 1 = mix node (+ the pitch node's transposer when that runs first), 2 = the rest of the pitch node, 4 = spectrum node
static int graph4_stages(nae_ctx* ctx, const nae_graph4* g, int mask)
{
    // node 1+2: the two inputs feed the 2-input mixer (audio-amix.cpp:86-324 with input_num = 2)
    // node 3: pitch (audio-velocity.cpp:462-477).  When its transposer runs first the mix happens inside that launch
    // (same arithmetic, same mix_out contents); otherwise the mix is launched on its own in front.
    if (!g->in_a.base || !g->in_b.base || !g->mix_out.base) return nae_fail(ctx, NAE_ERR_INVALID, "nae_graph4_run: null signal");
    const nae_mix_front front{&g->in_a, &g->in_b, g->vol_a, g->vol_b};
    int rc = NAE_OK;
    if (mask & 3) rc = stretch_block_impl(ctx, nae_pv_opts{}, g->rate, g->pitch, &g->mix_out, g->S, 2, g->n_streams, &g->pitch_out, &front, mask & 3);
    if (rc || !(mask & 4)) return rc;
    nae_stretch_plan pl;
    rc = nae_stretch_plan_make(g->rate, g->pitch, g->S, &pl);
    if (rc) return rc;
    // node 4: spectrum
    return nae_spectrum_block_f32(ctx, &g->pitch_out, pl.out_len, 2, g->n_streams, g->spec_out, g->spec_stream_stride);
}

int nae_graph4_run(nae_ctx* ctx, const nae_graph4* g)
{
    if (!ctx || !g) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return graph4_stages(ctx, g, 7);
}

int nae_debug_graph4_stages(nae_ctx* ctx, const nae_graph4* g, int mask)
{
    if (!ctx || !g) return NAE_ERR_INVALID;
    (void)nae_use_device(ctx);
    return graph4_stages(ctx, g, mask);
}

} // extern "C"
