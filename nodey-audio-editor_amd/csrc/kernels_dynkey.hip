// kernels_dynkey.hip — K15, the keyed dynamics ("K15 keyed dynamics") for gfx950: K12 with a side-chain.  The magnitude the
// detector reads comes from a key — another signal, or the signal itself — through up to NAE_DYNKEY_MAX_SECTIONS biquads; everything behind
// it is K12's walk (dyn_steps.h), applied to the signal.
//
// One wave per detector, as dyn_kernel: DC signal channels are read and written (2: a linked stereo stream), KC key channels are read (a
// linked detector hears the larger magnitude of a stereo key; an unlinked one hears its own key channel, or the one of a mono key).  With
// FILT the key's chunk goes, as 16 doubles per lane, through eq_section of eq_cascade.h section by section — K11's tiled form exactly, the
// tables from eq_make_tables, lane s keeping the carry of section s per key channel — and m = (float)|w|, rounded once; behind in_len m is
// zero, where the filter still rings.  The walk levels one chunk ahead of the rest, so at the end of a launch the filter has run through
// chunk c_stop; the carry a handle keeps is the one in front of that chunk (the next launch levels it again, then whole), which the key
// source remembers at every level.  Built with -ffp-contract=off: every step is one IEEE operation in the order of the CPU statement
// (tests/dynkey_ref/ref_dynkey.c).
#include "dyn_steps.h"
#include "eq_cascade.h"
#include <math.h>
#include <string.h>

namespace nae {

static_assert(NAE_DYNKEY_MAX_SECTIONS <= NAE_EQ_MAX_SECTIONS && NAE_DYNKEY_MAX_SECTIONS <= 64, "a lane per section, in K11's constant block");

// What the key source needs per level, kept in LDS and read where a level starts, as wave-uniform values: as kernel arguments the key's
// view, the section count and the tables' address are SGPRs through the whole chunk loop, which K12's walk has none to spare of.
enum { kKeyBase, kKeyCs, kKeyFs, kKeySections, kKeyWords };

__device__ __forceinline__ long long dynkey_uniform(long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The source of the magnitude of steps 1 and 2: a Mag of dyn_steps.h.  kw: the key's words in LDS; tab, pq: the sections' coefficients and
// maps, and their p and q, in LDS (FILT).  st: lane s holds the carry of section s of key channel c as the filter stands; sv: as it stood in
// front of the chunk levelled last, or, where the walk left a level out, as it stands.
template <int KC, bool FILT>
struct DynKeySource {
    const long long* kw;
    const DynParams& p;
    int lane;
    const double* tab;
    const double* pq;
    double st1[KC], st2[KC], sv1[KC], sv2[KC];
    static constexpr bool kSpareSgprs = FILT;          // the sections need the SGPRs the walk's lane masks and addresses would hold through their level

    __device__ void level(float* stage, long long ck, float (&x)[kChunkT])
    {
        const float* kp = reinterpret_cast<const float*>(dynkey_uniform(kw[kKeyBase]));
        const long long cs = dynkey_uniform(kw[kKeyCs]), fs = dynkey_uniform(kw[kKeyFs]);
        if constexpr (!FILT) dyn_plain_level<KC>(stage, kp, cs, fs, p.in_len, ck, lane, x);
        else {
            const int n_sections = (int)dynkey_uniform(kw[kKeySections]);
#pragma unroll
            for (int c = 0; c < KC; c++) {
                // the lane number as the compiler cannot follow it: the sections' lane masks (eight SGPR pairs) are then made here, channel
                // by channel, and not kept through the walk's chunk loop beside its own
                int ln = lane;
                asm volatile("" : "+v"(ln));
                sv1[c] = st1[c];
                sv2[c] = st2[c];
                float xf[kChunkT];
                dyn_load(stage, kp, c * cs, fs, p.in_len, ck, lane, xf);
                double w[kChunkT];
#pragma unroll
                for (int k = 0; k < kChunkT; k++) w[k] = (double)xf[k];
#pragma unroll 1
                for (int s = 0; s < n_sections; s++) eq_section(w, s, ln, tab, pq, st1[c], st2[c]);
                // the lane's samples inside the signal: one number, compared where it is used (sixteen bounds masks are 32 SGPRs)
                const long long left = p.in_len - (ck * kChunkC + ln * kChunkT);
                const int inside = left < 0 ? 0 : (left > kChunkT ? kChunkT : (int)left);
#pragma unroll
                for (int k = 0; k < kChunkT; k++) {
                    const float m = k < inside ? (float)fabs(w[k]) : 0.0f;         // the ringing behind the signal's end is no demand
                    x[k] = c == 0 ? m : (m > x[k] ? m : x[k]);
                    if ((k & 3) == 3) __builtin_amdgcn_sched_barrier(0);          // four samples' masks in flight, not sixteen
                }
            }
        }
    }
    __device__ void skip()
    {
#pragma unroll
        for (int c = 0; c < KC; c++) {
            sv1[c] = st1[c];
            sv2[c] = st2[c];
        }
    }
};

// state: as dyn_kernel's.  fstate: [n_det][KC][NAE_DYNKEY_MAX_SECTIONS][2] doubles, the key filter's carries (z1, z2) in front of chunk
// c_origin, replaced by the ones in front of chunk c_stop; null: zero in, nothing out (the block call).  key_ch: the key view's channels.
template <int DC, int KC, bool FILT>
__global__ __launch_bounds__(64) void dynkey_kernel(SigViewD src, SigViewD key, OutViewD out, DynParams p, int key_ch, int n_sections,
                                                    const double* __restrict__ tab, double* state, double* fstate)
{
    constexpr int kTab = FILT ? kEqTabOfs + NAE_DYNKEY_MAX_SECTIONS * kEqTab : 1, kPq = FILT ? NAE_DYNKEY_MAX_SECTIONS * 2 * kChunkT : 1;
    __shared__ long long kw[kKeyWords];
    __shared__ double ltab[kTab];      // the constant block as far as the sections reach: read at wave-uniform addresses (a broadcast)
    __shared__ double pq[kPq];         // p and q of every section, as eq_cascade_kernel keeps them
    const int lane = threadIdx.x;
    const long long det = blockIdx.x;
    if (det >= p.n_det) return;
    // DC = 2: the two channels of stereo stream `det`; DC = 1: stream-channel `det`, which hears its own key channel or a mono key's only one
    const long long s_idx = DC == 2 ? det : det / p.ch;
    const int c0 = DC == 2 ? 0 : (int)(det % p.ch);
    const float* ip = src.base + s_idx * src.ss + c0 * src.cs;
    float* op = out.base + s_idx * out.ss + c0 * out.cs;
    if (lane == 0) {
        kw[kKeyBase] = reinterpret_cast<long long>(key.base + s_idx * key.ss + (key_ch == 1 ? 0 : c0) * key.cs);
        kw[kKeyCs] = key.cs;
        kw[kKeyFs] = key.fs;
        kw[kKeySections] = n_sections;
    }
    DynKeySource<KC, FILT> mag{kw, p, lane, ltab, pq, {}, {}, {}, {}};
    // lane s keeps where section s's carries stand, or null: an address per lane in a VGPR pair, none of the walk's SGPRs
    double* carry = FILT && fstate && lane < n_sections ? fstate + (det * KC * NAE_DYNKEY_MAX_SECTIONS + lane) * 2 : nullptr;
    if constexpr (FILT) {
        for (int i = lane; i < kEqTabOfs + n_sections * kEqTab; i += 64) ltab[i] = tab[i];
        eq_stage_pq(pq, tab, n_sections, lane, 64);
#pragma unroll
        for (int c = 0; c < KC; c++) {
            mag.st1[c] = mag.st2[c] = 0.0;
            if (carry) {
                mag.st1[c] = carry[c * NAE_DYNKEY_MAX_SECTIONS * 2];
                mag.st2[c] = carry[c * NAE_DYNKEY_MAX_SECTIONS * 2 + 1];
            }
        }
    }
    chunk_lds_sync();
    dyn_walk<DC>(ip, op, src, out, p, state, det, lane, mag);
    if constexpr (FILT) {
#pragma unroll
        for (int c = 0; c < KC; c++) {
            if (carry) {
                carry[c * NAE_DYNKEY_MAX_SECTIONS * 2] = mag.sv1[c];
                carry[c * NAE_DYNKEY_MAX_SECTIONS * 2 + 1] = mag.sv2[c];
            }
        }
    }
}

} // namespace nae

// ================================================================================================ host side
using namespace nae;

// the one statement of the parameter rules of nae_dynkey_block_f32 and nae_dynkey_create (ctx may be null: no message then): K12's through
// nae_dyn_check, then the key's
int nae_dynkey_check(nae_ctx* ctx, const nae_dynkey_params* p, int ch)
{
    if (!p) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dynkey: null pointer");
    const int rc = nae_dyn_check(ctx, &p->dyn, ch);
    if (rc) return rc;
    if (p->key_ch != 0 && p->key_ch != 1 && p->key_ch != ch) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dynkey: key_ch must be 0, 1 or the channel count");
    if (p->n_sections < 0) return nae_fail_opt(ctx, NAE_ERR_INVALID, "dynkey: negative n_sections");
    if (p->n_sections > NAE_DYNKEY_MAX_SECTIONS) return nae_fail_opt(ctx, NAE_ERR_UNSUPPORTED, "dynkey: at most 4 sections");
    return p->n_sections ? nae_eq_check(ctx, &p->coef[0][0], p->n_sections, p->key_ch ? p->key_ch : ch) : NAE_OK;   // the sections run on the key's channels
}

size_t nae_dynkey_filter_doubles(const nae_dynkey_params* p, int ch, size_t n_streams)
{
    const int key_ch = p->key_ch ? p->key_ch : ch;
    return nae_dyn_detectors(&p->dyn, ch, n_streams) * (size_t)(p->dyn.link && ch == 2 ? key_ch : 1) * NAE_DYNKEY_MAX_SECTIONS * 2;
}

// chunks [c_origin, c_stop) of n_streams x ch signals of in_len samples under a key of kp->key_ch channels, or the signals' own with key_ch = 0
// (absolute indexing); d_block: the key filter's constant block, unused with no section; d_state and d_fstate as the kernel's
int nae_launch_dynkey(nae_ctx* ctx, const nae_dynkey_params* kp, const double* d_block, const nae_sig* src, const nae_sig* key, size_t in_len, int ch,
                      size_t n_streams, const nae_sig* dst, size_t c_origin, size_t c_stop, double* d_state, double* d_fstate)
{
    if (c_stop <= c_origin || n_streams == 0) return NAE_OK;
    const DynParams p = nae_dyn_launch_params(&kp->dyn, in_len, ch, n_streams, c_origin, c_stop);
    const int key_ch = kp->key_ch ? kp->key_ch : ch, n_sections = kp->n_sections;
    const SigViewD kv = to_view(kp->key_ch ? key : src);
    const bool linked = kp->dyn.link && ch == 2;
    // one wave per detector; an unlinked detector hears one key channel
    return with_flags(linked, linked && key_ch == 2, n_sections > 0, [&](auto l, auto k2, auto filt) {
        if constexpr (!l.value && k2.value) return nae_fail(ctx, NAE_ERR_INVALID, "dynkey: no such kernel");
        else
            return nae_launch_tiles(ctx, "dynkey_kernel", "dynkey_kernel: grid too large", dynkey_kernel<l.value ? 2 : 1, k2.value ? 2 : 1, filt.value>,
                                    p.n_det, 1, 64, 0, to_view(src), kv, to_out(dst), p, key_ch, n_sections, d_block, d_state, d_fstate);
    });
}

extern "C" {

int nae_dynkey_block_f32(nae_ctx* ctx, const nae_dynkey_params* params, const nae_sig* src, const nae_sig* key, size_t in_len, int ch,
                         size_t n_streams, const nae_sig* dst)
{
    if (!ctx) return NAE_ERR_INVALID;
    if (!params || !src || !dst) return nae_fail(ctx, NAE_ERR_INVALID, "dynkey: null pointer");
    int rc = nae_dynkey_check(ctx, params, ch);
    if (rc) return rc;
    if ((params->key_ch == 0) != (key == nullptr)) return nae_fail(ctx, NAE_ERR_INVALID, "dynkey: a key view with key_ch = 0, or none with key_ch > 0");
    if (in_len == 0 || n_streams == 0) return NAE_OK;
    if (!src->base || !dst->base || (key && !key->base)) return nae_fail(ctx, NAE_ERR_INVALID, "dynkey: null pointer");
    // the key filter's tables are the context's, with nae_eq_block_f32's: a call with the coefficients of the last one uploads nothing
    double* d_block = nullptr;
    if (params->n_sections && (rc = nae_eq_cached_block(ctx, &params->coef[0][0], params->n_sections, &d_block))) return rc;
    return nae_launch_dynkey(ctx, params, d_block, src, key, in_len, ch, n_streams, dst, 0, nae_chunks(in_len), nullptr, nullptr);
}

} // extern "C"
