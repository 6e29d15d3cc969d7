// launch.h — the launch layer of every kernel, once: the device views of a nae_sig, the dynamic-LDS attribute, the one launch (NAE_KLAUNCH and
// the launch's error stand here and nowhere else), the grid of the tiled kernels, the slices of a batch of streams, and the picks that turn a
// run-time frame size, format, channel count or flag into a compile-time one.  Every kernel file includes it (the STFT ones through stft_common.h).
#pragma once
#include "nae_internal.h"
#include <type_traits>

namespace nae {

// a nae_sig on the device: element (s, c, i) at base[s * ss + c * cs + i * fs].  A launch over a slice of the streams offsets `base`.
struct SigViewD { const float* base; long long ss, cs, fs; };
struct OutViewD { float* base; long long ss, cs, fs; };

inline SigViewD to_view(const nae_sig* s)
{
    return SigViewD{static_cast<const float*>(s->base), (long long)s->stream_stride, (long long)s->chan_stride, (long long)s->frame_stride};
}
inline OutViewD to_out(const nae_sig* s)
{
    return OutViewD{static_cast<float*>(s->base), (long long)s->stream_stride, (long long)s->chan_stride, (long long)s->frame_stride};
}

// More than 64 KiB of dynamic LDS needs the attribute: once per kernel and DEVICE, so the record of the kernels that have it
// (nae_ctx::lds_attr_done, by kernel address) lives in the context (no process-global launch state: contexts of different devices, or driven by
// different threads, do not share it).  Every instantiation is a kernel of its own, set at its own first launch; no kernel here is launched with
// two sizes above 64 KiB.
inline int nae_pv_lds_attr(nae_ctx* ctx, size_t lds, const void* kernel)
{
    for (const void* k : ctx->lds_attr_done)
        if (k == kernel) return NAE_OK;
    (void)nae_use_device(ctx);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return nae_check(ctx, e, "hipFuncSetAttribute(vocoder)");
    ctx->lds_attr_done.push_back(kernel);
    return NAE_OK;
}

// The one launch: the LDS attribute above 64 KiB, the launch under the profile name, and the launch's error, whose text is the profile name.
template <class K, class... A>
int nae_launch_grid(nae_ctx* ctx, const char* name, K kernel, dim3 grid, dim3 block, size_t lds, const A&... args)
{
    if (lds > 64 * 1024) {
        const int rc = nae_pv_lds_attr(ctx, lds, reinterpret_cast<const void*>(kernel));
        if (rc) return rc;
    }
    NAE_KLAUNCH(ctx, name, kernel, grid, block, lds, ctx->stream, args...);
    return nae_check(ctx, hipGetLastError(), name);
}

// A kernel that works on `items` pieces, `per_wg` of them per workgroup of `threads` threads with `lds` bytes of dynamic LDS: the grid and its
// bound (grid_err: the text of NAE_ERR_INVALID), then the one launch.  A site that launches nothing for zero items returns before it calls.
template <class K, class... A>
int nae_launch_tiles(nae_ctx* ctx, const char* name, const char* grid_err, K kernel, long long items, int per_wg, int threads, size_t lds,
                     const A&... args)
{
    const long long grid = (items + per_wg - 1) / per_wg;
    if (grid > 0x7fffffffll) return nae_fail(ctx, NAE_ERR_INVALID, grid_err);
    return nae_launch_grid(ctx, name, kernel, dim3((unsigned)grid), dim3(threads), lds, args...);
}

// Kernels whose grid is (tiles, streams): blockIdx.y holds at most 65535 entries, `group` streams each (1, or the 4 that share a workgroup), so
// a batch goes out in slices.  f(s0, ns) launches streams [s0, s0 + ns) on views moved there with at_stream; the first non-zero return ends
// the call, so no slice is launched behind a failed one.
template <typename F>
static int for_stream_slices(size_t n_streams, int group, F&& f)
{
    const size_t per_launch = (size_t)65535 * group;
    for (size_t s0 = 0; s0 < n_streams; s0 += per_launch) {
        const int rc = f(s0, n_streams - s0 < per_launch ? n_streams - s0 : per_launch);
        if (rc) return rc;
    }
    return NAE_OK;
}
inline SigViewD at_stream(SigViewD v, size_t s0) { v.base += (long long)s0 * v.ss; return v; }
inline OutViewD at_stream(OutViewD v, size_t s0) { v.base += (long long)s0 * v.ss; return v; }

// f(std::integral_constant<int, V>()) for the V of the list that equals v, else NAE_ERR_UNSUPPORTED with the text `none`: turns a run-time
// frame size or sample format into a compile-time one
template <int... Vs, typename F>
static int pick_value(nae_ctx* ctx, int v, const char* none, F&& f)
{
    int rc = NAE_OK;
    const bool hit = ((v == Vs ? (rc = f(std::integral_constant<int, Vs>()), true) : false) || ...);
    return hit ? rc : nae_fail(ctx, NAE_ERR_UNSUPPORTED, none);
}
// at the frame size N = n_fft of the vocoder, the FIR filter and the long convolution
template <typename F>
static int at_size(nae_ctx* ctx, int n_fft, F&& f)
{
    return pick_value<512, 1024, 2048, 4096>(ctx, n_fft, "vocoder: n_fft must be 512, 1024, 2048 or 4096", f);
}
// at the sample format of a frame that K6 converts (audio-velocity.cpp:223-228 refuses every other)
template <typename F>
static int at_format(nae_ctx* ctx, int fmt, F&& f)
{
    return pick_value<NAE_FMT_FLT, NAE_FMT_FLTP, NAE_FMT_S16, NAE_FMT_S16P, NAE_FMT_S32, NAE_FMT_S32P>(ctx, fmt, "Unsupported sample format", f);
}
// f(std::integral_constant<int, CH>()) for mono and stereo kernels: 2 is stereo, anything else the caller let through is mono
template <typename F>
static int with_channels(int ch, F&& f)
{
    return ch == 2 ? f(std::integral_constant<int, 2>()) : f(std::integral_constant<int, 1>());
}

// f(std::bool_constant<a>(), ...) for run-time flags a, ...: the variant pick of every launcher.  f is a generic lambda; a combination that has
// no kernel is refused in it with `if constexpr` (a nae_fail, not a launch), so it is never instantiated.
template <typename F>
static int with_flags(bool a, F&& f) { return a ? f(std::true_type()) : f(std::false_type()); }
template <typename F>
static int with_flags(bool a, bool b, F&& f)
{
    return with_flags(a, [&](auto ca) { return with_flags(b, [&](auto cb) { return f(ca, cb); }); });
}
template <typename F>
static int with_flags(bool a, bool b, bool c, F&& f)
{
    return with_flags(a, b, [&](auto ca, auto cb) { return with_flags(c, [&](auto cc) { return f(ca, cb, cc); }); });
}
template <typename F>
static int with_flags(bool a, bool b, bool c, bool d, F&& f)
{
    return with_flags(a, b, c, [&](auto ca, auto cb, auto cc) { return with_flags(d, [&](auto cd) { return f(ca, cb, cc, cd); }); });
}

} // namespace nae
