// kernels_spec_any.hip — K8 spectrum at every supported size: n_fft = 256 ... 4096 (powers of two), any hop 1 <= hop <= n_fft.
//
// The canonical FFT of DESIGN.md §3 ("K8 spectrum, every size") on M = n_fft/2 packed complex points, as an in-place
// decimation-in-frequency sequence of radix passes through a wave-private LDS scratch:
//   first pass radix R1 = 2, 4 or 8 (M = R1 * 8^s), twiddle W_M^(l q) on its outputs q >= 1;
//   then s radix-8 passes on blocks of MT = M / (R1 8^(t-1)) points, twiddle W_MT^(l q) = W512[(512/MT) l q] (none when MT = 8).
// At M = 512 this is the FFT512 of the 1024-point kernels pass for pass, so n_fft = 1024 gives their bits.
//
// Mapping: one wave = G = max(1, 512/M) consecutive frames of one (stream, channel); a 512-thread workgroup is 8 such waves that
// share only the W512 table in LDS.  A pass gives each lane G*M/(64 R) butterflies; its R inputs are read from the scratch (the first
// pass reads the windowed samples from memory instead) and its R outputs go back to the same positions, so a pass needs no buffer
// of its own and only a wave-level LDS ordering between passes.  Scratch position p lives at p + p/8: 8-byte accesses of the
// stride-64, stride-8 and stride-1 passes hit distinct banks.  LDS: 4 KiB + 8 x 9/8 x 512 x 8 B (n_fft <= 1024) ... 8 x 18 KiB
// (4096): 151 552 B (148 KiB) at 4096 = one workgroup, 2 waves per SIMD.  Hann_N and the split twiddles T_N are read through the caches
// (each element once per frame, coalesced); the first pass of M = 1024 / 2048 reads W_M likewise.
// Input reuse: a wave reads each of its frames' samples once; consecutive frames of a stream sit in neighbouring waves of one
// workgroup, so with hop < n_fft the shared samples are served by L2, not HBM.
#include "stft_common.h"
#include <math.h>

namespace nae {

constexpr int kAnyWaves = 8;
constexpr int kAnyThreads = 64 * kAnyWaves;

struct SpecAnyTables {
    const float* hann;   // Hann_N[n], n < N
    const cf* tn;        // T_N[k] = exp(-2 pi i k / N), k = 0..M
    const cf* wm;        // W_M[k], k < M (only read by the first pass when M > 512)
    const cf* w512;      // W512[k]
};

constexpr int ilog2c(int x) { return x <= 1 ? 0 : 1 + ilog2c(x / 2); }

template <int N>
struct SpecGeom {
    static constexpr int M = N / 2;
    static constexpr int kLog = ilog2c(M);
    static constexpr int R1 = kLog % 3 == 0 ? 8 : (1 << (kLog % 3));
    static constexpr int S8 = (kLog - ilog2c(R1)) / 3;      // radix-8 passes behind the first
    static constexpr int G = M >= 512 ? 1 : 512 / M;         // frames per wave
    static constexpr int BINS = M + 1;
    static constexpr int SCR = (G * M) + (G * M) / 8;        // padded scratch of one wave, complex
};

__device__ __forceinline__ int padx(int p) { return p + (p >> 3); }

__device__ __forceinline__ cf mul_mi_any(cf a) { return cf{a.y, -a.x}; }

template <int R>
__device__ __forceinline__ void dft_r(cf (&a)[R])
{
    if constexpr (R == 2) {
        const cf s = cf{a[0].x + a[1].x, a[0].y + a[1].y}, d = cf{a[0].x - a[1].x, a[0].y - a[1].y};
        a[0] = s;
        a[1] = d;
    } else if constexpr (R == 4) {
        // the inner layers of DFT8: two radix-2 DIF layers, natural-order output
        const cf s0 = cf{a[0].x + a[2].x, a[0].y + a[2].y}, d0 = cf{a[0].x - a[2].x, a[0].y - a[2].y};
        const cf s1 = cf{a[1].x + a[3].x, a[1].y + a[3].y};
        const cf d1 = mul_mi_any(cf{a[1].x - a[3].x, a[1].y - a[3].y});
        a[0] = cf{s0.x + s1.x, s0.y + s1.y};
        a[2] = cf{s0.x - s1.x, s0.y - s1.y};
        a[1] = cf{d0.x + d1.x, d0.y + d1.y};
        a[3] = cf{d0.x - d1.x, d0.y - d1.y};
    } else {
        dft8_fwd(a);
    }
}

// position of Z[k] after the passes: k = q1 + R1 k', k' with s octal digits -> q1 (M/R1) + (k' digit-reversed)
template <int N>
__device__ __forceinline__ int zpos(int k)
{
    using Gm = SpecGeom<N>;
    const int q1 = k & (Gm::R1 - 1);
    int kp = k >> ilog2c(Gm::R1), rev = 0;
#pragma unroll
    for (int t = 0; t < Gm::S8; t++) {
        rev = (rev << 3) | (kp & 7);
        kp >>= 3;
    }
    return q1 * (Gm::M / Gm::R1) + rev;
}

// how a frame's samples are addressed: frame stride 1 (8-byte pair loads), a stride whose offsets inside one frame fit 32 bits
// (a wave-uniform base plus an unsigned 32-bit lane offset: no 64-bit vector address arithmetic), or any stride
enum { kLoadUnit = 0, kLoadStride32 = 1, kLoadStride64 = 2 };

// first pass: windowed samples from memory -> radix R1 -> twiddle -> scratch
template <int N, int kLoad>
__device__ __forceinline__ void any_first_pass(cf* scr, const cf* w512l, const SpecAnyTables& tb, const ChanView& in,
                                               long long s0, long long hop, int nvalid, int lane)
{
    using Gm = SpecGeom<N>;
    constexpr int R = Gm::R1, S = Gm::M / R, BPL = Gm::G * Gm::M / (R * 64);
    static_assert(S % 64 == 0, "a first-pass butterfly row is whole waves: its frame is wave-uniform");
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int g = (64 * i) / S;                          // wave-uniform
        const int l = t & (S - 1);
        cf v[R];
        if (g < nvalid) {
            const float* p = in.p + (s0 + g * hop) * in.fs;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const int m = l + S * j;
                const float2 h = *reinterpret_cast<const float2*>(tb.hann + 2 * m);
                if (kLoad == kLoadUnit) {
                    const f2u x = *reinterpret_cast<const f2u*>(p + 2 * m);
                    v[j] = cf{x.x * h.x, x.y * h.y};
                } else if (kLoad == kLoadStride32) {
                    const unsigned fs = (unsigned)in.fs, o0 = (unsigned)(2 * m) * fs;
                    v[j] = cf{p[o0] * h.x, p[o0 + fs] * h.y};
                } else {
                    const long long fs = in.fs;
                    v[j] = cf{p[(2 * m) * fs] * h.x, p[(2 * m + 1) * fs] * h.y};
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < R; j++) v[j] = cf{0.0f, 0.0f};
        }
        dft_r<R>(v);
#pragma unroll
        for (int q = 1; q < R; q++) {
            const cf w = Gm::M > 512 ? tb.wm[l * q] : lds_ld(w512l + (512 / Gm::M) * l * q);
            v[q] = cmul_tw(v[q], w);
        }
        const int base = g * Gm::M + l;
#pragma unroll
        for (int j = 0; j < R; j++) lds_st(scr + padx(base + S * j), v[j]);
    }
}

// one radix-8 pass on blocks of MT points
template <int N, int MT>
__device__ __forceinline__ void any_pass8(cf* scr, const cf* w512l, int lane)
{
    using Gm = SpecGeom<N>;
    constexpr int S = MT / 8, BPL = Gm::G * Gm::M / 512;
    cf v[BPL][8];
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int base = (t / S) * MT + (t & (S - 1));
#pragma unroll
        for (int j = 0; j < 8; j++) v[i][j] = lds_ld(scr + padx(base + S * j));
    }
#pragma unroll
    for (int i = 0; i < BPL; i++) {
        const int t = lane + 64 * i;
        const int l = t & (S - 1);
        const int base = (t / S) * MT + l;
        dft8_fwd(v[i]);
        if (MT > 8) {
#pragma unroll
            for (int q = 1; q < 8; q++) v[i][q] = cmul_tw(v[i][q], lds_ld(w512l + (512 / MT) * l * q));
        }
#pragma unroll
        for (int j = 0; j < 8; j++) lds_st(scr + padx(base + S * j), v[i][j]);
    }
}

template <int N, int MT>
__device__ __forceinline__ void any_passes8(cf* scr, const cf* w512l, int lane)
{
    if constexpr (MT >= 8) {
        wave_lds_sync();
        any_pass8<N, MT>(scr, w512l, lane);
        any_passes8<N, MT / 8>(scr, w512l, lane);
    }
}

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

    any_first_pass<N, kLoad>(scr, w512l, tb, in, f0 * hop, hop, nvalid, lane);
    any_passes8<N, (Gm::M / Gm::R1)>(scr, w512l, lane);
    wave_lds_sync();

    // r2c split and magnitudes: output element o = g (M+1) + k, consecutive lanes -> consecutive addresses of one record
    float* out = dst + s * dst_ss + (f0 * ch + c) * (long long)Gm::BINS;
    constexpr int kOut = Gm::G * Gm::BINS;
#pragma unroll 4
    for (int o = lane; o < kOut; o += 64) {
        const int g = o / Gm::BINS, k = o - g * Gm::BINS;
        if (g >= nvalid) break;
        const cf* zf = scr + g * Gm::M + ((g * Gm::M) >> 3);       // padx(g M + p) = padx(g M) + padx(p): M is a multiple of 8
        const cf A = lds_ld(zf + padx(zpos<N>(k & (Gm::M - 1))));
        const cf B = lds_ld(zf + padx(zpos<N>((Gm::M - k) & (Gm::M - 1))));
        const cf E = cf{0.5f * (A.x + B.x), 0.5f * (A.y - B.y)};
        const cf O = cf{0.5f * (A.x - B.x), 0.5f * (A.y + B.y)};
        const cf P = cmul_tw(O, tb.tn[k]);
        const cf X = cf{E.x + P.y, E.y - P.x};
        out[(unsigned)(g * ch * Gm::BINS + k)] = __builtin_sqrtf(X.x * X.x + X.y * X.y);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
// table slot of a size that passed nae_spectrum_check: 256 -> 0 ... 4096 -> 4
static int spec_any_slot(int n_fft) { return ilog2c(n_fft) - 8; }

// Hann_N, T_N and W_M of one size: double, one rounding to f32; built on first use, freed with the context.
// n_fft = 1024 uses the context's own tables (the same formulas, built at creation).
static int spec_any_tables(nae_ctx* ctx, int n_fft, SpecAnyTables* tb)
{
    tb->w512 = ctx->d_w512;
    if (n_fft == NAE_FFT_N) {
        tb->hann = ctx->d_hann;
        tb->tn = ctx->d_t1024;
        tb->wm = ctx->d_w512;
        return NAE_OK;
    }
    const int slot = spec_any_slot(n_fft);
    nae_ctx::SpecAnyTab& t = ctx->spec_any_tab[slot];
    if (!t.hann) {
        const int M = n_fft / 2;
        const double two_pi = 6.283185307179586476925286766559;
        std::vector<float> hann(n_fft);
        std::vector<cf> tn(M + 1), wm(M);
        for (int n = 0; n < n_fft; n++) hann[n] = (float)(0.5 - 0.5 * cos(two_pi * n / (double)n_fft));
        for (int k = 0; k <= M; k++) tn[k] = cf{(float)cos(two_pi * k / (double)n_fft), (float)(-sin(two_pi * k / (double)n_fft))};
        for (int k = 0; k < M; k++) wm[k] = cf{(float)cos(two_pi * k / (double)M), (float)(-sin(two_pi * k / (double)M))};
        (void)nae_use_device(ctx);
        float* d_hann = nullptr;
        cf *d_tn = nullptr, *d_wm = nullptr;
        bool ok = hipMalloc((void**)&d_hann, n_fft * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&d_tn, (M + 1) * sizeof(cf)) == hipSuccess && hipMalloc((void**)&d_wm, M * sizeof(cf)) == hipSuccess;
        ok = ok && hipMemcpy(d_hann, hann.data(), n_fft * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d_tn, tn.data(), (M + 1) * sizeof(cf), hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(d_wm, wm.data(), M * sizeof(cf), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            if (d_hann) (void)hipFree(d_hann);
            if (d_tn) (void)hipFree(d_tn);
            if (d_wm) (void)hipFree(d_wm);
            return nae_fail(ctx, NAE_ERR_HIP, "spectrum tables: hipMalloc / hipMemcpy failed");
        }
        t.hann = d_hann;
        t.tn = d_tn;
        t.wm = d_wm;
    }
    tb->hann = t.hann;
    tb->tn = t.tn;
    tb->wm = t.wm;
    return NAE_OK;
}

template <int N, int kLoad>
static void launch_any_as(nae_ctx* ctx, const SigViewD& v, int ch, long long hop, long long F, long long n_groups, long long items,
                          float* dst, size_t dst_stream_stride, const SpecAnyTables& tb)
{
    // one item per wave (measured faster than waves walking items from a grid of 8 workgroups per CU: profiles/r07_spec_sizes.md);
    // a launch holds at most 2^22 workgroups (grid x block < 2^32 work-items), longer jobs take several
    constexpr long long kMaxItems = (1ll << 22) * kAnyWaves;
    for (long long item0 = 0; item0 < items; item0 += kMaxItems) {
        const long long n = items - item0 < kMaxItems ? items - item0 : kMaxItems;
        const unsigned grid = (unsigned)((n + kAnyWaves - 1) / kAnyWaves);
        NAE_KLAUNCH(ctx, "spectrum_any_kernel", (spectrum_any_kernel<N, kLoad>), dim3(grid), dim3(kAnyThreads), 0, ctx->stream, v, ch,
                    hop, F, n_groups, item0, items, dst, (long long)dst_stream_stride, tb);
    }
}

template <int N>
static void launch_any(nae_ctx* ctx, const nae_sig* src, int ch, long long hop, long long F, size_t n_streams, float* dst,
                       size_t dst_stream_stride, const SpecAnyTables& tb)
{
    constexpr int G = SpecGeom<N>::G;
    const long long n_groups = (F + G - 1) / G;
    const long long items = n_groups * (long long)n_streams * ch;
    const SigViewD v{static_cast<const float*>(src->base), (long long)src->stream_stride, (long long)src->chan_stride,
                     (long long)src->frame_stride};
    if (src->frame_stride == 1)
        launch_any_as<N, kLoadUnit>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
    else if ((unsigned long long)src->frame_stride * N < (1ull << 31))
        launch_any_as<N, kLoadStride32>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
    else
        launch_any_as<N, kLoadStride64>(ctx, v, ch, hop, F, n_groups, items, dst, dst_stream_stride, tb);
}

} // namespace nae

using namespace nae;

void nae_spec_any_free(nae_ctx* ctx)
{
    for (auto& t : ctx->spec_any_tab) {
        if (t.hann) (void)hipFree(t.hann);
        if (t.tn) (void)hipFree(t.tn);
        if (t.wm) (void)hipFree(t.wm);
        t = nae_ctx::SpecAnyTab{};
    }
}

int nae_launch_spectrum_any(nae_ctx* ctx, int n_fft, int hop, const nae_sig* src, size_t T, int ch, size_t n_streams, float* dst,
                            size_t dst_stream_stride)
{
    const size_t F = nae_spectrum_frames_ex(T, n_fft, hop);
    if (F == 0 || n_streams == 0) return NAE_OK;
    SpecAnyTables tb;
    const int rc = spec_any_tables(ctx, n_fft, &tb);
    if (rc) return rc;
    switch (n_fft) {
    case 256: launch_any<256>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb); break;
    case 512: launch_any<512>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb); break;
    case 1024: launch_any<1024>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb); break;
    case 2048: launch_any<2048>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb); break;
    case 4096: launch_any<4096>(ctx, src, ch, hop, (long long)F, n_streams, dst, dst_stream_stride, tb); break;
    default: return nae_fail(ctx, NAE_ERR_UNSUPPORTED, "spectrum: n_fft must be a power of two in [256, 4096]");   // (callers check first)
    }
    return nae_check(ctx, hipGetLastError(), "spectrum_any_kernel");
}
