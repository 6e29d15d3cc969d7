// stream_util.h — grow-only device buffers and the absolutely indexed device FIFO of the streaming handles (not installed)
#pragma once
#include "nae_internal.h"

// grow-only device scratch; a grow does not keep the contents
struct DevBuf {
    float* p = nullptr;
    size_t cap = 0; // floats
};

static inline int devbuf_reserve(nae_ctx* ctx, DevBuf& b, size_t want)
{
    if (want <= b.cap) return NAE_OK;
    size_t cap = b.cap ? b.cap : 1 << 16;
    while (cap < want) cap *= 2;
    float* np = nullptr;
    (void)nae_use_device(ctx);
    if (hipMalloc((void**)&np, cap * sizeof(float)) != hipSuccess) return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(stream buffer)");
    if (b.p) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(b.p);
    }
    b.p = np;
    b.cap = cap;
    return NAE_OK;
}

static inline void devbuf_free(DevBuf& b)
{
    if (b.p) (void)hipFree(b.p);
    b = DevBuf{};
}

// A FIFO of device samples addressed by ABSOLUTE element index; elements [head, total) are live.  Element `base` sits at
// p[0], and `base` only ever takes a value a caller passed to drop(), so the absolute origin of a view keeps the alignment
// of the drop points (the tiled transposer stages 16-byte loads from multiples of 4 samples).
//   interleaved: element i is p[(i - base) * width .. + width)
//   planar:      channel c of element i is p[c * cap + (i - base)] (`width` rows of cap floats)
// drop() only records the new head.  When reserve() runs out of room, the live part moves to the front in place if the
// dead prefix is at least as long as it (the two regions of the copy then do not overlap), else into a buffer twice as
// large; either way base becomes head.
struct DevFifo {
    float* p = nullptr;
    size_t cap = 0;              // elements
    size_t base = 0, head = 0, total = 0;
    size_t width = 1;            // floats per element
    bool planar = false;

    float* at(size_t i) const { return p + (ptrdiff_t)(i - base) * (ptrdiff_t)(planar ? 1 : width); }
    // the absolutely indexed signal (element i of channel c at base + c * chan_stride + i * frame_stride)
    nae_sig view() const
    {
        return planar ? nae_sig{p - (ptrdiff_t)base, 0, cap, 1} : nae_sig{p - (ptrdiff_t)(base * width), 0, 1, width};
    }

    // the live elements from `head` on to dst (rows of dst_cap floats when planar)
    int move_live(nae_ctx* ctx, float* dst, size_t dst_cap) const
    {
        const size_t n = total - head, rows = planar ? width : 1, row = planar ? n : n * width;
        for (size_t r = 0; r < rows && n; r++) {
            hipError_t e = hipMemcpyAsync(dst + r * dst_cap, at(head) + r * cap, row * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) return nae_check(ctx, e, "hipMemcpyAsync(FIFO)");
        }
        return NAE_OK;
    }

    // room for elements up to want_total (absolute); the live part survives
    int reserve(nae_ctx* ctx, size_t want_total)
    {
        if (want_total <= base + cap) return NAE_OK;
        const size_t need = want_total - head;
        if (need <= cap && head - base >= total - head) {
            const int rc = move_live(ctx, p, cap);
            if (rc) return rc;
            base = head;
            return NAE_OK;
        }
        size_t ncap = cap ? 2 * cap : (((size_t)1 << 16) + width - 1) / width;    // first: 64 Ki floats
        while (ncap < need) ncap *= 2;
        (void)nae_use_device(ctx);
        float* np = nullptr;
        if (hipMalloc((void**)&np, ncap * width * sizeof(float)) != hipSuccess) return nae_fail(ctx, NAE_ERR_NOMEM, "hipMalloc(stream FIFO)");
        const int rc = move_live(ctx, np, ncap);
        if (rc) { (void)hipFree(np); return rc; }
        if (p) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(p);
        }
        p = np;
        cap = ncap;
        base = head;
        return NAE_OK;
    }

    // forget the elements below new_base (clamped to total)
    void drop(long long new_base)
    {
        if (new_base > (long long)total) new_base = (long long)total;
        if (new_base <= (long long)head) return;
        head = (size_t)new_base;
        if (head == total) base = head;      // nothing live: the next element goes to p[0]
    }

    // append n interleaved elements from device memory, or from host memory (waited for: the caller may reuse its buffer)
    int push(nae_ctx* ctx, const float* src, size_t n, bool host)
    {
        int rc = reserve(ctx, total + n);
        if (rc) return rc;
        hipError_t e = hipMemcpyAsync(at(total), src, n * width * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                                      ctx->stream);
        if (e != hipSuccess) return nae_check(ctx, e, "hipMemcpyAsync(put)");
        if (host && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return nae_check(ctx, e, "hipStreamSynchronize(put)");
        total += n;
        return NAE_OK;
    }

    // copy the n interleaved elements from `from` on out to device or host memory (waited for), then drop them
    int pop(nae_ctx* ctx, size_t from, float* dst, size_t n, bool host)
    {
        hipError_t e = hipMemcpyAsync(dst, at(from), n * width * sizeof(float), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                      ctx->stream);
        if (e != hipSuccess) return nae_check(ctx, e, "hipMemcpyAsync(receive)");
        if (host && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return nae_check(ctx, e, "hipStreamSynchronize");
        drop((long long)(from + n));
        return NAE_OK;
    }

    void free()
    {
        if (p) (void)hipFree(p);
        *this = DevFifo{};
    }
};
