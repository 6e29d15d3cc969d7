// stream_util.h — grow-only device buffers, the absolutely indexed device FIFO of the streaming handles, and the handles' shared core: what
// a handle is (StreamHandle, BlockHandle) and its put / flush / available / receive / destroy (not installed).  Every handle of the library
// stands on it: the sixteen of nae_stream.hip, nae_wsola (nae_wsola.hip) and nae_swr (nae_swr.hip, whose convert entries feed and empty the
// FIFOs themselves)
#pragma once
#include "nae_internal.h"
#include <new>

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

// What every streaming handle is: a context, a channel count, an input and an output FIFO, the frames already handed out, and whether the
// flush has been seen.  The device allocations a handle makes through dev_alloc() are its own: the destructor frees them with the FIFOs, so
// a create that fails half way releases through the same routine as destroy.  process() computes what became computable after a put or
// the flush and is the one thing a handle must supply.
struct StreamHandle {
    nae_ctx* ctx = nullptr;
    int ch = 0;
    DevFifo in;                  // interleaved input, from the first sample the next launch still needs on
    DevFifo out;                 // result; elements [out_read, out.total) wait to be received
    size_t out_read = 0;
    size_t flush_tail = 0;       // zero frames the flush appends behind the input (the tail of an FIR)
    bool flushed = false;
    void* owned[3] = {};         // device allocations made by dev_alloc(): at most this many per handle (nae_dynkey, nae_echo and nae_loud make three)
    int n_owned = 0;

    virtual int process() = 0;
    virtual ~StreamHandle()
    {
        in.free();
        out.free();
        for (int i = 0; i < n_owned; i++) (void)hipFree(owned[i]);
    }

    // `count` elements of device memory that live as long as the handle
    template <class T>
    int dev_alloc(T** p, size_t count, const char* what)
    {
        if (n_owned == (int)(sizeof(owned) / sizeof(owned[0]))) return nae_fail(ctx, NAE_ERR_NOMEM, "dev_alloc: the handle's table of device allocations is full");
        if (hipMalloc((void**)p, count * sizeof(T)) != hipSuccess) return nae_fail(ctx, NAE_ERR_NOMEM, what);
        owned[n_owned++] = *p;
        return NAE_OK;
    }
};

// A block handle computes its output in whole units of U frames (a half FFT frame, a chunk) as the input fills them.
struct BlockHandle : StreamHandle {
    size_t done = 0;             // units computed

    // Runs the units that became computable, [done, ready): before the flush every whole unit with `wait` more frames behind it, after
    // the flush all the rest with the partial one at the end.  launch(src, dst, from, to) computes them from the absolutely indexed views
    // of the FIFOs; only when it succeeds do the output and `done` advance.  The last `keep` units of input stay in the FIFO (an
    // overlap-save block reads the half frame in front of it).
    template <class Launch>
    int run_units(size_t U, size_t wait, size_t keep, const Launch& launch)
    {
        const size_t ready = flushed ? (in.total + U - 1) / U : (in.total >= wait ? (in.total - wait) / U : 0);
        if (ready <= done) return NAE_OK;
        const size_t produced = flushed ? in.total : ready * U;
        int rc = out.reserve(ctx, produced);
        if (rc) return rc;
        const nae_sig src = in.view(), dst = out.view();
        rc = launch(src, dst, done, ready);
        if (rc) return rc;
        out.total = produced;
        done = ready;
        in.drop((long long)((ready - keep) * U));
        return NAE_OK;
    }
};

// a new handle of type H on `ctx` with interleaved FIFOs of `channels` floats per frame, `in_extra` more on the input side (channels that
// ride with the signal and do not come out: a key); nullptr when out of memory
template <class H>
static inline H* handle_new(nae_ctx* ctx, int channels, int in_extra = 0)
{
    H* h = new (std::nothrow) H();
    if (!h) return nullptr;
    h->ctx = ctx;
    h->ch = channels;
    h->out.width = (size_t)channels;
    h->in.width = (size_t)(channels + in_extra);
    return h;
}

static inline int handle_destroy(StreamHandle* h)
{
    if (!h) return NAE_OK;
    (void)nae_use_device(h->ctx);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
    return NAE_OK;
}

// the end of a create entry: hands the handle out, or releases it when a step after its construction failed
template <class H>
static inline int handle_created(H* h, int rc, H** out)
{
    if (rc) {
        (void)handle_destroy(h);
        return rc;
    }
    *out = h;
    return NAE_OK;
}

static inline int handle_append(StreamHandle* h, const float* p, size_t S, bool host)
{
    if (!h || (S && !p)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return nae_fail(h->ctx, NAE_ERR_STATE, "put after flush");
    if (S == 0) return NAE_OK;
    const int rc = h->in.push(h->ctx, p, S, host);
    return rc ? rc : h->process();
}

// the input ends here: flush_tail zero frames go in behind it, and process() releases everything that is left
static inline int handle_flush(StreamHandle* h)
{
    if (!h) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    if (h->flushed) return NAE_OK;
    if (const size_t tail = h->flush_tail) {
        const int rc = h->in.reserve(h->ctx, h->in.total + tail);
        if (rc) return rc;
        const hipError_t e = hipMemsetAsync(h->in.at(h->in.total), 0, tail * h->in.width * sizeof(float), h->ctx->stream);
        if (e != hipSuccess) return nae_check(h->ctx, e, "hipMemsetAsync(flush)");
        h->in.total += tail;
    }
    h->flushed = true;
    return h->process();
}

static inline size_t handle_available(const StreamHandle* h) { return h ? h->out.total - h->out_read : 0; }

static inline int handle_take(StreamHandle* h, float* dst, size_t max_frames, size_t* got, bool host)
{
    if (!h || !got || (max_frames && !dst)) return NAE_ERR_INVALID;
    (void)nae_use_device(h->ctx);
    size_t n = h->out.total - h->out_read;
    if (n > max_frames) n = max_frames;
    *got = n;
    if (n == 0) return NAE_OK;
    const int rc = h->out.pop(h->ctx, h->out_read, dst, n, host);
    if (rc) return rc;
    h->out_read += n;
    return NAE_OK;
}
