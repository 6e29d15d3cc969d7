// ctx_mem.h — the device memory a context owns, once: CtxBuf, a grow-only allocation, and CtxConst, a device constant that is made again only
// when the host parameters it was made of differ from the last call's.  Every workspace, table and constant block of nae_ctx (and of the WSOLA
// plan cache and handle) is one of the two; the streaming handles' FIFOs are stream_util.h's (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/nae_gpu.h"

struct nae_ctx;
int nae_check(nae_ctx* ctx, hipError_t e, const char* what);
int nae_ctx_drain(nae_ctx* ctx);   // selects the context's device and waits for its stream (nae_api.hip)

// A grow-only device allocation on a context's device; a grow does not keep the contents.  One growth rule for every user: an eighth more than
// asked and a page (the conv ring at its 256 MiB cap must not grow by half again).  A grow waits for the context's stream (a launch in flight
// may still read the old block), frees, then allocates, so a failed grow leaves an empty buffer and never a stale pointer.  Freed with its owner:
// nae_ctx_destroy has selected the device and drained the stream before the context's members go.
struct CtxBuf {
    void* p = nullptr;
    size_t cap = 0;                 // bytes

    CtxBuf() = default;
    CtxBuf(const CtxBuf&) = delete;
    CtxBuf& operator=(const CtxBuf&) = delete;
    ~CtxBuf() { release(); }

    template <class T>
    T* as() const { return static_cast<T*>(p); }

    // room for want_bytes; `what` names the buffer in the error text "hipMalloc(what): ..." of NAE_ERR_NOMEM
    int reserve(nae_ctx* ctx, size_t want_bytes, const char* what)
    {
        if (p && want_bytes <= cap) return NAE_OK;
        const int rc = nae_ctx_drain(ctx);
        if (rc) return rc;
        release();
        const size_t bytes = want_bytes + want_bytes / 8 + 4096;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            char text[96];
            snprintf(text, sizeof text, "hipMalloc(%s)", what);
            (void)nae_check(ctx, e, text);
            return NAE_ERR_NOMEM;
        }
        cap = bytes;
        return NAE_OK;
    }

    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// A device constant with the host bytes it was made of: a call with the last call's key gets the device block as it stands — no wait, no
// upload, no launch.  The key is a short header of ints (a frame size, a channel layout) followed by a payload (taps, coefficients, a rate).
// A miss is the same for every user, in this order: the key is dropped, the block reserved, the context's stream waited for — a launch in
// flight may still read the last constant — then make() fills the block, and only when it succeeded is the new key kept.  Every make() ends in
// a wait for its upload, so the stream drains on a miss either way; the wait in front of it is meant, and is not each user's to repeat or omit.
struct CtxConst {
    CtxBuf dev;
    std::vector<unsigned char> key;   // header, then payload; empty: nothing valid on the device

    template <class T>
    T* as() const { return dev.as<T>(); }

    template <class Make>
    int get(nae_ctx* ctx, std::initializer_list<int> head, const void* payload, size_t payload_bytes, size_t dev_bytes, const char* what,
            const Make& make)
    {
        const size_t hb = head.size() * sizeof(int);
        if (dev.p && key.size() == hb + payload_bytes && (hb == 0 || memcmp(key.data(), head.begin(), hb) == 0) &&
            (payload_bytes == 0 || memcmp(key.data() + hb, payload, payload_bytes) == 0))
            return NAE_OK;
        key.clear();
        int rc = dev.reserve(ctx, dev_bytes, what);
        if (!rc) rc = nae_ctx_drain(ctx);
        if (!rc) rc = make();
        if (rc) return rc;
        key.resize(hb + payload_bytes);
        if (hb) memcpy(key.data(), head.begin(), hb);
        if (payload_bytes) memcpy(key.data() + hb, payload, payload_bytes);
        return NAE_OK;
    }
};
