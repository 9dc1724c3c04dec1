// rb_queries.hpp -- what the queries (rb_queries.cpp) and the frame's post-processing (rb_frame.cpp) share: how a result
// leaves the device, how a caller's device buffer is checked, the scope of an engine-less form and a getter's read of a stage
// time.  Host code only; hidden: the library's dynamic symbols stay what they were.
#pragma once
#include "rb_engine.hpp"

#pragma GCC visibility push(hidden)
namespace rb {

inline bool page_locked(const void* p) {
    hipPointerAttribute_t attr{};
    if (p && hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost) return true;
    (void)hipGetLastError();   // an unregistered pointer makes the query fail: that is the ordinary case
    return false;
}

// device -> caller memory behind the stream's work: a DMA into page-locked memory, a blocking copy otherwise
inline int query_copy_out(rb_engine* e, void* dst, const void* src, size_t bytes, bool pinned) {
    if (pinned) {
        HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
        return RB_OK;
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RB_OK;
}

// the scene as a kernel of this module sees it, or the refusal of a traversal that its LDS stack column cannot hold
inline int scene_params(rb_engine* e, rb::KParams* p) {
    *p = make_params(e, 0, 0, e->cur, e->cur);
    if (!e->stack_depth_covers) return rb::fail(e, RB_ERR_DEVICE, "internal: a traversal is deeper than its LDS stack column (%u entries)", p->stack_depth);
    return RB_OK;
}

// rows of a frame of width w in one piece: whole 8-row tiles, about rb::kQueryPiece records, at least one band of tiles
inline uint32_t frame_piece_rows(uint32_t w) { return w == 0 ? 8u : std::max<uint32_t>(8u, (rb::kQueryPiece / w) & ~7u); }

// `bytes` of device memory of the engine's device at p, aligned to `align`?
inline int device_range(rb_engine* e, const void* p, size_t bytes, size_t align, const char* what) {
    hipPointerAttribute_t attr{};
    const hipError_t st = hipPointerGetAttributes(&attr, p);
    if (st != hipSuccess) (void)hipGetLastError();   // a pointer the runtime does not know: pageable host memory
    if (st != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != e->device)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s is not device memory of device %d", what, e->device);
    if (reinterpret_cast<uintptr_t>(p) % align != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s is not %zu-byte aligned", what, align);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: its allocation is unknown to the runtime", what);
    }
    const size_t off = static_cast<size_t>(static_cast<const char*>(p) - static_cast<const char*>(base));
    if (off > size || bytes > size - off) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: its allocation ends before %zu bytes", what, bytes);
    return RB_OK;
}

// The scope of an engine-less form: `device` made current (below 0: the current one stays) and a non-blocking stream of the
// call's own, with one sticky HIP status: once it is bad every member does nothing, so a call is its steps in order and none
// of them runs on a buffer that was not allocated.  It does not own the call's DevBufs: DECLARE IT AFTER THEM, so that on every
// path -- finish(), or the destructor where a return comes earlier -- the stream is synchronised before any of them is freed.
struct DeviceScope {
    hipStream_t stream = nullptr;
    hipError_t st = hipSuccess;
    int32_t refused = -1;   // the device hipSetDevice did not take
    explicit DeviceScope(int32_t device) {
        if (device >= 0 && hipSetDevice(device) != hipSuccess) {
            refused = device;
            st = hipErrorInvalidDevice;
        } else {
            st = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        }
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    ~DeviceScope() { close(); }
    bool ok() const { return st == hipSuccess; }
    template <class T>
    void alloc(rb::DevBuf<T>& buf, size_t count) {
        if (ok()) st = buf.resize(count);
    }
    void upload(void* dst, const void* src, size_t bytes) {
        if (ok() && bytes) st = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    }
    void download(void* dst, const void* src, size_t bytes) {
        if (ok() && bytes) st = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream);
    }
    // `launch()` queues kernels on `stream` and returns a HIP status.  A callable, not the status: the launch itself must not
    // happen once a step before it has failed.
    template <class Launch>
    void run(Launch&& launch) {
        if (ok()) st = static_cast<hipError_t>(launch());
    }
    void sync() {
        if (ok()) st = hipStreamSynchronize(stream);
    }
    void close() {
        if (!stream) return;
        const hipError_t s = hipStreamSynchronize(stream);   // whatever st is: the call's buffers are freed after this
        if (ok()) st = s;
        (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
    int finish(const char* who) {
        close();
        if (refused >= 0) return rb::fail(nullptr, RB_ERR_DEVICE, "hipSetDevice(%d) failed", refused);
        return ok() ? RB_OK : rb::fail(nullptr, RB_ERR_DEVICE, "%s failed: %s", who, hipGetErrorString(st));
    }
};

// A getter's read of one stage time, under the handle's lock: `t` is the engine that answers for the handle e -- e itself, or
// part 0 of a multi-device handle --, made current where the read has events to wait for
inline int stage_ms(rb_engine* e, rb_engine* t, StageTimer& timer, float* ms) {
    if (timer.pairs) set_device(t);
    HIP_TRY(e, timer.read(ms));
    return RB_OK;
}

// rb_frame.cpp, for rb_reproject_device: the refusals the forms of rb_reproject share
int reproject_check(rb_engine* e, const char* who, const rb_reproject_params* prm, uint32_t w, uint32_t h, const rb_view* view, const void* prev4,
                    const void* prev_guides, const void* cur_guides, const void* out4);

}  // namespace rb
#pragma GCC visibility pop
