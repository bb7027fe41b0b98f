// Host-side owners of the HIP resources behind the C ABI: device and pinned buffers, streams, events, the device scope and event chain of
// a handle, the layout of the blocks a handle keeps, and the one-shot staging of the synchronous host forms.  Each owner releases what it
// holds when it goes out of scope, so an early return leaks nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include <vector>

#include "orbx.h"

// on failure: the handle's error text names the call, and the function returns ORBX_ERR_DEVICE
#define HIPCHK(h, call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return ORBX_ERR_DEVICE;                                                          \
        }                                                                                    \
    } while (0)
// the same for the entry points without a handle
#define HIPTRY(call) do { if ((call) != hipSuccess) return ORBX_ERR_DEVICE; } while (0)

// internal to the library: none of these types is exported
#pragma GCC visibility push(hidden)
namespace orbx {

// Move-only owner of one HIP resource, released with Release.  bytes_: the size of an allocation (0 for streams and events).
template <class T, hipError_t (*Release)(T)>
class Owner {
  public:
    Owner() = default;
    Owner(Owner&& o) noexcept { *this = std::move(o); }
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) { reset(); v_ = std::exchange(o.v_, nullptr); bytes_ = std::exchange(o.bytes_, 0); }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() { if (v_) (void)Release(v_); v_ = nullptr; bytes_ = 0; }
    T release() { bytes_ = 0; return std::exchange(v_, nullptr); }      // hands the resource to the caller
    operator T() const { return v_; }
    size_t size() const { return bytes_; }

  protected:
    // ensure(): create the resource unless one is held; it is owned only once `make` has succeeded
    template <class F> hipError_t take(F make) {
        T t = nullptr;
        const hipError_t e = v_ ? hipSuccess : make(&t);
        if (e == hipSuccess && t) v_ = t;
        return e;
    }
    T v_ = nullptr;
    size_t bytes_ = 0;
};

// ensure(bytes) grows the buffer only when it is too small, dropping the old contents.  The size is recorded once the new allocation
// has succeeded: a failed grow leaves an empty buffer of size 0.
struct DevBuf : Owner<void*, hipFree> {
    hipError_t ensure(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        reset();
        const hipError_t e = take([&](void** p) { return hipMalloc(p, bytes); });
        if (e == hipSuccess) bytes_ = bytes;
        return e;
    }
    template <class T = uint8_t> T* as() const { return static_cast<T*>(v_); }
};

// pinned host memory (hipHostMalloc flags); with hipHostMallocMapped, mapped() is its device address
struct PinnedBuf : Owner<void*, hipHostFree> {
    hipError_t ensure(size_t bytes, unsigned flags) {
        if (bytes <= bytes_) return hipSuccess;
        reset();
        hipError_t e = take([&](void** p) { return hipHostMalloc(p, bytes, flags); });
        if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer(&mapped_, v_, 0);
        if (e == hipSuccess) bytes_ = bytes;
        else reset();
        return e;
    }
    template <class T = uint8_t> T* as() const { return static_cast<T*>(v_); }
    template <class T = uint8_t> T* mapped() const { return v_ ? static_cast<T*>(mapped_) : nullptr; }

  private:
    void* mapped_ = nullptr;
};

// ensure() creates the stream (non-blocking) or event (no timing) unless it exists
struct Stream : Owner<hipStream_t, hipStreamDestroy> {
    hipError_t ensure() { return take([](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }); }
};
struct Event : Owner<hipEvent_t, hipEventDestroy> {
    hipError_t ensure() { return take([](hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }); }
};

// Selects a handle's device for one entry point and gives the caller's current device back.
struct DeviceScope {
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    int prev = -1;
    bool ok = false;
};

// Orders the device work on one handle across its callers' streams: begin(st) makes `st` wait for the work the last end() recorded
// (before any end(): nothing to wait for), end(st) records what `st` holds so far, wait() blocks the host on it.
struct Chain {
    Event ev;
    bool chained = false;
    hipError_t begin(hipStream_t st) const { return chained ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }
    hipError_t end(hipStream_t st) {
        const hipError_t e = hipEventRecord(ev, st);
        chained = chained || e == hipSuccess;
        return e;
    }
    hipError_t wait() const { return chained ? hipEventSynchronize(ev) : hipSuccess; }
    // One piece of work, after begin(): recorded by end(), or when the scope is left early, so that the handle's next call waits for
    // whatever this one had enqueued (a copy out of a pinned block, say) before it touches the same memory.
    struct Link {
        Link(Chain& c, hipStream_t st) : c_(&c), st_(st) {}
        ~Link() { if (c_) (void)c_->end(st_); }
        Link(const Link&) = delete;
        hipError_t end() { return std::exchange(c_, nullptr)->end(st_); }
      private:
        Chain* c_;
        hipStream_t st_;
    };
};

// The layout of a block a handle keeps: typed slots reserved in order, each at a multiple of 256 bytes (the alignment separate
// hipMalloc calls give) with room for max(n, 1) elements.  An absent slot takes no room and resolves to a null pointer.  The slots
// reserved before end_upload() are one copy up, those between it and end_download() one copy down.
class Layout {
  public:
    template <class T> struct Slot { size_t off = 0; bool present = false; };
    template <class T> Slot<T> add(size_t n, bool present = true) {
        const size_t off = total_;
        if (present) total_ = (off + (n > 0 ? n : 1) * sizeof(T) + 255) & ~(size_t)255;
        return {off, present};
    }
    void end_upload() { up_ = down_ = total_; }
    void end_download() { down_ = total_; }
    size_t upload() const { return up_; }                  // bytes [0, upload()) go up
    size_t download() const { return down_ - up_; }        // bytes [upload(), upload() + download()) come back
    size_t total() const { return total_; }
    // the slot inside a block that starts at `base` (pinned host or device memory)
    template <class T> static T* at(void* base, Slot<T> s) { return s.present ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + s.off) : nullptr; }

  private:
    size_t total_ = 0, up_ = 0, down_ = 0;
};

// A pinned block and its device twin, kept by a handle and grown together: a failed grow leaves both empty, so the next call grows
// again and never pairs a block of the new size with a missing one.
struct Block {
    PinnedBuf h;
    DevBuf d;
    bool fits(size_t host_bytes, size_t dev_bytes) const { return host_bytes <= h.size() && dev_bytes <= d.size(); }
    hipError_t ensure(size_t host_bytes, size_t dev_bytes) {
        hipError_t e = h.ensure(host_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = d.ensure(dev_bytes);
        if (e != hipSuccess) { h.reset(); d.reset(); }
        return e;
    }
};

// One-shot staging of a synchronous host form: the arrays live in ONE device allocation laid out by Layout.  in() / out() reserve an
// array; alloc() allocates and uploads the inputs; get() downloads; everything is freed with the object unless `buf` is moved to a
// longer-lived owner.  Empty copies are skipped.
class Staging {
  public:
    template <class T> using Slot = Layout::Slot<T>;
    template <class T> Slot<T> in(const T* src, size_t n) {
        ups_.push_back({layout_.total(), src, n * sizeof(T)});
        return out<T>(n);
    }
    template <class T> Slot<T> out(size_t n) { return layout_.add<T>(n); }
    hipError_t alloc() {
        hipError_t e = buf.ensure(layout_.total());
        for (const Up& u : ups_)
            if (e == hipSuccess && u.bytes) e = hipMemcpy(buf.as() + u.off, u.src, u.bytes, hipMemcpyHostToDevice);
        return e;
    }
    template <class T> T* operator[](Slot<T> s) const { return Layout::at(buf.as(), s); }
    template <class T> hipError_t get(T* dst, Slot<T> s, size_t n) const {
        return n ? hipMemcpy(dst, (*this)[s], n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
    DevBuf buf;

  private:
    struct Up { size_t off; const void* src; size_t bytes; };
    std::vector<Up> ups_;
    Layout layout_;
};

}  // namespace orbx
#pragma GCC visibility pop
