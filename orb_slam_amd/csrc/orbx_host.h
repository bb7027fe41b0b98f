// Host-side owners of the HIP resources behind the C ABI: device and pinned buffers, streams, events, the device scope and event chain of
// a handle, the scope of one call on a handle (Call), the layout of the block a handle keeps (Layout, Block), the path of a synchronous
// host form through that block (Staged), and the one-shot staging of the host forms without a handle (Staging).  Each owner releases
// what it holds when it goes out of scope, so an early return leaks nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <mutex>
#include <optional>
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
// a step that returns an ORBX status: anything but ORBX_OK is the function's own result
#define TRY(call) do { const int rc_ = (call); if (rc_ != ORBX_OK) return rc_; } while (0)

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
    // One piece of work, after begin(): recorded by end(), or when the scope is left early, so that the stream of the handle's next
    // call waits for whatever this one had enqueued.  (What the next call's host writes wait for is Block::busy's business.)
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
    // The caller's host array `src` of n elements as the kernels read it: copied into the slot of the pinned block h and named inside the
    // device block d.  An absent slot passes `src` through: an array the caller does not have (NULL) or keeps on the device.
    template <class T> static const T* put(void* h, void* d, Slot<T> s, const T* src, size_t n) {
        if (!s.present) return src;
        if (n) std::memcpy(at(h, s), src, n * sizeof(T));
        return at(d, s);
    }

  private:
    size_t total_ = 0, up_ = 0, down_ = 0;
};

// A pinned block and its device twin, kept by a handle and grown together: a failed grow leaves both empty, so the next call grows
// again and never pairs a block of the new size with a missing one.  busy: a call left while copies of the block were in flight.
struct Block {
    PinnedBuf h;
    DevBuf d;
    bool busy = false;
    bool fits(size_t host_bytes, size_t dev_bytes) const { return host_bytes <= h.size() && dev_bytes <= d.size(); }
    hipError_t ensure(size_t host_bytes, size_t dev_bytes) {
        hipError_t e = h.ensure(host_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = d.ensure(dev_bytes);
        if (e != hipSuccess) { h.reset(); d.reset(); }
        return e;
    }
};

// The size a kept buffer of `have` bytes grows to for `need`: doubled from 4096, so a slowly growing need allocates seldom.
inline size_t doubled(size_t have, size_t need) {
    size_t want = have > 4096 ? have : 4096;
    while (want < need) want *= 2;
    return want;
}

// One entry point's grip on a handle H (mu, device, own, chain, err): the handle's mutex and its device for the scope, the stream the call
// runs on (the caller's, or the handle's own), and from begin() on its link of the chain, which every way out of the scope records.
template <class H>
class Call {
    std::lock_guard<std::mutex> lk_;                                    // released last: after the chain is recorded and the device given back
    DeviceScope ds_;

  public:
    H* const m;
    const hipStream_t st;
    Call(H* h, void* stream) : lk_(h->mu), ds_(h->device), m(h), st(stream ? (hipStream_t)stream : (hipStream_t)h->own) {}
    bool ok() const { return ds_.ok; }                                  // the device could be selected
    // `st` waits for the handle's earlier work; an unselectable device is reported here, with nothing enqueued or recorded
    int begin() {
        if (!ok()) return ORBX_ERR_DEVICE;
        HIPCHK(m, m->chain.begin(st));
        link_.emplace(m->chain, st);
        return ORBX_OK;
    }
    // records the chain
    int end() {
        HIPCHK(m, link_->end());
        return ORBX_OK;
    }

  private:
    std::optional<Chain::Link> link_;                                   // left first
};

// A synchronous host form through the block `b` a handle keeps, laid out by `L`: fit() makes the block fit and hands out h and d, the
// caller fills the upload span (put()), and run(body) uploads [0, upload()), lets `body` enqueue the kernels, downloads
// [upload(), upload() + download()), records the chain and waits for the stream.  What lies behind the download span is device memory
// only.  The forms of a handle share one block: each holds the handle's mutex until it has synchronised, so no two are in flight.  A call
// that leaves between its upload and its synchronise marks the block busy, and the next fit() waits for the chain (which that call's link
// recorded) before the host writes into the pinned half again; in the steady state fit() waits for nothing and allocates nothing.
template <class H>
class Staged {
  public:
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    Staged(Call<H>& c, Block& b, const Layout& L) : c_(c), b_(b), up_(L.upload()), down_(L.download()), total_(L.total()) {}
    int fit() {
        H* m = c_.m;
        if (!c_.ok()) return ORBX_ERR_DEVICE;
        const bool grow = !b_.fits(up_ + down_, total_);
        if (grow || b_.busy) HIPCHK(m, m->chain.wait());                // device work that may still read or write the block
        b_.busy = false;
        if (grow) HIPCHK(m, b_.ensure(doubled(b_.h.size(), up_ + down_), doubled(b_.d.size(), total_)));
        h = b_.h.as();
        d = b_.d.as();
        return ORBX_OK;
    }
    template <class T> const T* put(Layout::Slot<T> s, const T* src, size_t n) const { return Layout::put(h, d, s, src, n); }
    // body() returns an ORBX status; anything but ORBX_OK ends the call there, with the chain recorded
    template <class Body> int run(Body body) {
        H* m = c_.m;
        int rc = c_.begin();
        if (rc != ORBX_OK) return rc;
        b_.busy = true;
        HIPCHK(m, hipMemcpyAsync(d, h, up_, hipMemcpyHostToDevice, c_.st));
        if ((rc = body()) != ORBX_OK) return rc;
        if (down_) HIPCHK(m, hipMemcpyAsync(h + up_, d + up_, down_, hipMemcpyDeviceToHost, c_.st));
        if ((rc = c_.end()) != ORBX_OK) return rc;
        HIPCHK(m, hipStreamSynchronize(c_.st));
        b_.busy = false;
        return ORBX_OK;
    }

  private:
    Call<H>& c_;
    Block& b_;
    const size_t up_, down_, total_;
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
