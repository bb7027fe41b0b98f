// Host-only stand-in for the part of the HIP runtime that orb_slam_amd/csrc/orbx_host.h uses: allocations come from malloc, copies
// are memcpy, and `hip_stub_fail` makes the next n-th creating call fail.  `hip_stub_live` counts what is held; `hip_stub_device` is the
// current device (hip_stub_ndev of them), `hip_stub_waits` counts the waits on an event (by a stream or by the host).  `hip_stub_log` holds
// one letter per call, in order: m / f an allocation or creation made / freed, w the host waits for an event, s a stream waits for an event,
// r an event recorded, u / d an asynchronous copy up / down, y the host waits for a stream.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

typedef enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 } hipError_t;
typedef enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 } hipMemcpyKind;
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000, hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };

inline int hip_stub_fail = 0;      // 1: the next creating call fails, 2: the one after it, ...
inline int hip_stub_live = 0;
inline std::string hip_stub_log;
inline bool hip_stub_failing() { return hip_stub_fail > 0 && --hip_stub_fail == 0; }
inline hipError_t hip_stub_make(void** p, size_t bytes) {
    if (hip_stub_failing()) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    hip_stub_live++;
    hip_stub_log += 'm';
    return hipSuccess;
}
inline hipError_t hip_stub_free(void* p) { std::free(p); hip_stub_live--; hip_stub_log += 'f'; return hipSuccess; }

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_stub_make(p, bytes); }
inline hipError_t hipFree(void* p) { return hip_stub_free(p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_stub_make(p, bytes); }
inline hipError_t hipHostFree(void* p) { return hip_stub_free(p); }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
    if (hip_stub_failing()) return hipErrorOutOfMemory;
    *d = h;
    return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hip_stub_make(reinterpret_cast<void**>(s), 8); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_stub_free(s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hip_stub_make(reinterpret_cast<void**>(e), 8); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_stub_free(e); }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "hipErrorOutOfMemory"; }

inline int hip_stub_device = 0, hip_stub_ndev = 2, hip_stub_waits = 0;
inline hipError_t hipGetDevice(int* d) { *d = hip_stub_device; return hipSuccess; }
inline hipError_t hipSetDevice(int d) {
    if (d < 0 || d >= hip_stub_ndev) return hipErrorOutOfMemory;
    hip_stub_device = d;
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { hip_stub_log += 'r'; return e ? hipSuccess : hipErrorOutOfMemory; }
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { hip_stub_waits++; hip_stub_log += 's'; return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { hip_stub_waits++; hip_stub_log += 'w'; return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { hip_stub_log += 'y'; return hipSuccess; }
// the copy is done at once; the arguments of the last one up and of the last one down are kept
struct hip_stub_copy_t { void* dst; const void* src; size_t bytes; };
inline hip_stub_copy_t hip_stub_up, hip_stub_down;
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    std::memcpy(dst, src, bytes);
    (kind == hipMemcpyHostToDevice ? hip_stub_up : hip_stub_down) = {dst, src, bytes};
    hip_stub_log += kind == hipMemcpyHostToDevice ? 'u' : 'd';
    return hipSuccess;
}
