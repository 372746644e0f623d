// Resources of the synchronous host entry points (orbx.h's orbm_* / orbv_transform / stereo host
// calls).  Internal, not part of the C ABI.
//
// The reference calls ORBmatcher concurrently from Tracking, LocalMapping and LoopClosing, next to
// the two extractor threads (src/Frame.cc:94-103, src/LocalMapping.cc:215,268,
// src/LoopClosing.cc:265).  A host call therefore must not stall the other threads' streams: no
// hipMalloc / hipFree / hipDeviceSynchronize per call, no legacy null stream, and the caller's
// current device is restored on return.  Each call checks a context out of a process-wide pool
// (a non-blocking stream, a pinned staging buffer and a device buffer that only grow) and hands
// it back on return, so concurrent callers never share a stream and a warm pool allocates nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_pack.hpp"

namespace orbx {

// Valid HIP ordinal?
bool device_ok(int device);

// Switches the calling thread to `device` for one call and restores its current device after
// (an invalid ordinal switches nothing; the call reports ORBX_EDEVICE itself).
class DeviceGuard {
public:
    explicit DeviceGuard(int device)
    {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device && device_ok(device) && hipSetDevice(device) == hipSuccess)
            prev_ = cur;
    }
    ~DeviceGuard()
    {
        if (prev_ >= 0) hipSetDevice(prev_);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;

private:
    int prev_ = -1;
};

struct HostCtx;

// A block of a host call's layout: n elements of T at a byte offset both buffers share.
template <class T>
struct Blk {
    size_t off = 0, n = 0;
};
// An input block the wrapper fills itself, through HostCall::host().
template <class T>
struct Staged : Blk<T> {};

// One synchronous host call.  Usage:
//   HostCall c(device);                      // check a context out of the pool
//   auto a = c.in(src, n);                   // input block of n elements, copied from src
//   auto x = c.inout(ptr, n);                // input block that is also copied back to ptr by finish()
//   auto s = c.stage<T>(n);                  // input block the wrapper fills through host(s)
//   auto o = c.out<T>(n);                    // device-only blocks (outputs, scratch), after the inputs
//   c.begin();                               // size the buffers, fill the pinned inputs, H2D on the call's stream;
//                                            //   or prepare(), fill host(s) / patch in dev() pointers, upload()
//   launch ...(c.dev(a), c.dev(o, first), c.stream())
//   c.fetch(o, dst, n, first) ...; c.finish();   // D2H, stream sync, copy out
// An array states its type and length once, where its block is declared.  A block of no elements still
// reserves one slot that is never copied, so that every device pointer is a valid one.  Copies back are
// only queued (inout() blocks first, in the order declared, then the fetch() calls): a wrapper that returns
// before finish() writes nothing to the caller's arrays.
// Blocks are 64-byte aligned.  Blocks inside the pinned window go through pinned memory; larger
// layouts copy their tail blocks directly from / to the caller's memory, or, for a staged block, from a
// host-side copy of its own.
// A context's pinned buffer only grows; a replaced one is retired, not freed (hipHostFree waits for
// the whole device, which would stall every other thread's stream).
class HostCall {
public:
    explicit HostCall(int device);
    ~HostCall();
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

    orbx_status status() const { return st_; }
    hipStream_t stream() const;

    // src NULL with n > 0: an array the device call never reads.  Reserved and uploaded with whatever the pinned
    // buffer holds; past the pinned window prepare() cannot tell it from a stage() block and uploads zeros from a
    // host copy of its own.  A wrapper that fills a block itself declares it with stage().
    template <class T>
    Blk<T> in(const T* src, size_t n) { return {put(n ? src : nullptr, bytes<T>(n)), n}; }
    template <class T>
    Blk<T> inout(T* ptr, size_t n)
    {
        const Blk<T> b = in(ptr, n);
        fetch(b, ptr, n);
        return b;
    }
    template <class T>
    Staged<T> stage(size_t n) { return {{put(nullptr, bytes<T>(n)), n}}; }
    template <class T>
    Blk<T> out(size_t n) { return {reserve(bytes<T>(n)), n}; }

    orbx_status prepare();
    orbx_status upload();
    orbx_status begin() { return prepare() == ORBX_OK ? upload() : st_; }
    // the host copy of a staged block: never NULL after a successful prepare()
    template <class T>
    T* host(Staged<T> b) { return reinterpret_cast<T*>(staged_at(b.off)); }
    // device address of element `first` of a block
    template <class T>
    T* dev(Blk<T> b, size_t first = 0) const { return reinterpret_cast<T*>(at(b.off)) + first; }
    // queues the copy of elements [first, first + n) to dst (NULL: nothing)
    template <class T>
    void fetch(Blk<T> b, T* dst, size_t n, size_t first = 0)
    {
        if (first + n > b.n) st_ = ORBX_EINVAL;
        else get(b.off + sizeof(T) * first, dst, sizeof(T) * n);
    }
    orbx_status finish();

private:
    struct Block {
        size_t off, bytes;
        const void* src;
        int stage;   // index into staged_ for a source-less block past the pinned window, else -1
    };
    struct Fetch {
        size_t off, bytes;
        void* dst;
    };
    DeviceGuard guard_;
    HostCtx* ctx_ = nullptr;
    orbx_status st_ = ORBX_OK;
    size_t end_ = 0, in_end_ = 0;
    bool outs_started_ = false;
    std::vector<Block> ins_;
    std::vector<Fetch> fetches_;
    std::vector<std::vector<uint8_t>> staged_;
    size_t pin_ = 0;   // pinned window: blocks ending at or below it are staged through pinned memory
    bool queued_ = false;

    template <class T>
    static size_t bytes(size_t n) { return n ? sizeof(T) * n : 64; }
    size_t put(const void* src, size_t bytes);
    size_t reserve(size_t bytes);
    uint8_t* staged_at(size_t off);
    uint8_t* at(size_t off) const;
    void get(size_t off, void* dst, size_t bytes);
};

// run(scratch) with `bytes` of stream-ordered scratch, freed behind it on the stream; maps the last error
template <class Run>
orbx_status with_scratch(size_t bytes, hipStream_t s, Run run)
{
    void* scratch = nullptr;
    if (hipMallocAsync(&scratch, bytes, s) != hipSuccess) return ORBX_ENOMEM;
    run(scratch);
    hipFreeAsync(scratch, s);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
