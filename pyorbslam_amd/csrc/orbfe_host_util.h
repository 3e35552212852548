// orbfe_host_util.h — error plumbing, device buffers, launch timing and argument checks shared by the host
// translation units.  Header-only: tools/dbg/fuse_validate.hip links orbfe_fuse.hip alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/orbfe.h"

namespace orbfe {

// message of the last failed call on this thread (orbfe_last_error)
extern thread_local std::string g_err;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCK(expr)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            throw ::orbfe::Error(ORBFE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

template <class F>
int guarded(F&& f) {
    try {
        f();
        return ORBFE_OK;
    } catch (const Error& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "host allocation failed";
        return ORBFE_ENOMEM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return ORBFE_EINVAL;
    }
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void ensure(size_t count) {
        if (count <= n && p) return;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            throw Error(ORBFE_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        n = count;
    }
};

// Page-locked host buffer (hipHostMalloc): the per-frame results come back with asynchronous copies
// into it and one stream synchronisation.
template <class T>
struct HostBuf {
    T* p = nullptr;
    size_t n = 0;
    ~HostBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    void ensure(size_t count) {
        if (count <= n && p) return;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            throw Error(ORBFE_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        n = count;
    }
};

#pragma GCC visibility push(hidden)  // inline code of the host translation units from here on: not exported

// Device time of an entry's last call: two events around its launches on stream s,
//     begin(s); launches; end(s); ...; hipStreamSynchronize(s); last_ms = elapsed_ms();
// and, for an entry without a stream of the caller's, a non-blocking one of its own: get().  Stream and events are
// created on first use; an owner that only times another stream never calls get() and so never has a second
// stream.  A per-handle owner calls destroy() from its destructor; a process-wide one never does (the HIP runtime
// may already be gone when static destructors run).
struct TimedStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.f;  // what the entry's *_last_ms reports
    hipStream_t get() {
        if (!stream) HIPCK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return stream;
    }
    void begin(hipStream_t s) {
        for (hipEvent_t& e : ev)
            if (!e) HIPCK(hipEventCreate(&e));
        HIPCK(hipEventRecord(ev[0], s));
    }
    void end(hipStream_t s) { HIPCK(hipEventRecord(ev[1], s)); }
    float elapsed_ms() {  // after the stream was synchronised
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        return ms;
    }
    void destroy() {
        for (hipEvent_t& e : ev)
            if (e) (void)hipEventDestroy(e), e = nullptr;
        if (stream) (void)hipStreamDestroy(stream), stream = nullptr;
    }
};

inline bool all_finite(const double* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline std::string at_frame(int32_t f, const char* what) { return "frame " + std::to_string(f) + ": " + what; }

// bytes rounded up to a multiple of a (a power of two)
inline size_t pad_to(size_t bytes, size_t a) { return (bytes + a - 1) & ~(a - 1); }

// Ragged frames (frame f: features [off[f], off[f + 1]), nodes [fv_off[f], fv_off[f + 1]) of fv_node / fv_end, its
// fv_idx block at off[f]): the checks of frame f's feature vector.  Nodes ascend strictly, run ends do not decrease
// and stay within the frame, every feature index is in range and named once.  seen: scratch the caller keeps
// across frames.
inline void check_frame_runs(int32_t f, const int64_t* off, const int64_t* fv_off, const int32_t* fv_node,
                             const int32_t* fv_end, const int32_t* fv_idx, std::vector<uint8_t>& seen) {
    const int64_t n = off[f + 1] - off[f], nn = fv_off[f + 1] - fv_off[f];
    seen.assign((size_t)n, 0);
    int64_t prev_end = 0;
    for (int64_t r = 0; r < nn; ++r) {
        const int64_t at = fv_off[f] + r;
        if (r > 0 && fv_node[at] <= fv_node[at - 1])
            throw Error(ORBFE_EINVAL, at_frame(f, "feature vector nodes must be strictly ascending"));
        const int64_t end = fv_end[at];
        if (end < prev_end) throw Error(ORBFE_EINVAL, at_frame(f, "feature vector run ends must not decrease"));
        if (end > n) throw Error(ORBFE_EINVAL, at_frame(f, "a feature vector run ends past the index count"));
        if (end > prev_end && !fv_idx) throw Error(ORBFE_EINVAL, "null argument");
        for (int64_t k = prev_end; k < end; ++k) {
            const int32_t i = fv_idx[off[f] + k];
            if (i < 0 || i >= n) throw Error(ORBFE_EINVAL, at_frame(f, "a feature index is out of range"));
            if (seen[i]) throw Error(ORBFE_EINVAL, at_frame(f, "a feature index appears twice"));
            seen[i] = 1;
        }
        prev_end = end;
    }
}

// both frames that pair p names exist
inline void check_pair_frames(const int32_t* pairs, int32_t p, int32_t n_frames) {
    for (int s = 0; s < 2; ++s) {
        const int32_t f = pairs[2 * p + s];
        if (f < 0 || f >= n_frames)
            throw Error(ORBFE_EINVAL,
                        "pair " + std::to_string(p) + " names frame " + std::to_string(f) + ", which does not exist");
    }
}

#pragma GCC visibility pop

}  // namespace orbfe
