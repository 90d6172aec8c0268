// Private to the host side of libphmm.so: the small utilities every host file shares (device guard, HIP status, exception
// guard), the grow-only staging buffer and device-only workspace of the entry points that stage their arrays themselves, the
// layout builder that declares each staged array once, and the round trip of such a call.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "phmm_host.hpp"
#include "phmm_region_internal.hpp"  // phmm_host::up256, the one rounding every layout uses

namespace phmm_host {

// Entry points leave the calling thread's current HIP device as they found it.
struct DeviceGuard {
    int prev = -1, dev;
    bool ok = true;
    explicit DeviceGuard(int device) : dev(device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

// A failure leaves its message and code in the handle -- or, without one (phmm_create), in what phmm_last_error(nullptr) returns.
void set_create_error(const std::string &msg);  // phmm_api.cpp
inline int set_error(phmm_handle *h, const std::string &msg, int code) {
    if (h) {
        h->err = msg;
        h->err_code = code;
    } else {
        set_create_error(msg);
    }
    return code;
}
inline bool hip_ok(phmm_handle *h, hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    (void)set_error(h, std::string(what) + ": " + hipGetErrorString(e), PHMM_ERR_HIP);
    return false;
}

// No C++ exception crosses the C ABI: every extern "C" body that can allocate runs inside PHMM_GUARD.
inline int on_exception(phmm_handle *h, const char *where, const char *what, int code) {
    return set_error(h, std::string(where) + ": " + what, code);
}
#define PHMM_GUARD_BEGIN try {
#define PHMM_GUARD_END(h, where, fail)                                                                    \
    }                                                                                                     \
    catch (const std::bad_alloc &) {                                                                      \
        (void)phmm_host::on_exception((h), (where), "out of host memory", PHMM_ERR_NO_MEMORY);            \
        return fail(PHMM_ERR_NO_MEMORY);                                                                  \
    }                                                                                                     \
    catch (const std::exception &e) {                                                                     \
        (void)phmm_host::on_exception((h), (where), e.what(), PHMM_ERR_INTERNAL);                         \
        return fail(PHMM_ERR_INTERNAL);                                                                   \
    }                                                                                                     \
    catch (...) {                                                                                         \
        (void)phmm_host::on_exception((h), (where), "unknown exception", PHMM_ERR_INTERNAL);              \
        return fail(PHMM_ERR_INTERNAL);                                                                   \
    }
#define PHMM_FAIL_CODE(c) (c)
#define PHMM_FAIL_NULL(c) nullptr

// Where the arrays of one call lie in a StagingBuffer: one statement per array gives its element type and count, in the order
// [inputs | device-only scratch | results].  Every slot starts on a 256-byte boundary and a zero-count slot takes no room, so
// one H2D copy covers [0, in_bytes) and one D2H copy [out_begin, total).  A DeviceScratch is laid out the same way, with
// scratch slots only.
class StageLayout {
    struct Copy {
        size_t off;
        const void *src;
        size_t bytes;
    };
    struct CopyBack {
        size_t off;
        void *dst;
        size_t bytes;
    };
    std::vector<Copy> copies;
    std::vector<CopyBack> copy_backs;
    bool has_out = false;
    template <class T>
    StageSlot<T> place(size_t count) {
        const StageSlot<T> s{total, count};
        total += up256(count * sizeof(T));
        return s;
    }

public:
    size_t in_bytes = 0, out_begin = 0, total = 0;
    template <class T>
    StageSlot<T> in(const T *src, size_t count) {  // copied into the mirror by stage()
        if (count) copies.push_back({total, src, count * sizeof(T)});
        return place<T>(count);
    }
    template <class T>
    StageSlot<T> in(size_t count) {  // an input the caller fills by hand (StagingBuffer::host_ptr)
        return place<T>(count);
    }
    void end_inputs() { in_bytes = total; }
    template <class T>
    StageSlot<T> scratch(size_t count) {  // device only, never copied back
        return place<T>(count);
    }
    template <class T>
    StageSlot<T> out(size_t count) {  // a result the caller cuts or scatters by hand (StagingBuffer::host_ptr)
        if (!has_out) out_begin = total;
        has_out = true;
        return place<T>(count);
    }
    template <class T>
    StageSlot<T> out(T *dst, size_t count) {  // copied from the mirror by hand_over(); a null dst is an array the caller did not ask for
        const StageSlot<T> s = out<T>(count);
        if (dst && count) copy_backs.push_back({s.off, dst, count * sizeof(T)});
        return s;
    }
    size_t out_bytes() const { return has_out ? total - out_begin : 0; }  // what the D2H copy covers: 0 = there is none
    void stage(char *host) const {
        for (const Copy &c : copies) memcpy(host + c.off, c.src, c.bytes);
    }
    void hand_over(const char *host) const {
        for (const CopyBack &c : copy_backs) memcpy(c.dst, host + c.off, c.bytes);
    }
};

// A result the kernels write whether or not the caller asked for it: in the staging layout L if `user` is given (handed over
// like any L.out(user, count), or left to the caller's own copy with by_hand), else in the device-only workspace D.
template <class T>
struct OptionalOut {
    StageSlot<T> slot;
    bool staged;
    T *dev_ptr(const StagingBuffer &W, const DeviceScratch &ws) const { return staged ? W.dev_ptr(slot) : ws.ptr(slot); }
};
template <class T>
OptionalOut<T> out_or_scratch(StageLayout &L, StageLayout &D, T *user, size_t count, bool by_hand = false) {
    if (!user) return {D.scratch<T>(count), false};
    return {by_hand ? L.out<T>(count) : L.out(user, count), true};
}

// The round trip of a call on stream S, in pieces: the inputs of L to the device, any byte range of W back, the wait.  A HIP
// failure leaves "<step> <what>" in the handle and returns false.
inline bool stage_upload(phmm_handle *h, const StagingBuffer &W, const StageLayout &L, hipStream_t S, const char *what) {
    const hipError_t e = hipMemcpyAsync(W.dev, W.host, L.in_bytes, hipMemcpyHostToDevice, S);
    return e == hipSuccess || hip_ok(h, e, ("H2D " + std::string(what)).c_str());
}
inline bool stage_fetch(phmm_handle *h, const StagingBuffer &W, size_t begin, size_t bytes, hipStream_t S, const char *what) {
    const hipError_t e = hipMemcpyAsync(W.host + begin, W.dev + begin, bytes, hipMemcpyDeviceToHost, S);
    return e == hipSuccess || hip_ok(h, e, ("D2H " + std::string(what)).c_str());
}
inline bool stage_wait(phmm_handle *h, hipStream_t S, const char *what) {
    const hipError_t e = hipStreamSynchronize(S);
    return e == hipSuccess || hip_ok(h, e, ("sync(" + std::string(what) + ")").c_str());
}
// ... the results of L back, if it declared any, and the wait
inline bool stage_download(phmm_handle *h, const StagingBuffer &W, const StageLayout &L, hipStream_t S, const char *what) {
    if (L.out_bytes() && !stage_fetch(h, W, L.out_begin, L.out_bytes(), S, what)) return false;
    return stage_wait(h, S, what);
}
// ... and the whole of it for a call of one round: upload, `launch` (which enqueues on S and returns false with the error set),
// download, and every L.out(ptr, count) handed to the caller.  Nothing is handed over when a step fails.
template <class Launch>
bool stage_round_trip(phmm_handle *h, const StagingBuffer &W, const StageLayout &L, hipStream_t S, const char *what, Launch &&launch) {
    if (!stage_upload(h, W, L, S, what) || !launch() || !stage_download(h, W, L, S, what)) return false;
    L.hand_over(W.host);
    return true;
}

// The likelihood matrices of the regions some event uses, one behind the other (phmm_genotype_likelihoods,
// phmm_annotate_events): where each starts (0 for a region no event uses) and how many values they are together.
struct LikelihoodGather {
    uint32_t n_regions;
    const uint32_t *region_read_off, *region_hap_off;
    const std::vector<char> &used;
    std::vector<uint64_t> off;
    uint64_t n = 0;
    LikelihoodGather(uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off, const std::vector<char> &used)
        : n_regions(n_regions), region_read_off(region_read_off), region_hap_off(region_hap_off), used(used), off(n_regions, 0) {
        for (uint32_t g = 0; g < n_regions; ++g) {
            if (!used[g]) continue;
            off[g] = n;
            n += cells(g);
        }
    }
    uint64_t cells(uint32_t g) const { return (uint64_t)(region_read_off[g + 1] - region_read_off[g]) * (region_hap_off[g + 1] - region_hap_off[g]); }
    // the matrices into `lk`, and the reads' keep flags into `kp`: all ones when the caller gives none
    void into(double *lk, uint8_t *kp, const uint64_t *out_off, const double *likelihoods, const uint8_t *keep) const {
        for (uint32_t g = 0; g < n_regions; ++g)
            if (used[g] && cells(g)) memcpy(lk + off[g], likelihoods + out_off[g], 8 * cells(g));
        const uint32_t n_reads = n_regions ? region_read_off[n_regions] : 0;
        if (keep && n_reads) memcpy(kp, keep, n_reads);
        else if (n_reads) memset(kp, 1, n_reads);
    }
};

// The PL rows of the computed events one behind the other (phmm_allele_frequency, phmm_assign_genotypes): the n_samples x G[i]
// values of event computed[i] start at off[i].
struct DensePls {
    const std::vector<uint32_t> &computed, &G;
    uint32_t n_samples;
    std::vector<uint64_t> off;
    uint64_t n = 0;
    DensePls(const std::vector<uint32_t> &computed, const std::vector<uint32_t> &G, uint32_t n_samples)
        : computed(computed), G(G), n_samples(n_samples), off(computed.size()) {
        for (size_t i = 0; i < computed.size(); ++i) {
            off[i] = n;
            n += (uint64_t)n_samples * G[i];
        }
    }
    void into(int32_t *dst, const uint64_t *pl_off, const int32_t *pl) const {
        for (size_t i = 0; i < computed.size(); ++i)
            if ((uint64_t)n_samples * G[i]) memcpy(dst + off[i], pl + pl_off[computed[i]], 4ull * n_samples * G[i]);
    }
};

}  // namespace phmm_host

// Room for `total` bytes in the buffer and in its mirror; `owner` names the buffer in the message of a failure.  Growing waits
// for the handle's streams first: an earlier call's copies may still read the old allocations.
inline bool StagingBuffer::grow(phmm_handle *h, size_t total, const char *owner) {
    if (cap >= total) return true;
    for (int i = 0; i < kSlots; ++i) (void)hipStreamSynchronize(h->streams[i]);
    release();
    const size_t bytes = std::max<size_t>(total + total / 2, 1 << 20);
    const std::string of = "(" + std::string(owner) + ")";
    if (!phmm_host::hip_ok(h, hipMalloc((void **)&dev, bytes), ("hipMalloc" + of).c_str()) ||
        !phmm_host::hip_ok(h, hipHostMalloc((void **)&host, bytes, hipHostMallocDefault), ("hipHostMalloc" + of).c_str()))
        return false;
    cap = bytes;
    return true;
}
inline void StagingBuffer::release() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = host_dev = nullptr;
    cap = 0;
}
// ... for a layout, whose inputs are then copied into the mirror
inline bool StagingBuffer::reserve(phmm_handle *h, const phmm_host::StageLayout &L, const char *owner) {
    if (!grow(h, L.total, owner)) return false;
    L.stage(host);
    return true;
}

// Room for the layout D, one and a half times the need and no floor; growing waits for the handle's streams like
// StagingBuffer::grow.  An empty layout on an empty workspace allocates nothing.
inline bool DeviceScratch::reserve(phmm_handle *h, const phmm_host::StageLayout &D, const char *owner) {
    if (cap >= D.total) return true;
    for (int i = 0; i < kSlots; ++i) (void)hipStreamSynchronize(h->streams[i]);
    release();
    const size_t bytes = D.total + D.total / 2;
    if (!phmm_host::hip_ok(h, hipMalloc((void **)&dev, bytes), ("hipMalloc(" + std::string(owner) + ")").c_str())) {
        dev = nullptr;
        return false;
    }
    cap = bytes;
    return true;
}
inline void DeviceScratch::release() {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
    cap = 0;
}
