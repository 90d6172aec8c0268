// C ABI (include/phmm.h) of the MI355X PairHMM engine: the launch planner is phmm_plan.cpp, this file places its plans and launches them.
//
// Host side of the drop-in boundary: takes the flattened (reads, haplotypes, quals) of any number
// of assembly regions, bins the regions into kernel shape classes <L lanes per pair, K haplotype
// columns per lane>, and launches one gfx950 kernel per class.  Replaces, for the whole batch,
//   PairHMM::initialize            (reference src/pair_hmm/pair_hmm.rs:63-125)   -> phmm_create / plan
//   PairHMM::compute_likelihoods   (:345-375)                                     -> phmm_compute
// There is no CPU fallback anywhere in this file.
#include "../../include/phmm.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <unordered_map>
#include <mutex>
#include <string>
#include <system_error>
#include <sched.h>
#include <thread>
#include <vector>

#include "phmm_cigar_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"
#include <sched.h>
#include "phmm_internal.hpp"
#include "phmm_plan.hpp"
#include "phmm_tables.hpp"

using namespace phmm;
using namespace phmm_host;
using namespace phmm_plan;

namespace {

std::mutex g_err_mu;
std::string g_create_err = "";
// phmm_submit / phmm_wait are the only entry points several threads may call on one handle, so their messages are kept
// per calling thread; every other entry point resets the pair.
thread_local std::string tl_err;
thread_local const phmm_handle *tl_err_h = nullptr;
thread_local bool tl_internal_create = false;  // phmm_create is making a lane / a backing handle (phmm_host::create_internal)
// the caller's own handles alive per device, and the shared handles their small calls are routed through (phmm_host::route_shared)
std::atomic<int> g_user_handles[kMaxDevices];
std::mutex g_backing_mu;
std::map<std::pair<int, unsigned>, phmm_handle *> g_backing;

// Chunked host path: batches whose per-base arrays exceed kOneShotBytes are cut into chunks of regions whose arrays grow
// from kFirstChunkBytes (the GPU starts early) to kChunkBytes (large launches are the efficient ones).  Measured on
// config-2 batches, one shot vs chunked: 32 regions 548 -> 479 us, 256 regions 4.36 -> 3.13 ms, 4096 regions 43.2 ms with
// 4 MB chunks vs 45.5 ms with 512 KB chunks throughout.  (PHMM_CHUNK_KB, PHMM_FIRST_CHUNK_KB, PHMM_ONESHOT_KB: tuning.)
static const size_t kChunkBytes = 4u << 20;
static const size_t kFirstChunkBytes = 512u << 10;
static const size_t kMixedFirstChunkBytes = 4u << 20;  // (swept in round 5, tools/hostpath_ragged_sweep.py: 4 / 8 / 8 / 7 MB was the best schedule)
static const size_t kMixedChunkBytes = 8u << 20;
static const size_t kOneShotBytes = 512u << 10;
static const size_t kStageInBytes = 640u << 10;
static const size_t kZeroCopyOutBytes = 160u << 10;
static const int kForcedEagerD2H = getenv("PHMM_EAGER_D2H") ? atoi(getenv("PHMM_EAGER_D2H")) : -1;
// (these six are tuning knobs of the host path, latched when the library is loaded; everything else is in Switches)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

void phmm_host::set_create_error(const std::string &msg) {
    std::lock_guard<std::mutex> g(g_err_mu);
    g_create_err = msg;
}

struct phmm_batch {
    phmm_handle *h = nullptr;
    uint64_t n_out = 0, read_bytes = 0, hap_bytes = 0;
    BatchPlan plan;  // what is launched (phmm_plan.hpp); below: where it lives on the device
    struct ClassDevice {  // of plan.classes[i]
        uint32_t *reads = nullptr;       // null: identity, or a chained class without a per-read kernel behind it
        uint64_t *pair_first = nullptr;  // generic only
        double *scratch = nullptr;       // generic only
    };
    std::vector<ClassDevice> class_dev;
    std::vector<ChainItem *> d_group_items;  // of plan.chain_groups[i]
    // device metadata (one allocation)
    uint32_t *d_read_region = nullptr, *d_region_read_off = nullptr, *d_region_hap_off = nullptr, *d_read_off = nullptr,
             *d_hap_off = nullptr, *d_status = nullptr;
    uint64_t *d_out_off = nullptr;
    uint8_t *d_redo = nullptr;  // [n_reads] f32-first mode: reads the f64 per-read kernel has to redo
    // payload
    const uint8_t *d_read_bases = nullptr, *d_base_q = nullptr, *d_ins_q = nullptr, *d_del_q = nullptr, *d_gcp = nullptr,
                  *d_hap_bases = nullptr;
    double *d_out = nullptr;
    void *d_owned = nullptr;  // batch-owned payload + out (phmm_batch_upload)
    Arena *arena = nullptr;   // non-null: every device allocation of this batch lives in the handle's arena
    hipStream_t home_stream = nullptr;  // the handle stream this batch was staged on
    std::vector<void *> mallocs;  // hipMalloc'ed pieces owned by this batch (persistent batches, generic scratch)
    size_t out_arena_off = 0;     // arena mode: offset of [status word | out]
    bool tight_out = true;        // out_off has no gaps (every slot is written by a kernel)
    std::vector<std::pair<uint64_t, uint64_t>> out_extents;  // !tight_out: (first slot, Nr*Nh) per region -- gaps stay untouched
    double *rescue_scratch = nullptr;  // non-null: the exact pass rides behind every launch (persistent batches: own
                                       // scratch; engine-level call: the arena's, its results are consumed on the device)
    uint32_t rescue_blocks = 0;
    bool bound = false;
};

#define HIP_TRY(h, call, ret)                  \
    do {                                       \
        if (!hip_ok((h), (call), #call)) return ret; \
    } while (0)

// The one place the PHMM_* developer switches are read (phmm_set_switch changes them per handle afterwards): phmm_create,
// and phmm_plan_describe, so that a described plan is the plan an engine of this process makes.
static void read_env_switches(Switches &w) {
    auto env = [](const char *name, int &dst) {
        if (const char *e = getenv(name)) dst = atoi(e);
    };
    env("PHMM_FORCE_L", w.force_L);
    env("PHMM_FORCE_CHAIN", w.force_chain);
    env("PHMM_FORCE_STREAMS", w.force_streams);
    env("PHMM_SW_LITE", w.sw_lite);
    env("PHMM_SW_CHUNKS", w.sw_chunks);
    env("PHMM_SW_LANES", w.sw_lanes);
    env("PHMM_SW_TRANSPOSE", w.sw_transpose);
    env("PHMM_REGION_SW_ALL", w.region_sw_all);
    env("PHMM_REGION_SERVER", w.region_server);
    env("PHMM_SERVER_IDLE_US", w.server_idle_us);
    env("PHMM_SERVER_TRACE", w.server_trace);
    env("PHMM_REGION_FLAG_WAIT", w.region_flag_wait);
    env("PHMM_REGION_OWN_QUEUE", w.region_own_queue);
    env("PHMM_REGION_PICK_TIMEOUT_US", w.region_pick_timeout_us);
    env("PHMM_REGION_DEBUG_PICK", w.region_debug_pick);
    env("PHMM_MIRROR_CANARY", w.mirror_canary);
    env("PHMM_ROUTE_SHARED", w.route_shared);
    w.sw_no_zero_copy = getenv("PHMM_SW_NO_ZERO_COPY") != nullptr;
    w.sw_clock = getenv("PHMM_SW_CLOCK") != nullptr;
    w.no_pipeline = getenv("PHMM_NO_PIPELINE") != nullptr;
    w.no_rescue = getenv("PHMM_NO_RESCUE") != nullptr;
    w.trace = getenv("PHMM_TRACE") != nullptr;
}

extern "C" {

int phmm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *phmm_last_error(phmm_handle *h) {
    if (h && tl_err_h == h) return tl_err.c_str();
    if (h) return h->err.c_str();
    std::lock_guard<std::mutex> g(g_err_mu);
    return g_create_err.c_str();
}

phmm_handle *phmm_create(int device_id, unsigned flags) {
    int n = phmm_device_count();
    if (device_id < 0 || device_id >= n || device_id >= kMaxDevices) {
        set_create_error("phmm_create: no HIP device with that id (this engine has no CPU fallback)");
        return nullptr;
    }
    DeviceGuard dg(device_id);
    if (!dg.ok && !hip_ok(nullptr, hipErrorInvalidDevice, "hipSetDevice")) return nullptr;
    PHMM_GUARD_BEGIN
    phmm_handle *h = new phmm_handle();
    h->device = device_id;
    h->flags = flags;
    h->internal = tl_internal_create;
    if (!h->internal) g_user_handles[device_id].fetch_add(1, std::memory_order_relaxed);
    phmm_host::handle_born(h);
    read_env_switches(h->sw);
    const auto &eps = table_eps();
    const auto &eps3 = table_eps_third();
    const auto &mm = table_match_to_match();
    bool ok = true;
    // (slot 0 -- the stream of every call that is one enqueue -- is a hardware queue of the handle's own where the device's pool
    // has one left: phmm_region.cpp, queues_acquire)
    for (int i = 0; i < kSlots && ok; ++i)
        ok = hip_ok(nullptr, hipStreamCreateWithFlags(&h->streams[i], hipStreamNonBlocking), "hipStreamCreate");
    h->stream0_ordinary = h->streams[0];
    ok = ok &&
              hip_ok(nullptr, hipMalloc(&h->d_eps, 256 * sizeof(double)), "hipMalloc eps") &&
              hip_ok(nullptr, hipMalloc(&h->d_eps_mis, 256 * sizeof(double)), "hipMalloc eps_mis") &&
              hip_ok(nullptr, hipMalloc(&h->d_mm, mm.size() * sizeof(double)), "hipMalloc mm") &&
              hip_ok(nullptr, hipMemcpy(h->d_eps, eps.data(), 256 * sizeof(double), hipMemcpyHostToDevice), "copy eps") &&
              hip_ok(nullptr,
                     hipMemcpy(h->d_eps_mis, (flags & PHMM_FLAG_NO_TRISTATE) ? eps.data() : eps3.data(),
                               256 * sizeof(double), hipMemcpyHostToDevice),
                     "copy eps_mis") &&
              hip_ok(nullptr, hipMemcpy(h->d_mm, mm.data(), mm.size() * sizeof(double), hipMemcpyHostToDevice), "copy mm");
    if (ok) {  // derived tables of the pre-scaled row form (phmm_device.hpp, RowConst)
        std::vector<double> ratio(256, 0.0), inv_om(256, 0.0);
        const auto &mis = (flags & PHMM_FLAG_NO_TRISTATE) ? eps : eps3;
        for (int q = 1; q < 256; ++q) {
            ratio[q] = mis[q] / (1.0 - eps[q]);
            inv_om[q] = 1.0 / (1.0 - eps[q]);
        }
        ok = hip_ok(nullptr, hipMalloc(&h->d_ratio_mis, 256 * sizeof(double)), "hipMalloc ratio_mis") &&
             hip_ok(nullptr, hipMalloc(&h->d_inv_om, 256 * sizeof(double)), "hipMalloc inv_om") &&
             hip_ok(nullptr, hipMemcpy(h->d_ratio_mis, ratio.data(), 256 * sizeof(double), hipMemcpyHostToDevice), "copy ratio_mis") &&
             hip_ok(nullptr, hipMemcpy(h->d_inv_om, inv_om.data(), 256 * sizeof(double), hipMemcpyHostToDevice), "copy inv_om");
    }
    if (ok) {
        std::vector<unsigned char> all(4 * 128, 0);
        for (int m = 1; m <= 3; ++m) {
            const auto c = pcr_error_model_cache(m);
            std::copy(c.begin(), c.end(), all.begin() + m * 128);
        }
        ok = hip_ok(nullptr, hipMalloc((void **)&h->d_pcr_cache, all.size()), "hipMalloc pcr") &&
             hip_ok(nullptr, hipMemcpy(h->d_pcr_cache, all.data(), all.size(), hipMemcpyHostToDevice), "copy pcr");
    }
    if (!ok) {
        phmm_destroy(h);
        return nullptr;
    }
    return h;
    PHMM_GUARD_END(nullptr, "phmm_create", PHMM_FAIL_NULL)
}

void phmm_destroy(phmm_handle *h) {
    if (!h) return;
    if (h->comb) phmm_host::combiner_destroy(h->comb);
    DeviceGuard dg(h->device);
    h->streams[0] = h->stream0_ordinary;
    phmm_host::queues_release(h);
    phmm_host::handle_died(h);
    for (int i = 0; i < kSlots; ++i)
        if (h->streams[i]) (void)hipStreamDestroy(h->streams[i]);
    if (h->d_eps) (void)hipFree(h->d_eps);
    if (h->d_eps_mis) (void)hipFree(h->d_eps_mis);
    if (h->d_mm) (void)hipFree(h->d_mm);
    if (h->d_ratio_mis) (void)hipFree(h->d_ratio_mis);
    if (h->d_inv_om) (void)hipFree(h->d_inv_om);
    if (h->d_pcr_cache) (void)hipFree(h->d_pcr_cache);
    for (int i = 0; i < kSlots; ++i) {
        if (h->arenas[i].dev) (void)hipFree(h->arenas[i].dev);
        if (h->arenas[i].host) (void)hipHostFree(h->arenas[i].host);
        if (h->arenas[i].rescue) (void)hipFree(h->arenas[i].rescue);
    }
    for (StagingBuffer *b : {&h->swork.staging, &h->gwork.staging, &h->af_staging, &h->annotate_staging, &h->assign_staging, &h->events_staging, &h->activity_staging, &h->finalize_staging, &h->phase_staging, &h->asm_staging, &h->graph_staging, &h->prune_staging, &h->recover_staging, &h->seqgraph_staging, &h->paths_staging, &h->trim_staging, &h->regions_staging, &h->regions_out_staging, &h->regions_reads_staging}) b->release();
    for (DeviceScratch *b : {&h->events_scratch, &h->activity_scratch, &h->finalize_scratch, &h->phase_scratch, &h->asm_scratch, &h->prune_scratch, &h->recover_scratch, &h->seqgraph_scratch, &h->paths_scratch, &h->paths_table}) b->release();
    if (h->swork.slab) (void)hipFree(h->swork.slab);
    if (h->swork.ws) (void)hipFree(h->swork.ws);
    if (h->swork.ext) (void)hipFree(h->swork.ext);
    if (h->gwork.d_jacobian) (void)hipFree(h->gwork.d_jacobian);
    for (int c = 0; c < phmm_handle::SwWork::kMaxChunks; ++c)
        for (hipEvent_t e : {h->swork.ev_in[c], h->swork.ev_out[c], h->swork.ev_k0[c], h->swork.ev_k1[c]})
            if (e) (void)hipEventDestroy(e);
    if (h->swork.region_sw_done) (void)hipEventDestroy(h->swork.region_sw_done);
    if (h->swork.ev_second) (void)hipEventDestroy(h->swork.ev_second);
    if (h->swork.d_pair_done) (void)hipFree(h->swork.d_pair_done);
    phmm_host::halves_release(h);
    for (int i = 0; i < 2; ++i) {
        if (h->swork.all_stream[i]) (void)hipStreamDestroy(h->swork.all_stream[i]);
        if (h->swork.pair_main[i]) (void)hipStreamDestroy(h->swork.pair_main[i]);
    }
    for (int i = 0; i < phmm_handle::kSideStreams; ++i) {
        if (h->side_streams[i]) (void)hipStreamDestroy(h->side_streams[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    const bool internal = h->internal;
    const int device = h->device;
    delete h;
    if (internal) return;
    // The count reaching zero and the backing handles leaving the map are ONE step under the map's lock (route_shared looks
    // them up under the same lock): a handle created after this step finds no entry and makes its own backing handle; one
    // created before it keeps the count above zero.
    std::vector<phmm_handle *> gone;
    bool last_of_the_callers = false;
    {
        std::lock_guard<std::mutex> lk(g_backing_mu);
        last_of_the_callers = g_user_handles[device].fetch_sub(1, std::memory_order_acq_rel) == 1;
        if (last_of_the_callers) {
            for (auto it = g_backing.begin(); it != g_backing.end();) {
                if (it->first.first == device) {
                    gone.push_back(it->second);
                    it = g_backing.erase(it);
                } else {
                    ++it;
                }
            }
        }
    }
    if (last_of_the_callers) {  // nobody is left to route: the device's backing handles go too
        for (phmm_handle *b : gone) phmm_destroy(b);
        phmm_host::server_quiesce(device);  // (the region server leaves the chip by itself once idle: wait for that)
    }
}

size_t phmm_table_eps(const double **eps) {
    *eps = table_eps().data();
    return table_eps().size();
}
size_t phmm_table_match_to_match(const double **mm) {
    *mm = table_match_to_match().data();
    return table_match_to_match().size();
}

void phmm_batch_destroy(phmm_batch *b) {
    if (!b) return;
    DeviceGuard dg(b->h->device);
    for (void *m : b->mallocs) (void)hipFree(m);
    delete b;
}

}  // extern "C"

namespace phmm_host {

void set_thread_error(const phmm_handle *h, const std::string &msg) {
    tl_err = msg;
    tl_err_h = h;
}
void clear_thread_error(const phmm_handle *h) {
    if (tl_err_h == h) tl_err_h = nullptr;
}

phmm_handle *create_internal(int device, unsigned flags) {
    struct Mark {
        bool prev = tl_internal_create;
        Mark() { tl_internal_create = true; }
        ~Mark() { tl_internal_create = prev; }
    } mark;
    return phmm_create(device, flags);
}

int user_handles_on(int device) { return g_user_handles[device % kMaxDevices].load(std::memory_order_relaxed); }

// The wait of a one-shot call.  hipStreamSynchronize spins; with more caller threads than the process has cores -- its affinity
// mask or its container's CPU quota: 16 of 256 on the GPU box -- the spinning waiters are throttled together with the callers
// that have something to stage, and 32 private handles ran at HALF the rate of 16 (phmm_compute 46 -> 22 k regions/s, VERDICT r4;
// round 5 hid it by routing such handles through the shared combiner; the region server's waiters showed the same: 22.9 k
// spinning, 45.6 k with short sleeps, NOTEBOOK 20.2).  So: when the caller holds more handles on the device than it has cores,
// look at the stream, sleep 20 us, look again: 24 / 32 handles 31 / 22 -> 46 / 45 k, nothing routed, nothing combined.
int process_cores() {
    static const int cores = [] {
        cpu_set_t set;
        CPU_ZERO(&set);
        int n = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // (a container's CPU quota: spinning beyond it is throttled)
            long long quota = 0, period = 0;
            if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) n = std::min<int>(n, (int)((quota + period - 1) / period));
            fclose(f);
        }
        return n > 0 ? n : 1;
    }();
    return cores;
}
bool more_callers_than_cores(const phmm_handle *h) { return !h->internal && user_handles_on(h->device) > process_cores(); }
hipError_t wait_stream(const phmm_handle *h, hipStream_t s) {
    if (!more_callers_than_cores(h)) return hipStreamSynchronize(s);
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

phmm_handle *route_shared(phmm_handle *h) {
    // (opt-in since round 6: which regions share a flush depends on timing, so routed results are reproducible to ~1e-13, not bit
    // for bit -- the default for many private handles is the region server, whose results never depend on the load)
    if (h->internal || h->sw_touched || h->comb || h->sw.route_shared <= 0) return nullptr;
    const int above = h->sw.route_shared;
    if (g_user_handles[h->device].load(std::memory_order_relaxed) <= above) return nullptr;
    if (h->backing) return h->backing;  // (lives as long as one of the caller's handles does on the device: at least as long as h)
    std::lock_guard<std::mutex> lk(g_backing_mu);
    phmm_handle *&b = g_backing[{h->device, h->flags}];
    if (!b) {
        b = create_internal(h->device, h->flags);
        if (!b) {
            g_backing.erase({h->device, h->flags});
            return nullptr;  // (no memory for another engine: the call stays where it is)
        }
    }
    return h->backing = b;
}

const char *validate_offsets(uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                             const uint32_t *read_off, const uint32_t *hap_off, const uint64_t *out_off, bool *tight_out) {
    if (!region_read_off || !region_hap_off || !read_off || !hap_off || !out_off) return "phmm_batch_create: null offset array";
    if (region_read_off[0] != 0 || region_hap_off[0] != 0 || read_off[0] != 0 || hap_off[0] != 0 || out_off[0] != 0)
        return "phmm_batch_create: offset arrays must start at 0";
    const uint32_t n_reads = region_read_off[n_regions], n_haps = region_hap_off[n_regions];
    bool tight = true;
    for (uint32_t g = 0; g < n_regions; ++g) {
        if (region_read_off[g + 1] < region_read_off[g] || region_hap_off[g + 1] < region_hap_off[g])
            return "phmm_batch_create: region offsets not monotonic";
        const uint64_t need = (uint64_t)(region_read_off[g + 1] - region_read_off[g]) *
                              (uint64_t)(region_hap_off[g + 1] - region_hap_off[g]);
        if (out_off[g + 1] < out_off[g] || out_off[g + 1] - out_off[g] < need)
            return "phmm_batch_create: out_off leaves too little room for a region (needs Nr*Nh doubles)";
        if (out_off[g + 1] - out_off[g] != need) tight = false;
    }
    for (uint32_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r]) return "phmm_batch_create: read_off not monotonic";
    for (uint32_t a = 0; a < n_haps; ++a) {
        if (hap_off[a + 1] < hap_off[a]) return "phmm_batch_create: hap_off not monotonic";
        // the reference would compute 2^1020 / 0 (pair_hmm.rs:515-517); SURVEY 8b asks for an explicit error
        if (hap_off[a + 1] == hap_off[a]) return "phmm_batch_create: empty haplotype";
    }
    if (tight_out) *tight_out = tight;
    return nullptr;
}

}  // namespace phmm_host

namespace {

// ---- device memory provider (after planning: the arena is sized from the plan) -----------------
// arena mode: bump-allocate from the handle's arena, "uploads" go to the pinned mirror and travel in
// one copy later; otherwise hipMalloc per piece and async copies on the handle's stream.
// (the first failure latches: every later call does nothing)
struct Placer {
    phmm_handle *h;
    phmm_batch *b;
    bool ok = true;
    bool async_pending = false;
    void *dalloc(size_t bytes, void **mirror) {
        if (mirror) *mirror = nullptr;
        if (!ok) return nullptr;
        if (b->arena && align_up(b->arena->used, 256) + bytes <= b->arena->cap) {
            const size_t off = align_up(b->arena->used, 256);
            b->arena->used = off + bytes;
            if (mirror) *mirror = b->arena->host + off;
            return b->arena->dev + off;
        }
        void *p = nullptr;
        ok = hip_ok(h, hipMalloc(&p, std::max<size_t>(bytes, 256)), "hipMalloc(batch)");
        if (ok) b->mallocs.push_back(p);
        return p;
    }
    void up(void *dst, void *mirror, const void *src, size_t bytes) {
        if (!ok || !bytes) return;
        if (mirror) {
            memcpy(mirror, src, bytes);
        } else {
            ok = hip_ok(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->S()), "H2D meta");
            async_pending = true;
        }
    }
    template <class T>
    T *put(const T *src, size_t count) {
        void *mirror;
        T *dst = (T *)dalloc(count * sizeof(T), &mirror);
        up(dst, mirror, src, count * sizeof(T));
        return dst;
    }
};

// Places the finished plan of `b` (b->plan) in device memory: offset arrays, per-class lists, redo flags, generic scratch, the
// status word and rescue scratch of a persistent batch, the items of every chained launch.  Decides nothing about the launches.
// false: h->err says why; what was allocated on the way is the batch's (b->mallocs).
bool place_batch(phmm_handle *h, phmm_batch *b, const BatchOffsets &o, bool use_arena, size_t extra_arena_bytes) {
    const BatchPlan &plan = b->plan;
    const uint32_t n_regions = plan.n_regions, n_reads = plan.n_reads, n_haps = plan.n_haps;
    if (use_arena) {
        // bytes of per-class work lists placed below (the read list of every class: identity and purely chained classes upload none)
        size_t class_meta = 0;
        for (const ShapeClass &c : plan.classes) {
            class_meta += align_up(c.reads.size() * 4, 256);
            if (!c.L) class_meta += align_up(c.pair_first.size() * 8, 256);
        }
        for (const ChainGroup &grp : plan.chain_groups) class_meta += align_up(grp.items.size() * sizeof(ChainItem), 256);
        // exact: every dalloc() below and the payload / result placement of enqueue_compute (each piece starts on a
        // 256-byte boundary), so that nothing staged later can fail for lack of room
        const size_t need = align_up((size_t)n_reads * 4, 256) + align_up((size_t)(n_regions + 1) * 4, 256) * 2 +
                            align_up((size_t)(n_reads + 1) * 4, 256) + align_up((size_t)(n_haps + 1) * 4, 256) +
                            align_up((size_t)(n_regions + 1) * 8, 256) + class_meta + 5 * align_up(b->read_bytes, 256) +
                            align_up(b->hap_bytes, 256) + 256 + align_up(b->n_out * 8, 256) + 4096 + extra_arena_bytes +
                            align_up((size_t)n_reads, 256) /* redo flags of the f32-first mode */;
        Arena &A = h->A();
        if (!canary_before_staging(h, A)) return false;  // (PHMM_MIRROR_CANARY: a store landed in the last call's result block after it returned)
        if (A.cap < need) {
            (void)hipStreamSynchronize(h->S());
            if (A.dev) (void)hipFree(A.dev);
            if (A.host) (void)hipHostFree(A.host);
            A.dev = A.host = nullptr;
            A.cap = 0;
            const size_t cap = std::max<size_t>(need + need / 2, 1 << 20);
            if (!hip_ok(h, hipMalloc((void **)&A.dev, cap), "hipMalloc(arena)") ||
                !hip_ok(h, hipHostMalloc((void **)&A.host, cap, hipHostMallocDefault), "hipHostMalloc(arena)"))
                return false;
            A.cap = cap;
        }
        A.used = 0;
        b->arena = &A;
    }
    Placer p{h, b};

    // ---- device metadata --------------------------------------------------------------------
    b->d_read_region = p.put(plan.read_region.data(), n_reads);
    b->d_region_read_off = p.put(o.region_read_off, (size_t)n_regions + 1);
    b->d_region_hap_off = p.put(o.region_hap_off, (size_t)n_regions + 1);
    b->d_read_off = p.put(o.read_off, (size_t)n_reads + 1);
    b->d_hap_off = p.put(o.hap_off, (size_t)n_haps + 1);
    b->d_out_off = p.put(o.out_off, (size_t)n_regions + 1);
    if (!b->arena) {  // persistent batch: own status word (arena mode keeps it next to the results)
        b->d_status = (uint32_t *)p.dalloc(256, nullptr);
        if (p.ok) p.ok = hip_ok(h, hipMemsetAsync(b->d_status, 0, 4, h->S()), "memset status");
        // ... and own scratch for the exact pass, which rides behind the forward kernels of every launch (the caller
        // owns the stream, so the library cannot look at the status word in between)
        if (p.ok && n_reads && !h->sw.no_rescue) {
            size_t bytes = 0;
            rescue_geometry(plan.max_h, &b->rescue_blocks, &bytes);
            p.ok = hip_ok(h, hipMalloc((void **)&b->rescue_scratch, bytes), "hipMalloc(rescue scratch)");
            if (p.ok) b->mallocs.push_back(b->rescue_scratch);
        }
    }

    // ---- per-class lists ----------------------------------------------------------------------
    b->class_dev.resize(plan.classes.size());
    for (size_t i = 0; i < plan.classes.size(); ++i) {
        const ShapeClass &c = plan.classes[i];
        phmm_batch::ClassDevice &d = b->class_dev[i];
        // the per-read kernel's list of reads (the f64 per-read kernel of an f32-first class runs behind the f32 sweep over the reads it flags)
        if (!c.identity && (!c.chain || c.f32_first)) d.reads = p.put(c.reads.data(), c.reads.size());
        if (c.f32_first && !b->d_redo) b->d_redo = (uint8_t *)p.dalloc(align_up((size_t)n_reads, 256), nullptr);
        if (!c.L) {
            // scratch can be large: always its own allocation, never the arena
            if (p.ok) p.ok = hip_ok(h, hipMalloc((void **)&d.scratch, c.generic_scratch_bytes), "hipMalloc(generic scratch)");
            if (p.ok) b->mallocs.push_back(d.scratch);
            d.pair_first = p.put(c.pair_first.data(), c.pair_first.size());
        }
    }
    b->d_group_items.resize(plan.chain_groups.size());
    for (size_t i = 0; i < plan.chain_groups.size(); ++i)
        b->d_group_items[i] = p.put(plan.chain_groups[i].items.data(), plan.chain_groups[i].items.size());
    // the caller's offset arrays may die when the call returns: finish the async copies first (arena mode copied into the mirror)
    if (p.ok && p.async_pending) p.ok = hip_ok(h, hipStreamSynchronize(h->S()), "sync(meta)");
    return p.ok;
}

}  // namespace

// Plans a batch (phmm_plan.cpp) and places the plan on the device.
static phmm_batch *batch_create_impl(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                                     const uint32_t *region_hap_off, const uint32_t *read_off,
                                     const uint32_t *hap_off, const uint64_t *out_off, bool use_arena,
                                     size_t extra_arena_bytes = 0) {
    if (!h) return nullptr;
    h->err.clear();
    h->err_code = PHMM_OK;
    if (tl_err_h == h) tl_err_h = nullptr;
    bool tight = true;
    if (const char *bad = validate_offsets(n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, &tight)) {
        h->err = bad;
        h->err_code = PHMM_ERR_INVALID_ARG;
        return nullptr;
    }
    const uint32_t n_reads = region_read_off[n_regions], n_haps = region_hap_off[n_regions];
    DeviceGuard dg(h->device);
    if (!dg.ok) {
        h->err = "hipSetDevice failed";
        h->err_code = PHMM_ERR_HIP;
        return nullptr;
    }

    // (owned until the plan is placed: an exception on the way -- a host allocation -- releases it and what it holds)
    struct BatchDeleter {
        void operator()(phmm_batch *x) const {
            for (void *m : x->mallocs) (void)hipFree(m);
            delete x;
        }
    };
    std::unique_ptr<phmm_batch, BatchDeleter> owner(new phmm_batch());
    phmm_batch *b = owner.get();
    b->h = h;
    b->n_out = out_off[n_regions];
    b->read_bytes = read_off[n_reads];
    b->hap_bytes = hap_off[n_haps];
    b->tight_out = tight;
    if (!tight)
        for (uint32_t g = 0; g < n_regions; ++g)
            b->out_extents.emplace_back(out_off[g], (uint64_t)(region_read_off[g + 1] - region_read_off[g]) *
                                                        (uint64_t)(region_hap_off[g + 1] - region_hap_off[g]));
    b->home_stream = h->S();
    const BatchOffsets o{n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off};
    b->plan = plan_batch(o, h->sw, h->flags, h->gpu_sharers);
    if (!place_batch(h, b, o, use_arena, extra_arena_bytes)) return nullptr;
    return owner.release();
}

extern "C" {

phmm_batch *phmm_batch_create(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                              const uint32_t *region_hap_off, const uint32_t *read_off, const uint32_t *hap_off,
                              const uint64_t *out_off) {
    PHMM_GUARD_BEGIN
    return batch_create_impl(h, n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, false);
    PHMM_GUARD_END(h, "phmm_batch_create", PHMM_FAIL_NULL)
}

// What the planned launches sweep, in lane-cells: every row of every wave x 64 lanes x its K columns -- the columns beyond a
// haplotype's end inside its 16 x K lanes, haplotype slots a wave leaves empty, the rows of a multi-stream item's shorter
// streams.  executed / cells is the padding a batch's shapes cost (1.01 for the uniform config-2 batch: 304 columns for 300).
uint64_t phmm_batch_executed_cells(const phmm_batch *b) { return b ? b->plan.swept_cells : 0; }

int phmm_batch_bind_device(phmm_batch *b, const uint8_t *d_read_bases, const uint8_t *d_base_q, const uint8_t *d_ins_q,
                           const uint8_t *d_del_q, const uint8_t *d_gcp, const uint8_t *d_hap_bases, double *d_out) {
    if (!b) return PHMM_ERR_INVALID_ARG;
    if ((b->read_bytes && (!d_read_bases || !d_base_q || !d_ins_q || !d_del_q || !d_gcp)) ||
        (b->hap_bytes && !d_hap_bases) || (b->n_out && !d_out)) {
        b->h->err = "phmm_batch_bind_device: null device pointer";
        return PHMM_ERR_INVALID_ARG;
    }
    b->d_read_bases = d_read_bases;
    b->d_base_q = d_base_q;
    b->d_ins_q = d_ins_q;
    b->d_del_q = d_del_q;
    b->d_gcp = d_gcp;
    b->d_hap_bases = d_hap_bases;
    b->d_out = d_out;
    b->bound = true;
    return PHMM_OK;
}

int phmm_batch_upload(phmm_batch *b, const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                      const uint8_t *del_q, const uint8_t *gcp, const uint8_t *hap_bases) {
    if (!b) return PHMM_ERR_INVALID_ARG;
    phmm_handle *h = b->h;
    if ((b->read_bytes && (!read_bases || !base_q || !ins_q || !del_q || !gcp)) || (b->hap_bytes && !hap_bases)) {
        h->err = "phmm_batch_upload: null host pointer";
        return PHMM_ERR_INVALID_ARG;
    }
    DeviceGuard dg(h->device);
    const size_t rb = align_up(b->read_bytes, 256), hb = align_up(b->hap_bytes, 256), ob = align_up(b->n_out * 8, 256);
    if (!b->d_owned) {
        HIP_TRY(h, hipMalloc(&b->d_owned, 5 * rb + hb + ob + 256), PHMM_ERR_HIP);
        b->mallocs.push_back(b->d_owned);
    }
    uint8_t *p = (uint8_t *)b->d_owned;
    uint8_t *d[6];
    for (int i = 0; i < 5; ++i) { d[i] = p; p += rb; }
    d[5] = p; p += hb;
    double *d_out = (double *)p;
    const uint8_t *src[6] = {read_bases, base_q, ins_q, del_q, gcp, hap_bases};
    for (int i = 0; i < 6; ++i) {
        const size_t bytes = i < 5 ? b->read_bytes : b->hap_bytes;
        if (bytes) HIP_TRY(h, hipMemcpyAsync(d[i], src[i], bytes, hipMemcpyHostToDevice, b->home_stream), PHMM_ERR_HIP);
    }
    return phmm_batch_bind_device(b, d[0], d[1], d[2], d[3], d[4], d[5], d_out);
}

// Everything of a launch that does not depend on the shape class.
static ForwardParams base_params(const phmm_batch *b) {
    const phmm_handle *h = b->h;
    ForwardParams p{};
    p.read_region = b->d_read_region;
    p.region_read_off = b->d_region_read_off;
    p.region_hap_off = b->d_region_hap_off;
    p.read_off = b->d_read_off;
    p.hap_off = b->d_hap_off;
    p.out_off = b->d_out_off;
    p.read_bases = b->d_read_bases;
    p.base_q = b->d_base_q;
    p.ins_q = b->d_ins_q;
    p.del_q = b->d_del_q;
    p.gcp = b->d_gcp;
    p.hap_bases = b->d_hap_bases;
    p.out = b->d_out;
    p.eps = h->d_eps;
    p.eps_mis = h->d_eps_mis;
    p.mm = h->d_mm;
    p.ratio_mis = h->d_ratio_mis;
    p.inv_om = h->d_inv_om;
    p.initial_condition = initial_condition();
    p.initial_condition_log10 = initial_condition_log10();
    p.status = b->d_status;
    return p;
}

// The exact pass over the pairs below kRescueBelow (phmm_exact_kernels.hip).  force == 0: in-stream, the kernel looks
// at the status word itself and returns at once when no forward kernel raised STATUS_RESCUE.
static int launch_rescue_pass(phmm_batch *b, double *scratch, uint32_t n_blocks, bool force, hipStream_t stream) {
    RescueParams rp{};
    rp.f = base_params(b);
    rp.n_reads = b->plan.n_reads;
    rp.scratch = scratch;
    rp.max_h = b->plan.max_h;
    rp.n_blocks = n_blocks;
    rp.force = force ? 1u : 0u;
    return hip_ok(b->h, launch_rescue(rp, stream), "phmm_rescue") ? PHMM_OK : PHMM_ERR_HIP;
}

// Scratch of the exact pass for batches staged in arena `A` (grow-only; the caller has made sure nothing that could
// use the old buffer is in flight on this slot).
static bool ensure_arena_rescue(phmm_handle *h, Arena &A, uint32_t max_h, uint32_t *n_blocks) {
    size_t bytes = 0;
    rescue_geometry(max_h, n_blocks, &bytes);
    if (A.rescue_cap >= bytes) return true;
    if (A.rescue) (void)hipFree(A.rescue);
    A.rescue = nullptr;
    A.rescue_cap = 0;
    if (!hip_ok(h, hipMalloc((void **)&A.rescue, bytes), "hipMalloc(rescue scratch)")) return false;
    A.rescue_cap = bytes;
    return true;
}

int phmm_batch_launch(phmm_batch *b, void *stream_v) {
    if (!b) return PHMM_ERR_INVALID_ARG;
    phmm_handle *h = b->h;
    if (!b->bound) {
        h->err = "phmm_batch_launch: no device buffers bound";
        return PHMM_ERR_NOT_BOUND;
    }
    DeviceGuard dg(h->device);
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : b->home_stream;
    if (b->d_redo && !hip_ok(h, hipMemsetAsync(b->d_redo, 0, b->plan.n_reads, stream), "memset redo")) return PHMM_ERR_HIP;
    // The chained sweeps: one launch per lanes-per-pair value, precision and (mixed batches) range of K.  Several launches
    // run side by side: the first on the caller's stream, the others on the handle's side streams between a fork and a
    // join event -- each alone would leave the chip to its own tail before the next could start.
    const size_t n_groups = b->plan.chain_groups.size();
    // (not while the chunks of a pipelined host call are in flight: those already overlap each other on the slot streams,
    // and forks of several chunks would queue behind one another on the side streams -- 1 536 mixed regions through host
    // buffers: 25 ms without, 32 ms with)
    // (round 4, three large chunks: forking them all changes nothing either; round 5, the LAST chunk of a mixed call alone: 19.8-20.0
    // ms against 18.7-18.8 -- both measured and dropped)
    const bool fork = n_groups >= 2 && !h->defer_d2h;
    if (fork) {
        for (int i = 0; i < phmm_handle::kSideStreams; ++i) {
            if (!h->side_streams[i] && !hip_ok(h, hipStreamCreateWithFlags(&h->side_streams[i], hipStreamNonBlocking), "hipStreamCreate")) return PHMM_ERR_HIP;
            if (!h->ev_join[i] && !hip_ok(h, hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming), "hipEventCreate")) return PHMM_ERR_HIP;
        }
        if (!h->ev_fork && !hip_ok(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming), "hipEventCreate")) return PHMM_ERR_HIP;
        if (!hip_ok(h, hipEventRecord(h->ev_fork, stream), "hipEventRecord")) return PHMM_ERR_HIP;
    }
    auto launch_class = [&](size_t ci) -> int {
        const ShapeClass &c = b->plan.classes[ci];
        const phmm_batch::ClassDevice &cd = b->class_dev[ci];
        ForwardParams p = base_params(b);
        p.class_reads = c.identity ? nullptr : cd.reads;
        p.n_items = (uint32_t)c.reads.size();
        p.lds_rows = c.lds_rows;
        p.cnd_select = c.cnd_select;
        if (!p.n_items) return PHMM_OK;
        hipError_t e;
        if (c.chain && !c.f32_first) return PHMM_OK;  // done with its group
        if (c.chain) {  // behind the f32 sweep: the f64 per-read kernel over exactly the reads it flagged
            p.redo = b->d_redo;
            e = launch_forward(c.L, c.K, p, c.grid, c.waves_per_block, c.lds_bytes, stream);
        } else if (c.L) {
            e = launch_forward(c.L, c.K, p, c.grid, c.waves_per_block, c.lds_bytes, stream);
        } else {
            GenericParams gp{};
            gp.f = p;
            gp.scratch = cd.scratch;
            gp.max_h = c.max_h;
            gp.pair_first = cd.pair_first;
            gp.n_pairs = c.pair_first.back();
            gp.n_blocks = c.generic_blocks;
            e = gp.n_pairs ? launch_generic(gp, stream) : hipSuccess;
        }
        return hip_ok(h, e, c.name) ? PHMM_OK : PHMM_ERR_HIP;
    };
    // The per-read classes of a mixed batch (a few hundred microseconds of small kernels) depend on no chained launch: behind
    // the join they ran alone at the end of the batch, one after the other.  With the launches forked they go out FIRST on the
    // caller's stream -- the chained launches of the side streams start beside them, the caller's own behind them.
    // (The mixed batch resident, three runs each on one box: 15.59-15.66 ms against 15.80-15.89 the other way round.)
    const bool early_classes = fork;
    if (early_classes)
        for (size_t ci = 0; ci < b->plan.classes.size(); ++ci)
            if (!b->plan.classes[ci].chain && launch_class(ci) != PHMM_OK) return PHMM_ERR_HIP;
    bool side_used[phmm_handle::kSideStreams] = {};
    // (Measured and dropped, round 5: dealing the launches to the streams by load, every stream sending its lightest first -- in the
    // mixed batch's timeline the two lightest launches trail the second and third heaviest -- : 15.56-15.67 ms either way.)
    for (size_t gi = 0; gi < n_groups; ++gi) {
        hipStream_t s_x = stream;
        if (fork && gi > 0) {
            const int si = (int)((gi - 1) % phmm_handle::kSideStreams);
            s_x = h->side_streams[si];
            if (!side_used[si] && !hip_ok(h, hipStreamWaitEvent(s_x, h->ev_fork, 0), "hipStreamWaitEvent")) return PHMM_ERR_HIP;
            side_used[si] = true;
        }
        const ChainGroup &grp = b->plan.chain_groups[gi];
        if (grp.items.empty()) continue;
        ChainParams cp{};
        cp.f = base_params(b);
        cp.items = b->d_group_items[gi];
        cp.n_items = (uint32_t)grp.items.size();
        cp.redo = grp.f32 ? b->d_redo : nullptr;
        hipStream_t s = s_x;
        const hipError_t e = grp.f32 ? launch_chain_f32(grp.L, grp.single_k, cp, s) : launch_chain(grp.L, grp.single_k, cp, s);
        if (!hip_ok(h, e, grp.f32 ? "phmm_forward_chain_f32" : "phmm_forward_chain")) return PHMM_ERR_HIP;
    }
    for (int i = 0; i < phmm_handle::kSideStreams; ++i)
        if (side_used[i] && (!hip_ok(h, hipEventRecord(h->ev_join[i], h->side_streams[i]), "hipEventRecord") ||
                             !hip_ok(h, hipStreamWaitEvent(stream, h->ev_join[i], 0), "hipStreamWaitEvent")))
            return PHMM_ERR_HIP;
    // (the per-read classes that depend on no chained launch went out in front of the fork, above)
    for (size_t ci = 0; ci < b->plan.classes.size(); ++ci)
        if (!(early_classes && !b->plan.classes[ci].chain) && launch_class(ci) != PHMM_OK) return PHMM_ERR_HIP;
    // Results below kRescueBelow are redone in the reference's operation order.  Persistent batches and the
    // engine-level call carry the pass in-stream (it returns at once unless a forward kernel asked for it); the
    // host-buffer path looks at the status word in finish_compute instead and pays nothing in the common case.
    if (b->rescue_scratch && !h->sw.no_rescue && b->plan.n_reads)
        return launch_rescue_pass(b, b->rescue_scratch, b->rescue_blocks, false, stream);
    return PHMM_OK;
}

int phmm_batch_status(phmm_batch *b) {
    if (!b) return PHMM_ERR_INVALID_ARG;
    phmm_handle *h = b->h;
    DeviceGuard dg(h->device);
    uint32_t st = 0;
    HIP_TRY(h, hipMemcpy(&st, b->d_status, 4, hipMemcpyDeviceToHost), PHMM_ERR_HIP);
    if (st) HIP_TRY(h, hipMemset(b->d_status, 0, 4), PHMM_ERR_HIP);
    if (status_positive(st, b->rescue_scratch != nullptr && !h->sw.no_rescue)) {  // (the exact pass rode behind every launch: its verdict)
        h->err = "PairHmm Log Probability cannot be greater than 0.0";  // pair_hmm.rs:478-481
        return PHMM_ERR_POSITIVE_RESULT;
    }
    return PHMM_OK;
}

int phmm_batch_download(phmm_batch *b, double *out) {
    if (!b || (b->n_out && !out)) return PHMM_ERR_INVALID_ARG;
    phmm_handle *h = b->h;
    if (!b->bound) return PHMM_ERR_NOT_BOUND;
    DeviceGuard dg(h->device);
    if (b->n_out)
        HIP_TRY(h, hipMemcpyAsync(out, b->d_out, b->n_out * 8, hipMemcpyDeviceToHost, b->home_stream), PHMM_ERR_HIP);
    HIP_TRY(h, hipStreamSynchronize(b->home_stream), PHMM_ERR_HIP);
    return phmm_batch_status(b);
}

}  // extern "C"

namespace phmm_host {

// When is the D2H copy of the results enqueued?  Right behind the kernels ("eager": one host wait per call, 15 us less
// latency for a lone small call), or by finish_compute once the host has seen the kernels complete ("deferred").  A copy
// that waits for a kernel sits at the head of its SDMA engine's queue and holds up every later copy that lands on that
// engine -- the H2D of the next chunk, or of another lane (tools/ubench/overlap3.hip; seen as strict H2D / kernel / D2H
// serialisation in the rocprofv3 timeline of the chunked path).  So: deferred wherever something else is in flight
// (chunks of a pipelined call, combined flushes of phmm_wait), eager for a one-shot call.
// PHMM_EAGER_D2H=1 / 0 forces one or the other (A/B measurements only).
bool eager_d2h(const phmm_handle *h) {
    return kForcedEagerD2H >= 0 ? kForcedEagerD2H != 0 : !h->defer_d2h;
}

// The zero-copy path (inputs fetched from the pinned mirror by a kernel, results stored into it) has no copies to keep out of
// each other's way: a combined flush may take it too.  (PHMM_EAGER_D2H=0 still forces the copy path, for the tests.)
bool zero_copy_allowed(const phmm_handle *) { return kForcedEagerD2H >= 0 ? kForcedEagerD2H != 0 : true; }

// ---- PHMM_MIRROR_CANARY ------------------------------------------------------------------------------------------------
// Small calls hand inputs and results over through the pinned mirror, and their kernels tell the calling thread themselves
// when they are through (region_finish): nothing but the kernels' own ordering stands between a late store and the next
// call's staged inputs.  Round 4 shipped such a store (two timing words of the aligner, NOTEBOOK 18.7) that only a C++
// caller saw, as one read's likelihoods 20 decades low.  With the switch set every such store is a failed call:
//   * when a zero-copy call returns, its result block in the mirror is filled with 0xA5 and must still be 0xA5 when the arena
//     is staged again (a store that lands between two calls);
//   * the inputs a zero-copy call staged are kept aside and compared with the mirror when the call ends (a store that lands
//     in the NEXT call's inputs -- the device never writes there).
static bool canary_fail(phmm_handle *h, const char *what, size_t at, unsigned got) {
    char msg[256];
    snprintf(msg, sizeof msg, "PHMM_MIRROR_CANARY: %s: pinned mirror offset %zu holds 0x%02x", what, at, got);
    fprintf(stderr, "%s\n", msg);
    if (h->sw.mirror_canary >= 2) abort();
    h->err = msg;
    h->err_code = PHMM_ERR_INTERNAL;
    return false;
}
bool canary_before_staging(phmm_handle *h, Arena &A) {
    A.canary_inputs.clear();
    if (!h->sw.mirror_canary || !A.canary_bytes || !A.host) return true;
    const size_t off = A.canary_off, n = A.canary_bytes;
    A.canary_bytes = 0;
    if (off + n > A.cap) return true;  // (the arena was replaced by a larger one)
    const unsigned char *q = (const unsigned char *)A.host + off;
    for (size_t i = 0; i < n; ++i)
        if (q[i] != 0xA5) return canary_fail(h, "a device store landed in a result block after its call had returned", off + i, q[i]);
    return true;
}
void canary_staged(phmm_handle *h, Arena &A, size_t in_bytes) {
    if (!h->sw.mirror_canary) return;
    A.canary_inputs.assign((const unsigned char *)A.host, (const unsigned char *)A.host + in_bytes);
}
bool canary_after_call(phmm_handle *h, Arena &A, size_t res_off, size_t res_bytes) {
    if (!h->sw.mirror_canary) return true;
    bool good = true;
    const size_t n = std::min(A.canary_inputs.size(), A.cap);
    if (n && memcmp(A.host, A.canary_inputs.data(), n) != 0) {
        size_t i = 0;
        while (i < n && (unsigned char)A.host[i] == A.canary_inputs[i]) ++i;
        good = canary_fail(h, "a device store landed in the staged inputs of a call", i, (unsigned char)A.host[i]);
    }
    A.canary_inputs.clear();
    if (res_off + res_bytes <= A.cap) {
        memset(A.host + res_off, 0xA5, res_bytes);
        A.canary_off = res_off;
        A.canary_bytes = res_bytes;
    }
    return good;
}

// Stage one batch in the current slot's arena and enqueue H2D, kernels and D2H on its stream.  No sync.
int enqueue_compute(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                    const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                    const uint8_t *del_q, const uint8_t *gcp, const uint32_t *hap_off, const uint8_t *hap_bases,
                    const uint64_t *out_off, double *out, PendingCompute *pending, const Parts *parts) {
    const bool trace = h->sw.trace != 0;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_0 = now();
    double t_plan = 0, t_stage = 0, t_h2d = 0, t_launch = 0;
    bool zero_copy = false;
    phmm_batch *b = batch_create_impl(h, n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, true);
    if (!b) return h->err_code ? h->err_code : PHMM_ERR_INVALID_ARG;
    int st = PHMM_OK;
    if (!parts && ((b->read_bytes && (!read_bases || !base_q || !ins_q || !del_q || !gcp)) || (b->hap_bytes && !hap_bases) ||
                   (b->n_out && !out))) {
        h->err = "phmm_compute: null pointer";
        st = PHMM_ERR_INVALID_ARG;
    }
    Arena &A = h->A();
    t_plan = now();
    if (st == PHMM_OK) {
        // payload into the arena mirror, then [status | out] last so that one copy each way suffices
        const uint8_t *src[6] = {read_bases, base_q, ins_q, del_q, gcp, hap_bases};
        const uint8_t *d[6];
        size_t offs[6] = {0};
        for (int i = 0; i < 6; ++i) {
            const size_t bytes = i < 5 ? b->read_bytes : b->hap_bytes;
            const size_t off = align_up(A.used, 256);
            A.used = off + bytes;
            if (A.used > A.cap) {
                h->err = "phmm_compute: internal error, arena too small";
                st = PHMM_ERR_HIP;
                break;
            }
            offs[i] = off;
            h->stat_staged_bytes += bytes;
            d[i] = (const uint8_t *)(A.dev + off);
        }
        // everything rides in the single copy of the pinned mirror (the chunked path keeps every array of a
        // chunk at or below kChunkBytes so that staging chunk i+1 overlaps the kernels of chunk i)
        auto stage_array = [&](int i) {
            const size_t bytes = i < 5 ? b->read_bytes : b->hap_bytes;
            if (parts) {
                size_t o = offs[i];
                for (size_t s = 0; s < parts->src[i].size(); ++s) {
                    const size_t n = i < 5 ? parts->read_bytes[s] : parts->hap_bytes[s];
                    if (n) memcpy(A.host + o, parts->src[i][s], n);
                    o += n;
                }
            } else if (bytes) {
                memcpy(A.host + offs[i], src[i], bytes);
            }
        };
        if (st == PHMM_OK) {
            // A chunk of a large call is five arrays of megabytes: the quality tracks go through helper threads while this one
            // copies the bases and the haplotypes (1 536 mixed regions: 0.7-1.1 ms of staging per chunk on the calling thread,
            // a quarter of the call).  Small calls stay on the calling thread -- a thread costs more than their copies.
            if (b->read_bytes >= (1u << 20)) {
                std::thread helpers[4];
                int started = 0;
                try {
                    for (int i = 1; i <= 4; ++i) {
                        helpers[started] = std::thread(stage_array, i);
                        ++started;
                    }
                } catch (const std::system_error &) {  // no thread to be had: the rest on this one
                }
                stage_array(0);
                stage_array(5);
                for (int i = started + 1; i <= 4; ++i) stage_array(i);
                for (int i = 0; i < started; ++i) helpers[i].join();
            } else {
                for (int i = 0; i < 6; ++i) stage_array(i);
            }
        }
        const size_t in_bytes = align_up(A.used, 256);
        b->out_arena_off = in_bytes;
        A.used = in_bytes + 256 + b->n_out * 8;
        if (st != PHMM_OK || A.used > A.cap) {  // cannot happen: batch_create_impl reserved for exactly this layout
            h->err = "phmm_compute: internal error, arena too small";
            std::string keep = h->err;
            phmm_batch_destroy(b);
            h->err = keep;
            return PHMM_ERR_HIP;
        }
        t_stage = now();
        memset(A.host + in_bytes, 0, 256);  // status word
        b->d_status = (uint32_t *)(A.dev + in_bytes);
        double *d_out = (double *)(A.dev + in_bytes + 256);
        // A small one-shot call gets no D2H copy at all: its kernels store the few results straight into the pinned
        // mirror (8 bytes per pair over PCIe), and finish_compute applies the reference's `<= 0` check on the host.
        // (a combined flush of phmm_submit too: nothing on this path is a copy that could get in another flush's way)
        zero_copy = zero_copy_allowed(h) && b->tight_out && b->n_out * 8 <= kZeroCopyOutBytes;
        if (zero_copy) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, A.host + in_bytes + 256, 0) == hipSuccess && dp)
                d_out = (double *)dp;
            else
                zero_copy = false;
        }
        // ... and its inputs are fetched from the mirror by a kernel instead of the copy engine (no cross-engine
        // dependency in front of the first launch; phmm_cigar_kernels.hip)
        void *host_dp = nullptr;
        if (zero_copy && in_bytes + 256 <= kStageInBytes && hipHostGetDevicePointer(&host_dp, A.host, 0) == hipSuccess && host_dp) {
            canary_staged(h, A, in_bytes);
            if (!hip_ok(h, launch_stage_in(host_dp, A.dev, in_bytes + 256, h->S()), "phmm_stage_in_kernel")) st = PHMM_ERR_HIP;
        } else if (!hip_ok(h, hipMemcpyAsync(A.dev, A.host, in_bytes + 256, hipMemcpyHostToDevice, h->S()), "H2D batch")) {
            st = PHMM_ERR_HIP;
        }
        // (slots the kernels never write -- gaps the caller left in out_off -- are never copied back either)
        if (st == PHMM_OK) st = phmm_batch_bind_device(b, d[0], d[1], d[2], d[3], d[4], d[5], d_out);
        t_h2d = now();
    }
    if (st == PHMM_OK) st = phmm_batch_launch(b, nullptr);
    t_launch = now();
    const bool eager = eager_d2h(h);  // otherwise finish_compute fetches the results
    if (st == PHMM_OK && eager && !zero_copy &&
        !hip_ok(h, hipMemcpyAsync(A.host + b->out_arena_off, A.dev + b->out_arena_off, 256 + b->n_out * 8,
                                  hipMemcpyDeviceToHost, h->S()),
                "D2H results"))
        st = PHMM_ERR_HIP;
    if (st != PHMM_OK) {
        std::string keep = h->err;
        (void)hipStreamSynchronize(h->S());
        phmm_batch_destroy(b);
        h->err = keep;
        return st;
    }
    if (trace)
        fprintf(stderr, "  enqueue %u regions: plan %.0f us, stage %.0f us, H2D enqueue %.0f us, launch %.0f us, D2H enqueue %.0f us\n",
                n_regions, t_plan - t_0, t_stage - t_plan, t_h2d - t_stage, t_launch - t_h2d, now() - t_launch);
    pending->b = b;
    pending->slot = h->slot;
    pending->out = out;
    pending->parts = parts;
    pending->stream = h->S();
    pending->d2h_pending = !eager && !zero_copy;
    pending->zero_copy = zero_copy;
    return PHMM_OK;
}

// Next chunk after `c` of the regions [.., n_regions) (start with c.g1 == first region, c.started == false): grows while
// every per-base array stays below the direct-copy limit; `whole` takes everything that is left in one chunk.
bool next_chunk(ChunkView &c, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                const uint32_t *read_off, const uint32_t *hap_off, const uint64_t *out_off, bool whole) {
    const uint32_t g0 = c.g1;
    if (g0 >= n_regions) return false;
    uint32_t g1 = g0 + 1;
    const size_t base_r = read_off[region_read_off[g0]];
    // the first chunks are short so that the GPU starts early (0.5, 0.5, 1, 2, 4, 4 ... MB per array); staging and the
    // H2D copy of the following ones hide behind its kernels
    c.index = c.started ? c.index + 1 : 0;
    c.started = true;
    // f64: 0.5 MB per array four times, then 1, 1, 2, 2, 4, 4 ... (mid-size batches want many small chunks, large ones
    // large launches).  f32-first handles: 1, 2, 4, 4 ... -- the f32 sweep only exists as the chained kernel, which needs
    // a few hundred regions per launch.
    // Mixed batches (round 4): 4 MB per array, then 8, 16, 32 ... -- every chunk of a long-tailed mix is a launch per range of K
    // with a tail of its own, and since planning and staging take 0.85 instead of 2 ms per 4 MB the device no longer waits for
    // the host: 1 536 mixed regions 24.0 ms in seven chunks of 4 MB, 20.4 in three of 4 / 8 / 16 (resident: 15.8).
    // Round 5, the cap swept on one box (tools/hostpath_ragged_sweep.py, best of six calls, twice): 4 / 8 / 16: 18.75-18.85 ms;
    // 4 / 8 / 8 / 7: 18.1-18.3; cap 6: 19.3-19.4; cap 12: 18.7-18.8; first chunk 3 / 6 MB: 18.5 / 20.1; a first chunk of 1 or 2 MB and
    // 8 MB ones behind it (the device starts 0.5 ms earlier, one more set of launches): 18.1-18.3 -- so the cap is 8 MB.
    const uint32_t step = c.f32_first ? c.index + 1 : c.mixed ? c.index : (c.index < 4 ? 0 : (c.index - 2) / 2);
    const size_t max_bytes = c.mixed && !c.f32_first ? kMixedChunkBytes : kChunkBytes;
    const size_t limit = std::min(max_bytes, (c.f32_first ? (1u << 20) / 2 : c.mixed ? kMixedFirstChunkBytes : kFirstChunkBytes) << std::min<uint32_t>(step, 16));
    if (whole) {
        g1 = n_regions;
    } else if (!c.mixed) {
        while (g1 < n_regions && (size_t)read_off[region_read_off[g1 + 1]] - base_r <= limit) ++g1;
    } else {
        // A mixed batch falls into many shape classes, and a chunk of a few dozen regions is too small for the chained
        // kernel: every class then gets a small per-read launch of its own (1 536 mixed regions: the first six chunks
        // were 10-20 launches of ~5 us each for 184 regions).  Such a chunk keeps growing until it has enough wave-sweeps
        // to chain (or reaches the largest chunk size).
        auto units = [&](uint32_t g) {
            return (uint64_t)(region_read_off[g + 1] - region_read_off[g]) * ((region_hap_off[g + 1] - region_hap_off[g] + 3) / 4);
        };
        uint64_t u = units(g0);
        while (g1 < n_regions) {
            const size_t bytes = (size_t)read_off[region_read_off[g1 + 1]] - base_r;
            if (bytes > max_bytes || (bytes > limit && u >= 8ull * 2 * kNumSimd * 4)) break;
            u += units(g1);
            ++g1;
        }
        // ... and a remainder too small to chain on its own rides with this chunk instead of following as a per-read launch
        if (g1 < n_regions) {
            uint64_t rest = 0;
            for (uint32_t g = g1; g < n_regions && rest < 8ull * 2 * kNumSimd * 4; ++g) rest += units(g);
            if (rest < 8ull * 2 * kNumSimd * 4) g1 = n_regions;
        }
    }
    c.g0 = g0;
    c.g1 = g1;
    c.r0 = region_read_off[g0];
    c.r1 = region_read_off[g1];
    c.h0 = region_hap_off[g0];
    c.h1 = region_hap_off[g1];
    c.read_byte0 = read_off[c.r0];
    c.hap_byte0 = hap_off[c.h0];
    c.rro.resize(g1 - g0 + 1);
    c.rho.resize(g1 - g0 + 1);
    c.oo.resize(g1 - g0 + 1);
    for (uint32_t g = g0; g <= g1; ++g) {
        c.rro[g - g0] = region_read_off[g] - c.r0;
        c.rho[g - g0] = region_hap_off[g] - c.h0;
        c.oo[g - g0] = out_off[g] - out_off[g0];
    }
    c.ro.resize(c.r1 - c.r0 + 1);
    for (uint32_t r = c.r0; r <= c.r1; ++r) c.ro[r - c.r0] = read_off[r] - read_off[c.r0];
    c.ho.resize(c.h1 - c.h0 + 1);
    for (uint32_t a = c.h0; a <= c.h1; ++a) c.ho[a - c.h0] = hap_off[a] - hap_off[c.h0];
    return true;
}

// Wait for a pending batch, hand the results to the caller, release the batch.
int finish_compute(phmm_handle *h, PendingCompute *p) {
    if (!p->b) return PHMM_OK;
    int st = PHMM_OK;
    phmm_batch *b = p->b;
    Arena &A = h->arenas[p->slot];
    hipStream_t S = p->stream ? p->stream : h->streams[p->slot];
    const size_t res_bytes = 256 + b->n_out * 8;
    auto fetch = [&]() {  // [status | out] -> pinned mirror
        return hip_ok(h, hipMemcpyAsync(A.host + b->out_arena_off, A.dev + b->out_arena_off, res_bytes, hipMemcpyDeviceToHost, S),
                      "D2H results") &&
               hip_ok(h, wait_stream(h, S), "sync(D2H)");
    };
    if (!hip_ok(h, wait_stream(h, S), "sync") || (p->d2h_pending && !fetch())) {  // kernels are done: fetch now
        st = PHMM_ERR_HIP;
    } else {
        const char *hs = A.host + b->out_arena_off;
        const double *v = (const double *)(hs + 256);
        uint32_t bits = *(const uint32_t *)hs;
        auto each_result = [&](auto &&f) {  // every slot a kernel wrote
            if (b->tight_out)
                for (uint64_t i = 0; i < b->n_out; ++i) f(v[i]);
            else
                for (const auto &e : b->out_extents)
                    for (uint64_t i = 0; i < e.second; ++i) f(v[e.first + i]);
        };
        if (p->zero_copy) {  // the status word stayed on the device: every slot was written once, look at the values
            bits = 0;
            each_result([&](double x) { bits |= status_bits(x); });
        }
        if ((bits & STATUS_RESCUE) && !h->sw.no_rescue) {
            // some pair came out below kRescueBelow: redo those in the reference's operation order, fetch again
            uint32_t nb = 0;
            h->stat_rescue_passes += 1;
            if (!ensure_arena_rescue(h, A, b->plan.max_h, &nb) || launch_rescue_pass(b, A.rescue, nb, true, S) != PHMM_OK ||
                !hip_ok(h, hipStreamSynchronize(S), "sync(rescue)") || (!p->zero_copy && !fetch())) {
                st = PHMM_ERR_HIP;
            } else {
                // (from the values on every path: phmm_rescue only ORs into the device word, so a bit a fast kernel raised
                // for a pair the exact pass has since replaced would survive there)
                bits = 0;
                each_result([&](double x) { bits |= status_bits(x); });
            }
        }
        if (st == PHMM_OK) {
            const char *src = hs + 256;
            if (p->parts) {
                // part s owns the regions [first_region[s], first_region[s+1]) of the combined batch
                for (size_t s = 0; s < p->parts->out.size(); ++s) {
                    if (b->tight_out) {
                        if (p->parts->n_out[s]) memcpy(p->parts->out[s], src, p->parts->n_out[s] * 8);
                    } else {
                        const uint32_t g0 = p->parts->first_region[s], g1 = p->parts->first_region[s + 1];
                        for (uint32_t g = g0; g < g1; ++g) {  // the part's out_off starts at 0, like every offset array
                            const auto &e = b->out_extents[g];
                            if (e.second) memcpy(p->parts->out[s] + (e.first - b->out_extents[g0].first), v + e.first, e.second * 8);
                        }
                    }
                    src += p->parts->n_out[s] * 8;
                }
            } else if (b->tight_out) {
                if (b->n_out) memcpy(p->out, src, b->n_out * 8);
            } else {
                for (const auto &e : b->out_extents)
                    if (e.second) memcpy(p->out + e.first, v + e.first, e.second * 8);
            }
            if (bits & STATUS_POSITIVE) {
                h->err = "PairHmm Log Probability cannot be greater than 0.0";  // pair_hmm.rs:478-481
                st = PHMM_ERR_POSITIVE_RESULT;
            }
            // (PHMM_MIRROR_CANARY: the results are with the caller -- nothing may store into this call's block from here on)
            if (p->zero_copy && !canary_after_call(h, A, b->out_arena_off, res_bytes) && st == PHMM_OK) st = PHMM_ERR_INTERNAL;
        }
    }
    std::string keep = h->err;
    phmm_batch_destroy(b);
    h->err = keep;
    p->b = nullptr;
    return st;
}


phmm_batch *batch_create_in_arena(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                                  const uint32_t *read_off, const uint32_t *hap_off, const uint64_t *out_off, size_t extra_arena_bytes) {
    return batch_create_impl(h, n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, true, extra_arena_bytes);
}
BatchView batch_view(const phmm_batch *b) {
    BatchView v{};
    v.n_regions = b->plan.n_regions;
    v.n_reads = b->plan.n_reads;
    v.n_haps = b->plan.n_haps;
    v.max_h = b->plan.max_h;
    v.n_out = b->n_out;
    v.read_bytes = b->read_bytes;
    v.hap_bytes = b->hap_bytes;
    v.tight_out = b->tight_out;
    v.d_read_region = b->d_read_region;
    v.d_region_read_off = b->d_region_read_off;
    v.d_region_hap_off = b->d_region_hap_off;
    v.d_read_off = b->d_read_off;
    v.d_hap_off = b->d_hap_off;
    v.d_out_off = b->d_out_off;
    return v;
}
void batch_set_status(phmm_batch *b, uint32_t *d_status) { b->d_status = d_status; }
bool batch_set_inline_rescue(phmm_handle *h, phmm_batch *b) {
    if (!b->plan.n_reads || h->sw.no_rescue) return true;
    if (!ensure_arena_rescue(h, *b->arena, b->plan.max_h, &b->rescue_blocks)) return false;
    b->rescue_scratch = b->arena->rescue;
    return true;
}
void batch_copy_out(const phmm_batch *b, const double *src, double *out) {
    if (b->tight_out) {
        if (b->n_out) memcpy(out, src, b->n_out * 8);
    } else {  // gaps the caller left in out_off stay untouched
        for (const auto &e : b->out_extents)
            if (e.second) memcpy(out + e.first, src + e.first, e.second * 8);
    }
}
size_t one_shot_bytes() { return kOneShotBytes; }
size_t stage_in_bytes() { return kStageInBytes; }
size_t zero_copy_out_bytes() { return kZeroCopyOutBytes; }

}  // namespace phmm_host

extern "C" {

}  // extern "C"

namespace phmm_host {

// phmm_compute on the regions [g_begin, g_end) of the caller's (already validated) arrays; results go where
// phmm_compute on the whole batch would put them.  phmm_compute is the range [0, n_regions); phmm_compute_multi hands
// every engine a contiguous range -- no gather, every payload byte is copied once, into the pinned mirror.
int compute_range(phmm_handle *h, uint32_t g_begin, uint32_t g_end, const uint32_t *region_read_off,
                  const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *base_q,
                  const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *gcp, const uint32_t *hap_off,
                  const uint8_t *hap_bases, const uint64_t *out_off, double *out) {
    const bool trace = h->sw.trace != 0;
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    DeviceGuard dg(h->device);
    const uint32_t n_regions = g_end - g_begin;
    const size_t range_bytes = (size_t)read_off[region_read_off[g_end]] - read_off[region_read_off[g_begin]];
    // ---- small / medium batch: one shot ------------------------------------------------------------
    const bool f32_first = (h->flags & PHMM_FLAG_F32_FIRST) != 0;
    if (n_regions < 8 || range_bytes <= (f32_first ? (size_t)(8u << 20) : kOneShotBytes) || h->sw.no_pipeline) {
        h->slot = 0;
        PendingCompute p;
        int st;
        if (g_begin == 0) {  // offsets already start at 0
            st = enqueue_compute(h, n_regions, region_read_off, region_hap_off, read_off, read_bases, base_q, ins_q, del_q, gcp,
                                 hap_off, hap_bases, out_off, out, &p);
        } else {
            ChunkView c;
            c.g1 = g_begin;
            (void)next_chunk(c, g_end, region_read_off, region_hap_off, read_off, hap_off, out_off, true);
            const size_t bo = c.read_byte0, co = c.hap_byte0;
            st = enqueue_compute(h, n_regions, c.rro.data(), c.rho.data(), c.ro.data(), read_bases + bo, base_q + bo, ins_q + bo,
                                 del_q + bo, gcp + bo, c.ho.data(), hap_bases + co, c.oo.data(), out + out_off[g_begin], &p);
        }
        const double t1 = now();
        if (st == PHMM_OK) st = finish_compute(h, &p);
        if (trace)
            fprintf(stderr, "phmm_compute: plan+stage+enqueue %.1f us, wait+copy-out %.1f us\n", t1 - t0, now() - t1);
        return st;
    }
    // ---- large batch: chunks of regions rotate through kSlots (arena, stream) pairs, so the host staging
    //      and the H2D copy of chunk i+1 overlap the kernels of chunk i.  Results are identical: every
    //      region is independent, the chunk only rebases the offsets. -----------------------------------
    PendingCompute pend[kSlots];
    struct Drain {  // an exception on the way (host allocation) must not leave chunks in flight
        phmm_handle *h;
        PendingCompute *pend;
        ~Drain() {
            for (int i = 0; i < kSlots; ++i)
                if (pend[i].b) {
                    (void)hipStreamSynchronize(h->streams[pend[i].slot]);
                    phmm_batch_destroy(pend[i].b);
                    pend[i].b = nullptr;
                }
            h->slot = 0;
            h->defer_d2h = false;
        }
    } drain{h, pend};
    int st = PHMM_OK;
    ChunkView c;
    c.f32_first = f32_first;
    c.g1 = g_begin;
    {   // same read and haplotype counts and the same first haplotype length everywhere?
        const uint32_t nr0 = region_read_off[g_begin + 1] - region_read_off[g_begin];
        const uint32_t nh0 = region_hap_off[g_begin + 1] - region_hap_off[g_begin];
        const uint32_t hl0 = nh0 ? hap_off[region_hap_off[g_begin] + 1] - hap_off[region_hap_off[g_begin]] : 0;
        for (uint32_t g = g_begin + 1; g < g_end && !c.mixed; ++g)
            c.mixed = region_read_off[g + 1] - region_read_off[g] != nr0 || region_hap_off[g + 1] - region_hap_off[g] != nh0 ||
                      (nh0 && hap_off[region_hap_off[g] + 1] - hap_off[region_hap_off[g]] != hl0);
    }
    int n_chunks = 0;
    h->defer_d2h = true;
    while (st == PHMM_OK && next_chunk(c, g_end, region_read_off, region_hap_off, read_off, hap_off, out_off)) {
        const int slot = n_chunks % kSlots;
        st = finish_compute(h, &pend[slot]);  // the slot's previous chunk must be out of its arena
        if (st != PHMM_OK) break;
        h->slot = slot;
        const size_t bo = c.read_byte0, co = c.hap_byte0;
        st = enqueue_compute(h, c.g1 - c.g0, c.rro.data(), c.rho.data(), c.ro.data(), read_bases + bo, base_q + bo, ins_q + bo,
                             del_q + bo, gcp + bo, c.ho.data(), hap_bases + co, c.oo.data(), out + out_off[c.g0], &pend[slot]);
        ++n_chunks;
    }
    for (int i = 0; i < kSlots; ++i) {  // drain in submission order
        const int slot = (n_chunks + i) % kSlots;
        const int s2 = finish_compute(h, &pend[slot]);
        if (st == PHMM_OK) st = s2;
    }
    h->slot = 0;
    h->defer_d2h = false;
    if (trace) fprintf(stderr, "phmm_compute: %d chunks pipelined over %d slots, total %.1f us\n", n_chunks, kSlots, now() - t0);
    return st;
}

// The regions `list` (any order, any subset) of the caller's arrays on one engine: chunks of the list are staged
// straight from the caller's arrays (a scatter-gather `Parts` entry per region) and rotate through the engine's slots
// like the chunks of compute_range.  What phmm_compute_multi uses when a heavy-tailed set makes contiguous ranges
// unbalanced and regions are dealt out one by one.
int compute_list(phmm_handle *h, const uint32_t *list, uint32_t n_list, const uint32_t *region_read_off,
                 const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *base_q,
                 const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *gcp, const uint32_t *hap_off,
                 const uint8_t *hap_bases, const uint64_t *out_off, double *out) {
    DeviceGuard dg(h->device);
    struct Slot {
        PendingCompute pend;
        Parts parts;
        std::vector<uint32_t> rro, rho, ro, ho;
        std::vector<uint64_t> oo;
    } slots[kSlots];
    struct Drain {
        phmm_handle *h;
        Slot *s;
        ~Drain() {
            for (int i = 0; i < kSlots; ++i)
                if (s[i].pend.b) {
                    (void)hipStreamSynchronize(h->streams[s[i].pend.slot]);
                    phmm_batch_destroy(s[i].pend.b);
                    s[i].pend.b = nullptr;
                }
            h->slot = 0;
            h->defer_d2h = false;
        }
    } drain{h, slots};
    const uint8_t *src[6] = {read_bases, base_q, ins_q, del_q, gcp, hap_bases};
    int st = PHMM_OK, n_chunks = 0;
    h->defer_d2h = true;
    for (uint32_t i0 = 0; i0 < n_list && st == PHMM_OK;) {
        Slot &S = slots[n_chunks % kSlots];
        st = finish_compute(h, &S.pend);  // the slot's previous chunk must be out of its arena (and of S.parts)
        if (st != PHMM_OK) break;
        const size_t limit = std::min(kChunkBytes, kFirstChunkBytes << std::min(n_chunks / 2, 16));
        S.rro.assign(1, 0);
        S.rho.assign(1, 0);
        S.ro.assign(1, 0);
        S.ho.assign(1, 0);
        S.oo.assign(1, 0);
        for (int k = 0; k < 6; ++k) S.parts.src[k].clear();
        S.parts.read_bytes.clear();
        S.parts.hap_bytes.clear();
        S.parts.out.clear();
        S.parts.n_out.clear();
        S.parts.first_region.assign(1, 0);
        uint32_t i1 = i0;
        size_t bytes = 0;
        while (i1 < n_list && S.parts.out.size() < 4096) {
            const uint32_t g = list[i1];
            const uint32_t r0 = region_read_off[g], r1 = region_read_off[g + 1], a0 = region_hap_off[g], a1 = region_hap_off[g + 1];
            const size_t rb = (size_t)read_off[r1] - read_off[r0], hb = (size_t)hap_off[a1] - hap_off[a0];
            if (i1 > i0 && bytes + rb > limit) break;
            bytes += rb;
            for (uint32_t r = r0; r < r1; ++r) S.ro.push_back(S.ro.back() + (read_off[r + 1] - read_off[r]));
            for (uint32_t a = a0; a < a1; ++a) S.ho.push_back(S.ho.back() + (hap_off[a + 1] - hap_off[a]));
            S.rro.push_back(S.rro.back() + (r1 - r0));
            S.rho.push_back(S.rho.back() + (a1 - a0));
            S.oo.push_back(S.oo.back() + (out_off[g + 1] - out_off[g]));
            for (int k = 0; k < 5; ++k) S.parts.src[k].push_back(src[k] + read_off[r0]);
            S.parts.src[5].push_back(hap_bases + hap_off[a0]);
            S.parts.read_bytes.push_back(rb);
            S.parts.hap_bytes.push_back(hb);
            S.parts.out.push_back(out + out_off[g]);
            S.parts.n_out.push_back(out_off[g + 1] - out_off[g]);
            S.parts.first_region.push_back(S.parts.first_region.back() + 1);
            ++i1;
        }
        h->slot = n_chunks % kSlots;
        st = enqueue_compute(h, i1 - i0, S.rro.data(), S.rho.data(), S.ro.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                             S.ho.data(), nullptr, S.oo.data(), nullptr, &S.pend, &S.parts);
        ++n_chunks;
        i0 = i1;
    }
    for (int i = 0; i < kSlots; ++i) {
        const int s2 = finish_compute(h, &slots[(n_chunks + i) % kSlots].pend);
        if (st == PHMM_OK) st = s2;
    }
    h->slot = 0;
    h->defer_d2h = false;
    return st;
}

}  // namespace phmm_host

extern "C" {

int phmm_compute(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                 const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                 const uint8_t *del_q, const uint8_t *gcp, const uint32_t *hap_off, const uint8_t *hap_bases,
                 const uint64_t *out_off, double *out) {
    if (!h) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
    phmm_host::latch_slot0(h);
    // the whole batch is checked before anything is indexed: the chunked path walks the caller's arrays
    h->err_code = PHMM_OK;
    if (tl_err_h == h) tl_err_h = nullptr;
    if (const char *bad = validate_offsets(n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, nullptr)) {
        h->err = bad;
        return h->err_code = PHMM_ERR_INVALID_ARG;
    }
    const uint32_t n_reads = region_read_off[n_regions];
    if ((read_off[n_reads] && (!read_bases || !base_q || !ins_q || !del_q || !gcp)) ||
        (hap_off[region_hap_off[n_regions]] && !hap_bases) || (out_off[n_regions] && !out)) {
        h->err = "phmm_compute: null pointer";
        return h->err_code = PHMM_ERR_INVALID_ARG;
    }
    // (one of many private handles on the device: opt-in, PHMM_ROUTE_SHARED, a one-shot call goes through the device's shared handle.
    // The PairHMM alone through the region server -- built in round 6 -- gave a wrong likelihood once in 150 000 calls of the ragged
    // mix under TB_VERIFY and was taken out again; the whole region call, whose waves go on to the alignment, soaks clean.)
    if (n_regions < 8 || (size_t)read_off[n_reads] <= kOneShotBytes)
        if (phmm_handle *via = route_shared(h)) {
            uint64_t ticket = 0;
            int st = phmm_submit(via, n_regions, region_read_off, region_hap_off, read_off, read_bases, base_q, ins_q, del_q, gcp, hap_off, hap_bases,
                                 out_off, out, &ticket);
            if (st == PHMM_OK) st = phmm_wait(via, ticket);
            if (st != PHMM_OK) {
                h->err = phmm_last_error(via);
                h->err_code = st;
            }
            return st;
        }
    return compute_range(h, 0, n_regions, region_read_off, region_hap_off, read_off, read_bases, base_q, ins_q, del_q, gcp,
                         hap_off, hap_bases, out_off, out);
    PHMM_GUARD_END(h, "phmm_compute", PHMM_FAIL_CODE)
}

namespace {

struct PendingEngine {
    phmm_batch *b = nullptr;
    int slot = 0;
    hipStream_t stream = nullptr;  // the stream the batch was enqueued on
    bool zero_copy = false;        // the kernels stored the results into the pinned mirror
    double *out = nullptr;
    uint8_t *keep = nullptr;
    size_t res_off = 0, keep_bytes = 0, res_bytes = 0;
    uint32_t n_reads = 0;
    bool d2h_pending = false;
};

// Stage one batch of the engine-level call in the current slot's arena and enqueue H2D, pre-step, PairHMM, post-step
// and D2H on its stream.  No sync.
int engine_enqueue(phmm_handle *h, const phmm_engine_config *cfg, uint32_t n_regions, const uint32_t *region_read_off,
                   const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *base_q,
                   const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *mapq, const uint32_t *hap_off,
                   const uint8_t *hap_bases, const int32_t *region_ref_hap, const uint64_t *out_off, double *out, uint8_t *keep,
                   PendingEngine *pending) {
    const uint32_t n_reads = region_read_off[n_regions];
    const size_t rbytes = align_up((size_t)read_off[n_reads], 256);
    // originals (4 x read bytes + mapq + ref index) and device-only copies (4 x read bytes, thresholds, keep)
    const size_t extra = 4 * rbytes + 4 * rbytes + align_up((size_t)n_reads, 256) * 2 + align_up((size_t)n_reads * 8, 256) +
                         align_up((size_t)n_regions * 4, 256) + 18 * 256;
    phmm_batch *b = batch_create_impl(h, n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, true, extra);
    if (!b) return h->err_code ? h->err_code : PHMM_ERR_INVALID_ARG;
    int st = PHMM_OK;
    if ((b->read_bytes && (!read_bases || !base_q)) || (n_reads && (!mapq || !keep)) || (b->hap_bytes && !hap_bases) ||
        (b->n_out && !out)) {
        h->err = "phmm_engine_compute: null pointer";
        st = PHMM_ERR_INVALID_ARG;
    }
    Arena &A = h->A();
    if (st == PHMM_OK) {
        bool fits = true;
        auto place = [&](const void *src, size_t bytes) -> char * {  // into the mirror (travels in the one H2D copy)
            const size_t off = align_up(A.used, 256);
            if (off + bytes > A.cap) {
                fits = false;
                return A.dev;
            }
            A.used = off + bytes;
            if (src && bytes) memcpy(A.host + off, src, bytes);
            return A.dev + off;
        };
        const uint8_t *d_bases = (const uint8_t *)place(read_bases, b->read_bytes);
        const uint8_t *d_q0 = (const uint8_t *)place(base_q, b->read_bytes);
        const uint8_t *d_i0 = ins_q ? (const uint8_t *)place(ins_q, b->read_bytes) : nullptr;
        const uint8_t *d_d0 = del_q ? (const uint8_t *)place(del_q, b->read_bytes) : nullptr;
        const uint8_t *d_mapq = (const uint8_t *)place(mapq, n_reads);
        const uint8_t *d_haps = (const uint8_t *)place(hap_bases, b->hap_bytes);
        const int32_t *d_ref = region_ref_hap ? (const int32_t *)place(region_ref_hap, (size_t)n_regions * 4) : nullptr;
        // (a zeroed status block that travels with the inputs: what the kernels of a small call flag, see below)
        uint32_t *d_status_in = (uint32_t *)place(nullptr, 256);
        if (fits) memset(A.host + ((char *)d_status_in - A.dev), 0, 256);
        const size_t in_bytes = align_up(A.used, 256);
        // device-only
        uint8_t *d_q = (uint8_t *)place(nullptr, b->read_bytes), *d_i = (uint8_t *)place(nullptr, b->read_bytes),
                *d_d = (uint8_t *)place(nullptr, b->read_bytes), *d_g = (uint8_t *)place(nullptr, b->read_bytes);
        double *d_thr = (double *)place(nullptr, (size_t)n_reads * 8);
        // results: [status (256 B) | keep | out] contiguous, one D2H
        const size_t res_off = align_up(A.used, 256);
        const size_t keep_bytes = align_up((size_t)n_reads, 256);
        A.used = res_off + 256 + keep_bytes + b->n_out * 8;
        if (!fits || A.used > A.cap) {  // cannot happen: `extra` above reserves for exactly this layout
            h->err = "phmm_engine_compute: internal error, arena too small";
            std::string keep_err = h->err;
            phmm_batch_destroy(b);
            h->err = keep_err;
            return PHMM_ERR_HIP;
        }
        b->d_status = (uint32_t *)(A.dev + res_off);
        uint8_t *d_keep = (uint8_t *)(A.dev + res_off + 256);
        double *d_out = (double *)(A.dev + res_off + 256 + keep_bytes);
        const size_t res_bytes = 256 + keep_bytes + b->n_out * 8;
        // A small one-shot call (a region per call, the reference's pattern) does without the copy engine, like
        // phmm_compute: a kernel fetches the inputs from the pinned mirror, and the post-step stores keep flags and
        // normalised likelihoods -- and hands on the status word -- straight into it.
        char *mirror = nullptr;
        if (zero_copy_allowed(h) && b->tight_out && n_reads && in_bytes <= kStageInBytes && res_bytes <= kZeroCopyOutBytes) {
            void *dp = nullptr;
            if (hipHostGetDevicePointer(&dp, A.host, 0) == hipSuccess && dp) mirror = (char *)dp;
        }
        bool ok;
        if (mirror) {
            b->d_status = d_status_in;
            canary_staged(h, A, in_bytes);
            ok = hip_ok(h, launch_stage_in(mirror, A.dev, in_bytes, h->S()), "phmm_stage_in_kernel");
        } else {
            ok = hip_ok(h, hipMemcpyAsync(A.dev, A.host, in_bytes, hipMemcpyHostToDevice, h->S()), "H2D batch") &&
                 hip_ok(h, hipMemsetAsync(b->d_status, 0, 256, h->S()), "memset status");
        }
        // the post-step consumes the likelihoods on the device, so the exact pass below kRescueBelow rides in-stream
        // between the forward kernels and the post-step (phmm_batch_launch); nothing of this slot is in flight now
        if (ok && n_reads && !h->sw.no_rescue) {
            ok = ensure_arena_rescue(h, A, b->plan.max_h, &b->rescue_blocks);
            if (ok) b->rescue_scratch = A.rescue;
        }
        uint32_t max_r = 0;
        for (uint32_t r = 0; r < n_reads; ++r) max_r = std::max(max_r, read_off[r + 1] - read_off[r]);
        PrepParams pp{};
        pp.n_reads = n_reads;
        pp.read_off = b->d_read_off;
        pp.read_bases = d_bases;
        pp.base_q = d_q0;
        pp.ins_q = d_i0;
        pp.del_q = d_d0;
        pp.mapq = d_mapq;
        pp.pcr_cache = cfg->pcr_error_model ? h->d_pcr_cache + 128 * cfg->pcr_error_model : nullptr;
        pp.out_q = d_q;
        pp.out_ins = d_i;
        pp.out_del = d_d;
        pp.out_gcp = d_g;
        pp.threshold = d_thr;
        pp.lds_rows = (uint32_t)align_up((size_t)max_r + 1, 8);
        pp.waves_per_read = n_reads <= 2048 ? std::max<uint32_t>(1, (max_r + 63) / 64) : 1;  // few reads: a wave per 64 positions
        pp.default_indel_qual = 45;  // ReadUtils::DEFAULT_INSERTION_DELETION_QUAL (read_utils.rs:23)
        pp.constant_gcp = cfg->constant_gcp;
        pp.base_quality_score_threshold = cfg->base_quality_score_threshold;
        pp.disable_cap_to_mapq = cfg->disable_cap_read_qualities_to_mapq;
        pp.dynamic_disqualification = cfg->dynamic_read_disqualification;
        pp.read_disqualification_scale = cfg->read_disqualification_scale;
        pp.expected_error_rate_per_base = cfg->expected_error_rate_per_base;
        if (ok && (size_t)pp.lds_rows * 17 * 4 > kLdsBytesPerCU) {
            h->err = "phmm_engine_compute: read too long for the pre-step kernel";
            ok = false;
            st = PHMM_ERR_INVALID_ARG;
        }
        if (ok) ok = hip_ok(h, launch_prep(pp, h->S()), "phmm_prep_reads");
        if (ok) ok = phmm_batch_bind_device(b, d_bases, d_q, d_i, d_d, d_g, d_haps, d_out) == PHMM_OK;
        if (ok) ok = phmm_batch_launch(b, nullptr) == PHMM_OK;
        PostParams po{};
        po.n_reads = n_reads;
        po.read_region = b->d_read_region;
        po.region_read_off = b->d_region_read_off;
        po.region_hap_off = b->d_region_hap_off;
        po.out_off = b->d_out_off;
        po.region_ref_hap = d_ref;
        po.out = d_out;
        po.out_final = mirror ? (double *)(mirror + res_off + 256 + keep_bytes) : nullptr;
        po.threshold = d_thr;
        po.keep = mirror ? (uint8_t *)(mirror + res_off + 256) : d_keep;
        po.status_in = mirror ? b->d_status : nullptr;
        po.status_out = mirror ? (uint32_t *)(mirror + res_off) : nullptr;
        po.max_likelihood_difference_cap = cfg->log10_global_read_mismapping_rate;
        po.symmetric = cfg->symmetrically_normalize_alleles_to_reference;
        if (ok) ok = hip_ok(h, launch_post(po, h->S()), "phmm_post_reads");
        const bool eager = eager_d2h(h);  // otherwise engine_finish fetches the results
        if (ok && eager && !mirror)
            ok = hip_ok(h, hipMemcpyAsync(A.host + res_off, A.dev + res_off, res_bytes, hipMemcpyDeviceToHost, h->S()),
                        "D2H results");
        if (ok) {
            pending->res_bytes = res_bytes;
            pending->d2h_pending = !eager && !mirror;
            pending->b = b;
            pending->slot = h->slot;
            pending->out = out;
            pending->keep = keep;
            pending->stream = h->S();
            pending->zero_copy = mirror != nullptr;
            pending->res_off = res_off;
            pending->keep_bytes = keep_bytes;
            pending->n_reads = n_reads;
            return PHMM_OK;
        }
        if (st == PHMM_OK) st = PHMM_ERR_HIP;
    }
    std::string keep_err = h->err;
    (void)hipStreamSynchronize(h->S());
    phmm_batch_destroy(b);
    h->err = keep_err;
    return st;
}

// Wait for a pending engine batch, hand keep flags and likelihoods to the caller, release the batch.
int engine_finish(phmm_handle *h, PendingEngine *p) {
    if (!p->b) return PHMM_OK;
    int st = PHMM_OK;
    phmm_batch *b = p->b;
    Arena &A = h->arenas[p->slot];
    hipStream_t S = p->stream ? p->stream : h->streams[p->slot];
    if (!hip_ok(h, wait_stream(h, S), "sync") ||
        (p->d2h_pending &&
         (!hip_ok(h, hipMemcpyAsync(A.host + p->res_off, A.dev + p->res_off, p->res_bytes, hipMemcpyDeviceToHost, S),
                  "D2H results") ||
          !hip_ok(h, wait_stream(h, S), "sync(D2H)")))) {
        st = PHMM_ERR_HIP;
    } else {
        const char *hs = A.host + p->res_off;
        if (p->n_reads) memcpy(p->keep, hs + 256, p->n_reads);
        const double *v = (const double *)(hs + 256 + p->keep_bytes);
        if (b->tight_out) {
            if (b->n_out) memcpy(p->out, v, b->n_out * 8);
        } else {  // gaps the caller left in out_off stay untouched
            for (const auto &e : b->out_extents)
                if (e.second) memcpy(p->out + e.first, v + e.first, e.second * 8);
        }
        if (status_positive(*(const uint32_t *)hs, b->rescue_scratch != nullptr && !h->sw.no_rescue)) {
            h->err = "PairHmm Log Probability cannot be greater than 0.0";  // pair_hmm.rs:478-481
            st = PHMM_ERR_POSITIVE_RESULT;
        }
        if (p->zero_copy && !canary_after_call(h, A, p->res_off, p->res_bytes) && st == PHMM_OK) st = PHMM_ERR_INTERNAL;
    }
    std::string keep_err = h->err;
    phmm_batch_destroy(b);
    h->err = keep_err;
    p->b = nullptr;
    return st;
}

}  // namespace

int phmm_engine_compute(phmm_handle *h, const phmm_engine_config *cfg, uint32_t n_regions,
                        const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                        const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q,
                        const uint8_t *mapq, const uint32_t *hap_off, const uint8_t *hap_bases,
                        const int32_t *region_ref_hap, const uint64_t *out_off, double *out, uint8_t *keep) {
    if (!h || !cfg) return PHMM_ERR_INVALID_ARG;
    PHMM_GUARD_BEGIN
    phmm_host::latch_slot0(h);
    h->err_code = PHMM_OK;
    if (tl_err_h == h) tl_err_h = nullptr;
    if (cfg->pcr_error_model > 3) {
        h->err = "phmm_engine_compute: Unknown PCR Error Model";  // engine.rs:89
        return h->err_code = PHMM_ERR_INVALID_ARG;
    }
    // the whole batch is checked before anything is indexed: the chunked path below walks the caller's arrays
    if (const char *bad = validate_offsets(n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off, nullptr)) {
        h->err = bad;
        return h->err_code = PHMM_ERR_INVALID_ARG;
    }
    const uint32_t n_reads = region_read_off[n_regions];
    if ((read_off[n_reads] && (!read_bases || !base_q)) || (n_reads && (!mapq || !keep)) ||
        (hap_off[region_hap_off[n_regions]] && !hap_bases) || (out_off[n_regions] && !out)) {
        h->err = "phmm_engine_compute: null pointer";
        return h->err_code = PHMM_ERR_INVALID_ARG;
    }
    if (n_regions < 8 || (size_t)read_off[n_reads] <= kOneShotBytes)
        if (phmm_handle *via = route_shared(h)) {  // (one of many private handles on the device: phmm_compute has the comment)
            uint64_t ticket = 0;
            int st = phmm_engine_submit(via, cfg, n_regions, region_read_off, region_hap_off, read_off, read_bases, base_q, ins_q, del_q, mapq, hap_off,
                                        hap_bases, region_ref_hap, out_off, out, keep, &ticket);
            if (st == PHMM_OK) st = phmm_wait(via, ticket);
            if (st != PHMM_OK) {
                h->err = phmm_last_error(via);
                h->err_code = st;
            }
            return st;
        }
    DeviceGuard dg(h->device);
    // ---- small / medium batch: one shot ------------------------------------------------------------
    if (n_regions < 8 || (size_t)read_off[n_reads] <= kOneShotBytes || h->sw.no_pipeline) {
        h->slot = 0;
        PendingEngine p;
        int st = engine_enqueue(h, cfg, n_regions, region_read_off, region_hap_off, read_off, read_bases, base_q, ins_q, del_q,
                                mapq, hap_off, hap_bases, region_ref_hap, out_off, out, keep, &p);
        if (st == PHMM_OK) st = engine_finish(h, &p);
        return st;
    }
    // ---- large batch: chunks of regions through the kSlots (arena, stream) pairs, like phmm_compute ----
    PendingEngine pend[kSlots];
    struct Drain {  // an exception on the way (host allocation) must not leave chunks in flight
        phmm_handle *h;
        PendingEngine *pend;
        ~Drain() {
            for (int i = 0; i < kSlots; ++i)
                if (pend[i].b) {
                    (void)hipStreamSynchronize(h->streams[pend[i].slot]);
                    phmm_batch_destroy(pend[i].b);
                    pend[i].b = nullptr;
                }
            h->slot = 0;
            h->defer_d2h = false;
        }
    } drain{h, pend};
    int st = PHMM_OK;
    ChunkView c;
    int n_chunks = 0;
    h->defer_d2h = true;
    while (st == PHMM_OK && next_chunk(c, n_regions, region_read_off, region_hap_off, read_off, hap_off, out_off)) {
        const int slot = n_chunks % kSlots;
        st = engine_finish(h, &pend[slot]);  // the slot's previous chunk must be out of its arena
        if (st != PHMM_OK) break;
        h->slot = slot;
        const size_t bo = c.read_byte0, co = c.hap_byte0;
        st = engine_enqueue(h, cfg, c.g1 - c.g0, c.rro.data(), c.rho.data(), c.ro.data(), read_bases ? read_bases + bo : nullptr,
                            base_q ? base_q + bo : nullptr, ins_q ? ins_q + bo : nullptr, del_q ? del_q + bo : nullptr,
                            mapq ? mapq + c.r0 : nullptr, c.ho.data(), hap_bases ? hap_bases + co : nullptr,
                            region_ref_hap ? region_ref_hap + c.g0 : nullptr, c.oo.data(), out ? out + out_off[c.g0] : nullptr,
                            keep ? keep + c.r0 : nullptr, &pend[slot]);
        ++n_chunks;
    }
    for (int i = 0; i < kSlots; ++i) {  // drain in submission order
        const int slot = (n_chunks + i) % kSlots;
        const int s2 = engine_finish(h, &pend[slot]);
        if (st == PHMM_OK) st = s2;
    }
    h->slot = 0;
    h->defer_d2h = false;
    return st;
    PHMM_GUARD_END(h, "phmm_engine_compute", PHMM_FAIL_CODE)
}

int phmm_set_switch(phmm_handle *h, const char *name, int value) {
    if (!h || !name) return PHMM_ERR_INVALID_ARG;
    Switches &w = h->sw;
    const std::string n(name);
    if (n == "force_L") w.force_L = value > 0 ? value : 0;
    else if (n == "force_chain") w.force_chain = value;
    else if (n == "force_streams") w.force_streams = value > 0 ? value : 0;
    else if (n == "no_pipeline") w.no_pipeline = value != 0;
    else if (n == "no_rescue") w.no_rescue = value != 0;
    else if (n == "trace") w.trace = value != 0;
    else if (n == "sw_lite") {
        w.sw_lite = value;
        h->swork.lite_skip = 0;  // (what earlier calls have taught the handle starts over)
    }
    else if (n == "sw_chunks") w.sw_chunks = value > 0 ? value : 0;
    else if (n == "sw_transpose") w.sw_transpose = value < 0 ? -1 : value > 0 ? 1 : 0;
    else if (n == "sw_no_zero_copy") w.sw_no_zero_copy = value > 0;
    else if (n == "sw_clock") w.sw_clock = value != 0;
    else if (n == "region_sw_all") w.region_sw_all = value < 0 ? -1 : value;
    else if (n == "region_server") w.region_server = value < 0 ? -1 : value > 0 ? 1 : 0;
    else if (n == "server_idle_us") w.server_idle_us = value > 0 ? value : 1;
    else if (n == "server_trace") w.server_trace = value != 0;
    else if (n == "region_flag_wait") w.region_flag_wait = value != 0;
    else if (n == "region_pick_timeout_us") w.region_pick_timeout_us = value > 0 ? value : 1;
    else if (n == "region_debug_pick") w.region_debug_pick = value > 0 ? value : 0;
    else if (n == "mirror_canary") w.mirror_canary = value > 0 ? value : 0;
    else if (n == "route_shared") w.route_shared = value;
    else if (n == "asm_fingerprint_bits") w.asm_fingerprint_bits = value > 0 && value < 64 ? value : 0;
    else if (n == "sw_lanes") w.sw_lanes = value == 8 || value == 16 || value == 32 || value == 64 ? value : 0;
    else {
        h->err = "phmm_set_switch: unknown switch";
        return PHMM_ERR_INVALID_ARG;
    }
    h->sw_touched = true;  // (its calls stay on its own resources from now on: route_shared)
    if (h->comb) phmm_host::combiner_set_switches(h->comb, w);
    return PHMM_OK;
}

uint64_t phmm_get_stat(phmm_handle *h, const char *name) {
    if (!h || !name) return 0;
    const std::string n(name);
    uint64_t own = 0;
    if (n == "staged_bytes") own = h->stat_staged_bytes;
    else if (n == "rescue_passes") own = h->stat_rescue_passes;
    else if (n == "sw_kernel_us") return h->swork.last_kernel_us;
    else if (n == "sw_backtrack_bytes") return h->swork.last_backtrack_bytes;
    else if (n == "sw_second_pass") return h->swork.last_second_pass;
    else if (n == "sw_instance") return h->swork.last_instance;
    else if (n == "sw_instance_second") return h->swork.last_instance_second;
    else if (n == "sw_clock_mhz") return h->swork.last_clock_mhz;
    else if (n == "region_sw_all") own = h->swork.region_sw_all_calls;
    else if (n == "region_pick_timeouts") own = h->swork.region_pick_timeouts;
    else if (n.rfind("server_", 0) == 0) return phmm_host::server_stat(h->device, name);  // (the device's server: every handle's calls)
    else return 0;
    return own + (h->comb ? phmm_host::combiner_stat(h->comb, name) : 0);
}

int phmm_plan_describe(unsigned flags, uint32_t concurrent_callers, uint32_t n_regions, const uint32_t *region_read_off,
                       const uint32_t *region_hap_off, const uint32_t *read_off, const uint32_t *hap_off, phmm_plan_info *info) {
    if (!info) return PHMM_ERR_INVALID_ARG;
    try {
        memset(info, 0, sizeof *info);
        std::vector<uint64_t> oo((size_t)n_regions + 1, 0);
        if (region_read_off && region_hap_off)
            for (uint32_t g = 0; g < n_regions; ++g)
                oo[g + 1] = oo[g] + (uint64_t)(region_read_off[g + 1] - region_read_off[g]) * (region_hap_off[g + 1] - region_hap_off[g]);
        if (validate_offsets(n_regions, region_read_off, region_hap_off, read_off, hap_off, oo.data(), nullptr)) return PHMM_ERR_INVALID_ARG;
        Switches sw;  // the planner's switches: this process's PHMM_* environment
        read_env_switches(sw);
        const BatchPlan plan = plan_batch(BatchOffsets{n_regions, region_read_off, region_hap_off, read_off, hap_off, oo.data()}, sw, flags,
                                          concurrent_callers ? concurrent_callers : 1u);
        info->cells = plan.cells;
        info->n_launches = num_launches(plan);
        for (const auto &g : plan.chain_groups) {
            info->n_chain_launches += 1;
            info->chain_items += g.items.size();
            uint32_t fewest = 0xffffffffu;
            for (const ChainItem &it : g.items) fewest = std::min(fewest, it.read_end - it.read_begin);
            info->min_reads_per_run = info->min_reads_per_run ? std::min(info->min_reads_per_run, fewest) : fewest;
        }
        for (const auto &c : plan.classes)
            if (c.chain) info->chain_cells += c.cells;
        info->swept_cells = plan.swept_cells;
        info->pad_column_cells = plan.pad_column_cells;
        info->pad_slot_cells = plan.pad_slot_cells;
        snprintf(info->dominant_kernel, sizeof info->dominant_kernel, "%s", plan.dominant.c_str());
        return PHMM_OK;
    } catch (const std::bad_alloc &) {
        return PHMM_ERR_NO_MEMORY;
    } catch (...) {
        return PHMM_ERR_INTERNAL;
    }
}

uint64_t phmm_batch_cells(const phmm_batch *b) { return b ? b->plan.cells : 0; }
uint64_t phmm_batch_algorithmic_bytes(const phmm_batch *b) { return b ? b->plan.alg_bytes : 0; }
uint32_t phmm_batch_num_launches(const phmm_batch *b) {
    return b ? num_launches(b->plan) : 0;
}
const char *phmm_batch_dominant_kernel(const phmm_batch *b) { return b ? b->plan.dominant.c_str() : ""; }

}  // extern "C"
