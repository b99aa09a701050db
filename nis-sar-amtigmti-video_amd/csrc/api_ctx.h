// What the host units of the C ABI share (api_ctx.hip, api_csa.hip, api_focus.hip, api_comm.hip; the detection chain's api_gmti.hip,
// api_oscfar.hip, api_cluster.hip, api_atigate.hip, api_track.hip, api_balance.hip, api_coherence.hip, api_relocate.hip through api_gmti.h; the back-projection's
// api_tdbp_search.hip, api_tdbp_pair.hip, api_tdbp_pair_search.hip through api_tdbp.h): the context behind sarx_ctx*, its per-lane scratch,
// error reporting, the exception guard and the staged host copies.  Host only: no kernel file includes this header.
#pragma once
#include "../../include/sarx.h"
#include "../../include/sarx_gmti.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <new>
#include <string>

typedef struct ncclComm* ncclComm_t;     // as <rccl/rccl.h> declares it; api_comm.hip alone includes that header

constexpr double C_LIGHT = 299792458.0;     // sar_ati_dcpa_sim_csa.py:211
constexpr int N_EVENTS = 256;
constexpr int TW_MAX = 16384;

struct sarx_ctx;
namespace sarx {
// Grow-only device scratch of one lane.  tdbp_plan.h's grow does the same for a plan; it lives with the kernels, which see no context.
struct LaneScratch {
    void* p = nullptr;
    size_t cap = 0;                    // bytes p holds
    int grow(sarx_ctx* c, size_t bytes);       // p holds at least bytes; what it held is not kept
};
}  // namespace sarx

struct sarx_ctx {
    int device = -1;
    int cus = 256;                     // compute units of this device (persistent grids are sized from it)
    hipStream_t stream = nullptr;      // the CURRENT lane's stream: everything is enqueued here
    static constexpr int LANES = 4;
    hipStream_t lane[LANES] = {};      // lane 0 = the stream made by sarx_init; the others on first sarx_select_lane
    hipEvent_t lane_ev[LANES] = {};
    int cur_lane = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev[N_EVENTS] = {};
    bool ev_set[N_EVENTS] = {};
    hipEvent_t comm_fence = nullptr;
    hipEvent_t comm_done = nullptr;
    hipEvent_t comm_mark[4] = {};      // sarx_comm_mark / sarx_comm_wait_mark: "gathers enqueued up to here are finished"
    bool comm_mark_set[4] = {};
    float2* tw_all = nullptr;          // table for size n at offset n: exp(-2 pi i m/n)
    float* ati_part_max_all = nullptr;     // reduction scratch, one set per lane (two frames in flight must not share it)
    double2* ati_part_sum_all = nullptr;
    double* ati_out3_all = nullptr;
    static constexpr int POWER_STRIDE = 2048 + 8;   // per lane: 1024 {sum, max} partials, then the two fp32 noise levels
    double* power_part_all = nullptr;       // sarx_power_stats_dev partials, one set per lane (it used to hipMalloc / hipFree per call)
    float* ati_part_max_() const { return ati_part_max_all + (size_t)cur_lane * 4096; }
    double2* ati_part_sum_() const { return ati_part_sum_all + (size_t)cur_lane * 4096; }
    double* ati_out3_() const { return ati_out3_all + (size_t)cur_lane * 4; }
    // staged host transfers (sarx_memcpy_h2d / _d2h and the *_host entry points, large pageable buffers): COPY_THREADS host
    // threads, each with its own pinned chunk and stream, copy chunk by chunk in parallel with the DMA of the others
    static constexpr int COPY_THREADS = 8;
    static constexpr size_t COPY_CHUNK = (size_t)32 << 20;
    char* pin[COPY_THREADS] = {};
    hipStream_t copy_stream[COPY_THREADS] = {};
    hipEvent_t pin_free[COPY_THREADS] = {};     // "the DMA that last read pinned chunk i has finished"
    int up_streams = COPY_THREADS;     // uploads issue their DMAs on this many of the copy streams (SARX_UP_STREAMS, A/B).  Beside a download in
                                       // flight, 2 GiB each way: 67 ms with eight streams, 75 with two, 76 with one (= one after the other);
                                       // two plain DMAs (page-locked source) 44 ms: the staged upload is bound by the HOST's memory traffic (it
                                       // reads the array, writes the chunk, and the DMA reads the chunk again), not by the stream count
                                       // (profiles/r05_i_duplex.log)
    std::mutex copy_mu;                // the pinned chunks and copy streams are per-ctx state: one staged copy at a time
    // overlapped host transfers (sarx_memcpy_h2d_unordered, sarx_memcpy_d2h_begin / _end): downloads run on their own stream behind an
    // event of the producing lane, uploads into free buffers do not wait for enqueued GPU work - PCIe is full duplex
    static constexpr int DL_SLOTS = 8;
    hipStream_t dl_stream = nullptr, up_stream = nullptr;
    hipEvent_t dl_ready[DL_SLOTS] = {};    // recorded on the producing lane
    hipEvent_t dl_done[DL_SLOTS] = {};     // recorded on dl_stream behind the copy
    bool dl_busy[DL_SLOTS] = {};
    ncclComm_t comm = nullptr;
    int n_ranks = 0, rank = 0;
    int range_cus = 0;                 // > 0: persistent range launches size their grid for this many CUs (sarx_set_range_cus; frames in flight)
    int range_impl = 0;                // SARX_RANGE_IMPL: 0 auto, 1 = 16 pts/thread, 2 = 32 pts/thread split exchange, 3 = fused wave-private, 4 = sixteen-wave permuted-spectrum pair
    // device scratch that an entry point keeps between calls, one of each per lane (two frames in flight must not share it): the unordered
    // report list sarx_gmti_refine_dev sorts from, the S_k that sarx_refocus_dev's record launch reads when the caller passes no curves, the
    // keep flags between sarx_atigate_step_dev's two launches, the sort keys between sarx_relocate_dev's two
    enum Scratch { GMTI_COPY, REFOCUS_CURVES, ATIGATE_KEEP, RELOCATE_KEYS, N_SCRATCH };
    sarx::LaneScratch scratch[N_SCRATCH][LANES];
    sarx::LaneScratch& lane_scratch(Scratch k) { return scratch[k][cur_lane]; }
    std::string err;
};

namespace sarx { struct Tdbp; }
struct sarx_tdbp_plan {                // made and destroyed by api_focus.hip
    sarx_ctx* ctx = nullptr;
    sarx::Tdbp* t = nullptr;
    int n_p = 0, n_s = 0, nx = 0, ny = 0;
    float2* d_raw = nullptr;           // staging for the host entry points
    int search_chunks = 0;             // sarx_tdbp_search_set_chunks
};

namespace sarx {

// the plans alive (api_focus.hip, beside their creation), so that an entry point can refuse a destroyed one without reading it
void tdbp_plan_register(const sarx_tdbp_plan* p, bool alive);      // sarx_tdbp_plan_create / _destroy
bool tdbp_plan_live(const sarx_tdbp_plan* p);
extern thread_local std::string g_init_error;     // what sarx_last_error(NULL) returns: failures before a context exists (api_ctx.hip)
int fail(sarx_ctx* c, int code, const char* fmt, ...);
// The plan's turn in an entry point's refusals, after everything that needs no plan and before what needs its pulse count: NULL, or
// not (or no longer) one that sarx_tdbp_plan_create returned.  A usable plan's device is made current and *c is its context.
inline int tdbp_plan_usable(const sarx_tdbp_plan* p, sarx_ctx** c) {
    if (!p) return fail(nullptr, SARX_ERR_INVALID, "plan is NULL");
    if (!tdbp_plan_live(p)) return fail(nullptr, SARX_ERR_INVALID, "plan is not a live sarx_tdbp_plan (destroyed?)");
    *c = p->ctx;
    hipSetDevice(p->ctx->device);
    return SARX_OK;
}
#define HIPCHK(c, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), SARX_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define NEED_CTX(c) do { if (!(c)) return fail(nullptr, SARX_ERR_INVALID, "ctx is NULL"); hipSetDevice((c)->device); } while (0)
// p->d_raw, the device staging [n_p][n_s] of the host entry points' raw pulses, made by the first of them
inline int tdbp_plan_raw(sarx_ctx* c, sarx_tdbp_plan* p) {
    const size_t n = (size_t)p->n_p * p->n_s;
    if (!p->d_raw) HIPCHK(c, hipMalloc(&p->d_raw, n * sizeof(float2)));
    return SARX_OK;
}
// Frees only when p holds less than is asked, behind everything enqueued on the current lane; a frame loop allocates once per lane.
inline int LaneScratch::grow(sarx_ctx* c, size_t bytes) {
    if (bytes <= cap) return SARX_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(p));
    p = nullptr; cap = 0;
    HIPCHK(c, hipMalloc(&p, bytes));
    cap = bytes;
    return SARX_OK;
}

// No C++ exception crosses the C ABI: entry points that allocate on the host (new, std::vector, std::string) run their body through
// this guard; std::bad_alloc becomes SARX_ERR_NOMEM, anything else SARX_ERR_DEVICE, the message is set without allocating again.
template <class F> int guarded(sarx_ctx* c, F&& body) noexcept {
    int code = SARX_ERR_DEVICE;
    const char* what = "unexpected C++ exception inside libsarx";
    try {
        return body();
    } catch (const std::bad_alloc&) {
        code = SARX_ERR_NOMEM; what = "out of host memory";
    } catch (...) {
    }
    try { if (c) c->err.assign(what); else g_init_error.assign(what); } catch (...) {}
    return code;
}

// every lane's stream (sarx_select_lane): host-visible operations are ordered after all of them
hipError_t sync_all_lanes(sarx_ctx* c);
// blocking host <-> device copy of a large pageable buffer, staged through pinned chunks by COPY_THREADS threads (api_ctx.hip)
hipError_t staged_copy(sarx_ctx* c, void* dst, const void* src, size_t bytes, bool to_device, bool narrow = false, bool ordered = true,
                       bool lane_only = false);
bool is_page_locked(const void* p);

void comm_release(sarx_ctx* c);          // sarx_destroy's call into api_comm.hip: the communicator goes with the context

}  // namespace sarx
