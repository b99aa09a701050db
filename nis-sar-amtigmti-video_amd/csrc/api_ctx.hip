// libsarx C ABI (include/sarx.h), context and transfers: sarx_ctx and its lifecycle, memory, the threaded staged-copy engine, the
// download slots, lanes and events, and the hooks of the sanitizer build.
#include "api_ctx.h"
#include "csa_kernels.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <vector>

using namespace sarx;

namespace sarx {

thread_local std::string g_init_error;

int fail(sarx_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_init_error = buf;
    return code;
}

hipError_t sync_all_lanes(sarx_ctx* c) {
    for (int k = 0; k < sarx_ctx::LANES; ++k)
        if (c->lane[k]) { hipError_t e = hipStreamSynchronize(c->lane[k]); if (e != hipSuccess) return e; }
    return hipSuccess;
}

// The runtime calls staged_copy makes, behind function pointers: the sanitizer build (make asan, -DSARX_TESTING) replaces them with host
// stand-ins so that the chunking, the thread / inline-share / join logic and the error paths run under AddressSanitizer on a box
// without a GPU (tests/asan/abi_asan_test.cpp).  The product never changes the table.
struct CopyOps {
    hipError_t (*memcpy_async)(void*, const void*, size_t, hipMemcpyKind, hipStream_t) = hipMemcpyAsync;
    hipError_t (*stream_sync)(hipStream_t) = hipStreamSynchronize;
    hipError_t (*stream_create)(hipStream_t*, unsigned) = hipStreamCreateWithFlags;
    hipError_t (*event_create)(hipEvent_t*, unsigned) = hipEventCreateWithFlags;
    hipError_t (*event_record)(hipEvent_t, hipStream_t) = hipEventRecord;
    hipError_t (*event_sync)(hipEvent_t) = hipEventSynchronize;
    hipError_t (*host_alloc)(void**, size_t, unsigned) = [](void** p, size_t n, unsigned f) { return hipHostMalloc(p, n, f); };
    hipError_t (*set_device)(int) = hipSetDevice;
    bool (*page_locked)(const void*) = [](const void* p) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return true;
        (void)hipGetLastError();               // a pointer the runtime does not know is ordinary pageable memory: clear that error
        return false;
    };
    bool (*may_start_thread)(int) = [](int) { return true; };     // false = behave as if std::thread threw for share i
};
static CopyOps g_ops;

// Host <-> device copy of a large pageable buffer.  hipMemcpy from pageable memory runs at 8 GB/s here and into untouched
// memory (a fresh NumPy array) at 13 GB/s (tools/pcibench.hip); eight threads staging 32 MiB chunks through pinned buffers reach
// 51-54 GB/s both ways.  Blocking; ordered after everything on the ctx stream.  Small copies take the plain path.
// narrow: (host -> device only) the host buffer holds complex128 and is rounded to complex64 on the way into the pinned chunk
// (the reference's arrays are complex128; a NumPy astype of 2^28 elements costs more than the whole transfer)
// ordered = false (uploads into a buffer no enqueued work touches, downloads of data already complete): the copy does not wait for
// the lanes and runs on streams of its own, so it overlaps whatever the GPU is doing
// ordered: the copy waits for every lane's enqueued work (the buffer may have been written on any of them); lane_only: it waits for
// the CURRENT lane only and is issued behind it (a table that only this lane's launches read: the other lanes keep running)
hipError_t staged_copy(sarx_ctx* c, void* dst, const void* src, size_t bytes, bool to_device, bool narrow, bool ordered, bool lane_only) {
    const CopyOps& o = g_ops;
    hipError_t e = hipSuccess;
    if (ordered && lane_only) e = o.stream_sync(c->stream);
    else if (ordered)
        for (int k = 0; k < sarx_ctx::LANES && e == hipSuccess; ++k)
            if (c->lane[k]) e = o.stream_sync(c->lane[k]);
    if (e != hipSuccess) return e;
    hipStream_t direct = c->stream;
    if (!ordered) {
        if (!c->up_stream && (e = o.stream_create(&c->up_stream, hipStreamNonBlocking)) != hipSuccess) return e;
        direct = c->up_stream;
    }
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    // a buffer from sarx_host_alloc (page-locked, already faulted in) needs no staging: one DMA at the PCIe rate, no host memcpy,
    // no first touch
    if (!narrow && (bytes < 4 * sarx_ctx::COPY_CHUNK || o.page_locked(to_device ? src : dst))) {
        e = o.memcpy_async(dst, src, bytes, kind, direct);
        return e != hipSuccess ? e : o.stream_sync(direct);
    }
    constexpr int T = sarx_ctx::COPY_THREADS;
    constexpr size_t CH = sarx_ctx::COPY_CHUNK;
    std::lock_guard<std::mutex> lock(c->copy_mu);      // ctypes callers release the GIL: two host threads may arrive on one ctx
    if (!c->pin[0] && (e = o.host_alloc((void**)&c->pin[0], CH, hipHostMallocDefault)) != hipSuccess) return e;
    if (!c->copy_stream[0] && (e = o.stream_create(&c->copy_stream[0], hipStreamNonBlocking)) != hipSuccess) return e;
    if (narrow && bytes <= CH) {      // a small complex128 upload: rounded on the calling thread through one chunk, no thread is started
        const double* in = (const double*)src;
        float* out = (float*)c->pin[0];
        for (size_t k = 0; k < bytes / sizeof(float); ++k) out[k] = (float)in[k];
        e = o.memcpy_async(dst, c->pin[0], bytes, hipMemcpyHostToDevice, c->copy_stream[0]);
        return e != hipSuccess ? e : o.stream_sync(c->copy_stream[0]);
    }
    for (int i = 1; i < T; ++i) {
        if (!c->pin[i] && (e = o.host_alloc((void**)&c->pin[i], CH, hipHostMallocDefault)) != hipSuccess) return e;
        if (!c->copy_stream[i] && (e = o.stream_create(&c->copy_stream[i], hipStreamNonBlocking)) != hipSuccess) return e;
    }
    for (int i = 0; i < T; ++i)
        if (!c->pin_free[i] && (e = o.event_create(&c->pin_free[i], hipEventDisableTiming)) != hipSuccess) return e;
    const int US = to_device ? c->up_streams : T;       // uploads: thread i's DMAs go to copy stream i % US
    hipError_t errs[T];
    for (int i = 0; i < T; ++i) errs[i] = hipSuccess;
    std::thread th[T];                 // fixed storage: nothing here allocates, so nothing but thread creation can throw
    // thread i copies chunks i, i + T, ...; if a thread cannot be started (std::system_error must not cross the C ABI) the
    // calling thread does that share itself after the others
    auto share = [=, &errs](int i) {
            hipError_t r = o.set_device(c->device);
            char* d = (char*)dst;
            const char* s0 = (const char*)src;
            for (size_t off = (size_t)i * CH; r == hipSuccess && off < bytes; off += (size_t)T * CH) {
                const size_t len = bytes - off < CH ? bytes - off : CH;
                if (to_device) {
                    if (off >= (size_t)T * CH) r = o.event_sync(c->pin_free[i]);     // the chunk's previous DMA has left the pinned buffer
                    if (r != hipSuccess) break;
                    if (narrow) {
                        const double* in = (const double*)s0 + off / sizeof(float);      // off counts complex64 bytes: 2 floats <-> 2 doubles
                        float* out = (float*)c->pin[i];
                        for (size_t k = 0; k < len / sizeof(float); ++k) out[k] = (float)in[k];
                    } else {
                        memcpy(c->pin[i], s0 + off, len);
                    }
                    r = o.memcpy_async(d + off, c->pin[i], len, hipMemcpyHostToDevice, c->copy_stream[i % US]);
                    if (r == hipSuccess) r = o.event_record(c->pin_free[i], c->copy_stream[i % US]);
                } else {
                    r = o.memcpy_async(c->pin[i], s0 + off, len, hipMemcpyDeviceToHost, c->copy_stream[i]);
                    if (r == hipSuccess) r = o.stream_sync(c->copy_stream[i]);
                    if (r == hipSuccess) memcpy(d + off, c->pin[i], len);
                }
            }
            if (r == hipSuccess) r = to_device ? o.event_sync(c->pin_free[i]) : o.stream_sync(c->copy_stream[i]);
            errs[i] = r;
        };
    bool inline_share[T] = {};
    for (int i = 0; i < T; ++i) {
        try {
            if (!o.may_start_thread(i)) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            th[i] = std::thread(share, i);
        } catch (...) { inline_share[i] = true; }        // std::system_error / std::bad_alloc: no exception crosses the C ABI
    }
    for (int i = 0; i < T; ++i) if (inline_share[i]) share(i);
    for (int i = 0; i < T; ++i) if (th[i].joinable()) th[i].join();     // every started thread is joined on the one exit path
    for (int i = 0; i < T; ++i)
        if (errs[i] != hipSuccess) return errs[i];
    return hipSuccess;
}

bool is_page_locked(const void* p) { return g_ops.page_locked(p); }

}  // namespace sarx

extern "C" {

int sarx_version(void) { return SARX_VERSION; }

const char* sarx_last_error(const sarx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_init_error.c_str(); }

int sarx_device_count(int* out_count) {
    if (!out_count) return fail(nullptr, SARX_ERR_INVALID, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out_count = 0; return fail(nullptr, SARX_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *out_count = n;
    return SARX_OK;
}

static int sarx_init_impl(int device_id, sarx_ctx** out_ctx) {
    if (!out_ctx) return fail(nullptr, SARX_ERR_INVALID, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SARX_ERR_DEVICE, "no HIP device available (%s); libsarx has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_id < 0 || device_id >= n) return fail(nullptr, SARX_ERR_INVALID, "device_id %d out of range [0,%d)", device_id, n);
    HIPCHK(nullptr, hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, SARX_ERR_UNSUPPORTED, "device %d is %s; libsarx is built for gfx950 only", device_id, prop.gcnArchName);
    sarx_ctx* c = new sarx_ctx();
    c->device = device_id;
    if (prop.multiProcessorCount > 0) c->cus = prop.multiProcessorCount;
    if (const char* e2 = getenv("SARX_RANGE_IMPL")) c->range_impl = (e2[0] == 'v') ? atoi(e2 + 1) : atoi(e2);
    if (const char* e2 = getenv("SARX_RANGE_CUS")) c->range_cus = atoi(e2);
    if (const char* e2 = getenv("SARX_UP_STREAMS")) { const int v = atoi(e2); if (v >= 1 && v <= sarx_ctx::COPY_THREADS) c->up_streams = v; }
    HIPCHK(nullptr, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->lane[0] = c->stream;
    HIPCHK(nullptr, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    for (int i = 0; i < N_EVENTS; ++i) HIPCHK(nullptr, hipEventCreate(&c->ev[i]));
    HIPCHK(nullptr, hipEventCreateWithFlags(&c->comm_fence, hipEventDisableTiming));
    HIPCHK(nullptr, hipEventCreateWithFlags(&c->comm_done, hipEventDisableTiming));
    for (int i = 0; i < 4; ++i) HIPCHK(nullptr, hipEventCreateWithFlags(&c->comm_mark[i], hipEventDisableTiming));
    // twiddle tables for every power of two up to TW_MAX, fp64-evaluated
    std::vector<float2> tw(2 * TW_MAX);
    tw[0] = tw[1] = make_float2(1.f, 0.f);
    for (int n2 = 2; n2 <= TW_MAX; n2 <<= 1)
        for (int m = 0; m < n2; ++m) {
            const double ang = -2.0 * M_PI * (double)m / (double)n2;
            tw[n2 + m] = make_float2((float)cos(ang), (float)sin(ang));
        }
    HIPCHK(nullptr, hipMalloc(&c->tw_all, tw.size() * sizeof(float2)));
    HIPCHK(nullptr, hipMemcpy(c->tw_all, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMalloc(&c->ati_part_max_all, sarx_ctx::LANES * 4096 * sizeof(float)));
    HIPCHK(nullptr, hipMalloc(&c->ati_part_sum_all, sarx_ctx::LANES * 4096 * sizeof(double2)));
    HIPCHK(nullptr, hipMalloc(&c->ati_out3_all, sarx_ctx::LANES * 4 * sizeof(double)));
    HIPCHK(nullptr, hipMalloc(&c->power_part_all, sarx_ctx::LANES * sarx_ctx::POWER_STRIDE * sizeof(double)));
    *out_ctx = c;
    return SARX_OK;
}
int sarx_init(int device_id, sarx_ctx** out_ctx) {
    return guarded(nullptr, [&] { return sarx_init_impl(device_id, out_ctx); });
}

int sarx_destroy(sarx_ctx* c) {
    if (!c) return SARX_OK;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    comm_release(c);
    for (auto& kind : c->scratch)
        for (LaneScratch& s : kind) hipFree(s.p);
    hipFree(c->tw_all); hipFree(c->ati_part_max_all); hipFree(c->ati_part_sum_all); hipFree(c->ati_out3_all); hipFree(c->power_part_all);
    for (int i = 0; i < N_EVENTS; ++i) hipEventDestroy(c->ev[i]);
    hipEventDestroy(c->comm_fence);
    hipEventDestroy(c->comm_done);
    for (int i = 0; i < 4; ++i) hipEventDestroy(c->comm_mark[i]);
    for (int i = 0; i < sarx_ctx::COPY_THREADS; ++i) {
        if (c->pin[i]) hipHostFree(c->pin[i]);
        if (c->copy_stream[i]) hipStreamDestroy(c->copy_stream[i]);
        if (c->pin_free[i]) hipEventDestroy(c->pin_free[i]);
    }
    for (int i = 0; i < sarx_ctx::DL_SLOTS; ++i) {
        if (c->dl_ready[i]) hipEventDestroy(c->dl_ready[i]);
        if (c->dl_done[i]) hipEventDestroy(c->dl_done[i]);
    }
    if (c->dl_stream) hipStreamDestroy(c->dl_stream);
    if (c->up_stream) hipStreamDestroy(c->up_stream);
    for (int k = 0; k < sarx_ctx::LANES; ++k) {
        if (c->lane_ev[k]) hipEventDestroy(c->lane_ev[k]);
        if (k > 0 && c->lane[k]) hipStreamDestroy(c->lane[k]);
    }
    hipStreamDestroy(c->lane[0]);
    hipStreamDestroy(c->comm_stream);
    delete c;
    return SARX_OK;
}

int sarx_persistent_grid(int wgs_per_cu, int cus, int work_items) { return persistent_grid(wgs_per_cu, cus, work_items); }

int sarx_device_info(sarx_ctx* c, char* name, size_t name_len, int* cus, uint64_t* hbm, char* arch, size_t arch_len) {
    if (!c) return fail(nullptr, SARX_ERR_INVALID, "ctx is NULL");
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    if (name && name_len) snprintf(name, name_len, "%s", prop.name);
    if (arch && arch_len) snprintf(arch, arch_len, "%s", prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm) *hbm = (uint64_t)prop.totalGlobalMem;
    return SARX_OK;
}

// ---- memory / timing ----------------------------------------------------------

int sarx_malloc(sarx_ctx* c, size_t bytes, void** out) {
    NEED_CTX(c);
    if (!out) return fail(c, SARX_ERR_INVALID, "out_dptr is NULL");
    *out = nullptr;
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return SARX_OK;
}
int sarx_free(sarx_ctx* c, void* p) { NEED_CTX(c); HIPCHK(c, hipFree(p)); return SARX_OK; }
int sarx_host_alloc(sarx_ctx* c, size_t bytes, void** out) {
    NEED_CTX(c);
    if (!out) return fail(c, SARX_ERR_INVALID, "out_hptr is NULL");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(c, SARX_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return SARX_OK;
}
int sarx_host_free(sarx_ctx* c, void* p) { NEED_CTX(c); if (p) HIPCHK(c, hipHostFree(p)); return SARX_OK; }
int sarx_memcpy_h2d(sarx_ctx* c, void* d, const void* s, size_t n) {
    NEED_CTX(c);
    HIPCHK(c, staged_copy(c, d, s, n, true));
    return SARX_OK;
}
int sarx_memcpy_d2h(sarx_ctx* c, void* d, const void* s, size_t n) {
    NEED_CTX(c);
    HIPCHK(c, staged_copy(c, d, s, n, false));
    return SARX_OK;
}
int sarx_memcpy_d2d(sarx_ctx* c, void* d, const void* s, size_t n) {
    NEED_CTX(c);
    HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, c->stream));
    return SARX_OK;
}
int sarx_memcpy_h2d_lane(sarx_ctx* c, void* d, const void* s, size_t n) {
    NEED_CTX(c);
    if (!d || !s) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    HIPCHK(c, staged_copy(c, d, s, n, true, false, /*ordered=*/true, /*lane_only=*/true));
    return SARX_OK;
}
int sarx_memcpy_h2d_unordered(sarx_ctx* c, void* d, const void* s, size_t n) {
    NEED_CTX(c);
    if (!d || !s) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    HIPCHK(c, staged_copy(c, d, s, n, true, false, /*ordered=*/false));
    return SARX_OK;
}
int sarx_memcpy_d2h_begin(sarx_ctx* c, void* h, const void* d, size_t n, int* out_slot) {
    NEED_CTX(c);
    if (!h || !d || !out_slot) return fail(c, SARX_ERR_INVALID, "NULL pointer");
    *out_slot = -1;
    if (!is_page_locked(h))
        return fail(c, SARX_ERR_INVALID, "sarx_memcpy_d2h_begin needs a page-locked destination (sarx_host_alloc): a pageable one cannot be "
                                         "written by an asynchronous DMA (use sarx_memcpy_d2h)");
    int slot = -1;
    for (int i = 0; i < sarx_ctx::DL_SLOTS; ++i) if (!c->dl_busy[i]) { slot = i; break; }
    if (slot < 0) return fail(c, SARX_ERR_INVALID, "all %d download slots are in flight: call sarx_memcpy_d2h_end first", sarx_ctx::DL_SLOTS);
    if (!c->dl_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->dl_stream, hipStreamNonBlocking));
    if (!c->dl_ready[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->dl_ready[slot], hipEventDisableTiming));
    if (!c->dl_done[slot]) HIPCHK(c, hipEventCreateWithFlags(&c->dl_done[slot], hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->dl_ready[slot], c->stream));              // everything enqueued on the current lane so far
    HIPCHK(c, hipStreamWaitEvent(c->dl_stream, c->dl_ready[slot], 0));
    {   // in pieces (SARX_DL_CHUNK_MIB, A/B): does one 2 GiB download hold up the upload's 32 MiB DMAs more than many small ones?
        // beside a staged upload 2 GiB as one DMA took 65.9 ms for both, in 32 MiB pieces 62.9, in 256 MiB pieces 59.0 (profiles/r05_i_duplex.log)
        static const size_t piece = [] { const char* e = getenv("SARX_DL_CHUNK_MIB"); return (size_t)(e ? atoi(e) : 256) << 20; }();
        const size_t step = piece ? piece : n;
        for (size_t off = 0; off < n; off += step)
            HIPCHK(c, hipMemcpyAsync((char*)h + off, (const char*)d + off, n - off < step ? n - off : step, hipMemcpyDeviceToHost, c->dl_stream));
    }
    HIPCHK(c, hipEventRecord(c->dl_done[slot], c->dl_stream));
    c->dl_busy[slot] = true;
    *out_slot = slot;
    return SARX_OK;
}
int sarx_memcpy_d2h_end(sarx_ctx* c, int slot) {
    NEED_CTX(c);
    if (slot < 0 || slot >= sarx_ctx::DL_SLOTS || !c->dl_busy[slot]) return fail(c, SARX_ERR_INVALID, "download slot %d is not in flight", slot);
    c->dl_busy[slot] = false;                                            // released whatever the wait returns
    HIPCHK(c, hipEventSynchronize(c->dl_done[slot]));
    return SARX_OK;
}
int sarx_memcpy2d_d2h(sarx_ctx* c, void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height) {
    NEED_CTX(c);
    if (!d || !s || width > dpitch || width > spitch) return fail(c, SARX_ERR_INVALID, "bad 2-D copy arguments");
    if (!width || !height) return SARX_OK;
    HIPCHK(c, sync_all_lanes(c));
    HIPCHK(c, hipMemcpy2DAsync(d, dpitch, s, spitch, width, height, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SARX_OK;
}
int sarx_memcpy2d_h2d(sarx_ctx* c, void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height) {
    NEED_CTX(c);
    if (!d || !s || width > dpitch || width > spitch) return fail(c, SARX_ERR_INVALID, "bad 2-D copy arguments");
    if (!width || !height) return SARX_OK;
    HIPCHK(c, sync_all_lanes(c));
    HIPCHK(c, hipMemcpy2DAsync(d, dpitch, s, spitch, width, height, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SARX_OK;
}
int sarx_memset(sarx_ctx* c, void* d, int v, size_t n) { NEED_CTX(c); HIPCHK(c, hipMemsetAsync(d, v, n, c->stream)); return SARX_OK; }
int sarx_select_lane(sarx_ctx* c, int lane) {
    NEED_CTX(c);
    if (lane < 0 || lane >= sarx_ctx::LANES) return fail(c, SARX_ERR_INVALID, "lane %d out of range [0,%d)", lane, sarx_ctx::LANES);
    if (!c->lane[lane]) HIPCHK(c, hipStreamCreateWithFlags(&c->lane[lane], hipStreamNonBlocking));
    c->cur_lane = lane;
    c->stream = c->lane[lane];
    return SARX_OK;
}
// How concurrently do two lanes run?  Two small launches (64 one-wave workgroups spinning ~`us` microseconds each) on lanes a and b,
// timed from the host: *ratio = time of both together / time of one alone - 1.0 when the lanes' hardware queues run side by side,
// 2.0 when they take turns.
int sarx_probe_lanes(sarx_ctx* c, int a, int b, int us, double* ratio) {
    NEED_CTX(c);
    if (a < 0 || b < 0 || a >= sarx_ctx::LANES || b >= sarx_ctx::LANES || a == b || !ratio || us <= 0)
        return fail(c, SARX_ERR_INVALID, "bad lane probe arguments");
    for (int l : {a, b})
        if (!c->lane[l]) HIPCHK(c, hipStreamCreateWithFlags(&c->lane[l], hipStreamNonBlocking));
    unsigned* sink = reinterpret_cast<unsigned*>(c->power_part_all);          // never written (the kernel's condition is never true)
    const unsigned long long cycles = (unsigned long long)us * 100ull;         // s_memrealtime counts at 100 MHz
    auto wall = [&](bool both, double& ms) -> hipError_t {
        hipError_t e = sync_all_lanes(c);
        if (e != hipSuccess) return e;
        const auto t0 = std::chrono::steady_clock::now();
        e = launch_spin(64, cycles, sink, c->lane[a]);
        if (e == hipSuccess && both) e = launch_spin(64, cycles, sink, c->lane[b]);
        if (e == hipSuccess) e = hipStreamSynchronize(c->lane[a]);
        if (e == hipSuccess && both) e = hipStreamSynchronize(c->lane[b]);
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return e;
    };
    double one = 1e30, two = 1e30, ms = 0;
    for (int rep = 0; rep < 4; ++rep) {
        HIPCHK(c, wall(false, ms)); if (ms < one) one = ms;
        HIPCHK(c, wall(true, ms)); if (ms < two) two = ms;
    }
    *ratio = two / one;
    return SARX_OK;
}
int sarx_set_range_cus(sarx_ctx* c, int cus) {
    NEED_CTX(c);
    if (cus < 0) return fail(c, SARX_ERR_INVALID, "cus must be >= 0 (0 = all)");
    c->range_cus = cus;
    return SARX_OK;
}
int sarx_lanes_join(sarx_ctx* c) {
    NEED_CTX(c);
    for (int k = 0; k < sarx_ctx::LANES; ++k) {
        if (!c->lane[k]) continue;
        if (!c->lane_ev[k]) HIPCHK(c, hipEventCreateWithFlags(&c->lane_ev[k], hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->lane_ev[k], c->lane[k]));
    }
    for (int k = 0; k < sarx_ctx::LANES; ++k)
        for (int j = 0; j < sarx_ctx::LANES; ++j)
            if (j != k && c->lane[k] && c->lane[j]) HIPCHK(c, hipStreamWaitEvent(c->lane[k], c->lane_ev[j], 0));
    return SARX_OK;
}
int sarx_sync(sarx_ctx* c) {
    NEED_CTX(c);
    HIPCHK(c, sync_all_lanes(c));
    HIPCHK(c, hipStreamSynchronize(c->comm_stream));
    if (c->dl_stream) HIPCHK(c, hipStreamSynchronize(c->dl_stream));
    return SARX_OK;
}
int sarx_event_record(sarx_ctx* c, int slot) {
    NEED_CTX(c);
    if (slot < 0 || slot >= N_EVENTS) return fail(c, SARX_ERR_INVALID, "event slot %d out of range", slot);
    HIPCHK(c, hipEventRecord(c->ev[slot], c->stream));
    c->ev_set[slot] = true;
    return SARX_OK;
}
int sarx_event_elapsed_ms(sarx_ctx* c, int a, int b, float* ms) {
    NEED_CTX(c);
    if (a < 0 || a >= N_EVENTS || b < 0 || b >= N_EVENTS || !ms) return fail(c, SARX_ERR_INVALID, "bad event slots");
    if (!c->ev_set[a] || !c->ev_set[b]) return fail(c, SARX_ERR_INVALID, "event slot not recorded");
    HIPCHK(c, hipEventSynchronize(c->ev[b]));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev[a], c->ev[b]));
    return SARX_OK;
}

#ifdef SARX_TESTING
// ---- sanitizer-build hook (make asan; never part of libsarx.so) -----------------------------------------------------------------
// staged_copy on a stand-in context with host stand-ins for the runtime: "device" memory is host memory, a DMA is a memcpy, streams
// and events are opaque tokens.  no_thread_mask: bit i = share i's thread "cannot be started" (the inline-share path);
// fail_at >= 0: the fail_at-th copy call returns an error (every thread must still be joined, the error returned);
// page_locked != 0: the host side counts as page-locked (the one-DMA path).  Returns staged_copy's hipError_t as an int.
static std::atomic<int> t_copy_calls{0};
static int t_fail_at = -1;
static unsigned t_no_thread = 0;
static int t_locked = 0;
static std::atomic<int> t_tokens{0};
int sarx_test_staged_copy(void* dst, const void* src, size_t bytes, int to_device, int narrow, int ordered, unsigned no_thread_mask,
                          int fail_at, int page_locked, int up_streams, int* threads_inline) {
    CopyOps saved = g_ops;
    t_copy_calls = 0; t_fail_at = fail_at; t_no_thread = no_thread_mask; t_locked = page_locked;
    g_ops.memcpy_async = [](void* d, const void* s2, size_t n, hipMemcpyKind, hipStream_t st) {
        if (!st) return hipErrorInvalidHandle;
        if (t_copy_calls.fetch_add(1) == t_fail_at) return hipErrorUnknown;
        memcpy(d, s2, n);
        return hipSuccess;
    };
    g_ops.stream_sync = [](hipStream_t st) { return st ? hipSuccess : hipErrorInvalidHandle; };
    g_ops.stream_create = [](hipStream_t* st, unsigned) { *st = (hipStream_t)(uintptr_t)(0x1000 + 16 * t_tokens.fetch_add(1)); return hipSuccess; };
    g_ops.event_create = [](hipEvent_t* ev, unsigned) { *ev = (hipEvent_t)(uintptr_t)(0x100000 + 16 * t_tokens.fetch_add(1)); return hipSuccess; };
    g_ops.event_record = [](hipEvent_t ev, hipStream_t st) { return (ev && st) ? hipSuccess : hipErrorInvalidHandle; };
    g_ops.event_sync = [](hipEvent_t ev) { return ev ? hipSuccess : hipErrorInvalidHandle; };
    g_ops.host_alloc = [](void** p2, size_t n, unsigned) { *p2 = malloc(n); return *p2 ? hipSuccess : hipErrorOutOfMemory; };
    g_ops.set_device = [](int) { return hipSuccess; };
    g_ops.page_locked = [](const void*) { return t_locked != 0; };
    g_ops.may_start_thread = [](int i) { return !((t_no_thread >> i) & 1u); };
    int rc;
    {
        sarx_ctx c;
        c.device = 0;
        c.stream = (hipStream_t)(uintptr_t)0x10;
        c.lane[0] = c.stream;
        if (up_streams >= 1 && up_streams <= sarx_ctx::COPY_THREADS) c.up_streams = up_streams;
        rc = (int)staged_copy(&c, dst, src, bytes, to_device != 0, narrow != 0, ordered != 0);
        if (threads_inline) { int k = 0; for (int i = 0; i < sarx_ctx::COPY_THREADS; ++i) k += (no_thread_mask >> i) & 1u; *threads_inline = k; }
        for (int i = 0; i < sarx_ctx::COPY_THREADS; ++i) free(c.pin[i]);
    }
    g_ops = saved;
    return rc;
}
size_t sarx_test_copy_chunk(void) { return sarx_ctx::COPY_CHUNK; }
int sarx_test_copy_threads(void) { return sarx_ctx::COPY_THREADS; }
int sarx_test_guard(int what) {      // the exception guard of the allocating entry points: 0 ok, 1 bad_alloc, 2 any other exception
    return guarded(nullptr, [&]() -> int {
        if (what == 1) throw std::bad_alloc();
        if (what == 2) throw std::runtime_error("x");
        return SARX_OK;
    });
}
#endif

}  // extern "C"
