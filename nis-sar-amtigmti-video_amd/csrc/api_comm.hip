// libsarx C ABI (include/sarx.h), collectives: the RCCL loader and the sarx_comm_* / all-gather / all-reduce entry points.
#include "api_ctx.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace sarx;

struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    std::string path;      // file the symbols came from
    int version = 0;       // ncclGetVersion of that file
};
static RcclApi g_rccl;
// RCCL must be the build that belongs to the HIP runtime this process runs on: a process that imported torch first runs
// on torch's bundled libamdhip64 (soname libamdhip64.so.7, same as /opt/rocm's, so the loader hands it to libsarx too)
// and must take torch's bundled librccl; a plain C / ctypes process runs on /opt/rocm's runtime and takes /opt/rocm's
// librccl.  So: SARX_RCCL_PATH if set, else librccl from the directory of the loaded HIP runtime, else whatever
// librccl.so.1 is already mapped, else the loader's search path.  The six entry points used are ABI-stable across
// RCCL 2.2x; path and version are reported by sarx_rccl_info so a run states what it gathered with.
static bool load_rccl(std::string& err) {
    if (g_rccl.lib) return true;
    void* h = nullptr;
    std::string tried;
    auto attempt = [&](const std::string& name, int extra) {
        if (h || name.empty()) return;
        h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL | extra);
        if (!h) tried += name + "; ";
    };
    if (const char* e = getenv("SARX_RCCL_PATH")) attempt(e, 0);
    Dl_info di;
    if (!h && dladdr((void*)&hipGetDeviceCount, &di) && di.dli_fname) {
        std::string dir(di.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) {
            dir.resize(slash);
            attempt(dir + "/librccl.so.1", 0);
            attempt(dir + "/librccl.so", 0);
        }
    }
    attempt("librccl.so.1", RTLD_NOLOAD);
    attempt("librccl.so.1", 0);
    attempt("librccl.so", 0);
    if (!h) { err = "dlopen librccl failed (tried " + tried + ")"; return false; }
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(h, "ncclAllGather");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(h, "ncclAllReduce");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(h, "ncclGetErrorString");
    g_rccl.GetVersion = (decltype(g_rccl.GetVersion))dlsym(h, "ncclGetVersion");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.AllReduce || !g_rccl.CommDestroy) {
        err = "librccl lacks a required symbol";
        dlclose(h);
        return false;
    }
    if (dladdr((void*)g_rccl.GetUniqueId, &di) && di.dli_fname) g_rccl.path = di.dli_fname;
    if (g_rccl.GetVersion) g_rccl.GetVersion(&g_rccl.version);
    g_rccl.lib = h;
    return true;
}

void sarx::comm_release(sarx_ctx* c) {
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
}

extern "C" {

// ---- RCCL ------------------------------------------------------------------------
int sarx_comm_unique_id(void* id_out) {
    if (!id_out) return fail(nullptr, SARX_ERR_INVALID, "id_out is NULL");
    std::string err;
    if (!load_rccl(err)) return fail(nullptr, SARX_ERR_COMM, "%s", err.c_str());
    static_assert(sizeof(ncclUniqueId) == SARX_COMM_ID_BYTES, "unique id size");
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, SARX_ERR_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    memcpy(id_out, &id, sizeof id);
    return SARX_OK;
}
int sarx_rccl_info(char* path, size_t path_len, int* version, int* header_version) {
    std::string err;
    if (!load_rccl(err)) return fail(nullptr, SARX_ERR_COMM, "%s", err.c_str());
    if (path && path_len) snprintf(path, path_len, "%s", g_rccl.path.c_str());
    if (version) *version = g_rccl.version;
    if (header_version) *header_version = NCCL_VERSION_CODE;
    return SARX_OK;
}
int sarx_comm_init(sarx_ctx* c, const void* id, int n_ranks, int rank) {
    NEED_CTX(c);
    if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, SARX_ERR_INVALID, "bad comm arguments");
    std::string err;
    if (!load_rccl(err)) return fail(c, SARX_ERR_COMM, "%s", err.c_str());
    if (c->comm) return fail(c, SARX_ERR_COMM, "communicator already initialised");
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, n_ranks, uid, rank);
    if (r != ncclSuccess) { c->comm = nullptr; return fail(c, SARX_ERR_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"); }
    c->n_ranks = n_ranks; c->rank = rank;
    return SARX_OK;
}
int sarx_allgather_dev(sarx_ctx* c, const void* send, void* recv, size_t bytes_per_rank) {
    NEED_CTX(c);
    if (!c->comm) return fail(c, SARX_ERR_COMM, "communicator not initialised");
    if (!send || !recv || (bytes_per_rank & 3)) return fail(c, SARX_ERR_INVALID, "bad all-gather arguments");
    HIPCHK(c, hipEventRecord(c->comm_fence, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->comm_fence, 0));
    ncclResult_t r = g_rccl.AllGather(send, recv, bytes_per_rank / 4, ncclFloat32, c->comm, c->comm_stream);
    if (r != ncclSuccess) return fail(c, SARX_ERR_COMM, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    return SARX_OK;
}
int sarx_allreduce_max_dev(sarx_ctx* c, float* d_buf, size_t count) {
    NEED_CTX(c);
    if (!c->comm) return fail(c, SARX_ERR_COMM, "communicator not initialised");
    if (!d_buf || !count) return fail(c, SARX_ERR_INVALID, "bad all-reduce arguments");
    HIPCHK(c, hipEventRecord(c->comm_fence, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->comm_fence, 0));
    ncclResult_t r = g_rccl.AllReduce(d_buf, d_buf, count, ncclFloat32, ncclMax, c->comm, c->comm_stream);
    if (r != ncclSuccess) return fail(c, SARX_ERR_COMM, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    return SARX_OK;
}
int sarx_comm_sync(sarx_ctx* c) { NEED_CTX(c); HIPCHK(c, hipStreamSynchronize(c->comm_stream)); return SARX_OK; }
int sarx_comm_fence_compute(sarx_ctx* c) {
    NEED_CTX(c);
    HIPCHK(c, hipEventRecord(c->comm_done, c->comm_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->comm_done, 0));
    return SARX_OK;
}
int sarx_comm_mark(sarx_ctx* c, int slot) {
    NEED_CTX(c);
    if (slot < 0 || slot >= 4) return fail(c, SARX_ERR_INVALID, "comm mark slot %d out of range [0,4)", slot);
    HIPCHK(c, hipEventRecord(c->comm_mark[slot], c->comm_stream));
    c->comm_mark_set[slot] = true;
    return SARX_OK;
}
int sarx_comm_wait_mark(sarx_ctx* c, int slot) {
    NEED_CTX(c);
    if (slot < 0 || slot >= 4) return fail(c, SARX_ERR_INVALID, "comm mark slot %d out of range [0,4)", slot);
    if (c->comm_mark_set[slot]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->comm_mark[slot], 0));
    return SARX_OK;
}
int sarx_comm_destroy(sarx_ctx* c) {
    NEED_CTX(c);
    if (c->comm) { hipStreamSynchronize(c->comm_stream); g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    return SARX_OK;
}

}  // extern "C"
