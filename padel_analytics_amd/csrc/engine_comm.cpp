// RCCL: the one-time weight broadcast and the sharded runner's gather.  The only file that sees rccl.h and dlfcn.h.
#include "engine_internal.h"
#include <rccl/rccl.h>      // types only: librccl is dlopen'ed on first use

#include <dlfcn.h>

// ------------------------------------------------------------------------------- RCCL (one-time weight broadcast)
// librccl is dlopen'ed on first use: a process that already holds torch's bundled librccl.so.1 gets that one
// (same SONAME), a standalone process the ROCm one; single-GPU users never load it.

struct pa_comm {
    void* lib = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

static void* rccl_lib() {
    static void* lib = nullptr;
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    return lib;
}

int pa_comm_unique_id(void* out, size_t cap) {
    if (!out || cap < NCCL_UNIQUE_ID_BYTES) PA_FAIL((pa_engine*)nullptr, "pa_comm_unique_id: need %d bytes", NCCL_UNIQUE_ID_BYTES);
    void* lib = rccl_lib();
    if (!lib) PA_FAIL((pa_engine*)nullptr, "librccl.so.1 not found: %s", dlerror());
    auto get = (ncclResult_t (*)(ncclUniqueId*))dlsym(lib, "ncclGetUniqueId");
    if (!get) PA_FAIL((pa_engine*)nullptr, "ncclGetUniqueId missing");
    ncclUniqueId id;
    const ncclResult_t r = get(&id);
    if (r != ncclSuccess) PA_FAIL((pa_engine*)nullptr, "ncclGetUniqueId failed (%d)", (int)r);
    memcpy(out, &id, NCCL_UNIQUE_ID_BYTES);
    return 0;
}

int pa_engine_comm_init(pa_engine* e, const void* unique_id, size_t id_bytes, int nranks, int rank) {
    if (!e || !unique_id || id_bytes < NCCL_UNIQUE_ID_BYTES || nranks < 1 || rank < 0 || rank >= nranks)
        PA_FAIL(e, "pa_engine_comm_init: bad arguments");
    if (e->comm) PA_FAIL(e, "pa_engine_comm_init: communicator already initialised");
    void* lib = rccl_lib();
    if (!lib) PA_FAIL(e, "librccl.so.1 not found: %s", dlerror());
    pa_comm* c = new pa_comm();
    c->lib = lib; c->nranks = nranks; c->rank = rank;
    c->CommInitRank = (decltype(c->CommInitRank))dlsym(lib, "ncclCommInitRank");
    c->CommDestroy = (decltype(c->CommDestroy))dlsym(lib, "ncclCommDestroy");
    c->Broadcast = (decltype(c->Broadcast))dlsym(lib, "ncclBroadcast");
    c->AllReduce = (decltype(c->AllReduce))dlsym(lib, "ncclAllReduce");
    c->GetErrorString = (decltype(c->GetErrorString))dlsym(lib, "ncclGetErrorString");
    c->AllGather = (decltype(c->AllGather))dlsym(lib, "ncclAllGather");
    c->Send = (decltype(c->Send))dlsym(lib, "ncclSend");
    c->Recv = (decltype(c->Recv))dlsym(lib, "ncclRecv");
    c->GroupStart = (decltype(c->GroupStart))dlsym(lib, "ncclGroupStart");
    c->GroupEnd = (decltype(c->GroupEnd))dlsym(lib, "ncclGroupEnd");
    if (!c->CommInitRank || !c->CommDestroy || !c->Broadcast || !c->AllReduce || !c->GetErrorString || !c->AllGather || !c->Send || !c->Recv ||
        !c->GroupStart || !c->GroupEnd) {
        delete c;
        PA_FAIL(e, "librccl: missing symbols");
    }
    PA_HIP(e, hipSetDevice(e->dev));
    ncclUniqueId id;
    memcpy(&id, unique_id, NCCL_UNIQUE_ID_BYTES);
    const ncclResult_t r = c->CommInitRank(&c->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        const char* msg = c->GetErrorString(r);
        delete c;
        PA_FAIL(e, "ncclCommInitRank(%d/%d): %s", rank, nranks, msg);
    }
    e->comm = c;
    return 0;
}

void pa_engine_comm_destroy(pa_engine* e) {
    if (!e || !e->comm) return;
    hipSetDevice(e->dev);
    hipStreamSynchronize(e->main_stream_wait_only());
    if (e->comm->comm) e->comm->CommDestroy(e->comm->comm);
    delete e->comm;
    e->comm = nullptr;
}

// in-place broadcast of device memory from `root` over the engine's communicator (xGMI inside a node)
int pa_engine_bcast(pa_engine* e, void* dev_ptr, size_t nbytes, int root) {
    if (!e || !dev_ptr) return 1;
    if (!e->comm) PA_FAIL(e, "pa_engine_bcast: call pa_engine_comm_init first");
    PA_HIP(e, hipSetDevice(e->dev));
    const ncclResult_t r = e->comm->Broadcast(dev_ptr, dev_ptr, nbytes, ncclUint8, root, e->comm->comm, e->main_stream());
    if (r != ncclSuccess) PA_FAIL(e, "ncclBroadcast: %s", e->comm->GetErrorString(r));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

// the one collective of the path: the packed weight blob goes from the rank that loaded the checkpoint to every
// other GPU, HBM to HBM (north_star "one-time RCCL broadcast of weights over xGMI")
int pa_engine_bcast_weights(pa_engine* e, pa_model* m, int root) {
    if (!e || !m || m->e != e) return 1;
    m->wr_valid = false;
    return pa_engine_bcast(e, m->d_w.get(), m->n_w * sizeof(float), root);
}

// The same broadcast with a separate SOURCE on the root: the root rank sends `src`'s blob (the model it loaded), every rank —
// the root included — receives into `dst` (a model created from a NULL blob).  Ranks other than the root pass src = NULL.
// On one GPU (nranks == 1) this is how a test proves that a blob that only ever travelled through RCCL gives bitwise the
// detections of the loaded one (BASELINE configs[3]: weights reach 7 of the 8 shards this way).
int pa_engine_bcast_weights_from(pa_engine* e, pa_model* src, pa_model* dst, int root) {
    if (!e || !dst || dst->e != e || (src && (src->e != e || src->n_w != dst->n_w))) return 1;
    if (!e->comm) PA_FAIL(e, "pa_engine_bcast_weights_from: call pa_engine_comm_init first");
    PA_HIP(e, hipSetDevice(e->dev));
    dst->wr_valid = false;
    const void* send = src ? src->d_w.get() : dst->d_w.get();
    const ncclResult_t r = e->comm->Broadcast(send, dst->d_w.get(), dst->n_w * sizeof(float), ncclUint8, root, e->comm->comm, e->main_stream());
    if (r != ncclSuccess) PA_FAIL(e, "ncclBroadcast: %s", e->comm->GetErrorString(r));
    PA_HIP(e, hipStreamSynchronize(e->main_stream_wait_only()));
    return 0;
}

// The sharded runner's gather (include/padel_hip.h, ABI v5): variable-length host buffers of every rank to the root, over the
// communicator the library owns.  Lengths by ncclAllGather (pa_engine_gather_sizes), payload by one ncclSend per rank and
// nranks - 1 ncclRecv on the root inside one group (the root's own part is a host copy); device staging buffers live for the call.
int pa_engine_gather_sizes(pa_engine* e, size_t nbytes, uint64_t* sizes) {
    if (!e || !sizes) PA_FAIL(e, "pa_engine_gather_sizes: NULL argument");
    const int nranks = e->comm ? e->comm->nranks : 1;
    if (nranks == 1) { sizes[0] = nbytes; return 0; }
    PA_HIP(e, hipSetDevice(e->dev));
    pa_comm* c = e->comm;
    DevMem<unsigned long long> sizes_dev;          // (the stream is waited for below, before any return)
    PA_HIP(e, sizes_dev.alloc((size_t)(nranks + 1) * sizeof(unsigned long long)));
    unsigned long long* const d_sizes = sizes_dev.get();
    const unsigned long long mine = nbytes;
    hipError_t h = hipMemcpyAsync(d_sizes + nranks, &mine, sizeof(mine), hipMemcpyHostToDevice, e->main_stream());
    ncclResult_t r = ncclSuccess;
    if (h == hipSuccess) r = c->AllGather(d_sizes + nranks, d_sizes, 1, ncclUint64, c->comm, e->main_stream());
    std::vector<unsigned long long> hs((size_t)nranks);
    if (h == hipSuccess && r == ncclSuccess) h = hipMemcpyAsync(hs.data(), d_sizes, (size_t)nranks * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->main_stream());
    if (h == hipSuccess) h = hipStreamSynchronize(e->main_stream_wait_only());
    if (r != ncclSuccess) PA_FAIL(e, "ncclAllGather: %s", c->GetErrorString(r));
    if (h != hipSuccess) PA_FAIL(e, "pa_engine_gather_sizes: %s", hipGetErrorString(h));
    for (int k = 0; k < nranks; ++k) sizes[k] = hs[(size_t)k];
    return 0;
}

int pa_engine_gather(pa_engine* e, const void* send, size_t nbytes, void* recv, size_t recv_cap, const uint64_t* sizes, int root) {
    if (!e || !sizes || (nbytes && !send)) PA_FAIL(e, "pa_engine_gather: NULL argument");
    const int nranks = e->comm ? e->comm->nranks : 1, me = e->comm ? e->comm->rank : 0;
    if (root < 0 || root >= nranks) PA_FAIL(e, "pa_engine_gather: root %d of %d", root, nranks);
    if (sizes[me] != nbytes) PA_FAIL(e, "pa_engine_gather: sizes[%d] = %llu, nbytes = %zu", me, (unsigned long long)sizes[me], nbytes);
    size_t total = 0;
    for (int k = 0; k < nranks; ++k) total += (size_t)sizes[k];
    // the capacity check comes BEFORE the exchange and depends only on what every rank knows: a root that bails out alone would
    // leave the others inside their sends
    if (me == root && (recv_cap < total || (total && !recv))) PA_FAIL(e, "pa_engine_gather: recv capacity %zu < %zu", recv_cap, total);
    if (nranks == 1) {
        if (nbytes) memcpy(recv, send, nbytes);
        return 0;
    }
    PA_HIP(e, hipSetDevice(e->dev));
    pa_comm* c = e->comm;
    DevMem<char> d_send, d_recv;          // (likewise)
    hipError_t h = hipSuccess;
    ncclResult_t r = ncclSuccess;
    if (me != root && nbytes) {
        h = (hipError_t)d_send.alloc(nbytes);
        if (h == hipSuccess) h = hipMemcpyAsync(d_send.get(), send, nbytes, hipMemcpyHostToDevice, e->main_stream());
    }
    if (me == root && total) h = (hipError_t)d_recv.alloc(total);
    // (an allocation failure still enters the group with nothing posted: the peers' sends then fail inside RCCL instead of hanging)
    r = c->GroupStart();
    if (h == hipSuccess && r == ncclSuccess) {
        if (me == root) {
            size_t off = 0;
            for (int k = 0; k < nranks && r == ncclSuccess; ++k) {
                if (k != root && sizes[k]) r = c->Recv(d_recv.get() + off, (size_t)sizes[k], ncclUint8, k, c->comm, e->main_stream());
                off += (size_t)sizes[k];
            }
        } else if (nbytes) {
            r = c->Send(d_send.get(), nbytes, ncclUint8, root, c->comm, e->main_stream());
        }
    }
    const ncclResult_t r2 = c->GroupEnd();
    if (r == ncclSuccess) r = r2;
    if (h == hipSuccess && r == ncclSuccess && me == root) {
        size_t off = 0;
        for (int k = 0; k < nranks && h == hipSuccess; ++k) {
            const size_t nb = (size_t)sizes[k];
            if (k == root) { if (nb) memcpy((char*)recv + off, send, nb); }
            else if (nb) h = hipMemcpyAsync((char*)recv + off, d_recv.get() + off, nb, hipMemcpyDeviceToHost, e->main_stream());
            off += nb;
        }
    }
    if (h == hipSuccess) h = hipStreamSynchronize(e->main_stream_wait_only());
    if (r != ncclSuccess) PA_FAIL(e, "ncclSend/Recv: %s", c->GetErrorString(r));
    if (h != hipSuccess) PA_FAIL(e, "pa_engine_gather: %s", hipGetErrorString(h));
    return 0;
}

// max over ranks of one double (bench: step time) — keeps the measurement inside the same communicator
int pa_engine_allreduce_max(pa_engine* e, double* value) {
    if (!e || !value) return 1;
    if (!e->comm) PA_FAIL(e, "pa_engine_allreduce_max: call pa_engine_comm_init first");
    PA_HIP(e, hipSetDevice(e->dev));
    DevMem<double> d_val;
    PA_HIP(e, d_val.alloc(sizeof(double)));
    double* const d = d_val.get();
    hipError_t h = hipMemcpyAsync(d, value, sizeof(double), hipMemcpyHostToDevice, e->main_stream());
    ncclResult_t r = ncclSuccess;
    if (h == hipSuccess) r = e->comm->AllReduce(d, d, 1, ncclDouble, ncclMax, e->comm->comm, e->main_stream());
    if (h == hipSuccess && r == ncclSuccess) h = hipMemcpyAsync(value, d, sizeof(double), hipMemcpyDeviceToHost, e->main_stream());
    if (h == hipSuccess) h = hipStreamSynchronize(e->main_stream_wait_only());
    if (r != ncclSuccess) PA_FAIL(e, "ncclAllReduce: %s", e->comm->GetErrorString(r));
    if (h != hipSuccess) PA_FAIL(e, "pa_engine_allreduce_max: %s", hipGetErrorString(h));
    return 0;
}
