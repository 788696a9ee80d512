// rt_rccl_stub.cpp — a stand-in for librccl, for tests only: the seven entry
// points rt_rccl.cpp loads, with ncclGather done by ordinary stream copies, so
// that the library's multi-rank RCCL path (rank-major staging, assemble
// offsets, the ranks' streams) runs on a machine with one GPU.  Loaded through
// RT_RCCL_LIB; rt_rccl_stub_marker tells the library that this is not RCCL,
// and only then does rt_render_gather_async take a device list that names one
// device several times.
//
// ncclGather calls between ncclGroupStart and ncclGroupEnd are recorded.  At
// ncclGroupEnd the k-th call of every rank forms collective k: the root's
// stream records "receive buffer ready", every other rank's stream waits for
// that (no rank's data lands before the root's stream reaches the call, as
// with the real one), copies its block to recvbuff + rank * count * size with
// hipMemcpyAsync and records an event that the root's stream waits for; the
// root copies its own block on its own stream.  Nothing else is issued: no
// kernel, no host synchronisation.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <vector>

struct ncclComm {
    int rank, nranks, device;
};

namespace {

struct Call {
    ncclComm_t comm;
    const void* send;
    void* recv;
    size_t count;
    ncclDataType_t type;
    int root;
    hipStream_t stream;
};

thread_local int t_depth = 0;
thread_local std::vector<Call> t_calls;

size_t type_size(ncclDataType_t t) { return t == ncclFloat64 ? 8 : t == ncclUint32 ? 4 : 0; }

struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int d)
    {
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(d);
    }
    ~DeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// One collective: `calls` holds exactly one call per rank of the communicator.
ncclResult_t run_gather(const std::vector<Call>& calls)
{
    const Call* root = nullptr;
    for (const Call& c : calls)
        if (c.comm->rank == c.root) root = &c;
    if (!root || !root->recv || (int)calls.size() != root->comm->nranks) return ncclInvalidUsage;
    const size_t bytes = root->count * type_size(root->type);
    for (const Call& c : calls)
        if (c.count != root->count || c.type != root->type || c.root != root->root || !c.send)
            return ncclInvalidArgument;
    hipEvent_t ready = nullptr;
    {
        DeviceScope d(root->comm->device);
        if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess) return ncclUnhandledCudaError;
        if (hipEventRecord(ready, root->stream) != hipSuccess) return ncclUnhandledCudaError;
    }
    ncclResult_t rc = ncclSuccess;
    for (const Call& c : calls) {
        char* dst = (char*)root->recv + (size_t)c.comm->rank * bytes;
        hipError_t e;
        if (&c == root) {
            DeviceScope d(c.comm->device);
            e = hipMemcpyAsync(dst, c.send, bytes, hipMemcpyDeviceToDevice, c.stream);
        } else {
            hipEvent_t sent = nullptr;
            {
                DeviceScope d(c.comm->device);
                e = hipStreamWaitEvent(c.stream, ready, 0);
                if (e == hipSuccess) e = hipMemcpyAsync(dst, c.send, bytes, hipMemcpyDefault, c.stream);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&sent, hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventRecord(sent, c.stream);
            }
            if (e == hipSuccess) {
                DeviceScope d(root->comm->device);
                e = hipStreamWaitEvent(root->stream, sent, 0);
            }
            if (sent) (void)hipEventDestroy(sent);      // released once the recorded work is done
        }
        if (e != hipSuccess) rc = ncclUnhandledCudaError;
    }
    (void)hipEventDestroy(ready);
    return rc;
}

ncclResult_t run_group()
{
    std::vector<Call> calls;
    calls.swap(t_calls);
    // the k-th call of each communicator belongs to collective k
    std::vector<std::vector<Call>> coll;
    std::vector<ncclComm_t> seen;
    std::vector<size_t> next;
    for (const Call& c : calls) {
        size_t i = 0;
        while (i < seen.size() && seen[i] != c.comm) ++i;
        if (i == seen.size()) {
            seen.push_back(c.comm);
            next.push_back(0);
        }
        const size_t k = next[i]++;
        if (k >= coll.size()) coll.resize(k + 1);
        coll[k].push_back(c);
    }
    for (const auto& one : coll) {
        const ncclResult_t rc = run_gather(one);
        if (rc != ncclSuccess) return rc;
    }
    return ncclSuccess;
}

}  // namespace

extern "C" {

int rt_rccl_stub_marker = 1;

ncclResult_t ncclGetVersion(int* version)
{
    if (!version) return ncclInvalidArgument;
    *version = NCCL_VERSION_CODE;
    return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t result)
{
    switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "stub: HIP call failed";
    case ncclInvalidArgument: return "stub: invalid argument";
    case ncclInvalidUsage: return "stub: invalid usage";
    default: return "stub: error";
    }
}

// A repeated device is accepted: the ranks are then streams of one GPU.
ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist)
{
    if (!comm || ndev < 1) return ncclInvalidArgument;
    for (int i = 0; i < ndev; ++i) comm[i] = new ncclComm{i, ndev, devlist ? devlist[i] : i};
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclGroupStart()
{
    ++t_depth;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    if (t_depth < 1) return ncclInvalidUsage;
    return --t_depth == 0 ? run_group() : ncclSuccess;
}

ncclResult_t ncclGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, int root,
                        ncclComm_t comm, hipStream_t stream)
{
    if (!comm || !type_size(datatype) || root < 0 || root >= comm->nranks) return ncclInvalidArgument;
    t_calls.push_back(Call{comm, sendbuff, recvbuff, sendcount, datatype, root, stream});
    return t_depth ? ncclSuccess : run_group();
}

}  // extern "C"
