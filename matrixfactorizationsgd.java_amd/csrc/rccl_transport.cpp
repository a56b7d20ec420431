// rccl_transport.cpp -- the DSGD ring's transport in the product (transport.hpp): one point-to-point message per block
// and sub-epoch over xGMI (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the communication stream), RMSE as
// one 2-double all-reduce.  RCCL is bound at run time (dlopen of librccl.so.1 on first use): single-GPU hosts never
// load it, and a process that already holds a copy (PyTorch bundles one) shares it by SONAME.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <mutex>

#include "transport.hpp"

namespace {

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};

Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {std::getenv("MFSGD_RCCL_LIBRARY"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            if (!n || !*n) continue;
            r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (r.lib) break;
            r.why = dlerror();
        }
        if (!r.lib) return;
        auto sym = [&](const char* s) {
            void* p = dlsym(r.lib, s);
            if (!p) r.why = std::string("librccl lacks ") + s;
            return p;
        };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
        if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.Send || !r.Recv ||
            !r.AllReduce || !r.GetErrorString) {
            dlclose(r.lib);
            r.lib = nullptr;
        }
    });
    return r;
}

#define TRANSPORT_NCCL(err, call)                                                                                      \
    do {                                                                                                               \
        ncclResult_t r_ = (call);                                                                                      \
        if (r_ != ncclSuccess) return mfsgd::transport_fail((err), MFSGD_ERR_HIP, std::string(#call) + ": " + rccl().GetErrorString(r_)); \
    } while (0)

struct RcclTransport final : mfsgd::Transport {
    ncclComm_t comm = nullptr;
    int to = 0, from = 0;  // rank - 1, rank + 1
    size_t count = 0;
    hipStream_t wire = nullptr;
    double* red = nullptr;

    ~RcclTransport() override {
        if (comm) (void)rccl().CommDestroy(comm);
    }

    int bring_up(const void* id, int rank, int world, int, size_t count_, hipStream_t wire_, double* red_, std::string& err) override {
        to = (rank + world - 1) % world;
        from = (rank + 1) % world;
        count = count_;
        wire = wire_;
        red = red_;
        ncclUniqueId uid;
        std::memcpy(&uid, id, sizeof uid);
        ncclResult_t r = rccl().CommInitRank(&comm, world, uid, rank);
        if (r == ncclSuccess) return MFSGD_OK;
        comm = nullptr;
        return mfsgd::transport_fail(err, MFSGD_ERR_HIP, std::string("dsgd_create: ncclCommInitRank: ") + rccl().GetErrorString(r));
    }

    int shift(int, const float* send, float* recv, hipEvent_t trained, hipEvent_t arrived, std::string& err) override {
        Rccl& R = rccl();
        TRANSPORT_HIP(err, hipStreamWaitEvent(wire, trained, 0));
        TRANSPORT_NCCL(err, R.GroupStart());
        TRANSPORT_NCCL(err, R.Send(send, count, ncclFloat, to, comm, wire));
        TRANSPORT_NCCL(err, R.Recv(recv, count, ncclFloat, from, comm, wire));
        TRANSPORT_NCCL(err, R.GroupEnd());
        TRANSPORT_HIP(err, hipEventRecord(arrived, wire));
        bytes_sent += (int64_t)(count * sizeof(float));
        return MFSGD_OK;
    }

    int allreduce2(double* v, bool max, std::string& err) override {
        TRANSPORT_HIP(err, hipMemcpyAsync(red, v, 2 * sizeof(double), hipMemcpyHostToDevice, wire));
        TRANSPORT_NCCL(err, rccl().AllReduce(red, red, 2, ncclDouble, max ? ncclMax : ncclSum, comm, wire));
        TRANSPORT_HIP(err, hipMemcpyAsync(v, red, 2 * sizeof(double), hipMemcpyDeviceToHost, wire));
        TRANSPORT_HIP(err, hipStreamSynchronize(wire));
        return MFSGD_OK;
    }
};

}  // namespace

namespace mfsgd {

int rccl_unique_id(void* id_out, std::string& err) {
    static_assert(sizeof(ncclUniqueId) <= MFSGD_DSGD_ID_BYTES, "id buffer");
    Rccl& R = rccl();
    if (!R.lib) return mfsgd::transport_fail(err, MFSGD_ERR_UNSUPPORTED, "RCCL is not available: " + R.why);
    ncclUniqueId id;
    ncclResult_t r = R.GetUniqueId(&id);
    if (r != ncclSuccess) return mfsgd::transport_fail(err, MFSGD_ERR_HIP, std::string("ncclGetUniqueId: ") + R.GetErrorString(r));
    std::memset(id_out, 0, MFSGD_DSGD_ID_BYTES);
    std::memcpy(id_out, &id, sizeof id);
    return MFSGD_OK;
}

std::unique_ptr<Transport> rccl_transport(std::string& err) {
    Rccl& R = rccl();
    if (R.lib) return std::make_unique<RcclTransport>();
    err = "RCCL is not available: " + R.why;
    return nullptr;
}

}  // namespace mfsgd
