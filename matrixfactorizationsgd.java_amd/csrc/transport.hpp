// transport.hpp -- the seam between the DSGD ring (dsgd.cpp) and what moves its blocks: the four things the ring needs
// from a transport, and the two transports there are.  Internal: installed nowhere.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>

#include "../../include/mfsgd.h"

namespace mfsgd {

// Every call returns MFSGD_OK or a code with its message in `err`.  Tear-down is the destructor; the ring has waited
// for both of its streams by then.
struct Transport {
    int64_t bytes_sent = 0;  // by shift(), since bring_up()
    virtual ~Transport() = default;
    // Collective.  `id` is the ring's MFSGD_DSGD_ID_BYTES; a block is `count` floats, a rank holds `slots` of them at a
    // time; `wire` is the ring's communication stream and `red` device memory for two doubles.
    virtual int bring_up(const void* id, int rank, int world, int slots, size_t count, hipStream_t wire, double* red,
                         std::string& err) = 0;
    // Shift slot j: once `trained` has happened, `send` goes to rank - 1 and the block of rank + 1 lands in `recv`;
    // `arrived` is recorded on the communication stream behind it.
    virtual int shift(int j, const float* send, float* recv, hipEvent_t trained, hipEvent_t arrived, std::string& err) = 0;
    // v[0], v[1] become their sums (their maxima: `max`) over the ranks, the same bits on every rank.  Synchronous.
    virtual int allreduce2(double* v, bool max, std::string& err) = 0;
};

inline int transport_fail(std::string& err, int code, std::string msg) {
    err = std::move(msg);
    return code;
}
#define TRANSPORT_HIP(err, call)                                                                       \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mfsgd::transport_fail((err), e_ == hipErrorOutOfMemory ? MFSGD_ERR_OOM : MFSGD_ERR_HIP, \
                                         std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

// rccl_transport.cpp -- the product's: ncclSend / ncclRecv in a group on the communication stream.  RCCL is bound on
// first use; where there is none, rccl_transport() is null and rccl_unique_id() MFSGD_ERR_UNSUPPORTED, `err` says why.
int rccl_unique_id(void* id_out, std::string& err);
std::unique_ptr<Transport> rccl_transport(std::string& err);

// shm_transport.cpp -- the rehearsal transport, in lib/libmfsgd_rehearsal.so only: several ranks on ONE GPU, blocks
// staged through a POSIX shared-memory segment that the id names.  Null and `err`: more ranks than it has room for.
void shm_unique_id(void* id_out);
std::unique_ptr<Transport> shm_transport(int world, std::string& err);

// An id that names a segment, not an RCCL id.  (Either library can tell; only the rehearsal library can use one.)
constexpr char kShmMagic[8] = {'M', 'F', 'S', 'G', 'D', 'S', 'H', 'M'};
inline bool is_shm_id(const void* id) { return std::memcmp(id, kShmMagic, sizeof kShmMagic) == 0; }

}  // namespace mfsgd
