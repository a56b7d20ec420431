// dsgd.cpp -- DSGD over the GPUs of one node, under the C-ABI (mfsgd_dsgd_*, include/mfsgd.h).
//
// No reference counterpart exists (/root/reference/README.md:1-2 is the whole reference); this is
// SURVEY.md section 3's call stack (train -> kernel -> ncclGroupStart / ncclSend / ncclRecv /
// ncclGroupEnd) and section 8e: one process per GPU, rank g keeps the P rows of its users for the
// whole run, the item-factor blocks travel along a ring -- one point-to-point message per block and
// sub-epoch over xGMI, no all-to-all, no data-path all-reduce; RMSE is one 2-double all-reduce.
//
// A pure client of the library's own public entry points (mfsgd_part_*), HIP streams / events and a
// transport (transport.hpp): this file is the ring, what moves its blocks is behind that seam -- RCCL
// in the product (rccl_transport.cpp), shared memory for rehearsals on one GPU (shm_transport.cpp).
//
// Streams: the partitions of a rank's group are trained one after another on the compute stream
// (they update the same P rows); block j leaves on the communication stream as soon as ITS training
// has finished -- while block j + 1 is being trained -- and the next sub-epoch's training of slot j
// waits for slot j's arrival only.  With one partition per rank that is train -> shift -> train with
// no host involvement; with m > 1 the shifts hide behind the training of the other blocks.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mfsgd.h"
#include "devmem.hpp"
#include "guard.hpp"
#include "records.hpp"
#include "transport.hpp"

struct mfsgd_dsgd {
    mfsgd_handle* h = nullptr;
    int rank = 0, world = 1, m = 1;  // m: partitions a rank holds at a time (its "group")
    int n_parts = 1, kp = 0, k = 0, device = 0;
    int32_t max_rows = 0;
    int64_t nnz_local = 0;
    int cur = 0;
    int group = 0;  // group currently held: partitions group * m .. group * m + m - 1
    // counters (mfsgd_dsgd_stats): sub-epoch trainings enqueued, of those with the recovery point, of those re-run
    // as round launches; the bytes sent are the transport's
    int64_t n_trained = 0, n_checked = 0, n_rerun = 0;
    bool always_check = false;  // MFSGD_DSGD_CHECK=1: the recovery point in every sub-epoch
    std::string err;
    // What the destructor leaves goes in reverse order: the events, the streams, the buffers.
    mfsgd::DevBuf d_red;   // 2 doubles for the RMSE all-reduce
    mfsgd::DevBuf buf[2];  // [cur, nxt]: m blocks of max_rows x kp floats each
    mfsgd::Stream wire, compute;
    mfsgd::Event ev1, ev0;
    std::vector<mfsgd::Event> arrived, trained;  // per slot j
    std::unique_ptr<mfsgd::Transport> tp;

    ~mfsgd_dsgd() {
        (void)hipSetDevice(device);
        if (compute) (void)hipStreamSynchronize(compute);
        if (wire) (void)hipStreamSynchronize(wire);
        tp.reset();
    }
    size_t count() const { return (size_t)max_rows * kp; }  // floats of one block
    float* block(int which, int j) const { return buf[which].as<float>() + (size_t)j * count(); }
    int part(int j) const { return group * m + j; }
};

namespace {

thread_local std::string g_dsgd_error;

int dfail(mfsgd_dsgd* d, int code, const std::string& msg) {
    if (d) d->err = msg;
    else g_dsgd_error = msg;
    return code;
}

// The guard (guard.hpp) with this unit's error channel: the ring's message or, without a ring, the thread's.
template <class F>
int dsgd_guarded(mfsgd_dsgd* d, const char* name, F&& body) {
    return mfsgd::guard_run(body, MFSGD_ERR_HIP, [&](int code, const char* what) { return dfail(d, code, std::string(name) + ": " + what); });
}

#define DHIP(d, call) TRANSPORT_HIP((d)->err, call)
#define DLIB(d, call)                                                                                   \
    do {                                                                                                \
        int rc_ = (call);                                                                               \
        if (rc_ != MFSGD_OK) return dfail((d), rc_, std::string(#call) + ": " + mfsgd_last_error((d)->h)); \
    } while (0)
// ... and while the ring is made: "dsgd_create: <what>: <HIP's message>", `code`
#define DMAKE(d, code, what, call)                                                                      \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return dfail((d), (code), std::string("dsgd_create: ") + (what) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Which library this is.  libmfsgd_rehearsal.so (the Makefile's -D, and shm_transport.cpp linked in) hands a request
// for the rehearsal transport on to it; the product has no such transport and refuses.
#ifdef MFSGD_DSGD_REHEARSAL
constexpr auto kShmUniqueId = &mfsgd::shm_unique_id;
constexpr auto kShmTransport = &mfsgd::shm_transport;
#else
constexpr decltype(&mfsgd::shm_unique_id) kShmUniqueId = nullptr;
constexpr decltype(&mfsgd::shm_transport) kShmTransport = nullptr;
#endif  // MFSGD_DSGD_REHEARSAL

// One rotation: `world` sub-epochs over the m slots, after which every block is home again.  Slot j waits for its
// block's arrival, work(j) is enqueued on (or waits for) the compute stream, and the block goes to rank - 1 behind it
// while the next one arrives from rank + 1.  No host synchronisation of its own.
template <class Work>
int rotation(mfsgd_dsgd* d, Work&& work) {
    for (int s = 0; s < d->world; ++s) {
        for (int j = 0; j < d->m; ++j) {
            DHIP(d, hipStreamWaitEvent(d->compute, d->arrived[(size_t)j], 0));
            int rc = work(j);
            if (rc) return rc;
            DHIP(d, hipEventRecord(d->trained[(size_t)j], d->compute));
            rc = d->tp->shift(j, d->block(d->cur, j), d->block(d->cur ^ 1, j), d->trained[(size_t)j], d->arrived[(size_t)j], d->err);
            if (rc) return rc;
        }
        d->cur ^= 1;
        d->group = (d->group + 1) % d->world;
    }
    return MFSGD_OK;
}

// One epoch: a rotation of train-the-group, pass-it-on.  Asynchronous -- no host synchronisation inside --
// unless `checked`: then every block passes the recovery point (mfsgd_part_settle) before it leaves.  A persistent
// training launch that finds its workgroups not co-resident (an exchange of the ring, or a foreign kernel, holds CUs)
// changes nothing; unnoticed, the untrained block would travel on and the ranks' factors diverge for good.  At the
// recovery point the host waits for the training, and a launch that gave up is repeated as round launches before the
// block is sent.  Cost: the launch latencies of one sub-epoch, exposed once per sub-epoch.
int enqueue_epoch(mfsgd_dsgd* d, bool checked) {
    return rotation(d, [&](int j) -> int {
        DLIB(d, mfsgd_part_train(d->h, d->part(j), d->block(d->cur, j), d->compute));
        d->n_trained++;
        if (checked) {
            int32_t rerun = 0;
            DLIB(d, mfsgd_part_settle(d->h, d->part(j), d->block(d->cur, j), d->compute, &rerun));
            d->n_checked++;
            d->n_rerun += rerun;
        }
        return MFSGD_OK;
    });
}

// Whether epoch e of a train call passes the recovery point:
//  - the first epoch of every train call: what a launch meets on this node shows there (the partition then stays on
//    round launches, so later epochs cannot fail the same way);
//  - every epoch when a rank holds several partitions (m > 1): slot j's exchange is in flight while slot j + 1 is
//    trained, for the whole run, and how long a peer keeps an exchange waiting is not this rank's to know;
//  - every epoch under MFSGD_DSGD_CHECK=1.
// With m = 1 nothing of the ring runs beside a training launch (train -> shift -> train), so the later epochs go
// unchecked; a launch that still gives up (a foreign process) surfaces in finish() as "factors invalid".
bool checked_epoch(const mfsgd_dsgd* d, int e) { return e == 0 || d->m > 1 || d->always_check; }

int finish(mfsgd_dsgd* d) {
    DHIP(d, hipStreamSynchronize(d->compute));
    DHIP(d, hipStreamSynchronize(d->wire));
    for (int p = 0; p < d->n_parts; ++p) DLIB(d, mfsgd_part_sync(d->h, p, d->compute));
    return MFSGD_OK;
}

// Sum of squared errors of this rank's ratings: one read-only rotation (blocks come home again).
int local_sse(mfsgd_dsgd* d, double* out) {
    int rc = finish(d);
    if (rc) return rc;
    double total = 0.0;
    rc = rotation(d, [&](int j) -> int {
        double sse = 0.0;
        DLIB(d, mfsgd_part_sse(d->h, d->part(j), d->block(d->cur, j), d->compute, &sse));  // synchronous
        total += sse;
        return MFSGD_OK;
    });
    if (rc) return rc;
    DHIP(d, hipStreamSynchronize(d->wire));
    *out = total;
    return MFSGD_OK;
}

int rmse(mfsgd_dsgd* d, double* out) {
    double v[2] = {0.0, (double)d->nnz_local};
    int rc = local_sse(d, &v[0]);
    if (rc) return rc;
    if ((rc = d->tp->allreduce2(v, false, d->err))) return rc;
    *out = v[1] > 0 ? std::sqrt(v[0] / v[1]) : 0.0;
    return MFSGD_OK;
}

// A block on the host is `rows` rows `stride` floats apart, k of them used; on the device max_rows x kp, zero padded.
int put_block(mfsgd_dsgd* d, int j, const float* src, int32_t rows, int stride) {
    std::vector<float> host(d->count(), 0.0f);
    for (int32_t x = 0; x < rows; ++x) std::memcpy(&host[(size_t)x * d->kp], src + (size_t)x * stride, sizeof(float) * (size_t)d->k);
    for (float& x : host) x = mfsgd::canon_nan(x);  // (records.hpp: no NaN keeps a payload of the caller's)
    DHIP(d, hipMemcpy(d->block(d->cur, j), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return MFSGD_OK;
}

int get_block(mfsgd_dsgd* d, int j, float* dst, int32_t rows) {
    std::vector<float> host(d->count());
    DHIP(d, hipMemcpy(host.data(), d->block(d->cur, j), host.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int32_t x = 0; x < rows; ++x) std::memcpy(dst + (size_t)x * d->k, &host[(size_t)x * d->kp], sizeof(float) * (size_t)d->k);
    return MFSGD_OK;
}

// Everything of mfsgd_dsgd_create that can fail half-way: the caller owns d, so an error is a return.
int make_ring(mfsgd_dsgd* d, const void* id) {
    if (const char* c = std::getenv("MFSGD_DSGD_CHECK")) d->always_check = std::atoi(c) != 0;
    for (int p = 0; p < d->n_parts; ++p) {
        int32_t rows = 0;
        mfsgd_schedule_info info;
        if (mfsgd_part_rows(d->h, p, &rows) != MFSGD_OK || mfsgd_get_schedule_info(d->h, p, &info) != MFSGD_OK)
            return dfail(d, MFSGD_ERR_STATE, std::string("dsgd_create: ") + mfsgd_last_error(d->h) + " (set the ratings first)");
        d->max_rows = std::max(d->max_rows, rows);
        d->nnz_local += info.nnz;
    }
    if (d->max_rows < 1) d->max_rows = 1;
    DMAKE(d, MFSGD_ERR_NO_DEVICE, "hipSetDevice", hipSetDevice(d->device));
    DMAKE(d, MFSGD_ERR_HIP, "hipStreamCreate", d->compute.create(hipStreamNonBlocking));
    DMAKE(d, MFSGD_ERR_HIP, "hipStreamCreate", d->wire.create(hipStreamNonBlocking));
    DMAKE(d, MFSGD_ERR_HIP, "hipEventCreate", d->ev0.create(hipEventDefault));
    DMAKE(d, MFSGD_ERR_HIP, "hipEventCreate", d->ev1.create(hipEventDefault));
    const size_t bytes = (size_t)d->m * d->count() * sizeof(float);
    for (int b = 0; b < 2; ++b) {
        DMAKE(d, MFSGD_ERR_OOM, "hipMalloc(Q blocks)", d->buf[b].alloc(bytes));
        DMAKE(d, MFSGD_ERR_HIP, "hipMemset", hipMemset(d->buf[b].get(), 0, bytes));
    }
    DMAKE(d, MFSGD_ERR_OOM, "hipMalloc", d->d_red.alloc(2 * sizeof(double)));
    d->trained.resize((size_t)d->m);
    d->arrived.resize((size_t)d->m);
    for (int j = 0; j < d->m; ++j) {
        DMAKE(d, MFSGD_ERR_HIP, "hipEventCreate", d->trained[(size_t)j].create(hipEventDisableTiming));
        DMAKE(d, MFSGD_ERR_HIP, "hipEventCreate", d->arrived[(size_t)j].create(hipEventDisableTiming));
    }
    return d->tp->bring_up(id, d->rank, d->world, d->m, d->count(), d->wire, d->d_red.as<double>(), d->err);
}

}  // namespace

extern "C" {

const char* mfsgd_dsgd_last_error(const mfsgd_dsgd* d) { return d ? d->err.c_str() : g_dsgd_error.c_str(); }

int mfsgd_dsgd_unique_id(void* id_out) {
    return dsgd_guarded(nullptr, "dsgd_unique_id", [&]() -> int {
        if (!id_out) return dfail(nullptr, MFSGD_ERR_INVALID_ARG, "dsgd_unique_id: null argument");
        const char* tr = std::getenv("MFSGD_DSGD_TRANSPORT");
        if (tr && std::strcmp(tr, "shm") == 0) {
            if (!kShmUniqueId)
                return dfail(nullptr, MFSGD_ERR_UNSUPPORTED, "MFSGD_DSGD_TRANSPORT=shm: this library has no rehearsal transport; load lib/libmfsgd_rehearsal.so (MFSGD_LIBRARY)");
            kShmUniqueId(id_out);
            return MFSGD_OK;
        }
        std::string why;
        const int rc = mfsgd::rccl_unique_id(id_out, why);
        return rc ? dfail(nullptr, rc, why) : MFSGD_OK;
    });
}

int mfsgd_dsgd_create(mfsgd_handle* h, int32_t rank, int32_t world, const void* id, mfsgd_dsgd** out) {
    if (out) *out = nullptr;
    return dsgd_guarded(nullptr, "dsgd_create", [&]() -> int {
        if (!h || !id || !out || world < 1 || rank < 0 || rank >= world)
            return dfail(nullptr, MFSGD_ERR_INVALID_ARG, "dsgd_create: bad argument");
        std::string why;
        std::unique_ptr<mfsgd::Transport> tp;
        if (!mfsgd::is_shm_id(id))
            tp = mfsgd::rccl_transport(why);
        else if (kShmTransport)
            tp = kShmTransport(world, why);
        else
            why = "dsgd_create: the id names a shared-memory segment, and this library has no rehearsal transport; "
                  "load lib/libmfsgd_rehearsal.so (MFSGD_LIBRARY)";
        if (!tp) return dfail(nullptr, MFSGD_ERR_UNSUPPORTED, why);
        int32_t n_parts = 0, kp = 0, device = 0, k = 0;
        if (mfsgd_get_parts(h, &n_parts, &kp, &device) != MFSGD_OK || mfsgd_get_dims(h, nullptr, nullptr, &k) != MFSGD_OK)
            return dfail(nullptr, MFSGD_ERR_INVALID_ARG, "dsgd_create: bad handle");
        if (n_parts < 2 && world > 1) return dfail(nullptr, MFSGD_ERR_STATE, "dsgd_create: the handle was created with n_parts <= 1");
        if (n_parts % world != 0)
            return dfail(nullptr, MFSGD_ERR_INVALID_ARG, "dsgd_create: n_parts (" + std::to_string(n_parts) + ") is not a multiple of world (" +
                                                             std::to_string(world) + ")");
        auto d = std::make_unique<mfsgd_dsgd>();
        d->h = h;
        d->rank = rank;
        d->world = world;
        d->n_parts = n_parts;
        d->m = n_parts / world;
        d->kp = kp;
        d->k = k;
        d->device = device;
        d->group = rank;
        d->tp = std::move(tp);
        const int rc = make_ring(d.get(), id);
        if (rc) return dfail(nullptr, rc, d->err);
        *out = d.release();
        return MFSGD_OK;
    });
}

void mfsgd_dsgd_destroy(mfsgd_dsgd* d) { delete d; }

int mfsgd_dsgd_init_q(mfsgd_dsgd* d, int64_t seed, int64_t u_total) {
    return dsgd_guarded(d, "dsgd_init_q", [&]() -> int {
        if (!d || u_total < 0) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_init_q: bad argument");
        int rc = finish(d);
        if (rc) return rc;
        if (d->group != d->rank) return dfail(d, MFSGD_ERR_STATE, "dsgd_init_q: blocks are not home");
        std::vector<float> host(d->count());  // rows x kp of it are written
        for (int j = 0; j < d->m; ++j) {
            int32_t rows = 0;
            DLIB(d, mfsgd_part_rows(d->h, d->part(j), &rows));
            DLIB(d, mfsgd_part_init_q(d->h, d->part(j), seed, u_total, host.data()));
            if ((rc = put_block(d, j, host.data(), rows, d->kp))) return rc;
        }
        return MFSGD_OK;
    });
}

int mfsgd_dsgd_set_q(mfsgd_dsgd* d, int32_t j, const float* block_host) {
    return dsgd_guarded(d, "dsgd_set_q", [&]() -> int {
        if (!d || !block_host || j < 0 || j >= d->m) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_set_q: bad argument");
        int rc = finish(d);
        if (rc) return rc;
        int32_t rows = 0;
        DLIB(d, mfsgd_part_rows(d->h, d->part(j), &rows));
        return put_block(d, j, block_host, rows, d->k);
    });
}

int mfsgd_dsgd_get_q(mfsgd_dsgd* d, int32_t j, int32_t* part, int32_t* rows_out, float* block_host) {
    return dsgd_guarded(d, "dsgd_get_q", [&]() -> int {
        if (!d || j < 0 || j >= d->m) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_get_q: bad argument");
        int rc = finish(d);
        if (rc) return rc;
        int32_t rows = 0;
        DLIB(d, mfsgd_part_rows(d->h, d->part(j), &rows));
        if (part) *part = d->part(j);
        if (rows_out) *rows_out = rows;
        return block_host ? get_block(d, j, block_host, rows) : MFSGD_OK;
    });
}

int mfsgd_dsgd_rmse(mfsgd_dsgd* d, double* out) {
    return dsgd_guarded(d, "dsgd_rmse", [&]() -> int {
        if (!d || !out) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_rmse: null argument");
        return rmse(d, out);
    });
}

int mfsgd_dsgd_train(mfsgd_dsgd* d, int32_t epochs, double* rmse_per_epoch) {
    return dsgd_guarded(d, "dsgd_train", [&]() -> int {
        if (!d || epochs < 0) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_train: bad argument");
        for (int e = 0; e < epochs; ++e) {
            int rc = enqueue_epoch(d, checked_epoch(d, e));
            if (rc) return rc;
            if (rmse_per_epoch && (rc = rmse(d, &rmse_per_epoch[e]))) return rc;
        }
        return finish(d);
    });
}

int mfsgd_dsgd_train_timed(mfsgd_dsgd* d, int32_t epochs, double* elapsed_ms) {
    return dsgd_guarded(d, "dsgd_train_timed", [&]() -> int {
        if (!d || epochs < 0 || !elapsed_ms) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_train_timed: bad argument");
        int rc = finish(d);
        if (rc) return rc;
        DHIP(d, hipEventRecord(d->ev0, d->compute));
        for (int e = 0; e < epochs; ++e)
            if ((rc = enqueue_epoch(d, checked_epoch(d, e)))) return rc;
        // the last blocks arrive on the communication stream: the epoch ends when they are home
        for (int j = 0; j < d->m; ++j) DHIP(d, hipStreamWaitEvent(d->compute, d->arrived[(size_t)j], 0));
        DHIP(d, hipEventRecord(d->ev1, d->compute));
        DHIP(d, hipEventSynchronize(d->ev1));
        float ms = 0.f;
        DHIP(d, hipEventElapsedTime(&ms, d->ev0, d->ev1));
        *elapsed_ms = (double)ms;
        return finish(d);
    });
}

int mfsgd_dsgd_stats(const mfsgd_dsgd* d, int64_t* out4) {
    if (!d || !out4) return MFSGD_ERR_INVALID_ARG;
    out4[0] = d->n_trained;
    out4[1] = d->n_checked;
    out4[2] = d->n_rerun;
    out4[3] = d->tp->bytes_sent;
    return MFSGD_OK;
}

int mfsgd_dsgd_allreduce(mfsgd_dsgd* d, double* values2, int32_t op) {
    return dsgd_guarded(d, "dsgd_allreduce", [&]() -> int {
        if (!d || !values2 || op < 0 || op > 1) return dfail(d, MFSGD_ERR_INVALID_ARG, "dsgd_allreduce: bad argument");
        return d->tp->allreduce2(values2, op == 1, d->err);
    });
}

}  // extern "C"
