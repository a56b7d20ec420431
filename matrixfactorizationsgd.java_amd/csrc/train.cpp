// train.cpp -- epochs: the launch paths (one launch per round, the persistent kernel, the captured graph), the
// persistent kernel's recovery protocol, the training calls, lr / lambda on a live handle, the held-out set with its
// RMSE and early stopping on it, the DSGD partition calls and the diagnostics of the epoch kernel.  (Online updates of
// the live factors: online_update.cpp.)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "handle.hpp"
#include "serve_util.hpp"

namespace mfsgd {

static CellLaunch make_launch(const mfsgd_handle* h, const Part& p, float* Q) {
    CellLaunch a{};
    a.P = p.swapped ? Q : h->dP.data();
    a.Q = p.swapped ? h->dP.data() : Q;
    a.cells = p.d_cells.data();
    a.rows = p.d_rows.data();
    a.subs = p.d_subs.data();
    a.entries = p.d_entries.data();
    a.B = p.sched.B;
    a.rd = 0;
    a.grid = p.sched.B;
    a.lds_bytes = p.sched.lds_bytes;
    a.sched_cap = p.sched.sched_cap;
    a.lr = h->cfg.lr;
    a.c = 1.0f - h->cfg.lr * h->cfg.lambda;
    a.sse_partial = p.d_sse_partial.as<double>();
    return a;
}

static int launch_epoch_eager(mfsgd_handle* h, Part& p, float* Q, hipStream_t st) {
    CellLaunch a = make_launch(h, p, Q);
    for (int rd = 0; rd < p.sched.B; ++rd) {
        a.rd = rd;
        HIPCHK(h, launch_cell(true, h->geo.L, p.sched.W, a, st));
    }
    return MFSGD_OK;
}

// The persistent epoch kernel needs every one of its workgroups resident at once.
static int probe_persistent(mfsgd_handle* h, Part& p) {
    if (p.persistent_np >= 0) return MFSGD_OK;
    p.persistent_np = 0;
    if (h->cfg.flags & MFSGD_FLAG_ROUND_LAUNCH) return MFSGD_OK;
    CellLaunch a = make_launch(h, p, nullptr);
    int per_cu = 0;
    hipError_t e = epoch_blocks_per_cu(h->geo.L, p.sched.W, a, &per_cu);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return MFSGD_OK;  // fall back to one launch per round
    }
    // DSGD partitions share the GPU with RCCL's send / recv kernels (a few workgroups, on their own stream): leave
    // them some CUs, or a persistent launch that needs the whole chip would sit in its residency check until the
    // exchange in flight has finished
    long np = (long)per_cu * (h->n_parts > 1 ? std::max(1, h->n_cu - 8) : h->n_cu);
    p.persistent_np = (int)std::min<long>(np, p.sched.B);
    return MFSGD_OK;
}

static int launch_epoch_body(mfsgd_handle* h, Part& p, float* Q, hipStream_t st) {
    if (p.persistent_np > 0) {
        CellLaunch a = make_launch(h, p, Q);
        a.grid = p.persistent_np;
        // flags are counted within the launch: zero them (and the abort word) every time
        // no memset: the kernel resets its own hand-off flags behind a device-side barrier (epoch.hip,
        // run_ring) -- a memset node in a replayed graph is not reliably ordered before the kernel node
        HIPCHK(h, launch_epoch_persistent(h->geo.L, p.sched.W, a, p.sched.B, p.d_sync.data(), abort_word(p), st));
        return MFSGD_OK;
    }
    return launch_epoch_eager(h, p, Q, st);
}

// One epoch of partition p against Q on stream st (asynchronous).
static int launch_epoch(mfsgd_handle* h, Part& p, float* Q, hipStream_t st) {
    if (p.sched.nnz == 0) return MFSGD_OK;
    int rc = probe_persistent(h, p);
    if (rc) return rc;
    if (h->cfg.flags & MFSGD_FLAG_NO_GRAPH) return launch_epoch_body(h, p, Q, st);
    const auto key = std::make_pair((const void*)h->dP.data(), (const void*)Q);
    auto it = p.graphs.find(key);
    if (it == p.graphs.end()) {
        // capture the launch(es) of one epoch once; replayed every epoch
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        rc = launch_epoch_body(h, p, Q, h->stream);
        hipError_t e = hipStreamEndCapture(h->stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        HIPCHK(h, e);
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HIPCHK(h, e);
        if (p.graphs.size() >= 32) {
            // replays of the old graphs may still be in flight on a caller's stream
            HIPCHK(h, hipDeviceSynchronize());
            p.drop_graphs();
        }
        it = p.graphs.emplace(key, exec).first;
    }
    HIPCHK(h, hipGraphLaunch(it->second, st));
    return MFSGD_OK;
}

// After a synchronisation point: did a persistent launch give up?  Returns MFSGD_OK, MFSGD_ERR_HIP (a
// hand-off or a solo helper timed out mid-epoch: the factors are invalid), or kNotResident: the
// launch found its workgroups not co-resident and did NOTHING (nor did any launch queued behind it);
// *started receives the number of launches since the last check that did run.
constexpr int kNotResident = 1;
static int check_abort(mfsgd_handle* h, Part& p, unsigned* started = nullptr) {
    if (started) *started = 0;
    if (p.persistent_np <= 0 || !p.d_sync) return MFSGD_OK;
    unsigned w[2] = {0, 0};
    HIPCHK(h, hipMemcpy(w, abort_word(p), sizeof w, hipMemcpyDeviceToHost));
    if (started) *started = w[1];
    if (w[0] != 0 || w[1] != 0) {
        // the device is idle on this stream (the caller has synchronised).  A give-up also leaves arrivals (and the
        // "somebody left" bit) in the start barrier's counter: zero it.  The GENERATION word next to it is never reset:
        // the tile mailboxes are tagged with it, and a launch that reused a generation could take a granule an aborted
        // launch left behind for this launch's (advisor finding, round 2).
        const unsigned zeros[2] = {0, 0};
        if (w[0] != 0) (void)hipMemcpy(abort_word(p) - 4, zeros, sizeof(unsigned), hipMemcpyHostToDevice);
        (void)hipMemcpy(abort_word(p), zeros, 2 * sizeof(unsigned), hipMemcpyHostToDevice);
    }
    if (w[0] == 2u) return kNotResident;
    if (w[0] != 0)
        return fail(h, MFSGD_ERR_HIP, "persistent epoch kernel timed out waiting for a tile hand-off (results invalid)");
    return MFSGD_OK;
}

// The persistent kernel could not get all its workgroups onto the chip (something else is running
// there): from now on this partition is trained with one launch per round, which needs no co-residency.
// `idle` (nullable): the one stream this partition's launches went to, already synchronised by the caller -- then
// nothing of the partition is in flight and the device-wide wait (which would also wait for a DSGD ring's exchange
// with a slower peer on its communication stream) is not needed.
static void give_up_persistence(mfsgd_handle* h, Part& p, const hipStream_t* idle = nullptr) {
    if (!idle) (void)hipDeviceSynchronize();
    p.drop_graphs();
    p.persistent_np = 0;
    h->n_not_resident++;
}

// For callers that cannot re-run what was skipped (asynchronous DSGD sub-epochs on caller-owned blocks).
static int check_abort_strict(mfsgd_handle* h, Part& p) {
    const int rc = check_abort(h, p);
    if (rc != kNotResident) return rc;
    give_up_persistence(h, p);
    return fail(h, MFSGD_ERR_HIP,
                "persistent epoch kernel: workgroups not co-resident (another kernel holds the GPU); the launch and those "
                "queued behind it of THIS partition were NOT applied -- the partition now uses one launch per round.  If other "
                "work depended on it (a DSGD ring that passed the block on), the factors are invalid: seed or load them again");
}

static int launch_sse(mfsgd_handle* h, Part& p, const float* Q, hipStream_t st) {
    CellLaunch a = make_launch(h, p, const_cast<float*>(Q));
    const int n_cells = (int)p.sched.cells.size();  // chunk descriptors: every one is independent here
    if (h->cfg.flags & MFSGD_FLAG_ROUND_LAUNCH) {  // reference form: one workgroup per chunk
        a.grid = n_cells;
        HIPCHK(h, launch_cell(false, h->geo.L, p.sched.W, a, st));
    } else {
        const int per_cu = std::max(1, std::min(4, (160 * 1024) / std::max(1, p.sched.lds_bytes)));
        a.grid = std::min(n_cells, per_cu * std::max(1, h->n_cu));
        HIPCHK(h, launch_sse_persistent(h->geo.L, p.sched.W, a, n_cells, st));
    }
    HIPCHK(h, launch_reduce_sse(a.sse_partial, (int64_t)a.grid, p.d_sse_out.data(), st));
    return MFSGD_OK;
}

static int part_sse_sync(mfsgd_handle* h, Part& p, const float* Q, hipStream_t st, double* sse) {
    if (p.sched.nnz == 0) {
        *sse = 0.0;
        return MFSGD_OK;
    }
    int rc = launch_sse(h, p, Q, st);
    if (rc) return rc;
    HIPCHK(h, copy_down(sse, p.d_sse_out, 1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return check_abort_strict(h, p);
}

// The RMSE of partition p against Q, on the handle's stream; *out is written when the call succeeds.
static int rmse_of(mfsgd_handle* h, Part& p, const float* Q, double* out) {
    double sse = 0.0;
    const int rc = part_sse_sync(h, p, Q, h->stream, &sse);
    if (rc) return rc;
    *out = p.sched.nnz > 0 ? std::sqrt(sse / (double)p.sched.nnz) : 0.0;
    return MFSGD_OK;
}

// `launched` epochs of a single-partition handle are in flight on st: wait, and if the persistent
// kernel found itself not resident (it then did nothing, nor did the launches behind it), run what
// is missing as one launch per round.
static int settle_epochs(mfsgd_handle* h, Part& p, float* Q, hipStream_t st, int launched) {
    HIPCHK(h, hipStreamSynchronize(st));
    unsigned started = 0;
    int rc = check_abort(h, p, &started);
    if (rc != kNotResident) return rc;
    give_up_persistence(h, p, &st);
    for (int e = (int)std::min<unsigned>(started, (unsigned)launched); e < launched; ++e)
        if ((rc = launch_epoch(h, p, Q, st))) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    return kNotResident;  // recovered: the missing epochs ran as round launches
}

static int settle_epochs_ok(mfsgd_handle* h, Part& p, float* Q, hipStream_t st, int launched) {
    const int rc = settle_epochs(h, p, Q, st, launched);
    return rc == kNotResident ? MFSGD_OK : rc;
}

// lr and lambda on a live handle ---------------------------------------------------
// The schedules keep their structure; the entries are re-baked wherever they live ("Changing lr and
// lambda"): the device copy by rehyper.hip on the handle's stream, the host copy by rehyper_schedule, both at once.
// The cached training graphs carry lr and c as kernel arguments: they are dropped and captured again on demand.
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static int apply_hyper(mfsgd_handle* h, float lr, float lambda) {
    if (same_bits(lr, h->cfg.lr) && same_bits(lambda, h->cfg.lambda)) return MFSGD_OK;
    if (!h->have_ratings) {
        h->cfg.lr = lr;
        h->cfg.lambda = lambda;
        return MFSGD_OK;
    }
    // whatever goes wrong from here on leaves entries half rewritten: the schedules are dropped then, and the next
    // mfsgd_set_ratings builds them again, with the new values
    auto broken = [&](int code, const std::string& msg) {
        if (h->device_ready) (void)hipDeviceSynchronize();
        h->parts.clear();
        h->have_ratings = false;
        h->cfg.lr = lr;
        h->cfg.lambda = lambda;
        return fail(h, code, "set_hyper: " + msg + " (the schedules were dropped: call mfsgd_set_ratings again)");
    };
    try {
        if (h->device_ready) {
            HIPCHK(h, hipSetDevice(h->cfg.device));
            // DSGD partitions are trained on the callers' streams: the header rules out launches in flight, this
            // makes sure of it before their graphs go
            HIPCHK(h, h->n_parts > 1 ? hipDeviceSynchronize() : hipStreamSynchronize(h->stream));
        }
        const float c = 1.0f - lr * lambda;
        // descriptors of a part that is not on the device yet; freed before this returns
        std::vector<DevArray<CellDesc>> temp_cells;
        std::vector<DevArray<SubDesc>> temp_subs;
        bool launched = false;
        for (Part& p : h->parts) {
            Schedule& s = p.sched;
            Entry* d_entries = p.on_device ? p.d_entries.data() : s.dev.entries.data();
            if (!d_entries || s.n_entry_recs == 0 || s.cells.empty()) continue;
            const CellDesc* d_cells = p.d_cells.data();
            const SubDesc* d_subs = p.on_device ? p.d_subs.data() : s.dev.subs.data();
            if (!p.on_device) {  // the device packer's buffers, not adopted yet: the descriptors are still on the host only
                temp_cells.emplace_back();
                if (const int rc = upload(h, temp_cells.back(), s.cells)) return broken(rc, "the chunk descriptors did not reach the device: " + h->err);
                d_cells = temp_cells.back().data();
                if (!d_subs) {
                    temp_subs.emplace_back();
                    if (const int rc = upload(h, temp_subs.back(), s.subs)) return broken(rc, "the sub-cell tables did not reach the device: " + h->err);
                    d_subs = temp_subs.back().data();
                }
            }
            const hipError_t e = launch_rehyper(d_cells, d_subs, d_entries, (int64_t)s.cells.size(), s.n_entry_recs, s.W,
                                                s.geo.G, lr, c, h->stream);
            if (e != hipSuccess) return broken(MFSGD_ERR_HIP, std::string("the re-bake kernel could not be launched: ") + hipGetErrorString(e));
            launched = true;
        }
        for (Part& p : h->parts) {
            Schedule& s = p.sched;
            if (s.entries.empty()) continue;
            if (!s.subs.empty()) {
                rehyper_schedule(s, lr, lambda, h->cfg.host_threads);
            } else {
                // (a host copy of a device-packed schedule whose sub-cell tables never came down: it is a copy made
                // on demand, and the next demand makes it again, from the re-baked device arrays)
                s.entries = PodVec<Entry>();
            }
        }
        if (launched) {
            const hipError_t e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) return broken(MFSGD_ERR_HIP, std::string("the re-bake kernel failed: ") + hipGetErrorString(e));
        }
        for (Part& p : h->parts) p.drop_graphs();
        h->cfg.lr = lr;
        h->cfg.lambda = lambda;
        return MFSGD_OK;
    } catch (const std::bad_alloc&) {
        return broken(MFSGD_ERR_OOM, "out of host memory");
    }
}

static bool is_nan(float x) { return !(x == x); }

// `epochs` epochs of partition 0 on the handle's stream.  lr and lambda (each nullable) hold the values of every
// epoch: an epoch without one runs at the handle's own.  rmse_per_epoch (nullable) receives the RMSE after every epoch.
static int run_epochs(mfsgd_handle* h, int epochs, const float* lr, const float* lambda, double* rmse_per_epoch) {
    int rc = prepare_compute(h);
    if (rc) return rc;
    float* Q = h->dQ.data();
    int pending = 0;  // epochs launched and not settled yet: all at the handle's current values
    for (int e = 0; e < epochs; ++e) {
        const float lr_e = lr ? lr[e] : h->cfg.lr, lam = lambda ? lambda[e] : h->cfg.lambda;
        if (!same_bits(lr_e, h->cfg.lr) || !same_bits(lam, h->cfg.lambda)) {
            // (a persistent launch that found itself not resident is made up for at the values it was launched with)
            if ((rc = settle_epochs_ok(h, h->parts[0], Q, h->stream, pending))) return rc;
            pending = 0;
            if ((rc = apply_hyper(h, lr_e, lam))) return rc;
        }
        Part& p = h->parts[0];
        if ((rc = launch_epoch(h, p, Q, h->stream))) return rc;
        ++pending;
        if (rmse_per_epoch) {
            if ((rc = settle_epochs_ok(h, p, Q, h->stream, pending))) return rc;
            pending = 0;
            if ((rc = rmse_of(h, p, Q, &rmse_per_epoch[e]))) return rc;
        }
    }
    return settle_epochs_ok(h, h->parts[0], Q, h->stream, pending);
}

// Held-out pairs ("Held-out validation and early stopping") ---------------------
// Pairs of one upload of mfsgd_rmse_pairs: 12 MB of staging.  A list of at most this many pairs is one launch, the
// launch mfsgd_validation_rmse makes for the handle's own set.  (include/mfsgd.h states the size, and PIECE of
// tests/test_validation_gpu.py cuts its slices by it: change the three together.)
constexpr int64_t kPairsPiece = (int64_t)1 << 20;

// The argument checks of a pair list, before any device work: `call` starts the message.
static int check_pairs(const mfsgd_handle* h, const char* call, const int32_t* u, const int32_t* i, const float* r, int64_t n) {
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": n is negative");
    if (n > 0 && (!u || !i || !r)) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": u, i or r is null");
    const int64_t j = first_outside(u, h->cfg.n_users, i, h->cfg.n_items, n);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": pair " + std::to_string(j) + " out of range");
    return MFSGD_OK;
}

// SSE of n >= 1 pairs that are on the device, under the handle's factors (P is always the users' matrix, whichever
// side of the kernels the schedule gave it: as mfsgd_predict reads it), on the handle's stream; waits for it.
static int pairs_sse_sync(mfsgd_handle* h, const char* call, const Validation& v, int64_t n, double* sse) {
    const std::string prefix = std::string(call) + ": ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    double* partial = v.d_sse.data();
    HIPCHK_OR(bad, launch_pairs_sse(h->geo.L, h->dP.data(), h->dQ.data(), v.du.data(), v.di.data(), v.dr.data(), n, partial,
                                    partial + kPairsSlots, h->stream));
    HIPCHK_OR(bad, copy_down(sse, v.d_sse, 1, h->stream, kPairsSlots));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// The handle's held-out set on the device (the device is there: the caller has asked for it); the host copy goes.
static int validation_to_device(mfsgd_handle* h) {
    Validation& v = h->val;
    if (v.on_device || v.n == 0) return MFSGD_OK;
    int rc;
    if ((rc = upload(h, v.du, v.hu)) || (rc = upload(h, v.di, v.hi)) || (rc = upload(h, v.dr, v.hr)) ||
        (rc = dev_alloc(h, v.d_sse, (size_t)kPairsSlots + 1))) {
        v.du.reset(), v.di.reset(), v.dr.reset(), v.d_sse.reset();
        return rc;
    }
    v.on_device = true;
    std::vector<int32_t>().swap(v.hu);
    std::vector<int32_t>().swap(v.hi);
    std::vector<float>().swap(v.hr);
    return MFSGD_OK;
}

// SSE of the handle's held-out set (not empty) under the current factors.
static int validation_sse(mfsgd_handle* h, const char* call, double* sse) {
    int rc = factors_to_device(h);
    if (rc || (rc = validation_to_device(h))) return rc;
    return pairs_sse_sync(h, call, h->val, h->val.n, sse);
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

int mfsgd_train(mfsgd_handle* h, int32_t epochs, double* rmse_per_epoch) {
    return guarded(h, "train", [&]() -> int {
        if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "train: bad argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "train: handle has n_parts > 1, drive it with mfsgd_part_train");
        if (const int rc = check_has_q(h, "train")) return rc;
        return run_epochs(h, epochs, nullptr, nullptr, rmse_per_epoch);
    });
}

int mfsgd_train_timed(mfsgd_handle* h, int32_t epochs, double* elapsed_ms, int64_t* launches) {
    return guarded(h, "train_timed", [&]() -> int {
        if (epochs < 0 || !elapsed_ms) return fail(h, MFSGD_ERR_INVALID_ARG, "train_timed: bad argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "train_timed: single-partition handles only");
        int rc = check_has_q(h, "train_timed");
        if (rc || (rc = prepare_compute(h))) return rc;
        Part& p = h->parts[0];
        float* Q = h->dQ.data();
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        for (int e = 0; e < epochs; ++e)
            if ((rc = launch_epoch(h, p, Q, h->stream))) return rc;
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipEventSynchronize(h->ev1));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        *elapsed_ms = (double)ms;
        if (launches) *launches = p.sched.nnz > 0 ? (int64_t)epochs * (p.persistent_np > 0 ? 1 : p.sched.B) : 0;
        return check_abort_strict(h, p);  // a timing of launches that did nothing would be meaningless
    });
}

int mfsgd_set_hyper(mfsgd_handle* h, float lr, float lambda) {
    return guarded(h, "set_hyper", [&]() -> int {
        if (is_nan(lr) || is_nan(lambda)) return fail(h, MFSGD_ERR_INVALID_ARG, "set_hyper: lr / lambda is NaN");
        return apply_hyper(h, lr, lambda);
    });
}

int mfsgd_get_hyper(const mfsgd_handle* h, float* lr, float* lambda) {
    if (!h) return MFSGD_ERR_INVALID_ARG;
    if (lr) *lr = h->cfg.lr;
    if (lambda) *lambda = h->cfg.lambda;
    return MFSGD_OK;
}

int mfsgd_train_schedule(mfsgd_handle* h, int32_t epochs, const float* lr, const float* lambda, double* rmse_per_epoch) {
    return guarded(h, "train_schedule", [&]() -> int {
        if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "train_schedule: negative epochs");
        if (epochs > 0 && !lr) return fail(h, MFSGD_ERR_INVALID_ARG, "train_schedule: lr is null");
        for (int e = 0; e < epochs; ++e)
            if (is_nan(lr[e]) || (lambda && is_nan(lambda[e])))
                return fail(h, MFSGD_ERR_INVALID_ARG, "train_schedule: lr / lambda of epoch " + std::to_string(e) + " is NaN");
        if (epochs == 0) return MFSGD_OK;
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "train_schedule: handle has n_parts > 1, drive it with mfsgd_part_train");
        if (const int rc = check_has_q(h, "train_schedule")) return rc;
        return run_epochs(h, epochs, lr, lambda, rmse_per_epoch);
    });
}

int mfsgd_train_bold_driver(mfsgd_handle* h, int32_t epochs, float up, float down, float* lr_used, double* rmse_per_epoch) {
    return guarded(h, "bold_driver", [&]() -> int {
        if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "bold_driver: negative epochs");
        if (!(up > 0.0f) || !(down > 0.0f)) return fail(h, MFSGD_ERR_INVALID_ARG, "bold_driver: up and down must be above zero");
        if (epochs > 0 && (!lr_used || !rmse_per_epoch))
            return fail(h, MFSGD_ERR_INVALID_ARG, "bold_driver: lr_used and rmse_per_epoch are both required");
        if (epochs == 0) return MFSGD_OK;
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "bold_driver: handle has n_parts > 1, drive it with mfsgd_part_train");
        int rc = check_has_q(h, "bold_driver");
        if (rc || (rc = prepare_compute(h))) return rc;
        float* Q = h->dQ.data();
        double prev = 0.0;
        if ((rc = rmse_of(h, h->parts[0], Q, &prev))) return rc;
        for (int e = 0; e < epochs; ++e) {
            lr_used[e] = h->cfg.lr;
            if ((rc = launch_epoch(h, h->parts[0], Q, h->stream))) return rc;
            if ((rc = settle_epochs_ok(h, h->parts[0], Q, h->stream, 1))) return rc;
            if ((rc = rmse_of(h, h->parts[0], Q, &rmse_per_epoch[e]))) return rc;
            // (a NaN RMSE compares false: the rate shrinks)
            const float next = rmse_per_epoch[e] < prev ? h->cfg.lr * up : h->cfg.lr * down;
            prev = rmse_per_epoch[e];
            if (is_nan(next)) return fail(h, MFSGD_ERR_STATE, "bold_driver: the learning rate became NaN after epoch " + std::to_string(e));
            if ((rc = apply_hyper(h, next, h->cfg.lambda))) return rc;
        }
        return MFSGD_OK;
    });
}

int mfsgd_rmse(mfsgd_handle* h, double* out) {
    return guarded(h, "rmse", [&]() -> int {
        if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, "rmse: null argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "rmse: handle has n_parts > 1, use mfsgd_part_sse");
        int rc = check_has_q(h, "rmse");
        if (rc || (rc = prepare_compute(h))) return rc;
        return rmse_of(h, h->parts[0], h->dQ.data(), out);
    });
}

int mfsgd_set_validation(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n) {
    return guarded(h, "set_validation", [&]() -> int {
        if (const int rc = check_pairs(h, "set_validation", u, i, r, n)) return rc;
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "set_validation: single-partition handles only");
        Validation fresh;
        if (n > 0) {
            fresh.hu.assign(u, u + n);
            fresh.hi.assign(i, i + n);
            fresh.hr.assign(r, r + n);
            fresh.n = n;
        }
        if (h->val.on_device) {  // an SSE pass over the old set cannot be in flight (every call waits), a D2H copy neither
            (void)hipSetDevice(h->cfg.device);
            (void)hipStreamSynchronize(h->stream);
        }
        h->val = std::move(fresh);
        return MFSGD_OK;
    });
}

int mfsgd_validation_size(const mfsgd_handle* h, int64_t* n) {
    return guarded(h, "validation_size", [&]() -> int {
        if (!n) return fail(h, MFSGD_ERR_INVALID_ARG, "validation_size: null argument");
        *n = h->val.n;
        return MFSGD_OK;
    });
}

int mfsgd_validation_rmse(mfsgd_handle* h, double* rmse, double* sse) {
    return guarded(h, "validation_rmse", [&]() -> int {
        if (!rmse) return fail(h, MFSGD_ERR_INVALID_ARG, "validation_rmse: rmse is null");
        if (const int rc = check_reads_factors(h, "validation_rmse")) return rc;
        double s = 0.0;
        if (h->val.n > 0)
            if (const int rc = validation_sse(h, "validation_rmse", &s)) return rc;
        *rmse = h->val.n > 0 ? std::sqrt(s / (double)h->val.n) : 0.0;
        if (sse) *sse = s;
        return MFSGD_OK;
    });
}

int mfsgd_rmse_pairs(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n, double* rmse, double* sse) {
    return guarded(h, "rmse_pairs", [&]() -> int {
        if (!rmse) return fail(h, MFSGD_ERR_INVALID_ARG, "rmse_pairs: rmse is null");
        if (const int rc = check_pairs(h, "rmse_pairs", u, i, r, n)) return rc;
        if (n == 0) {
            *rmse = 0.0;
            if (sse) *sse = 0.0;
            return MFSGD_OK;
        }
        int rc = check_reads_factors(h, "rmse_pairs");
        if (rc || (rc = factors_to_device(h))) return rc;
        auto bad = [h](hipError_t e) { return serve_fail(h, "rmse_pairs: ", e); };
        const int64_t piece = std::min(n, kPairsPiece);
        Validation st;  // the staging of one piece, and the scratch: the device arrays of a held-out set, for this call
        if ((rc = dev_alloc(h, st.du, (size_t)piece)) || (rc = dev_alloc(h, st.di, (size_t)piece))) return rc;
        if ((rc = dev_alloc(h, st.dr, (size_t)piece)) || (rc = dev_alloc(h, st.d_sse, (size_t)kPairsSlots + 1))) return rc;
        double total = 0.0;
        for (int64_t j0 = 0; j0 < n; j0 += piece) {
            const int64_t c = std::min(piece, n - j0);
            double s = 0.0;
            HIPCHK_OR(bad, copy_up(st.du, u + j0, (size_t)c, h->stream));
            HIPCHK_OR(bad, copy_up(st.di, i + j0, (size_t)c, h->stream));
            HIPCHK_OR(bad, copy_up(st.dr, r + j0, (size_t)c, h->stream));
            if ((rc = pairs_sse_sync(h, "rmse_pairs", st, c, &s))) return rc;  // (the staging buffers are reused)
            total = j0 == 0 ? s : total + s;
        }
        *rmse = std::sqrt(total / (double)n);
        if (sse) *sse = total;
        return MFSGD_OK;
    });
}

int mfsgd_train_early_stop(mfsgd_handle* h, int32_t max_epochs, int32_t patience, double min_delta, int32_t restore_best,
                           const float* lr, const float* lambda, double* val_rmse, double* train_rmse, int32_t* epochs_run,
                           int32_t* best_epoch) {
    return guarded(h, "early_stop", [&]() -> int {
        if (max_epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: negative max_epochs");
        if (patience < 1) return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: patience must be at least 1");
        if (!(min_delta >= 0.0)) return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: min_delta is NaN or negative");
        if (!epochs_run || !best_epoch) return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: epochs_run or best_epoch is null");
        if (max_epochs > 0 && !val_rmse) return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: val_rmse is null");
        for (int e = 0; e < max_epochs; ++e)
            if ((lr && is_nan(lr[e])) || (lambda && is_nan(lambda[e])))
                return fail(h, MFSGD_ERR_INVALID_ARG, "early_stop: lr / lambda of epoch " + std::to_string(e) + " is NaN");
        if (max_epochs == 0) {
            *epochs_run = 0;
            *best_epoch = -1;
            return MFSGD_OK;
        }
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "early_stop: handle has n_parts > 1, drive it with mfsgd_part_train");
        if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "early_stop: no ratings: call mfsgd_set_ratings first");
        if (h->val.n == 0) return fail(h, MFSGD_ERR_STATE, "early_stop: no validation set: call mfsgd_set_validation first");
        int rc = check_reads_factors(h, "early_stop");
        if (rc) return rc;
        *epochs_run = 0;  // (a call rejected above has touched nothing; from here on the two say how far it got)
        *best_epoch = -1;
        if ((rc = prepare_compute(h)) || (rc = validation_to_device(h))) return rc;
        auto bad = [h](hipError_t e) { return serve_fail(h, "early_stop: ", e); };
        DevBuf snap_p, snap_q;  // the factors after the best epoch so far; gone when this returns, whichever way
        if (restore_best) {
            if ((rc = dev_alloc(h, snap_p, h->p_bytes()))) return rc;
            if ((rc = dev_alloc(h, snap_q, h->q_bytes()))) return rc;
        }
        double best = HUGE_VAL;
        int bad_epochs = 0;
        for (int e = 0; e < max_epochs; ++e) {
            if ((rc = run_epochs(h, 1, lr ? lr + e : nullptr, lambda ? lambda + e : nullptr, train_rmse ? train_rmse + e : nullptr)))
                return rc;
            *epochs_run = e + 1;
            double s = 0.0;
            if ((rc = validation_sse(h, "early_stop", &s))) return rc;
            const double v = val_rmse[e] = std::sqrt(s / (double)h->val.n);
            if (v < best - min_delta) {  // (a NaN compares false)
                best = v;
                *best_epoch = e;
                bad_epochs = 0;
                if (restore_best) {
                    HIPCHK_OR(bad, hipMemcpyAsync(snap_p.get(), h->dP.data(), h->p_bytes(), hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK_OR(bad, hipMemcpyAsync(snap_q.get(), h->dQ.data(), h->q_bytes(), hipMemcpyDeviceToDevice, h->stream));
                }
            } else if (++bad_epochs >= patience) {
                break;
            }
        }
        if (restore_best && *best_epoch >= 0 && *best_epoch != *epochs_run - 1) {
            HIPCHK_OR(bad, hipMemcpyAsync(h->dP.data(), snap_p.get(), h->p_bytes(), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(h->dQ.data(), snap_q.get(), h->q_bytes(), hipMemcpyDeviceToDevice, h->stream));
        }
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the snapshot is freed behind this
        return MFSGD_OK;
    });
}

int mfsgd_part_train(mfsgd_handle* h, int32_t part, float* q_block_dev, void* stream) {
    return guarded(h, "part_train", [&]() -> int {
        if (!q_block_dev) return fail(h, MFSGD_ERR_INVALID_ARG, "part_train: null argument");
        int rc = check_part(h, part, "part_train");
        if (rc || (rc = prepare_compute(h))) return rc;
        // the caller owns the Q block, so the caller names the stream (NULL = HIP's null stream)
        return launch_epoch(h, h->parts[(size_t)part], q_block_dev, static_cast<hipStream_t>(stream));
    });
}

int mfsgd_part_settle(mfsgd_handle* h, int32_t part, float* q_block_dev, void* stream, int32_t* rerun) {
    if (rerun) *rerun = 0;
    return guarded(h, "part_settle", [&]() -> int {
        if (!q_block_dev) return fail(h, MFSGD_ERR_INVALID_ARG, "part_settle: null argument");
        if (int rc = check_part(h, part, "part_settle")) return rc;
        if (!h->device_ready || !h->have_ratings) return MFSGD_OK;  // nothing can have been launched
        HIPCHK(h, hipSetDevice(h->cfg.device));
        Part& p = h->parts[(size_t)part];
        if (p.sched.nnz == 0) {
            HIPCHK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
            return MFSGD_OK;
        }
        const int rc = settle_epochs(h, p, q_block_dev, static_cast<hipStream_t>(stream), 1);
        if (rc == kNotResident) {
            if (rerun) *rerun = 1;
            return MFSGD_OK;
        }
        return rc;
    });
}

int mfsgd_part_sync(mfsgd_handle* h, int32_t part, void* stream) {
    return guarded(h, "part_sync", [&]() -> int {
        if (int rc = check_part(h, part, "part_sync")) return rc;
        if (!h->device_ready || !h->have_ratings) return MFSGD_OK;  // nothing can have been launched
        HIPCHK(h, hipSetDevice(h->cfg.device));
        HIPCHK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        return check_abort_strict(h, h->parts[(size_t)part]);
    });
}

int mfsgd_part_sse(mfsgd_handle* h, int32_t part, const float* q_block_dev, void* stream, double* sse) {
    return guarded(h, "part_sse", [&]() -> int {
        if (!q_block_dev || !sse) return fail(h, MFSGD_ERR_INVALID_ARG, "part_sse: null argument");
        int rc = check_part(h, part, "part_sse");
        if (rc || (rc = prepare_compute(h))) return rc;
        return part_sse_sync(h, h->parts[(size_t)part], q_block_dev, static_cast<hipStream_t>(stream), sse);
    });
}

int mfsgd_debug_epoch_profile(mfsgd_handle* h, uint64_t* out, int32_t* n_workgroups) {
    return guarded(h, "debug_epoch_profile", [&]() -> int {
        if (!out || !n_workgroups) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_epoch_profile: null argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_epoch_profile: single-partition handles only");
        int rc = check_has_q(h, "debug_epoch_profile");
        if (rc || (rc = prepare_compute(h))) return rc;
        Part& p = h->parts[0];
        if ((rc = probe_persistent(h, p))) return rc;
        if (p.persistent_np <= 0) return fail(h, MFSGD_ERR_STATE, "debug_epoch_profile: persistent kernel not in use");
        const size_t words = (size_t)p.persistent_np * 16;
        if ((rc = dev_alloc(h, p.d_sse_partial, std::max(words * sizeof(uint64_t), sizeof(double) * p.sched.cells.size())))) return rc;
        CellLaunch a = make_launch(h, p, h->dQ.data());
        a.grid = p.persistent_np;
        a.diag = true;
        a.sse_partial = p.d_sse_partial.as<double>();
        HIPCHK(h, hipMemsetAsync(p.d_sse_partial.get(), 0, words * sizeof(uint64_t), h->stream));
        HIPCHK(h, launch_epoch_persistent(h->geo.L, p.sched.W, a, p.sched.B, p.d_sync.data(), abort_word(p), h->stream));
        HIPCHK(h, hipMemcpyAsync(out, p.d_sse_partial.get(), words * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *n_workgroups = p.persistent_np;
        return check_abort_strict(h, p);
    });
}

int mfsgd_debug_counters(const mfsgd_handle* h, int64_t* out4) {
    return guarded(h, "debug_counters", [&]() -> int {
        if (!out4) return MFSGD_ERR_INVALID_ARG;
        out4[0] = h->n_not_resident;
        out4[1] = out4[2] = 0;
        out4[3] = h->n_schedule_builds;
        for (const Part& p : h->parts) {
            out4[1] += p.persistent_np > 0 ? 1 : 0;  // partitions trained by the persistent kernel
            out4[2] += (int64_t)p.graphs.size();
        }
        return MFSGD_OK;
    });
}

int mfsgd_debug_occupy(mfsgd_handle* h, int32_t milliseconds) {
    return guarded(h, "debug_occupy", [&]() -> int {
        if (milliseconds < 0 || milliseconds > 5000) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_occupy: bad argument");
        int rc = ensure_device(h);
        if (rc) return rc;
        if (!h->side_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
        // one workgroup on all but four CUs, each with (nearly) the whole LDS: nothing that needs LDS fits beside
        // it, and a persistent launch of more than a handful of workgroups finds only SOME of them resident
        // ... once they are ON the CUs: a launch on another stream is not ordered against what the caller launches
        // next, and a training launch that overtook this kernel met an empty chip (the not-resident test failed once in
        // five full runs that way).  The workgroups count themselves in a pinned host word; this call returns when all
        // have started (or after 0.2 s: a chip too busy to take them is occupied enough).
        if (!h->occupy_started) HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&h->occupy_started), sizeof(unsigned), hipHostMallocDefault));
        HIPCHK(h, hipStreamSynchronize(h->side_stream));  // (an earlier occupation has ended: the word is ours)
        *h->occupy_started = 0u;
        const int wgs = std::max(1, h->n_cu - 4);
        HIPCHK(h, launch_occupy(wgs, 160 * 1024 - 1024, (unsigned long long)milliseconds * 100000ull, h->occupy_started, h->side_stream));
        const auto t0 = std::chrono::steady_clock::now();
        while (__atomic_load_n(h->occupy_started, __ATOMIC_ACQUIRE) < (unsigned)wgs &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(200))
            std::this_thread::yield();
        return MFSGD_OK;
    });
}

int mfsgd_debug_round_stamps(mfsgd_handle* h, int32_t part, int32_t round, uint64_t* out) {
    return guarded(h, "debug_round_stamps", [&]() -> int {
        if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_round_stamps: null argument");
        if (h->n_parts != 1 || part != 0) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_round_stamps: single-partition handles only");
        int rc = check_has_q(h, "debug_round_stamps");
        if (rc || (rc = prepare_compute(h))) return rc;
        Part& p = h->parts[0];
        if (round < 0 || round >= p.sched.B) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_round_stamps: bad round");
        const size_t words = (size_t)p.sched.B * (6 + (size_t)p.sched.W * p.sched.W * 4);
        if (words * sizeof(uint64_t) > p.d_sse_partial.bytes()) {
            int rc2 = dev_alloc(h, p.d_sse_partial, words * sizeof(uint64_t));
            if (rc2) return rc2;
        }
        CellLaunch a = make_launch(h, p, h->dQ.data());
        a.rd = round;
        a.diag = true;
        HIPCHK(h, hipMemsetAsync(p.d_sse_partial.get(), 0, words * sizeof(uint64_t), h->stream));
        a.sse_partial = p.d_sse_partial.as<double>();
        HIPCHK(h, launch_cell(true, h->geo.L, p.sched.W, a, h->stream));
        HIPCHK(h, hipMemcpyAsync(out, p.d_sse_partial.get(), words * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

}  // extern "C"
