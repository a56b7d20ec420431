// train.cpp -- epochs: the launch paths (one launch per round, the persistent kernel, the captured graph), the
// persistent kernel's recovery protocol, the training calls, lr / lambda on a live handle, the held-out set with its
// RMSE and early stopping on it, online updates of the live factors (their dependency levels and launches), the DSGD
// partition calls and the diagnostics of the epoch kernel.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "handle.hpp"

namespace mfsgd {

static CellLaunch make_launch(const mfsgd_handle* h, const Part& p, float* Q) {
    CellLaunch a{};
    a.P = p.swapped ? Q : h->dP.as<float>();
    a.Q = p.swapped ? h->dP.as<float>() : Q;
    a.cells = p.d_cells.as<const CellDesc>();
    a.rows = p.d_rows.as<const uint32_t>();
    a.subs = p.d_subs.as<const SubDesc>();
    a.entries = p.d_entries.as<const Entry>();
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
        HIPCHK(h, launch_epoch_persistent(h->geo.L, p.sched.W, a, p.sched.B, p.d_sync.as<unsigned>(), abort_word(p), st));
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
    const auto key = std::make_pair((const void*)h->dP.get(), (const void*)Q);
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
    HIPCHK(h, launch_reduce_sse(a.sse_partial, (int64_t)a.grid, p.d_sse_out.as<double>(), st));
    return MFSGD_OK;
}

static int part_sse_sync(mfsgd_handle* h, Part& p, const float* Q, hipStream_t st, double* sse) {
    if (p.sched.nnz == 0) {
        *sse = 0.0;
        return MFSGD_OK;
    }
    int rc = launch_sse(h, p, Q, st);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(sse, p.d_sse_out.get(), sizeof(double), hipMemcpyDeviceToHost, st));
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
        std::vector<DevBuf> temps;  // descriptors of a part that is not on the device yet; freed before this returns
        bool launched = false;
        for (Part& p : h->parts) {
            Schedule& s = p.sched;
            Entry* d_entries = p.on_device ? p.d_entries.as<Entry>() : s.dev.entries.as<Entry>();
            if (!d_entries || s.n_entry_recs == 0 || s.cells.empty()) continue;
            const CellDesc* d_cells = p.d_cells.as<const CellDesc>();
            const SubDesc* d_subs = p.on_device ? p.d_subs.as<const SubDesc>() : s.dev.subs.as<const SubDesc>();
            if (!p.on_device) {  // the device packer's buffers, not adopted yet: the descriptors are still on the host only
                temps.emplace_back();
                if (const int rc = upload(h, temps.back(), s.cells)) return broken(rc, "the chunk descriptors did not reach the device: " + h->err);
                d_cells = temps.back().as<const CellDesc>();
                if (!d_subs) {
                    temps.emplace_back();
                    if (const int rc = upload(h, temps.back(), s.subs)) return broken(rc, "the sub-cell tables did not reach the device: " + h->err);
                    d_subs = temps.back().as<const SubDesc>();
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
    float* Q = h->dQ.as<float>();
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
    for (int64_t j = 0; j < n; ++j)
        if (u[j] < 0 || u[j] >= h->cfg.n_users || i[j] < 0 || i[j] >= h->cfg.n_items)
            return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": pair " + std::to_string(j) + " out of range");
    return MFSGD_OK;
}

// What every call that reads the factors asks before it asks for a device.
static int check_reads_factors(const mfsgd_handle* h, const char* call) {
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, std::string(call) + ": single-partition handles only");
    if (h->where == mfsgd_handle::Where::None) return fail(h, MFSGD_ERR_STATE, std::string(call) + ": factors not initialised");
    return check_has_q(h, call);
}

// The scratch of launch_pairs_sse: its partials, then the sum.
static int alloc_pairs_scratch(mfsgd_handle* h, DevBuf& b) { return dev_alloc(h, b, sizeof(double) * ((size_t)kPairsSlots + 1)); }

// SSE of n >= 1 pairs that are on the device, under the handle's factors (P is always the users' matrix, whichever
// side of the kernels the schedule gave it: as mfsgd_predict reads it), on the handle's stream; waits for it.
static int pairs_sse_sync(mfsgd_handle* h, const char* call, const DevBuf& du, const DevBuf& di, const DevBuf& dr, int64_t n,
                          const DevBuf& scratch, double* sse) {
    const std::string prefix = std::string(call) + ": ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    double* partial = scratch.as<double>();
    HIPCHK_OR(bad, launch_pairs_sse(h->geo.L, h->dP.as<const float>(), h->dQ.as<const float>(), du.as<const int32_t>(),
                                    di.as<const int32_t>(), dr.as<const float>(), n, partial, partial + kPairsSlots, h->stream));
    HIPCHK_OR(bad, hipMemcpyAsync(sse, partial + kPairsSlots, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// The handle's held-out set on the device (the device is there: the caller has asked for it); the host copy goes.
static int validation_to_device(mfsgd_handle* h) {
    Validation& v = h->val;
    if (v.on_device || v.n == 0) return MFSGD_OK;
    int rc;
    if ((rc = upload(h, v.du, v.hu)) || (rc = upload(h, v.di, v.hi)) || (rc = upload(h, v.dr, v.hr)) ||
        (rc = alloc_pairs_scratch(h, v.d_sse))) {
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
    const Validation& v = h->val;
    return pairs_sse_sync(h, call, v.du, v.di, v.dr, v.n, v.d_sse, sse);
}

// Online updates ("Online updates") ----------------------------------------------
// Ratings of one piece: the pieces of a list are consecutive and applied one after the other, so the levels are those of
// a piece, and the device buffers of a call are sized by one.  (include/mfsgd.h states the size.)
constexpr int64_t kOnlinePiece = (int64_t)1 << 20;
// Consecutive narrow levels one workgroup walks in one launch: bounds the time a single launch runs.
constexpr int32_t kOnlineRun = 1 << 16;

static int check_online_pairs(const mfsgd_handle* h, const char* call, const int32_t* u, const int32_t* i, int64_t n) {
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": n is negative");
    if (n > 0 && (!u || !i)) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": u or i is null");
    for (int64_t j = 0; j < n; ++j)
        if (u[j] < 0 || u[j] >= h->cfg.n_users || i[j] < 0 || i[j] >= h->cfg.n_items)
            return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": rating " + std::to_string(j) + " out of range");
    return MFSGD_OK;
}

// level[j] of the n ratings of one piece (every index in range), and how many levels there are: one pass, and a second
// one that puts the handle's two "last level" arrays back to zero -- O(n), whatever n_users and n_items are.
static int32_t online_levels_of(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n, int32_t* level) {
    if (h->online_last_u.empty()) h->online_last_u.assign((size_t)h->cfg.n_users, 0);
    if (h->online_last_i.empty()) h->online_last_i.assign((size_t)h->cfg.n_items, 0);
    int32_t* lu = h->online_last_u.data();
    int32_t* li = h->online_last_i.data();
    int32_t n_levels = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int32_t l = std::max(lu[u[j]], li[i[j]]);
        level[j] = l;
        lu[u[j]] = li[i[j]] = l + 1;
        n_levels = std::max(n_levels, l + 1);
    }
    for (int64_t j = 0; j < n; ++j) lu[u[j]] = li[i[j]] = 0;
    return n_levels;
}

// One piece ready for the device: its ratings in a stable counting sort by level.
struct OnlinePiece {
    std::vector<int32_t> level, level_ptr, u, i, orig;
    std::vector<float> r;
    int32_t n_levels = 0;
};

static void online_sort_piece(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n, OnlinePiece& pc) {
    pc.level.resize((size_t)n);
    pc.u.resize((size_t)n), pc.i.resize((size_t)n), pc.orig.resize((size_t)n), pc.r.resize((size_t)n);
    pc.n_levels = online_levels_of(h, u, i, n, pc.level.data());
    pc.level_ptr.assign((size_t)pc.n_levels + 1, 0);
    for (int64_t j = 0; j < n; ++j) ++pc.level_ptr[(size_t)pc.level[(size_t)j] + 1];
    for (int32_t l = 0; l < pc.n_levels; ++l) pc.level_ptr[(size_t)l + 1] += pc.level_ptr[(size_t)l];
    std::vector<int32_t> next(pc.level_ptr.begin(), pc.level_ptr.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
        const int32_t at = next[(size_t)pc.level[(size_t)j]]++;
        pc.u[(size_t)at] = u[j];
        pc.i[(size_t)at] = i[j];
        pc.r[(size_t)at] = canon_nan(r[j]);  // (records.hpp: a payload must not reach P and Q)
        pc.orig[(size_t)at] = (int32_t)j;
    }
}

static void online_count(mfsgd_online_info* info, const int32_t* level_ptr, int32_t n_levels) {
    info->pieces += 1;
    info->levels += n_levels;
    for (int32_t l = 0; l < n_levels; ++l) info->max_width = std::max<int64_t>(info->max_width, level_ptr[l + 1] - level_ptr[l]);
}

// The launches of one piece that is on the device.  A wide level (more ratings than one pass of one workgroup holds) is a
// launch of its own, of as many workgroups as it has passes: stream order is the barrier before and behind it.  A run of
// consecutive narrow levels is ONE launch of ONE workgroup, which walks them (online.hip).  (Narrow is one pass, not a few:
// calling levels of up to 4, 8 or 16 passes narrow saved launches and no time on the bench workload, 32 passes cost four
// times the time -- DESIGN.md, "Online updates".)
template <class Launch>
static hipError_t online_launches(const std::vector<int32_t>& level_ptr, int32_t n_levels, int L, int64_t* launches, Launch&& launch) {
    const int32_t gpb = 256 / L;
    for (int32_t l = 0; l < n_levels;) {
        const int32_t width = level_ptr[(size_t)l + 1] - level_ptr[(size_t)l];
        int32_t l1 = l + 1, wgs = 1;
        if (width > gpb) {
            wgs = (width + gpb - 1) / gpb;
        } else {
            while (l1 < n_levels && l1 - l < kOnlineRun && level_ptr[(size_t)l1 + 1] - level_ptr[(size_t)l1] <= gpb) ++l1;
        }
        const hipError_t e = launch(l, l1, wgs);
        if (e != hipSuccess) return e;
        ++*launches;
        l = l1;
    }
    return hipSuccess;
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
        float* Q = h->dQ.as<float>();
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
        float* Q = h->dQ.as<float>();
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
        return rmse_of(h, h->parts[0], h->dQ.as<const float>(), out);
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
        DevBuf du, di, dr, scratch;
        if ((rc = dev_alloc(h, du, sizeof(int32_t) * (size_t)piece))) return rc;
        if ((rc = dev_alloc(h, di, sizeof(int32_t) * (size_t)piece))) return rc;
        if ((rc = dev_alloc(h, dr, sizeof(float) * (size_t)piece))) return rc;
        if ((rc = alloc_pairs_scratch(h, scratch))) return rc;
        double total = 0.0;
        for (int64_t j0 = 0; j0 < n; j0 += piece) {
            const int64_t c = std::min(piece, n - j0);
            double s = 0.0;
            HIPCHK_OR(bad, hipMemcpyAsync(du.get(), u + j0, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(di.get(), i + j0, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(dr.get(), r + j0, sizeof(float) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            if ((rc = pairs_sse_sync(h, "rmse_pairs", du, di, dr, c, scratch, &s))) return rc;  // (the staging buffers are reused)
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
                    HIPCHK_OR(bad, hipMemcpyAsync(snap_p.get(), h->dP.get(), h->p_bytes(), hipMemcpyDeviceToDevice, h->stream));
                    HIPCHK_OR(bad, hipMemcpyAsync(snap_q.get(), h->dQ.get(), h->q_bytes(), hipMemcpyDeviceToDevice, h->stream));
                }
            } else if (++bad_epochs >= patience) {
                break;
            }
        }
        if (restore_best && *best_epoch >= 0 && *best_epoch != *epochs_run - 1) {
            HIPCHK_OR(bad, hipMemcpyAsync(h->dP.get(), snap_p.get(), h->p_bytes(), hipMemcpyDeviceToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(h->dQ.get(), snap_q.get(), h->q_bytes(), hipMemcpyDeviceToDevice, h->stream));
        }
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the snapshot is freed behind this
        return MFSGD_OK;
    });
}

int mfsgd_online_levels(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n, int32_t* level, mfsgd_online_info* info) {
    return guarded(h, "online_levels", [&]() -> int {
        if (const int rc = check_online_pairs(h, "online_levels", u, i, n)) return rc;
        mfsgd_online_info got{};
        got.n = n;
        std::vector<int32_t> own, count;
        if (!level && n > 0) own.resize((size_t)std::min(n, kOnlinePiece));
        for (int64_t j0 = 0; j0 < n; j0 += kOnlinePiece) {
            const int64_t c = std::min(kOnlinePiece, n - j0);
            int32_t* lv = level ? level + j0 : own.data();
            const int32_t n_levels = online_levels_of(h, u + j0, i + j0, c, lv);
            count.assign((size_t)n_levels + 1, 0);  // (as a level_ptr: entry l + 1 counts level l)
            for (int64_t j = 0; j < c; ++j) ++count[(size_t)lv[j] + 1];
            for (int32_t l = 0; l < n_levels; ++l) count[(size_t)l + 1] += count[(size_t)l];
            online_count(&got, count.data(), n_levels);
        }
        if (info) *info = got;
        return MFSGD_OK;
    });
}

int mfsgd_apply_ratings(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n, float* err,
                        mfsgd_online_info* info) {
    return guarded(h, "apply_ratings", [&]() -> int {
        int rc = check_online_pairs(h, "apply_ratings", u, i, n);
        if (rc) return rc;
        if (n > 0 && !r) return fail(h, MFSGD_ERR_INVALID_ARG, "apply_ratings: r is null");
        if ((rc = check_reads_factors(h, "apply_ratings"))) return rc;
        mfsgd_online_info got{};
        got.n = n;
        if (n == 0) {
            if (info) *info = got;
            return MFSGD_OK;
        }
        if ((rc = factors_to_device(h))) return rc;
        auto bad = [h](hipError_t e) { return serve_fail(h, "apply_ratings: ", e); };
        const size_t piece = (size_t)std::min(n, kOnlinePiece);
        DevBuf du, di, dr, dorig, dptr, derr;  // sized by the largest piece; gone when this returns, whichever way
        if ((rc = dev_alloc(h, du, sizeof(int32_t) * piece))) return rc;
        if ((rc = dev_alloc(h, di, sizeof(int32_t) * piece))) return rc;
        if ((rc = dev_alloc(h, dr, sizeof(float) * piece))) return rc;
        if ((rc = dev_alloc(h, dorig, sizeof(int32_t) * piece))) return rc;
        if ((rc = dev_alloc(h, dptr, sizeof(int32_t) * (piece + 1)))) return rc;
        if (err && (rc = dev_alloc(h, derr, sizeof(float) * piece))) return rc;
        const float lr = h->cfg.lr, c1 = 1.0f - h->cfg.lr * h->cfg.lambda;
        OnlinePiece pc;
        for (int64_t j0 = 0; j0 < n; j0 += kOnlinePiece) {
            const int64_t c = std::min(kOnlinePiece, n - j0);
            online_sort_piece(h, u + j0, i + j0, r + j0, c, pc);
            online_count(&got, pc.level_ptr.data(), pc.n_levels);
            HIPCHK_OR(bad, hipMemcpyAsync(du.get(), pc.u.data(), sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(di.get(), pc.i.data(), sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(dr.get(), pc.r.data(), sizeof(float) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(dorig.get(), pc.orig.data(), sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, hipMemcpyAsync(dptr.get(), pc.level_ptr.data(), sizeof(int32_t) * ((size_t)pc.n_levels + 1),
                                          hipMemcpyHostToDevice, h->stream));
            HIPCHK_OR(bad, online_launches(pc.level_ptr, pc.n_levels, h->geo.L, &got.launches, [&](int32_t l0, int32_t l1, int32_t wgs) {
                return launch_apply_levels(h->geo.L, h->dP.as<float>(), h->dQ.as<float>(), du.as<const int32_t>(),
                                           di.as<const int32_t>(), dr.as<const float>(), dorig.as<const int32_t>(),
                                           dptr.as<const int32_t>(), l0, l1, wgs, h->cfg.k, lr, c1, err ? derr.as<float>() : nullptr,
                                           h->stream);
            }));
            if (err) HIPCHK_OR(bad, hipMemcpyAsync(err + j0, derr.get(), sizeof(float) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
            HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the staging buffers, the host's and the device's, are reused
        }
        if (info) *info = got;
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
        CellLaunch a = make_launch(h, p, h->dQ.as<float>());
        a.grid = p.persistent_np;
        a.diag = true;
        a.sse_partial = p.d_sse_partial.as<double>();
        HIPCHK(h, hipMemsetAsync(p.d_sse_partial.get(), 0, words * sizeof(uint64_t), h->stream));
        HIPCHK(h, launch_epoch_persistent(h->geo.L, p.sched.W, a, p.sched.B, p.d_sync.as<unsigned>(), abort_word(p), h->stream));
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
        CellLaunch a = make_launch(h, p, h->dQ.as<float>());
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
