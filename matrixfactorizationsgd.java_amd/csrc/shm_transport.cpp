// shm_transport.cpp -- the DSGD ring's rehearsal transport (transport.hpp): blocks staged through POSIX shared memory.
// NOT in the product library: linked into lib/libmfsgd_rehearsal.so only, which the multi-process tests and bench.py
// --rehearse-on-one-gpu load through MFSGD_LIBRARY.  libmfsgd.so moves blocks with RCCL or not at all.
// RCCL cannot put two ranks on one GPU, and a host without RCCL has no ring at all.  With MFSGD_DSGD_TRANSPORT=shm
// mfsgd_dsgd_unique_id() hands out the name of a shared-memory segment instead of an RCCL id, and a ring created from
// such an id moves its blocks device -> segment -> device with blocking copies and sequence counters.  Same ring, same
// order of events, no xGMI: it exists so that the multi-rank logic of dsgd.cpp (groups, slots, double buffering, event
// ordering, the RMSE reduction) runs -- and is tested -- with several REAL processes on one GPU.  Not a performance path.
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>

#include "transport.hpp"

namespace {

using mfsgd::transport_fail;

constexpr int kShmMaxWorld = 16, kShmMaxSlots = 64;
struct ShmHeader {
    std::atomic<uint32_t> ready[kShmMaxWorld];
    std::atomic<uint64_t> written[kShmMaxWorld][kShmMaxSlots];  // channel (rank -> rank - 1, slot): blocks written
    std::atomic<uint64_t> taken[kShmMaxWorld][kShmMaxSlots];    // ... and taken by the receiver
    std::atomic<uint64_t> ar_seq[kShmMaxWorld], ar_done[kShmMaxWorld];
    double ar_val[kShmMaxWorld][2];
};
constexpr size_t kShmDataOffset = (sizeof(ShmHeader) + 4095) & ~(size_t)4095;

template <class Pred>
bool spin_until(Pred ok, double seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned n = 0; !ok(); ++n) {
        if ((n & 1023u) == 1023u) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
            std::this_thread::yield();
        }
    }
    return true;
}

struct ShmRing final : mfsgd::Transport {
    std::string name;
    int fd = -1;
    unsigned char* base = nullptr;
    size_t bytes = 0, slot_bytes = 0;
    int rank = 0, world = 1, m = 1;
    uint64_t ar_round = 0;
    hipStream_t wire = nullptr;
    ShmHeader* hdr() const { return reinterpret_cast<ShmHeader*>(base); }
    unsigned char* slot(int r, int j) const { return base + kShmDataOffset + ((size_t)r * m + j) * slot_bytes; }

    ~ShmRing() override {
        if (base) (void)munmap(base, bytes);
        if (fd >= 0) (void)close(fd);
        if (rank == 0 && !name.empty()) (void)shm_unlink(name.c_str());  // rank 0 unlinks the segment
    }

    int bring_up(const void* id, int rank_, int world_, int slots, size_t count, hipStream_t wire_, double*, std::string& err) override {
        if (slots > kShmMaxSlots) return transport_fail(err, MFSGD_ERR_UNSUPPORTED, "dsgd_create (shm transport): at most 64 partitions per rank");
        name.assign(static_cast<const char*>(id) + 8, strnlen(static_cast<const char*>(id) + 8, MFSGD_DSGD_ID_BYTES - 9));
        rank = rank_;
        world = world_;
        m = slots;
        wire = wire_;
        slot_bytes = count * sizeof(float);
        bytes = kShmDataOffset + (size_t)world * m * slot_bytes;
        fd = shm_open(name.c_str(), O_CREAT | O_RDWR, 0600);
        if (fd < 0 || ftruncate(fd, (off_t)bytes) != 0)
            return transport_fail(err, MFSGD_ERR_OOM, "dsgd_create (shm transport): cannot create " + name);
        void* mp = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        if (mp == MAP_FAILED) return transport_fail(err, MFSGD_ERR_OOM, "dsgd_create (shm transport): cannot map " + name);
        base = static_cast<unsigned char*>(mp);  // a fresh segment is all zeros: every counter starts at 0
        ShmHeader* H = hdr();
        H->ready[rank].store(1, std::memory_order_release);
        if (!spin_until([&] {
                for (int x = 0; x < world; ++x)
                    if (H->ready[x].load(std::memory_order_acquire) == 0) return false;
                return true;
            }, 120.0))
            return transport_fail(err, MFSGD_ERR_HIP, "dsgd_create (shm transport): not every rank arrived");
        return MFSGD_OK;
    }

    // the same shift with blocking copies through shared memory
    int shift(int j, const float* send, float* recv, hipEvent_t trained, hipEvent_t arrived, std::string& err) override {
        ShmHeader* H = hdr();
        const int src = (rank + 1) % world;
        TRANSPORT_HIP(err, hipEventSynchronize(trained));
        auto& wr = H->written[rank][j];
        auto& tk = H->taken[rank][j];
        if (!spin_until([&] { return tk.load(std::memory_order_acquire) == wr.load(std::memory_order_relaxed); }, 120.0))
            return transport_fail(err, MFSGD_ERR_HIP, "dsgd (shm transport): rank " + std::to_string((rank + world - 1) % world) + " never took the last block");
        TRANSPORT_HIP(err, hipMemcpy(slot(rank, j), send, slot_bytes, hipMemcpyDeviceToHost));
        bytes_sent += (int64_t)slot_bytes;
        wr.store(wr.load(std::memory_order_relaxed) + 1, std::memory_order_release);
        auto& swr = H->written[src][j];
        auto& stk = H->taken[src][j];
        if (!spin_until([&] { return swr.load(std::memory_order_acquire) > stk.load(std::memory_order_relaxed); }, 120.0))
            return transport_fail(err, MFSGD_ERR_HIP, "dsgd (shm transport): rank " + std::to_string(src) + " never sent its block");
        TRANSPORT_HIP(err, hipMemcpy(recv, slot(src, j), slot_bytes, hipMemcpyHostToDevice));
        stk.store(stk.load(std::memory_order_relaxed) + 1, std::memory_order_release);
        TRANSPORT_HIP(err, hipEventRecord(arrived, wire));
        return MFSGD_OK;
    }

    int allreduce2(double* v, bool max, std::string& err) override {
        ShmHeader* H = hdr();
        const uint64_t q = ++ar_round;
        auto all_at = [&](std::atomic<uint64_t>* seq, uint64_t least) {
            return spin_until([&] {
                for (int x = 0; x < world; ++x)
                    if (seq[x].load(std::memory_order_acquire) < least) return false;
                return true;
            }, 120.0);
        };
        // nobody may still be reading the previous round's values
        if (!all_at(H->ar_done, q - 1)) return transport_fail(err, MFSGD_ERR_HIP, "dsgd (shm transport): all-reduce, a rank is missing");
        H->ar_val[rank][0] = v[0];
        H->ar_val[rank][1] = v[1];
        H->ar_seq[rank].store(q, std::memory_order_release);
        if (!all_at(H->ar_seq, q)) return transport_fail(err, MFSGD_ERR_HIP, "dsgd (shm transport): all-reduce, a rank is missing");
        double a = H->ar_val[0][0], b = H->ar_val[0][1];
        for (int x = 1; x < world; ++x) {  // rank order: every rank gets the same bits
            a = max ? std::max(a, H->ar_val[x][0]) : a + H->ar_val[x][0];
            b = max ? std::max(b, H->ar_val[x][1]) : b + H->ar_val[x][1];
        }
        v[0] = a;
        v[1] = b;
        H->ar_done[rank].store(q, std::memory_order_release);
        return MFSGD_OK;
    }
};

}  // namespace

namespace mfsgd {

// the id is the magic and the name of a shared-memory segment
void shm_unique_id(void* id_out) {
    std::memset(id_out, 0, MFSGD_DSGD_ID_BYTES);
    std::memcpy(id_out, kShmMagic, sizeof kShmMagic);
    const auto now = std::chrono::steady_clock::now().time_since_epoch().count();
    std::snprintf(static_cast<char*>(id_out) + 8, MFSGD_DSGD_ID_BYTES - 8, "/mfsgd_%d_%llx", (int)getpid(), (unsigned long long)now);
}

std::unique_ptr<Transport> shm_transport(int world, std::string& err) {
    if (world <= kShmMaxWorld) return std::make_unique<ShmRing>();
    err = "dsgd (shm transport): at most 16 ranks";
    return nullptr;
}

}  // namespace mfsgd
