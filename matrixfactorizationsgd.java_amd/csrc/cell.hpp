// cell.hpp -- device side only: everything one workgroup does with one cell of the block schedule.
//
// Shape of the work: one workgroup = one cell.  The cell's touched factor rows (users AND
// items) are gathered from HBM/L2 into LDS with 16-byte-per-lane loads (one row = L lanes x 16 B, a wave moves 64/L
// rows per instruction), every rating of the cell is then applied out of LDS, and the rows are scattered back.  A
// rating occupies a group of L lanes (4 floats per lane); a wave applies G = 64/L ratings per step; the dot product is
// reduced inside the lane group with DPP row operations (no LDS traffic, no MFMA: this is gather + axpy, not a dense
// contraction).
//
// Included by the units that run cells: epoch.hip (the persistent ring) and cells.hip (one launch per round, the
// RMSE passes).  Arithmetic is the contract of DESIGN.md section 3 and must stay bit-for-bit what the CPU checker
// under oracle/ computes: those units are built with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "records.hpp"
#include "run_asm.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Workgroup barrier that waits for this wave's LDS traffic only.  __syncthreads() would also
// drain the vector-memory counter, i.e. any LDS-DMA prefetch still in flight.
__device__ __forceinline__ void wg_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

using gptr_t = const __attribute__((address_space(1))) void*;
using lptr_t = __attribute__((address_space(3))) void*;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float4 lds_ld(const unsigned char* base, unsigned off) {
    return *reinterpret_cast<const float4*>(base + off);
}
__device__ __forceinline__ void lds_st(unsigned char* base, unsigned off, const float4 v) {
    *reinterpret_cast<float4*>(base + off) = v;
}

// (the hand-scheduled run loop text lives in run_asm.hpp, shared with tools/ubench3.hip)
template <int EST, int L>
__device__ __forceinline__ void run_loop_asm(float4& rq, const unsigned ea, const unsigned rowbase, int pairs,
                                             const float lr) {
    static_assert(L == 16 || L == 32 || L == 64, "hand-scheduled run loop: 16, 32 or 64 lanes per rating");
    using f4 = __attribute__((ext_vector_type(4))) float;
    f4 q = {rq.x, rq.y, rq.z, rq.w};
    uint64_t live, sv;  // the lanes of the step's live slots / the wave's exec mask (scalar temporaries of the text)
    constexpr int PADV = mfsgd_pad_run(L);
    if constexpr (L == 16)
        asm volatile(MFSGD_RUN_LOOP_ASM_TEXT("", MFSGD_SFMA_V) MFSGD_RUN_LOOP_ASM_OPERANDS);
    else if constexpr (L == 32)
        asm volatile(MFSGD_RUN_LOOP_ASM_TEXT(MFSGD_SWAP_ADD16, MFSGD_SFMA_V) MFSGD_RUN_LOOP_ASM_OPERANDS);
    else
        asm volatile(MFSGD_RUN_LOOP_ASM_TEXT(MFSGD_BCAST_ADD64, MFSGD_SFMA_S) MFSGD_RUN_LOOP_ASM_OPERANDS);
    rq = make_float4(q[0], q[1], q[2], q[3]);
}

// ---- general steps (run_asm.hpp, MFSGD_GEN_LOOP_ASM_TEXT) ---------------------------------
// `ea`: LDS byte address of this lane group's entry of step 0 (stride EST), n >= 1 steps, c2 = {c, c}.
template <int EST, int L>
__device__ __forceinline__ void gen_loop_asm(const unsigned ea, const unsigned rowbase, int n, const float lr, const uint64_t c2) {
    static_assert(L == 16 || L == 32 || L == 64, "hand-scheduled general loop: 16, 32 or 64 lanes per rating");
    n = __builtin_amdgcn_readfirstlane(n);
    constexpr int PADV = mfsgd_pad_gen(L);
    if constexpr (L == 16)
        asm volatile(MFSGD_GEN_LOOP_ASM_TEXT("", MFSGD_SFMA_V) MFSGD_GEN_LOOP_ASM_OPERANDS);
    else if constexpr (L == 32)
        asm volatile(MFSGD_GEN_LOOP_ASM_TEXT(MFSGD_SWAP_ADD16, MFSGD_SFMA_V) MFSGD_GEN_LOOP_ASM_OPERANDS);
    else
        asm volatile(MFSGD_GEN_LOOP_ASM_TEXT(MFSGD_BCAST_ADD64, MFSGD_SFMA_S) MFSGD_GEN_LOOP_ASM_OPERANDS);
}

// ---- solo run: chain wave / helper wave (run_asm.hpp) -------------------------------------
// `ea`: LDS byte address of the run's header record, `s0`: that record's slots word (p row of step 0 | q row << 16),
// `rowbase`: LDS byte address of row slot 0 plus this lane's 16-byte offset inside a row, n >= 1 steps, c2 = {c, c}
// as one 64-bit scalar.  The loop loads the q row itself (next to its first p row and entry words).
template <int L>
__device__ __forceinline__ void solo_chain_asm(float4& rq, const unsigned ea, const unsigned s0, const unsigned rowbase, int n,
                                               const float lr, const uint64_t c2) {
    static_assert(L == 16 || L == 32 || L == 64, "solo loops: 16, 32 or 64 lanes per rating");
    using f4 = __attribute__((ext_vector_type(4))) float;
    f4 q;
    n = __builtin_amdgcn_readfirstlane(n);
    constexpr int PADV = mfsgd_pad_chain_tail(L), PADS = mfsgd_pad_chain_steady(L);  // the loop's two heads
    if constexpr (L == 16)
        asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT("", MFSGD_SFMA2_V) MFSGD_SOLO_CHAIN_OPERANDS);
    else if constexpr (L == 32)
        asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT(MFSGD_BCAST_ADD32, MFSGD_SFMA2_S) MFSGD_SOLO_CHAIN_OPERANDS);
    else
        asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT(MFSGD_BCAST_ADD64, MFSGD_SFMA2_S) MFSGD_SOLO_CHAIN_OPERANDS);
    rq = make_float4(q[0], q[1], q[2], q[3]);  // q after the n steps (the helper stores it; the caller needs it when it cuts a run)
}
// Returns false if it gave up waiting for the chain wave (bounded polling; cannot happen with a
// schedule the packer built -- the bound only keeps a corrupt one from hanging the GPU).
template <int L>
__device__ __forceinline__ bool solo_helper_asm(const unsigned ea, const unsigned rowbase, int n, const uint64_t c2,
                                                int fin = 1) {  // fin = 0: do not store q at the end (ubench3's cut runs)
    constexpr int PADV = mfsgd_pad_helper(L);
    n = __builtin_amdgcn_readfirstlane(n);  // (workgroup-uniform by construction; the compiler cannot always see it)
    fin = __builtin_amdgcn_readfirstlane(fin);
    asm volatile("" : "+s"(fin));  // a register, not an immediate, in the text below
    int spins = 1 << 22;
    asm volatile(MFSGD_SOLO_HELPER_ASM_TEXT MFSGD_SOLO_HELPER_OPERANDS);
    return spins != 0;
}

// The chain wave of a lone-tile cell (run_asm.hpp, MFSGD_LONE_CHAIN_ASM_TEXT): sets the run up, takes the row from its
// mailbox `src` (tag `want`), joins ONE workgroup barrier, runs the n steps and posts the row to `dst` (tag `ptag`, lanes
// of the mask `pm`).  `ctl`: LDS byte address of the control block ([0] abort broadcast, [1] arrival stamp when `prof`).
// Returns false if it gave up waiting (abort word and ctl[0] raised, barrier joined, nothing trained or posted).
template <int L>
__device__ __forceinline__ bool lone_chain_asm(const unsigned ea, const unsigned s0, const unsigned rowbase, int n, const float lr,
                                               const uint64_t c2, const __attribute__((address_space(1))) unsigned long long* src,
                                               unsigned want, const __attribute__((address_space(1))) unsigned* abw,
                                               const unsigned ctl, __attribute__((address_space(1))) unsigned long long* dst,
                                               unsigned ptag, uint64_t pm, unsigned prof) {
    static_assert(L == 16 || L == 32 || L == 64, "solo loops: 16, 32 or 64 lanes per rating");
    // (workgroup-uniform by construction; the compiler cannot always see it, and the text wants scalar registers)
    n = __builtin_amdgcn_readfirstlane(n);
    pm = (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)pm) |
         (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(pm >> 32)) << 32;
    want = (unsigned)__builtin_amdgcn_readfirstlane((int)want);
    ptag = (unsigned)__builtin_amdgcn_readfirstlane((int)ptag);
    prof = (unsigned)__builtin_amdgcn_readfirstlane((int)prof);
    unsigned spins = 0, gave = 0, t0;
    uint64_t tmp;
    constexpr int PADV = mfsgd_pad_chain_tail(L), PADS = mfsgd_pad_chain_steady(L);  // the same heads at the same places
    if constexpr (L == 16)
        asm volatile(MFSGD_LONE_CHAIN_ASM_TEXT("", MFSGD_SFMA2_V) MFSGD_LONE_CHAIN_OPERANDS);
    else if constexpr (L == 32)
        asm volatile(MFSGD_LONE_CHAIN_ASM_TEXT(MFSGD_BCAST_ADD32, MFSGD_SFMA2_S) MFSGD_LONE_CHAIN_OPERANDS);
    else
        asm volatile(MFSGD_LONE_CHAIN_ASM_TEXT(MFSGD_BCAST_ADD64, MFSGD_SFMA2_S) MFSGD_LONE_CHAIN_OPERANDS);
    return gave == 0;
}

// copy waves of the persistent training kernel: as many again as apply waves, up to 8 waves in all
// (16 waves would leave each only 128 VGPRs; the assembly loops use fixed registers up to v159 -- the lone-tile chain
// text of run_asm.hpp -- and the persistent kernel comes to 175-178 VGPRs)
template <int L, int W>
constexpr int epoch_helpers() {
    return W <= 4 ? W : 0;
}

// A chunk descriptor through the scalar path: the index is the same in every lane (it comes from
// workgroup-uniform counters and from descriptors loaded this way), which the compiler cannot see
// once it has been through memory -- pin it to an SGPR so that the load is an s_load and the
// descriptor lives in SGPRs (it is live across the rating loops, where VGPRs are scarce).
__device__ __forceinline__ CellDesc load_desc(const CellDesc* __restrict__ cells, unsigned idx) {
    idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
    asm volatile("" : "+s"(idx));
    return cells[idx];
}

// Everything one workgroup does with one cell, phase by phase.  Shared by the
// per-round kernel, the SSE pass and the persistent epoch kernel.
//
// LDS image of a workgroup:
//   [control block 16 B][schedule buffer 0: sched_cap][schedule buffer 1: sched_cap][rows ...]
//   schedule buffer: [entries: n_steps x G x 16][subs: W*W x 8, padded to 16][row ids: nrows x 4]
//   rows: [nrows x ROWB][2G zero rows]; slots [0, nu) hold p-side (user) rows, [nu, nrows) q-side (item) rows.
// Two schedule buffers: the persistent kernel fetches the next cell's schedule (LDS-DMA)
// while the current cell is being worked on.
//
// NH copy waves (0, or W in the persistent training kernel): waves W .. W+NH-1.  They take part
// in staging, gathers and scatters like any other wave -- an LDS-DMA gather or a scatter is bound by
// how fast a wave can issue (~150 cycles per LDS-DMA instruction), so more waves shorten those
// phases -- and only keep the barriers company in apply(), whose W waves own the sub-cells.
template <int L, int W, int NH = 0>
struct Cell {
    static constexpr int G = 64 / L;
    static constexpr int ROWB = 16 * L;
    static constexpr int KP = 4 * L;
    static constexpr int NWV = W + NH;   // waves of the workgroup
    static constexpr int NT = 64 * NWV;
    static constexpr int CTL = 16;  // control block at the start of the dynamic LDS
    static constexpr int SUBB = (W * W * 8 + 15) & ~15;  // sub-cell table, padded to 16-byte units

    int tid, lane, wave, g, lig;
    int wave_all;      // index among all NWV waves (copy loops); `wave` is the sub-cell owner index
    bool helper;       // this wave is a copy wave (NH > 0 only)
    unsigned laneoff;
    int nu, nrows, n_steps;
    bool critical;  // the cell carries a long per-row chain (scheduler flag)
    volatile unsigned* fail_flag = nullptr;  // LDS control word a helper raises when it gives up (persistent kernel)
    // [r3] Early hand-off of a tile that is ONE row (run_ring's mailboxes): when the cell's last work is a solo run, the
    // chain wave posts the row from its registers the moment the run ends -- {value, tag} granules at post_at, tag
    // post_tag -- instead of leaving it to the workgroup behind the helper's stores, the sub-round barriers and an LDS
    // round trip; it says so in *posted_flag (an LDS control word), and the workgroup does not post again.
    unsigned long long* post_at = nullptr;
    unsigned post_tag = 0;
    volatile unsigned* posted_flag = nullptr;
    unsigned char* lrows;
    uint4* lent;
    uint2* lsub;
    uint32_t* lids;

    __device__ __forceinline__ void init_thread() {
        tid = threadIdx.x;
        lane = tid & 63;
        wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
        helper = NH > 0 && wave_all >= W;
        wave = helper ? wave_all - W : wave_all;
        g = lane / L;
        lig = lane % L;
        laneoff = (unsigned)lig * 16u;
    }
    __device__ __forceinline__ void bind(const CellDesc& cd, unsigned char* smem, int buf, int sched_cap) {
        nu = cd.nu;
        nrows = (int)cd.nu + (int)cd.ni;
        n_steps = (int)(cd.n_steps & 0x7FFFFFFFu);
        critical = (cd.n_steps >> 31) != 0;
        lrows = smem + CTL + 2 * (size_t)sched_cap;
        lent = reinterpret_cast<uint4*>(smem + CTL + (size_t)buf * sched_cap);
        lsub = reinterpret_cast<uint2*>(lent + (size_t)n_steps * G);
        lids = reinterpret_cast<uint32_t*>(reinterpret_cast<unsigned char*>(lsub) + SUBB);
    }

    // Zeroes the 2G rows idle step slots point at (r = 0 keeps them zero).
    __device__ __forceinline__ void zero_idle_rows() {
        for (int x = tid; x < 2 * G * L; x += NT)
            lds_st(lrows, (unsigned)(nrows * ROWB + x * 16), make_float4(0.f, 0.f, 0.f, 0.f));
    }

    // The schedule of ANOTHER cell -> schedule buffer `buf`, by LDS-DMA (no registers held,
    // nothing waited for here): entries, sub-cell table, row ids, each a contiguous copy of
    // whole 16-byte units.  The caller waits (vmcnt) and barriers before binding that buffer.
    __device__ __forceinline__ void prefetch_schedule(const CellDesc& nd, int ncell, unsigned char* smem, int buf,
                                                      int sched_cap, const uint32_t* __restrict__ rows,
                                                      const SubDesc* __restrict__ subs,
                                                      const Entry* __restrict__ entries) {
        unsigned char* const dst = smem + CTL + (size_t)buf * sched_cap;
        const int nn = (int)nd.nu + (int)nd.ni;
        const int ent_bytes = (int)(nd.n_steps & 0x7FFFFFFFu) * G * 16;
        const int sub_bytes = SUBB;
        const int ids_bytes = (nn * 4 + 15) & ~15;
        auto copy = [&](const unsigned char* src, unsigned char* d, int bytes) {
            for (int off0 = wave_all * 1024; off0 < bytes; off0 += NWV * 1024) {
                const int off = off0 + lane * 16;
                if (off < bytes)
                    __builtin_amdgcn_global_load_lds((gptr_t)(src + off), (lptr_t)(d + off0), 16, 0, 0);
            }
        };
        copy(reinterpret_cast<const unsigned char*>(entries + (size_t)nd.ent_off * G), dst, ent_bytes);
        copy(reinterpret_cast<const unsigned char*>(subs + (size_t)ncell * W * W), dst + ent_bytes, sub_bytes);
        copy(reinterpret_cast<const unsigned char*>(rows + nd.row_off), dst + ent_bytes + sub_bytes, ids_bytes);
    }

    // Row ids, step entries and the sub-cell table -> LDS; zeroes the idle rows.
    // One global latency for all of it.  Caller barriers before using any of it.
    __device__ __forceinline__ void stage_schedule(const CellDesc& cd, int cell, const uint32_t* __restrict__ rows,
                                                   const SubDesc* __restrict__ subs,
                                                   const Entry* __restrict__ entries) {
        const uint32_t* const crow = rows + cd.row_off;
        for (int x = tid; x < nrows; x += NT) lids[x] = crow[x];
        const uint4* gent = reinterpret_cast<const uint4*>(entries) + (size_t)cd.ent_off * G;
        const int ne = n_steps * G;
        for (int x = tid; x < ne; x += NT) lent[x] = gent[x];
        if (tid < W * W) lsub[tid] = reinterpret_cast<const uint2*>(subs)[(size_t)cell * W * W + tid];
        zero_idle_rows();
    }

    // Factor rows of LDS slots [lo, hi) -> LDS, straight from memory (LDS-DMA).  One
    // wave instruction moves G whole rows (64 lanes x 16 B = G x ROWB contiguous LDS
    // bytes); the source address is per lane, so it is a row gather.  Issues every
    // load of the wave back to back and does NOT wait: caller does vmcnt(0) + barrier.
    // COH: the loads carry sc1 (they bypass this CU's L1), for rows another workgroup stored write-through inside
    // the same launch -- the ring hand-off then needs no acquire fence in front of them (Guideline 16, form R1
    // with sc1 loads in place of the acquire).
    template <bool COH = false>
    __device__ __forceinline__ void gather(const float* __restrict__ P, const float* __restrict__ Q, int lo, int hi) {
        constexpr int AUX = COH ? 16 : 0;  // cache policy bits of the builtin: 16 = sc1
        constexpr int UNR = 4;  // row ids of UNR instructions are fetched before any of them is issued
        const int first = (lo / G) * G;  // keep wave instructions aligned to G-slot groups
        int s0 = first + wave_all * G;
        for (; s0 + (UNR - 1) * NWV * G < hi; s0 += UNR * NWV * G) {
            uint32_t rid[UNR];
            bool in[UNR];
#pragma unroll
            for (int x = 0; x < UNR; ++x) {
                const int sx = s0 + x * NWV * G + g;
                in[x] = sx >= lo && sx < hi;
                rid[x] = lids[in[x] ? sx : lo];
            }
#pragma unroll
            for (int x = 0; x < UNR; ++x) {
                const int sb = s0 + x * NWV * G;
                if (in[x]) {
                    const float* src = (sb + g < nu ? P : Q) + (size_t)rid[x] * KP + lig * 4;
                    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lrows + (size_t)sb * ROWB), 16, 0, AUX);
                }
            }
        }
        for (; s0 < hi; s0 += NWV * G) {
            const int sx = s0 + g;
            if (sx >= lo && sx < hi) {
                const uint32_t rid = lids[sx];
                const float* src = (sx < nu ? P : Q) + (size_t)rid * KP + lig * 4;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(lrows + (size_t)s0 * ROWB), 16, 0, AUX);
            }
        }
    }

    // LDS slots [lo, hi) -> factor rows.  WT: write-through (sc1) stores, for rows another
    // workgroup will read inside the same launch (cdna guide, Guideline 16, form R1).
    template <bool WT>
    __device__ __forceinline__ void scatter(float* __restrict__ P, float* __restrict__ Q, int lo, int hi) {
        constexpr int UNR = 4;
        auto put = [&](int s, uint32_t rid, const float4 v) {
            float* dst = (s < nu ? P : Q) + (size_t)rid * KP + lig * 4;
            if constexpr (WT) {
                const f32x4 vv = {v.x, v.y, v.z, v.w};
                // hipcc pads nothing inside asm: a VALU write of a >64-bit store operand needs a wait
                // state before the store reads it, and the operands must not be rewritten right after
                asm volatile("s_nop 1\n\tglobal_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(vv) : "memory");
            } else {
                *reinterpret_cast<float4*>(dst) = v;
            }
        };
        int s = lo + wave_all * G + g;
        for (; s + (UNR - 1) * NWV * G < hi; s += UNR * NWV * G) {
            uint32_t rid[UNR];
            float4 v[UNR];
#pragma unroll
            for (int x = 0; x < UNR; ++x) {
                rid[x] = lids[s + x * NWV * G];
                v[x] = lds_ld(lrows, (unsigned)((s + x * NWV * G) * ROWB) + laneoff);
            }
#pragma unroll
            for (int x = 0; x < UNR; ++x) put(s + x * NWV * G, rid[x], v[x]);
        }
        for (; s < hi; s += NWV * G) put(s, lids[s], lds_ld(lrows, (unsigned)(s * ROWB) + laneoff));
    }

    // ---- the lone-tile fast lane of the persistent kernel (epoch.hip, run_ring) ----------------
    // The cell's only work is ONE solo run in sub-cell 0 (workgroup-uniform; the schedule of the bound cell is in LDS):
    // no general and no run steps in front of it, its records end where the cell's steps end -- the test apply() makes
    // for the early post -- and every other sub-cell is empty.
    __device__ __forceinline__ bool lone_solo_only() const {
        if constexpr (NH > 0 && kAsmLoops && W * W <= 64) {
            const uint2 sd = lsub[lane < W * W ? lane : 0];
            const int nsolo = (int)(sd.x >> 16);
            const bool ok = lane == 0 ? (sd.x & 0xFFFFu) == 0u && sd.y == 0u && nsolo > 0 &&
                                            (nsolo + 2 + G - 1) / G + kSoloPad + 2 == n_steps
                                      : lane >= W * W || (sd.y == 0u && nsolo == 0);
            return __builtin_amdgcn_ballot_w64(!ok) == 0ull;
        } else {
            return false;
        }
    }
    // Sub-round 0 of such a cell, all waves; called behind the workgroup barrier that has the own rows and the next
    // schedule in LDS, and with the tile's row still on its way.  The chain wave (apply wave 0) takes the row from
    // `src` itself (lone_chain_asm); every other wave goes straight to the ONE barrier the chain wave joins on arrival
    // and waits THERE through the tile wait -- the helper with its run decoded, but not inside its loop, whose spin
    // bound is sized for a chain wave one step away.  Ends with the cell's W sub-round barriers, as apply() would: the
    // other sub-cells are empty (lone_solo_only), so sub-rounds 1 .. W - 1 are their barrier and nothing else.
    // Returns false, in every wave, if the chain wave gave up (ctl[0] is set): nothing was trained, posted or stored.
    __device__ __forceinline__ bool lone_round0(const float lr, const float c,
                                                const __attribute__((address_space(1))) unsigned long long* src,
                                                const unsigned want, const __attribute__((address_space(1))) unsigned* abw,
                                                volatile unsigned* ctl, const bool prof) {
        const uint4* const hdr = lent + (size_t)kSoloPad * G;  // sub-cell 0 starts at step 0 and has no other steps
        if constexpr (NH > 0 && kAsmLoops) {
            if (wave_all == 0) {
                const unsigned s0 = hdr->x;
                const int nsolo = __builtin_amdgcn_readfirstlane((int)(lsub[0].x >> 16));
                const bool post = post_at != nullptr;  // the run ends the cell (lone_solo_only): hand the row on behind it
                const uint64_t pm = !post ? 0ull : L == 64 ? ~0ull : (1ull << (L & 63)) - 1ull;  // lane group 0
                auto* dst = (__attribute__((address_space(1))) unsigned long long*)post_at + lig * 4;
                const bool ok = lone_chain_asm<L>((unsigned)(uintptr_t)(lptr_t)hdr, s0, row_base(lrows, laneoff), nsolo, lr, pack_c2(c),
                                                  src + lig * 4, want, abw, (unsigned)(uintptr_t)(lptr_t)ctl, dst, post_tag, pm,
                                                  prof ? 1u : 0u);
                if (!ok) return false;
                if (post && lane == 0) *posted_flag = 1u;
                for (int s = 0; s < W; ++s) wg_barrier();
                return true;
            }
            int ns = 0;
            const bool mine = helper && (wave + 1) % W == 0;  // apply wave 0's helper
            if (mine) ns = __builtin_amdgcn_readfirstlane((int)(lsub[0].x >> 16));
            wg_barrier();  // the chain wave has the row (or has given up)
            if (ctl[0] != 0) return false;
            if (mine && !solo_helper_asm<L>((unsigned)(uintptr_t)(lptr_t)hdr, row_base(lrows, laneoff), ns, pack_c2(c)) && fail_flag)
                *fail_flag = 1;
            for (int s = 0; s < W; ++s) wg_barrier();
        }
        return true;
    }

    // ---- apply the ratings out of LDS ------------------------------------------
    // A sub-cell's record (SubDesc), decoded -- the one definition of its layout for the sub-round loop of apply():
    // its entries are `n` general steps from step `first` of the cell's image, then `nr` run steps, then -- kSoloPad
    // idle steps further on -- the header of its `nsolo` solo records.
    struct Sub {
        int n, nr;  // general steps; run steps, stored after the general ones
        int offs;   // first entry | solo records (stored after the run steps) << 16
        __device__ __forceinline__ int first() const { return offs & 0xFFFF; }
        __device__ __forceinline__ int nsolo() const { return (int)((unsigned)offs >> 16); }
    };
    __device__ __forceinline__ Sub sub(const int x) const {
        const uint2 sd = lsub[x];
        const int nall = __builtin_amdgcn_readfirstlane((int)sd.y);
        return Sub{nall & 0xFFFF, (int)((unsigned)nall >> 16), __builtin_amdgcn_readfirstlane((int)sd.x)};
    }
    // What the assembly loops take beside the entries: the decay as one 64-bit scalar {c, c}, and the LDS byte address
    // of row slot 0 plus this lane's 16-byte offset inside a row.
    static __device__ __forceinline__ uint64_t pack_c2(const float c) {
        return ((uint64_t)__builtin_bit_cast(unsigned, c) << 32) | __builtin_bit_cast(unsigned, c);
    }
    static __device__ __forceinline__ unsigned row_base(unsigned char* rows, const unsigned lo) {
        return (unsigned)(uintptr_t)(lptr_t)rows + lo;
    }
    // the loops that have a hand-scheduled form (k in 33..256: 16, 32 or 64 lanes per rating)
    static constexpr bool kAsmLoops = L == 16 || L == 32 || L == 64;

    // Software pipeline: the rows of step t+1 are read before the rows of step t are
    // written back.  The scheduler guarantees (schedule.cpp, "Eligibility") that a
    // row read that early was not written in step t, except a q-side row in the same
    // lane slot, which is flagged and taken from registers instead.
    struct StepRegs {
        uint4 en;  // entry: addresses | flag, rating, lr*rating, decay factor
        unsigned pa, qa;
        float4 p, q;
    };

    template <bool TRAIN, bool TIMED = false>
    __device__ __forceinline__ void apply(const float lr, const float c, double& acc,
                                          unsigned long long* timers = nullptr) {
        unsigned char* const lr_ = lrows;
        const unsigned lo = laneoff;
        if constexpr (NH > 0 && TRAIN) {
            if (helper) {
                // Copy waves keep the barriers company: one per sub-round like everybody else.  Copy wave h
                // is also the HELPER of apply wave (h + 1) % W -- a wave on another SIMD -- whenever that
                // wave's sub-cell ends in a solo run: it follows the chain wave through the run's mailboxes,
                // redoes the q recurrence and does all the stores (run_asm.hpp).
                for (int s = 0; s < W; ++s) {
                    if constexpr (L >= 16) {
                        // header record of apply wave a's solo run in this sub-round, and its length (the sums are
                        // taken per lane, in front of the readfirstlane: decoded through sub() it is other code)
                        auto run_of = [&](const int a, int& ns) -> const uint4* {
                            const uint2 sd = lsub[s * W + a];
                            ns = __builtin_amdgcn_readfirstlane((int)(sd.x >> 16));
                            const int first = __builtin_amdgcn_readfirstlane((int)((sd.x & 0xFFFFu) + (sd.y & 0xFFFFu) + (sd.y >> 16))) + kSoloPad;
                            return lent + (size_t)first * G;
                        };
                        int ns;
                        const uint4* hdr = run_of((wave + 1) % W, ns);
                        // (cutting a long run in two and giving the second half to a second, idle copy wave was
                        // measured -- tools/ubench3 mode 4: 128.7 against 133.5 cycles per step at 16 lanes, no gain
                        // at 32 / 64; in situ 4.120 against 4.125 ms per epoch -- and is not done)
                        if (ns > 0 && !solo_helper_asm<L>((unsigned)(uintptr_t)(lptr_t)hdr, row_base(lr_, lo), ns, pack_c2(c)) && fail_flag)
                            *fail_flag = 1;
                    }
                    wg_barrier();
                }
                return;
            }
        }
        auto set_addr = [&](StepRegs& x) {
            x.pa = ((x.en.x & 0xFFFFu) << 4) + lo;
            x.qa = (__builtin_amdgcn_ubfe(x.en.x, 16, 15) << 4) + lo;
        };
        // One general step: `cur` holds step t (entry, addresses, rows); `nxt.en` holds
        // entry t+1.  Leaves `nxt` complete for step t+1 and cur.en = entry t+2.
        // Two register sets alternate roles, so the loop is unrolled by two and nothing
        // is copied between iterations.
        auto step = [&](StepRegs& cur, StepRegs& nxt, const uint4* eptr, const int e2) {
            __builtin_amdgcn_sched_barrier(0);  // the prefetch below must not climb into the previous step
            asm volatile("" : "+v"(nxt.en.x));   // ... nor its address arithmetic (no instruction emitted)
            const float r = __builtin_bit_cast(float, TRAIN ? cur.en.z : cur.en.y);  // lr*r when training
            set_addr(nxt);
            const float4 pn = lds_ld(lr_, nxt.pa);
            const float4 qn = lds_ld(lr_, nxt.qa);
            cur.en = eptr[e2];
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the arithmetic
            const float dot = group_allreduce<L>(chunk_dot(cur.p, cur.q));
            if constexpr (TRAIN) {
                const float sc = __builtin_fmaf(-lr, dot, r);  // lr*(r - dot): one dependent operation
                const float4 p2 = axpy_row(sc, cur.q, c, cur.p);
                const float4 q2 = axpy_row(sc, cur.p, c, cur.q);
                lds_st(lr_, cur.pa, p2);
                lds_st(lr_, cur.qa, q2);
                const bool fwd = (int)nxt.en.x < 0;
                nxt.q.x = fwd ? q2.x : qn.x;
                nxt.q.y = fwd ? q2.y : qn.y;
                nxt.q.z = fwd ? q2.z : qn.z;
                nxt.q.w = fwd ? q2.w : qn.w;
            } else {
                const float err = r - dot;
                acc += (double)err * (double)err;
                nxt.q = qn;
            }
            nxt.p = pn;
        };
        // Run step: the slot's q row is resident in `rq` for the whole run (no q load, no
        // select, no q store); idle slots are flagged.
        float4 rq;
        auto run_step = [&](StepRegs& cur, StepRegs& nxt, const uint4* eptr, const int e2) {
            __builtin_amdgcn_sched_barrier(0);  // the prefetch below must not climb into the previous step
            asm volatile("" : "+v"(nxt.en.x));   // ... nor its address arithmetic (no instruction emitted)
            const float r = __builtin_bit_cast(float, TRAIN ? cur.en.z : cur.en.y);
            const float ce = __builtin_bit_cast(float, cur.en.w);
            const bool idle = (int)cur.en.x < 0;
            nxt.pa = ((nxt.en.x & 0xFFFFu) << 4) + lo;
            const float4 pn = lds_ld(lr_, nxt.pa);
            cur.en = eptr[e2];
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the arithmetic
            const float dot = group_allreduce<L>(chunk_dot(cur.p, rq));
            if constexpr (TRAIN) {
                // idle slot (p = the all-zero row, r = 0, ce = 1): the resident row stays as it is and nothing is stored.
                // Not left to fma(0, p, 1*q): a resident row that holds an Inf or a NaN makes the dot with the zero row
                // NaN, which would turn the whole row NaN (run_asm.hpp masks the same lanes).
                const float sc = __builtin_fmaf(-lr, dot, r);
                const float4 p2 = axpy_row(sc, rq, ce, cur.p);
                const float4 q2 = axpy_row(sc, cur.p, ce, rq);
                if (!idle) {
                    rq = q2;
                    lds_st(lr_, cur.pa, p2);
                }
            } else if (!idle) {
                const float err = r - dot;
                acc += (double)err * (double)err;
            }
            nxt.p = pn;
        };
        // Training: sub-round s, this wave's sub-cell, a barrier after every sub-round.  The RMSE pass
        // writes nothing, so its sub-cells are independent: every wave of the workgroup (copy waves
        // included) takes sub-cells wave_all, wave_all + NWV, ... with no barrier in between.
        const int n_iter = TRAIN ? W : (W * W - wave_all + NWV - 1) / NWV;
        for (int s = 0; s < n_iter; ++s) {
            const Sub sc = sub(TRAIN ? s * W + wave : wave_all + s * NWV);
            const int n = sc.n, nr = sc.nr, nsolo = sc.nsolo();
            // entries of this wave's sub-cell; the host pads every cell with two idle
            // steps, so reading entries t+1 and t+2 past the end stays inside the image
            const uint4* ebase = lent + (size_t)sc.first() * G + g;
            unsigned long long tm0 = 0, tm1 = 0, tm2 = 0;
            if constexpr (TIMED) tm0 = __builtin_amdgcn_s_memtime();
            if (TRAIN && kAsmLoops && n > 0) {
                // hand-scheduled form of the loop below
                if constexpr (kAsmLoops) gen_loop_asm<G * 16, L>((unsigned)(uintptr_t)(lptr_t)ebase, row_base(lr_, lo), n, lr, pack_c2(c));
            } else if (n > 0) {
                const uint4* eptr = ebase;
                StepRegs A, B;
                A.en = eptr[0];
                B.en = eptr[G];
                set_addr(A);
                A.p = lds_ld(lr_, A.pa);
                A.q = lds_ld(lr_, A.qa);
                int t = 0;
                for (; t + 1 < n; t += 2, eptr += 2 * G) {
                    step(A, B, eptr, 2 * G);
                    step(B, A, eptr, 3 * G);
                }
                if (t < n) step(A, B, eptr, 2 * G);
            }
            if constexpr (TIMED) tm1 = __builtin_amdgcn_s_memtime();
            if (TRAIN && kAsmLoops && nr > 0 && (nr & 1) == 0) {
                // hand-scheduled form of the loop below
                const uint4* eptr = ebase + (size_t)n * G;
                const unsigned rqa = (__builtin_amdgcn_ubfe(eptr->x, 16, 15) << 4) + lo;
                rq = lds_ld(lr_, rqa);
                if constexpr (kAsmLoops) run_loop_asm<G * 16, L>(rq, (unsigned)(uintptr_t)(lptr_t)eptr, row_base(lr_, lo), nr >> 1, lr);
                lds_st(lr_, rqa, rq);
            } else if (nr > 0) {
                const uint4* eptr = ebase + (size_t)n * G;
                StepRegs A, B;
                A.en = eptr[0];
                B.en = eptr[G];
                // every run entry of a slot carries the slot's item address
                const unsigned rqa = (__builtin_amdgcn_ubfe(A.en.x, 16, 15) << 4) + lo;
                A.pa = ((A.en.x & 0xFFFFu) << 4) + lo;
                rq = lds_ld(lr_, rqa);
                A.p = lds_ld(lr_, A.pa);
                int t = 0;
                for (; t + 1 < nr; t += 2, eptr += 2 * G) {
                    run_step(A, B, eptr, 2 * G);
                    run_step(B, A, eptr, 3 * G);
                }
                if (t < nr) run_step(A, B, eptr, 2 * G);
                if constexpr (TRAIN) lds_st(lr_, rqa, rq);
            }
            if (TRAIN && nsolo > 0) {
                // Solo run: header record, then one 16-byte record per step {next slots, mailbox, lr*r, r}.
                const uint4* hdr = lent + (size_t)(sc.first() + n + nr + kSoloPad) * G;
                const unsigned s0 = hdr->x;
                if constexpr (TRAIN && NH > 0 && L >= 16) {
                    // chain wave: dot -> s -> q' only; its helper (a copy wave) stores the p rows and q
                    float4 q;
                    solo_chain_asm<L>(q, (unsigned)(uintptr_t)(lptr_t)hdr, s0, row_base(lr_, lo), nsolo, lr, pack_c2(c));
                    // the run was the cell's last work (its records end where the cell's steps end): hand the row on now
                    const int units = (nsolo + 2 + G - 1) / G + kSoloPad;
                    if (post_at != nullptr && sc.first() + n + nr + units + 2 == n_steps) {
                        if (lane < L) {  // lane group 0: lane l holds elements 4l .. 4l + 3 of the row
                            using gu64 = __attribute__((address_space(1))) unsigned long long;
                            gu64* dst = (gu64*)post_at + lig * 4;
                            const unsigned long long tag = (unsigned long long)post_tag << 32;
                            __hip_atomic_store(dst + 0, tag | __builtin_bit_cast(unsigned, q.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(dst + 1, tag | __builtin_bit_cast(unsigned, q.y), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(dst + 2, tag | __builtin_bit_cast(unsigned, q.z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(dst + 3, tag | __builtin_bit_cast(unsigned, q.w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        if (lane == 0) *posted_flag = 1u;
                    }
                } else if constexpr (TRAIN) {
                    // one wave does everything (kernels without copy waves); every lane group computes the
                    // same step -- the chain is sequential -- and they all store the same bits
                    const unsigned rqa = (__builtin_amdgcn_ubfe(s0, 16, 15) << 4) + lo;
                    float4 q = lds_ld(lr_, rqa);
                    unsigned pa = ((s0 & 0xFFFFu) << 4) + lo;
                    for (int t = 0; t < nsolo; ++t) {
                        const uint4 e = hdr[1 + t];
                        const float4 p = lds_ld(lr_, pa);
                        const float dot = group_allreduce<L>(chunk_dot(p, q));
                        const float sc = __builtin_fmaf(-lr, dot, __builtin_bit_cast(float, e.z));
                        const float4 p2 = axpy_row(sc, q, c, p);
                        q = axpy_row(sc, p, c, q);
                        lds_st(lr_, pa, p2);
                        pa = ((e.x & 0xFFFFu) << 4) + lo;
                    }
                    lds_st(lr_, rqa, q);
                }
                // (RMSE: the solo records of ALL sub-cells are shared out over all waves below)
            }
            if constexpr (TIMED) {
                tm2 = __builtin_amdgcn_s_memtime();
                if (lane == 0) {  // [wave][sub-round] -> {general cycles, run cycles, general steps, run steps}
                    unsigned long long* o = timers + ((size_t)wave * W + s) * 4;
                    o[0] = tm1 - tm0;
                    o[1] = tm2 - tm1;
                    o[2] = (unsigned long long)n;
                    o[3] = (unsigned long long)nr;
                }
            }
            if constexpr (TRAIN) wg_barrier();
        }
        if constexpr (!TRAIN) {
            // RMSE over the solo records: nothing is written, so the records of EVERY sub-cell are dealt out over
            // all waves of the workgroup and, inside a wave, lane group g takes record t0 + g (the address of
            // step t sits in record t - 1; groups past the end read the terminator: the zero row with r = 0).
            // (A cell that is one solo run -- an item with a tile of its own -- would otherwise be one wave's job.)
            // (the record's second word is only fetched for a sub-cell that has solo records: not sub())
            for (int sc = 0; sc < W * W; ++sc) {
                const uint2 sd = lsub[sc];
                const int offs = __builtin_amdgcn_readfirstlane((int)sd.x);
                const int nsolo = (int)((unsigned)offs >> 16);
                if (nsolo == 0) continue;
                const int nall = __builtin_amdgcn_readfirstlane((int)sd.y);
                const uint4* hdr = lent + (size_t)((offs & 0xFFFF) + (nall & 0xFFFF) + (int)((unsigned)nall >> 16) + kSoloPad) * G;
                const float4 q = lds_ld(lr_, (__builtin_amdgcn_ubfe(hdr->x, 16, 15) << 4) + lo);
                for (int t0 = wave_all * G; t0 < nsolo; t0 += NWV * G) {
                    const int t = t0 + g;
                    const bool live = t < nsolo;
                    const uint4 e = hdr[1 + (live ? t : nsolo)];  // past the end: the terminator (r = 0)
                    const unsigned sl = hdr[live ? t : nsolo].x;    // ... whose predecessor addresses the zero row
                    const float4 p = lds_ld(lr_, ((sl & 0xFFFFu) << 4) + lo);
                    const float err = __builtin_bit_cast(float, e.w) - group_allreduce<L>(chunk_dot(p, q));
                    acc += (double)err * (double)err;
                }
            }
        }
    }
};

}  // namespace
}  // namespace mfsgd
