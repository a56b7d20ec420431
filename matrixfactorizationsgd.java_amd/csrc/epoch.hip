// epoch.hip -- the persistent training kernel: one launch runs n_rounds consecutive rounds of the block schedule,
// the item tiles handed from workgroup to workgroup inside the GPU.  What a workgroup does with
// a cell is cell.hpp; the one-launch-per-round form of the same rounds is cells.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cell.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {

namespace {

// ---- persistent epoch kernel -----------------------------------------------------
// One launch = n_rounds consecutive rounds (an epoch is B rounds).  Workgroup x owns
// user blocks x, x + NP, ... for the whole launch: their P rows are only ever touched
// by this workgroup (this CU), so they need no inter-workgroup protocol.  Item tiles
// move: tile (b + rd) % B is trained by block b in round rd and by block b - 1 in
// round rd + 1, i.e. block b waits for block b + 1 -- a ring hand-off between
// workgroups inside the GPU, the same shape as the DSGD ring between GPUs.
//   producer: q rows stored write-through (sc1) -> every wave s_waitcnt vmcnt(0) ->
//             workgroup barrier -> one lane stores done[b] = R + 1 (relaxed, agent scope);
//   consumer: one lane polls done[b + 1] >= R (relaxed, agent scope, s_sleep) -> workgroup
//             barrier -> the tile's rows are gathered with sc1 loads (they bypass this CU's L1,
//             which is all an acquire fence in front of plain loads would have done).
// (cdna_hip_programming.md Guideline 16, form R1 with sc1 loads in place of the acquire; round 1
// had the fence -- buffer_inv sc1 + s_waitcnt vmcnt(0), ~1.5 us per hop.)  A tile that is ONE item
// row does not use the flags at all: it travels through its mailbox (below).  While it waits, a workgroup has
// already staged the next cell's schedule and gathered its own P rows.  All NP
// workgroups must be co-resident (the host sizes NP from the occupancy query); every
// spin is bounded and raises *abort_word instead of hanging.
constexpr int kFlagStride = 32;  // one done[] word per 128-byte line

using gu32 = __attribute__((address_space(1))) unsigned;
using gu64 = __attribute__((address_space(1))) unsigned long long;

// ---- the ring's protocol, piece by piece ----------------------------------------------------
// Start-of-launch rendezvous, before anything is touched (one thread of the workgroup).  Returns the abort code
// (0: go on) and, in my_gen, the launch generation that tags this launch's mailbox posts.  It does two jobs with one
// device-side barrier (sense reversing: abort_word[-4] counts arrivals, abort_word[-3] is the generation):
//  * the hand-off flags are reset HERE, by their owners (block b's flag by the workgroup that runs
//    block b), and nobody proceeds until everybody has -- the host zeroes nothing between launches
//    (a memset node in a replayed hipGraph was measured NOT to be reliably ordered before the kernel
//    node behind it: flags still standing from the previous epoch let consumers run ahead of their
//    producers);
//  * it proves that all NP workgroups are on the chip at once, which the hand-off protocol needs.
//    When they are not -- another kernel holds CUs -- the launch gives up with the factors untouched
//    (abort code 2) and the host runs the epoch as one launch per round instead.  A launch that finds
//    the abort word already set (an earlier launch of the same stream gave up) does nothing either.
__device__ __forceinline__ unsigned start_barrier(unsigned* __restrict__ done, unsigned* __restrict__ abort_word,
                                                  const int B, const int wg, const int NP, unsigned& my_gen) {
    unsigned bad = __hip_atomic_load((gu32*)abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    my_gen = 0;
    if (bad == 0u) {
        gu32* arrive = (gu32*)(abort_word - 4);
        gu32* gen = (gu32*)(abort_word - 3);
        for (int b = wg; b < B; b += NP)
            __hip_atomic_store((gu32*)(done + (size_t)b * kFlagStride), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned g0 = __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // before arriving
        my_gen = (g0 + 1u) & 0xFFFFu;  // the same in every workgroup of this launch
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // my flags are zero before my arrival counts
        // Arrival counter: low 31 bits count arrivals, bit 31 says "a waiter has given up".  Giving up and
        // releasing are decided on this ONE word, so they cannot both happen: a waiter that times out sets the bit
        // and leaves; the last arriver finds it set and refuses to release (it raises the abort code instead).
        // (Round 2 had the waiter set the abort word and leave without looking back: the last workgroup could
        // arrive in that window, release the others and let them train with one workgroup missing.)
        constexpr unsigned kGaveUp = 0x80000000u;
        const unsigned old = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((old & ~kGaveUp) == (unsigned)NP - 1u) {
            // the last one in: NP -> 0 releases, and only if nobody has set the bit -- one compare-and-swap, so a
            // waiter's give-up (NP -> NP | bit) and the release exclude each other whichever comes first
            unsigned expected = (unsigned)NP;
            if ((old & kGaveUp) == 0u &&
                __hip_atomic_compare_exchange_strong(arrive, &expected, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_store(gen, g0 + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                expected = 0u;
                __hip_atomic_compare_exchange_strong((gu32*)abort_word, &expected, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                bad = 2u;  // somebody left: nobody trains (the host zeroes the counter when it handles the abort)
            }
        } else {
            unsigned spins = 0;
            while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g0) {
                __builtin_amdgcn_s_sleep(8);
                if ((++spins & 63u) == 0u) {
                    bad = __hip_atomic_load((gu32*)abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bad == 0u && spins > (1u << 19)) {
                        // give up -- unless the barrier completed meanwhile: the release zeroes the counter, so a
                        // release that has happened shows as a count of 0 here; then take the bit back and wait
                        // for the generation (which the last arriver advances next)
                        const unsigned was = __hip_atomic_fetch_or(arrive, kGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((was & ~kGaveUp) == 0u) {
                            __hip_atomic_fetch_and(arrive, ~kGaveUp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g0) __builtin_amdgcn_s_sleep(1);
                            break;
                        }
                        unsigned expected = 0u;  // only the first one to give up sets the code
                        __hip_atomic_compare_exchange_strong((gu32*)abort_word, &expected, 2u, __ATOMIC_RELAXED,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        bad = 2u;
                    }
                    if (bad != 0u) break;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    return bad;
}

// The wait for a tile's flag (one thread): until the flag reaches R.  Bounded: raises the abort word and ctl[0]
// instead of hanging.
__device__ __forceinline__ void wait_flag(gu32* flag, const unsigned R, unsigned* __restrict__ abort_word,
                                          volatile unsigned* ctl) {
    unsigned spins = 0;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < R) {
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0u) {
            if (__hip_atomic_load((gu32*)abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
                spins > (1u << 22)) {
                __hip_atomic_store((gu32*)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ctl[0] = 1;
                break;
            }
        }
    }
    asm volatile("" ::: "memory");  // the tile's rows are loaded sc1 below: no acquire fence
}

// The post of a row to its mailbox (one wave): lane l stores the granules {tag, element l + 64 j of the LDS row `row`}
// to dst[64 j].  (The take of a row, its counterpart, is written out in run_ring: as a function of its own it did not
// compile to the same code.)
template <int NGR>
__device__ __forceinline__ void post_row(gu64* dst, const unsigned long long tag, const int lane,
                                         const unsigned char* row) {
#pragma unroll
    for (int j = 0; j < NGR; ++j) {
        const unsigned bits = *reinterpret_cast<const unsigned*>(row + (size_t)(lane + 64 * j) * 4);
        __hip_atomic_store(dst + 64 * j, tag | bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One ring: workgroup `wg` of `NP` runs its share of the B x n_rounds cells of one schedule.
template <int L, int W, int NH>
__device__ __forceinline__ void run_ring(unsigned char* smem, float* __restrict__ P, float* __restrict__ Q,
                                         const CellDesc* __restrict__ cells, const uint32_t* __restrict__ rows,
                                         const SubDesc* __restrict__ subs, const Entry* __restrict__ entries,
                                         const int B, const int n_rounds, const float lr, const float c,
                                         unsigned* __restrict__ done, unsigned* __restrict__ abort_word,
                                         const int sched_cap, const int wg, const int NP,
                                         unsigned long long* __restrict__ prof) {
    volatile unsigned* const ctl = reinterpret_cast<volatile unsigned*>(smem);  // [0] = abort broadcast
    Cell<L, W, NH> cx;
    cx.init_thread();
    cx.fail_flag = ctl;
    cx.posted_flag = ctl + 3;
    if (cx.tid == 0) {
        unsigned my_gen;
        const unsigned bad = start_barrier(done, abort_word, B, wg, NP, my_gen);
        ctl[0] = bad != 0u ? 1u : 0u;
        ctl[1] = bad;
        ctl[2] = my_gen;
    }
    wg_barrier();
    if (ctl[0] != 0) return;  // uniform; nothing has been modified
    // Tile mailboxes (cells marked kCellLoneTile: a tile that is ONE item row in every cell -- the item whose chain
    // the epoch waits for).  The row travels as KP granules {value, tag}, each written by ONE 8-byte sc1 store and
    // read by ONE 8-byte sc1 load (a granule is never seen torn), tag = launch generation << 16 | round + 1: the
    // consumer polls the granules themselves until every tag is the one it expects -- one memory round trip per
    // hop, no drain, no flag, no gather -- and nothing of an earlier round or launch can be mistaken for it.
    // Only the holder in the launch's LAST round stores the row to Q; the first round takes it from Q.
    // THE FAST LANE.  The hop the epoch waits for is the lone tile of the heaviest item, whose cell is ONE solo run in
    // sub-cell 0 (Cell::lone_solo_only; R > 0).  Nothing but the row's VALUE is missing while such a cell waits, so
    // everything else happens in front of the wait (Cell::lone_round0, run_asm.hpp MFSGD_LONE_CHAIN_ASM_TEXT):
    //   all waves    s_waitcnt vmcnt(0) + workgroup barrier: own P rows and the next schedule are in LDS; ctl[0] is looked at;
    //   chain wave   (apply wave 0) decodes its run, prepares the post (address, tag, lane mask), reads {lr r_0, slots_1}
    //                and p row 0, then polls the mailbox ITSELF, four granules per lane in the layout the chain loop
    //                keeps q in (every lane group the same addresses), bounded like the poll below;
    //   other waves  wait at ONE s_barrier -- the helper with its run decoded, outside its loop;
    //   arrival      tag test, one ds_write_b128 of q into the row's LDS slot (for the helper, which reads it behind
    //                s_0), that s_barrier, step 0.  Behind the last step's q' the four granule stores of the post;
    //   giving up    the chain wave raises the abort word and ctl[0], joins the barrier, and every wave leaves behind
    //                it as on the other path: nothing trained, posted or stored.
    // The barriers of a cell are as many as on the other path, in every wave.  Every other cell -- R == 0, a lone tile
    // whose run is not one solo run in sub-cell 0, W = 8 (no helpers) -- takes the path below, unchanged.
    gu64* const mbox = (gu64*)(abort_word + 4);
    const unsigned tag_hi = ctl[2] << 16;
    constexpr int KP = Cell<L, W, NH>::KP, ROWB = Cell<L, W, NH>::ROWB;
    constexpr int NGR = KP >= 64 ? KP / 64 : 1;  // granules per lane of one wave

    // This workgroup's work list: (round R, block b) for b = blockIdx.x, +NP, ... in round order,
    // and within a cell its chunks in chain order.
    struct Item {
        int R, b;
        unsigned idx;  // chunk descriptor
        bool first;    // first chunk of its cell: the tile has to be waited for
    };
    auto cell_of = [&](int R, int b) { return (unsigned)(b * B + (b + R % B) % B); };
    auto next_item = [&](const Item& it, const CellDesc& d) {
        Item n = it;
        if (d.next != 0) {
            n.idx = d.next;
            n.first = false;
        } else {
            n.b += NP;
            if (n.b >= B) {
                n.b = wg;
                ++n.R;
            }
            n.idx = cell_of(n.R, n.b);
            n.first = true;
        }
        return n;
    };
    // Software pipeline over the list: descriptors are fetched two items ahead (registers),
    // schedules one item ahead (LDS-DMA into the other schedule buffer).
    Item it0{0, wg, cell_of(0, wg), true};
    CellDesc cd = load_desc(cells, it0.idx);
    Item it1 = next_item(it0, cd);
    CellDesc cd1 = it1.R < n_rounds ? load_desc(cells, it1.idx) : cd;
    int buf = 0;
    cx.bind(cd, smem, buf, sched_cap);
    cx.stage_schedule(cd, (int)it0.idx, rows, subs, entries);  // the first one synchronously
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_barrier();

    // optional phase accounting (diagnostic launches only): shader cycles of wave 0 per phase
    unsigned long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [7]: the longest single "ratings" phase (its slowest cell)
    unsigned long long pcur[7] = {0, 0, 0, 0, 0, 0, 0}, pmax[7] = {0, 0, 0, 0, 0, 0, 0};  // this pass / the pass of [7]
    unsigned long long pt = 0;
    auto mark = [&](int k) {
        if (prof) {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            pacc[k] += now - pt;
            pcur[k] = now - pt;
            if (k == 6 && pcur[4] > pacc[7]) {  // end of a pass whose ratings phase is the longest so far
                pacc[7] = pcur[4];
                for (int x = 0; x < 7; ++x) pmax[x] = pcur[x];
            }
            pt = now;
        }
    };
    // ... up to a stamp another part of the wave's code took (the low word of s_memtime)
    auto mark_at = [&](int k, const unsigned now_lo) {
        const unsigned long long now = pt + (unsigned long long)(now_lo - (unsigned)pt);
        pacc[k] += now - pt;
        pcur[k] = now - pt;
        pt = now;
    };
    if (prof) pt = __builtin_amdgcn_s_memtime();

    for (; it0.R < n_rounds;) {
        const int R = it0.R, b = it0.b;
        CellDesc cd2 = cd1;
        cx.bind(cd, smem, buf, sched_cap);
        const bool work = cx.nrows != 0;  // uniform over the workgroup
        const bool last = cd.next == 0;   // last chunk of its cell: the tile is handed on after it
        cx.zero_idle_rows();
        if (cx.tid == 0) ctl[3] = 0u;  // "the chain wave has posted the tile's row" (read behind the barriers below)
        // The rows stored at the end of the previous iteration may be gathered again below.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef MFSGD_DIAG_SPLIT_PHASE0  // (a build for tools/phase_profile.py that takes phase 0 apart)
        mark(0);  // phase 0 = zeroing + drain only
#endif
        if (it1.R < n_rounds) cx.prefetch_schedule(cd1, (int)it1.idx, smem, buf ^ 1, sched_cap, rows, subs, entries);
        if (work) cx.gather(P, Q, 0, cx.nu);  // own rows: no dependency on other workgroups
        // descriptor used two iterations from now: a scalar load issued here, in front of the wait for the tile,
        // so that it completes in that wait's shadow (behind the tile gather it was exposed -- ~1.4 K cycles --
        // whenever there was no gather to hide it: a tile taken from its mailbox)
        const Item it2 = next_item(it1, cd1);
        const bool lone = KP >= 64 && (cd.rsv[0] & kCellLoneTile) != 0;  // uniform
#ifdef MFSGD_DIAG_SPLIT_PHASE0
        mark(2);  // diagnostic build: the issue of prefetch and gather, booked under "barrier"
#endif
        if (it2.R < n_rounds) cd2 = load_desc(cells, it2.idx);
#ifdef MFSGD_DIAG_SPLIT_PHASE0
        mark(6);  // diagnostic build: the descriptor load (s_memtime waits for it), booked under "own store"
#else
        mark(0);  // drain of the previous stores + issue of the prefetch and the P gather
#endif
        // The fast lane of the hop the epoch waits for (protocol: the comment above run_ring): a lone-tile cell whose only
        // work is ONE solo run takes everything that does not depend on the row's VALUE in front of the wait for it.
        const bool fast = R > 0 && it0.first && lone && cx.lone_solo_only();  // uniform
        if (fast) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own rows (and the prefetched schedule) have landed
            wg_barrier();
            mark(2);  // the other waves' arrival
            if (ctl[0] != 0) {  // uniform: a solo helper of this workgroup gave up in the previous cell
                if (cx.tid == 0) __hip_atomic_store((gu32*)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            const unsigned tile = (unsigned)((b + R % B) % B);
            if (R + 1 < n_rounds) {
                cx.post_at = (unsigned long long*)(mbox + (size_t)tile * KP);  // the tile's mailbox
                cx.post_tag = tag_hi | (unsigned)(R + 1);
            } else {
                cx.post_at = nullptr;
            }
            // every wave but the chain wave waits inside for the row, at the barrier the chain wave joins on arrival; the
            // run and the cell's sub-round barriers follow inside too
            if (!cx.lone_round0(lr, c, mbox + (size_t)tile * KP, tag_hi | (unsigned)R, (gu32*)abort_word, ctl, prof != nullptr))
                return;  // uniform: the row never came (abort word and ctl[0] are set); nothing has been stored
            if (prof) {
                const unsigned arrived = ctl[1];  // the chain wave's stamp (this thread's own wave: tid 0 books)
                mark_at(1, arrived);  // waiting for the tile
                mark_at(3, arrived);  // (nothing is gathered)
            }
            mark(4);  // the ratings, from the row's arrival
            // posted by the chain wave; in the launch's last round the row goes to Q from its LDS slot (the helper's store)
            if (R + 1 >= n_rounds) cx.template scatter<true>(P, Q, cx.nu, cx.nrows);
        } else {
            if (R > 0 && it0.first && lone) {
                // the tile is one row: take it from the tile's mailbox as soon as block b + 1 has posted it
                if (cx.wave_all == 0) {
                    const unsigned tile = (unsigned)((b + R % B) % B);
                    const unsigned want = tag_hi | (unsigned)R;  // posted in round R - 1
                    const gu64* src = mbox + (size_t)tile * KP + cx.lane;
                    unsigned long long v[NGR];
                    unsigned spins = 0;
                    for (;;) {
                        bool ok = true;
#pragma unroll
                        for (int j = 0; j < NGR; ++j) {
                            v[j] = __hip_atomic_load(src + 64 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            ok = ok && (unsigned)(v[j] >> 32) == want;
                        }
                        if (__builtin_amdgcn_ballot_w64(!ok) == 0ull) break;
                        __builtin_amdgcn_s_sleep(1);
                        if ((++spins & 255u) == 0u) {
                            if (__hip_atomic_load((gu32*)abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
                                spins > (1u << 22)) {
                                if (cx.lane == 0) {
                                    __hip_atomic_store((gu32*)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    ctl[0] = 1;
                                }
                                break;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NGR; ++j)
                        *reinterpret_cast<unsigned*>(cx.lrows + (size_t)cx.nu * ROWB + (size_t)(cx.lane + 64 * j) * 4) = (unsigned)v[j];
                }
            } else if (R > 0 && it0.first) {
                // wait until block b + 1 has finished round R - 1 (it held our tile)
                if (cx.tid == 0) {
                    wait_flag((gu32*)(done + (size_t)((b + 1) % B) * kFlagStride), (unsigned)R, abort_word, ctl);
                }
            }
            mark(1);  // waiting for the tile (wave 0)
            const bool from_mbox = lone && R > 0;  // the tile's row is in LDS already (wave 0 put it there)
            // (Waiting for the own rows in front of this barrier and dropping the second one for a row that came from its
            // mailbox -- one barrier less on the hop the epoch waits for -- was measured: 4.00 against 3.97 ms per epoch
            // on the same box, three runs each; the second barrier stays.)
            wg_barrier();
            mark(2);  // the other waves' arrival
            if (ctl[0] != 0) {  // uniform: some workgroup timed out (or a solo helper of this one gave up)
                if (cx.tid == 0) __hip_atomic_store((gu32*)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            if (work && !from_mbox) cx.template gather<true>(P, Q, cx.nu, cx.nrows);  // the tile's q rows, sc1: stored by another CU
            if (work) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // rows (and the prefetched schedule) have landed
                wg_barrier();
                mark(3);  // tile rows (and own rows, and the next schedule) landed
                double acc = 0.0;
                if (lone && R + 1 < n_rounds) {
                    cx.post_at = (unsigned long long*)(abort_word + 4) + (size_t)((b + R % B) % B) * KP;  // the tile's mailbox
                    cx.post_tag = tag_hi | (unsigned)(R + 1);
                } else {
                    cx.post_at = nullptr;
                }
                cx.template apply<true>(lr, c, acc);  // ends with a workgroup barrier
                mark(4);  // the ratings
                // write-through even when more chunks of this cell follow: item rows that no later
                // chunk touches have to be visible to the next workgroup all the same
                if (lone && R + 1 < n_rounds) {
                    // post the row for block b - 1 (round R + 1); Q gets it from the holder in the last round
                    // (unless the chain wave has posted it from its registers already, Cell::post_at)
                    if (cx.wave_all == 0 && ctl[3] == 0u) {
                        const unsigned tile = (unsigned)((b + R % B) % B);
                        const unsigned long long tag = (unsigned long long)(tag_hi | (unsigned)(R + 1)) << 32;
                        post_row<NGR>(mbox + (size_t)tile * KP + cx.lane, tag, cx.lane, cx.lrows + (size_t)cx.nu * ROWB);
                    }
                } else {
                    cx.template scatter<true>(P, Q, cx.nu, cx.nrows);
                }
            }
        }
        // publish the tile: every storing wave drains, then one lane signals
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_barrier();
        if (last && cx.tid == 0)
            __hip_atomic_store((gu32*)(done + (size_t)b * kFlagStride), (unsigned)(R + 1), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        mark(5);  // tile rows stored write-through, drained, flag published
        if (work) cx.template scatter<false>(P, Q, 0, cx.nu);
        // The rows image and this schedule buffer are reused from here on: their LDS reads (the
        // scatter above) are complete once every wave has passed this barrier.  The next
        // schedule has been complete since the vmcnt(0) + barrier above.
        wg_barrier();
        buf ^= 1;
        cd = cd1;
        cd1 = cd2;
        it0 = it1;
        it1 = it2;
        mark(6);  // own rows stored (not drained), end barrier
    }
    if (ctl[0] != 0 && cx.tid == 0)  // raised during the last cell
        __hip_atomic_store((gu32*)abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wg == 0 && cx.tid == 0)  // launches that got past the residency check (the host counts on it when one did not)
        __hip_atomic_fetch_add((gu32*)(abort_word + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prof && cx.tid == 0) {
        for (int k = 0; k < 8; ++k) prof[(size_t)wg * 16 + k] = pacc[k];
        for (int k = 0; k < 7; ++k) prof[(size_t)wg * 16 + 8 + k] = pmax[k];
    }
}

template <int L, int W>
__global__ void __launch_bounds__(64 * (W + epoch_helpers<L, W>()))
epoch_kernel(float* __restrict__ P, float* __restrict__ Q, const CellDesc* __restrict__ cells,
             const uint32_t* __restrict__ rows, const SubDesc* __restrict__ subs,
             const Entry* __restrict__ entries, const int B, const int n_rounds, const float lr,
             const float c, unsigned* __restrict__ done, unsigned* __restrict__ abort_word,
             const int sched_cap, unsigned long long* __restrict__ prof) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    run_ring<L, W, epoch_helpers<L, W>()>(smem, P, Q, cells, rows, subs, entries, B, n_rounds, lr, c, done, abort_word,
                                           sched_cap, (int)blockIdx.x, (int)gridDim.x, prof);
}

// > 64 KiB of dynamic LDS has to be granted per function; cheap to repeat.
template <int L, int W>
hipError_t epoch_grant_lds(const CellLaunch& a) {
    return hipFuncSetAttribute((const void*)epoch_kernel<L, W>, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
}

template <int L, int W>
hipError_t epoch_occupancy_LW(const CellLaunch& a, int* blocks_per_cu) {
    const hipError_t e = epoch_grant_lds<L, W>(a);
    if (e != hipSuccess) return e;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, (const void*)epoch_kernel<L, W>,
                                                        64 * (W + epoch_helpers<L, W>()), (size_t)a.lds_bytes);
}

template <int L, int W>
hipError_t epoch_launch_LW(const CellLaunch& a, int n_rounds, unsigned* done, unsigned* abort_word, hipStream_t st) {
    const hipError_t e = epoch_grant_lds<L, W>(a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((epoch_kernel<L, W>), dim3((unsigned)a.grid), dim3(64 * (W + epoch_helpers<L, W>())),
                       (size_t)a.lds_bytes, st, a.P, a.Q, a.cells, a.rows, a.subs, a.entries, a.B, n_rounds, a.lr, a.c, done,
                       abort_word, a.sched_cap, reinterpret_cast<unsigned long long*>(a.diag ? a.sse_partial : nullptr));
    return hipGetLastError();
}

}  // namespace

hipError_t epoch_blocks_per_cu(int L, int W, const CellLaunch& a, int* blocks_per_cu) {
    return with_L(L, [&](auto l) { return with_W(W, [&](auto w) { return epoch_occupancy_LW<l(), w()>(a, blocks_per_cu); }); });
}

hipError_t launch_epoch_persistent(int L, int W, const CellLaunch& a, int n_rounds, unsigned* done,
                                   unsigned* abort_word, hipStream_t st) {
    return with_L(L, [&](auto l) {
        return with_W(W, [&](auto w) { return epoch_launch_LW<l(), w()>(a, n_rounds, done, abort_word, st); });
    });
}

}  // namespace mfsgd
