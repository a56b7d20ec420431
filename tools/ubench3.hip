// Microbenchmark + correctness check of the SOLO run loops (csrc/run_asm.hpp): one workgroup of
// two waves on two SIMDs, wave 0 = chain wave, wave 1 = helper.  Prints cycles per step of the pair
// (and of the chain wave alone, MODE=1: no helper, nothing stored) and compares every p row and the
// q row with a plain host restatement of DESIGN.md section 3.
// Modes 3 / 8 (`ubench3 loops`): the one-wave loops of a sub-cell, wave 0 alone -- the run loop (slot 0 carries the chain, the
// other slots idle) and the general loop (every lane group a rating per step, forwarded q rows and p rows recurring at
// distance two in the data) -- cycles per step and the same comparison.
// Modes 6 / 7 (`ubench3 lone`): the run of a lone-tile cell of the persistent kernel -- q comes out of a mailbox in global
// memory into the chain wave's registers, p row 0 and the entry words are read in front of the wait, the helper waits at
// the barrier the chain wave joins on arrival (MFSGD_LONE_CHAIN_ASM_TEXT); timed from the arrival stamp, beside mode 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../matrixfactorizationsgd.java_amd/csrc/run_asm.hpp"

#ifndef LG
#define LG 16  // lanes per rating
#endif
#define SWAP16 "v_mov_b32 v133, v132\n\ts_nop 1\n\tv_permlane16_swap_b32 v132, v133\n\ts_nop 1\n\tv_add_f32 v132, v132, v133\n\t"
#define SWAP32 "v_mov_b32 v133, v132\n\ts_nop 1\n\tv_permlane32_swap_b32 v132, v133\n\ts_nop 1\n\tv_add_f32 v132, v132, v133\n\t"
#define SFMA MFSGD_SFMA_V
#define SFMA2 MFSGD_SFMA2_V
#if LG == 16
#define EXTRA ""
#elif LG == 32
#define EXTRA SWAP16
#ifndef OLD32
#define EXTRA_SOLO MFSGD_BCAST_ADD32  // the solo chain: one rating per wave
#undef SFMA2
#define SFMA2 MFSGD_SFMA2_S
#endif
#else
#ifdef OLD64
#define EXTRA SWAP16 SWAP32
#else
#define EXTRA MFSGD_BCAST_ADD64
#undef SFMA
#define SFMA MFSGD_SFMA_S
#undef SFMA2
#define SFMA2 MFSGD_SFMA2_S
#endif
#endif

#ifndef EXTRA_SOLO
#define EXTRA_SOLO EXTRA
#endif

constexpr int ROWB = 16 * LG;
constexpr int NSTEP = (LG == 64 ? 120 : LG == 32 ? 200 : 300), NROWS = NSTEP + 2;  // p rows 0..NSTEP-1, q row NSTEP, zero row NSTEP+1
constexpr int ENT_OFF = NROWS * ROWB;          // entries behind the rows
constexpr int GS = 64 / LG;                    // slots per step of the (old) run loop
constexpr int RUN_OFF = ENT_OFF + (NSTEP + 2) * 16;  // mode 3: run-loop entries, NSTEP + 2 steps x GS x 16 bytes
constexpr int EXTRA_ZERO = NROWS;              // (mode 3 idle slots use the zero row too)
constexpr int CTL_OFF = RUN_OFF + (NSTEP + 2) * GS * 16;  // modes 6 / 7: control block ([0] abort broadcast, [1] arrival stamp)
using gu64 = __attribute__((address_space(1))) unsigned long long;
using gu32 = __attribute__((address_space(1))) unsigned;

__global__ void __launch_bounds__(192) k(const float* rows_in, const uint32_t* ent_in, float* rows_out, uint32_t* ent_out,
                                         unsigned long long* cyc, int n_steps, float lr, float c, int mode,
                                         const uint32_t* run_in, int first_row, const unsigned long long* mbox,
                                         unsigned* abort_word, unsigned long long* post_box, unsigned want_tag) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    for (int x = threadIdx.x; x < NROWS * ROWB / 4; x += blockDim.x) ((float*)smem)[x] = rows_in[x];
    for (int x = threadIdx.x; x < (NSTEP + 2) * 4; x += blockDim.x) ((uint32_t*)(smem + ENT_OFF))[x] = ent_in[x];
    for (int x = threadIdx.x; x < (NSTEP + 2) * GS * 4; x += blockDim.x) ((uint32_t*)(smem + RUN_OFF))[x] = run_in[x];
    if (threadIdx.x < 4) ((uint32_t*)(smem + CTL_OFF))[threadIdx.x] = 0u;
    __syncthreads();
    if (mode == 6 || mode == 7) {  // the q row is NOT in LDS: it comes out of the mailbox
        for (int x = threadIdx.x; x < ROWB / 4; x += blockDim.x) ((float*)(smem + NSTEP * ROWB))[x] = -7.0f;
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned rowbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem + (lane % LG) * 16;
    const unsigned ea = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + ENT_OFF);
    const uint64_t c2 = ((uint64_t)__builtin_bit_cast(uint32_t, c) << 32) | __builtin_bit_cast(uint32_t, c);
    unsigned long long t0 = 0, t1 = 0;
    int n = n_steps;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    if (wave == 0 && mode == 3) {
        // the one-wave run loop (cell.hpp run_loop_asm): slot 0 carries the chain, the others idle
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int g = lane / LG;
        const unsigned qaddr = (g == 0 ? NSTEP : NSTEP + 1) * ROWB + (lane % LG) * 16;
        f4 q = *(const f4*)(smem + qaddr);
        const unsigned ea = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + RUN_OFF) + g * 16;
        int pairs = n_steps / 2;
        uint64_t live, sv;  // scalar temporaries of the run loop's text
        constexpr int EST = GS * 16;
        constexpr int PADV = mfsgd_pad_run(LG);
        asm volatile(MFSGD_RUN_LOOP_ASM_TEXT(EXTRA, SFMA) MFSGD_RUN_LOOP_ASM_OPERANDS);
        if (g == 0) *(f4*)(smem + qaddr) = q;
    } else if (wave == 0 && mode == 8) {
        // the one-wave general loop (cell.hpp gen_loop_asm): every lane group one rating per step, both rows from LDS
        const unsigned ea = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + RUN_OFF) + (lane / LG) * 16;
        constexpr int EST = GS * 16;
        constexpr int PADV = mfsgd_pad_gen(LG);
        asm volatile(MFSGD_GEN_LOOP_ASM_TEXT(EXTRA, SFMA) MFSGD_GEN_LOOP_ASM_OPERANDS);
    } else if (wave == 0 && mode == 4) {
        // cut run: the chain wave stores q into its row between the halves (measured and not used by the product: run_asm.hpp)
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4 q;  // (the chain loop loads the q row itself)
        constexpr int PADV = mfsgd_pad_chain_tail(LG), PADS = mfsgd_pad_chain_steady(LG);
        const int m = (n_steps / 2) & ~1;
        const unsigned ea0 = ea;
        n = m;
        {
            const unsigned s0 = *(const uint32_t*)(smem + ENT_OFF);
            asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT(EXTRA_SOLO, SFMA2) MFSGD_SOLO_CHAIN_OPERANDS);
        }
        *(f4*)(smem + NSTEP * ROWB + (lane % LG) * 16) = q;
        {
            const unsigned ea = ea0 + m * 16;
            const unsigned s0 = *(const uint32_t*)(smem + ENT_OFF + m * 16);  // entry m - 1 serves as the second half's header
            n = n_steps - m;
            asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT(EXTRA_SOLO, SFMA2) MFSGD_SOLO_CHAIN_OPERANDS);
        }
    } else if (mode == 6 || mode == 7) {
        const unsigned ctl = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)(smem + CTL_OFF);
        if (wave == 0) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            if (mode == 7) {  // mode 5's case: the p row of step 0 updated in front of the run (here: in front of its early read)
                f4* p0 = (f4*)(smem + first_row * ROWB + (lane % LG) * 16);
                f4 v = *p0;
                v += 1.0f;
                *p0 = v;
            }
            const unsigned s0 = *(const uint32_t*)(smem + ENT_OFF);
            const gu64* src = (const gu64*)mbox + (lane % LG) * 4;
            gu64* dst = (gu64*)post_box + (lane % LG) * 4;
            const gu32* abw = (const gu32*)abort_word;
            const unsigned want = (unsigned)__builtin_amdgcn_readfirstlane((int)want_tag), ptag = want + 1u, prof = 1u;
            const uint64_t pm = LG == 64 ? ~0ull : (1ull << (LG & 63)) - 1ull;
            unsigned spins = 0, gave = 0, t0;
            uint64_t tmp;
            constexpr int PADV = mfsgd_pad_chain_tail(LG), PADS = mfsgd_pad_chain_steady(LG);
            asm volatile(MFSGD_LONE_CHAIN_ASM_TEXT(EXTRA_SOLO, SFMA2) MFSGD_LONE_CHAIN_OPERANDS);
            if (gave && lane == 0) cyc[2] = 2;
        } else if (wave == 1) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (*(volatile uint32_t*)(smem + CTL_OFF) == 0u) {
                int spins = 1 << 20, fin = 1;
                asm volatile("" : "+s"(fin));
                constexpr int PADV = mfsgd_pad_helper(LG);
                asm volatile(MFSGD_SOLO_HELPER_ASM_TEXT MFSGD_SOLO_HELPER_OPERANDS);
                if (spins == 0 && lane == 0) cyc[2] = 1;
            }
        }
    } else if (wave == 0 && mode != 2) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        if (mode == 5) {
            // (mode 5 = mode 0 plus this; correctness only, the delay is inside the timed region)
            // what the product's chain wave does in front of a solo run: general steps of its sub-cell, which may update
            // p rows the run is about to use -- here: p row of step 0 += 1, late enough for a helper that reads rows
            // before s_0 is posted to have read the old one (the host reference starts from the updated row)
            for (int d = 0; d < 40; ++d) __builtin_amdgcn_s_sleep(64);
            f4* p0 = (f4*)(smem + first_row * ROWB + (lane % LG) * 16);
            f4 v = *p0;
            v += 1.0f;
            *p0 = v;
        }
        f4 q;  // (the chain loop loads the q row itself)
        const unsigned s0 = *(const uint32_t*)(smem + ENT_OFF);  // the header's slots word, as Cell::apply reads it
        constexpr int PADV = mfsgd_pad_chain_tail(LG), PADS = mfsgd_pad_chain_steady(LG);
        asm volatile(MFSGD_SOLO_CHAIN_ASM_TEXT(EXTRA_SOLO, SFMA2) MFSGD_SOLO_CHAIN_OPERANDS);
    } else if (wave == 1 && (mode == 0 || mode == 2 || mode == 5)) {
        int spins = 1 << 20, fin = 1;
        asm volatile("" : "+s"(fin));
        constexpr int PADV = mfsgd_pad_helper(LG);
        asm volatile(MFSGD_SOLO_HELPER_ASM_TEXT MFSGD_SOLO_HELPER_OPERANDS);
        if (spins == 0 && lane == 0) cyc[2] = 1;
    } else if ((wave == 1 || wave == 2) && mode == 4) {
        // the two helpers of a cut run: wave 1 follows [0, m) and leaves q alone, wave 2 follows [m, n)
        const int m = (n_steps / 2) & ~1;
        int spins = 1 << 20, fin = wave == 2;
        fin = __builtin_amdgcn_readfirstlane(fin);
        asm volatile("" : "+s"(fin));
        const unsigned ea0 = ea;
        {
            const unsigned ea = wave == 1 ? ea0 : ea0 + m * 16;
            n = __builtin_amdgcn_readfirstlane(wave == 1 ? m : n_steps - m);
            constexpr int PADV = mfsgd_pad_helper(LG);
            asm volatile(MFSGD_SOLO_HELPER_ASM_TEXT MFSGD_SOLO_HELPER_OPERANDS);
        }
        if (spins == 0 && lane == 0) cyc[2] = 1;
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
    if (mode == 6 || mode == 7) t0 = t1 - (unsigned long long)((unsigned)t1 - ((volatile uint32_t*)(smem + CTL_OFF))[1]);  // from the row's arrival
    if (lane == 0) cyc[wave == 2 ? 3 : wave] = t1 - t0;
    __syncthreads();
    for (int x = threadIdx.x; x < NROWS * ROWB / 4; x += blockDim.x) rows_out[x] = ((float*)smem)[x];
    for (int x = threadIdx.x; x < (NSTEP + 2) * 4; x += blockDim.x) ent_out[x] = ((uint32_t*)(smem + ENT_OFF))[x];
}

static float ref_dot(const float* p, const float* q) {
    float s[64];
    for (int c = 0; c < LG; ++c) {
        float t0 = p[4 * c] * q[4 * c], t1 = p[4 * c + 1] * q[4 * c + 1];
        t0 = fmaf(p[4 * c + 2], q[4 * c + 2], t0);
        t1 = fmaf(p[4 * c + 3], q[4 * c + 3], t1);
        s[c] = t0 + t1;
    }
    for (int m = 1; m < LG; m <<= 1) {
        float t[64];
        for (int c = 0; c < LG; ++c) t[c] = s[c] + s[c ^ m];
        memcpy(s, t, sizeof(float) * LG);
    }
    return s[0];
}

// ubench3          : every mode at n = NSTEP, NSTEP - 1, 1, 2, 50, 51; then mode 8, the general loop, at n = 1..33 and 64
//                    (forwarded-q flags and p rows recurring at distance two in its data)
// ubench3 chain    : the chain wave's loop only (modes 0 and 1) at those n and at every n = 1..33 -- every exit of a
//                    tail of up to eight steps and every hand-over from a steady body of 8 or 16, twice over (built with
//                    -DMFSGD_CHAIN_STEADY=8|16, -DMFSGD_PAD_CHAIN_STEADY=0|2|4|6, -DMFSGD_PAD_CHAIN_TAIL=0|2|4|6 and
//                    -DMFSGD_CHAIN_PAIRS=1|2|4: tools/build_ubench.sh); one line per n, the short runs as one line
// ubench3 loops    : the one-wave loops only -- mode 3, the run loop, at every even n = 2..34 and the longest, then mode 8
int main(int argc, char** argv) {
    const bool loops_only = argc > 1 && strcmp(argv[1], "loops") == 0;
    const bool chain_only = argc > 1 && strcmp(argv[1], "chain") == 0;
    const bool lone_only = argc > 1 && strcmp(argv[1], "lone") == 0;
    std::vector<int> lengths = {NSTEP, NSTEP - 1, 1, 2, 50, 51};
    if (chain_only || lone_only)
        for (int n = 3; n <= 33; ++n) lengths.push_back(n);
    if (loops_only) {
        lengths = {NSTEP};
        for (int n = 2; n <= 34; n += 2) lengths.push_back(n);
    }
    const int KP = 4 * LG;
    std::vector<float> rows((size_t)NROWS * KP), ref;
    uint32_t seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / (float)(1 << 24); };
    for (int r = 0; r <= NSTEP; ++r)
        for (int f = 0; f < KP; ++f) rows[(size_t)r * KP + f] = rnd() * 0.25f;
    for (int f = 0; f < KP; ++f) rows[(size_t)(NSTEP + 1) * KP + f] = 0.f;
    const float lr = 0.01f, c = 1.0f - 0.01f * 0.05f;
    // steps visit the p rows in a scrambled order
    std::vector<int> prow(NSTEP);
    for (int t = 0; t < NSTEP; ++t) prow[t] = (t * 7) % NSTEP;
    std::vector<float> rr(NSTEP);
    std::vector<uint32_t> ent((NSTEP + 2) * 4, 0);
    auto slots = [&](int pr) { return (uint32_t)(pr * LG) | ((uint32_t)(NSTEP * LG) << 16); };
    // entry t = {slots_{t+1}, mailbox_t, lr * r_t, r_t}; header = {slots_0, 0, 0, 0} (run_asm.hpp)
    ent[0] = slots(prow[0]);
    for (int t = 0; t < NSTEP; ++t) {
        rr[t] = 1.0f + 4.0f * rnd();
        const float lrr = lr * rr[t];
        memcpy(&ent[(t + 1) * 4 + 2], &lrr, 4);
        ent[(t + 1) * 4 + 0] = t + 1 < NSTEP ? slots(prow[t + 1]) : slots(NSTEP + 1);
        ent[(t + 1) * 4 + 1] = 0xFFFFFFFFu;
        memcpy(&ent[(t + 1) * 4 + 3], &rr[t], 4);
    }
    ent[(NSTEP + 1) * 4 + 0] = slots(NSTEP + 1);
    ent[(NSTEP + 1) * 4 + 1] = 0xFFFFFFFFu;
    // host restatement
    ref = rows;
    float* q = &ref[(size_t)NSTEP * KP];
    for (int t = 0; t < NSTEP; ++t) {
        float* p = &ref[(size_t)prow[t] * KP];
        const float dot = ref_dot(p, q), s = fmaf(-lr, dot, lr * rr[t]);
        for (int f = 0; f < KP; ++f) {
            const float po = p[f], qo = q[f];
            p[f] = fmaf(s, qo, c * po);
            q[f] = fmaf(s, po, c * qo);
        }
    }
    float *d_in, *d_out;
    uint32_t *d_ent, *d_ent_out;
    unsigned long long* d_cyc;
    (void)hipMalloc(&d_in, rows.size() * 4);
    (void)hipMalloc(&d_out, rows.size() * 4);
    (void)hipMalloc(&d_ent, ent.size() * 4);
    (void)hipMalloc(&d_ent_out, ent.size() * 4);
    (void)hipMalloc(&d_cyc, 32);
    (void)hipMemcpy(d_in, rows.data(), rows.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_ent, ent.data(), ent.size() * 4, hipMemcpyHostToDevice);
    const size_t lds = (size_t)NROWS * ROWB + (NSTEP + 2) * 16 + (size_t)(NSTEP + 2) * GS * 16 + 16;
    // modes 6 / 7: the q row as its mailbox holds it ({value, tag} granules), the abort word, the mailbox it is posted to
    const unsigned want_tag = (5u << 16) | 3u;
    std::vector<unsigned long long> mb(KP), posted(KP);
    for (int f = 0; f < KP; ++f) {
        uint32_t bits;
        memcpy(&bits, &rows[(size_t)NSTEP * KP + f], 4);
        mb[f] = ((unsigned long long)want_tag << 32) | bits;
    }
    unsigned long long *d_mb, *d_post;
    unsigned* d_abw;
    (void)hipMalloc(&d_mb, KP * 8);
    (void)hipMalloc(&d_post, KP * 8);
    (void)hipMalloc(&d_abw, 4);
    (void)hipMemcpy(d_mb, mb.data(), KP * 8, hipMemcpyHostToDevice);
    (void)hipMemset(d_abw, 0, 4);
    (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    // mode 2: mailboxes pre-filled with the reference's s_t -> the helper's own pace
    std::vector<uint32_t> ent2 = ent;
    {
        std::vector<float> r2 = rows;
        float* qq = &r2[(size_t)NSTEP * KP];
        for (int t = 0; t < NSTEP; ++t) {
            float* p = &r2[(size_t)prow[t] * KP];
            const float dot = ref_dot(p, qq), s = fmaf(-lr, dot, lr * rr[t]);
            memcpy(&ent2[(t + 1) * 4 + 1], &s, 4);
            for (int f = 0; f < KP; ++f) {
                const float po = p[f], qo = qq[f];
                p[f] = fmaf(s, qo, c * po);
                qq[f] = fmaf(s, po, c * qo);
            }
        }
    }
    // mode 3: the same chain as run-loop entries {slots, r, lr*r, ce}, slot 0 live, other slots idle
    std::vector<uint32_t> run((NSTEP + 2) * GS * 4, 0);
    for (int t = 0; t < NSTEP + 2; ++t)
        for (int g = 0; g < GS; ++g) {
            uint32_t* e = &run[(size_t)(t * GS + g) * 4];
            const float one = 1.0f;
            if (g == 0 && t < NSTEP) {
                const float lrr = lr * rr[t];
                e[0] = slots(prow[t]);
                memcpy(&e[1], &rr[t], 4);
                memcpy(&e[2], &lrr, 4);
                memcpy(&e[3], &c, 4);
            } else {
                e[0] = (uint32_t)((NSTEP + 1) * LG) | ((uint32_t)((g == 0 ? NSTEP : NSTEP + 1) * LG) << 16) | 0x80000000u;
                memcpy(&e[3], &one, 4);
            }
        }
    uint32_t* d_run;
    (void)hipMalloc(&d_run, run.size() * 4);
    (void)hipMemcpy(d_run, run.data(), run.size() * 4, hipMemcpyHostToDevice);
    struct Res { double chain, helper; int bad; };
    std::vector<Res> res[8];
    for (auto& v : res) v.resize(NSTEP + 1);
    for (int mode = 0; mode < (chain_only ? 2 : 8); ++mode)
        for (int n : lengths) {
            if ((mode == 3 && (n & 1)) || (mode == 4 && n < 8) || (loops_only && mode != 3)) continue;
            if (lone_only ? (mode != 0 && mode < 6) : (!chain_only && mode >= 6 && n > 2 && n < 50)) continue;
            (void)hipMemcpy(d_ent, (mode == 2 ? ent2 : ent).data(), ent.size() * 4, hipMemcpyHostToDevice);
            unsigned long long best[2] = {~0ull, ~0ull}, h[4];
            std::vector<float> out(rows.size());
            for (int rep = 0; rep < 5; ++rep) {
                (void)hipMemset(d_cyc, 0, 32);
                (void)hipMemset(d_post, 0, KP * 8);
                hipLaunchKernelGGL(k, dim3(1), dim3(mode == 4 ? 192 : 128), lds, 0, d_in, d_ent, d_out, d_ent_out, d_cyc, n, lr, c, mode, d_run, prow[0],
                                   d_mb, d_abw, d_post, want_tag);
                (void)hipMemcpy(h, d_cyc, 32, hipMemcpyDeviceToHost);
                if (h[2]) puts(h[2] == 2 ? "chain wave gave up!" : "helper gave up!");
                if (mode == 4 && h[3] > h[1]) h[1] = h[3];  // cut run: the later of the two helpers
                for (int w = 0; w < 2; ++w) best[w] = h[w] < best[w] ? h[w] : best[w];
            }
            (void)hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost);
            int bad = 0;
            if (mode != 1) {  // the reference for n steps (mode 0: p row of step 0 was updated in front of the run)
                std::vector<float> r2 = rows;
                if (mode == 5 || mode == 7)
                    for (int f = 0; f < KP; ++f) r2[(size_t)prow[0] * KP + f] += 1.0f;
                float* qq = &r2[(size_t)NSTEP * KP];
                for (int t = 0; t < n; ++t) {
                    float* p = &r2[(size_t)prow[t] * KP];
                    const float dot = ref_dot(p, qq), s = fmaf(-lr, dot, lr * rr[t]);
                    for (int f = 0; f < KP; ++f) {
                        const float po = p[f], qo = qq[f];
                        p[f] = fmaf(s, qo, c * po);
                        qq[f] = fmaf(s, po, c * qo);
                    }
                }
                bad = memcmp(out.data(), r2.data(), out.size() * 4) != 0;
                if (mode >= 6) {  // ... and the row as it was posted: {q after n steps, tag + 1}
                    (void)hipMemcpy(posted.data(), d_post, KP * 8, hipMemcpyDeviceToHost);
                    for (int f = 0; f < KP; ++f) {
                        uint32_t bits;
                        memcpy(&bits, &qq[f], 4);
                        bad |= posted[f] != (((unsigned long long)(want_tag + 1u) << 32) | bits);
                    }
                }
            }
            if (chain_only || lone_only) {  // one line per n below
                res[mode][n] = {(double)best[0], (double)best[1], bad};
                continue;
            }
            printf("L=%d mode=%d (%s) n=%d: chain %.1f cycles/step, helper %.1f cycles/step%s\n", LG, mode,
                   mode == 1 ? "chain alone" : mode == 6 ? "lone-tile start: q from its mailbox in registers, chain + helper, from arrival" : mode == 7 ? "lone-tile start, p row of step 0 updated in front of the run" : mode == 4 ? "cut run: chain + two helpers" : mode == 2 ? "helper alone" : mode == 3 ? "one-wave run loop" : mode == 5 ? "chain + helper, p row of step 0 updated in front of the run" : "chain + helper", n, (double)best[0] / n, (double)best[1] / n,
                   mode == 1 ? "" : (bad ? "  MISMATCH" : "  bit-exact"));
        }
    if (!chain_only && !lone_only) {
        // mode 8: the general loop.  Group g keeps three q rows of its own (the pool's last 3 GS rows) and visits them
        // 0 0 1 0 2 0 0 1 ...: the second of two visits in a row is flagged as forwarded (bit 31 of its slots word), the
        // others recur at distance two or three; its p rows are fresh ones, every third step the row of two steps before.
        const int NG = 64;
        static_assert((NG + 1) * GS + 3 * GS <= NSTEP, "general mode: rows");
        auto prow_g = [&](int t, int g) { return (t % 3 == 2 ? t - 2 : t) * GS + g; };
        auto qrow_g = [&](int t, int g) { const int pat[5] = {0, 0, 1, 0, 2}; return NSTEP - 1 - (g * 3 + pat[t % 5]); };
        std::vector<uint32_t> gen((NSTEP + 2) * GS * 4, 0);
        std::vector<float> rg((size_t)NG * GS);
        int flags = 0, dist2 = 0;
        for (int t = 0; t < NSTEP + 2; ++t)
            for (int g = 0; g < GS; ++g) {
                uint32_t* e = &gen[(size_t)(t * GS + g) * 4];
                if (t < NG) {
                    const float r = rg[(size_t)t * GS + g] = 1.0f + 4.0f * rnd(), lrr = lr * r;
                    const bool fwd = t > 0 && qrow_g(t, g) == qrow_g(t - 1, g);
                    e[0] = (uint32_t)(prow_g(t, g) * LG) | ((uint32_t)(qrow_g(t, g) * LG) << 16) | (fwd ? 0x80000000u : 0u);
                    memcpy(&e[1], &r, 4);
                    memcpy(&e[2], &lrr, 4);
                    memcpy(&e[3], &c, 4);
                    flags += fwd;
                    dist2 += t >= 2 && prow_g(t, g) == prow_g(t - 2, g);
                } else {
                    e[0] = (uint32_t)((NSTEP + 1) * LG) | ((uint32_t)((NSTEP + 1) * LG) << 16);
                }
            }
        (void)hipMemcpy(d_run, gen.data(), gen.size() * 4, hipMemcpyHostToDevice);
        std::vector<int> glen;
        for (int n = 1; n <= 33; ++n) glen.push_back(n);
        glen.push_back(NG);
        int exact = 0, wrong = 0;
        std::vector<double> cyc_n(NG + 1, 0.0);
        for (int n : glen) {
            unsigned long long best = ~0ull, h[4];
            for (int rep = 0; rep < 5; ++rep) {
                (void)hipMemset(d_cyc, 0, 32);
                hipLaunchKernelGGL(k, dim3(1), dim3(128), lds, 0, d_in, d_ent, d_out, d_ent_out, d_cyc, n, lr, c, 8, d_run, prow[0], d_mb, d_abw,
                                   d_post, want_tag);
                (void)hipMemcpy(h, d_cyc, 32, hipMemcpyDeviceToHost);
                best = h[0] < best ? h[0] : best;
            }
            std::vector<float> out(rows.size()), r2 = rows;
            (void)hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost);
            for (int t = 0; t < n; ++t)
                for (int g = 0; g < GS; ++g) {
                    float *p = &r2[(size_t)prow_g(t, g) * KP], *qq = &r2[(size_t)qrow_g(t, g) * KP];
                    const float dot = ref_dot(p, qq), s = fmaf(-lr, dot, lr * rg[(size_t)t * GS + g]);
                    for (int f = 0; f < KP; ++f) {
                        const float po = p[f], qo = qq[f];
                        p[f] = fmaf(s, qo, c * po);
                        qq[f] = fmaf(s, po, c * qo);
                    }
                }
            (memcmp(out.data(), r2.data(), out.size() * 4) != 0 ? wrong : exact)++;
            cyc_n[n] = (double)best;
        }
        printf("L=%d mode=8 (one-wave general loop, pad %d; %d forwarded-q flags, %d p rows at distance two in the data) n=1..33 and %d: %d bit-exact, %d MISMATCH\n",
               LG, mfsgd_pad_gen(LG), flags, dist2, NG, exact, wrong);
        printf("L=%d mode=8 n=%d: %.1f cycles/step; cycles per run at n = 1 2 3 4 5 8 16 33:", LG, NG, cyc_n[NG] / NG);
        for (int n : {1, 2, 3, 4, 5, 8, 16, 33}) printf(" %.0f", cyc_n[n]);
        printf("  (step of a long run: %.1f)\n", (cyc_n[NG] - cyc_n[32]) / (NG - 32));
    }
    if (chain_only) {
        // pair = the later of the two waves of mode 0; alone = mode 1; the short runs as one line (cycles per RUN, alone)
        int exact = 0, wrong = 0;
        for (int n = 1; n <= 33; ++n) (res[0][n].bad ? wrong : exact)++;
        for (int n : {NSTEP, NSTEP - 1, 50, 51, 2, 1}) {
            const Res &p = res[0][n], &a = res[1][n];
            printf("L=%d P=%d pairs=%d pad=%d/%d n=%d: pair %.1f, chain in the pair %.1f, chain alone %.1f cycles/step%s\n", LG, mfsgd_chain_steady(),
                   mfsgd_chain_pairs(), mfsgd_pad_chain_steady(LG), mfsgd_pad_chain_tail(LG), n, (p.helper > p.chain ? p.helper : p.chain) / n, p.chain / n, a.chain / n, p.bad ? "  MISMATCH" : "  bit-exact");
        }
        printf("L=%d P=%d pairs=%d pad=%d/%d n=1..33: %d bit-exact, %d MISMATCH; chain alone, cycles per run at n = 7 8 9 15 16 17 31 32 33:", LG,
               mfsgd_chain_steady(), mfsgd_chain_pairs(), mfsgd_pad_chain_steady(LG), mfsgd_pad_chain_tail(LG), exact, wrong);
        for (int n : {7, 8, 9, 15, 16, 17, 31, 32, 33}) printf(" %.0f", res[1][n].chain);
        printf("\n");
    }
    if (lone_only) {
        // whole-run cycles (the later of the two waves / the chain wave), LDS start (mode 0) beside the lone-tile start (mode 6)
        int exact = 0, wrong = 0;
        for (int n = 1; n <= 33; ++n) {
            (res[6][n].bad ? wrong : exact)++;
            (res[7][n].bad ? wrong : exact)++;
        }
        for (int n : {1, 2, 50, 51, NSTEP - 1, NSTEP}) {
            const Res &a = res[0][n], &b = res[6][n];
            printf("L=%d lone n=%d: cycles per run, pair / chain wave: LDS start %.0f / %.0f, lone-tile start %.0f / %.0f (%+.0f / %+.0f)%s\n", LG, n,
                   a.helper > a.chain ? a.helper : a.chain, a.chain, b.helper > b.chain ? b.helper : b.chain, b.chain,
                   (b.helper > b.chain ? b.helper : b.chain) - (a.helper > a.chain ? a.helper : a.chain), b.chain - a.chain,
                   a.bad || b.bad || res[7][n].bad ? "  MISMATCH" : "  bit-exact");
        }
        printf("L=%d lone n=1..33, modes 6 and 7: %d bit-exact, %d MISMATCH\n", LG, exact, wrong);
    }
    return 0;
}
