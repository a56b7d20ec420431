// Slot costs of the solo chain step (csrc/run_asm.hpp, MFSGD_SOLO_CHAIN_HALF): one wave alone on its SIMD runs a chain
// of dependent v_add_f32_dpp -- each needs two wait states behind the VALU write it reads -- with the two slots behind
// every add filled by one candidate at a time, and prints cycles per link beyond the all-s_nop chain:
//     {X, s_nop 0}   one slot holds the candidate, the other an s_nop 0 (how the LDS instructions sit in the step)
//     {X, X}         both slots hold it (two destinations, no dependence between them or on the chain)
// Then the dependent latency of v_pk_fma_f32 -> v_pk_mul_f32 -> v_pk_fma_f32 against v_fma_f32 -> v_mul_f32 -> v_fma_f32
// (one chain, and the two halves of the packed registers as two interleaved chains), and what ONE independent VALU
// instruction costs between the last DPP add and the v_fma_f32 that reads it (where a step has no wait state to fill).
// Nothing here is checked for its values: the operands are 1.0 and 0.0 and stay so.
//     tools/build_ubench.sh && tools/bin/ub5
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define DPP "v_add_f32_dpp v132, v132, v132 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
constexpr int LINKS = 16;  // per pass (straight line), PASSES passes: the loop end is in the baseline too
constexpr int PASSES = 64;

// v113 / v139 row address (this lane's 16 bytes of a 256-byte row at LDS 0), v138 entry address (LDS 1024, every lane
// the same, as in the step); v[100:107] = 1.0, v[116:117] = v128 = v130 = v132 = 0.  The LDS block is 4096 bytes; the
// highest byte touched is 1024 + 4 * 6 + 3.
#define UB5_CLOBBERS                                                                                                    \
    "memory", "scc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", \
        "v113", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", \
        "v130", "v131", "v132", "v138", "v139", "v140", "v141", "v142", "v143", "v144", "v145"
#define UB5_KERNEL(NAME, BODY)                                                                                          \
    __global__ void __launch_bounds__(64) NAME(unsigned long long* cyc, float c) {                                      \
        __shared__ __attribute__((aligned(16))) unsigned char smem[4096];                                               \
        for (int x = threadIdx.x; x < 1024; x += 64) ((uint32_t*)smem)[x] = 0u;                                         \
        __syncthreads();                                                                                                \
        const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;                       \
        const unsigned rb = base + (threadIdx.x % 16) * 16, ea = base + 1024;                                           \
        const uint64_t c2 = ((uint64_t)__builtin_bit_cast(uint32_t, c) << 32) | __builtin_bit_cast(uint32_t, c);        \
        const unsigned c1 = (unsigned)c2;                                                                               \
        unsigned long long t0, t1;                                                                                      \
        int n = PASSES;                                                                                                 \
        asm volatile(                                                                                                   \
            "v_mov_b32 v113, %[rb]\n\tv_mov_b32 v139, %[rb]\n\tv_mov_b32 v138, %[ea]\n\t"                               \
            ".irp r,100,101,102,103,104,105,106,107\n\tv_mov_b32 v\\r, 1.0\n\t.endr\n\t"                                \
            ".irp r,116,117,128,130,131,132\n\tv_mov_b32 v\\r, 0\n\t.endr\n\t"                                          \
            "s_memtime %[t0]\n\ts_waitcnt lgkmcnt(0)\n\t"                                                               \
            ".p2align 6\n\t"                                                                                            \
            "1:\n\t"                                                                                                    \
            ".rept %c[links]\n\t" BODY ".endr\n\t"                                                                      \
            "s_sub_u32 %[n], %[n], 1\n\t"                                                                               \
            "s_cmp_lg_u32 %[n], 0\n\t"                                                                                  \
            "s_cbranch_scc1 1b\n\t"                                                                                     \
            "s_waitcnt lgkmcnt(0)\n\t"                                                                                  \
            "s_memtime %[t1]\n\ts_waitcnt lgkmcnt(0)\n\t"                                                               \
            : [n] "+s"(n), [t0] "=&s"(t0), [t1] "=&s"(t1)                                                               \
            : [rb] "v"(rb), [ea] "v"(ea), [c2] "s"(c2), [c] "s"(c1), [links] "n"(LINKS)                                 \
            : UB5_CLOBBERS);                                                                                            \
        if (threadIdx.x == 0) cyc[0] = t1 - t0;                                                                         \
    }

#define NOP0 "s_nop 0\n\t"
#define MUL_A "v_mul_f32 v122, %[c], v100\n\t"
#define MUL_B "v_mul_f32 v124, %[c], v102\n\t"
#define FMA_A "v_fma_f32 v122, v100, v104, v106\n\t"
#define FMA_B "v_fma_f32 v124, v102, v105, v107\n\t"
#define PKMUL_A "v_pk_mul_f32 v[122:123], v[100:101], %[c2]\n\t"
#define PKMUL_B "v_pk_mul_f32 v[124:125], v[102:103], %[c2]\n\t"
#define PKFMA_A "v_pk_fma_f32 v[122:123], v[100:101], v[104:105], v[106:107]\n\t"
#define PKFMA_B "v_pk_fma_f32 v[124:125], v[102:103], v[104:105], v[106:107]\n\t"
#define MAD_A "v_mad_u32_u16 v113, v117, 16, v139\n\t"
#define MAD_B "v_mad_u32_u16 v112, v116, 16, v139\n\t"
#define WAITC "s_waitcnt lgkmcnt(0)\n\t"
#define RD128 "ds_read_b128 v[108:111], v113\n\t"
#define RD2 "ds_read2_b32 v[118:119], v138 offset0:6 offset1:4\n\t"
#define WR2 "ds_write2_b32 v138, v130, v128 offset0:1 offset1:5\n\t"

UB5_KERNEL(k_nop, DPP NOP0 NOP0)
UB5_KERNEL(k_mul1, DPP MUL_A NOP0)
UB5_KERNEL(k_mul2, DPP MUL_A MUL_B)
UB5_KERNEL(k_fma1, DPP FMA_A NOP0)
UB5_KERNEL(k_fma2, DPP FMA_A FMA_B)
UB5_KERNEL(k_pkmul1, DPP PKMUL_A NOP0)
UB5_KERNEL(k_pkmul2, DPP PKMUL_A PKMUL_B)
UB5_KERNEL(k_pkfma1, DPP PKFMA_A NOP0)
UB5_KERNEL(k_pkfma2, DPP PKFMA_A PKFMA_B)
UB5_KERNEL(k_mad1, DPP MAD_A NOP0)
UB5_KERNEL(k_mad2, DPP MAD_A MAD_B)
UB5_KERNEL(k_wait1, DPP WAITC NOP0)
UB5_KERNEL(k_wait2, DPP WAITC WAITC)
UB5_KERNEL(k_rd128_1, DPP RD128 NOP0)
UB5_KERNEL(k_rd128_2, DPP RD128 RD128)
UB5_KERNEL(k_rd2_1, DPP RD2 NOP0)
UB5_KERNEL(k_rd2_2, DPP RD2 RD2)
UB5_KERNEL(k_wr2_1, DPP WR2 NOP0)
UB5_KERNEL(k_wr2_2, DPP WR2 WR2)
// the slots as the step fills them: LDS read + multiply, and the packed form of the same
UB5_KERNEL(k_rd128_mul, DPP RD128 MUL_A)
UB5_KERNEL(k_rd128_pkmul, DPP RD128 PKMUL_A)
UB5_KERNEL(k_rd2_mul, DPP RD2 MUL_A)
UB5_KERNEL(k_mad_mul, DPP MAD_A MUL_A)
UB5_KERNEL(k_mad_pkmul, DPP MAD_A PKMUL_A)

// Groups of LDS instructions in the gaps of a whole step (four links, two slots each, as the run and general loops fill
// them): the same instructions in one gap, in two and in three.  Every body below is four links long, so the printed
// figure is per STEP, beyond four links of {s_nop 0, s_nop 0} with the same VALU fillers and no LDS instruction.
#define RD32 "ds_read_b32 v118, v138 offset:32\n\t"
#define RD32B "ds_read_b32 v119, v138 offset:24\n\t"
#define RD64 "ds_read_b64 v[118:119], v138 offset:24\n\t"
#define RD128B "ds_read_b128 v[140:143], v139\n\t"
#define WR128 "ds_write_b128 v113, v[104:107]\n\t"
#define PKMUL_C "v_pk_mul_f32 v[126:127], v[104:105], %[c2]\n\t"
#define PKMUL_D "v_pk_mul_f32 v[144:145], v[106:107], %[c2]\n\t"
// run loop: no LDS; three groups of reads as it was ({p}, {}, {slots, entry}); the three reads in the first gap
UB5_KERNEL(k_step_run_none, DPP PKMUL_A NOP0 DPP PKMUL_B PKMUL_C DPP PKMUL_D NOP0 DPP NOP0 NOP0)
UB5_KERNEL(k_step_run_old, DPP RD128 PKMUL_A DPP PKMUL_B PKMUL_C DPP RD32 RD64 DPP PKMUL_D NOP0)
UB5_KERNEL(k_step_run_new, DPP RD128 RD32 RD64 DPP PKMUL_B PKMUL_C DPP PKMUL_A PKMUL_D DPP NOP0 NOP0)
UB5_KERNEL(k_step_run_gap2, DPP PKMUL_A PKMUL_D DPP RD128 RD32 RD64 DPP PKMUL_B PKMUL_C DPP NOP0 NOP0)
// general loop: reads {p}, {q}, {}, {slots, lr*r} as it was; all four in the first gap; two gaps of two
UB5_KERNEL(k_step_gen_none, DPP MAD_A PKMUL_A DPP PKMUL_B PKMUL_C DPP PKMUL_D NOP0 DPP NOP0 NOP0)
UB5_KERNEL(k_step_gen_old, DPP RD128 MAD_A DPP RD128B PKMUL_A DPP PKMUL_B PKMUL_C DPP PKMUL_D RD32 RD32B)
UB5_KERNEL(k_step_gen_four, DPP RD128 RD128B RD32 RD32B DPP PKMUL_A PKMUL_B DPP PKMUL_C PKMUL_D DPP MAD_A NOP0)
UB5_KERNEL(k_step_gen_2x2, DPP RD128 RD128B DPP RD32 RD32B DPP PKMUL_A PKMUL_B DPP PKMUL_C PKMUL_D MAD_A)
// the chain wave's post: {read, read} in a gap and the ds_write2_b32 behind the last link; the write in that gap too
UB5_KERNEL(k_step_post_own, DPP RD128 RD2 DPP PKMUL_A NOP0 DPP PKMUL_B NOP0 DPP NOP0 NOP0 PKMUL_C PKMUL_D WR2)
UB5_KERNEL(k_step_post_gap, DPP RD128 RD2 WR2 DPP PKMUL_A NOP0 DPP PKMUL_B NOP0 DPP NOP0 NOP0 PKMUL_C PKMUL_D)
UB5_KERNEL(k_step_post_none, DPP PKMUL_A NOP0 DPP PKMUL_B NOP0 DPP NOP0 NOP0 DPP NOP0 NOP0 PKMUL_C PKMUL_D)
// the helper's write of p' and read of the next row outside any gap: apart (VALU between them), adjacent
UB5_KERNEL(k_step_wr_rd_apart, DPP NOP0 NOP0 PKMUL_A PKMUL_B WR128 MAD_B PKMUL_C RD128B PKMUL_D)
UB5_KERNEL(k_step_wr_rd_adj, DPP NOP0 NOP0 PKMUL_A PKMUL_B MAD_B PKMUL_C WR128 RD128B PKMUL_D)
UB5_KERNEL(k_step_wr_rd_none, DPP NOP0 NOP0 PKMUL_A PKMUL_B MAD_B PKMUL_C PKMUL_D)

// dependent latency, three operations per link
UB5_KERNEL(k_lat_pk, "v_pk_fma_f32 v[100:101], v[104:105], v[116:117], v[100:101]\n\t"
                     "v_pk_mul_f32 v[100:101], v[100:101], v[104:105]\n\t"
                     "v_pk_fma_f32 v[100:101], v[100:101], v[104:105], v[116:117]\n\t")
UB5_KERNEL(k_lat_plain, "v_fma_f32 v100, v104, v116, v100\n\t"
                        "v_mul_f32 v100, v100, v104\n\t"
                        "v_fma_f32 v100, v100, v104, v116\n\t")
UB5_KERNEL(k_lat_plain2, "v_fma_f32 v100, v104, v116, v100\n\tv_fma_f32 v101, v105, v117, v101\n\t"
                         "v_mul_f32 v100, v100, v104\n\tv_mul_f32 v101, v101, v105\n\t"
                         "v_fma_f32 v100, v100, v104, v116\n\tv_fma_f32 v101, v101, v105, v117\n\t")
// pk_mul / pk_fma / add (the chunk dot of a step) against its plain form: mul, mul, fma, fma, add
UB5_KERNEL(k_dot_pk, "v_pk_mul_f32 v[120:121], v[104:105], v[100:101]\n\t"
                     "v_pk_fma_f32 v[120:121], v[106:107], v[102:103], v[120:121]\n\t"
                     "v_add_f32 v100, v120, v121\n\t")
UB5_KERNEL(k_dot_plain, "v_mul_f32 v120, v104, v100\n\tv_mul_f32 v121, v105, v100\n\t"
                        "v_fma_f32 v120, v106, v102, v120\n\tv_fma_f32 v121, v107, v103, v121\n\t"
                        "v_add_f32 v100, v120, v121\n\t")
// behind the last DPP add of a step: VALU write, two wait states, DPP add, [one independent VALU,] the v_fma_f32 that reads it
#define TAILLINK(X) "v_add_f32 v132, v130, v130\n\ts_nop 1\n\t" DPP X "v_fma_f32 v130, v131, v132, v116\n\t"
UB5_KERNEL(k_tail_none, TAILLINK(""))
UB5_KERNEL(k_tail_mul, TAILLINK(MUL_A))
UB5_KERNEL(k_tail_pkmul, TAILLINK(PKMUL_A))

struct Case {
    const char* name;
    void (*one)(unsigned long long*, float);
    void (*two)(unsigned long long*, float);
};

static double run(void (*kern)(unsigned long long*, float), unsigned long long* d_cyc) {
    unsigned long long best = ~0ull, h = 0;
    for (int rep = 0; rep < 7; ++rep) {
        hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, 0, d_cyc, 0.9995f);
        if (hipMemcpy(&h, d_cyc, 8, hipMemcpyDeviceToHost) != hipSuccess) {
            puts("hipMemcpy failed");
            exit(1);
        }
        best = h < best ? h : best;
    }
    return (double)best / (LINKS * PASSES);
}

int main() {
    unsigned long long* d_cyc;
    if (hipMalloc(&d_cyc, 8) != hipSuccess) return 1;
    const double base = run(k_nop, d_cyc);
    printf("chain of dependent v_add_f32_dpp, two slots behind each, one wave on its SIMD, %d links: %.2f cycles per link with {s_nop 0, s_nop 0}\n",
           LINKS * PASSES, base);
    printf("cycles per link beyond that      {X, s_nop 0}   {X, X}\n");
    const std::vector<Case> cases = {{"v_mul_f32", k_mul1, k_mul2},          {"v_fma_f32", k_fma1, k_fma2},
                                     {"v_pk_mul_f32", k_pkmul1, k_pkmul2},    {"v_pk_fma_f32", k_pkfma1, k_pkfma2},
                                     {"v_mad_u32_u16", k_mad1, k_mad2},       {"s_waitcnt (satisfied)", k_wait1, k_wait2},
                                     {"ds_read_b128", k_rd128_1, k_rd128_2},  {"ds_read2_b32", k_rd2_1, k_rd2_2},
                                     {"ds_write2_b32", k_wr2_1, k_wr2_2}};
    for (const Case& cs : cases) printf("%-28s %+12.2f %+10.2f\n", cs.name, run(cs.one, d_cyc) - base, run(cs.two, d_cyc) - base);
    printf("the step's own pairs: {ds_read_b128, v_mul_f32} %+.2f  {ds_read_b128, v_pk_mul_f32} %+.2f  {ds_read2_b32, v_mul_f32} %+.2f  "
           "{v_mad_u32_u16, v_mul_f32} %+.2f  {v_mad_u32_u16, v_pk_mul_f32} %+.2f\n",
           run(k_rd128_mul, d_cyc) - base, run(k_rd128_pkmul, d_cyc) - base, run(k_rd2_mul, d_cyc) - base, run(k_mad_mul, d_cyc) - base,
           run(k_mad_pkmul, d_cyc) - base);
    {
        const double run0 = run(k_step_run_none, d_cyc), gen0 = run(k_step_gen_none, d_cyc), post0 = run(k_step_post_none, d_cyc),
                     wr0 = run(k_step_wr_rd_none, d_cyc);
        printf("groups of LDS instructions in a step of four links, cycles per step beyond the same step without them:\n");
        printf("  run loop      {p} {} {slots, entry} (three gaps, as it was) %+.2f   {p, slots, entry} in the first gap %+.2f   in the second gap %+.2f\n",
               run(k_step_run_old, d_cyc) - run0, run(k_step_run_new, d_cyc) - run0, run(k_step_run_gap2, d_cyc) - run0);
        printf("  general loop  {p} {q} {} {slots, lr*r} (as it was) %+.2f   {p, q, slots, lr*r} in the first gap %+.2f   {p, q} {slots, lr*r} %+.2f\n",
               run(k_step_gen_old, d_cyc) - gen0, run(k_step_gen_four, d_cyc) - gen0, run(k_step_gen_2x2, d_cyc) - gen0);
        printf("  chain post    {read, read} and ds_write2_b32 behind the step %+.2f   {read, read, write2} in one gap %+.2f\n",
               run(k_step_post_own, d_cyc) - post0, run(k_step_post_gap, d_cyc) - post0);
        printf("  helper        ds_write_b128, VALU, ds_read_b128 outside a gap %+.2f   adjacent %+.2f\n", run(k_step_wr_rd_apart, d_cyc) - wr0,
               run(k_step_wr_rd_adj, d_cyc) - wr0);
    }
    printf("dependent latency, cycles per operation: pk_fma -> pk_mul -> pk_fma %.2f, fma -> mul -> fma %.2f, the two halves as two interleaved chains %.2f per pair\n",
           run(k_lat_pk, d_cyc) / 3, run(k_lat_plain, d_cyc) / 3, run(k_lat_plain2, d_cyc) / 3);
    printf("chunk dot, cycles per link: pk_mul, pk_fma, add %.2f; mul, mul, fma, fma, add %.2f\n", run(k_dot_pk, d_cyc), run(k_dot_plain, d_cyc));
    const double tail = run(k_tail_none, d_cyc);
    printf("add, s_nop 1, DPP add, [X,] fma reading it: %.2f cycles per link; X = v_mul_f32 %+.2f, X = v_pk_mul_f32 %+.2f\n", tail,
           run(k_tail_mul, d_cyc) - tail, run(k_tail_pkmul, d_cyc) - tail);
    return 0;
}
