// run_asm.hpp -- hand-scheduled gfx950 rating loops: the run loop (up to G resident items, one wave)
// and, first described here, the loops of a SOLO run: one item's
// chain of dependent updates, split between the wave that owns the sub-cell (the CHAIN wave:
// dot -> s -> q', nothing else) and one copy wave of the same workgroup on another SIMD (the
// HELPER: re-runs the cheap q recurrence from the posted s and does everything that is not on
// the chain -- p' = fma(s, q, c p), its store, and the final store of q).
//
// A solo run of n steps is a compact stream of 16-byte entries in the LDS schedule image:
//     [header][entry 0] ... [entry n-1][terminator]
//     entry t   = { slots_{t+1},  mailbox_t,  lr * r_t,  r_t }      ([r3] order: {slots, mailbox} is an aligned 8-byte
//     header    = { slots_0,      0,          0,         0   }       unit, see the helper wave below)
//     slots_t   = p-row LDS address | q-row LDS address << 16 (16-byte units); slots_n (in entry
//                 n-1 and in the terminator) addresses an all-zero row
//     mailbox_t = 0xFFFFFFFF in the schedule; the chain wave overwrites it with the bits of s_t,
//                 which is how the helper learns that step t has happened and what s_t was.
// The decay factor is the same for every step (there are no idle slots in a solo run), so it is
// an operand (SGPR pair {c, c}), not part of the entry.  Arithmetic is, instruction for
// instruction, DESIGN.md section 3: the pair of waves produces the bits the one-wave C++ form of the run (cell.hpp, Cell::apply) does.
//
// [r2, late] s of an even and the following odd step are posted TOGETHER (one ds_write2_b32 behind the odd
// step; a last odd-numbered step is posted alone): the chain wave issues half an LDS write per step less.
// (A long run can be cut in two -- the chain wave stores q into its LDS row between the halves, a second copy wave
// follows the second half from there and the first helper leaves q alone, %[fin] = 0: tools/ubench3 mode 4.  Measured
// and not used by the product: the helper is the slower of the pair at 16 lanes per rating, but a third wave on the
// LDS slows the chain wave by what the second helper gains.)
//
// Every loop here has ONE form: what is in this file is what the product runs (the pads, the chain loop's steady
// steps and its tail's pairs per pass below are the only build-time knobs, for tools/ubench3.hip).  Included by
// cell.hpp, whose wrappers bind the operands, and by tools/ubench3.hip, which times the loops against each other in isolation.
#pragma once

// The loops below are a few 64-byte instruction-cache lines long and their cycle count per pass depends on
// where the loop head sits inside a 32-byte fetch window (tools/ubench3.hip built with -DMFSGD_PAD_*=n;
// period 8 instructions).  Cycles per step at 0 / 2 / 4 / 6 s_nops past a 64-byte boundary:
//     solo pair   L = 16: 136.1 137.5 133.7 138.8    L = 32: 165.4 168.6 174.3 178.0    L = 64: 173.4 175.4 170.3 176.4
//     run loop    L = 16: 145.6 143.6 149.6 151.6    L = 32: 174.5 174.5 182.4 180.4    L = 64: 177.8 177.7 181.7 183.7
// The run loop with its idle slots masked (the loop below; profiles/run_idle_mask_ubench3.log, pad 2): L = 16: 157.6, the
// loop without the mask at 143.6 in that session.
// The solo pair before the steady body (s posted in pairs, the chain wave's body four A/B pairs long; at the longest n the
// microbenchmark holds -- 300 / 200 / 120 steps; profiles/chain_unroll_ubench3.log, the pair +- 1.5 from run to run):
//     solo pair   L = 16: 124.7 125.6 125.1 125.4    L = 32: 144.8 147.7 147.2 147.0    L = 64: 162.3 157.7 165.7 160.7
//     chain alone L = 16: 118.3 120.3 120.3 120.3    L = 32: 138.2 140.2 140.2 140.2    L = 64: 152.8 148.9 154.9 150.8
// The chain wave's loop with a steady body of P steps without exits in front of that four-pair loop, now its tail (see
// MFSGD_SOLO_CHAIN_ASM_TEXT; profiles/chain_steady_ubench3.log, same n, the parent's loop at 118.3 / 138.2 / 148.8 alone
// and 125.0 / 145.7 / 158.5 as a pair in that session), at 0 / 2 / 4 / 6 s_nops in front of the STEADY head:
//     chain alone, P = 8   L = 16: 113.1 113.1 114.1 114.6    L = 32: 127.7 127.7 128.8 129.2    L = 64: 141.3 141.4 142.4 142.9
//     chain alone, P = 16  L = 16: 111.8 111.9 112.3 112.5    L = 32: 126.7 126.8 127.3 127.5    L = 64: 140.6 140.7 141.2 141.4
//     solo pair,   P = 8   L = 16: 118.7 118.7 118.1 117.9    L = 32: 134.0 136.0 137.3 137.4    L = 64: 150.4 150.5 152.3 151.7
//     solo pair,   P = 16  L = 16: 118.9 119.6 119.4 120.3    L = 32: 133.4 134.0 134.1 133.4    L = 64: 150.0 148.2 149.0 149.9
// and in front of the TAIL head (P = 8, steady pad 0; the tail decides runs shorter than P and the last steps of the others:
// chain alone at n = 50, cycles per step):
//     L = 16: 123.0 123.0 123.5 123.4    L = 32: 136.8 136.5 137.0 137.0    L = 64: 148.2 148.3 148.8 148.4
// The chain wave's two LDS reads behind ONE DPP add and the helper's two reads adjacent (see MFSGD_SOLO_CHAIN_HALF and
// MFSGD_SOLO_HELPER_PAIR; profiles/chain_scale_ubench3.log, same n, the parent's loops at 111.8 / 127.1 / 141.2 alone and
// 118.5-121.6 / 132.4-132.8 / 148.5-148.7 as a pair in the sessions of that log), at 0 / 2 / 4 / 6 s_nops in front of the
// STEADY head (helper as in the parent), the TAIL head (chain alone at n = 50) and the HELPER's head (the pair):
//     chain alone, steady  L = 16: 101.9 101.9 102.4 102.6    L = 32: 119.1 119.2 119.7 119.9    L = 64: 133.3 133.4 133.9 134.1
//     chain alone, tail    L = 16: 112.1 112.0 112.5 112.5    L = 32: 128.8 128.6 129.0 129.0    L = 64: 140.5 140.6 141.0 140.6
//     solo pair,   helper  L = 16: 119.2 109.5 113.3 117.0    L = 32: 122.8 125.3 124.1 124.3    L = 64: 142.1 141.8 141.3 141.2
// The run loop's and the general loop's LDS reads of a step as ONE group behind the first DPP add (see MFSGD_RUN_LOOP_ASM_TEXT
// and MFSGD_GEN_HALF; profiles/loop_groups_ubench.log: tools/ubench3 modes 3 and 8, one wave, cycles per step at the longest
// n -- 300 / 200 / 120 run steps with the idle slots masked, 64 general steps -- the parent's loops at 157.7 / 188.4 / 193.5
// and 226.2 / 260.4 / 258.5 in that session, alternating, every figure repeating to 0.1), at 0 / 2 / 4 / 6 s_nops:
//     run loop      L = 16: 147.7 149.6 151.7 153.6    L = 32: 178.5 180.6 182.6 184.5    L = 64: 183.6 185.6 187.9 189.7
//     general loop  L = 16: 212.2 214.4 220.4 216.2    L = 32: 244.6 236.4 244.5 252.4    L = 64: 242.5 244.6 250.6 244.9
// Every loop head is therefore placed explicitly (operands [pad] / [pads], assembly-time constants): the product
// runs the layout that was timed, whatever code the compiler puts in front of the loop.
constexpr int mfsgd_pad_run(int lanes) {
#ifdef MFSGD_PAD_RUN
    return MFSGD_PAD_RUN;
#else
    return 0;  // the loop with its three reads in one group, last table above (profiles/loop_groups_ubench.log)
#endif
}
constexpr int mfsgd_pad_gen(int lanes) {
#ifdef MFSGD_PAD_GEN
    return MFSGD_PAD_GEN;
#else
    return lanes == 32 ? 2 : 0;  // the loop with its four reads in one group, last table above
#endif
}
// The chain wave's loop has two heads (the steady body and the tail, see MFSGD_SOLO_CHAIN_ASM_TEXT), each placed on its own.
constexpr int mfsgd_pad_chain_steady(int lanes) {
#ifdef MFSGD_PAD_CHAIN_STEADY
    return MFSGD_PAD_CHAIN_STEADY;
#else
    return 0;
#endif
}
constexpr int mfsgd_pad_chain_tail(int lanes) {
#ifdef MFSGD_PAD_CHAIN_TAIL
    return MFSGD_PAD_CHAIN_TAIL;
#else
    return lanes == 64 ? 2 : 0;  // the four-pair body with its exits, second table above (profiles/chain_unroll_ubench3.log)
#endif
}
constexpr int mfsgd_pad_helper(int lanes) {
#ifdef MFSGD_PAD_HELPER
    return MFSGD_PAD_HELPER;
#else
    return lanes == 16 ? 2 : lanes == 32 ? 0 : 6;  // the pair loop with its two reads adjacent (profiles/chain_scale_ubench3.log)
#endif
}
// A/B pairs of solo chain steps per pass of the chain wave's TAIL loop, an assembly-time constant like the pads (1, 2 or 4:
// a taken backward branch costs this loop about 9 cycles more than a not-taken exit -- about 15 against 6, DESIGN.md
// section 5 -- which is 4.7 cycles per step at one pair per pass and 1.2 at four).
constexpr int mfsgd_chain_pairs() {
#ifdef MFSGD_CHAIN_PAIRS
    return MFSGD_CHAIN_PAIRS;
#else
    return 4;
#endif
}
// Steps per pass of the chain wave's STEADY body (P: even, at most 16), which runs while at least P steps remain.
constexpr int mfsgd_chain_steady() {
#ifdef MFSGD_CHAIN_STEADY
    return MFSGD_CHAIN_STEADY;
#else
    return 16;  // third table above
#endif
}
static_assert(mfsgd_chain_steady() % 2 == 0 && mfsgd_chain_steady() >= 2 && mfsgd_chain_steady() <= 16, "steady body: A/B pairs, at most eight");
#define MFSGD_LOOP_ALIGN ".p2align 6\n\t.rept %c[pad]\n\ts_nop 0\n\t.endr\n\t"
#define MFSGD_LOOP_ALIGN_STEADY ".p2align 6\n\t.rept %c[pads]\n\ts_nop 0\n\t.endr\n\t"

// ---- hand-scheduled run loop (gfx950) ---------------------------------------------------
// `pairs` x 2 run steps of one wave: resident q rows in v[100:103] / v[140:143] (alternating),
// one p row prefetched a step ahead, entry words fetched one / two steps ahead.  Per step:
// 3 dot ops, 4 DPP adds whose two required wait states are filled with the independent
// scale / address / LDS-issue instructions (the address is one v_mad_u32_u16: low 16 bits of
// the entry word x 16 + row base), 1 fma for s, 4 pk_fma, 1 store.  Arithmetic is
// instruction for instruction what Cell::apply's run_step does in C++ (which remains the
// reference for it and the RMSE path).  Fixed VGPRs v100..v143 are declared clobbered.
//   ea      : LDS byte address of this lane group's entry of run step 0 (entry stride `EST`)
//   rowbase : LDS byte address of row slot 0 plus this lane's 16-byte offset inside a row
// Register map (the text is a macro, which cannot carry comments line by line):
//   v138 entry pointer, v139 row base; v114 / v115 entry word `slots` of the even / odd step in
//   flight, v[116:117] / v[118:119] its {lr*r, ce}; v112 / v113 p-row address, v[104:107] / v[108:111]
//   p row (prefetched one step ahead); v[100:103] <-> v[140:143] resident q rows; v[120:121] chunk
//   products, v132 dot, v[122:125] ce*q, v[126:129] ce*p, v130 s, v[134:137] p'.
//   Step: wait for p and the entry words -> chunk dot (pk_mul, pk_fma, add) -> 4 DPP adds
//   (quad_perm xor 1, xor 2, row_half_mirror, row_mirror) interleaved with the next p address, the
//   ce scalings, the p prefetch and the entry prefetches -> EXTRA: the xor-16 / xor-32 levels for
//   32 / 64 lanes per rating -> s = fma(-lr, dot, lr*r) -> q' = fma(s, p, ce*q), p' = fma(s, q, ce*p)
//   -> store p'.  The prologue loads step 0; a harmless rewrite of an entry word keeps "one LDS
//   operation behind the reads" so that every pass can use the same counted wait.
//   IDLE slots (bit 31 of the slots word: p = the all-zero row, r = 0, ce = 1) keep their resident row by construction,
//   not by arithmetic: ce*q is computed straight into the other q set and q' = fma(s, p, .) accumulated onto it in place
//   with the idle lanes masked out of exec (%[live] = lanes of the live slots, %[sv] = the wave's exec; from the last DPP
//   add to the two q' operations), so an idle slot's row is 1*q whatever s is.  Left to fma(0, p, 1*q), a resident row
//   holding Inf or NaN gave 0*Inf = NaN as its dot and turned NaN as a whole; the NaN p' went into the zero row, and from
//   there into the resident rows of other idle slots.  p' is still computed and stored for every lane (the counted waits
//   rely on the store): an idle slot's goes to its dummy row, which nothing that reaches P or Q reads any more.
//   (A lane group is one or two whole DPP rows, and the partner rows of the swap levels belong to the same group.)
//   LDS operations of one step, in issue order: read p(t+1), read slots(t+2), read {lr*r, ce}(t+1) -- ONE group, in the
//   two wait states behind the FIRST DPP add, where the chain wave's reads measured best (an LDS instruction behind VALU
//   work costs the wave about 8 cycles per group of adjacent ones, tools/ubench5.hip; the entry reads used to be a group
//   of their own behind the third add) -- then, behind the arithmetic, write p'(t).  The order is the one the step always
//   had, so the counted wait is too: LDS operations of a wave complete in order, and "all but the last one" at the top of
//   step t + 1 leaves only the write of p'(t) outstanding -- p(t+1), slots(t+2) and {lr*r, ce}(t+1) are in registers.
//   The prefetch of p(t+1) is issued in front of the store of p'(t) as before (a p row may recur at distance two, never
//   at distance one).  What the moved reads overwrite is dead by then: v114 / v115 (slots of the step in flight) is last
//   read by the v_cmp at the top of its step, v[116:117] / v[118:119] by the other half's SFMA.  The wait states in
//   front of the four adds hold, in order: {p address, ce*q01}, {the three reads}, {ce*p01, ce*p23}, {ce*q23, s_and_saveexec}.
#define MFSGD_RUN_LOOP_ASM_TEXT(EXTRA, SFMA) \
        "v_mov_b32 v138, %[ea]\n\t" \
        "v_mov_b32 v131, %[lr]\n\t" \
        "v_mov_b32 v139, %[rb]\n\t" \
        "ds_read_b32 v114, v138\n\t" \
        "ds_read_b64 v[116:117], v138 offset:8\n\t" \
        "ds_read_b32 v115, v138 offset:%c[e1]\n\t" \
        "v_mov_b32 v100, %[q0]\n\t" \
        "v_mov_b32 v101, %[q1]\n\t" \
        "v_mov_b32 v102, %[q2]\n\t" \
        "v_mov_b32 v103, %[q3]\n\t" \
        "s_waitcnt lgkmcnt(2)\n\t" \
        "v_and_b32 v133, 0xffff, v114\n\t" \
        "v_lshl_add_u32 v112, v133, 4, v139\n\t" \
        "ds_read_b128 v[104:107], v112\n\t" \
        "ds_write_b32 v138, v114\n\t" \
        MFSGD_LOOP_ALIGN \
        "1:\n\t" \
        "s_waitcnt lgkmcnt(1)\n\t" \
        "v_cmp_lt_i32_e64 %[live], -1, v114\n\t" \
        "v_pk_mul_f32 v[120:121], v[104:105], v[100:101]\n\t" \
        "v_pk_fma_f32 v[120:121], v[106:107], v[102:103], v[120:121]\n\t" \
        "v_add_f32 v132, v120, v121\n\t" \
        "v_mad_u32_u16 v113, v115, 16, v139\n\t" \
        "v_pk_mul_f32 v[140:141], v[116:117], v[100:101] op_sel:[1,0]\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "ds_read_b128 v[108:111], v113\n\t" \
        "ds_read_b32 v114, v138 offset:%c[e2]\n\t" \
        "ds_read_b64 v[118:119], v138 offset:%c[e1p8]\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[126:127], v[116:117], v[104:105] op_sel:[1,0]\n\t" \
        "v_pk_mul_f32 v[128:129], v[116:117], v[106:107] op_sel:[1,0]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[142:143], v[116:117], v[102:103] op_sel:[1,0]\n\t" \
        "s_and_saveexec_b64 %[sv], %[live]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        EXTRA \
        SFMA("116") \
        "v_pk_fma_f32 v[140:141], v[130:131], v[104:105], v[140:141] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[142:143], v[130:131], v[106:107], v[142:143] op_sel_hi:[0,1,1]\n\t" \
        "s_mov_b64 exec, %[sv]\n\t" \
        "v_pk_fma_f32 v[134:135], v[130:131], v[100:101], v[126:127] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[136:137], v[130:131], v[102:103], v[128:129] op_sel_hi:[0,1,1]\n\t" \
        "s_sub_u32 %[n], %[n], 1\n\t" \
        "ds_write_b128 v112, v[134:137]\n\t" \
        "s_waitcnt lgkmcnt(1)\n\t" \
        "v_cmp_lt_i32_e64 %[live], -1, v115\n\t" \
        "v_pk_mul_f32 v[120:121], v[108:109], v[140:141]\n\t" \
        "v_pk_fma_f32 v[120:121], v[110:111], v[142:143], v[120:121]\n\t" \
        "v_add_f32 v132, v120, v121\n\t" \
        "v_mad_u32_u16 v112, v114, 16, v139\n\t" \
        "v_pk_mul_f32 v[100:101], v[118:119], v[140:141] op_sel:[1,0]\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "ds_read_b128 v[104:107], v112\n\t" \
        "ds_read_b32 v115, v138 offset:%c[e3]\n\t" \
        "ds_read_b64 v[116:117], v138 offset:%c[e2p8]\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[126:127], v[118:119], v[108:109] op_sel:[1,0]\n\t" \
        "v_pk_mul_f32 v[128:129], v[118:119], v[110:111] op_sel:[1,0]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[102:103], v[118:119], v[142:143] op_sel:[1,0]\n\t" \
        "s_and_saveexec_b64 %[sv], %[live]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        EXTRA \
        SFMA("118") \
        "v_pk_fma_f32 v[100:101], v[130:131], v[108:109], v[100:101] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[102:103], v[130:131], v[110:111], v[102:103] op_sel_hi:[0,1,1]\n\t" \
        "s_mov_b64 exec, %[sv]\n\t" \
        "v_pk_fma_f32 v[134:135], v[130:131], v[140:141], v[126:127] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[136:137], v[130:131], v[142:143], v[128:129] op_sel_hi:[0,1,1]\n\t" \
        "v_add_u32 v138, %c[e2], v138\n\t" \
        "s_cmp_lg_u32 %[n], 0\n\t" \
        "ds_write_b128 v113, v[134:137]\n\t" \
        "s_cbranch_scc1 1b\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_mov_b32 %[q0], v100\n\t" \
        "v_mov_b32 %[q1], v101\n\t" \
        "v_mov_b32 %[q2], v102\n\t" \
        "v_mov_b32 %[q3], v103\n\t"

// xor-16 / xor-32 levels of the dot reduction for L = 32 / 64 (see swap_add16 / swap_add32): v133 is free
#define MFSGD_SWAP_ADD16 "v_mov_b32 v133, v132\n\ts_nop 1\n\tv_permlane16_swap_b32 v132, v133\n\ts_nop 1\n\tv_add_f32 v132, v132, v133\n\t"
#define MFSGD_SWAP_ADD32 "v_mov_b32 v133, v132\n\ts_nop 1\n\tv_permlane32_swap_b32 v132, v133\n\ts_nop 1\n\tv_add_f32 v132, v132, v133\n\t"
// Both levels at once for L = 64 (one rating per wave, so the dot is wave-uniform): after the 16-lane
// reduction every lane of row r holds S_r; row_bcast:15 adds lane 15 of rows 0 / 2 into rows 1 / 3
// (S0+S1, S2+S3), row_bcast:31 adds lane 31 into rows 2 / 3, so lane 63 holds (S2+S3)+(S0+S1) -- the
// bits of the contract's tree, addition being commutative -- and a v_readlane broadcasts it.  Two DPP
// adds and two moves on the dependent chain instead of two five-instruction swap levels.
#define MFSGD_BCAST_ADD64 "s_nop 1\n\tv_add_f32_dpp v132, v132, v132 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\tv_add_f32_dpp v132, v132, v132 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 0\n\tv_readlane_b32 vcc_lo, v132, 63\n\t"
// The same idea for the xor-16 level of a SOLO run at L = 32 (one rating per wave there too: both lane groups
// work on it): row_bcast:15 puts S0+S1 into row 1 (lane 31), a v_readlane hands it on as a scalar.
#define MFSGD_BCAST_ADD32 "s_nop 1\n\tv_add_f32_dpp v132, v132, v132 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 0\n\tv_readlane_b32 vcc_lo, v132, 31\n\t"
// s = fma(-lr, dot, lr*r): the dot in v132 (every lane of the group holds it), or -- after
// MFSGD_BCAST_ADD64 -- in vcc_lo, with lr in v131 (one scalar operand per VALU instruction on gfx9)
#define MFSGD_SFMA_V(LRR) "v_fma_f32 v130, -%[lr], v132, v" LRR "\n\t"
#define MFSGD_SFMA_S(LRR) "v_fma_f32 v130, -v131, vcc_lo, v" LRR "\n\t"
// the same with the destination named (the solo chain keeps s of an even and an odd step apart)
#define MFSGD_SFMA2_V(S, LRR) "v_fma_f32 v" S ", -%[lr], v132, v" LRR "\n\t"
#define MFSGD_SFMA2_S(S, LRR) "v_fma_f32 v" S ", -v131, vcc_lo, v" LRR "\n\t"
#define MFSGD_RUN_LOOP_ASM_OPERANDS                                                                                   \
    : [q0] "+v"(q[0]), [q1] "+v"(q[1]), [q2] "+v"(q[2]), [q3] "+v"(q[3]), [n] "+s"(pairs), [live] "=&s"(live),        \
      [sv] "=&s"(sv)                                                                                                  \
    : [ea] "v"(ea), [rb] "v"(rowbase), [lr] "s"(lr), [e1] "n"(EST), [e2] "n"(2 * EST), [e3] "n"(3 * EST),              \
      [e1p8] "n"(EST + 8), [e2p8] "n"(2 * EST + 8), [pad] "n"(PADV)                                                                    \
    : "memory", "scc", "vcc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", \
      "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125",  \
      "v126", "v127", "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139",  \
      "v140", "v141", "v142", "v143"



// ---- hand-scheduled GENERAL step loop (gfx950) [r3] -------------------------------------------
// `n` general steps of one wave (cell.hpp Cell::apply, `step`): every lane group applies one rating per step --
// both rows come from LDS, both go back -- and consecutive steps are independent except where the packer flagged a
// q row as forwarded (bit 31 of the next entry's slots word: the same item in the same lane slot; its new row is taken
// from registers, the LDS copy read ahead of the write being stale).  The compiler's schedule of the C++ step waits
// twice per step for LDS reads it issued a few instructions earlier (~335 cycles per step of G ratings, measured
// in situ); here the rows of step t + 1 and the entry words of step t + 2 are fetched under the arithmetic of step
// t with counted waits, as in the run loop above: 24 VALU + 6 LDS instructions per step.
//   entry (16 bytes per slot and step): {slots = p address | q address << 16 | forward flag << 31 (16-byte units),
//   rating, lr * rating, decay}; the decay factor of a general step is the uniform c (operand c2 = {c, c}).
// Register map (two sets, A = even steps, B = odd steps):
//   v138 entry pointer, v139 row base + this lane's 16-byte offset; v114 / v115 slots word whose rows are fetched
//   during an odd / even step; v116 / v117 lr*r of the even / odd step; v112, v148 / v113, v149 p and q address of
//   set A / B; v[104:107], v[100:103] / v[108:111], v[140:143] p and q row of set A / B; v[144:147] the q row read
//   ahead (selected against the forwarded q'); v[120:121] chunk products, v132 dot, v[122:125] c*q, v[126:129] c*p,
//   v130 s, v[134:137] p'; q' is computed straight into the OTHER set's q registers.
// LDS operations of one step, in issue order: read p(t+1), read q(t+1), read slots(t+2), read lr*r(t+1) -- ONE group of
// four adjacent reads in the wait states behind the FIRST DPP add (an LDS instruction behind VALU work costs the wave
// about 8 cycles per group of adjacent ones, tools/ubench5.hip; they used to be three groups, one behind each of the
// first, second and fourth add), with the q address computed in front of that add beside the p address -- then, behind
// the arithmetic, write p'(t), write q'(t).  The order is the one the step always had, so the counts are too: LDS
// operations of a wave complete in order, six are outstanding behind the writes, "all but the last four" has p(t+1) and
// q(t+1) in registers (the select behind the writes) and "all but the last two" at the top of the next step has the two
// entry words as well, only the writes still in flight.  The stale-read rule holds as before: the rows of step t + 1
// are read in front of the writes of step t, and the forwarded q' is selected behind them.  What the moved reads
// overwrite is dead by then: the slots word of the step in flight (its addresses were computed a step ago; the flag
// test reads the NEXT step's word), lr*r of the other set, and v[144:147], last read by the previous step's select.
// Hazards, as the packer guarantees (schedule.cpp, "Eligibility"): a p row never appears in two consecutive steps
// of a wave; a q row only in the same lane slot, flagged.  Arithmetic: instruction for instruction DESIGN.md section 3.
#define MFSGD_GEN_HALF(P0, P1, P2, P3, Q0, Q1, Q2, Q3, PADDR, QADDR, NP0, NP3, NQ0, NQ1, NQ2, NQ3, NPADDR, NQADDR, SLOT_NEXT, \
                       SLOT_NEXT2, OFF_SLOT2, LRR, LRR_NEXT, OFF_LRR1, EXTRA, SFMA)                                              \
        "s_waitcnt lgkmcnt(2)\n\t" \
        "v_pk_mul_f32 v[120:121], v[" P0 ":" P1 "], v[" Q0 ":" Q1 "]\n\t" \
        "v_pk_fma_f32 v[120:121], v[" P2 ":" P3 "], v[" Q2 ":" Q3 "], v[120:121]\n\t" \
        "v_add_f32 v132, v120, v121\n\t" \
        "v_mad_u32_u16 v" NPADDR ", v" SLOT_NEXT ", 16, v139\n\t" \
        "v_bfe_u32 v133, v" SLOT_NEXT ", 16, 15\n\t" \
        "v_lshl_add_u32 v" NQADDR ", v133, 4, v139\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "ds_read_b128 v[" NP0 ":" NP3 "], v" NPADDR "\n\t" \
        "ds_read_b128 v[144:147], v" NQADDR "\n\t" \
        "ds_read_b32 v" SLOT_NEXT2 ", v138 offset:" OFF_SLOT2 "\n\t" \
        "ds_read_b32 v" LRR_NEXT ", v138 offset:" OFF_LRR1 "\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[122:123], v[" Q0 ":" Q1 "], %[c2]\n\t" \
        "v_pk_mul_f32 v[124:125], v[" Q2 ":" Q3 "], %[c2]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[126:127], v[" P0 ":" P1 "], %[c2]\n\t" \
        "v_pk_mul_f32 v[128:129], v[" P2 ":" P3 "], %[c2]\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        EXTRA \
        SFMA(LRR) \
        "v_pk_fma_f32 v[" NQ0 ":" NQ1 "], v[130:131], v[" P0 ":" P1 "], v[122:123] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[" NQ2 ":" NQ3 "], v[130:131], v[" P2 ":" P3 "], v[124:125] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[134:135], v[130:131], v[" Q0 ":" Q1 "], v[126:127] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[136:137], v[130:131], v[" Q2 ":" Q3 "], v[128:129] op_sel_hi:[0,1,1]\n\t" \
        "s_sub_u32 %[n], %[n], 1\n\t" \
        "v_cmp_gt_i32 vcc, 0, v" SLOT_NEXT "\n\t" \
        "ds_write_b128 v" PADDR ", v[134:137]\n\t" \
        "ds_write_b128 v" QADDR ", v[" NQ0 ":" NQ3 "]\n\t" \
        "s_cmp_eq_u32 %[n], 0\n\t" \
        "s_waitcnt lgkmcnt(4)\n\t" \
        "v_cndmask_b32 v" NQ0 ", v144, v" NQ0 ", vcc\n\t" \
        "v_cndmask_b32 v" NQ1 ", v145, v" NQ1 ", vcc\n\t" \
        "v_cndmask_b32 v" NQ2 ", v146, v" NQ2 ", vcc\n\t" \
        "v_cndmask_b32 v" NQ3 ", v147, v" NQ3 ", vcc\n\t"

// `ea`: LDS byte address of this lane group's entry of general step 0 (entry stride EST), n >= 1 steps.
#define MFSGD_GEN_LOOP_ASM_TEXT(EXTRA, SFMA) \
        "v_mov_b32 v138, %[ea]\n\t" \
        "v_mov_b32 v131, %[lr]\n\t" \
        "v_mov_b32 v139, %[rb]\n\t" \
        "ds_read_b32 v114, v138\n\t" \
        "ds_read_b32 v116, v138 offset:8\n\t" \
        "ds_read_b32 v115, v138 offset:%c[e1]\n\t" \
        "s_waitcnt lgkmcnt(2)\n\t" \
        "v_mad_u32_u16 v112, v114, 16, v139\n\t" \
        "v_bfe_u32 v133, v114, 16, 15\n\t" \
        "v_lshl_add_u32 v148, v133, 4, v139\n\t" \
        "ds_read_b128 v[104:107], v112\n\t" \
        "ds_read_b128 v[100:103], v148\n\t" \
        "ds_write_b32 v138, v114\n\t" \
        "ds_write_b32 v138, v114\n\t" \
        MFSGD_LOOP_ALIGN \
        "1:\n\t" \
        MFSGD_GEN_HALF("104", "105", "106", "107", "100", "101", "102", "103", "112", "148", "108", "111", "140", "141", "142", "143", \
                       "113", "149", "115", "114", "%c[e2]", "116", "117", "%c[e1p8]", EXTRA, SFMA) \
        "s_cbranch_scc1 2f\n\t" \
        MFSGD_GEN_HALF("108", "109", "110", "111", "140", "141", "142", "143", "113", "149", "104", "107", "100", "101", "102", "103", \
                       "112", "148", "114", "115", "%c[e3]", "117", "116", "%c[e2p8]", EXTRA, SFMA) \
        "v_add_u32 v138, %c[e2], v138\n\t" \
        "s_cbranch_scc0 1b\n\t" \
        "2:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t"

#define MFSGD_GEN_LOOP_ASM_OPERANDS                                                                                    \
    : [n] "+s"(n)                                                                                                      \
    : [ea] "v"(ea), [rb] "v"(rowbase), [lr] "s"(lr), [c2] "s"(c2), [e1] "n"(EST), [e2] "n"(2 * EST), [e3] "n"(3 * EST), \
      [e1p8] "n"(EST + 8), [e2p8] "n"(2 * EST + 8), [pad] "n"(PADV)                                                    \
    : "memory", "scc", "vcc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", \
      "v112", "v113", "v114", "v115", "v116", "v117", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127",  \
      "v128", "v129", "v130", "v131", "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141",  \
      "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149"

// ---- chain wave -------------------------------------------------------------------------------
// v138 entry pointer (-> entry t at the top of half A), v139 row base + this lane's 16-byte offset;
// v[100:103] q (updated in place); v[104:107] / v[108:111] p row of the even / odd step (prefetched
// a step ahead); v[116:117] / v[118:119] {lr*r, next slots} of the even / odd step; v113 p address;
// v[120:121] chunk products, v132 dot, v[122:125] c*q, v130 s.
// The two wait states behind each of the four DPP adds hold, in order: {p address, c*q01}, {the p-row read, the entry
// read}, {c*q23, s_nop}, GAP.  Any VALU, SALU or s_nop filler costs such a slot nothing (tools/ubench5.hip,
// profiles/chain_slots_ubench.log: packed or not); what costs is an LDS instruction -- 8 cycles per GAP that holds
// one, and no more for a second one beside it -- so the step's two reads share ONE gap (one read in each of two gaps,
// as this step had them: 111.8 instead of 101.9 cycles at L = 16; both in the next gap down: 107.8).  They are issued in
// the order they always were, so the counted waits and what the helper sees are unchanged.
#define MFSGD_SOLO_CHAIN_HALF(P0, P1, P2, P3, N0, N1, N2, N3, ELRR, ESLOT, NEXTE, OFF_NEXT, WAIT, S, S1, GAP, EXTRA, SFMA) \
        "s_waitcnt lgkmcnt(" WAIT ")\n\t" \
        "v_pk_mul_f32 v[120:121], v[" P0 ":" P1 "], v[100:101]\n\t" \
        "v_pk_fma_f32 v[120:121], v[" P2 ":" P3 "], v[102:103], v[120:121]\n\t" \
        "v_add_f32 v132, v120, v121\n\t" \
        "v_mad_u32_u16 v113, v" ESLOT ", 16, v139\n\t" \
        "v_pk_mul_f32 v[122:123], v[100:101], %[c2]\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "ds_read_b128 v[" N0 ":" N3 "], v113\n\t" \
        "ds_read2_b32 v[" NEXTE "], v138 " OFF_NEXT "\n\t" \
        "v_add_f32_dpp v132, v132, v132 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_pk_mul_f32 v[124:125], v[102:103], %[c2]\n\t" \
        "s_nop 0\n\t" \
        "v_add_f32_dpp v132, v132, v132 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        GAP \
        "v_add_f32_dpp v132, v132, v132 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        EXTRA \
        SFMA(S, ELRR) \
        "v_pk_fma_f32 v[100:101], v[" S ":" S1 "], v[" P0 ":" P1 "], v[122:123] op_sel_hi:[0,1,1]\n\t" \
        "v_pk_fma_f32 v[102:103], v[" S ":" S1 "], v[" P2 ":" P3 "], v[124:125] op_sel_hi:[0,1,1]\n\t"

// `ea` = LDS byte address of the header entry, `s0` = its slots word (the caller has read it to find the q row; the
// helper wave needs the header in LDS, so the record stays); n >= 1 steps.  The q row is loaded HERE, not by the
// caller: {lr*r_0, slots_1}, p row 0 and q are three LDS reads in flight together, one round trip in front of step 0.
// (The harmless rewrite of the header word keeps "one LDS operation behind the reads", as in the run loop.)
// The loop has TWO bodies built from the same half step.
// STEADY (5:), while at least P = %c[steady] steps remain (mfsgd_chain_steady): P steps in a straight line with no exit
// and no per-step counter -- an s_nop 1 fills the DPP gap where the tail counts -- and, in that gap of the pass's last
// step, n -= P and the compare against P; v138 is bumped and the backward branch taken once per pass.
// TAIL (1:), for the n < P steps that remain (all of a run shorter than P; skipped when none remain): %c[pairs] A/B pairs
// per pass (mfsgd_chain_pairs), every step with its own forward exit test -- after an A step to that step's "post s
// alone" tail (2<j>), after a B step to the end.  The state at the top of either body is that at the top of an A step:
// v138 -> its entry, its p row, its entry words and one LDS write behind them in flight, q in v[100:103].
// Both bodies read ahead and post s of a pair with the same instructions at the same offsets and points of a B step, so
// what the helper sees is what the one-pair loop posts.
#define MFSGD_SOLO_CHAIN_GAP_COUNT "s_sub_u32 %[n], %[n], 1\n\ts_cmp_eq_u32 %[n], 0\n\t"
#define MFSGD_SOLO_CHAIN_GAP_NOP "s_nop 1\n\t"
#define MFSGD_SOLO_CHAIN_GAP_PASS \
        ".if 2 * \\j + 2 < %c[steady]\n\ts_nop 1\n\t.else\n\ts_sub_u32 %[n], %[n], %c[steady]\n\ts_cmp_ge_u32 %[n], %c[steady]\n\t.endif\n\t"
#define MFSGD_SOLO_CHAIN_PAIR(GAP_A, GAP_B, EXIT_A, EXTRA, SFMA) \
        MFSGD_SOLO_CHAIN_HALF("104", "105", "106", "107", "108", "109", "110", "111", "116", "117", "118:119", "offset0:6+8*\\j offset1:4+8*\\j", "1", "130", "131", GAP_A, EXTRA, SFMA) \
        EXIT_A \
        MFSGD_SOLO_CHAIN_HALF("108", "109", "110", "111", "104", "105", "106", "107", "118", "119", "116:117", "offset0:10+8*\\j offset1:8+8*\\j", "0", "128", "129", GAP_B, EXTRA, SFMA) \
        "ds_write2_b32 v138, v130, v128 offset0:1+8*\\j offset1:5+8*\\j\n\t"
// (The two bodies and the tail's "post s alone" exits are a macro of their own: MFSGD_LONE_CHAIN_ASM_TEXT below enters the
// same text from a second prologue.  Entered with scc = "n < P" tested; left at the label 3 that follows it.)
#define MFSGD_SOLO_CHAIN_BODIES(EXTRA, SFMA) \
        "s_cbranch_scc1 1f\n\t" \
        MFSGD_LOOP_ALIGN_STEADY \
        "5:\n\t" \
        ".irp j,0,1,2,3,4,5,6,7\n\t" \
        ".if 2 * \\j < %c[steady]\n\t" \
        MFSGD_SOLO_CHAIN_PAIR(MFSGD_SOLO_CHAIN_GAP_NOP, MFSGD_SOLO_CHAIN_GAP_PASS, "", EXTRA, SFMA) \
        ".endif\n\t" \
        ".endr\n\t" \
        "v_add_u32 v138, %c[sbump], v138\n\t" \
        "s_cbranch_scc1 5b\n\t" \
        "s_cmp_eq_u32 %[n], 0\n\t" \
        "s_cbranch_scc1 3f\n\t" \
        "s_branch 1f\n\t" \
        MFSGD_LOOP_ALIGN \
        "1:\n\t" \
        ".irp j,0,1,2,3\n\t" \
        ".if \\j < %c[pairs]\n\t" \
        MFSGD_SOLO_CHAIN_PAIR(MFSGD_SOLO_CHAIN_GAP_COUNT, MFSGD_SOLO_CHAIN_GAP_COUNT, "s_cbranch_scc1 2\\j\\()f\n\t", EXTRA, SFMA) \
        ".if \\j + 1 < %c[pairs]\n\t" \
        "s_cbranch_scc1 3f\n\t" \
        ".endif\n\t" \
        ".endif\n\t" \
        ".endr\n\t" \
        "v_add_u32 v138, %c[bump], v138\n\t" \
        "s_cbranch_scc0 1b\n\t" \
        "s_branch 3f\n\t" \
        ".irp j,3,2,1,0\n\t" \
        ".if \\j < %c[pairs]\n\t" \
        "2\\j:\n\t" \
        "ds_write_b32 v138, v130 offset:4+32*\\j\n\t" \
        ".if \\j > 0\n\t" \
        "s_branch 3f\n\t" \
        ".endif\n\t" \
        ".endif\n\t" \
        ".endr\n\t"

#define MFSGD_SOLO_CHAIN_ASM_TEXT(EXTRA, SFMA) \
        "v_mov_b32 v138, %[ea]\n\t" \
        "v_mov_b32 v131, %[lr]\n\t" \
        "v_mov_b32 v139, %[rb]\n\t" \
        "ds_read2_b32 v[116:117], v138 offset0:6 offset1:4\n\t" \
        "v_mad_u32_u16 v113, %[s0], 16, v139\n\t" \
        "v_bfe_u32 v133, %[s0], 16, 15\n\t" \
        "ds_read_b128 v[104:107], v113\n\t" \
        "v_lshl_add_u32 v133, v133, 4, v139\n\t" \
        "ds_read_b128 v[100:103], v133\n\t" \
        "ds_write_b32 v138, %[s0]\n\t" \
        "v_add_u32 v138, 16, v138\n\t" \
        "s_cmp_lt_u32 %[n], %c[steady]\n\t" \
        MFSGD_SOLO_CHAIN_BODIES(EXTRA, SFMA) \
        "3:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_mov_b32 %[q0], v100\n\t" \
        "v_mov_b32 %[q1], v101\n\t" \
        "v_mov_b32 %[q2], v102\n\t" \
        "v_mov_b32 %[q3], v103\n\t"

#define MFSGD_SOLO_CHAIN_OPERANDS                                                                                      \
    : [n] "+s"(n), [q0] "=v"(q[0]), [q1] "=v"(q[1]), [q2] "=v"(q[2]), [q3] "=v"(q[3])                                  \
    : [ea] "v"(ea), [rb] "v"(rowbase), [s0] "v"(s0), [lr] "s"(lr), [c2] "s"(c2), [pad] "n"(PADV),                      \
      [pads] "n"(PADS), [pairs] "n"(mfsgd_chain_pairs()), [bump] "n"(32 * mfsgd_chain_pairs()),                         \
      [steady] "n"(mfsgd_chain_steady()), [sbump] "n"(16 * mfsgd_chain_steady())                                       \
    : "memory", "scc", "vcc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", \
      "v113", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v128", "v129", "v130",  \
      "v131", "v132", "v133", "v138", "v139"

// ---- chain wave of a LONE-TILE cell: the row comes out of its mailbox straight into the loop ----------------------
// The persistent kernel's fast lane (epoch.hip, run_ring): the cell is ONE solo run, and its q row
// arrives from another workgroup as 4 L granules {value, tag} in global memory.  This is MFSGD_SOLO_CHAIN_ASM_TEXT
// with a second prologue and a second epilogue around the same bodies, and the wait for the row between the halves of
// the prologue:
//   before the wait   v138 / v131 / v139 as above; {lr*r_0, slots_1} and p row 0 read and WAITED for; the q row's LDS
//                     address in v133; the tags of the post in the odd registers of v[150:157];
//   the wait          every lane loads granules 4 lig .. 4 lig + 3 (8 bytes each, sc1: what the compiler emits for a
//                     relaxed agent-scope atomic load) -- every lane group the same addresses, so all hold the same q --
//                     value of granule j into v100 / v142 / v144 / v146, its tag beside it; every lane tests its four
//                     tags against %[want]; one vcc test for the wave.  A miss: s_sleep 1, and every 256th the abort
//                     word (%[abw]) and the bound of 2^22 polls;
//   arrival           three moves complete q in v[100:103]; ONE ds_write_b128 puts it into the row's LDS slot for the
//                     helper (which reads it only behind s_0, and this wave's LDS operations complete in order: no wait)
//                     and is the "one LDS write behind the reads" the bodies' counted waits expect; ONE s_barrier, at
//                     which the other waves of the workgroup have been waiting; then the bodies.  No VMEM is outstanding.
//   the post          straight behind the last step's q': four moves pair the values with the tags, four 8-byte sc1
//                     stores under the exec mask %[pm] (lanes 0 .. L - 1, or none when the row is not handed on).
//   giving up         (abort word set, or the bound): lane 0 raises the abort word and the LDS word at %[ctl], both are
//                     waited for, the wave joins the barrier and leaves with %[gave] = 1: nothing trained or posted.
// %[prof] != 0 (diagnostic launches): the low word of s_memtime at arrival goes to the LDS word at %[ctl] + 4.
// n >= 1 steps; %[src] / %[dst]: this lane's first granule of the mailbox taken from / posted to.
// (-DMFSGD_LONE_POLL_NO_SLEEP: the poll without its s_sleep 1, a build for the A/B of DESIGN.md section 5 only)
#ifdef MFSGD_LONE_POLL_NO_SLEEP
#define MFSGD_LONE_POLL_SLEEP ""
#else
#define MFSGD_LONE_POLL_SLEEP "s_sleep 1\n\t"
#endif
#define MFSGD_LONE_CHAIN_ASM_TEXT(EXTRA, SFMA) \
        "v_mov_b32 v138, %[ea]\n\t" \
        "v_mov_b32 v131, %[lr]\n\t" \
        "v_mov_b32 v139, %[rb]\n\t" \
        "ds_read2_b32 v[116:117], v138 offset0:6 offset1:4\n\t" \
        "v_mad_u32_u16 v113, %[s0], 16, v139\n\t" \
        "v_bfe_u32 v133, %[s0], 16, 15\n\t" \
        "ds_read_b128 v[104:107], v113\n\t" \
        "v_lshl_add_u32 v133, v133, 4, v139\n\t" \
        "v_add_u32 v138, 16, v138\n\t" \
        "v_mov_b32 v151, %[ptag]\n\t" \
        "v_mov_b32 v153, %[ptag]\n\t" \
        "v_mov_b32 v155, %[ptag]\n\t" \
        "v_mov_b32 v157, %[ptag]\n\t" \
        "v_mov_b32 v149, 0\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "60:\n\t" \
        "global_load_dwordx2 v[100:101], %[src], off sc1\n\t" \
        "global_load_dwordx2 v[142:143], %[src], off offset:8 sc1\n\t" \
        "global_load_dwordx2 v[144:145], %[src], off offset:16 sc1\n\t" \
        "global_load_dwordx2 v[146:147], %[src], off offset:24 sc1\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "v_xor_b32 v101, %[want], v101\n\t" \
        "v_xor_b32 v143, %[want], v143\n\t" \
        "v_xor_b32 v145, %[want], v145\n\t" \
        "v_xor_b32 v147, %[want], v147\n\t" \
        "v_or3_b32 v101, v101, v143, v145\n\t" \
        "v_or_b32 v101, v101, v147\n\t" \
        "v_cmp_ne_u32 vcc, 0, v101\n\t" \
        "s_cbranch_vccz 62f\n\t" \
        MFSGD_LONE_POLL_SLEEP \
        "s_add_u32 %[spins], %[spins], 1\n\t" \
        "s_and_b32 %[t0], %[spins], 0xff\n\t" \
        "s_cbranch_scc1 60b\n\t" \
        "global_load_dword v148, v149, %[abw] sc1\n\t" \
        "s_waitcnt vmcnt(0)\n\t" \
        "v_readfirstlane_b32 %[t0], v148\n\t" \
        "s_cmp_lg_u32 %[t0], 0\n\t" \
        "s_cbranch_scc1 61f\n\t" \
        "s_cmp_le_u32 %[spins], 0x400000\n\t" \
        "s_cbranch_scc1 60b\n\t" \
        "61:\n\t" \
        "v_mov_b32 v148, 1\n\t" \
        "s_mov_b64 %[tmp], exec\n\t" \
        "s_mov_b64 exec, 1\n\t" \
        "global_store_dword v149, v148, %[abw] sc1\n\t" \
        "ds_write_b32 %[ctl], v148\n\t" \
        "s_mov_b64 exec, %[tmp]\n\t" \
        "s_mov_b32 %[gave], 1\n\t" \
        "s_waitcnt vmcnt(0) lgkmcnt(0)\n\t" \
        "s_barrier\n\t" \
        "s_branch 69f\n\t" \
        "62:\n\t" \
        "v_mov_b32 v101, v142\n\t" \
        "v_mov_b32 v102, v144\n\t" \
        "v_mov_b32 v103, v146\n\t" \
        "s_cmp_eq_u32 %[prof], 0\n\t" \
        "s_cbranch_scc1 63f\n\t" \
        "s_memtime %[tmp]\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_mov_b64 v[158:159], %[tmp]\n\t" \
        "ds_write_b32 %[ctl], v158 offset:4\n\t" \
        "63:\n\t" \
        "s_cmp_lt_u32 %[n], %c[steady]\n\t" \
        "ds_write_b128 v133, v[100:103]\n\t" \
        "s_barrier\n\t" \
        MFSGD_SOLO_CHAIN_BODIES(EXTRA, SFMA) \
        "3:\n\t" \
        "v_mov_b32 v150, v100\n\t" \
        "v_mov_b32 v152, v101\n\t" \
        "v_mov_b32 v154, v102\n\t" \
        "v_mov_b32 v156, v103\n\t" \
        "s_and_saveexec_b64 %[tmp], %[pm]\n\t" \
        "global_store_dwordx2 %[dst], v[150:151], off sc1\n\t" \
        "global_store_dwordx2 %[dst], v[152:153], off offset:8 sc1\n\t" \
        "global_store_dwordx2 %[dst], v[154:155], off offset:16 sc1\n\t" \
        "global_store_dwordx2 %[dst], v[156:157], off offset:24 sc1\n\t" \
        "s_mov_b64 exec, %[tmp]\n\t" \
        "69:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t"

#define MFSGD_LONE_CHAIN_OPERANDS                                                                                      \
    : [n] "+s"(n), [spins] "+s"(spins), [gave] "+s"(gave), [tmp] "=&s"(tmp), [t0] "=&s"(t0)                            \
    : [ea] "v"(ea), [rb] "v"(rowbase), [s0] "v"(s0), [lr] "s"(lr), [c2] "s"(c2), [src] "v"(src), [want] "s"(want),     \
      [abw] "s"(abw), [ctl] "v"(ctl), [dst] "v"(dst), [ptag] "s"(ptag), [pm] "s"(pm), [prof] "s"(prof),                \
      [pad] "n"(PADV), [pads] "n"(PADS), [pairs] "n"(mfsgd_chain_pairs()), [bump] "n"(32 * mfsgd_chain_pairs()),        \
      [steady] "n"(mfsgd_chain_steady()), [sbump] "n"(16 * mfsgd_chain_steady())                                       \
    : "memory", "scc", "vcc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", \
      "v113", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v128", "v129", "v130",  \
      "v131", "v132", "v133", "v138", "v139", "v142", "v143", "v144", "v145", "v146", "v147", "v148", "v149", "v150",  \
      "v151", "v152", "v153", "v154", "v155", "v156", "v157", "v158", "v159"

// ---- helper wave ------------------------------------------------------------------------------
// [r3] The helper takes the steps in PAIRS, as the chain wave posts them: ONE ds_read2_b64 fetches {slots_{t+1}, s_t}
// and {slots_{t+2}, s_{t+1}} -- bytes 4..11 of two consecutive entries; the address is 4 modulo 8, which the LDS of
// gfx9 takes in the unaligned mode the driver runs it in -- one poll test per pair (both mailboxes: v_max_u32 is all
// ones iff either is), and the loop counter per pair.  Round 2's loop read {s, slots} per step with a ds_read2_b32 and
// tested per step: 130 cycles per step at 16 lanes per rating against the chain wave's 120, so the pair ran at the
// helper's pace.  A last odd step (posted alone by the chain wave) is a tail of its own.
// v138 -> entry t + 4 at the top of a pair; v139 row base + lane offset; v[100:103] q_t; v[104:107] / v[108:111] p row
// of the pair's first / second step, v112 / v113 their addresses; v[116:119] <-> v[150:153] the pair's words
// {slots_{t+1}, s_t, slots_{t+2}, s_{t+1}} (s is the HIGH half of an aligned register pair: op_sel:[1,0,0]); v140 q
// address; v[122:125] c*q, v[126:129] c*p, v[134:137] p'.  %[spins]: polls left before giving up (the chain wave
// always arrives; the bound only keeps a broken schedule from hanging the GPU) -- on return %[spins] == 0 means it
// gave up and nothing further was written.
// LDS operations of a pair, in issue order: read p_{t+1}, read the next pair's words, write p'_t, read p_{t+2}, write
// p'_{t+1}: "all but the last one" at the top of the next pair has its words and its first p row.  The first two reads
// are ADJACENT instructions (c*p23 behind them, not between them): an LDS instruction that follows VALU work costs the
// wave about 8 cycles and a second one beside it nothing (tools/ubench5.hip, profiles/chain_slots_ubench.log).
// NOTHING of the rows is read before s_0 has been posted: the chain wave runs the general and run steps of its sub-cell
// before the solo run, and they may update the p rows the run is about to use (the helper starts with the sub-round).
// Once s_0 is there they are final -- only the helper writes them.  (A first version of this loop fetched p_0 in its
// prologue, in front of the poll: bit-exact in tools/ubench3 -- which has no general steps -- and wrong in the product
// whenever a user of step 0 also had a general step in the sub-cell.  tools/ubench3 now dirties p_0 first.)
#define MFSGD_SOLO_HELPER_PAIR(TAG, M0, M1, M2, M3, N0, N3) \
        "s_waitcnt lgkmcnt(1)\n\t" \
        "v_max_u32 v133, v" M1 ", v" M3 "\n\t" \
        "v_mad_u32_u16 v113, v" M0 ", 16, v139\n\t" \
        "v_cmp_eq_u32 vcc, -1, v133\n\t" \
        "v_pk_mul_f32 v[126:127], v[104:105], %[c2]\n\t" \
        "s_cbranch_vccnz 7" TAG "f\n\t" \
        "6" TAG ":\n\t" \
        "ds_read_b128 v[108:111], v113\n\t" \
        "ds_read2_b64 v[" N0 ":" N3 "], v138 offset0:4 offset1:6\n\t" \
        "v_pk_mul_f32 v[128:129], v[106:107], %[c2]\n\t" \
        "v_pk_mul_f32 v[122:123], v[100:101], %[c2]\n\t" \
        "v_pk_mul_f32 v[124:125], v[102:103], %[c2]\n\t" \
        "v_pk_fma_f32 v[134:135], v[" M0 ":" M1 "], v[100:101], v[126:127] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[136:137], v[" M0 ":" M1 "], v[102:103], v[128:129] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[100:101], v[" M0 ":" M1 "], v[104:105], v[122:123] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[102:103], v[" M0 ":" M1 "], v[106:107], v[124:125] op_sel:[1,0,0]\n\t" \
        "s_sub_u32 %[n], %[n], 2\n\t" \
        "ds_write_b128 v112, v[134:137]\n\t" \
        "v_mad_u32_u16 v112, v" M2 ", 16, v139\n\t" \
        "s_waitcnt lgkmcnt(2)\n\t" \
        "ds_read_b128 v[104:107], v112\n\t" \
        "v_pk_mul_f32 v[126:127], v[108:109], %[c2]\n\t" \
        "v_pk_mul_f32 v[128:129], v[110:111], %[c2]\n\t" \
        "v_pk_mul_f32 v[122:123], v[100:101], %[c2]\n\t" \
        "v_pk_mul_f32 v[124:125], v[102:103], %[c2]\n\t" \
        "v_pk_fma_f32 v[134:135], v[" M2 ":" M3 "], v[100:101], v[126:127] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[136:137], v[" M2 ":" M3 "], v[102:103], v[128:129] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[100:101], v[" M2 ":" M3 "], v[108:109], v[122:123] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[102:103], v[" M2 ":" M3 "], v[110:111], v[124:125] op_sel:[1,0,0]\n\t" \
        "v_add_u32 v138, 32, v138\n\t" \
        "s_cmp_lt_u32 %[n], 2\n\t" \
        "ds_write_b128 v113, v[134:137]\n\t"

// re-poll of a pair whose s has not been posted yet (out of line)
#define MFSGD_SOLO_HELPER_SLOW(TAG, M0, M1, M3) \
        "7" TAG ":\n\t" \
        "s_sleep 1\n\t" \
        "ds_read2_b64 v[" M0 ":" M3 "], v138 offset1:2\n\t" \
        "s_sub_u32 %[spins], %[spins], 1\n\t" \
        "s_cmp_eq_u32 %[spins], 0\n\t" \
        "s_cbranch_scc1 9f\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_max_u32 v133, v" M1 ", v" M3 "\n\t" \
        "v_cmp_eq_u32 vcc, -1, v133\n\t" \
        "s_cbranch_vccnz 7" TAG "b\n\t" \
        "s_branch 6" TAG "b\n\t"

// the last step of an odd-length run: its s is posted alone, behind the chain wave's loop
#define MFSGD_SOLO_HELPER_TAIL(TAG, M0, M1) \
        "8" TAG ":\n\t" \
        "s_cmp_eq_u32 %[n], 0\n\t" \
        "s_cbranch_scc1 40f\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_pk_mul_f32 v[126:127], v[104:105], %[c2]\n\t" \
        "v_pk_mul_f32 v[128:129], v[106:107], %[c2]\n\t" \
        "v_pk_mul_f32 v[122:123], v[100:101], %[c2]\n\t" \
        "v_pk_mul_f32 v[124:125], v[102:103], %[c2]\n\t" \
        "3" TAG ":\n\t" \
        "v_cmp_eq_u32 vcc, -1, v" M1 "\n\t" \
        "s_cbranch_vccz 2" TAG "f\n\t" \
        "s_sleep 1\n\t" \
        "ds_read_b32 v" M1 ", v138 offset:4\n\t" \
        "s_sub_u32 %[spins], %[spins], 1\n\t" \
        "s_cmp_eq_u32 %[spins], 0\n\t" \
        "s_cbranch_scc1 9f\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "s_branch 3" TAG "b\n\t" \
        "2" TAG ":\n\t" \
        "v_pk_fma_f32 v[134:135], v[" M0 ":" M1 "], v[100:101], v[126:127] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[136:137], v[" M0 ":" M1 "], v[102:103], v[128:129] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[100:101], v[" M0 ":" M1 "], v[104:105], v[122:123] op_sel:[1,0,0]\n\t" \
        "v_pk_fma_f32 v[102:103], v[" M0 ":" M1 "], v[106:107], v[124:125] op_sel:[1,0,0]\n\t" \
        "s_nop 0\n\t" \
        "ds_write_b128 v112, v[134:137]\n\t"

#define MFSGD_SOLO_HELPER_ASM_TEXT \
        "v_mov_b32 v141, %[ea]\n\t" \
        "v_mov_b32 v139, %[rb]\n\t" \
        "ds_read_b32 v133, v141\n\t" \
        "v_add_u32 v138, 16, v141\n\t" \
        "3:\n\t" \
        "ds_read2_b64 v[116:119], v138 offset1:2\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t" \
        "v_cmp_eq_u32 vcc, -1, v117\n\t" \
        "s_cbranch_vccz 4f\n\t" \
        "s_sleep 1\n\t" \
        "s_sub_u32 %[spins], %[spins], 1\n\t" \
        "s_cmp_eq_u32 %[spins], 0\n\t" \
        "s_cbranch_scc1 9f\n\t" \
        "s_branch 3b\n\t" \
        "4:\n\t" \
        "v_mad_u32_u16 v112, v133, 16, v139\n\t" \
        "v_bfe_u32 v140, v133, 16, 15\n\t" \
        "v_lshl_add_u32 v140, v140, 4, v139\n\t" \
        "ds_read_b128 v[100:103], v140\n\t" \
        "ds_read_b128 v[104:107], v112\n\t" \
        "ds_write_b32 v141, v133\n\t" \
        "s_cmp_lt_u32 %[n], 2\n\t" \
        "s_cbranch_scc1 80f\n\t" \
        MFSGD_LOOP_ALIGN \
        "5:\n\t" \
        MFSGD_SOLO_HELPER_PAIR("0", "116", "117", "118", "119", "150", "153") \
        "s_cbranch_scc1 81f\n\t" \
        MFSGD_SOLO_HELPER_PAIR("1", "150", "151", "152", "153", "116", "119") \
        "s_cbranch_scc0 5b\n\t" \
        MFSGD_SOLO_HELPER_TAIL("0", "116", "117") \
        "s_branch 40f\n\t" \
        MFSGD_SOLO_HELPER_TAIL("1", "150", "151") \
        "40:\n\t" \
        "s_cmp_eq_u32 %[fin], 0\n\t" \
        "s_cbranch_scc1 9f\n\t" \
        "ds_write_b128 v140, v[100:103]\n\t" \
        "s_branch 9f\n\t" \
        MFSGD_SOLO_HELPER_SLOW("0", "116", "117", "119") \
        MFSGD_SOLO_HELPER_SLOW("1", "150", "151", "153") \
        "9:\n\t" \
        "s_waitcnt lgkmcnt(0)\n\t"

#define MFSGD_SOLO_HELPER_OPERANDS                                                                                     \
    : [n] "+s"(n), [spins] "+s"(spins)                                                                                 \
    : [ea] "v"(ea), [rb] "v"(rowbase), [c2] "s"(c2), [fin] "s"(fin), [pad] "n"(PADV)                                                                 \
    : "memory", "scc", "vcc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110",  \
      "v111", "v112", "v113", "v116", "v117", "v118", "v119", "v122", "v123", "v124", "v125", "v126", "v127", "v128",  \
      "v129", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v150", "v151", "v152", "v153"
