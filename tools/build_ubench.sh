#!/bin/bash
# Builds the microbenchmarks of the rating loops into tools/bin/ (git-ignored; they travel to the GPU box with gpurun).
#   tools/build_ubench.sh && gpurun -- 'for L in 16 32 64; do tools/bin/ub3_$L; done'
set -e
cd "$(dirname "$0")"
mkdir -p bin
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
for L in 16 32 64; do
    $HIPCC --offload-arch=gfx950 -O2 -ffp-contract=off -DLG=$L -Wno-unused-value ubench3.hip -o bin/ub3_$L
done
# the chain wave's loop: steady body of P = 8 / 16 steps at every placement of its head, and every placement of the tail's
# head at P = 8 (profiles/chain_steady_ubench3.log); each -D defaults to the shipped value:
#   for f in tools/bin/ub3s_*; do echo $f; $f chain; done
for L in 16 32 64; do
    for P in 8 16; do
        for PAD in 0 2 4 6; do
            $HIPCC --offload-arch=gfx950 -O2 -ffp-contract=off -DLG=$L -DMFSGD_CHAIN_STEADY=$P -DMFSGD_PAD_CHAIN_STEADY=$PAD -Wno-unused-value ubench3.hip -o bin/ub3s_${L}_P${P}_s${PAD} &
        done
        wait
    done
    for PAD in 0 2 4 6; do
        $HIPCC --offload-arch=gfx950 -O2 -ffp-contract=off -DLG=$L -DMFSGD_CHAIN_STEADY=8 -DMFSGD_PAD_CHAIN_TAIL=$PAD -Wno-unused-value ubench3.hip -o bin/ub3s_${L}_P8_t${PAD} &
    done
    wait
done
# the one-wave loops (run loop, general loop) at every placement of their heads (profiles/loop_groups_ubench.log):
#   for f in tools/bin/ub3p_*; do echo $f; $f loops; done
for L in 16 32 64; do
    for PAD in 0 2 4 6; do
        $HIPCC --offload-arch=gfx950 -O2 -ffp-contract=off -DLG=$L -DMFSGD_PAD_RUN=$PAD -DMFSGD_PAD_GEN=$PAD -Wno-unused-value ubench3.hip -o bin/ub3p_${L}_$PAD &
    done
    wait
done
# L = 64 with the two v_permlane*_swap levels instead of the row_bcast reduction (what round 1 ran)
$HIPCC --offload-arch=gfx950 -O2 -ffp-contract=off -DLG=64 -DOLD64 -Wno-unused-value ubench3.hip -o bin/ub3_64old
$HIPCC --offload-arch=gfx950 -O2 ubench.hip -o bin/ubench
$HIPCC --offload-arch=gfx950 -O2 -Wno-unused-value ubench4.hip -o bin/ub4
# what the two wait-state slots behind a DPP add cost by what fills them (profiles/chain_slots_ubench.log)
$HIPCC --offload-arch=gfx950 -O2 -Wno-unused-value ubench5.hip -o bin/ub5
