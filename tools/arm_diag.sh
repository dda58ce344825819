#!/bin/bash
# Diagnostic variants of the training kernels (container side): each drops one part of a kernel
# (t_arm: bias MFMAs / weight-gradient MFMAs / context-gradient scatter; t_arm16; t_lvl_bwd),
# giving an upper bound on what that part costs.  Results are wrong by construction; never
# benchmarked as results.  Only the unit that holds the variant's kernel is recompiled with the
# define (csrc/train_arm.hip, or csrc/train_ups.hip for LVL_*) and linked against the other
# objects of a finished `make`.
# Usage (cool-chic_amd/): bash ../tools/arm_diag.sh   -> lib/diag/libccmi_arm_<v>.so
set -eu
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -fwrapv --offload-arch=gfx950 -munsafe-fp-atomics -Wno-unused-function"
mkdir -p lib/diag
for v in ${ARM_DIAG_VARIANTS:-NOBIAS NOOUTER NOSCATTER NOLDSATOM NOGATOM}; do  # t_arm16: A16_NORATE A16_NOOUTER A16_NOGATHER; t_lvl_bwd: LVL_NOREF LVL_NOUP LVL_NODW
    case $v in
    LVL_*) unit=train_ups; def=CCMI_DIAG_$v ;;
    A16_*) unit=train_arm; def=CCMI_DIAG_$v ;;
    NOHMFMA) unit=train_head; def=CCMI_DIAG_ARM_$v ;; # the full-width head backward's MFMAs
    *) unit=train_arm; def=CCMI_DIAG_ARM_$v ;;
    esac
    OTHERS=$(ls build/*.o | grep -v "/$unit.o\$")
    $CXX -D$def -x hip -c csrc/$unit.hip -o build/diag_${unit}_$v.obj
    /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o lib/diag/libccmi_arm_$v.so $OTHERS build/diag_${unit}_$v.obj
done
