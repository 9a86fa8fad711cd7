// One window of the head-summed MFMA cell kernel: logits, classification epilogue, confusion matrix, regression epilogue.
// Explicit instantiations only; xna_head.hip declares them extern and dispatches.
#ifndef NAF_KS
#error "compile with -DNAF_KS=<window> (naf_amd/build.py: INSTANCES)"
#endif
#include "xna_head_kernel.h"

NAF_XNA_HEAD_WINDOW(, NAF_KS)
