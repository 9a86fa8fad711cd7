// Head-summed MFMA cell kernel, 3x3 window (one translation unit per window: parallel compilation).
#include "xna_head_kernel.h"

NAF_XNA_HEAD_WINDOW(, 3)
