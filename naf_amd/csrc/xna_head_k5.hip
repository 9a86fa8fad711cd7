// Head-summed MFMA cell kernel, 5x5 window (one translation unit per window: parallel compilation).
#include "xna_head_kernel.h"

NAF_XNA_HEAD_WINDOW(, 5)
