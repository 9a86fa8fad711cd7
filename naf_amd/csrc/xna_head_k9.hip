// Head-summed MFMA cell kernel, 9x9 window (one translation unit per window: parallel compilation).
#include "xna_head_kernel.h"

NAF_XNA_HEAD_WINDOW(, 9)
