// Head-summed MFMA cell kernel, 13x13 window (one translation unit per window: parallel compilation).
#include "xna_head_kernel.h"

NAF_XNA_HEAD_WINDOW(, 13)
