// precision16 (one bf16 pass) conv kernels, epilogue mode EPI_DGRAD_ACT (see fdet_conv3x3_x3_kernel.inc)
#define X3_MODE EPI_DGRAD_ACT
#define X3_MODE_ID 4
#define X3_P16 1
#include "fdet_conv3x3_x3_configs.h"
#include "fdet_conv3x3_x3_kernel.inc"
