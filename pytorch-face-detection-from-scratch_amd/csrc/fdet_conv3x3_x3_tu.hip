// bf16x3 / precision16 3x3 conv kernels (fdet_conv3x3_x3_kernel.inc): the Makefile builds this source twelve times,
// -DX3_TU=<6*P16 + epilogue mode> -- one translation unit per (epilogue mode, precision) behind fdet_x3_launch_m<mode>[_bf16]()
#ifndef X3_TU
#error "compile with -DX3_TU=<0..11>"
#endif
#if X3_TU >= 6
#define X3_P16 1
#endif
#if X3_TU % 6 == 0
#define X3_MODE EPI_GENERIC
#define X3_MODE_ID 0
#elif X3_TU % 6 == 1
#define X3_MODE EPI_FWD_FULL
#define X3_MODE_ID 1
#elif X3_TU % 6 == 2
#define X3_MODE EPI_FWD_BOTH
#define X3_MODE_ID 2
#elif X3_TU % 6 == 3
#define X3_MODE EPI_FWD_OUT
#define X3_MODE_ID 3
#elif X3_TU % 6 == 4
#define X3_MODE EPI_DGRAD_ACT
#define X3_MODE_ID 4
#else
#define X3_MODE EPI_DGRAD_ADD
#define X3_MODE_ID 5
#endif
#include "fdet_conv3x3_x3_configs.h"
#include "fdet_conv3x3_x3_kernel.inc"
