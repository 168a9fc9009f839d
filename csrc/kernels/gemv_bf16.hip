// The decode GEMV kernels' instantiations for BF16 weights, in a translation unit of their own
// (the third; see gemv_legacy.hip): the weights are unquantised, so these kernels keep x in f32
// (gemv_dev.h, XPrologue's XF form) and their inner product is plain fp32 FMAs - code that is new
// and is compiled without the packed fp32 instructions (runtime/build.py). gemv.hip defines
// gemv_bf16() and gemv_qkv1_bf16() (and nothing else with external linkage) under these macros.
#define LFK_GEMV_LEGACY_TU
#define LFK_GEMV_BF16_TU
#include "gemv.hip"
