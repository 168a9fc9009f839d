// The decode GEMV kernels' instantiations for the legacy 32-weight block types (Q4_0, Q4_1,
// Q5_0, Q5_1), the 2- and 3-bit K-quants (Q2_K, Q3_K) and the non-linear 4-bit pair (IQ4_NL,
// IQ4_XS), in a translation unit of their own: gemv.hip is the longest compile of the build, and
// these eight types would more than double it. gemv.hip defines gemv_legacy() and
// gemv_qkv1_legacy() (and nothing else with external linkage) under this macro.
#define LFK_GEMV_LEGACY_TU
#include "gemv.hip"
