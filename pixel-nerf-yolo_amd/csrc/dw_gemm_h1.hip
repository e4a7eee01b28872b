// The weight-gradient GEMM of PNY_PRECISION_F16_TRAIN: dw_gemm_h2.hip with ONE f16 plane per operand (pny_dw_gemm_h1_kernel),
// one v_mfma_f32_32x32x16_f16 per product and 16 samples, fp32 accumulation, the same per-launch power-of-two scale of dY
// (dw_gemm_h2.hip header).
#define PNY_H2_PLANES 1
#include "dw_gemm_h2.hip"
