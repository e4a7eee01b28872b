// The backward dX chain of PNY_PRECISION_F16_TRAIN: mlp_bwd_h2.hip with ONE f16 plane per operand (pny_mlp_bwd_h1_kernel), one
// v_mfma_f32_32x32x16_f16 per accumulator tile and 16 k, fp32 accumulation, in the same per-tile power-of-two scaled domain
// (headroom for one plane: mlp_bwd_h2.hip header).  The transposed weights are single-plane images in the
// model's h1 buffer (model_api.hip build_h1_images).
#define PNY_H2_PLANES 1
#include "mlp_bwd_h2.hip"
