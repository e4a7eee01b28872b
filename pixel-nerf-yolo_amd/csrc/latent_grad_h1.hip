// The latent gradient of PNY_PRECISION_F16_TRAIN: latent_grad_h2.hip with ONE f16 plane per operand (latent_grad_h1_kernel),
// one v_mfma_f32_32x32x16_f16 per accumulator tile and 16 k, fp32 accumulation, the same per-launch power-of-two scale of dY
// (latent_grad_h2.hip header).
#define PNY_H2_PLANES 1
#include "latent_grad_h2.hip"
