// The single-plane (F16_TRAIN) GEMM of the deterministic latent gradient: latent_grad_h2.hip with one f16 plane per operand and
// the fixed-point epilogue (latent_grad_fx.h), latent_grad_h1_det_kernel, launched by launch_latent_grad_det (latent_grad_det.hip).
#define PNY_LG_FIXED
#define PNY_H2_PLANES 1
#include "latent_grad_h2.hip"
