// The split-f16 GEMM of the deterministic latent gradient: latent_grad_h2.hip with the fixed-point epilogue (latent_grad_fx.h),
// latent_grad_h2_det_kernel, launched by launch_latent_grad_det (latent_grad_det.hip).
#define PNY_LG_FIXED
#include "latent_grad_h2.hip"
