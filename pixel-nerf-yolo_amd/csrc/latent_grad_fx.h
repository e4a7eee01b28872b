// The two builds of the latent-gradient GEMMs (latent_grad.hip, latent_grad_h2.hip, latent_grad_h1.hip):
//
//   default         the epilogue adds each tap's contribution w_k . dz to the fp32 gradient with a float atomic;
//   PNY_LG_FIXED    (latent_grad_det.hip, latent_grad_h2_det.hip, latent_grad_h1_det.hip: pny_model_set_deterministic) the
//                   same fp32 product is rounded to a 64-bit fixed-point integer, round(w_k . dz . S), and added with an
//                   integer atomic into the scene's accumulator.  Integer addition is associative, so the sum does not depend
//                   on the order in which the tiles arrive; launch_latent_grad_det then adds acc / S to the fp32 gradient.
//                   S (a power of two, fx[0]) is chosen per launch so that no partial sum can leave +-2^62 (the bound is in
//                   latent_grad_det.hip lg_scale_kernel).
//
// Without PNY_LG_FIXED the macros expand to the tokens the kernels were written with: the default kernels are unchanged.
#pragma once

#ifdef PNY_LG_FIXED
#define PNY_LG32_KERNEL latent_grad_det_kernel
#define PNY_LG_OUT unsigned long long
#define PNY_LG_FX_ARG , const double* __restrict__ fx
#define PNY_LG_FX_LOAD const double fx_scale = fx[0];
#define PNY_LG_FX_PASS , fx
#define PNY_LG_ADD(p, x) atomicAdd((p), lg_to_fixed((x), fx_scale))

namespace pny {
// round(x . S) as a two's-complement 64-bit integer; |x . S| <= 2^62 by the choice of S (clamped all the same, so that a value
// outside the bound -- only a non-finite one can be -- never converts out of range)
__device__ __forceinline__ unsigned long long lg_to_fixed(float x, double S) {
    const double v = fmin(fmax((double)x * S, -0x1p62), 0x1p62);
    return (unsigned long long)(long long)__builtin_rint(v);
}
}  // namespace pny
#else
#define PNY_LG32_KERNEL latent_grad_kernel
#define PNY_LG_OUT float
#define PNY_LG_FX_ARG
#define PNY_LG_FX_LOAD
#define PNY_LG_FX_PASS
#define PNY_LG_ADD(p, x) unsafeAtomicAdd((p), (x))
#endif
