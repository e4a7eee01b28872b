// The fused MLP kernel of PNY_PRECISION_F16: one f16 plane per operand (round to nearest), one v_mfma_f32_32x32x16_f16 per
// accumulator tile and 16 k, fp32 accumulation -- a third of the matrix work and half the weight bytes of the split-f16
// kernel, at an error of order 1e-3 instead of 1e-6.  Same source as mlp_h2.hip in its default 2 x 2 tile
// shape (8 waves, 64-sample tiles) for every launch size, so a sample's result does not depend on the launch it is rendered
// in; the weight ring is 4 steps deep in the registers of the two-plane depth-2 ring (mlp_h2_core.h).  Render launches only.
#define PNY_H2_PLANES 1
#include "mlp_h2.hip"
