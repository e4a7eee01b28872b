// The training forward of PNY_PRECISION_F16_TRAIN: the STASH instantiation of the single-plane kernel (mlp_h1.hip), with the
// split kernel's stash layout and fp32 stash contents -- the values of THIS forward.  A translation unit of its
// own: instantiated beside the render kernel, the shared helpers would be inlined differently and change that kernel's code.
#define PNY_H2_PLANES 1
#define PNY_H1_STASH
#include "mlp_h2.hip"
