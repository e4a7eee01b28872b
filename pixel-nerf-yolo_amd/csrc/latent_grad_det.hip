// Deterministic latent gradient (pny_model_set_deterministic).  The float-atomic scatter of the
// latent-gradient kernels (latent_grad.hip, latent_grad_h2.hip) sums each latent pixel's contributions in the order in which
// the tiles happen to arrive, so d loss / d latent -- and the trunk gradients computed from it -- differ in the last bits from
// run to run.  This mode keeps the GEMM (same tiles, same arithmetic, same fp32 products w_k . dz) and makes the SUM exact:
//
//   1. lg_wmax_kernel: W = max |lin_z^T| over the packed operand (an atomic max: order-free);
//   2. lg_scale_kernel: the bound T = 8 . n_points . K . W . max|dY| on any partial sum of the launch (below), and the power of
//      two S with T . S < 2^62;
//   3. the GEMM built with -DPNY_LG_FIXED (latent_grad_fx.h): each contribution becomes round(w_k . dz . S), an int64 added
//      with a 64-bit integer atomic into the scene's accumulator.  Integer addition is associative: the accumulator holds the
//      same bits whatever the order;
//   4. lg_fixed_apply_kernel: grad += (float)(acc / S) element by element, and acc back to 0.
//
// Launches of one backward run in stream order (chunks, coarse then fine) or on disjoint slices (scenes on side streams, each
// with its own accumulator), so the whole gradient is bit-identical from run to run.  It is NOT the same across chunkings or
// batchings: S depends on the launch, and every launch rounds its sum to fp32 once when it adds it.
//
// The bound.  |dz[c]| = |sum_k lin_z^T[c][k] dY[k]| <= K . W . max|dY| in exact arithmetic; the fp32 / split-f16 / single-plane
// products and fp32 accumulation add relative errors far below the factor 2 kept for them.  A sample adds into at most 4 taps
// per channel with bilinear weights in [0, 1] (taps outside the latent carry weight 0 and are skipped), so no partial sum of a
// launch exceeds 4 . n_points . 2 . K . W . max|dY| = T.  Resolution: 1/S < T . 2^-61.  Measured against the atomic path on the
// same inputs: <= 3.3e-7 of the gradient's max.
// A non-finite max|dY| or W (the f16 range guard reports the former: PNY_RANGE_GRADIENT) makes the launch's whole gradient NaN.
//
// max|dY| must be the chain's running max of THIS launch's tiles (a per-scene word): the model-wide word of a deferred backward
// is still being raised by other scenes' chains on their streams, and a value read from it would differ from run to run.
#define PNY_LG_FIXED
#include "latent_grad.hip"

namespace pny {

void launch_latent_grad_h2_det(const MlpArgs& a, const float* dy_stash, const StashLayout& lay, const float* w_cat,
                               unsigned long long* grad, int nvb, hipStream_t st, const unsigned* dy_absmax, const double* fx);
void launch_latent_grad_h1_det(const MlpArgs& a, const float* dy_stash, const StashLayout& lay, const float* w_cat,
                               unsigned long long* grad, int nvb, hipStream_t st, const unsigned* dy_absmax, const double* fx);

namespace {

__global__ __launch_bounds__(256) void lg_wmax_kernel(const float4* __restrict__ w, long long n4, unsigned* __restrict__ wmax) {
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = w[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(wmax, __float_as_uint(m));   // non-negative floats order like their bit patterns
}

// fx[0] = S, fx[1] = 1 / S (fx[1] = NaN: the bound is not finite); dy_used = the max |dY| the launch's GEMM scales by.  Both
// running maxima are reset for the next launch here, in stream order (no memset between the kernels of a launch)
__global__ void lg_scale_kernel(unsigned* __restrict__ wmax, unsigned* __restrict__ dy_absmax, double n_terms, double* __restrict__ fx,
                                unsigned* __restrict__ dy_used) {
    if (threadIdx.x != 0) return;
    const unsigned wb = *wmax, db = *dy_absmax;
    *wmax = 0u;
    *dy_absmax = 0u;
    *dy_used = db;
    const double t = n_terms * (double)__uint_as_float(wb) * (double)__uint_as_float(db);
    double s = 1.0, inv = 1.0;
    if (!(t <= 1e300)) {
        inv = __builtin_nan("");
    } else if (t > 0.0) {
        int e;
        (void)frexp(t, &e);   // t < 2^e
        s = ldexp(1.0, 62 - e);
        inv = ldexp(1.0, e - 62);
    }
    fx[0] = s;
    fx[1] = inv;
}

__global__ __launch_bounds__(256) void lg_fixed_apply_kernel(unsigned long long* __restrict__ acc, float* __restrict__ grad, long long n,
                                                             const double* __restrict__ fx) {
    const double inv = fx[1];
    const bool poison = inv != inv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const unsigned long long q = acc[i];
        if (q != 0ull || poison) {   // (untouched elements keep their bits, signed zeros included)
            grad[i] += (float)((double)(long long)q * inv);
            acc[i] = 0ull;
        }
    }
}

__global__ void lg_absmax_fold_kernel(unsigned* __restrict__ dst, const unsigned* __restrict__ src) {
    if (threadIdx.x == 0) atomicMax(dst, *src);
}

}  // namespace

int launch_latent_grad_det(const MlpArgs& a, const float* dy_stash, const StashLayout& lay, const float* w_cat, float* grad, int nvb,
                           hipStream_t st, unsigned* dy_absmax, int arith, unsigned long long* acc, long long acc_elems,
                           void* words) {
    double* fx = reinterpret_cast<double*>(words);
    unsigned* wmax = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(words) + 16);
    unsigned* dy_used = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(words) + 24);
    const long long K = (long long)nvb * HID, n4 = (long long)a.L * K / 4;
    hipLaunchKernelGGL(lg_wmax_kernel, dim3((unsigned)std::min<long long>(1024, (n4 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(w_cat), n4, wmax);
    hipLaunchKernelGGL(lg_scale_kernel, dim3(1), dim3(64), 0, st, wmax, dy_absmax, 8.0 * (double)a.n_points * (double)K, fx, dy_used);
    if (arith == 0)
        launch_latent_grad_f32_det(a, dy_stash, lay, w_cat, acc, nvb, st, fx);
    else if (arith == 2)
        launch_latent_grad_h1_det(a, dy_stash, lay, w_cat, acc, nvb, st, dy_used, fx);
    else
        launch_latent_grad_h2_det(a, dy_stash, lay, w_cat, acc, nvb, st, dy_used, fx);
    hipLaunchKernelGGL(lg_fixed_apply_kernel, dim3((unsigned)std::min<long long>(4096, (acc_elems + 255) / 256)), dim3(256), 0, st, acc,
                       grad, acc_elems, fx);
    PNY_HIP(hipGetLastError());
    return 0;
}

void launch_absmax_fold(unsigned* dst, const unsigned* src, hipStream_t st) {
    hipLaunchKernelGGL(lg_absmax_fold_kernel, dim3(1), dim3(64), 0, st, dst, src);
}

}  // namespace pny
