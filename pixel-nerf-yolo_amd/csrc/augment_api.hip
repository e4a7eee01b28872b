// C entry point of the colour jitter (include/pnyolo.h, "colour jitter" section; kernel in augment.hip): argument checks, the
// per-object factors copied into the kernel arguments, one launch.  No workspace, no allocation, no synchronisation.
#include <math.h>

#include <string>

#include "api_internal.h"
#include "pny_augment.h"

namespace pny {
void launch_color_jitter(const JitterArgs& a, int n_images, hipStream_t st);
}

using namespace pny;

static_assert(JITTER_MAX_OBJS == PNY_JITTER_MAX_OBJS, "pny_augment.h and pnyolo.h disagree on the objects per launch");
static_assert(JITTER_F32_NCHW_PM1 == PNY_IMG_F32_NCHW_PM1 && JITTER_U8_NHWC == PNY_IMG_U8_NHWC, "image formats");

extern "C" {

int pny_color_jitter(const pny_color_jitter_desc* desc, const void* images_dev, const float* factors_host, float* out_dev,
                     pny_stream stream) {
    const char* who = "pny_color_jitter: ";
    if (!desc || !images_dev || !factors_host || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (desc->n_objs <= 0 || desc->n_views <= 0 || desc->height <= 0 || desc->width <= 0)
        return fail(PNY_ERR_ARG, std::string(who) + "n_objs, n_views, height and width must be positive");
    if (desc->in_format != PNY_IMG_F32_NCHW_PM1 && desc->in_format != PNY_IMG_U8_NHWC)
        return fail(PNY_ERR_ARG, std::string(who) + "unknown in_format");
    if (desc->n_objs > PNY_JITTER_MAX_OBJS)
        return fail(PNY_ERR_ARG, std::string(who) + "more than 64 objects in one launch (the caller splits)");
    const int64_t pixels = (int64_t)desc->height * desc->width;                 // each factor is below 2^31: no overflow
    const int64_t images = (int64_t)desc->n_objs * desc->n_views;
    if (pixels >= ((int64_t)1 << 31) || images * pixels * 3 >= ((int64_t)1 << 31))
        return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    JitterArgs a;
    for (int o = 0; o < desc->n_objs; ++o) {
        const float* f = factors_host + 4 * o;
        if (!(fabsf(f[0]) <= 0.5f)) return fail(PNY_ERR_ARG, std::string(who) + "hue factor outside [-0.5, 0.5]");
        for (int i = 1; i < 4; ++i)
            if (!(f[i] >= 0.0f) || isinf(f[i]))
                return fail(PNY_ERR_ARG, std::string(who) + "saturation, brightness and contrast factors must be finite and not negative");
        a.f[o].hue = f[0], a.f[o].sat = f[1], a.f[o].bri = f[2], a.f[o].con = f[3];
    }
    for (int o = desc->n_objs; o < JITTER_MAX_OBJS; ++o) a.f[o] = JitterFactors{0.0f, 1.0f, 1.0f, 1.0f};
    if (desc->in_format == PNY_IMG_U8_NHWC && (const void*)out_dev == images_dev)
        return fail(PNY_ERR_ARG, std::string(who) + "in place needs the float format (the byte format's output is four times its input)");
    a.in = images_dev, a.out = out_dev;
    a.n_views = desc->n_views, a.hw = (int)pixels, a.format = desc->in_format;
    launch_color_jitter(a, (int)images, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

}  // extern "C"
