// C entry points of LPIPS (include/pnyolo.h, "LPIPS" section; kernels in lpips.hip and encoder.hip): the handle that holds the
// VGG-16 and linear-layer weights, argument checks, and the 23 launches of a batch.
#include <map>
#include <string>
#include <vector>

#include "api_internal.h"
#include "pny_lpips.h"

namespace pny {
void launch_lpips_prepare(const LpipsPrepareArgs& a, hipStream_t st);
void launch_maxpool2(const float* in, float* out, int n, int hin, int win, int c, hipStream_t st);
bool launch_lpips_distance(const float* feat, const float* wl, double* out, int n, int npix, int c, int accumulate, hipStream_t st);
void launch_lpips_pack_conv(const float* w, float* packed, int cin, int cin_p, int cout, int J, hipStream_t st);
}  // namespace pny

struct pny_lpips {
    std::map<std::string, HostTensor> host;   // tensors as loaded
    bool finalized = false;
    int device = 0;                            // where finalize put the weights
    ConvLayer convs[LPIPS_CONVS];
    const float* lin[LPIPS_TAPS] = {};
    std::vector<DevBuf> allocs;                // what convs[] and lin[] point into
};

namespace {

// "conv7.bias" -> (0, 7, false); "lin3.weight" -> (1, 3, true); unknown -> false
bool parse_name(const std::string& name, int* family, int* index, bool* weight) {
    const size_t dot = name.find('.');
    if (dot == std::string::npos) return false;
    const std::string head = name.substr(0, dot), tail = name.substr(dot + 1);
    if (tail != "weight" && tail != "bias") return false;
    *weight = tail == "weight";
    size_t digits;
    if (head.compare(0, 4, "conv") == 0) *family = 0, digits = 4;
    else if (head.compare(0, 3, "lin") == 0) *family = 1, digits = 3;
    else return false;
    const std::string num = head.substr(digits);
    if (num.empty() || num.size() > 2 || num.find_first_not_of("0123456789") != std::string::npos || (num.size() == 2 && num[0] == '0'))
        return false;
    *index = std::stoi(num);
    if (*family == 0) return *index < LPIPS_CONVS;
    return *index < LPIPS_TAPS && *weight;
}

std::string conv_name(int i, const char* what) { return "conv" + std::to_string(i) + "." + what; }
std::string lin_name(int k) { return "lin" + std::to_string(k) + ".weight"; }

ConvLayer vgg_geometry(int layer) {
    ConvLayer L;
    L.cin = LPIPS_CIN[layer];
    L.cin_p = (L.cin + 3) / 4 * 4;
    L.cout = LPIPS_COUT[layer];
    L.k = 3;
    L.stride = 1;
    L.pad = 1;
    L.J = lpips_conv_J(layer);
    return L;
}

// size limits of a batch, shared by the sizing call and the forward
int check_size(const char* who, int n_pairs, int height, int width) {
    if (n_pairs <= 0) return fail(PNY_ERR_ARG, std::string(who) + "n_pairs must be positive");
    if (height < LPIPS_MIN_SIZE || width < LPIPS_MIN_SIZE)
        return fail(PNY_ERR_ARG, std::string(who) + "height and width must be at least 16 (relu5_3 would be empty), got " +
                                     std::to_string(height) + " x " + std::to_string(width));
    if (!lpips_fits_32bit(n_pairs, height, width))
        return fail(PNY_ERR_ARG, std::string(who) + "the largest activation, 2 * " + std::to_string(n_pairs) + " * " + std::to_string(height) +
                                     " * " + std::to_string(width) + " * 64 floats, does not fit 32-bit indexing: use a smaller batch");
    return 0;
}

bool known_kind(int k) { return k == LPIPS_F32_NHWC_01 || k == LPIPS_F32_NCHW_PM1 || k == LPIPS_U8_NHWC || k == LPIPS_F32_NCHW_01; }

int check_desc(const char* who, const pny_lpips_desc* d) {
    if (!known_kind(d->pred_kind)) return fail(PNY_ERR_ARG, std::string(who) + "unknown pred_kind");
    if (!known_kind(d->gt_kind)) return fail(PNY_ERR_ARG, std::string(who) + "unknown gt_kind");
    return 0;
}

LpipsPrepareArgs prepare_args(const pny_lpips_desc* d, const void* pred, const void* gt, int n, float* out, double* zero) {
    LpipsPrepareArgs a;
    a.pred = pred, a.gt = gt, a.out = out, a.zero = zero;
    a.n = n, a.h = d->height, a.w = d->width;
    a.pred_kind = d->pred_kind, a.gt_kind = d->gt_kind, a.clamp = d->clamp;
    return a;
}

int upload(const std::vector<float>& v, DevBuf* b) {
    if (int rc = b->reserve(v.size() * sizeof(float), "hipMalloc(LPIPS weights)")) return rc;
    PNY_HIP(hipMemcpy(b->p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

extern "C" {

int pny_lpips_create(pny_lpips** out) {
    if (!out) return fail(PNY_ERR_ARG, "pny_lpips_create: null argument");
    *out = new pny_lpips();
    return PNY_OK;
}

void pny_lpips_destroy(pny_lpips* h) {
    if (!h) return;
    if (h->finalized) drain_device(h->device);
    delete h;
}

int pny_lpips_load_weights(pny_lpips* h, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    const char* who = "pny_lpips_load_weights: ";
    if (!h || !name || !data_host || !shape || ndim < 1 || ndim > 8) return fail(PNY_ERR_ARG, std::string(who) + "bad argument");
    int family, index;
    bool weight;
    if (!parse_name(name, &family, &index, &weight))
        return fail(PNY_ERR_ARG, std::string(who) + "unknown tensor '" + name + "' (conv0..12.weight, conv0..12.bias, lin0..4.weight)");
    std::vector<int64_t> shp(shape, shape + ndim);
    int64_t count = 1;
    for (int64_t s : shp) count *= s > 0 ? s : 0;
    bool ok;
    if (family == 0 && weight) ok = shp == std::vector<int64_t>{LPIPS_COUT[index], LPIPS_CIN[index], 3, 3};
    else if (family == 0) ok = shp == std::vector<int64_t>{LPIPS_COUT[index]};
    else ok = count == LPIPS_TAP_CH[index];
    if (!ok) {
        std::string got;
        for (int64_t s : shp) got += (got.empty() ? "" : ", ") + std::to_string(s);
        return fail(PNY_ERR_ARG, std::string(who) + "'" + name + "' has shape (" + got + ")");
    }
    HostTensor& t = h->host[name];
    t.shape = shp;
    t.data.assign(data_host, data_host + count);
    return PNY_OK;
}

int pny_lpips_finalize(pny_lpips* h, pny_stream stream) {
    const char* who = "pny_lpips_finalize: ";
    if (!h) return fail(PNY_ERR_ARG, std::string(who) + "null handle");
    for (int i = 0; i < LPIPS_CONVS; ++i)
        for (const char* what : {"weight", "bias"})
            if (!h->host.count(conv_name(i, what))) return fail(PNY_ERR_STATE, std::string(who) + "missing tensor '" + conv_name(i, what) + "'");
    for (int k = 0; k < LPIPS_TAPS; ++k)
        if (!h->host.count(lin_name(k))) return fail(PNY_ERR_STATE, std::string(who) + "missing tensor '" + lin_name(k) + "'");
    hipStream_t st = (hipStream_t)stream;
    if (h->finalized) drain_device(h->device);   // launches that read the old weights
    h->finalized = false;
    h->allocs.clear();
    PNY_HIP(hipGetDevice(&h->device));
    std::vector<DevBuf> raw(LPIPS_CONVS);          // the tensors as loaded, read by the packing launches
    for (int i = 0; i < LPIPS_CONVS; ++i) {
        ConvLayer L = vgg_geometry(i);
        DevBuf packed, scale, shift;
        if (int rc = upload(h->host[conv_name(i, "weight")].data, &raw[i])) return rc;
        if (int rc = packed.reserve((size_t)(L.cout / 32) * L.J * 256 * sizeof(float), "hipMalloc(LPIPS weights)")) return rc;
        if (int rc = upload(std::vector<float>((size_t)L.cout, 1.0f), &scale)) return rc;
        if (int rc = upload(h->host[conv_name(i, "bias")].data, &shift)) return rc;
        launch_lpips_pack_conv(raw[i].f(), packed.f(), L.cin, L.cin_p, L.cout, L.J, st);
        PNY_HIP(hipGetLastError());
        L.w = packed.f(), L.scale = scale.f(), L.shift = shift.f();
        h->convs[i] = L;
        h->allocs.push_back(std::move(packed));
        h->allocs.push_back(std::move(scale));
        h->allocs.push_back(std::move(shift));
    }
    for (int k = 0; k < LPIPS_TAPS; ++k) {
        DevBuf w;
        if (int rc = upload(h->host[lin_name(k)].data, &w)) return rc;
        h->lin[k] = w.f();
        h->allocs.push_back(std::move(w));
    }
    PNY_HIP(hipStreamSynchronize(st));   // the packing has read `raw`
    h->finalized = true;
    return PNY_OK;
}

int pny_lpips_workspace_bytes(int n_pairs, int height, int width, size_t* bytes) {
    if (!bytes) return fail(PNY_ERR_ARG, "pny_lpips_workspace_bytes: null argument");
    if (int rc = check_size("pny_lpips_workspace_bytes: ", n_pairs, height, width)) return rc;
    *bytes = lpips_workspace_floats((size_t)n_pairs, (size_t)height, (size_t)width) * sizeof(float);
    return PNY_OK;
}

int pny_lpips_prepare(const pny_lpips_desc* desc, const void* pred_dev, const void* gt_dev, int n_pairs, float* out_dev, pny_stream stream) {
    const char* who = "pny_lpips_prepare: ";
    if (!desc || !pred_dev || !gt_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n_pairs <= 0 || desc->height <= 0 || desc->width <= 0 || !lpips_fits_32bit(n_pairs, desc->height, desc->width))
        return fail(PNY_ERR_ARG, std::string(who) + "n_pairs, height and width must be positive and 2 n H W 64 below 2^31");
    if (int rc = check_desc(who, desc)) return rc;
    launch_lpips_prepare(prepare_args(desc, pred_dev, gt_dev, n_pairs, out_dev, nullptr), (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_lpips_maxpool2(const float* in_dev, int n, int h, int w, int c, float* out_dev, pny_stream stream) {
    const char* who = "pny_lpips_maxpool2: ";
    if (!in_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n <= 0 || h < 2 || w < 2 || c <= 0 || c % 4) return fail(PNY_ERR_ARG, std::string(who) + "needs n > 0, h and w >= 2, c % 4 == 0");
    if ((long long)n * h * w * c >= (1ll << 31)) return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    launch_maxpool2(in_dev, out_dev, n, h, w, c, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_lpips_distance(const float* tap_dev, const float* weight_dev, int n_pairs, int h, int w, int c, int accumulate, double* out_dev,
                       pny_stream stream) {
    const char* who = "pny_lpips_distance: ";
    if (!tap_dev || !weight_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (n_pairs <= 0 || h <= 0 || w <= 0) return fail(PNY_ERR_ARG, std::string(who) + "n_pairs, h and w must be positive");
    if (c != 64 && c != 128 && c != 256 && c != 512) return fail(PNY_ERR_ARG, std::string(who) + "c must be 64, 128, 256 or 512");
    if (2ll * n_pairs * h * w * c >= (1ll << 31)) return fail(PNY_ERR_ARG, std::string(who) + "2^31 elements or more");
    launch_lpips_distance(tap_dev, weight_dev, out_dev, n_pairs, h * w, c, accumulate, (hipStream_t)stream);
    PNY_HIP(hipGetLastError());
    return PNY_OK;
}

int pny_lpips_conv(pny_lpips* h, int layer, const float* in_dev, int n, int height, int width, float* out_dev, int* variant,
                   pny_stream stream) {
    const char* who = "pny_lpips_conv: ";
    if (!h || !in_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (!h->finalized) return fail(PNY_ERR_STATE, std::string(who) + "pny_lpips_finalize has not run");
    if (layer < 0 || layer >= LPIPS_CONVS) return fail(PNY_ERR_ARG, std::string(who) + "layer must be 0 .. 12");
    if (n <= 0 || height <= 0 || width <= 0 || (long long)n * height * width * 512 >= (1ll << 31))
        return fail(PNY_ERR_ARG, std::string(who) + "n, height and width must be positive and n H W 512 below 2^31");
    PNY_HIP(hipSetDevice(h->device));
    if (!run_conv_ex(h->convs[layer], in_dev, n, height, width, height, width, 0, nullptr, 1, out_dev, (hipStream_t)stream, variant,
                     lpips_conv_variant(layer, height, width, n)))
        return hip_fail(hipGetLastError(), "conv_mfma_kernel (LPIPS)");
    return PNY_OK;
}

int pny_lpips_forward(pny_lpips* h, const pny_lpips_desc* desc, const void* pred_dev, const void* gt_dev, int n_pairs, void* work_dev,
                      double* out_dev, pny_stream stream) {
    const char* who = "pny_lpips_forward: ";
    if (!h || !desc || !pred_dev || !gt_dev || !work_dev || !out_dev) return fail(PNY_ERR_ARG, std::string(who) + "null argument");
    if (!h->finalized) return fail(PNY_ERR_STATE, std::string(who) + "pny_lpips_finalize has not run");
    const int batch = desc->batch_size > 0 ? desc->batch_size : n_pairs;
    if (n_pairs > batch) return fail(PNY_ERR_ARG, std::string(who) + "n_pairs exceeds desc->batch_size, which sized the workspace");
    if (int rc = check_size(who, batch, desc->height, desc->width)) return rc;
    if (n_pairs <= 0) return fail(PNY_ERR_ARG, std::string(who) + "n_pairs must be positive");
    if (int rc = check_desc(who, desc)) return rc;
    PNY_HIP(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int H = desc->height, W = desc->width, n2 = 2 * n_pairs;
    // the workspace is laid out for the configured batch (pny_lpips.h), whatever this call's n_pairs
    Carver c{static_cast<float*>(work_dev)};
    float* img4 = c.take((size_t)2 * batch * H * W * 4);
    float* buf[2] = {c.take((size_t)2 * batch * H * W * 64), c.take((size_t)2 * batch * H * W * 64)};

    launch_lpips_prepare(prepare_args(desc, pred_dev, gt_dev, n_pairs, img4, out_dev), st);
    PNY_HIP(hipGetLastError());
    const float* x = img4;
    int cur = 0, tap = 0;   // buf[cur] is written next
    for (int i = 0; i < LPIPS_CONVS; ++i) {
        const int s = LPIPS_STAGE[i], hs = H >> s, ws = W >> s;
        if (i > 0 && s != LPIPS_STAGE[i - 1]) {
            launch_maxpool2(x, buf[cur], n2, H >> (s - 1), W >> (s - 1), LPIPS_CIN[i], st);
            PNY_HIP(hipGetLastError());
            x = buf[cur], cur ^= 1;
        }
        if (!run_conv_ex(h->convs[i], x, n2, hs, ws, hs, ws, 0, nullptr, 1, buf[cur], st, nullptr, lpips_conv_variant(i, hs, ws, 2 * batch)))
            return hip_fail(hipGetLastError(), "conv_mfma_kernel (LPIPS)");
        x = buf[cur], cur ^= 1;
        if (tap < LPIPS_TAPS && i == LPIPS_TAP_CONV[tap]) {
            launch_lpips_distance(x, h->lin[tap], out_dev, n_pairs, hs * ws, LPIPS_TAP_CH[tap], 1, st);
            PNY_HIP(hipGetLastError());
            ++tap;
        }
    }
    return PNY_OK;
}

}  // extern "C"
