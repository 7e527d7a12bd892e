// C-ABI glue: error state, version, single-operator entry points (include/pvr_hip.h).
#include <stdarg.h>
#include "encoder_internal.h"
#include "sample_rng.h"
#include <dlfcn.h>

namespace pvr {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
const std::string &last_error() { return g_err; }

namespace {
typedef int (*roctx_push_fn)(const char *);
typedef int (*roctx_pop_fn)();
struct Roctx {
    roctx_push_fn push = nullptr;
    roctx_pop_fn pop = nullptr;
    Roctx() {
        const char *e = getenv("PVR_ROCTX");
        if (!e || atoi(e) == 0) return;
        for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
                push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
                pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
const Roctx &roctx() { static Roctx r; return r; }
}  // namespace
void trace_push(const char *name) { if (roctx().push) roctx().push(name); }
void trace_pop() { if (roctx().pop) roctx().pop(); }

// (the launchers the encoder shares: encoder_internal.h)
long long conv_expand_launches();
long long bneck_frame_launches();
long long pp_persistent_launches();
long long conv_wfrag_launches();
long long conv_split16_launches();
pvr_status launch_split16_pack(const float *w, void *out, int rows, int K, hipStream_t stream);
pvr_status launch_conv_split16(const float *in, const void *wsp, const float *bias, const float *res, float *out, int n, int h, int w, int cin,
                               int cout, int k, int stride, int pad, int relu, hipStream_t stream, float *out2 = nullptr, int n1 = 0, void *out16 = nullptr,
                               int terms = 3);

static void *g_zero = nullptr;
static pvr_status zero_page(void **out) {
    if (!g_zero) {
        PVR_HIP_TRY(hipMalloc(&g_zero, PVR_ZERO_BYTES));       // (the split-K launch reads an all-zero bias of cout floats from it)
        PVR_HIP_TRY(hipMemset(g_zero, 0, PVR_ZERO_BYTES));
        PVR_HIP_TRY(hipDeviceSynchronize());
    }
    *out = g_zero;
    return PVR_OK;
}

}  // namespace pvr

using namespace pvr;

extern "C" {

const char *pvr_version(void) { return "pvr_hip 0.1.0 (gfx950)"; }

int64_t pvr_debug_conv_expand_launches(void) { return (int64_t)conv_expand_launches(); }
int64_t pvr_debug_bneck_frame_launches(void) { return (int64_t)bneck_frame_launches(); }
// (rows, K) 16-bit weights in pvr_op_conv2d's layout -> the fragment-blocked layout pvr_op_bneck_frame reads (same size; rows % 32 == 0, K % 32 == 0)
pvr_status pvr_op_pack_frag_weights(const void *w, void *out, int32_t rows, int32_t k, void *stream) {
    return launch_pack_frag_weights(w, out, rows, k, (hipStream_t)stream);
}

// single-operator entry point of the per-frame fused layer3 bottleneck tail (bneck_frame.hip), for the op-level parity tests
pvr_status pvr_op_bneck_frame(const void *t1, const void *w2, const float *b2, const void *w3, const float *b3, const void *residual, void *y,
                              void *t2_out, const void *w1n, const float *b1n, void *t1n, const void *w1f, const float *b1f, int32_t n, int32_t phases,
                              int32_t dtype, void *stream) {
    PVR_REQUIRE(n > 0 && n <= 1300, "pvr_op_bneck_frame: n must be 1..1300");
    return launch_bneck_frame(op_switches(), t1, w2, b2, w3, b3, residual, y, t2_out, n, phases, dtype, (hipStream_t)stream, nullptr, w1n, b1n, t1n, w1f, b1f);
}
// the same launch with s_memtime stamps of block 8 (20 x uint64 on the device: waves 0 and 4, ten phase boundaries each) - diagnostics only
pvr_status pvr_debug_bneck_frame_stamps(const void *t1, const void *w2, const float *b2, const void *w3, const float *b3, const void *residual, void *y,
                                        const void *w1n, const float *b1n, void *t1n, const void *w1f, const float *b1f, int32_t n, int32_t dtype,
                                        uint64_t *stamps_dev, void *stream) {
    PVR_REQUIRE(stamps_dev && n > 8, "pvr_debug_bneck_frame_stamps: needs a stamp buffer and more than 8 frames");
    return launch_bneck_frame(op_switches(), t1, w2, b2, w3, b3, residual, y, nullptr, n, (w1n ? 7 : 3) | (w1f ? 8 : 0), dtype, (hipStream_t)stream, (unsigned long long *)stamps_dev,
                              w1n, b1n, t1n, w1f, b1f);
}
// single-operator entry point of the small-M implicit-GEMM kernel with weights as L2 fragments (conv_wfrag.hip), for the op-level parity tests
pvr_status pvr_op_conv_wfrag(const void *in, const void *wgt_packed, const float *bias, const void *residual, void *out, int32_t n, int32_t h, int32_t w,
                             int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t relu, int32_t out_f32, int32_t dtype,
                             void *stream) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "pvr_op_conv_wfrag: empty input");
    return launch_conv_wfrag(op_switches(), in, wgt_packed, bias, residual, out, n, h, w, cin, cout, kh, kw, stride, pad, relu, out_f32, dtype, (hipStream_t)stream);
}
// conv_pp256's two-operand form (conv3 & downsample in one accumulation), for the op-level parity tests
pvr_status pvr_op_conv2d_dual(const void *in, const void *in2, const void *wgt, const float *bias, void *out, int32_t n, int32_t h, int32_t w, int32_t cin,
                              int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t h2, int32_t w2, int32_t cin2, int32_t stride2,
                              int32_t relu, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && in2 && wgt && bias && out && n > 0, "pvr_op_conv2d_dual: null argument");
    PVR_REQUIRE(dtype == PVR_BF16 || dtype == PVR_F16, "pvr_op_conv2d_dual: 16-bit storage types only");
    return launch_conv_pp256(op_switches(), in, wgt, bias, nullptr, out, n, h, w, cin, cout, kh, kw, stride, pad, relu, 0, 0, dtype, 224, (hipStream_t)stream, in2, h2, w2,
                             cin2, stride2);
}
// the pooled form of conv_wfrag: a 1 x 1 convolution on 7 x 7 maps + identity + ReLU whose only output is the average over each frame's 49 pixels
pvr_status pvr_op_conv_wfrag_pool(const void *in, const void *wgt_packed, const float *bias, const void *residual, float *pool_out, int64_t pool_stride,
                                  int32_t n, int32_t cin, int32_t cout, int32_t dtype, void *stream) {
    PVR_REQUIRE(n > 0 && pool_out, "pvr_op_conv_wfrag_pool: empty input");
    return launch_conv_wfrag(op_switches(), in, wgt_packed, bias, residual, nullptr, n, 7, 7, cin, cout, 1, 1, 1, 0, 1, 1, dtype, (hipStream_t)stream, pool_out, pool_stride);
}
int64_t pvr_debug_conv_wfrag_launches(void) { return (int64_t)conv_wfrag_launches(); }
// fp32 convolution on the 16-bit matrix pipe (conv_split16.hip): weights packed once, fp32 NHWC activations in and out
pvr_status pvr_op_split16_pack_weights(const float *w, void *out, int32_t rows, int32_t k, void *stream) {
    return launch_split16_pack(w, out, rows, k, (hipStream_t)stream);
}
pvr_status pvr_op_conv2d_split16(const float *in, const void *wgt_split, const float *bias, const float *residual, float *out, int32_t n, int32_t h,
                                 int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, void *stream) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "pvr_op_conv2d_split16: empty input");
    return launch_conv_split16(in, wgt_split, bias, residual, out, n, h, w, cin, cout, k, stride, pad, relu, (hipStream_t)stream);
}
// the same convolution on the f32-input MFMA (conv_f32.hip: the kernel of the PVR_F32 reference-precision mode), fp32 weights (cout_pad, k*k*cin)
pvr_status pvr_op_conv2d_f32(const float *in, const float *wgt, const float *bias, const float *residual, float *out, int32_t n, int32_t h, int32_t w,
                             int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, void *stream) {
    PVR_REQUIRE(in && wgt && bias && out && n > 0, "pvr_op_conv2d_f32: null argument");
    return launch_conv_f32(in, wgt, bias, residual, out, n, h, w, cin, cout, k, stride, pad, relu, (hipStream_t)stream);
}
int64_t pvr_debug_conv_split16_launches(void) { return (int64_t)conv_split16_launches(); }
// conv1 of the PVR_F32S plan (stem_split16.hip): the zero-bordered fp32 NHWC4 image, split weights (rows 64, K 224)
pvr_status pvr_op_stem_split16(const float *img_padded, const void *wgt_split, const float *bias, float *out, int32_t n, int32_t S, void *stream) {
    return launch_stem_split16(img_padded, wgt_split, bias, out, n, S, (hipStream_t)stream);
}
int64_t pvr_debug_stem_split16_launches(void) { return (int64_t)stem_split16_launches(); }
int64_t pvr_debug_pp_persistent_launches(void) { return (int64_t)pp_persistent_launches(); }

size_t pvr_last_error(char *buf, size_t cap) {
    const std::string &e = last_error();
    if (buf && cap) {
        size_t n = e.size() < cap - 1 ? e.size() : cap - 1;
        memcpy(buf, e.data(), n);
        buf[n] = 0;
    }
    return e.size();
}

pvr_status pvr_op_preprocess(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop,
                             void *out, int32_t dtype, void *stream) {
    PVR_REQUIRE(frames && out, "pvr_op_preprocess: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PVR_HIP_TRY(hipMemsetAsync(out, 0, (size_t)n * (crop + 6) * (crop + 8) * 4 * 2, st));
    return launch_preprocess(frames, n, h, w, resize, crop, out, dtype, st);
}

pvr_status pvr_op_stem(const void *img, const void *wgt, const float *bias, void *out, int32_t n, int32_t dtype,
                       void *stream) {
    PVR_REQUIRE(img && wgt && bias && out, "pvr_op_stem: null pointer");
    return launch_stem(img, wgt, bias, out, n, 224, dtype, (hipStream_t)stream);
}

pvr_status pvr_op_maxpool(const void *in, void *out, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype,
                          void *stream) {
    PVR_REQUIRE(in && out, "pvr_op_maxpool: null pointer");
    return launch_maxpool(in, out, n, h, w, c, dtype, (hipStream_t)stream);
}

pvr_status pvr_op_conv2d(const void *in, const void *wgt, const float *bias, const void *residual, void *out, int32_t n,
                         int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride,
                         int32_t pad, int32_t relu, int32_t out_f32, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && wgt && bias && out, "pvr_op_conv2d: null pointer");
    void *z;
    pvr_status s = zero_page(&z);
    if (s) return s;
    return launch_conv(op_switches(), in, wgt, bias, residual, out, z, n, h, w, cin, cout, kh, kw, stride, pad, relu, out_f32, dtype,
                       (hipStream_t)stream);
}

// the pvr_op_* calls' kernel choice (op_switches); an encoder handle has its own switch (pvr_encoder_debug_set_switch "conv_algo")
pvr_status pvr_debug_set_conv_algo(int32_t algo) {
    PVR_REQUIRE(algo >= -1 && algo <= 4, "pvr_debug_set_conv_algo: algo must be -1 (auto), 0 (conv_igemm), 1 / 2 / 3 (conv_pp256 with 256- / 128- / 224-pixel tiles), 4 (conv_w4)");
#ifndef PVR_EXPERIMENTS
    PVR_REQUIRE(algo != 4, "pvr_debug_set_conv_algo: conv_w4 is an experiment kernel; this library was built without it (make EXPERIMENTS=1)");
#endif
    op_switches().conv_algo = algo;
    return PVR_OK;
}

pvr_status pvr_op_avgpool(const void *in, float *out, int64_t out_stride, int32_t n, int32_t hw, int32_t c, int32_t in_f32,
                          int32_t dtype, void *stream) {
    PVR_REQUIRE(in && out, "pvr_op_avgpool: null pointer");
    return launch_avgpool(in, out, out_stride, n, hw, c, in_f32, dtype, (hipStream_t)stream);
}

// The fused forms of the stem one at a time (tests/test_gpu_resnet_kernels.py): the form is chosen on a copy of op_switches()
static pvr_status stem_form_switches(int form, PlanSwitches &sw) {
    PVR_REQUIRE(form >= 0 && form <= 2, "pvr_op_stem_pool: form must be 0 (stem_pool_kernel), 1 (LDS tile) or 2 (register pooling), got %d", form);
    sw = op_switches();
    sw.stem_lds = form >= 1;
    sw.stem_regpool = form == 2;
    return PVR_OK;
}
pvr_status pvr_op_stem_pool(const void *img_padded, const void *wgt, const float *bias, void *out, int32_t n, int32_t form, const void *c1_w, const float *c1_b,
                            void *c1_t1, int32_t dtype, void *stream) {
    PVR_REQUIRE(img_padded && wgt && bias && out && n > 0, "pvr_op_stem_pool: null pointer or empty batch");
    PVR_REQUIRE(dtype == PVR_BF16 || dtype == PVR_F16, "pvr_op_stem_pool: 16-bit storage types only");
    PlanSwitches sw;
    if (pvr_status s = stem_form_switches(form, sw)) return s;
    return launch_stem_pool(sw, img_padded, wgt, bias, out, n, 224, dtype, (hipStream_t)stream, c1_w, c1_b, c1_t1, 0);
}
pvr_status pvr_op_stem_pool_u8(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t top, int32_t left, const void *wgt, const float *bias, void *out,
                               int32_t form, const void *c1_w, const float *c1_b, void *c1_t1, int32_t dtype, void *stream) {
    PVR_REQUIRE(frames && wgt && bias && out && n > 0, "pvr_op_stem_pool_u8: null pointer or empty batch");
    PVR_REQUIRE(dtype == PVR_BF16 || dtype == PVR_F16, "pvr_op_stem_pool_u8: 16-bit storage types only");
    PlanSwitches sw;
    if (pvr_status s = stem_form_switches(form, sw)) return s;
    PVR_REQUIRE(form != 0, "pvr_op_stem_pool_u8: stem_pool_kernel (form 0) has no uint8 form");
    return launch_stem_pool_u8(sw, frames, n, h, w, top, left, wgt, bias, out, dtype, (hipStream_t)stream, c1_w, c1_b, c1_t1, 0);
}
pvr_status pvr_debug_stem_c1_pack(const uint16_t *w, uint16_t *image) {
    PVR_REQUIRE(w && image, "pvr_debug_stem_c1_pack: null pointer");
    stem_c1_pack(w, image);
    return PVR_OK;
}

pvr_status pvr_op_conv2d_splitk(const void *in, const void *wgt, const float *bias, const void *residual, void *out, float *scratch, int32_t ksplit, int32_t n,
                                int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t relu,
                                int32_t out_f32, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && wgt && bias && out && n > 0 && h > 0 && w > 0, "pvr_op_conv2d_splitk: null pointer or empty input");
    PVR_REQUIRE(dtype == PVR_BF16 || dtype == PVR_F16, "pvr_op_conv2d_splitk: 16-bit storage types only");
    void *z;
    if (pvr_status s = zero_page(&z)) return s;
    return launch_conv_splitk(in, wgt, bias, residual, out, z, scratch, ksplit, n, h, w, cin, cout, kh, kw, stride, pad, relu, out_f32, dtype, (hipStream_t)stream);
}

// the layout and format kernels one at a time
pvr_status pvr_op_avgpool2(const void *in, void *out, int32_t n, int32_t h, int32_t w, int32_t c, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && out && n > 0 && (dtype == PVR_BF16 || dtype == PVR_F16), "pvr_op_avgpool2: null pointer, empty batch or not a 16-bit type");
    return launch_avgpool2(in, out, n, h, w, c, dtype, (hipStream_t)stream);
}
pvr_status pvr_op_attnpool_tokens(const float *x, const float *pos, void *tokens, int32_t n, int32_t hw, int32_t c, int32_t dtype, void *stream) {
    PVR_REQUIRE(x && pos && tokens && n > 0 && hw > 0 && c > 0 && (dtype == PVR_BF16 || dtype == PVR_F16), "pvr_op_attnpool_tokens: null pointer, empty input or not a 16-bit type");
    return launch_attnpool_tokens(x, pos, tokens, n, hw, c, dtype, (hipStream_t)stream);
}
pvr_status pvr_op_nhwc_to_chw(const float *in, float *out, int64_t out_stride, int32_t n, int32_t hw, int32_t cpad, int32_t creal, void *stream) {
    PVR_REQUIRE(in && out && n > 0 && hw > 0 && creal > 0 && creal <= cpad && out_stride >= (int64_t)hw * creal, "pvr_op_nhwc_to_chw: bad argument");
    return launch_nhwc_to_chw(in, out, out_stride, n, hw, cpad, creal, (hipStream_t)stream);
}
pvr_status pvr_op_f32_to_h(const float *in, void *out, int64_t count, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && out && count > 0 && (dtype == PVR_BF16 || dtype == PVR_F16), "pvr_op_f32_to_h: null pointer, empty input or not a 16-bit type");
    return launch_f32_to_h(in, out, (size_t)count, dtype, (hipStream_t)stream);
}
pvr_status pvr_op_h_to_f32(const void *in, float *out, int64_t count, int32_t dtype, void *stream) {
    PVR_REQUIRE(in && out && count > 0 && (dtype == PVR_BF16 || dtype == PVR_F16), "pvr_op_h_to_f32: null pointer, empty input or not a 16-bit type");
    return launch_h_to_f32(in, out, (size_t)count, dtype, (hipStream_t)stream);
}

// Finite check of an embedding block ON THE DEVICE: rows x cols fp32 with row stride `stride`; *flag (a device int32 the caller zeroed) is
// set to 1 if any value is inf / NaN.  stream_embed checks every batch this way and reads the flag once at the end, instead of a host pass over
// the whole result (np.isfinite over 31 310 floats x N frames of the 5-crop uber PVR was 19 % of that leg's wall clock).
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const float *x, long long rows, long long cols, long long stride, int *flag) {
    const long long n = rows * cols;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = x[(i / cols) * stride + (i % cols)];
        bad |= (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u;
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

pvr_status pvr_op_nonfinite_flag(const float *x, int64_t rows, int64_t cols, int64_t stride, int32_t *flag, void *stream) {
    PVR_REQUIRE(x && flag && rows >= 0 && cols > 0 && stride >= cols, "pvr_op_nonfinite_flag: bad argument");
    if (rows == 0) return PVR_OK;
    const long long n = rows * cols;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (long long)rows, (long long)cols, (long long)stride, flag);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// ViT kernels one by one (tests/test_gpu_vit_kernels.py): the launch dispatchers of vit.hip the encoder plans use, nothing else
pvr_status pvr_op_attention(const void *qkv, void *out, int32_t T, int32_t W, int32_t heads, int32_t nb, int32_t dtype, void *stream) {
    return launch_attention(qkv, out, T, W, heads, nb, dtype, (hipStream_t)stream);
}

pvr_status pvr_op_layernorm(const float *x, const float *patch_emb, const float *cls, const float *pos, const float *gamma, const float *beta,
                            float *out_f32, void *out_h, int32_t rows, int32_t T, int32_t W, float eps, int32_t normalize, int32_t dtype, void *stream) {
    return launch_layernorm(x, patch_emb, cls, pos, gamma, beta, out_f32, out_h, rows, T, W, eps, normalize, dtype, (hipStream_t)stream);
}

pvr_status pvr_op_cls_head(const float *x, const float *gamma, const float *beta, const float *proj_or_null, float *out, int64_t out_stride, int32_t nb,
                           int32_t T, int32_t W, int32_t out_dim, float eps, void *stream) {
    return launch_cls_head(x, gamma, beta, proj_or_null, out, out_stride, nb, T, W, out_dim, eps, (hipStream_t)stream);
}

int32_t pvr_debug_stem_u8_geometry_ok(const void *frames, int32_t h, int32_t w, int32_t top, int32_t left) { return stem_pool_u8_ok(frames, h, w, top, left) ? 1 : 0; }

// test hook: the uniform in (0, 1) the action sampler makes of 32 random bits (sample_rng.h) - host arithmetic, no GPU work
float pvr_debug_sample_uniform(uint32_t bits) { return pvr::uniform_open01(bits); }

// 1 when the library carries the round-3 experiment kernels (conv_w4, split-bf16 GEMM, fused / persistent BPTT: make EXPERIMENTS=1), else 0
int32_t pvr_has_experiments(void) {
#ifdef PVR_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

// host-only helper used by the CPU tests: the weight conversion finalize() applies
pvr_status pvr_debug_convert(const float *src, uint16_t *dst, int64_t n, int32_t dtype) {
    PVR_REQUIRE(src && dst, "pvr_debug_convert: null pointer");
    for (int64_t i = 0; i < n; ++i) dst[i] = f32_to_h(src[i], dtype);
    return PVR_OK;
}

}  // extern "C"
