// K1+K2: uint8 NHWC frames -> Resize(short side) -> CenterCrop -> stem input image.
//
// Replaces reference src/embeddings.py:391-393 (.to(device), NHWC->NCHW transposes, the
// T.Resize/T.CenterCrop part of the transforms at :80-85).  ConvertImageDtype(/255) and
// Normalize are NOT applied here: they are folded into the stem weights (encoder.hip), so this
// kernel hands the stem the exact centred uint8 values x-128 (integers -128..127 are exact in bf16 and f16).
//
// torchvision 0.10 tensor Resize on uint8 = float32 bilinear (align_corners=False) then
// round-half-even back to uint8; restated in oracle/encoder_oracle.py:resize_u8.
//
// HBM-bound byte kernel: 3 B read (or 12 B for the 4 bilinear taps) + 8 B written per pixel.
// Output layout: (n, crop+6, crop+8, 4) 16-bit, pixel (y,x) at [y+3][x+3], channels
// (R-128,G-128,B-128,valid=1); the 3-pixel zero border (valid=0) is the conv1 padding and is never written.
#include "common.h"
#include "sample_rng.h"
#include "../../include/pvr_train.h"

namespace pvr {

struct PreP {
    const uint8_t *src;
    u16 *dst;
    int n, h, w;        // source frame size
    int rh, rw;         // size after Resize
    int top, left;      // crop offset inside the resized image
    int crop;
    int resize_needed;
    float scale_h, scale_w;
};

template <bool F16>
__global__ __launch_bounds__(256) void preprocess_kernel(PreP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (x >= p.crop || y >= p.crop) return;
    const int Y = y + p.top, X = x + p.left;
    const uint8_t *img = p.src + (size_t)n * p.h * p.w * 3;
    float v[3];
    if (!p.resize_needed) {
        const uint8_t *s = img + ((size_t)Y * p.w + X) * 3;
        v[0] = (float)s[0]; v[1] = (float)s[1]; v[2] = (float)s[2];
    } else {
#pragma clang fp contract(off)
        // ATen upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5, clamped at 0
        float sy = p.scale_h * ((float)Y + 0.5f) - 0.5f;
        float sx = p.scale_w * ((float)X + 0.5f) - 0.5f;
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < p.h - 1 ? 1 : 0), x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const uint8_t *r0 = img + (size_t)y0 * p.w * 3, *r1 = img + (size_t)y1 * p.w * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p00 = (float)r0[x0 * 3 + c], p01 = (float)r0[x1 * 3 + c];
            const float p10 = (float)r1[x0 * 3 + c], p11 = (float)r1[x1 * 3 + c];
            const float val = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
            v[c] = rintf(val);     // torch.round (half to even) then .to(uint8)
        }
    }
    const int PW = p.crop + 8, PH = p.crop + 6;
    ushort4 o;
    // centred values (x - 128, exact integers in bf16/f16): keeps the folded-Normalize products small, so the
    // 16-bit rounding of the stem weights is not amplified by the common-mode ~128 of every pixel
    o.x = to_h<F16>(v[0] - 128.f); o.y = to_h<F16>(v[1] - 128.f); o.z = to_h<F16>(v[2] - 128.f); o.w = to_h<F16>(1.0f);
    *reinterpret_cast<ushort4 *>(p.dst + (((size_t)n * PH + (y + 3)) * PW + (x + 3)) * 4) = o;
}

// host: resized size per torchvision resize(int size): smaller edge -> size, other edge int(size*long/short)
void resized_size(int h, int w, int size, int *rh, int *rw) {
    int sh = w <= h ? w : h, lg = w <= h ? h : w;
    if (sh == size) { *rh = h; *rw = w; return; }
    int ns = size, nl = (int)((double)size * (double)lg / (double)sh);
    if (w <= h) { *rw = ns; *rh = nl; } else { *rh = ns; *rw = nl; }
}

// the geometry launch_preprocess applies (for callers that fuse the no-resize case into their own kernel: stem_pool_lds_kernel<., true>)
void preprocess_geometry(int h, int w, int resize, int crop, int crop_pos, int *resize_needed, int *top, int *left) {
    int rh, rw;
    resized_size(h, w, resize, &rh, &rw);
    *resize_needed = (rh != h || rw != w) || rh < crop || rw < crop;
    *top = (int)nearbyint((rh - crop) / 2.0);
    *left = (int)nearbyint((rw - crop) / 2.0);
    if (crop_pos > 0) {
        *top = (crop_pos == 3 || crop_pos == 4) ? rh - crop : 0;
        *left = (crop_pos == 2 || crop_pos == 4) ? rw - crop : 0;
    }
}

// crop_pos: 0 centre (the reference's CenterCrop), 1 top-left, 2 top-right, 3 bottom-left, 4 bottom-right of the resized frame
// (the four corner crops of torchvision FiveCrop; build-defined 5-crop extension of BASELINE config 5)
pvr_status launch_preprocess(const uint8_t *frames, int n, int h, int w, int resize, int crop, void *out,
                             int dtype, hipStream_t stream, int crop_pos) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "preprocess: bad shape n=%d h=%d w=%d", n, h, w);
    PreP p;
    p.src = frames; p.dst = (u16 *)out; p.n = n; p.h = h; p.w = w; p.crop = crop;
    resized_size(h, w, resize, &p.rh, &p.rw);
    PVR_REQUIRE(p.rh >= crop && p.rw >= crop, "preprocess: resized frame %dx%d smaller than crop %d", p.rh, p.rw, crop);
    p.resize_needed = (p.rh != h || p.rw != w);
    // CenterCrop: int(round((H - crop) / 2.0)) with Python's round-half-even
    p.top = (int)nearbyint((p.rh - crop) / 2.0);
    p.left = (int)nearbyint((p.rw - crop) / 2.0);
    PVR_REQUIRE(crop_pos >= 0 && crop_pos <= 4, "preprocess: crop position %d outside 0..4", crop_pos);
    if (crop_pos > 0) {
        p.top = (crop_pos == 3 || crop_pos == 4) ? p.rh - crop : 0;
        p.left = (crop_pos == 2 || crop_pos == 4) ? p.rw - crop : 0;
    }
    p.scale_h = (float)h / (float)p.rh;
    p.scale_w = (float)w / (float)p.rw;
    dim3 grid((crop + 63) / 64, (crop + 3) / 4, n);
    if (dtype == PVR_F16) hipLaunchKernelGGL(preprocess_kernel<true>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(preprocess_kernel<false>, grid, dim3(256), 0, stream, p);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// The trainer's random-crop input (pvr_trainer_forward_windows): uint8 NHWC frames -> Resize -> a crop x crop window PER FRAME -> /255 -> Normalize, as
// the dense fp32 NHWC4 image (n, crop, crop, 4) conv1 and its weight gradient read, in ONE launch (preprocess_kernel + normalize_nhwc4_kernel take two
// and a 16-bit image in between), followed per pixel by normalize_nhwc4_kernel's expression.  HBM-bound: 3 B (12 B for the four taps) read + 16 B
// written per pixel.
// The bilinear sum is preprocess_kernel's geometry in the ROUNDING ORDER of ATen's host kernel, which is what oracle/encoder_oracle.py:resize_u8 runs:
// the source index is one fma, fma(scale, dst + 0.5, -0.5), and each two-tap sum is w0 * a + w1 * b as fma(w0, a, round(w1 * b)), along x and then
// along y.  preprocess_kernel rounds every product and sum by itself; the two orders agree wherever the arithmetic is exact - no resize, and the
// power-of-two scales of 64 x 64 and 128 x 128 frames, where this launch has the bits of preprocess + normalize at the same window - and at other
// scales they part at .5 ties of the sum, where preprocess_kernel can be one uint8 step away from the reference (tests/test_gpu_encoder.py allows it
// that) and this kernel is not: tests/test_random_crop_cpu.py restates the order in numpy and finds no differing value on whole resized frames.
struct WinP {
    const uint8_t *src;
    float *dst;
    const int32_t *windows;   // n x (top, left) in the resized frame; clamped here (the rect source: n x (top, left, height, width) in the frame itself)
    int n, h, w;              // source frame size
    int rh, rw;               // size after Resize
    int crop;
    int resize_needed;
    float scale_h, scale_w;
    float m0, m1, m2, s0, s1, s2;
};

// the resized frame's pixel (x, y) of frame n's window, x and y below crop, as three uint8 values held in floats: shared by the windows kernel and the two
// colour-jitter kernels below, which therefore see the same bits
__device__ __forceinline__ void window_pixel(const WinP &p, int n, int y, int x, float (&v)[3]) {
    // the frame's window, clamped to [0, rh - crop] x [0, rw - crop] (rh, rw >= crop: the launcher refuses smaller frames): whatever the array holds,
    // 0 <= Y < rh and 0 <= X < rw below, and every tap stays inside the frame
    int top = p.windows[2 * n], left = p.windows[2 * n + 1];
    top = top < 0 ? 0 : (top > p.rh - p.crop ? p.rh - p.crop : top);
    left = left < 0 ? 0 : (left > p.rw - p.crop ? p.rw - p.crop : left);
    const int Y = y + top, X = x + left;
    const uint8_t *img = p.src + (size_t)n * p.h * p.w * 3;
    if (!p.resize_needed) {
        const uint8_t *s = img + ((size_t)Y * p.w + X) * 3;
        v[0] = (float)s[0]; v[1] = (float)s[1]; v[2] = (float)s[2];
    } else {
#pragma clang fp contract(off)
        // ATen upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5 as one fma, clamped at 0 (only the fmas written out are fused)
        float sy = __builtin_fmaf(p.scale_h, (float)Y + 0.5f, -0.5f);
        float sx = __builtin_fmaf(p.scale_w, (float)X + 0.5f, -0.5f);
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        int y0 = (int)sy, x0 = (int)sx;
        y0 = y0 > p.h - 1 ? p.h - 1 : y0;          // (never taken for Y < rh, X < rw: the taps stay inside the frame whatever the rounding does)
        x0 = x0 > p.w - 1 ? p.w - 1 : x0;
        const int y1 = y0 + (y0 < p.h - 1 ? 1 : 0), x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const uint8_t *r0 = img + (size_t)y0 * p.w * 3, *r1 = img + (size_t)y1 * p.w * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p00 = (float)r0[x0 * 3 + c], p01 = (float)r0[x1 * 3 + c];
            const float p10 = (float)r1[x0 * 3 + c], p11 = (float)r1[x1 * 3 + c];
            const float a = __builtin_fmaf(hx, p00, lx * p01), b = __builtin_fmaf(hx, p10, lx * p11);
            const float val = __builtin_fmaf(hy, a, ly * b);
            v[c] = rintf(val);     // torch.round (half to even) then .to(uint8)
        }
    }
}

// Random resized crop (pvr_op_preprocess_rects, the trainer's "preprocess rects" launch): output pixel (x, y), x and y below crop, of frame n = the bilinear
// resize of the frame's OWN rectangle (top, left, height, width) - in the h x w frame, no Resize before it - to crop x crop, as three uint8 values held in
// floats: torchvision's resized_crop on a uint8 tensor, F.interpolate(bilinear, align_corners=False) of the cropped array and round-half-even, in
// window_pixel's rounding order.  Per frame and per axis scale = (float)size / (float)crop; the taps are clamped to the rectangle's last row and column,
// not the frame's - the crop comes first - and offset by (top, left).  A crop x crop rectangle is a plain copy (the same bits: at scale 1 the weights are 1
// and 0).  p.windows holds n x 4 int32 here; p.rh, p.rw, p.resize_needed and the scales are not read.  Hardened: height is clamped to [1, h], width to
// [1, w], top to [0, h - height], left to [0, w - width], so whatever the array holds every tap lies inside the frame and no value is a NaN.
__device__ __forceinline__ void rect_pixel(const WinP &p, int n, int y, int x, float (&v)[3]) {
    int top = p.windows[4 * n], left = p.windows[4 * n + 1], rh = p.windows[4 * n + 2], rw = p.windows[4 * n + 3];
    rh = rh < 1 ? 1 : (rh > p.h ? p.h : rh);
    rw = rw < 1 ? 1 : (rw > p.w ? p.w : rw);
    top = top < 0 ? 0 : (top > p.h - rh ? p.h - rh : top);
    left = left < 0 ? 0 : (left > p.w - rw ? p.w - rw : left);
    const uint8_t *img = p.src + ((size_t)n * p.h * p.w + (size_t)top * p.w + left) * 3;      // the rectangle's pixel (0, 0); rows stay p.w pixels apart
    if (rh == p.crop && rw == p.crop) {
        const uint8_t *s = img + ((size_t)y * p.w + x) * 3;
        v[0] = (float)s[0]; v[1] = (float)s[1]; v[2] = (float)s[2];
    } else {
#pragma clang fp contract(off)
        const float scale_h = (float)rh / (float)p.crop, scale_w = (float)rw / (float)p.crop;
        float sy = __builtin_fmaf(scale_h, (float)y + 0.5f, -0.5f);
        float sx = __builtin_fmaf(scale_w, (float)x + 0.5f, -0.5f);
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        int y0 = (int)sy, x0 = (int)sx;
        y0 = y0 > rh - 1 ? rh - 1 : y0;            // (never taken for y, x < crop; it keeps the taps inside the rectangle whatever the rounding does)
        x0 = x0 > rw - 1 ? rw - 1 : x0;
        const int y1 = y0 + (y0 < rh - 1 ? 1 : 0), x1 = x0 + (x0 < rw - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float hy = 1.f - ly, hx = 1.f - lx;
        const uint8_t *r0 = img + (size_t)y0 * p.w * 3, *r1 = img + (size_t)y1 * p.w * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p00 = (float)r0[x0 * 3 + c], p01 = (float)r0[x1 * 3 + c];
            const float p10 = (float)r1[x0 * 3 + c], p11 = (float)r1[x1 * 3 + c];
            const float a = __builtin_fmaf(hx, p00, lx * p01), b = __builtin_fmaf(hx, p10, lx * p11);
            const float val = __builtin_fmaf(hy, a, ly * b);
            v[c] = rintf(val);
        }
    }
}

// the two pixel sources of the image kernels and the colour kernels
struct WindowSource {
    static __device__ __forceinline__ void pixel(const WinP &p, int n, int y, int x, float (&v)[3]) { window_pixel(p, n, y, x, v); }
};
struct RectSource {
    static __device__ __forceinline__ void pixel(const WinP &p, int n, int y, int x, float (&v)[3]) { rect_pixel(p, n, y, x, v); }
};

// /255 and Normalize of three uint8 values, channel 3 = 0: one 16-byte store per pixel, a wave's 64 along x
__device__ __forceinline__ void store_normalized(const WinP &p, int n, int y, int x, const float (&v)[3]) {
    f32x4 o;
    o[0] = (v[0] / 255.0f - p.m0) / p.s0; o[1] = (v[1] / 255.0f - p.m1) / p.s1; o[2] = (v[2] / 255.0f - p.m2) / p.s2; o[3] = 0.f;
    reinterpret_cast<f32x4 *>(p.dst)[((size_t)n * p.crop + y) * p.crop + x] = o;
}

__global__ __launch_bounds__(256) void preprocess_windows_f32_kernel(WinP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (x >= p.crop || y >= p.crop) return;
    float v[3];
    window_pixel(p, n, y, x, v);
    store_normalized(p, n, y, x, v);
}

// "preprocess rects": the same grid and store, the pixel from the frame's rectangle
__global__ __launch_bounds__(256) void preprocess_rects_f32_kernel(WinP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (x >= p.crop || y >= p.crop) return;
    float v[3];
    rect_pixel(p, n, y, x, v);
    store_normalized(p, n, y, x, v);
}

// Colour jitter (pvr_op_preprocess_color, the trainer's "colour stats" and "preprocess colour" launches): torchvision's ColorJitter without hue on the
// uint8 values of the window, between window_pixel and store_normalized - where T.ColorJitter would sit between CenterCrop and ConvertImageDtype.
// Every product and sum is one fp32 rounding (contraction off), the blend's result is clamped to [0, 255] and truncated as .to(uint8) does:
//   gray(r, g, b) = trunc(((0.2989 r) + (0.587 g)) + (0.114 b));   blend(a, b, f) = trunc(clamp((f a) + ((1 - f) b), 0, 255))
//   brightness f: blend(v, 0, f);   saturation f: blend(v, gray(v), f);   contrast f: blend(v, m, f), m = (float)S / (float)(crop crop),
// S = the INTEGER sum of gray over the frame's window of the image as it stands when contrast is applied.  S <= 255 * 256^2 < 2^24 (the launcher refuses a larger crop), so (float)S is exact
// and m does not depend on the order of the sum: a parallel integer reduction gives the bits of torch.mean.  Per frame four words (float b, c, s and the
// int32 order code 0 .. 5 of the permutation of (brightness, contrast, saturation) in lexicographic order), hardened here: a NaN factor counts as 1, a
// factor is clamped to [0, 4] (4 * 255 and the blend stay finite: no NaN image), an order outside 0 .. 5 counts as 0.
struct ColP {
    WinP win;
    const uint32_t *color;    // n x (float b, float c, float s, int32 order)
    uint32_t *gray_sums;      // n integer sums, zeroed by the launcher before the stats kernel
    float pixels;             // (float)(crop * crop)
};

struct FrameColor {
    float f[3];               // brightness, contrast, saturation factors, hardened
    uint32_t ops;             // the frame's three ops, two bits each, first op lowest: 0 brightness, 1 contrast, 2 saturation
};

__device__ __forceinline__ FrameColor frame_color(const uint32_t *color, int n) {
    FrameColor fc;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float f = __uint_as_float(color[4 * n + j]);
        fc.f[j] = (f != f) ? 1.0f : (f < 0.f ? 0.f : (f > 4.0f ? 4.0f : f));
    }
    const uint32_t order = color[4 * n + 3];
    // the six permutations in lexicographic order: bcs, bsc, cbs, csb, sbc, scb
    const uint64_t table = 0x24ull | (0x18ull << 8) | (0x21ull << 16) | (0x09ull << 24) | (0x12ull << 32) | (0x06ull << 40);
    fc.ops = (uint32_t)(table >> (8 * (order < 6u ? order : 0u))) & 0x3fu;
    return fc;
}

__device__ __forceinline__ float gray_u8(const float (&v)[3]) {
#pragma clang fp contract(off)
    return truncf(((0.2989f * v[0]) + (0.587f * v[1])) + (0.114f * v[2]));
}

__device__ __forceinline__ float blend_u8(float a, float b, float f) {
#pragma clang fp contract(off)
    const float r = (f * a) + ((1.0f - f) * b);
    return truncf(r < 0.f ? 0.f : (r > 255.0f ? 255.0f : r));
}

// one op on the pixel; m: the frame's gray mean, read by contrast alone
__device__ __forceinline__ void color_op(float (&v)[3], uint32_t op, const FrameColor &fc, float m) {
    const float f = op == 0 ? fc.f[0] : (op == 1 ? fc.f[1] : fc.f[2]);
    const float g = gray_u8(v);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend_u8(v[c], op == 0 ? 0.f : (op == 1 ? m : g), f);
}

// "colour stats": gray_sums[n] += the gray values of frame n's window after the ops that precede contrast in the frame's order.  A workgroup walks
// STATS_ROWS rows of a 64-pixel column band, four rows at a time (a wave's 64 lanes along x, as the image kernels read); then a wave reduction, the
// block's four waves through LDS, and one integer atomicAdd per workgroup - 16 per 224 x 224 frame: with one per four rows (224 per frame) the launch
// was bound by the atomics on n neighbouring words, about twice the time of the image launch.  Integer addition commutes, so two runs give the same bits.
// No lane leaves before the shuffles; a lane outside the window adds 0 and reads nothing.
// Src: where a pixel comes from - WindowSource (window_pixel) or RectSource (rect_pixel, the random resized crop)
constexpr int STATS_ROWS = 56;

template <class Src>
__global__ __launch_bounds__(256) void color_stats_kernel(ColP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int n = blockIdx.z;
    unsigned g = 0;
    if (x < p.win.crop) {
        const FrameColor fc = frame_color(p.color, n);
        for (int r = 0; r < STATS_ROWS; r += 4) {
            const int y = blockIdx.y * STATS_ROWS + r + (threadIdx.x >> 6);
            if (y >= p.win.crop) break;
            float v[3];
            Src::pixel(p.win, n, y, x, v);
            uint32_t ops = fc.ops;
            for (int k = 0; k < 3 && (ops & 3u) != 1u; ++k, ops >>= 2) color_op(v, ops & 3u, fc, 0.f);
            g += (unsigned)gray_u8(v);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off, 64);
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = g;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&p.gray_sums[n], part[0] + part[1] + part[2] + part[3]);
}

// "preprocess colour": the image - the source's pixel, the frame's three ops in its order (contrast reads the finished sum), /255 and Normalize
template <class Src>
__global__ __launch_bounds__(256) void preprocess_color_f32_kernel(ColP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (x >= p.win.crop || y >= p.win.crop) return;
    const FrameColor fc = frame_color(p.color, n);
    const float m = (float)p.gray_sums[n] / p.pixels;
    float v[3];
    Src::pixel(p.win, n, y, x, v);
    uint32_t ops = fc.ops;
#pragma unroll
    for (int k = 0; k < 3; ++k, ops >>= 2) color_op(v, ops & 3u, fc, m);
    store_normalized(p.win, n, y, x, v);
}

// the checks and parameters the windows launch and the colour launches share; what: the launch's name in the refusals
static pvr_status window_params(const char *what, const uint8_t *frames, int n, int h, int w, int resize, int crop, const float *mean, const float *std_,
                                const int32_t *windows, float *out, WinP &p) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0 && crop > 0, "%s: bad shape n=%d h=%d w=%d crop=%d", what, n, h, w, crop);
    PVR_REQUIRE(n <= 65535, "%s: %d frames in one launch (at most 65535: one grid plane per frame)", what, n);
    p.src = frames; p.dst = out; p.windows = windows; p.n = n; p.h = h; p.w = w; p.crop = crop;
    resized_size(h, w, resize, &p.rh, &p.rw);
    PVR_REQUIRE(p.rh >= crop && p.rw >= crop, "%s: resized frame %dx%d smaller than crop %d", what, p.rh, p.rw, crop);
    PVR_REQUIRE(((uintptr_t)windows & 3) == 0, "%s: windows_dev %p is not 4-byte aligned (n x (top, left) int32)", what, (const void *)windows);
    PVR_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out_dev %p is not 16-byte aligned (a pixel is one float4 store)", what, (void *)out);
    p.resize_needed = (p.rh != h || p.rw != w);
    p.scale_h = (float)h / (float)p.rh;
    p.scale_w = (float)w / (float)p.rw;
    p.m0 = mean[0]; p.m1 = mean[1]; p.m2 = mean[2]; p.s0 = std_[0]; p.s1 = std_[1]; p.s2 = std_[2];
    return PVR_OK;
}

// the arguments have passed the callers' null checks
pvr_status launch_preprocess_windows(const uint8_t *frames, int n, int h, int w, int resize, int crop, const float *mean, const float *std_,
                                     const int32_t *windows, float *out, hipStream_t stream) {
    WinP p;
    if (pvr_status s = window_params("preprocess windows", frames, n, h, w, resize, crop, mean, std_, windows, out, p)) return s;
    dim3 grid((crop + 63) / 64, (crop + 3) / 4, n);
    hipLaunchKernelGGL(preprocess_windows_f32_kernel, grid, dim3(256), 0, stream, p);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// the colour checks and the launch of one stage, behind the source's own checks (p.win is filled)
template <class Src>
static pvr_status color_stage(int stage, ColP &p, int n, int crop, const void *color, uint32_t *gray_sums, hipStream_t stream) {
    PVR_REQUIRE(((uintptr_t)color & 3) == 0, "preprocess colour: color_dev %p is not 4-byte aligned (n x (float b, float c, float s, int32 order))", color);
    PVR_REQUIRE(((uintptr_t)gray_sums & 3) == 0, "preprocess colour: gray_sums_dev %p is not 4-byte aligned (n uint32 of scratch)", (void *)gray_sums);
    PVR_REQUIRE((int64_t)crop * crop <= (1 << 16), "preprocess colour: crop %d (at most 256: 255 crop^2 must stay below 2^24 for the gray mean to be exact)",
                crop);
    p.color = (const uint32_t *)color; p.gray_sums = gray_sums; p.pixels = (float)(crop * crop);
    dim3 grid((crop + 63) / 64, (crop + 3) / 4, n);
    if (stage == 0) {
        PVR_HIP_TRY(hipMemsetAsync(gray_sums, 0, (size_t)n * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(color_stats_kernel<Src>, dim3(grid.x, (crop + STATS_ROWS - 1) / STATS_ROWS, n), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(preprocess_color_f32_kernel<Src>, grid, dim3(256), 0, stream, p);
    }
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// the two launches of pvr_op_preprocess_color, one at a time so that the trainer can name and time each; both check everything before they launch.  The
// stats launch zeroes the n sums first (hipMemsetAsync on the same stream), so the scratch needs no state between calls.
pvr_status launch_color_stage(int stage, const uint8_t *frames, int n, int h, int w, int resize, int crop, const float *mean, const float *std_,
                              const int32_t *windows, const void *color, uint32_t *gray_sums, float *out, hipStream_t stream) {
    ColP p;
    if (pvr_status s = window_params("preprocess colour", frames, n, h, w, resize, crop, mean, std_, windows, out, p.win)) return s;
    return color_stage<WindowSource>(stage, p, n, crop, color, gray_sums, stream);
}

// the checks and parameters of the launches that read a rectangle per frame; what: the launch's name in the refusals.  No Resize comes before the
// rectangle, so a frame may be smaller than the crop.
static pvr_status rect_params(const char *what, const uint8_t *frames, int n, int h, int w, int crop, const float *mean, const float *std_,
                              const int32_t *rects, float *out, WinP &p) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0 && crop > 0, "%s: bad shape n=%d h=%d w=%d crop=%d", what, n, h, w, crop);
    PVR_REQUIRE(n <= 65535, "%s: %d frames in one launch (at most 65535: one grid plane per frame)", what, n);
    PVR_REQUIRE(((uintptr_t)rects & 3) == 0, "%s: rects_dev %p is not 4-byte aligned (n x (top, left, height, width) int32)", what, (const void *)rects);
    PVR_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out_dev %p is not 16-byte aligned (a pixel is one float4 store)", what, (void *)out);
    p.src = frames; p.dst = out; p.windows = rects; p.n = n; p.h = h; p.w = w; p.crop = crop;
    p.rh = h; p.rw = w; p.resize_needed = 0; p.scale_h = p.scale_w = 1.0f;        // (not read by rect_pixel: every frame has its own)
    p.m0 = mean[0]; p.m1 = mean[1]; p.m2 = mean[2]; p.s0 = std_[0]; p.s1 = std_[1]; p.s2 = std_[2];
    return PVR_OK;
}

// the arguments have passed the callers' null checks
pvr_status launch_preprocess_rects(const uint8_t *frames, int n, int h, int w, int crop, const float *mean, const float *std_, const int32_t *rects,
                                   float *out, hipStream_t stream) {
    WinP p;
    if (pvr_status s = rect_params("preprocess rects", frames, n, h, w, crop, mean, std_, rects, out, p)) return s;
    dim3 grid((crop + 63) / 64, (crop + 3) / 4, n);
    hipLaunchKernelGGL(preprocess_rects_f32_kernel, grid, dim3(256), 0, stream, p);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// launch_color_stage with the rectangle as the pixel source: the same two launches, checks and scratch
pvr_status launch_color_stage_rects(int stage, const uint8_t *frames, int n, int h, int w, int crop, const float *mean, const float *std_,
                                    const int32_t *rects, const void *color, uint32_t *gray_sums, float *out, hipStream_t stream) {
    ColP p;
    if (pvr_status s = rect_params("preprocess colour", frames, n, h, w, crop, mean, std_, rects, out, p.win)) return s;
    return color_stage<RectSource>(stage, p, n, crop, color, gray_sums, stream);
}

// Grayscale and Gaussian blur (pvr_op_preprocess_staged + pvr_op_blur_normalize, the trainer's "stage image" and "blur normalize" launches): the two
// augmentations that follow the colour jitter in MoCo v2's recipe.  A blurred pixel is no function of one source pixel, so the image is made in two steps:
// "stage image" writes the uint8 values the un-staged kernels would normalise - the source's pixel, then the frame's colour ops - as 4 bytes per pixel
// (r, g, b, 0), and "blur normalize" reads them back, a 23 x 23 neighbourhood per pixel.
struct StageP {
    ColP col;                 // col.win.dst is not written; col.color == nullptr: no colour ops, and gray_sums is not read
    uint32_t *staged;         // (n, crop, crop) packed pixels, r in the lowest byte
};

template <class Src>
__global__ __launch_bounds__(256) void stage_image_kernel(StageP p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (x >= p.col.win.crop || y >= p.col.win.crop) return;
    float v[3];
    Src::pixel(p.col.win, n, y, x, v);
    if (p.col.color) {        // (uniform over the launch) exactly preprocess_color_f32_kernel's ops
        const FrameColor fc = frame_color(p.col.color, n);
        const float m = (float)p.col.gray_sums[n] / p.col.pixels;
        uint32_t ops = fc.ops;
#pragma unroll
        for (int k = 0; k < 3; ++k, ops >>= 2) color_op(v, ops & 3u, fc, m);
    }
    // every value is an integer in [0, 255] held in a float (a resize rounds, a blend clamps and truncates): the conversion is exact
    p.staged[((size_t)n * p.col.win.crop + y) * p.col.win.crop + x] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
}

// "blur normalize": per frame grayscale if flagged (gray_u8 on all three channels: torchvision's rgb_to_grayscale(num_output_channels=3) on uint8), then
// torchvision's GaussianBlur(23, sigma) on the uint8 values if sigma > 0, then store_normalized.  The blur's weights are pdf_i = exp(-0.5 (i / sigma)^2),
// i = -11 .. 11, over their sum; the 2-D kernel is their outer product, so the filter is separable: a horizontal 23-tap pass and a vertical one, both in
// fp32 with nothing rounded in between, reflect padding of 11, and one rintf (half to even) at the end.  torchvision sums the 529 products of the 2-D
// kernel in fp32; the separable sum differs from it by rounding alone, about 1e-4 of a uint8 step (tests/gaussian_blur_refs.py derives the bound and the
// share of pixels near a .5 tie that it leaves undecided).
// A workgroup of 256 owns a BLUR_W x BLUR_H output tile of one frame.  It loads the tile plus an 11-pixel halo as packed uint8x4 into LDS, the reflection
// resolved (and the grayscale applied) at load time; the horizontal pass writes three fp32 planes of (BLUR_H + 22) x BLUR_W to LDS - one packed load feeds
// the three channels' sums; the vertical pass reads them, each lane producing BLUR_VR outputs down a column from a sliding run of BLUR_VR + 22 loads, so
// a loaded value feeds up to BLUR_VR taps.  In both passes a wave's 64 lanes lie along x: consecutive lanes read consecutive banks.  The 12 distinct
// weights are computed once per workgroup.  LDS: 54 x 86 x 4 + 3 x 54 x 64 x 4 + 48 = 60096 bytes, two workgroups (8 waves) per CU.
// A frame with sigma == 0 takes a branch that is uniform over the workgroup and touches no LDS: the staged pixel, gray if flagged, normalised.
// Hardened: a NaN or non-positive sigma means no blur, sigma is clamped to at most 16, tap 0's pdf is 1 by definition (a tiny sigma gives the identity,
// never 0 / 0), any non-zero gray word counts as 1, and every read is reflected and then clamped into the frame: no value of the array can produce a NaN
// image or a read outside the frame.  Plain loads and stores, no atomics.
constexpr int BLUR_R = 11, BLUR_W = 64, BLUR_H = 32, BLUR_VR = 8;
constexpr int BLUR_IW = BLUR_W + 2 * BLUR_R, BLUR_IH = BLUR_H + 2 * BLUR_R;

struct BlurP {
    WinP win;                 // dst, crop, mean and std: what store_normalized reads
    const uint32_t *staged;   // (n, crop, crop) packed pixels
    const uint32_t *blur;     // n x (float sigma, int32 gray)
};

__device__ __forceinline__ uint32_t gray_packed(uint32_t px) {
    const float v[3] = {(float)(px & 255u), (float)((px >> 8) & 255u), (float)((px >> 16) & 255u)};
    const uint32_t g = (uint32_t)gray_u8(v);      // (0.2989 + 0.587 + 0.114) * 255 < 256: at most 255
    return g | (g << 8) | (g << 16);
}

__global__ __launch_bounds__(256) void blur_normalize_kernel(BlurP p) {
    const int n = blockIdx.z, crop = p.win.crop;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * BLUR_W, y0 = blockIdx.y * BLUR_H;
    float sigma = __uint_as_float(p.blur[2 * n]);
    sigma = sigma > 0.f ? (sigma > 16.0f ? 16.0f : sigma) : 0.f;         // (a NaN compares false: no blur)
    const bool gray = p.blur[2 * n + 1] != 0u;
    const uint32_t *img = p.staged + (size_t)n * crop * crop;
    if (sigma == 0.f) {                           // uniform over the workgroup: no LDS, no barrier
        const int x = x0 + lane;
        if (x >= crop) return;
        for (int r = wave; r < BLUR_H; r += 4) {
            const int y = y0 + r;
            if (y >= crop) break;
            uint32_t px = img[(size_t)y * crop + x];
            if (gray) px = gray_packed(px);
            const float v[3] = {(float)(px & 255u), (float)((px >> 8) & 255u), (float)((px >> 16) & 255u)};
            store_normalized(p.win, n, y, x, v);
        }
        return;
    }
    __shared__ uint32_t s_in[BLUR_IH][BLUR_IW];
    __shared__ float s_h[3][BLUR_IH][BLUR_W];
    __shared__ float s_w[BLUR_R + 1];
    if (threadIdx.x <= BLUR_R) {
        const float t = (float)threadIdx.x / sigma;
        s_w[threadIdx.x] = threadIdx.x == 0 ? 1.0f : expf(-0.5f * (t * t));
    }
    for (int i = threadIdx.x; i < BLUR_IH * BLUR_IW; i += 256) {
        const int r = i / BLUR_IW, c = i - r * BLUR_IW;
        int y = y0 - BLUR_R + r, x = x0 - BLUR_R + c;
        y = y < 0 ? -y : (y >= crop ? 2 * (crop - 1) - y : y);          // reflect (crop >= 12: one reflection lands inside) ...
        x = x < 0 ? -x : (x >= crop ? 2 * (crop - 1) - x : x);
        y = y < 0 ? 0 : (y > crop - 1 ? crop - 1 : y);                  // ... then clamp: a tile that overhangs the frame reads inside it for the
        x = x < 0 ? 0 : (x > crop - 1 ? crop - 1 : x);                  // outputs it will not store
        const uint32_t px = img[(size_t)y * crop + x];
        s_in[r][c] = gray ? gray_packed(px) : px;
    }
    __syncthreads();
    float wt[BLUR_R + 1];                         // the normalised weights, the sum taken in one fixed order by every lane
    {
        float sum = 0.f;
#pragma unroll
        for (int i = BLUR_R; i >= 1; --i) sum += s_w[i];
        sum = 2.0f * sum + s_w[0];
#pragma unroll
        for (int i = 0; i <= BLUR_R; ++i) wt[i] = s_w[i] / sum;
    }
    // horizontal pass: a wave takes every fourth row of the haloed tile
    for (int r = wave; r < BLUR_IH; r += 4) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * BLUR_R + 1; ++k) {
            const uint32_t px = s_in[r][lane + k];
            const float w = wt[k < BLUR_R ? BLUR_R - k : k - BLUR_R];
            a0 = __builtin_fmaf(w, (float)(px & 255u), a0);
            a1 = __builtin_fmaf(w, (float)((px >> 8) & 255u), a1);
            a2 = __builtin_fmaf(w, (float)((px >> 16) & 255u), a2);
        }
        s_h[0][r][lane] = a0; s_h[1][r][lane] = a1; s_h[2][r][lane] = a2;
    }
    __syncthreads();
    // vertical pass: a wave takes BLUR_VR output rows, a lane one column of them
    const int x = x0 + lane, yb = wave * BLUR_VR;
    float o[3][BLUR_VR];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int j = 0; j < BLUR_VR; ++j) o[c][j] = 0.f;
#pragma unroll
        for (int r = 0; r < BLUR_VR + 2 * BLUR_R; ++r) {
            const float v = s_h[c][yb + r][lane];
#pragma unroll
            for (int j = 0; j < BLUR_VR; ++j) {
                const int k = r - j;              // the tap of output row j that row r is
                if (k >= 0 && k <= 2 * BLUR_R) o[c][j] = __builtin_fmaf(wt[k < BLUR_R ? BLUR_R - k : k - BLUR_R], v, o[c][j]);
            }
        }
    }
    if (x >= crop) return;
#pragma unroll
    for (int j = 0; j < BLUR_VR; ++j) {
        const int y = y0 + yb + j;
        if (y >= crop) break;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = rintf(o[c][j]);       // torch.round (half to even) then .to(uint8); the clamp never acts on a convex sum of uint8 values
            v[c] = r < 0.f ? 0.f : (r > 255.0f ? 255.0f : r);
        }
        store_normalized(p.win, n, y, x, v);
    }
}

// "stage image": the checks of the source's launcher, then the staging kernel.  color == nullptr: no colour ops.  The arguments have passed the
// callers' null checks
pvr_status launch_stage_image(const uint8_t *frames, int n, int h, int w, int resize, int crop, const int32_t *windows, const int32_t *rects,
                              const void *color, uint32_t *gray_sums, void *staged, hipStream_t stream) {
    PVR_REQUIRE(((uintptr_t)staged & 15) == 0, "stage image: staged_dev %p is not 16-byte aligned ((n, crop, crop, 4) uint8 of the caller's scratch)", staged);
    PVR_REQUIRE((windows != nullptr) != (rects != nullptr), "stage image: exactly one pixel source, windows_dev (n x (top, left)) or rects_dev (n x (top, "
                "left, height, width))");
    const float mean[3] = {0.f, 0.f, 0.f}, std_[3] = {1.f, 1.f, 1.f};     // (not read: the staged values are not normalised)
    StageP p;
    pvr_status s = windows ? window_params("stage image", frames, n, h, w, resize, crop, mean, std_, windows, (float *)staged, p.col.win)
                           : rect_params("stage image", frames, n, h, w, crop, mean, std_, rects, (float *)staged, p.col.win);
    if (s) return s;
    if (color) {
        PVR_REQUIRE(((uintptr_t)color & 3) == 0, "stage image: color_dev %p is not 4-byte aligned (n x (float b, float c, float s, int32 order))", color);
        PVR_REQUIRE(gray_sums && ((uintptr_t)gray_sums & 3) == 0, "stage image: gray_sums_dev %p is null or not 4-byte aligned (n uint32 of scratch)",
                    (void *)gray_sums);
        PVR_REQUIRE((int64_t)crop * crop <= (1 << 16), "stage image: crop %d (at most 256: 255 crop^2 must stay below 2^24 for the gray mean to be exact)", crop);
    }
    p.col.color = (const uint32_t *)color; p.col.gray_sums = gray_sums; p.col.pixels = (float)(crop * crop);
    p.staged = (uint32_t *)staged;
    dim3 grid((crop + 63) / 64, (crop + 3) / 4, n);
    if (windows) hipLaunchKernelGGL(stage_image_kernel<WindowSource>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(stage_image_kernel<RectSource>, grid, dim3(256), 0, stream, p);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// the "colour stats" launch of the staged path: launch_color_stage's or launch_color_stage_rects' stage 0, as it is (the image pointer is only checked)
pvr_status launch_staged_color_stats(const uint8_t *frames, int n, int h, int w, int resize, int crop, const int32_t *windows, const int32_t *rects,
                                     const void *color, uint32_t *gray_sums, void *staged, hipStream_t stream) {
    const float mean[3] = {0.f, 0.f, 0.f}, std_[3] = {1.f, 1.f, 1.f};
    PVR_REQUIRE(((uintptr_t)staged & 15) == 0, "stage image: staged_dev %p is not 16-byte aligned ((n, crop, crop, 4) uint8 of the caller's scratch)", staged);
    PVR_REQUIRE((windows != nullptr) != (rects != nullptr), "stage image: exactly one pixel source, windows_dev (n x (top, left)) or rects_dev (n x (top, "
                "left, height, width))");
    return windows ? launch_color_stage(0, frames, n, h, w, resize, crop, mean, std_, windows, color, gray_sums, (float *)staged, stream)
                   : launch_color_stage_rects(0, frames, n, h, w, crop, mean, std_, rects, color, gray_sums, (float *)staged, stream);
}

pvr_status launch_blur_normalize(const void *staged, int n, int crop, const float *mean, const float *std_, const void *blur, float *out,
                                 hipStream_t stream) {
    PVR_REQUIRE(n > 0, "blur normalize: bad shape n=%d crop=%d", n, crop);
    PVR_REQUIRE(n <= 65535, "blur normalize: %d frames in one launch (at most 65535: one grid plane per frame)", n);
    PVR_REQUIRE(crop >= BLUR_R + 1, "blur normalize: crop %d (at least 12: a reflect padding of 11 needs 12 pixels)", crop);
    PVR_REQUIRE(crop <= 256, "blur normalize: crop %d (at most 256, as the colour launches)", crop);
    PVR_REQUIRE(((uintptr_t)staged & 15) == 0, "blur normalize: staged_dev %p is not 16-byte aligned ((n, crop, crop, 4) uint8)", staged);
    PVR_REQUIRE(((uintptr_t)blur & 3) == 0, "blur normalize: blur_dev %p is not 4-byte aligned (n x (float sigma, int32 gray))", blur);
    PVR_REQUIRE(((uintptr_t)out & 15) == 0, "blur normalize: out_dev %p is not 16-byte aligned (a pixel is one float4 store)", (void *)out);
    BlurP p;
    p.win.src = nullptr; p.win.dst = out; p.win.windows = nullptr; p.win.n = n; p.win.h = p.win.w = p.win.rh = p.win.rw = crop; p.win.crop = crop;
    p.win.resize_needed = 0; p.win.scale_h = p.win.scale_w = 1.0f;
    p.win.m0 = mean[0]; p.win.m1 = mean[1]; p.win.m2 = mean[2]; p.win.s0 = std_[0]; p.win.s1 = std_[1]; p.win.s2 = std_[2];
    p.staged = (const uint32_t *)staged; p.blur = (const uint32_t *)blur;
    hipLaunchKernelGGL(blur_normalize_kernel, dim3((crop + BLUR_W - 1) / BLUR_W, (crop + BLUR_H - 1) / BLUR_H, n), dim3(256), 0, stream, p);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

__global__ __launch_bounds__(256) void blur_params_kernel(unsigned long long seed, unsigned long long call, long long first_frame, long long n, float p_blur,
                                                          float lo, float hi, float p_gray, uint32_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t w[2];
    blur_params(seed, call, (uint64_t)(first_frame + i), p_blur, lo, hi, p_gray, w);
    out[2 * i] = w[0]; out[2 * i + 1] = w[1];
}

__global__ __launch_bounds__(256) void crop_rects_kernel(unsigned long long seed, unsigned long long call, long long first_frame, long long n, int h, int w,
                                                         float lo, float hi, int32_t *__restrict__ rects) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t r[4];
    crop_rect(seed, call, (uint64_t)(first_frame + i), h, w, lo, hi, r);
    rects[4 * i] = r[0]; rects[4 * i + 1] = r[1]; rects[4 * i + 2] = r[2]; rects[4 * i + 3] = r[3];
}

__global__ __launch_bounds__(256) void color_params_kernel(unsigned long long seed, unsigned long long call, long long first_frame, long long n, float sb,
                                                           float sc, float ss, uint32_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4];
    color_params(seed, call, (uint64_t)(first_frame + i), sb, sc, ss, w);
    out[4 * i] = w[0]; out[4 * i + 1] = w[1]; out[4 * i + 2] = w[2]; out[4 * i + 3] = w[3];
}

__global__ __launch_bounds__(256) void crop_windows_kernel(unsigned long long seed, unsigned long long call, long long first_frame, long long n, int max_top,
                                                           int max_left, int32_t *__restrict__ windows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t top, left;
    crop_window(seed, call, (uint64_t)(first_frame + i), max_top, max_left, &top, &left);
    windows[2 * i] = top;
    windows[2 * i + 1] = left;
}

}  // namespace pvr

extern "C" {

pvr_status pvr_op_preprocess_windows(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const float *mean,
                                     const float *std_, const int32_t *windows, float *out, void *stream) {
    PVR_REQUIRE(frames && mean && std_ && windows && out, "pvr_op_preprocess_windows: null argument");
    return pvr::launch_preprocess_windows(frames, n, h, w, resize, crop, mean, std_, windows, out, (hipStream_t)stream);
}

void pvr_host_crop_windows(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t max_top, int32_t max_left, int32_t *windows) {
    for (int64_t i = 0; windows && i < n; ++i)
        pvr::crop_window(seed, call, (uint64_t)(first_frame + i), max_top, max_left, &windows[2 * i], &windows[2 * i + 1]);
}

pvr_status pvr_op_crop_windows(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t max_top, int32_t max_left, int32_t *windows,
                               void *stream) {
    PVR_REQUIRE(windows, "pvr_op_crop_windows: null windows_dev (n x (top, left) int32 of device memory)");
    PVR_REQUIRE(((uintptr_t)windows & 3) == 0, "pvr_op_crop_windows: windows_dev %p is not 4-byte aligned (int32 pairs)", (void *)windows);
    PVR_REQUIRE(n >= 1 && n <= (1ll << 31), "pvr_op_crop_windows: n = %lld frames (1 .. 2^31)", (long long)n);
    PVR_REQUIRE(first_frame >= 0, "pvr_op_crop_windows: first_frame = %lld (a frame index of the step, 0 or above)", (long long)first_frame);
    PVR_REQUIRE(max_top >= 0 && max_left >= 0, "pvr_op_crop_windows: max_top = %d, max_left = %d (the largest legal offsets, resized size - crop: 0 or above)",
                max_top, max_left);
    hipLaunchKernelGGL(pvr::crop_windows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)call, (long long)first_frame, (long long)n, (int)max_top, (int)max_left, windows);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_preprocess_color(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const float *mean,
                                   const float *std_, const int32_t *windows, const void *color, uint32_t *gray_sums, float *out, void *stream) {
    PVR_REQUIRE(frames && mean && std_ && windows && out, "pvr_op_preprocess_color: null argument");
    PVR_REQUIRE(color, "pvr_op_preprocess_color: null color_dev (n x (float b, float c, float s, int32 order) of device memory)");
    PVR_REQUIRE(gray_sums, "pvr_op_preprocess_color: null gray_sums_dev (n uint32 of device scratch, the caller's)");
    for (int stage = 0; stage < 2; ++stage)
        if (pvr_status s = pvr::launch_color_stage(stage, frames, n, h, w, resize, crop, mean, std_, windows, color, gray_sums, out, (hipStream_t)stream))
            return s;
    return PVR_OK;
}

void pvr_host_crop_rects(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t h, int32_t w, float scale_lo, float scale_hi,
                         int32_t *rects) {
    for (int64_t i = 0; rects && i < n; ++i) pvr::crop_rect(seed, call, (uint64_t)(first_frame + i), h, w, scale_lo, scale_hi, rects + 4 * i);
}

pvr_status pvr_op_crop_rects(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, int32_t h, int32_t w, float scale_lo, float scale_hi,
                             int32_t *rects, void *stream) {
    PVR_REQUIRE(rects, "pvr_op_crop_rects: null rects_dev (n x (top, left, height, width) int32 of device memory)");
    PVR_REQUIRE(((uintptr_t)rects & 3) == 0, "pvr_op_crop_rects: rects_dev %p is not 4-byte aligned (four int32 per frame)", (void *)rects);
    PVR_REQUIRE(n >= 1 && n <= (1ll << 31), "pvr_op_crop_rects: n = %lld frames (1 .. 2^31)", (long long)n);
    PVR_REQUIRE(first_frame >= 0, "pvr_op_crop_rects: first_frame = %lld (a frame index of the step, 0 or above)", (long long)first_frame);
    PVR_REQUIRE(h >= 1 && w >= 1, "pvr_op_crop_rects: frame size h = %d, w = %d (1 or above)", h, w);
    PVR_REQUIRE(scale_lo > 0.f && scale_lo <= scale_hi && scale_hi <= 1.0f, "pvr_op_crop_rects: scale (%g, %g) (the rectangle's share of the frame's area: "
                "finite, 0 < lo <= hi <= 1)", (double)scale_lo, (double)scale_hi);
    hipLaunchKernelGGL(pvr::crop_rects_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)call, (long long)first_frame, (long long)n, (int)h, (int)w, scale_lo, scale_hi, rects);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_preprocess_rects(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t crop, const float *mean, const float *std_,
                                   const int32_t *rects, const void *color, uint32_t *gray_sums, float *out, void *stream) {
    PVR_REQUIRE(frames && mean && std_ && out, "pvr_op_preprocess_rects: null argument");
    PVR_REQUIRE(rects, "pvr_op_preprocess_rects: null rects_dev (n x (top, left, height, width) int32 of device memory)");
    if (!color) return pvr::launch_preprocess_rects(frames, n, h, w, crop, mean, std_, rects, out, (hipStream_t)stream);
    PVR_REQUIRE(gray_sums, "pvr_op_preprocess_rects: color_dev without gray_sums_dev (n uint32 of device scratch, the caller's)");
    for (int stage = 0; stage < 2; ++stage)
        if (pvr_status s = pvr::launch_color_stage_rects(stage, frames, n, h, w, crop, mean, std_, rects, color, gray_sums, out, (hipStream_t)stream))
            return s;
    return PVR_OK;
}

void pvr_host_color_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float strength_b, float strength_c, float strength_s,
                           void *params) {
    for (int64_t i = 0; params && i < n; ++i)
        pvr::color_params(seed, call, (uint64_t)(first_frame + i), strength_b, strength_c, strength_s, (uint32_t *)params + 4 * i);
}

pvr_status pvr_op_color_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float strength_b, float strength_c, float strength_s,
                               void *params, void *stream) {
    PVR_REQUIRE(params, "pvr_op_color_params: null color_dev (n x (float b, float c, float s, int32 order) of device memory)");
    PVR_REQUIRE(((uintptr_t)params & 3) == 0, "pvr_op_color_params: color_dev %p is not 4-byte aligned (four 32-bit words per frame)", params);
    PVR_REQUIRE(n >= 1 && n <= (1ll << 31), "pvr_op_color_params: n = %lld frames (1 .. 2^31)", (long long)n);
    PVR_REQUIRE(first_frame >= 0, "pvr_op_color_params: first_frame = %lld (a frame index of the step, 0 or above)", (long long)first_frame);
    PVR_REQUIRE(strength_b >= 0.f && strength_c >= 0.f && strength_s >= 0.f && strength_b <= 3.4e38f && strength_c <= 3.4e38f && strength_s <= 3.4e38f,
                "pvr_op_color_params: strengths %g, %g, %g (brightness, contrast, saturation: finite, 0 or above; 0 leaves that factor at 1)",
                (double)strength_b, (double)strength_c, (double)strength_s);
    hipLaunchKernelGGL(pvr::color_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)call, (long long)first_frame, (long long)n, strength_b, strength_c, strength_s, (uint32_t *)params);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

void pvr_host_blur_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float p_blur, float sigma_lo, float sigma_hi, float p_gray,
                          void *params) {
    for (int64_t i = 0; params && i < n; ++i)
        pvr::blur_params(seed, call, (uint64_t)(first_frame + i), p_blur, sigma_lo, sigma_hi, p_gray, (uint32_t *)params + 2 * i);
}

pvr_status pvr_op_blur_params(uint64_t seed, uint64_t call, int64_t first_frame, int64_t n, float p_blur, float sigma_lo, float sigma_hi, float p_gray,
                              void *params, void *stream) {
    PVR_REQUIRE(params, "pvr_op_blur_params: null blur_dev (n x (float sigma, int32 gray) of device memory)");
    PVR_REQUIRE(((uintptr_t)params & 3) == 0, "pvr_op_blur_params: blur_dev %p is not 4-byte aligned (two 32-bit words per frame)", params);
    PVR_REQUIRE(n >= 1 && n <= (1ll << 31), "pvr_op_blur_params: n = %lld frames (1 .. 2^31)", (long long)n);
    PVR_REQUIRE(first_frame >= 0, "pvr_op_blur_params: first_frame = %lld (a frame index of the step, 0 or above)", (long long)first_frame);
    PVR_REQUIRE(p_blur >= 0.f && p_blur <= 1.0f && p_gray >= 0.f && p_gray <= 1.0f, "pvr_op_blur_params: probabilities %g (blur), %g (grayscale) (finite, "
                "in [0, 1])", (double)p_blur, (double)p_gray);
    PVR_REQUIRE(sigma_lo > 0.f && sigma_lo <= sigma_hi && sigma_hi <= 3.4e38f, "pvr_op_blur_params: sigma range (%g, %g) (finite, 0 < lo <= hi)",
                (double)sigma_lo, (double)sigma_hi);
    hipLaunchKernelGGL(pvr::blur_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long)seed,
                       (unsigned long long)call, (long long)first_frame, (long long)n, p_blur, sigma_lo, sigma_hi, p_gray, (uint32_t *)params);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_preprocess_staged(const uint8_t *frames, int32_t n, int32_t h, int32_t w, int32_t resize, int32_t crop, const int32_t *windows,
                                    const int32_t *rects, const void *color, uint32_t *gray_sums, void *staged, void *stream) {
    PVR_REQUIRE(frames, "pvr_op_preprocess_staged: null frames_dev");
    PVR_REQUIRE(staged, "pvr_op_preprocess_staged: null staged_dev ((n, crop, crop, 4) uint8 of device scratch, the caller's)");
    PVR_REQUIRE((windows != nullptr) != (rects != nullptr), "pvr_op_preprocess_staged: exactly one pixel source, windows_dev (n x (top, left)) or rects_dev "
                "(n x (top, left, height, width))");
    if (color) {
        PVR_REQUIRE(gray_sums, "pvr_op_preprocess_staged: color_dev without gray_sums_dev (n uint32 of device scratch, the caller's)");
        // (everything the second launch checks, before the first one runs: a refusal launches nothing)
        PVR_REQUIRE(((uintptr_t)staged & 15) == 0, "pvr_op_preprocess_staged: staged_dev %p is not 16-byte aligned", staged);
        if (pvr_status s = pvr::launch_staged_color_stats(frames, n, h, w, resize, crop, windows, rects, color, gray_sums, staged, (hipStream_t)stream))
            return s;
    }
    return pvr::launch_stage_image(frames, n, h, w, resize, crop, windows, rects, color, gray_sums, staged, (hipStream_t)stream);
}

pvr_status pvr_op_blur_normalize(const void *staged, int32_t n, int32_t crop, const float *mean, const float *std_, const void *blur, float *out,
                                 void *stream) {
    PVR_REQUIRE(staged && mean && std_ && out, "pvr_op_blur_normalize: null argument");
    PVR_REQUIRE(blur, "pvr_op_blur_normalize: null blur_dev (n x (float sigma, int32 gray) of device memory)");
    return pvr::launch_blur_normalize(staged, n, crop, mean, std_, blur, out, (hipStream_t)stream);
}

}  // extern "C"
