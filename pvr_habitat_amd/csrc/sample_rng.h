// Action sampling of PolicyNet.forward in training mode (reference src/models.py:78-80: torch.multinomial(F.softmax(policy_logits), 1)).
// One sample of softmax(l) per row through the Gumbel-max identity - argmax_a (l[a] - log(-log u_a)) is distributed as softmax(l) - with
// u from a counter-based Philox-4x32-10 stream keyed by the caller's seed and counted by (call, row, action / 4): the same (seed, call,
// row) gives the same action on any grid, nothing is stored between calls but the call counter.  Shared by the HIP plan (heads_kernel)
// and the host plan (host_policy.hip).  torch's own generator stream cannot be reproduced (its offsets depend on torch's launch
// geometry); the reference's contract here is the distribution, which tests/test_gpu_policy.py checks.
#pragma once
#include <cstdint>
#include <cmath>

namespace pvr {

__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// 32 random bits -> a uniform in the OPEN interval (0, 1): 23 bits, so that x + 0.5 is exact in fp32 (x < 2^23) and the result is never 0 or 1
// (with 24 bits, 2^24 - 1 + 0.5 rounds to 2^24: u = 1, -log(-log u) = +inf and that action would win whatever the logits say)
__host__ __device__ inline float uniform_open01(uint32_t bits) { return ((float)(bits >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// one sample of softmax(l[0..A)), A <= 16
__host__ __device__ inline int sample_softmax_row(const float *l, int A, uint64_t seed, uint64_t call, uint64_t row) {
    int best = 0;
    float bv = 0.f;
    for (int a0 = 0; a0 < A; a0 += 4) {
        uint32_t c[4] = {(uint32_t)row, (uint32_t)(row >> 32) ^ ((uint32_t)(a0 >> 2) << 24), (uint32_t)call, (uint32_t)(call >> 32)};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        for (int j = 0; j < 4 && a0 + j < A; ++j) {
            const float u = uniform_open01(c[j]);
            const float v = l[a0 + j] - logf(-logf(u));
            if ((a0 + j) == 0 || v > bv) { bv = v; best = a0 + j; }
        }
    }
    return best;
}

// The random crop window of one frame (pvr_op_crop_windows / pvr_host_crop_windows, include/pvr_train.h): counter (frame, call), key seed; top from the
// first word and left from the second by multiply-shift, (bits * (max + 1)) >> 32, which lies in [0, max].  A value's probability differs from
// 1 / (max + 1) by less than 2^-32: relative to it, a bias below (max + 1) 2^-32 <= 2^-26 for ranges of at most 64 values.  The window depends on
// (seed, call, frame) alone - not on the grid, and not on how a step's frames are cut into passes.  A negative max counts as 0.
__host__ __device__ inline void crop_window(uint64_t seed, uint64_t call, uint64_t frame, int32_t max_top, int32_t max_left, int32_t *top, int32_t *left) {
    uint32_t c[4] = {(uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    *top = (int32_t)(((uint64_t)c[0] * (uint64_t)((max_top < 0 ? 0 : max_top) + 1)) >> 32);
    *left = (int32_t)(((uint64_t)c[1] * (uint64_t)((max_left < 0 ? 0 : max_left) + 1)) >> 32);
}

// The colour-jitter parameters of one frame (pvr_op_color_params / pvr_host_color_params, include/pvr_train.h): counter (frame, call) as crop_window's,
// key (seed_lo, seed_hi ^ 'COLR'), so the stream is independent of the windows' and leaves them untouched.  Words 0 .. 2 give the brightness, contrast
// and saturation factors, torchvision's ranges: factor = fma(hi - lo, u, lo) with u = uniform_open01(bits), lo = max(0, 1 - strength), hi = 1 + strength
// (strength 0: fma(0, u, 1) = 1 exactly); word 3 gives the order code (bits * 6) >> 32 in 0 .. 5, the index of the frame's permutation of (brightness,
// contrast, saturation) in lexicographic order.  out: four 32-bit words, float b, float c, float s, int32 order.  The only multiply-add is the fma
// written out, so host and device agree bit for bit.  A negative or NaN strength counts as 0 (the callers refuse it before).
__host__ __device__ inline void color_params(uint64_t seed, uint64_t call, uint64_t frame, float strength_b, float strength_c, float strength_s,
                                             uint32_t *out) {
    uint32_t c[4] = {(uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ 0x434F4C52u);
    const float strength[3] = {strength_b, strength_c, strength_s};
    for (int j = 0; j < 3; ++j) {
        const float s = strength[j] > 0.f ? strength[j] : 0.f;
        const float lo = fmaxf(0.f, 1.0f - s), hi = 1.0f + s;
        const float f = fmaf(hi - lo, uniform_open01(c[j]), lo);
        __builtin_memcpy(&out[j], &f, 4);
    }
    out[3] = (uint32_t)(((uint64_t)c[3] * 6u) >> 32);
}

// The random-resized-crop rectangle of one frame (pvr_op_crop_rects / pvr_host_crop_rects, include/pvr_train.h): torchvision's
// RandomResizedCrop.get_params(scale = (lo, hi), ratio = (3/4, 4/3)) on an h x w frame -> out = (top, left, height, width).  Up to 10 tries; try t draws
// four words from Philox with counter (frame, call), as crop_window's, and key (seed_lo, (seed_hi ^ 'RECT') + t * 0x9E3779B9): a stream of its own per
// try, so the windows and the colour parameters of the same (seed, call) keep their bits.  Word 0: area = (h w) * fma(hi - lo, u, lo), u =
// uniform_open01; word 1: the ratio r = RRC_RATIO[bits >> 24]; cw = rint(sqrt(area * r)), ch = rint(sqrt(area / r)); the try is accepted if 0 < cw <= w
// and 0 < ch <= h; words 2 and 3: top in [0, h - ch] and left in [0, w - cw] by crop_window's multiply-shift.  After 10 refused tries, torchvision's
// fallback in integers: the whole frame if 3/4 <= w / h <= 4/3, else the centred rectangle of the nearest bound - width w and height round(4 w / 3) for a
// tall frame, height h and width round(4 h / 3) for a wide one (4 x / 3 is never a .5 tie) - with top = (h - ch) / 2 and left = (w - cw) / 2.
// How the ratio differs from torchvision's: there log r is continuous uniform on [log 3/4, log 4/3]; here it is one of the 256 midpoints
// log(3/4) + (k + 0.5) / 256 * log(16/9), each with probability 1/256, as fp32 literals - no expf / logf runs at draw time, whose results differ between
// host and device libraries.  The mean of log r is unchanged, its variance is smaller by (log(16/9) / 256)^2 / 12 = 4.2e-7 of 2.76e-2, and the rounding
// to whole pixels that follows is far coarser than the step between neighbouring ratios (0.22 %).  torch.rand's doubles are fp32 values here.  Only +, -,
// *, /, sqrtf, fmaf and rintf touch floats, each correctly rounded on host and device, with contraction off: the two agree bit for bit.
// A scale that is not finite or not 0 < lo <= hi <= 1 counts as (1, 1), h or w below 1 as 1 (the op refuses them before).
__host__ __device__ inline void crop_rect(uint64_t seed, uint64_t call, uint64_t frame, int32_t h, int32_t w, float lo, float hi, int32_t *out) {
#pragma clang fp contract(off)
    constexpr float RRC_RATIO[256] = {
        0.750843287f, 0.752532721f, 0.754225969f, 0.755922973f, 0.757623851f, 0.759328544f, 0.761037052f, 0.762749434f, 0.76446563f, 0.76618576f, 0.767909706f, 0.769637525f,
        0.771369219f, 0.773104846f, 0.774844348f, 0.776587784f, 0.778335154f, 0.780086458f, 0.781841695f, 0.783600867f, 0.785363972f, 0.787131071f, 0.788902164f, 0.790677249f,
        0.792456269f, 0.794239342f, 0.796026409f, 0.797817528f, 0.799612641f, 0.801411808f, 0.803215027f, 0.805022299f, 0.806833625f, 0.808649063f, 0.810468554f, 0.812292099f,
        0.814119816f, 0.815951645f, 0.817787528f, 0.819627583f, 0.82147181f, 0.82332015f, 0.825172663f, 0.827029347f, 0.828890204f, 0.830755234f, 0.832624435f, 0.834497929f,
        0.836375535f, 0.838257432f, 0.840143561f, 0.842033923f, 0.843928516f, 0.845827401f, 0.847730577f, 0.849637985f, 0.851549685f, 0.853465736f, 0.855386078f, 0.857310712f,
        0.859239697f, 0.861173034f, 0.863110721f, 0.86505276f, 0.866999149f, 0.86894995f, 0.870905101f, 0.872864664f, 0.874828696f, 0.87679708f, 0.878769934f, 0.880747199f,
        0.882728875f, 0.88471508f, 0.886705697f, 0.888700843f, 0.890700459f, 0.892704606f, 0.894713223f, 0.89672637f, 0.898744047f, 0.900766253f, 0.90279299f, 0.904824317f,
        0.906860232f, 0.908900678f, 0.910945773f, 0.912995458f, 0.915049732f, 0.917108595f, 0.919172168f, 0.92124033f, 0.923313141f, 0.925390661f, 0.92747283f, 0.929559648f,
        0.931651235f, 0.93374747f, 0.935848475f, 0.937954128f, 0.940064609f, 0.942179799f, 0.944299698f, 0.946424425f, 0.94855392f, 0.950688243f, 0.952827334f, 0.954971194f,
        0.957119942f, 0.959273517f, 0.961431921f, 0.963595152f, 0.96576333f, 0.967936337f, 0.970114231f, 0.972297013f, 0.974484742f, 0.976677358f, 0.978874922f, 0.981077433f,
        0.983284891f, 0.985497355f, 0.987714767f, 0.989937127f, 0.992164552f, 0.994396985f, 0.996634424f, 0.99887687f, 1.00112438f, 1.00337696f, 1.00563455f, 1.00789738f,
        1.0101651f, 1.01243806f, 1.01471603f, 1.01699924f, 1.01928759f, 1.02158093f, 1.02387953f, 1.02618337f, 1.02849233f, 1.03080642f, 1.03312588f, 1.03545046f,
        1.03778017f, 1.04011524f, 1.04245555f, 1.04480112f, 1.04715204f, 1.04950809f, 1.05186951f, 1.05423629f, 1.05660844f, 1.05898583f, 1.06136858f, 1.0637567f,
        1.06615019f, 1.06854904f, 1.07095337f, 1.07336307f, 1.07577813f, 1.07819867f, 1.0806247f, 1.08305621f, 1.08549309f, 1.08793545f, 1.09038341f, 1.09283686f,
        1.09529579f, 1.0977602f, 1.10023022f, 1.10270572f, 1.10518694f, 1.10767365f, 1.11016595f, 1.11266387f, 1.11516738f, 1.11767662f, 1.12019145f, 1.1227119f,
        1.12523806f, 1.12776983f, 1.13030744f, 1.13285065f, 1.13539958f, 1.13795435f, 1.14051473f, 1.14308095f, 1.14565289f, 1.14823067f, 1.15081429f, 1.15340364f,
        1.15599883f, 1.15859997f, 1.16120684f, 1.16381955f, 1.16643822f, 1.16906273f, 1.17169321f, 1.17432952f, 1.17697191f, 1.17962015f, 1.18227434f, 1.1849345f,
        1.18760061f, 1.19027281f, 1.19295096f, 1.19563508f, 1.1983254f, 1.20102167f, 1.20372403f, 1.20643246f, 1.20914698f, 1.21186757f, 1.21459436f, 1.21732724f,
        1.22006631f, 1.22281146f, 1.22556281f, 1.22832048f, 1.23108423f, 1.23385417f, 1.23663044f, 1.2394129f, 1.24220169f, 1.24499667f, 1.24779797f, 1.25060558f,
        1.2534194f, 1.25623965f, 1.25906634f, 1.26189923f, 1.26473856f, 1.26758432f, 1.27043641f, 1.27329493f, 1.27615988f, 1.27903128f, 1.28190923f, 1.28479362f,
        1.28768444f, 1.2905817f, 1.29348564f, 1.29639602f, 1.29931295f, 1.30223644f, 1.3051666f, 1.3081032f, 1.31104648f, 1.31399643f, 1.31695294f, 1.31991625f,
        1.32288611f, 1.32586265f, 1.32884586f, 1.33183587f
    };
    if (!(lo > 0.f && lo <= hi && hi <= 1.0f)) lo = hi = 1.0f;
    h = h < 1 ? 1 : h;
    w = w < 1 ? 1 : w;
    const float hw = (float)h * (float)w;
    for (uint32_t t = 0; t < 10; ++t) {
        uint32_t c[4] = {(uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
        philox4x32_10(c, (uint32_t)seed, ((uint32_t)(seed >> 32) ^ 0x52454354u) + t * 0x9E3779B9u);
        const float area = hw * fmaf(hi - lo, uniform_open01(c[0]), lo);
        const float r = RRC_RATIO[c[1] >> 24];
        const float fw = rintf(sqrtf(area * r)), fh = rintf(sqrtf(area / r));
        if (fw > 0.f && fw <= (float)w && fh > 0.f && fh <= (float)h) {
            const int32_t cw = (int32_t)fw, ch = (int32_t)fh;
            out[0] = (int32_t)(((uint64_t)c[2] * (uint64_t)(h - ch + 1)) >> 32);
            out[1] = (int32_t)(((uint64_t)c[3] * (uint64_t)(w - cw + 1)) >> 32);
            out[2] = ch;
            out[3] = cw;
            return;
        }
    }
    int64_t ch = h, cw = w;
    if (4 * (int64_t)w < 3 * (int64_t)h) ch = (8 * (int64_t)w + 3) / 6;            // w / h < 3/4: height round(w / (3/4)) < h
    else if (3 * (int64_t)w > 4 * (int64_t)h) cw = (8 * (int64_t)h + 3) / 6;       // w / h > 4/3: width round(h * (4/3)) < w
    out[0] = (int32_t)((h - ch) / 2);
    out[1] = (int32_t)((w - cw) / 2);
    out[2] = (int32_t)ch;
    out[3] = (int32_t)cw;
}

// The blur and grayscale parameters of one frame (pvr_op_blur_params / pvr_host_blur_params, include/pvr_train.h): counter (frame, call) as crop_window's,
// key (seed_lo, seed_hi ^ 'BLUR'), so the stream is independent of the windows', the rectangles' and the colour parameters' and leaves them untouched.
// With u_j = uniform_open01(word j): word 0 decides the blur (u_0 < p_blur), word 1 gives sigma = fma(hi - lo, u_1, lo) in [lo, hi], word 2 decides the
// grayscale (u_2 < p_gray).  u lies in the open interval (0, 1), so p = 1 always applies and p = 0 (or a NaN) never does.  out: two 32-bit words, float
// sigma (0: not blurred) and int32 gray (0 or 1).  The only multiply-add is the fma written out, so host and device agree bit for bit.  A sigma range that
// is not finite or not 0 < lo <= hi counts as (1, 1) (the callers refuse it before).
__host__ __device__ inline void blur_params(uint64_t seed, uint64_t call, uint64_t frame, float p_blur, float lo, float hi, float p_gray, uint32_t *out) {
    uint32_t c[4] = {(uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32) ^ 0x424C5552u);
    if (!(lo > 0.f && lo <= hi && hi <= 3.4e38f)) lo = hi = 1.0f;
    const float sigma = uniform_open01(c[0]) < p_blur ? fmaf(hi - lo, uniform_open01(c[1]), lo) : 0.f;
    __builtin_memcpy(&out[0], &sigma, 4);
    out[1] = uniform_open01(c[2]) < p_gray ? 1u : 0u;
}

}  // namespace pvr
