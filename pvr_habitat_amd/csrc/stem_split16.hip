// conv1 of the fp32-parity mode on the 16-bit matrix pipe (dtype PVR_F32S): 7x7 / 2 pad 3 + folded BN + ReLU as the exact split product of conv_split16.hip.
//
// Where: torchvision's ResNet stem (conv1 -> bn1 -> relu, reference src/embeddings.py:112-120 through resnet.py / moco.py) on the normalised fp32 image.  It is
// the one convolution of the network conv_split16_kernel cannot take (cin = 3); in the PVR_F32 plan it runs as 196 f32-input MFMAs of K = 4 per 16 pixels
// (conv_f32.hip: stem_f32_kernel).
//
// How: the image arrives in the zero-bordered NHWC4 layout the 16-bit stem reads - (n, S + 6, S + 8, 4) fp32, pixel (y, x) at [y + 3][x + 3], channel 3 and
// the border (3 rows above and below, 3 columns left, 5 right) zero: zero in normalised space is exactly torch's padding.  Output pixel (oy, ox) then needs, for
// filter row a, the 8 columns x 4 channels = 32 consecutive floats at ((f (S + 6) + 2 oy + a) (S + 8) + 2 ox) 4: one contiguous, 32-byte-aligned 128-byte row
// piece, i.e. conv_split16's "128 B per pixel and step" staging with K = 7 rows x 32 = 224 in 7 steps and no per-element bounds test.  The weights are the
// folded fp32 [64][7][8][4] matrix (column 7 and channel 3 zero; K index (a 8 + b) 4 + c as in the 16-bit stem) through launch_split16_pack (rows 64, K 224).
//
// Kernel: 128 pixels x 64 couts per 512-thread workgroup (M = n S/2 S/2 pixel rows: 98 tiles per 224 x 224 frame).  A wave owns 16 couts x 64 pixels: per
// step its two 1 KB weight fragments come straight from L2 one step ahead, the pixels are split in registers and written to LDS as
// [hi, lo][k chunk][pixel ^ (2 chunk)][8] (8-byte stores and 16-byte fragment reads both conflict-free, see conv_split16.hip), double buffered, one barrier
// per step; three 16x16x32 f16 MFMAs per fragment pair into two accumulator sets, the cross terms scaled once in the epilogue.
#include "common.h"

namespace pvr {

constexpr int STEM_S16_BM = 128, STEM_S16_STEPS = 7;

__global__ __launch_bounds__(512) void stem_split16_kernel(const float *__restrict__ img, const u16 *__restrict__ wsp, const float *__restrict__ bias,
                                                           float *__restrict__ out, int S, int M, unsigned in_bytes) {
    constexpr int BM = STEM_S16_BM, NWC = 4, WP = 64, JT = 4, RPT = 2, NS = STEM_S16_STEPS;
    __shared__ __attribute__((aligned(16))) u16 sm[2][2][BM * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int wc = wave % NWC, wp = wave / NWC;
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM;
    const int So = S >> 1, PW = S + 8, PH = S + 6;
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(img), 0, in_bytes, 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16 *>(wsp), 0, 64 * 224 * 4, 0x00020000);
    constexpr int OOB = 0x7ffffff0;
    // pixel rows this thread loads: row (tid >> 3) + 64 i, 16-byte piece tid & 7 (= filter column b, 4 channels) of the step's 128 bytes
    const int piece = tid & 7, chunk = piece >> 1, half = piece & 1;
    const int row_bytes = PW * 16;                                                 // one image row: the stride of filter row a
    int a_off[RPT], s_off[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int row = (tid >> 3) + 64 * i, m = m0 + row;
        const int ox = m % So, t = m / So, oy = t % So, f = t / So;
        // rows past M (the ragged last tile) read nothing: the buffer load returns zeros for an offset past the image
        a_off[i] = m < M ? (((f * PH + 2 * oy) * PW + 2 * ox) * 4 + piece * 4) * 4 : OOB;
        s_off[i] = (chunk * BM + (row ^ (chunk << 1))) * 8 + half * 4;           // u16 elements
    }
    const int w_off = wc * NS * 2048 + lane * 16;                                 // bytes; + step * 2048 (+ 1024 for lo)
    f32x4 ra[RPT];
    f16x8 a_hi, a_lo, n_hi, n_lo;
#define PVR_ST_LOAD(ks_)                                                                                         \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < RPT; ++i) {                                                        \
            const int vo = a_off[i] == OOB ? OOB : a_off[i] + (ks_) * row_bytes;                                 \
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, vo, 0, 0));           \
        }                                                                                                        \
        n_hi = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_off, (ks_) * 2048, 0));   \
        n_lo = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_off + 1024, (ks_) * 2048, 0)); \
    }
#define PVR_ST_STORE(buf_)                                                                                       \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < RPT; ++i) {                                                        \
            const unsigned h01 = pack2_h<true>(ra[i][0], ra[i][1]), h23 = pack2_h<true>(ra[i][2], ra[i][3]);     \
            const pk_f16x2 q01 = __builtin_bit_cast(pk_f16x2, h01), q23 = __builtin_bit_cast(pk_f16x2, h23);     \
            *reinterpret_cast<uint2 *>(&sm[buf_][0][s_off[i]]) = make_uint2(h01, h23);                           \
            const unsigned l01 = pack2_h<true>((ra[i][0] - (float)q01[0]) * 2048.f, (ra[i][1] - (float)q01[1]) * 2048.f); \
            const unsigned l23 = pack2_h<true>((ra[i][2] - (float)q23[0]) * 2048.f, (ra[i][3] - (float)q23[1]) * 2048.f); \
            *reinterpret_cast<uint2 *>(&sm[buf_][1][s_off[i]]) = make_uint2(l01, l23);                           \
        }                                                                                                        \
    }
    f32x4 acc0[JT], acc1[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) { acc0[j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    PVR_ST_LOAD(0);
    PVR_ST_STORE(0);
    a_hi = n_hi; a_lo = n_lo;
    __syncthreads();
    // fragment read: pixel tile j of this wave, k chunk fq
    const int r_off = (fq * BM + ((wp * WP + fr) ^ (fq << 1))) * 8;                // + j * 16 * 8 (the XOR touches bits 1..2 only)
    int cur = 0;
#pragma unroll 1
    for (int ks = 0; ks < NS; ++ks) {
        const bool more = ks + 1 < NS;
        if (more) PVR_ST_LOAD(ks + 1);
        const u16 *Bh = sm[cur][0] + r_off, *Bl = sm[cur][1] + r_off;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const f16x8 bh = *reinterpret_cast<const f16x8 *>(Bh + j * 128);
            const f16x8 bl = *reinterpret_cast<const f16x8 *>(Bl + j * 128);
            acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, bh, acc0[j], 0, 0, 0);
            acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, bl, acc1[j], 0, 0, 0);
            acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, bh, acc1[j], 0, 0, 0);
        }
        if (more) { PVR_ST_STORE(cur ^ 1); a_hi = n_hi; a_lo = n_lo; }
        __syncthreads();
        cur ^= 1;
    }
#undef PVR_ST_LOAD
#undef PVR_ST_STORE
    // D: row = cout 4 fq + r, column = pixel fr: four consecutive couts of one pixel per lane
    const int co = wc * 16 + fq * 4;
    const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + co);
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        const int m = m0 + wp * WP + j * 16 + fr;
        if (m >= M) continue;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc0[j][r] + acc1[j][r] * (1.f / 2048.f) + bv[r], 0.f);
        *reinterpret_cast<f32x4 *>(out + (size_t)m * 64 + co) = v;
    }
}

static long long g_stem_split16_launches = 0;
long long stem_split16_launches() { return g_stem_split16_launches; }

// img: the zero-bordered fp32 NHWC4 image (n, S + 6, S + 8, 4); wsp: launch_split16_pack (rows 64, K 224) of the folded fp32 [64][7][8][4] weights;
// bias: 64 floats; out: fp32 (n, S / 2, S / 2, 64)
pvr_status launch_stem_split16(const float *img, const void *wsp, const float *bias, float *out, int n, int S, hipStream_t stream) {
    PVR_REQUIRE(img && wsp && bias && out, "stem_split16: null argument");
    PVR_REQUIRE(n > 0 && S >= 2 && S % 2 == 0, "stem_split16: n %d must be positive and the image size %d even", n, S);
    const int64_t M = (int64_t)n * (S / 2) * (S / 2), inb = (int64_t)n * (S + 6) * (S + 8) * 16;
    PVR_REQUIRE(M < (1ll << 31) - STEM_S16_BM && inb < 0x7ffffff0ll, "stem_split16: image batch larger than 2 GiB (use a smaller chunk)");
    ++g_stem_split16_launches;
    hipLaunchKernelGGL(stem_split16_kernel, dim3((unsigned)((M + STEM_S16_BM - 1) / STEM_S16_BM)), dim3(512), 0, stream, img, (const u16 *)wsp, bias, out, S, (int)M,
                       (unsigned)inb);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

}  // namespace pvr
