// Forward convolutions and data gradients of the trainable encoder as exact-split products on the f16 matrix pipe (pvr_trainer_set_conv_split16;
// include/pvr_train.h: pvr_op_conv_fwd_split16 / pvr_op_conv_dgrad_split16).
//
// Arithmetic: conv_split16.hip's split (a = a_hi + 2^-11 a_lo, three v_mfma_f32_16x16x32_f16 per fragment pair, the two cross terms in a second fp32
// accumulator that is scaled by 2^-11 once) with BOTH operands first multiplied by a per-tensor power of two s = 2^(14 - floor(log2 max|t|))
// (pvr_op_absmax_scale's rule: the scaled maximum lies in [2^14, 2^15)).  conv_split16_kernel has no such scale: it serves frozen plans whose operands
// are O(1).  A trainer's operands are not: dz has magnitudes near 1e-6 (its f16 high parts would be subnormal), weights may be 1e-5, an activation
// behind a large BatchNorm gamma may pass 65504.  The scales are read from device memory (no host synchronisation); the epilogue multiplies by 1 / s_x
// and 1 / s_w (powers of two: exact) and adds the optional fp32 operand - the data gradient's accumulate form - with one fp32 addition.  No bias, no
// activation, no 16-bit output.  The BNF instance is the frozen prefix op of the trainer as ONE launch behind the pack (pvr_trainer_set_prefix_fused): the same
// K loop and scale undoing give the pre-BN z in registers, and the epilogue is bn_frozen_apply_kernel's expression per element,
// y = (z - running_mean) * rstd * gamma + beta [+ residual] [ReLU] with rstd = 1 / sqrtf(running_var + 1e-5f), in that kernel's order of roundings
// (subtract, multiply, one fma, add, max): the bits of pvr_op_conv_fwd_split16 followed by pvr_op_bn_frozen_forward; no z, mean or rstd is written.
//
// Kernel: the implicit GEMM of conv_split16_kernel<BM, BN, 3>: BM pixels x BN couts per 512-thread workgroup, K steps of 32 channels of one tap;
//   * weights: split16_scaled_pack_kernel reads torch's (cout, cin, k, k), multiplies by *s_w, splits, and writes MFMA A fragments
//     [cout >> 4][k >> 5][hi, lo][k chunk][cout & 15][8] - the forward matrix (rows = cout, K = (tap, cin)) or, for the data gradient, the rotated,
//     transposed one (rows = cin, K = (rot180 tap, cout)) in the same launch; rows are padded with zeros to a multiple of 64.  A wave owns 16 rows and
//     reads its two 1 KB fragments per step straight from L2, one step ahead
//   * pixels: fp32 NHWC rows are loaded one step ahead, multiplied by *s_x, split in registers and written to LDS as
//     [hi, lo][k chunk][pixel ^ (2 * chunk)][8] (8-byte stores and 16-byte fragment reads are conflict-free), double buffered, one barrier per step
// No float atomics: an output element is one workgroup's register sum, two runs give the same bits.
// The data gradient of a stride-2 convolution keeps dilate2_kernel's zero-filled grid (zeros do not move a maximum: the grid's scale is dz's).
#include "common.h"
#include "train_internal.h"
#include "../../include/pvr_train.h"

namespace pvr {

struct ConvSS {
    const float *in, *res, *sx, *sw;
    const u16 *w;
    float *out;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, M, n_ctiles, nsteps;
    unsigned in_bytes, w_bytes;
    const float *gamma, *beta, *run_mean, *run_var;      // BNF only: the frozen BatchNorm of the epilogue
    int relu;
};

template <int BM, int BN, bool BNF = false>
__global__ __launch_bounds__(512) void conv_split16_scaled_kernel(ConvSS p) {
    constexpr int NWC = BN / 16, NWP = 8 / NWC, WP = BM / NWP, JT = WP / 16, RPT = BM / 64;
    static_assert(NWC * NWP == 8 && WP % 16 == 0 && RPT >= 1, "tile shape");
    __shared__ __attribute__((aligned(16))) u16 sm[2][2][BM * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int wc = wave % NWC, wp = wave / NWC;
    const int swz = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (swz / p.n_ctiles) * BM, n0 = (swz % p.n_ctiles) * BN;
    const auto rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in), 0, p.in_bytes, 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16 *>(p.w), 0, p.w_bytes, 0x00020000);
    constexpr int OOB = 0x7ffffff0;
    const float sx = *p.sx;
    // pixel rows this thread loads: row (tid >> 3) + 64 i, 16-byte piece tid & 7 of the step's 128 bytes
    const int piece = tid & 7, chunk = piece >> 1, half = piece & 1;
    int a_off[RPT], a_mask[RPT], s_off[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int row = (tid >> 3) + 64 * i, m = m0 + row;
        const bool ok = m < p.M;
        const int mm = ok ? m : 0;
        const int wo = mm % p.Wo, t = mm / p.Wo, ho = t % p.Ho, n = t / p.Ho;
        const int hi0 = ho * p.stride - p.pad, wi0 = wo * p.stride - p.pad;
        a_off[i] = (((n * p.H + hi0) * p.W + wi0) * p.Cin + piece * 4) * 4;
        int hb = 0, wb = 0;
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) {
            hb |= (int)(ok && t3 < p.KH && (unsigned)(hi0 + t3) < (unsigned)p.H) << t3;
            wb |= (int)(t3 < p.KW && (unsigned)(wi0 + t3) < (unsigned)p.W) << t3;
        }
        int mask = 0;
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) mask |= ((hb >> t3) & 1) ? (wb << (t3 * p.KW)) : 0;
        a_mask[i] = mask;
        s_off[i] = (chunk * BM + (row ^ (chunk << 1))) * 8 + half * 4;          // u16 elements
    }
    // weight fragments of this wave: [row block][step][hi, lo][512 elements], lane-linear 16 bytes
    const int cb = (n0 >> 4) + wc;
    const int w_off = cb * p.nsteps * 2048 + lane * 16;                          // bytes; + step * 2048 (+ 1024 for lo)
    const int cpt = p.Cin / 32;
    int kh = 0, kw = 0, cs = 0, tap = 0;
    f32x4 ra[RPT];
    f16x8 a_hi, a_lo, n_hi, n_lo;
#define PVR_SS_LOAD(ks_)                                                                                         \
    {                                                                                                            \
        const int tap_off = ((kh * p.W + kw) * p.Cin + cs * 32) * 4;                                             \
        _Pragma("unroll") for (int i = 0; i < RPT; ++i) {                                                        \
            const int vo = ((a_mask[i] >> tap) & 1) ? a_off[i] + tap_off : OOB;                                  \
            ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, vo, 0, 0));           \
        }                                                                                                        \
        n_hi = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_off, (ks_) * 2048, 0));   \
        n_lo = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, w_off + 1024, (ks_) * 2048, 0)); \
        if (++cs == cpt) { cs = 0; ++tap; if (++kw == p.KW) { kw = 0; ++kh; } }                                  \
    }
#define PVR_SS_STORE(buf_)                                                                                       \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < RPT; ++i) {                                                        \
            const f32x4 v = ra[i] * sx;                                                                          \
            const unsigned h01 = pack2_h<true>(v[0], v[1]), h23 = pack2_h<true>(v[2], v[3]);                     \
            const pk_f16x2 q01 = __builtin_bit_cast(pk_f16x2, h01), q23 = __builtin_bit_cast(pk_f16x2, h23);     \
            *reinterpret_cast<uint2 *>(&sm[buf_][0][s_off[i]]) = make_uint2(h01, h23);                           \
            const unsigned l01 = pack2_h<true>((v[0] - (float)q01[0]) * 2048.f, (v[1] - (float)q01[1]) * 2048.f); \
            const unsigned l23 = pack2_h<true>((v[2] - (float)q23[0]) * 2048.f, (v[3] - (float)q23[1]) * 2048.f); \
            *reinterpret_cast<uint2 *>(&sm[buf_][1][s_off[i]]) = make_uint2(l01, l23);                           \
        }                                                                                                        \
    }
    f32x4 acc0[JT], acc1[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) { acc0[j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    PVR_SS_LOAD(0);
    PVR_SS_STORE(0);
    a_hi = n_hi; a_lo = n_lo;
    __syncthreads();
    // fragment read: pixel tile j of this wave, k chunk fq
    const int r_off = (fq * BM + ((wp * WP + fr) ^ (fq << 1))) * 8;                // + j * 16 * 8 (the XOR touches bits 1..2 only)
    int cur = 0;
    for (int ks = 0; ks < p.nsteps; ++ks) {
        const bool more = ks + 1 < p.nsteps;
        if (more) PVR_SS_LOAD(ks + 1);
        const u16 *Bh = sm[cur][0] + r_off, *Bl = sm[cur][1] + r_off;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const f16x8 bh = *reinterpret_cast<const f16x8 *>(Bh + j * 128);
            const f16x8 bl = *reinterpret_cast<const f16x8 *>(Bl + j * 128);
            acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, bh, acc0[j], 0, 0, 0);
            acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_hi, bl, acc1[j], 0, 0, 0);
            acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_lo, bh, acc1[j], 0, 0, 0);
        }
        if (more) { PVR_SS_STORE(cur ^ 1); a_hi = n_hi; a_lo = n_lo; }
        __syncthreads();
        cur ^= 1;
    }
#undef PVR_SS_LOAD
#undef PVR_SS_STORE
    // D: row = cout 4 fq + r, column = pixel fr: four consecutive couts of one pixel per lane (Cout % 4 == 0: they exist together)
    const int co = n0 + wc * 16 + fq * 4;
    if (co >= p.Cout) return;
    const float ix = 1.f / sx, iw = 1.f / *p.sw;                                  // powers of two, exponents in [-126, 126]: exact and normal
    if constexpr (BNF) {
        // a lane's four channels are the same for every pixel tile: their constants are loaded once, outside the pixel loop
        float mu[4], rs[4], ga[4], be[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mu[r] = p.run_mean[co + r]; rs[r] = 1.f / sqrtf(p.run_var[co + r] + 1e-5f);
            ga[r] = p.gamma[co + r]; be[r] = p.beta[co + r];
        }
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const int m = m0 + wp * WP + j * 16 + fr;
            if (m >= p.M) continue;
            f32x4 rv = f32x4{0.f, 0.f, 0.f, 0.f}, o;
            if (p.res) rv = *reinterpret_cast<const f32x4 *>(p.res + (size_t)m * p.Cout + co);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = ((acc0[j][r] + acc1[j][r] * (1.f / 2048.f)) * ix) * iw;
                float t = __fmaf_rn(__fmul_rn(__fsub_rn(z, mu[r]), rs[r]), ga[r], be[r]);
                if (p.res) t = __fadd_rn(t, rv[r]);
                o[r] = p.relu ? fmaxf(t, 0.f) : t;
            }
            *reinterpret_cast<f32x4 *>(p.out + (size_t)m * p.Cout + co) = o;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        const int m = m0 + wp * WP + j * 16 + fr;
        if (m >= p.M) continue;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = ((acc0[j][r] + acc1[j][r] * (1.f / 2048.f)) * ix) * iw;
        if (p.res) {
            const f32x4 rv = *reinterpret_cast<const f32x4 *>(p.res + (size_t)m * p.Cout + co);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += rv[r];
        }
        *reinterpret_cast<f32x4 *>(p.out + (size_t)m * p.Cout + co) = v;
    }
}

// torch's (cout, cin, k, k) fp32 weights, times *sw, -> the split fragment layout.  plain: rows = cout, K index (tap, cin).  flip: rows = cin,
// K index (tap', cout) with tap' the 180-degree rotated tap (launch_pack_conv_weights' two matrices).  Rows past `rows` are zeros.  A thread owns the
// 8 consecutive K values of one row that make one 16-byte piece of a fragment (the column count is a multiple of 32: they share a tap).
__global__ __launch_bounds__(256) void split16_scaled_pack_kernel(const float *__restrict__ w, u16 *__restrict__ out, const float *sw, int cout, int cin, int k,
                                                                  int rows_pad, int flip) {
    const int rows = flip ? cin : cout, cols = flip ? cout : cin, kk = k * k, K = kk * cols;
    const float s = *sw;
    const long long total = (long long)rows_pad * (K / 8);
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int row = (int)(idx / (K / 8)), k8 = (int)(idx % (K / 8));
        const int tap = (k8 * 8) / cols, c0 = (k8 * 8) % cols, t = flip ? kk - 1 - tap : tap;
        const size_t base = (((size_t)(row >> 4) * (K / 32) + (k8 >> 2)) * 2) * 512 + (size_t)((k8 & 3) * 16 + (row & 15)) * 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int co = flip ? c0 + e : row, ci = flip ? row : c0 + e;
            v[e] = row < rows ? w[((size_t)co * cin + ci) * kk + t] * s : 0.f;
        }
        unsigned hi[4], lo[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hi[e] = pack2_h<true>(v[2 * e], v[2 * e + 1]);
            const pk_f16x2 q = __builtin_bit_cast(pk_f16x2, hi[e]);
            lo[e] = pack2_h<true>((v[2 * e] - (float)q[0]) * 2048.f, (v[2 * e + 1] - (float)q[1]) * 2048.f);
        }
        *reinterpret_cast<uint4 *>(out + base) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        *reinterpret_cast<uint4 *>(out + base + 512) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
}

namespace {

struct FrozenBn {                                // the BNF instance's epilogue operands
    const float *gamma, *beta, *run_mean, *run_var;
    int relu;
};

// conv_split16's tiles: 128 couts where the padded rows allow it, 128 pixels where that still fills the chip
template <bool BNF>
void launch_tiles(ConvSS &p, int cout_pad, int64_t M, int cus, hipStream_t stream) {
    if (cout_pad % 128 == 0) {
        p.n_ctiles = cout_pad / 128;
        const int64_t t128 = ((M + 127) / 128) * p.n_ctiles;
        if (t128 >= cus) hipLaunchKernelGGL((conv_split16_scaled_kernel<128, 128, BNF>), dim3((unsigned)t128), dim3(512), 0, stream, p);
        else hipLaunchKernelGGL((conv_split16_scaled_kernel<64, 128, BNF>), dim3((unsigned)(((M + 63) / 64) * p.n_ctiles)), dim3(512), 0, stream, p);
    } else {
        p.n_ctiles = cout_pad / 64;
        const int64_t t128 = ((M + 127) / 128) * p.n_ctiles;
        if (t128 >= cus) hipLaunchKernelGGL((conv_split16_scaled_kernel<128, 64, BNF>), dim3((unsigned)t128), dim3(512), 0, stream, p);
        else hipLaunchKernelGGL((conv_split16_scaled_kernel<64, 64, BNF>), dim3((unsigned)(((M + 63) / 64) * p.n_ctiles)), dim3(512), 0, stream, p);
    }
}

// x (n, h, w, cin) * packed rows (cout) -> out (n, ho, wo, cout) [+ res]; the shapes have passed the callers' checks.  bn: the frozen BatchNorm of the
// BNF instance (res is then the residual behind it), null for the plain convolution
pvr_status launch_kernel(const float *in, const void *wsp, const float *res, float *out, int n, int h, int w, int cin, int cout, int k, int stride, int pad,
                         const float *sx, const float *sw, hipStream_t stream, const FrozenBn *bn = nullptr) {
    ConvSS p;
    p.in = in; p.res = res; p.sx = sx; p.sw = sw; p.w = (const u16 *)wsp; p.out = out;
    p.gamma = p.beta = p.run_mean = p.run_var = nullptr; p.relu = 0;
    if (bn) { p.gamma = bn->gamma; p.beta = bn->beta; p.run_mean = bn->run_mean; p.run_var = bn->run_var; p.relu = bn->relu; }
    p.N = n; p.H = h; p.W = w; p.Cin = cin; p.Cout = cout; p.KH = k; p.KW = k; p.stride = stride; p.pad = pad;
    p.Ho = (h + 2 * pad - k) / stride + 1; p.Wo = (w + 2 * pad - k) / stride + 1;
    const int cout_pad = (cout + 63) / 64 * 64;
    const int64_t M = (int64_t)n * p.Ho * p.Wo, inb = (int64_t)n * h * w * cin * 4, wb = (int64_t)cout_pad * k * k * cin * 4;
    PVR_REQUIRE(M < (1ll << 31) && inb < 0x7ffffff0ll && wb < 0x7ffffff0ll, "conv_split16_scaled: operand larger than 2 GiB (use a smaller batch)");
    p.M = (int)M; p.in_bytes = (unsigned)inb; p.w_bytes = (unsigned)wb; p.nsteps = k * k * cin / 32;
    static const int cus = [] { int v = 0, dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev); return v > 0 ? v : 256; }();
    if (bn) launch_tiles<true>(p, cout_pad, M, cus, stream);
    else launch_tiles<false>(p, cout_pad, M, cus, stream);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status fwd_check(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "conv_fwd_split16: empty input");
    PVR_REQUIRE(k >= 1 && k <= 3 && (stride == 1 || stride == 2) && pad >= 0 && pad < k, "conv_fwd_split16: k %d stride %d pad %d (k 1..3, stride 1 or 2, pad < k)", k,
                stride, pad);
    PVR_REQUIRE(cin % 32 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "conv_fwd_split16: cin %d must be a multiple of 32 (a K step is 32 channels of one tap) and "
                "cout %d of 4", cin, cout);
    PVR_REQUIRE(h + 2 * pad >= k && w + 2 * pad >= k, "conv_fwd_split16: the %d x %d input is smaller than the filter", h, w);
    return PVR_OK;
}

pvr_status dgrad_check(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "conv_dgrad_split16: empty input");
    PVR_REQUIRE((k == 3 && pad == 1) || (k == 1 && pad == 0), "conv_dgrad_split16: (k, pad) = (%d, %d); built for (3, 1) and (1, 0)", k, pad);
    PVR_REQUIRE(stride == 1 || stride == 2, "conv_dgrad_split16: stride %d (1 or 2)", stride);
    PVR_REQUIRE(stride == 1 || (h % 2 == 0 && w % 2 == 0), "conv_dgrad_split16: a stride-2 convolution of an odd %d x %d input is not built (the zero-filled grid is "
                "exact for even sizes)", h, w);
    PVR_REQUIRE(cout % 32 == 0 && cin % 4 == 0 && cin > 0 && cout > 0, "conv_dgrad_split16: cout %d must be a multiple of 32 (a K step is 32 channels of one tap) and "
                "cin %d of 4", cout, cin);
    return PVR_OK;
}

int pack_blocks(long long work) {
    const long long b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

}  // namespace

pvr_status launch_split16_scaled_pack(const float *w, void *out, int cout, int cin, int k, bool flip, const float *sw, hipStream_t st) {
    const int rows_pad = ((flip ? cin : cout) + 63) / 64 * 64, K = k * k * (flip ? cout : cin);
    PVR_REQUIRE(K % 32 == 0, "split16_scaled_pack: the K dimension %d must be a multiple of 32", K);
    hipLaunchKernelGGL(split16_scaled_pack_kernel, dim3(pack_blocks((long long)rows_pad * (K / 8))), dim3(256), 0, st, w, (u16 *)out, sw, cout, cin, k, rows_pad,
                       flip ? 1 : 0);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status launch_conv_fwd_split16(const float *x, const float *w, float *z, int n, int h, int wd, int cin, int cout, int k, int stride, int pad, const float *sx,
                                   const float *sw, float *wpack, hipStream_t st) {
    pvr_status s;
    if ((s = fwd_check(n, h, wd, cin, cout, k, stride, pad))) return s;
    if ((s = launch_split16_scaled_pack(w, wpack, cout, cin, k, false, sw, st))) return s;
    return launch_kernel(x, wpack, nullptr, z, n, h, wd, cin, cout, k, stride, pad, sx, sw, st);
}

pvr_status launch_conv_bn_frozen_split16(const float *x, const float *w, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                         const float *res, float *y, int n, int h, int wd, int cin, int cout, int k, int stride, int pad, int relu, const float *sx,
                                         const float *sw, float *wpack, hipStream_t st) {
    pvr_status s;
    if ((s = fwd_check(n, h, wd, cin, cout, k, stride, pad))) return s;
    if ((s = launch_split16_scaled_pack(w, wpack, cout, cin, k, false, sw, st))) return s;
    const FrozenBn bn{gamma, beta, run_mean, run_var, relu ? 1 : 0};
    return launch_kernel(x, wpack, res, y, n, h, wd, cin, cout, k, stride, pad, sx, sw, st, &bn);
}

pvr_status launch_conv_dgrad_split16(const float *dz, const float *w, float *dx, int accumulate, int n, int h, int wd, int cin, int cout, int k, int stride, int pad,
                                     const float *sdz, const float *sw, float *wflip, float *dil, hipStream_t st) {
    pvr_status s;
    if ((s = dgrad_check(n, h, wd, cin, cout, k, stride, pad))) return s;
    if ((s = launch_split16_scaled_pack(w, wflip, cout, cin, k, true, sw, st))) return s;
    const float *src = dz;
    int hs = (h + 2 * pad - k) / stride + 1, ws = (wd + 2 * pad - k) / stride + 1;
    if (stride == 2) {
        if ((s = launch_dilate2(dz, dil, n, h, wd, cout, st))) return s;
        src = dil; hs = h; ws = wd;
    }
    return launch_kernel(src, wflip, accumulate ? dx : nullptr, dx, n, hs, ws, cout, cin, k, 1, k - 1 - pad, sdz, sw, st);
}

}  // namespace pvr

using namespace pvr;

extern "C" {

int64_t pvr_op_conv_fwd_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (fwd_check(n, h, w, cin, cout, k, stride, pad)) return 0;
    return (int64_t)((cout + 63) / 64 * 64) * k * k * cin;                         // the split weights: two f16 per value
}

pvr_status pvr_op_conv_fwd_split16(const float *x, const float *wt, float *z, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride,
                                   int32_t pad, const float *x_scale, const float *w_scale, float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(x && wt && z && scratch, "pvr_op_conv_fwd_split16: null argument");
    PVR_REQUIRE(x_scale && w_scale, "pvr_op_conv_fwd_split16: null scale (pvr_op_absmax_scale writes one per operand)");
    pvr_status s;
    if ((s = fwd_check(n, h, w, cin, cout, k, stride, pad))) return s;
    const int64_t need = pvr_op_conv_fwd_split16_scratch_floats(n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_fwd_split16: scratch of %lld floats, pvr_op_conv_fwd_split16_scratch_floats asks for %lld",
                (long long)scratch_floats, (long long)need);
    return launch_conv_fwd_split16(x, wt, z, n, h, w, cin, cout, k, stride, pad, x_scale, w_scale, scratch, (hipStream_t)stream);
}

int64_t pvr_op_conv_bn_frozen_forward_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    return pvr_op_conv_fwd_split16_scratch_floats(n, h, w, cin, cout, k, stride, pad);
}

pvr_status pvr_op_conv_bn_frozen_forward_split16(const float *x, const float *wt, const float *gamma, const float *beta, const float *run_mean,
                                                 const float *run_var, const float *res, float *y, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                                 int32_t k, int32_t stride, int32_t pad, int32_t relu, const float *x_scale, const float *w_scale, float *scratch,
                                                 int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(x && wt && gamma && beta && run_mean && run_var && y && scratch, "pvr_op_conv_bn_frozen_forward_split16: null argument");
    PVR_REQUIRE(x_scale && w_scale, "pvr_op_conv_bn_frozen_forward_split16: null scale (pvr_op_absmax_scale writes one per operand)");
    pvr_status s;
    if ((s = fwd_check(n, h, w, cin, cout, k, stride, pad))) return s;
    const int64_t need = pvr_op_conv_fwd_split16_scratch_floats(n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_bn_frozen_forward_split16: scratch of %lld floats, pvr_op_conv_bn_frozen_forward_split16_scratch_floats asks "
                "for %lld", (long long)scratch_floats, (long long)need);
    return launch_conv_bn_frozen_split16(x, wt, gamma, beta, run_mean, run_var, res, y, n, h, w, cin, cout, k, stride, pad, relu, x_scale, w_scale, scratch,
                                         (hipStream_t)stream);
}

// scratch: [rotated split weights (cin_pad, k*k*cout)] [dz on the zero-filled grid (stride 2)]
int64_t pvr_op_conv_dgrad_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (dgrad_check(n, h, w, cin, cout, k, stride, pad)) return 0;
    const int64_t cin_pad = (cin + 63) / 64 * 64;
    return cin_pad * k * k * cout + (stride == 2 ? (int64_t)n * h * w * cout : 0);
}

pvr_status pvr_op_conv_dgrad_split16(const float *dz, const float *wt, float *dx, int32_t accumulate, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout,
                                     int32_t k, int32_t stride, int32_t pad, const float *dz_scale, const float *w_scale, float *scratch, int64_t scratch_floats,
                                     void *stream) {
    PVR_REQUIRE(dz && wt && dx && scratch, "pvr_op_conv_dgrad_split16: null argument");
    PVR_REQUIRE(dz_scale && w_scale, "pvr_op_conv_dgrad_split16: null scale (pvr_op_absmax_scale writes one per operand)");
    pvr_status s;
    if ((s = dgrad_check(n, h, w, cin, cout, k, stride, pad))) return s;
    const int64_t need = pvr_op_conv_dgrad_split16_scratch_floats(n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_dgrad_split16: scratch of %lld floats, pvr_op_conv_dgrad_split16_scratch_floats asks for %lld",
                (long long)scratch_floats, (long long)need);
    const int64_t cin_pad = (cin + 63) / 64 * 64;
    return launch_conv_dgrad_split16(dz, wt, dx, accumulate, n, h, w, cin, cout, k, stride, pad, dz_scale, w_scale, scratch, scratch + cin_pad * k * k * cout,
                                     (hipStream_t)stream);
}

}  // extern "C"
