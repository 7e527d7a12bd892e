// Device code of the trainable encoder's backward pass and of its training-mode BatchNorm (include/pvr_train.h; the executor is encoder_train.hip):
// BatchNorm on batch statistics and its backward, the weight gradient on the f32-input MFMA, the data gradient through conv_f32.hip, conv1's weight
// gradient, max-pool and average-pool backward.  fp32 NHWC throughout.  No float atomics: every reduction that is split over workgroups writes partials
// that a second kernel sums in a fixed order, so results are bit-reproducible run to run.
#include "common.h"
#include "train_internal.h"
#include "../../include/pvr_train.h"

namespace pvr {

pvr_status launch_conv_f32(const float *, const float *, const float *, const float *, float *, int, int, int, int, int, int, int, int, int, hipStream_t);

// ------------------------------------------------------------------------------------------------------------------------------------------------
// BatchNorm2d, training mode.  Statistics per channel over `rows` rows of NHWC: a block is 32 channels x 8 row lanes over BN_CHUNK rows, so a thread's
// fp32 chain is at most 256 terms; the lanes are summed as a tree, the blocks' partials in double by bn_finalize_kernel.
// MODE 0: sum z   1: sum (z - mean)^2 (two-pass variance: no E[x^2] - E[x]^2 cancellation)   2: sum g and sum g * xhat, g = dy masked by y > 0
// ------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int BN_CH = 32, BN_RL = 8, BN_CHUNK = 2048;
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;

struct BnRed {
    const float *z, *y, *dy, *mean, *rstd;
    float *part;                                  // [split][2][C]
    int64_t rows;
    int C, relu;
};

template <int MODE>
__global__ __launch_bounds__(256) void bn_reduce_kernel(BnRed p) {
    __shared__ float sm[2][BN_RL][BN_CH];
    const int cl = threadIdx.x & (BN_CH - 1), rl = threadIdx.x >> 5;
    const int c = blockIdx.x * BN_CH + cl;
    const int64_t r0 = (int64_t)blockIdx.y * BN_CHUNK, r1 = min(r0 + BN_CHUNK, p.rows);
    float s0 = 0.f, s1 = 0.f;
    if (c < p.C) {
        const float m = MODE >= 1 ? p.mean[c] : 0.f, rs = MODE == 2 ? p.rstd[c] : 0.f;
        for (int64_t r = r0 + rl; r < r1; r += BN_RL) {
            const size_t i = (size_t)r * p.C + c;
            if constexpr (MODE == 0) s0 += p.z[i];
            else if constexpr (MODE == 1) { const float d = p.z[i] - m; s0 += d * d; }
            else {
                float g = p.dy[i];
                if (p.relu && !(p.y[i] > 0.f)) g = 0.f;
                s0 += g;
                s1 += g * ((p.z[i] - m) * rs);
            }
        }
    }
    sm[0][rl][cl] = s0; sm[1][rl][cl] = s1;
    __syncthreads();
    if (rl < 2 && c < p.C) {
        const float (*a)[BN_CH] = sm[rl];
        const float v = ((a[0][cl] + a[1][cl]) + (a[2][cl] + a[3][cl])) + ((a[4][cl] + a[5][cl]) + (a[6][cl] + a[7][cl]));
        p.part[((size_t)blockIdx.y * 2 + rl) * p.C + c] = v;
    }
}

struct BnFin {
    const float *part;
    int nsplit, C;
    int64_t rows;
    float *mean, *rstd, *run_mean, *run_var, *sums, *dgamma, *dbeta;
    long long *nbt;
};

template <int MODE>
__global__ __launch_bounds__(256) void bn_finalize_kernel(BnFin p) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    double a0 = 0.0, a1 = 0.0;
    for (int s = 0; s < p.nsplit; ++s) {
        a0 += (double)p.part[((size_t)s * 2) * p.C + c];
        if (MODE == 2) a1 += (double)p.part[((size_t)s * 2 + 1) * p.C + c];
    }
    if constexpr (MODE == 0) {
        p.mean[c] = (float)(a0 / (double)p.rows);
    } else if constexpr (MODE == 1) {
        const double var = a0 / (double)p.rows;
        p.rstd[c] = (float)(1.0 / sqrt(var + (double)BN_EPS));
        if (p.run_mean) {
            p.run_mean[c] = (1.f - BN_MOMENTUM) * p.run_mean[c] + BN_MOMENTUM * p.mean[c];
            p.run_var[c] = (1.f - BN_MOMENTUM) * p.run_var[c] + BN_MOMENTUM * (float)(a0 / (double)(p.rows - 1));      // unbiased
            if (c == 0) *p.nbt += 1;
        }
    } else {
        p.sums[c] = (float)a0; p.sums[p.C + c] = (float)a1;
        p.dbeta[c] = (float)a0; p.dgamma[c] = (float)a1;
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ z, const float *res, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ rstd, float *y, size_t total4, int C, int relu) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % (size_t)C);
        const f32x4 v = *reinterpret_cast<const f32x4 *>(z + i * 4);
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f}, o;
        if (res) r = *reinterpret_cast<const f32x4 *>(res + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = (v[e] - mean[c + e]) * rstd[c + e] * gamma[c + e] + beta[c + e];
            if (res) t += r[e];
            o[e] = relu ? fmaxf(t, 0.f) : t;
        }
        *reinterpret_cast<f32x4 *>(y + i * 4) = o;
    }
}

__global__ __launch_bounds__(256) void bn_backward_apply_kernel(const float *__restrict__ z, const float *__restrict__ y, const float *__restrict__ dy,
                                                                const float *__restrict__ gamma, const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                const float *__restrict__ sums, float *dz, float *dres, int accumulate, size_t total4, int C,
                                                                int relu, float inv_rows) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % (size_t)C);
        const f32x4 zv = *reinterpret_cast<const f32x4 *>(z + i * 4), gv = *reinterpret_cast<const f32x4 *>(dy + i * 4);
        f32x4 yv = f32x4{1.f, 1.f, 1.f, 1.f}, rv = f32x4{0.f, 0.f, 0.f, 0.f}, o, g;
        if (relu) yv = *reinterpret_cast<const f32x4 *>(y + i * 4);
        if (dres && accumulate) rv = *reinterpret_cast<const f32x4 *>(dres + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            g[e] = yv[e] > 0.f ? gv[e] : 0.f;
            const float xh = (zv[e] - mean[c + e]) * rstd[c + e];
            o[e] = gamma[c + e] * rstd[c + e] * (g[e] - sums[c + e] * inv_rows - xh * (sums[C + c + e] * inv_rows));
            rv[e] += g[e];
        }
        *reinterpret_cast<f32x4 *>(dz + i * 4) = o;
        if (dres) *reinterpret_cast<f32x4 *>(dres + i * 4) = rv;
    }
}

static int ew_blocks(size_t work) {
    size_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : b > 256 * 32 ? 256 * 32 : b);
}
static int bn_splits(int64_t rows) { return (int)((rows + BN_CHUNK - 1) / BN_CHUNK); }

// ------------------------------------------------------------------------------------------------------------------------------------------------
// BatchNorm2d in training mode on its RUNNING statistics (model.train() with every BatchNorm in eval(): the fine-tuning mode of a pre-trained trunk).
// Every row is independent of the others, so a step over N frames is a sum over chunks of frames.
// Forward: one pass over z, no reduction, no scratch; the mean / rstd slots the backward reads receive the running mean and 1 / sqrt(running_var + eps)
// (the same fp32 expression a thread evaluates for itself); the running buffers are read only.  FIXED: the grid stride is a multiple of the channel
// groups of a row, so a thread's four channels - and their scale and shift - are the same in every iteration.
// Backward: dz = gamma * rstd * g has no mean terms, so ONE kernel streams z, y, dy -> dz [, dres] and reduces sum g and sum g * xhat on the way: a block
// is 64 channels (16 threads of 4) x 16 row lanes over BN_CHUNK rows - a thread's fp32 chain is at most 128 terms, the lanes are summed as a 4-step tree
// (fewer roundings than bn_reduce_kernel's 256 + 3) - and writes partials in bn_reduce_kernel<2>'s layout, which bn_finalize_kernel<2> sums in double.
// ------------------------------------------------------------------------------------------------------------------------------------------------
template <bool FIXED>
__global__ __launch_bounds__(256) void bn_frozen_apply_kernel(const float *__restrict__ z, const float *res, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, const float *__restrict__ run_mean,
                                                              const float *__restrict__ run_var, float *y, float *mean_out, float *rstd_out, size_t total4, int C,
                                                              int relu) {
    if (blockIdx.x == 0 && mean_out)
        for (int c = threadIdx.x; c < C; c += 256) {
            mean_out[c] = run_mean[c];
            rstd_out[c] = 1.f / sqrtf(run_var[c] + BN_EPS);
        }
    const size_t c4n = (size_t)(C / 4);
    float m[4], rs[4], ga[4], be[4];
    auto load = [&](int c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m[e] = run_mean[c + e]; rs[e] = 1.f / sqrtf(run_var[c + e] + BN_EPS);
            ga[e] = gamma[c + e]; be[e] = beta[c + e];
        }
    };
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (FIXED && first < total4) load((int)(first % c4n) * 4);
    for (size_t i = first; i < total4; i += (size_t)gridDim.x * 256) {
        if (!FIXED) load((int)(i % c4n) * 4);
        const f32x4 v = *reinterpret_cast<const f32x4 *>(z + i * 4);
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f}, o;
        if (res) r = *reinterpret_cast<const f32x4 *>(res + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = (v[e] - m[e]) * rs[e] * ga[e] + be[e];
            if (res) t += r[e];
            o[e] = relu ? fmaxf(t, 0.f) : t;
        }
        *reinterpret_cast<f32x4 *>(y + i * 4) = o;
    }
}

constexpr int BF_C4 = 16, BF_RL = 16;             // 16 threads of 4 channels x 16 row lanes
struct BnFrozenBwd {
    const float *z, *y, *dy, *gamma, *mean, *rstd;
    float *dz, *dres, *part;                      // part: [split][2][C]
    int64_t rows;
    int C, relu, accumulate;
};

__global__ __launch_bounds__(256) void bn_frozen_backward_kernel(BnFrozenBwd p) {
    __shared__ f32x4 sm[2][BF_RL][BF_C4];
    const int cl = threadIdx.x & (BF_C4 - 1), rl = threadIdx.x >> 4;
    const int c = (blockIdx.x * BF_C4 + cl) * 4;
    const int64_t r0 = (int64_t)blockIdx.y * BN_CHUNK, r1 = min(r0 + BN_CHUNK, p.rows);
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (c < p.C) {                                // (C % 4 == 0: channels c .. c + 3 exist together)
        float m[4], rs[4], k[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { m[e] = p.mean[c + e]; rs[e] = p.rstd[c + e]; k[e] = p.gamma[c + e] * rs[e]; }
#pragma unroll 2
        for (int64_t r = r0 + rl; r < r1; r += BF_RL) {
            const size_t i = (size_t)r * p.C + c;
            const f32x4 zv = *reinterpret_cast<const f32x4 *>(p.z + i), gv = *reinterpret_cast<const f32x4 *>(p.dy + i);
            f32x4 yv = f32x4{1.f, 1.f, 1.f, 1.f}, rv = f32x4{0.f, 0.f, 0.f, 0.f}, o;
            if (p.relu) yv = *reinterpret_cast<const f32x4 *>(p.y + i);
            if (p.dres && p.accumulate) rv = *reinterpret_cast<const f32x4 *>(p.dres + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = yv[e] > 0.f ? gv[e] : 0.f;
                s0[e] += g;
                s1[e] += g * ((zv[e] - m[e]) * rs[e]);
                o[e] = k[e] * g;
                rv[e] += g;
            }
            *reinterpret_cast<f32x4 *>(p.dz + i) = o;
            if (p.dres) *reinterpret_cast<f32x4 *>(p.dres + i) = rv;
        }
    }
    sm[0][rl][cl] = s0; sm[1][rl][cl] = s1;
    __syncthreads();
    if (rl < 2 && c < p.C) {
        const f32x4 (*a)[BF_C4] = sm[rl];
        const f32x4 v = (((a[0][cl] + a[1][cl]) + (a[2][cl] + a[3][cl])) + ((a[4][cl] + a[5][cl]) + (a[6][cl] + a[7][cl]))) +
                        (((a[8][cl] + a[9][cl]) + (a[10][cl] + a[11][cl])) + ((a[12][cl] + a[13][cl]) + (a[14][cl] + a[15][cl])));
        float *out = p.part + ((size_t)blockIdx.y * 2 + rl) * p.C + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = v[e];
    }
}

// grads += pass: one fp32 addition per element (the gradient accumulation of pvr_trainer_backward_acc)
__global__ __launch_bounds__(256) void grad_add_kernel(float *__restrict__ g, const float *__restrict__ s, size_t n) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(g + i * 4), b = *reinterpret_cast<const f32x4 *>(s + i * 4);
        *reinterpret_cast<f32x4 *>(g + i * 4) = a + b;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[n4 * 4 + threadIdx.x] += s[n4 * 4 + threadIdx.x];
}

static pvr_status bn_frozen_check(const char *what, int64_t rows, int c) {
    PVR_REQUIRE(rows >= 1 && c > 0 && c % 4 == 0, "%s: %lld rows of %d channels (rows >= 1 and c %% 4 == 0)", what, (long long)rows, c);
    PVR_REQUIRE(rows * c < (1ll << 40) && rows / BN_CHUNK < 65535, "%s: %lld rows are more than one launch takes", what, (long long)rows);
    return PVR_OK;
}
// pvr_op_bn_frozen_forward's launch; mean_out / rstd_out may both be null (the frozen prefix of pvr_trainer_set_train_from keeps nothing for a backward)
pvr_status launch_bn_frozen_apply(const float *z, const float *res, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                  float *y, float *mean_out, float *rstd_out, int64_t rows, int c, int relu, hipStream_t stream) {
    pvr_status s;
    if ((s = bn_frozen_check("pvr_op_bn_frozen_forward", rows, c))) return s;
    const size_t total4 = (size_t)rows * c / 4;
    // a grid whose stride (blocks * 256 float4s) is a multiple of the c / 4 channel groups of a row keeps a thread on the same four channels
    int blocks = ew_blocks(total4);
    int per = c / 4, a = per, b = 256;
    while (b) { const int t = a % b; a = b; b = t; }
    per /= a;                                     // blocks must be a multiple of (c / 4) / gcd(c / 4, 256)
    const bool fixed = blocks >= per;
    if (fixed) blocks -= blocks % per;
    if (fixed)
        hipLaunchKernelGGL(bn_frozen_apply_kernel<true>, dim3(blocks), dim3(256), 0, stream, z, res, gamma, beta, run_mean, run_var, y, mean_out,
                           rstd_out, total4, c, relu);
    else
        hipLaunchKernelGGL(bn_frozen_apply_kernel<false>, dim3(blocks), dim3(256), 0, stream, z, res, gamma, beta, run_mean, run_var, y, mean_out,
                           rstd_out, total4, c, relu);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status launch_grad_add(float *grads, const float *pass, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(grad_add_kernel, dim3(ew_blocks((size_t)(n + 3) / 4)), dim3(256), 0, st, grads, pass, (size_t)n);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// weight layouts
// ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_conv_weights_kernel(const float *__restrict__ w, float *__restrict__ out, int cout, int cin, int k, int rows_pad, int flip) {
    // plain: rows = cout, columns (tap, cin);  flip: rows = cin, columns (tap', cout) with tap' the 180-degree rotated tap
    const int rows = flip ? cin : cout, cols_c = flip ? cout : cin, kk = k * k;
    const size_t total = (size_t)rows_pad * kk * cols_c;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int cc = (int)(i % cols_c), tap = (int)((i / cols_c) % kk), r = (int)(i / ((size_t)cols_c * kk));
        float v = 0.f;
        if (r < rows) {
            const int co = flip ? cc : r, ci = flip ? r : cc, t = flip ? kk - 1 - tap : tap;
            v = w[((size_t)co * cin + ci) * kk + t];
        }
        out[i] = v;
    }
}
__global__ __launch_bounds__(256) void pack_stem_weights_kernel(const float *__restrict__ w, float *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;       // [64][49][4]
    if (i >= 64 * 49 * 4) return;
    const int c = i & 3, tap = (i >> 2) % 49, co = i / (49 * 4);
    out[i] = c < 3 ? w[(co * 3 + c) * 49 + tap] : 0.f;
}

pvr_status launch_pack_conv_weights(const float *w, float *out, int cout, int cin, int k, bool flip, hipStream_t st) {
    const int rows_pad = ((flip ? cin : cout) + 63) / 64 * 64;
    const size_t total = (size_t)rows_pad * k * k * (flip ? cout : cin);
    hipLaunchKernelGGL(pack_conv_weights_kernel, dim3(ew_blocks(total)), dim3(256), 0, st, w, out, cout, cin, k, rows_pad, flip ? 1 : 0);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}
pvr_status launch_pack_stem_weights(const float *w, float *out, hipStream_t st) {
    hipLaunchKernelGGL(pack_stem_weights_kernel, dim3(49), dim3(256), 0, st, w, out);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// Weight gradient on the f32-input MFMA: per filter tap a GEMM dW[co][ci] = sum over pixels m of dz[m][co] * x[pix(m, tap)][ci] whose reduction
// dimension is the pixels.  A workgroup owns a 64 (co) x 64 (ci) tile of one tap and one range of `chunk` pixels; 2 x 2 waves of 32 x 32, 32 pixels
// per step through LDS (pixel-major rows of 64 channels, as they lie in memory).  k-step ks of every slice feeds accumulator set ks & 3 (as
// conv_f32_kernel<8>: a single fma chain over 25 000 pixels is the inaccurate form); the sets are summed pairwise, the workgroups' partials by
// wgrad_reduce_kernel in split order, in double, into torch's (cout, cin, k, k) layout.
// ------------------------------------------------------------------------------------------------------------------------------------------------
struct WGrad {
    const float *x, *dz;
    float *part;                                  // [split][cout][tap][cin]
    int N, H, W, Cin, Ho, Wo, Cout, K, stride, pad, M, chunk, ci_tiles, co_tiles;
};

__device__ __forceinline__ f32x4 mfma_f32_16x16x4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(256) void conv_wgrad_kernel(WGrad p) {
    constexpr int BP = 32, LD = 80, SETS = 4;     // LD: rows fq .. fq + 3 of a k-step start 16 banks apart
    __shared__ __attribute__((aligned(16))) float sA[BP * LD], sB[BP * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4, wm = wave >> 1, wn = wave & 1;
    int b = blockIdx.x;
    const int cit = b % p.ci_tiles; b /= p.ci_tiles;
    const int cot = b % p.co_tiles, tap = b / p.co_tiles;
    const int kh = tap / p.K, kw = tap % p.K;
    const int m_begin = blockIdx.y * p.chunk, m_end = min(m_begin + p.chunk, p.M);
    f32x4 acc[SETS][2][2];
#pragma unroll
    for (int t = 0; t < SETS; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = m_begin; m0 < m_end; m0 += BP) {
        f32x4 ra[2], rb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, pr = idx >> 4, c4 = (idx & 15) * 4, m = m0 + pr;
            ra[i] = rb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, n = t / p.Ho;
                const int co = cot * 64 + c4, ci = cit * 64 + c4;
                if (co < p.Cout) ra[i] = *reinterpret_cast<const f32x4 *>(p.dz + (size_t)m * p.Cout + co);
                const int hi = ho * p.stride + kh - p.pad, wi = wo * p.stride + kw - p.pad;
                if (ci < p.Cin && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
                    rb[i] = *reinterpret_cast<const f32x4 *>(p.x + (((size_t)n * p.H + hi) * p.W + wi) * p.Cin + ci);
            }
        }
        __syncthreads();                           // the previous step's reads of sA / sB are done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + 256 * i, pr = idx >> 4, c4 = (idx & 15) * 4;
            *reinterpret_cast<f32x4 *>(&sA[pr * LD + c4]) = ra[i];
            *reinterpret_cast<f32x4 *>(&sB[pr * LD + c4]) = rb[i];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < BP / 4; ++ks) {
            const int k = ks * 4 + fq;
            float a[2], bb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sA[k * LD + wm * 32 + i * 16 + fr];
#pragma unroll
            for (int j = 0; j < 2; ++j) bb[j] = sB[k * LD + wn * 32 + j * 16 + fr];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[ks & 3][i][j] = mfma_f32_16x16x4(a[i], bb[j], acc[ks & 3][i][j]);
        }
    }
    // D: row = co (4 * fq + r), column = ci (fr)
    const int taps = p.K * p.K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 v = (acc[0][i][j] + acc[1][i][j]) + (acc[2][i][j] + acc[3][i][j]);
            const int ci = cit * 64 + wn * 32 + j * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = cot * 64 + wm * 32 + i * 16 + fq * 4 + r;
                if (co < p.Cout && ci < p.Cin) p.part[(((size_t)blockIdx.y * p.Cout + co) * taps + tap) * p.Cin + ci] = v[r];
            }
        }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, int nsplit, int cout, int taps, int cin) {
    const size_t per = (size_t)cout * taps * cin;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        double a = 0.0;
        for (int s = 0; s < nsplit; ++s) a += (double)part[(size_t)s * per + i];
        const int ci = (int)(i % cin), tap = (int)((i / cin) % taps), co = (int)(i / ((size_t)cin * taps));
        dw[((size_t)co * cin + ci) * taps + tap] = (float)a;
    }
}

struct WGradPlan { int M, ho, wo, ci_tiles, co_tiles, chunk, nsplit; };
static WGradPlan wgrad_plan(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    WGradPlan g;
    g.ho = (h + 2 * pad - k) / stride + 1; g.wo = (w + 2 * pad - k) / stride + 1;
    g.M = n * g.ho * g.wo;
    g.ci_tiles = (cin + 63) / 64; g.co_tiles = (cout + 63) / 64;
    const int tiles = g.ci_tiles * g.co_tiles * k * k;
    // about 1024 workgroups per launch, a pixel range of at least 64: the deep layers (many tiles, few pixels) are not split at all
    int want = std::max(1, std::min(1024 / tiles, (g.M + 63) / 64));
    g.chunk = ((g.M + want - 1) / want + 31) / 32 * 32;
    g.nsplit = (g.M + g.chunk - 1) / g.chunk;
    return g;
}
static pvr_status wgrad_check(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "conv_wgrad: empty input");
    PVR_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad < k, "conv_wgrad: k %d stride %d pad %d (k 1 or 3, stride 1 or 2, pad < k)", k, stride, pad);
    PVR_REQUIRE(cin % 32 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "conv_wgrad: cin %d must be a multiple of 32 and cout %d of 4", cin, cout);
    PVR_REQUIRE(h + 2 * pad >= k && w + 2 * pad >= k, "conv_wgrad: the %d x %d input is smaller than the filter", h, w);
    PVR_REQUIRE((int64_t)n * h * w * std::max(cin, cout) < (1ll << 31), "conv_wgrad: operand of 2^31 elements or more (use a smaller batch)");
    return PVR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// data gradient: dz written to the even pixels of a zeroed (h, w) grid (stride 2), then launch_conv_f32 with the rotated, transposed weights
// ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dilate2_kernel(const float *__restrict__ dz, float *__restrict__ out, int n, int h, int w, int c) {
    const int c4n = c / 4, ho = h / 2, wo = w / 2;
    const size_t total = (size_t)n * h * w * c4n;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c4 = (int)(i % c4n);
        size_t r = i / c4n;
        const int x = (int)(r % w); r /= w;
        const int y = (int)(r % h), b = (int)(r / h);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!((x | y) & 1)) v = *reinterpret_cast<const f32x4 *>(dz + (((size_t)b * ho + (y >> 1)) * wo + (x >> 1)) * c + c4 * 4);
        *reinterpret_cast<f32x4 *>(out + i * 4) = v;
    }
}

// (the split-f16 data gradient's use of the same grid: conv_split16_scaled.hip)
pvr_status launch_dilate2(const float *dz, float *out, int n, int h, int w, int c, hipStream_t st) {
    hipLaunchKernelGGL(dilate2_kernel, dim3(ew_blocks((size_t)n * h * w * c / 4)), dim3(256), 0, st, dz, out, n, h, w, c);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

static pvr_status dgrad_check(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "conv_dgrad: empty input");
    PVR_REQUIRE((k == 3 && pad == 1) || (k == 1 && pad == 0), "conv_dgrad: (k, pad) = (%d, %d); built for (3, 1) and (1, 0)", k, pad);
    PVR_REQUIRE(stride == 1 || stride == 2, "conv_dgrad: stride %d (1 or 2)", stride);
    PVR_REQUIRE(stride == 1 || (h % 2 == 0 && w % 2 == 0), "conv_dgrad: a stride-2 convolution of an odd %d x %d input is not built (the zero-filled grid is exact for even sizes)", h, w);
    PVR_REQUIRE(cout % 32 == 0 && cin % 4 == 0 && cin > 0 && cout > 0, "conv_dgrad: cout %d must be a multiple of 32 and cin %d of 4", cout, cin);
    return PVR_OK;
}

pvr_status launch_conv_dgrad(const float *dz, const float *w, float *dx, int accumulate, int n, int h, int wd, int cin, int cout, int k, int stride, int pad,
                             float *wflip, float *dil, const float *zero_bias, hipStream_t st) {
    pvr_status s;
    if ((s = dgrad_check(n, h, wd, cin, cout, k, stride, pad))) return s;
    if ((s = launch_pack_conv_weights(w, wflip, cout, cin, k, true, st))) return s;
    const float *src = dz;
    int hs = (h + 2 * pad - k) / stride + 1, ws = (wd + 2 * pad - k) / stride + 1;
    if (stride == 2) {
        hipLaunchKernelGGL(dilate2_kernel, dim3(ew_blocks((size_t)n * h * wd * cout / 4)), dim3(256), 0, st, dz, dil, n, h, wd, cout);
        PVR_LAUNCH_CHECK();
        src = dil; hs = h; ws = wd;
    }
    return launch_conv_f32(src, wflip, zero_bias, accumulate ? dx : nullptr, dx, n, hs, ws, cout, cin, k, 1, k - 1 - pad, 0, st);
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// conv1's weight gradient (7x7 / 2, pad 3, the image as NHWC4): 0.24 GFLOP per frame, a plain VALU reduction.  A block is one tap and one range of
// STEM_CHUNK pixels, a thread one (cout, channel) with four interleaved chains; the partials are summed in split order, in double.
// ------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int STEM_CHUNK = 1024;
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float *__restrict__ img, const float *__restrict__ dz, float *__restrict__ part, int S, long long M) {
    const int co = threadIdx.x & 63, c = threadIdx.x >> 6;
    if (c == 3) return;                            // (the NHWC4 pad channel)
    const int tap = blockIdx.x, kh = tap / 7, kw = tap % 7, So = S / 2;
    const long long m_begin = (long long)blockIdx.y * STEM_CHUNK, m_end = min(m_begin + STEM_CHUNK, M);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long m0 = m_begin; m0 < m_end; m0 += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long m = m0 + q;
            if (m >= m_end) break;
            const int ox = (int)(m % So), oy = (int)((m / So) % So), b = (int)(m / ((long long)So * So));
            const int iy = 2 * oy + kh - 3, ix = 2 * ox + kw - 3;
            if ((unsigned)iy < (unsigned)S && (unsigned)ix < (unsigned)S) acc[q] += dz[(size_t)m * 64 + co] * img[(((size_t)b * S + iy) * S + ix) * 4 + c];
        }
    }
    part[((size_t)blockIdx.y * 64 + co) * 147 + c * 49 + tap] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, int nsplit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * 147) return;
    double a = 0.0;
    for (int s = 0; s < nsplit; ++s) a += (double)part[(size_t)s * (64 * 147) + i];
    dw[i] = (float)a;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// pools
// ------------------------------------------------------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) backward as a gather: an input pixel receives dy of each of the <= 4 windows that cover it and whose FIRST maximum in scan
// order (torch: a later element wins only if it is greater) it is
__global__ __launch_bounds__(256) void maxpool_backward_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ dx, int n, int h, int w,
                                                               int c, int ho, int wo) {
    const size_t total = (size_t)n * h * w * c;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ch = (int)(i % c);
        size_t r = i / c;
        const int ix = (int)(r % w); r /= w;
        const int iy = (int)(r % h), b = (int)(r / h);
        const float *xb = x + (size_t)b * h * w * c + ch;
        float g = 0.f;
        for (int oy = iy / 2; oy <= min((iy + 1) / 2, ho - 1); ++oy)
            for (int ox = ix / 2; ox <= min((ix + 1) / 2, wo - 1); ++ox) {
                float best = -INFINITY;
                int by = -1, bx = -1;
                for (int dy_ = 0; dy_ < 3; ++dy_) {
                    const int yy = 2 * oy - 1 + dy_;
                    if (yy < 0 || yy >= h) continue;
                    for (int dx_ = 0; dx_ < 3; ++dx_) {
                        const int xx = 2 * ox - 1 + dx_;
                        if (xx < 0 || xx >= w) continue;
                        const float v = xb[((size_t)yy * w + xx) * c];
                        if (v > best || by < 0) { best = v; by = yy; bx = xx; }
                    }
                }
                if (by == iy && bx == ix) g += dy[(((size_t)b * ho + oy) * wo + ox) * c + ch];
            }
        dx[i] = g;
    }
}

__global__ __launch_bounds__(256) void avgpool_backward_kernel(const float *__restrict__ dout, int64_t stride, float *__restrict__ dx, int n, int hw, int c) {
    const size_t total = (size_t)n * hw * c;
    const float fhw = (float)hw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int ch = (int)(i % c), b = (int)(i / ((size_t)hw * c));
        dx[i] = dout[(size_t)b * stride + ch] / fhw;
    }
}

}  // namespace pvr

using namespace pvr;

extern "C" {

int64_t pvr_op_bn_scratch_floats(int64_t rows, int32_t c) { return rows > 0 && c > 0 ? ((int64_t)bn_splits(rows) + 1) * 2 * c : 0; }

static pvr_status bn_check(const char *what, int64_t rows, int c, float *scratch, int64_t scratch_floats) {
    PVR_REQUIRE(rows >= 2 && c > 0 && c % 4 == 0, "%s: %lld rows of %d channels (rows >= 2 - batch statistics need more than one value per channel - and c %% 4 == 0)",
                what, (long long)rows, c);
    PVR_REQUIRE(rows * c < (1ll << 40) && rows / BN_CHUNK < 65535, "%s: %lld rows are more than one launch takes", what, (long long)rows);
    PVR_REQUIRE(scratch && scratch_floats >= pvr_op_bn_scratch_floats(rows, c), "%s: scratch of %lld floats, pvr_op_bn_scratch_floats asks for %lld", what,
                (long long)scratch_floats, (long long)pvr_op_bn_scratch_floats(rows, c));
    return PVR_OK;
}

pvr_status pvr_op_bn_train_forward(const float *z, const float *res, const float *gamma, const float *beta, float *run_mean, float *run_var, int64_t *nbt,
                                   float *y, float *mean_out, float *rstd_out, int64_t rows, int32_t c, int32_t relu, float *scratch, int64_t scratch_floats,
                                   void *stream) {
    PVR_REQUIRE(z && gamma && beta && y && mean_out && rstd_out, "pvr_op_bn_train_forward: null argument");
    PVR_REQUIRE((run_mean && run_var && nbt) || (!run_mean && !run_var && !nbt), "pvr_op_bn_train_forward: running_mean, running_var and num_batches_tracked go together");
    pvr_status s;
    if ((s = bn_check("pvr_op_bn_train_forward", rows, c, scratch, scratch_floats))) return s;
    hipStream_t st = (hipStream_t)stream;
    const int nsplit = bn_splits(rows);
    const dim3 grid((c + BN_CH - 1) / BN_CH, nsplit);
    BnRed r{z, nullptr, nullptr, mean_out, rstd_out, scratch, rows, c, relu};
    BnFin f{scratch, nsplit, c, rows, mean_out, rstd_out, run_mean, run_var, nullptr, nullptr, nullptr, (long long *)nbt};
    hipLaunchKernelGGL(bn_reduce_kernel<0>, grid, dim3(256), 0, st, r);
    hipLaunchKernelGGL(bn_finalize_kernel<0>, dim3((c + 255) / 256), dim3(256), 0, st, f);
    hipLaunchKernelGGL(bn_reduce_kernel<1>, grid, dim3(256), 0, st, r);
    hipLaunchKernelGGL(bn_finalize_kernel<1>, dim3((c + 255) / 256), dim3(256), 0, st, f);
    const size_t total4 = (size_t)rows * c / 4;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_blocks(total4)), dim3(256), 0, st, z, res, gamma, beta, mean_out, rstd_out, y, total4, c, relu);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_bn_train_backward(const float *z, const float *y, const float *dy, const float *gamma, const float *mean, const float *rstd, float *dz,
                                    float *dres, int32_t dres_accumulate, float *dgamma, float *dbeta, int64_t rows, int32_t c, int32_t relu, float *scratch,
                                    int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(z && dy && gamma && mean && rstd && dz && dgamma && dbeta && (y || !relu), "pvr_op_bn_train_backward: null argument");
    pvr_status s;
    if ((s = bn_check("pvr_op_bn_train_backward", rows, c, scratch, scratch_floats))) return s;
    hipStream_t st = (hipStream_t)stream;
    const int nsplit = bn_splits(rows);
    float *sums = scratch + (size_t)nsplit * 2 * c;
    BnRed r{z, y, dy, mean, rstd, scratch, rows, c, relu};
    BnFin f{scratch, nsplit, c, rows, nullptr, nullptr, nullptr, nullptr, sums, dgamma, dbeta, nullptr};
    hipLaunchKernelGGL(bn_reduce_kernel<2>, dim3((c + BN_CH - 1) / BN_CH, nsplit), dim3(256), 0, st, r);
    hipLaunchKernelGGL(bn_finalize_kernel<2>, dim3((c + 255) / 256), dim3(256), 0, st, f);
    const size_t total4 = (size_t)rows * c / 4;
    hipLaunchKernelGGL(bn_backward_apply_kernel, dim3(ew_blocks(total4)), dim3(256), 0, st, z, y, dy, gamma, mean, rstd, sums, dz, dres, dres_accumulate, total4, c,
                       relu, 1.0f / (float)rows);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_bn_frozen_forward(const float *z, const float *res, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                    float *y, float *mean_out, float *rstd_out, int64_t rows, int32_t c, int32_t relu, void *stream) {
    PVR_REQUIRE(z && gamma && beta && run_mean && run_var && y && mean_out && rstd_out, "pvr_op_bn_frozen_forward: null argument");
    return pvr::launch_bn_frozen_apply(z, res, gamma, beta, run_mean, run_var, y, mean_out, rstd_out, rows, c, relu, (hipStream_t)stream);
}

pvr_status pvr_op_bn_frozen_backward(const float *z, const float *y, const float *dy, const float *gamma, const float *mean, const float *rstd, float *dz,
                                     float *dres, int32_t dres_accumulate, float *dgamma, float *dbeta, int64_t rows, int32_t c, int32_t relu, float *scratch,
                                     int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(z && dy && gamma && mean && rstd && dz && dgamma && dbeta && (y || !relu), "pvr_op_bn_frozen_backward: null argument");
    pvr_status s;
    if ((s = bn_frozen_check("pvr_op_bn_frozen_backward", rows, c))) return s;
    PVR_REQUIRE(scratch && scratch_floats >= pvr_op_bn_scratch_floats(rows, c), "pvr_op_bn_frozen_backward: scratch of %lld floats, pvr_op_bn_scratch_floats asks for %lld",
                (long long)scratch_floats, (long long)pvr_op_bn_scratch_floats(rows, c));
    hipStream_t st = (hipStream_t)stream;
    const int nsplit = bn_splits(rows);
    float *sums = scratch + (size_t)nsplit * 2 * c;
    BnFrozenBwd r{z, y, dy, gamma, mean, rstd, dz, dres, scratch, rows, c, relu, dres_accumulate};
    BnFin f{scratch, nsplit, c, rows, nullptr, nullptr, nullptr, nullptr, sums, dgamma, dbeta, nullptr};
    hipLaunchKernelGGL(bn_frozen_backward_kernel, dim3((c / 4 + BF_C4 - 1) / BF_C4, nsplit), dim3(256), 0, st, r);
    hipLaunchKernelGGL(bn_finalize_kernel<2>, dim3((c + 255) / 256), dim3(256), 0, st, f);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// scratch: the packed weights, launch_pack_conv_weights' (cout_pad, k*k*cin) matrix
int64_t pvr_op_conv_bn_frozen_forward_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin % 32 || cout <= 0 || cout % 4 || k < 1 || k > 3 || (stride != 1 && stride != 2) || pad < 0 || pad >= k) return 0;
    return (int64_t)((cout + 63) / 64 * 64) * k * k * cin;
}

pvr_status pvr_op_conv_bn_frozen_forward(const float *x, const float *wt, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                         const float *res, float *y, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride,
                                         int32_t pad, int32_t relu, float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(x && wt && gamma && beta && run_mean && run_var && y && scratch, "pvr_op_conv_bn_frozen_forward: null argument");
    const int64_t need = pvr_op_conv_bn_frozen_forward_scratch_floats(n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(need > 0, "pvr_op_conv_bn_frozen_forward: n %d, h %d, w %d, cin %d (%% 32 == 0), cout %d (%% 4 == 0), k %d (1 .. 3), stride %d (1 or 2), pad %d (< k)",
                n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(h + 2 * pad >= k && w + 2 * pad >= k, "pvr_op_conv_bn_frozen_forward: a %d x %d image is smaller than the %d x %d filter", h, w, k, k);
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_bn_frozen_forward: scratch of %lld floats, pvr_op_conv_bn_frozen_forward_scratch_floats asks for %lld",
                (long long)scratch_floats, (long long)need);
    const int64_t ho = (h + 2 * pad - k) / stride + 1, wo = (w + 2 * pad - k) / stride + 1;
    PVR_REQUIRE((int64_t)n * h * w * cin * 4 < 0x7ffffff0ll && need * 4 < 0x7ffffff0ll && (int64_t)n * ho * wo * cout * 4 < 0x7ffffff0ll,
                "pvr_op_conv_bn_frozen_forward: operand larger than 2 GiB (use fewer frames)");
    pvr_status s;
    if ((s = launch_pack_conv_weights(wt, scratch, cout, cin, k, false, (hipStream_t)stream))) return s;
    return launch_conv_bn_frozen_f32(x, scratch, gamma, beta, run_mean, run_var, res, y, n, h, w, cin, cout, k, stride, pad, relu, (hipStream_t)stream);
}

int64_t pvr_op_conv_wgrad_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (wgrad_check(n, h, w, cin, cout, k, stride, pad)) return 0;
    return (int64_t)wgrad_plan(n, h, w, cin, cout, k, stride, pad).nsplit * cout * k * k * cin;
}

pvr_status pvr_op_conv_wgrad(const float *x, const float *dz, float *dw, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride,
                             int32_t pad, float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(x && dz && dw && scratch, "pvr_op_conv_wgrad: null argument");
    pvr_status s;
    if ((s = wgrad_check(n, h, w, cin, cout, k, stride, pad))) return s;
    const WGradPlan g = wgrad_plan(n, h, w, cin, cout, k, stride, pad);
    const int64_t need = (int64_t)g.nsplit * cout * k * k * cin;
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_wgrad: scratch of %lld floats, pvr_op_conv_wgrad_scratch_floats asks for %lld", (long long)scratch_floats, (long long)need);
    WGrad p{x, dz, scratch, n, h, w, cin, g.ho, g.wo, cout, k, stride, pad, g.M, g.chunk, g.ci_tiles, g.co_tiles};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3(g.ci_tiles * g.co_tiles * k * k, g.nsplit), dim3(256), 0, st, p);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ew_blocks((size_t)cout * k * k * cin)), dim3(256), 0, st, scratch, dw, g.nsplit, cout, k * k, cin);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// scratch: [rotated weights (cin_pad, k*k*cout)] [zero bias, cin_pad] [dz on the zero-filled grid (stride 2)]
int64_t pvr_op_conv_dgrad_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (dgrad_check(n, h, w, cin, cout, k, stride, pad)) return 0;
    const int64_t cin_pad = (cin + 63) / 64 * 64;
    return cin_pad * k * k * cout + cin_pad + (stride == 2 ? (int64_t)n * h * w * cout : 0);
}

pvr_status pvr_op_conv_dgrad(const float *dz, const float *wt, float *dx, int32_t accumulate, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k,
                             int32_t stride, int32_t pad, float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(dz && wt && dx && scratch, "pvr_op_conv_dgrad: null argument");
    pvr_status s;
    if ((s = dgrad_check(n, h, w, cin, cout, k, stride, pad))) return s;
    const int64_t need = pvr_op_conv_dgrad_scratch_floats(n, h, w, cin, cout, k, stride, pad);
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_dgrad: scratch of %lld floats, pvr_op_conv_dgrad_scratch_floats asks for %lld", (long long)scratch_floats, (long long)need);
    const int64_t cin_pad = (cin + 63) / 64 * 64;
    float *wflip = scratch, *zero = scratch + cin_pad * k * k * cout, *dil = zero + cin_pad;
    PVR_HIP_TRY(hipMemsetAsync(zero, 0, (size_t)cin_pad * 4, (hipStream_t)stream));
    return launch_conv_dgrad(dz, wt, dx, accumulate, n, h, w, cin, cout, k, stride, pad, wflip, dil, zero, (hipStream_t)stream);
}

int64_t pvr_op_stem_wgrad_scratch_floats(int32_t n, int32_t S) {
    if (n <= 0 || S <= 0 || (S & 1)) return 0;
    const long long M = (long long)n * (S / 2) * (S / 2);
    return (M + STEM_CHUNK - 1) / STEM_CHUNK * 64 * 147;
}

pvr_status pvr_op_stem_wgrad(const float *img, const float *dz, float *dw, int32_t n, int32_t S, float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(img && dz && dw && scratch, "pvr_op_stem_wgrad: null argument");
    PVR_REQUIRE(n > 0 && S > 0 && S % 2 == 0, "pvr_op_stem_wgrad: %d frames of %d x %d (an even size)", n, S, S);
    const long long M = (long long)n * (S / 2) * (S / 2);
    const long long nsplit = (M + STEM_CHUNK - 1) / STEM_CHUNK;
    PVR_REQUIRE(nsplit < 65535, "pvr_op_stem_wgrad: %d frames are more than one launch takes", n);
    PVR_REQUIRE(scratch_floats >= nsplit * 64 * 147, "pvr_op_stem_wgrad: scratch of %lld floats, pvr_op_stem_wgrad_scratch_floats asks for %lld",
                (long long)scratch_floats, nsplit * 64 * 147);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(49, (unsigned)nsplit), dim3(256), 0, st, img, dz, scratch, S, M);
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3((64 * 147 + 255) / 256), dim3(256), 0, st, scratch, dw, (int)nsplit);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_maxpool_backward(const float *x, const float *dy, float *dx, int32_t n, int32_t h, int32_t w, int32_t c, void *stream) {
    PVR_REQUIRE(x && dy && dx, "pvr_op_maxpool_backward: null argument");
    PVR_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0, "pvr_op_maxpool_backward: empty input");
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    hipLaunchKernelGGL(maxpool_backward_kernel, dim3(ew_blocks((size_t)n * h * w * c)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n, h, w, c, ho, wo);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_avgpool_backward(const float *dout, int64_t dout_stride, float *dx, int32_t n, int32_t hw, int32_t c, void *stream) {
    PVR_REQUIRE(dout && dx, "pvr_op_avgpool_backward: null argument");
    PVR_REQUIRE(n > 0 && hw > 0 && c > 0 && dout_stride >= c, "pvr_op_avgpool_backward: n %d hw %d c %d stride %lld", n, hw, c, (long long)dout_stride);
    hipLaunchKernelGGL(avgpool_backward_kernel, dim3(ew_blocks((size_t)n * hw * c)), dim3(256), 0, (hipStream_t)stream, dout, dout_stride, dx, n, hw, c);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

}  // extern "C"
