// Weight gradients of the trainable encoder as exact-split products on the f16 matrix pipe (pvr_trainer_set_wgrad_split16; include/pvr_train.h).
//
// Arithmetic: conv_split16.hip's split, pointed at dW[co][ci] = sum over pixels m of dz[m][co] * x[pix(m, tap)][ci].  Both operands are first
// multiplied by a per-tensor power of two s = 2^(14 - floor(log2 max|t|)) (absmax_scale: gradients of 1e-6 and below would otherwise land in f16's
// subnormal range; the scaled maximum lies in [2^14, 2^15), below 65504), then a' = a_hi + 2^-11 a_lo with a_hi = f16(a'), a_lo = f16(2^11 (a' - a_hi)),
// and per fragment pair three v_mfma_f32_16x16x32_f16: hi*hi into one fp32 accumulator, the two cross terms into a second one that is scaled by 2^-11
// once at the end; the 2^-22 lo*lo term is dropped.  Products of 11-bit significands are exact in fp32.  The pixel range is split over workgroups, the
// partials go to a scratch and a second kernel sums them in split order in double, undoes s_x * s_dz (a power of two: exact) and writes torch's
// layout.  No float atomics: two runs give the same bits.  (The maximum itself is an integer max over the bit patterns of |x|: order-independent.)
//
// LDS: the reduction dimension is the pixels, so a lane's MFMA operand is 8 consecutive PIXELS of one channel, while memory has the channels of one
// pixel together.  Of the two images the guides offer, this file takes the CHANNEL-MAJOR image written by the staging pass ([hi, lo][channel][32 pixels],
// rows of 80 bytes) and reads fragments with one ds_read_b128 per operand, not pixel-major rows read with ds_read_b64_tr_b16: the transposed read needs
// EXEC all ones and 8-byte aligned four-element pieces, gives 4 of the 8 k values per instruction (twice the LDS reads per MFMA), and the staging pass
// converts fp32 to two f16 images in registers anyway, so the transpose costs it nothing but the store width.  A staging thread takes the SAME four
// channels of two neighbouring pixels and stores pixel pairs as 32-bit words: with 16 pixel pairs x 2 channel quads per 32-lane half and 20-dword rows
// the stores hit 32 distinct banks (quad stride 80 dwords = 16 mod 32), and a fragment read is 16 bytes at channel * 80 + 16 * (lane >> 4).
#include "common.h"
#include "train_internal.h"
#include "../../include/pvr_train.h"

namespace pvr {

// ------------------------------------------------------------------------------------------------------------------------------------------------
// per-tensor scale.  The maximum is an integer max over the bit patterns of |x| (vector integer atomics: order-independent).
//   pvr_op_absmax_scale: the slot is zeroed by a memset on the stream, absmax_bits_kernel takes the max into it, absmax_to_scale_kernel turns it into s.
//   pvr_op_absmax_scale_pair (the trainer's form): ONE launch for up to two tensors.  A tensor's blocks take the max into aux[0] and count themselves in
//   aux[1]; the block that counts last reads the max, writes s and leaves both words zero for the next launch (the caller zeroes aux once).
// ------------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned absmax_bits_of(const float *__restrict__ x, size_t n, int block, int blocks) {
    unsigned m = 0u;
    size_t head = (size_t)((16 - ((uintptr_t)x & 15)) & 15) / 4;                     // floats before the first 16-byte boundary
    if (head > n) head = n;
    const size_t n4 = (n - head) / 4, tail = head + n4 * 4;
    const f32x4 *x4 = reinterpret_cast<const f32x4 *>(x + head);
    const size_t stride = (size_t)blocks * 256;
    size_t i = (size_t)block * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {                                    // four loads in flight
        u32x4 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = __builtin_bit_cast(u32x4, x4[i + q * stride]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) m = max(m, b[q][e] & 0x7fffffffu);
    }
    for (; i < n4; i += stride) {
        const u32x4 b = __builtin_bit_cast(u32x4, x4[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) m = max(m, b[e] & 0x7fffffffu);
    }
    if (block == 0) {
        if (threadIdx.x < head) m = max(m, __float_as_uint(x[threadIdx.x]) & 0x7fffffffu);
        if (tail + threadIdx.x < n) m = max(m, __float_as_uint(x[tail + threadIdx.x]) & 0x7fffffffu);
    }
    return m;
}

// bits of max|x| -> the bits of s = 2^(14 - floor(log2 max)); zero and a non-finite maximum (Inf or any NaN: its pattern is above Inf's) give 1; the
// exponent is clamped to [-126, 126] so that s and 1 / s are normal (a subnormal maximum takes 126)
__device__ __forceinline__ unsigned scale_bits_of(unsigned bits) {
    const unsigned E = bits >> 23;
    int e = 0;
    if (bits != 0u && E != 255u) e = min(max(141 - (int)E, -126), 126);
    return (unsigned)(e + 127) << 23;
}

__global__ __launch_bounds__(256) void absmax_bits_kernel(const float *__restrict__ x, size_t n, unsigned *slot) {
    __shared__ unsigned sm;
    if (threadIdx.x == 0) sm = 0u;
    __syncthreads();
    atomicMax(&sm, absmax_bits_of(x, n, blockIdx.x, gridDim.x));
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(slot, sm);
}
__global__ void absmax_to_scale_kernel(unsigned *slot) { *slot = scale_bits_of(*slot); }

struct AbsMaxJob {
    const float *x;
    size_t n;
    unsigned *slot, *aux;                         // aux: [max bits, blocks done], zero on entry and on exit
    int blocks;
};
__global__ __launch_bounds__(256) void absmax_pair_kernel(AbsMaxJob a, AbsMaxJob b) {
    __shared__ unsigned sm;
    const bool first = (int)blockIdx.x < a.blocks;
    const AbsMaxJob j = first ? a : b;
    const int block = first ? blockIdx.x : blockIdx.x - a.blocks;
    if (threadIdx.x == 0) sm = 0u;
    __syncthreads();
    atomicMax(&sm, absmax_bits_of(j.x, j.n, block, j.blocks));
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(&j.aux[0], sm);
        __threadfence();                           // the max is in place before this block counts itself
        if (atomicAdd(&j.aux[1], 1u) == (unsigned)j.blocks - 1u) {
            __threadfence();
            *j.slot = scale_bits_of(atomicExch(&j.aux[0], 0u));
            atomicExch(&j.aux[1], 0u);
        }
    }
}

__device__ __forceinline__ void split_pair(float a0, float a1, unsigned &hi, unsigned &lo) {
    hi = pack2_h<true>(a0, a1);
    const pk_f16x2 q = __builtin_bit_cast(pk_f16x2, hi);
    lo = pack2_h<true>((a0 - (float)q[0]) * 2048.f, (a1 - (float)q[1]) * 2048.f);
}
__device__ __forceinline__ f32x4 mfma_h(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

constexpr int RS = 40;                            // u16 elements of a channel's row: 32 pixels + 8 (80 bytes: 16-byte aligned fragments, see the header)
constexpr float CROSS = 1.f / 2048.f;

// ------------------------------------------------------------------------------------------------------------------------------------------------
// k x k convolutions: the tiling of conv_wgrad_kernel (a 64 co x 64 ci tile of one tap and one pixel range per workgroup, 2 x 2 waves of 32 x 32),
// one step = 32 pixels = one K of the MFMA.  Border taps, the M tail and partial cout / cin tiles are zeros in the images.
// ------------------------------------------------------------------------------------------------------------------------------------------------
struct WGradS {
    const float *x, *dz, *sx, *sdz;
    float *part;                                  // [split][cout][tap][cin]
    int N, H, W, Cin, Ho, Wo, Cout, K, stride, pad, M, chunk, ci_tiles, co_tiles;
};

// TCO x TCI: the workgroup's tile.  Tiles of 128 channels (half the operand bytes per product) were measured SLOWER at batch 32, as was a split
// into fewer workgroups: these launches are bound by the latency of a workgroup's load - stage - barrier - MFMA chain, not by bytes or MFMAs, and what
// hides it is workgroups in flight (profiles/wgrad_split16_times.txt)
__global__ __launch_bounds__(256) void conv_wgrad_split16_kernel(WGradS p) {
    constexpr int TCO = 64, TCI = 64;
    constexpr int FI = TCO / 32, FJ = TCI / 32, RA = TCO / 64, RB = TCI / 64;        // fragments of a wave's (TCO / 2) x (TCI / 2); staging rounds
    __shared__ __attribute__((aligned(16))) u16 sA[2][TCO * RS], sB[2][TCI * RS];    // [hi, lo][channel][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4, wm = wave >> 1, wn = wave & 1;
    int b = blockIdx.x;
    const int cit = b % p.ci_tiles; b /= p.ci_tiles;
    const int cot = b % p.co_tiles, tap = b / p.co_tiles;
    const int kh = tap / p.K, kw = tap % p.K;
    const int m_begin = blockIdx.y * p.chunk, m_end = min(m_begin + p.chunk, p.M);
    const float sx = *p.sx, sdz = *p.sdz;
    // staging: pixels 2 pp and 2 pp + 1 of the step, channels c4 + 64 r .. + 3 of both tiles
    const int pp = lane & 15, c4 = ((lane >> 4) + 4 * wave) * 4;
    f32x4 hh[FI][FJ], xx[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) hh[i][j] = xx[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[RA][2], rb[RB][2];
    auto load = [&](int m0) {                     // the step's global loads, issued one step ahead: they fly while the MFMAs of the current step run
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + 2 * pp + i;
#pragma unroll
            for (int r = 0; r < RA; ++r) ra[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RB; ++r) rb[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (m < m_end) {
                const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, n = t / p.Ho;
#pragma unroll
                for (int r = 0; r < RA; ++r) {
                    const int co = cot * TCO + 64 * r + c4;
                    if (co < p.Cout) ra[r][i] = *reinterpret_cast<const f32x4 *>(p.dz + (size_t)m * p.Cout + co);
                }
                const int hi = ho * p.stride + kh - p.pad, wi = wo * p.stride + kw - p.pad;
                if ((unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W)
#pragma unroll
                    for (int r = 0; r < RB; ++r) {
                        const int ci = cit * TCI + 64 * r + c4;
                        if (ci < p.Cin) rb[r][i] = *reinterpret_cast<const f32x4 *>(p.x + (((size_t)n * p.H + hi) * p.W + wi) * p.Cin + ci);
                    }
            }
        }
    };
    load(m_begin);
    for (int m0 = m_begin; m0 < m_end; m0 += 32) {
        __syncthreads();                           // the previous step's fragment reads are done
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned h, l;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                split_pair(ra[r][0][e] * sdz, ra[r][1][e] * sdz, h, l);
                *reinterpret_cast<unsigned *>(&sA[0][(64 * r + c4 + e) * RS + 2 * pp]) = h;
                *reinterpret_cast<unsigned *>(&sA[1][(64 * r + c4 + e) * RS + 2 * pp]) = l;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                split_pair(rb[r][0][e] * sx, rb[r][1][e] * sx, h, l);
                *reinterpret_cast<unsigned *>(&sB[0][(64 * r + c4 + e) * RS + 2 * pp]) = h;
                *reinterpret_cast<unsigned *>(&sB[1][(64 * r + c4 + e) * RS + 2 * pp]) = l;
            }
        }
        __syncthreads();
        f16x8 ah[FI], al[FI], bh[FJ], bl[FJ];
#pragma unroll
        for (int i = 0; i < FI; ++i) {
            const int o = (wm * (TCO / 2) + i * 16 + fr) * RS + fq * 8;
            ah[i] = *reinterpret_cast<const f16x8 *>(&sA[0][o]); al[i] = *reinterpret_cast<const f16x8 *>(&sA[1][o]);
        }
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int o = (wn * (TCI / 2) + j * 16 + fr) * RS + fq * 8;
            bh[j] = *reinterpret_cast<const f16x8 *>(&sB[0][o]); bl[j] = *reinterpret_cast<const f16x8 *>(&sB[1][o]);
        }
        if (m0 + 32 < m_end) load(m0 + 32);        // (uniform over the workgroup)
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int j = 0; j < FJ; ++j) {
                hh[i][j] = mfma_h(ah[i], bh[j], hh[i][j]);
                xx[i][j] = mfma_h(ah[i], bl[j], xx[i][j]);
                xx[i][j] = mfma_h(al[i], bh[j], xx[i][j]);
            }
    }
    // D: row = co (4 * fq + r), column = ci (fr)
    const int taps = p.K * p.K;
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int cc = cit * TCI + wn * (TCI / 2) + j * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oo = cot * TCO + wm * (TCO / 2) + i * 16 + fq * 4 + r;
                if (oo < p.Cout && cc < p.Cin) p.part[(((size_t)blockIdx.y * p.Cout + oo) * taps + tap) * p.Cin + cc] = hh[i][j][r] + xx[i][j][r] * CROSS;
            }
        }
}

__global__ __launch_bounds__(256) void wgrad_split16_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, const float *sx, const float *sdz, int nsplit,
                                                                   int cout, int taps, int cin) {
    const double inv = (1.0 / (double)*sx) * (1.0 / (double)*sdz);                  // powers of two: exact
    const size_t per = (size_t)cout * taps * cin;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        double a = 0.0;
        for (int s = 0; s < nsplit; ++s) a += (double)part[(size_t)s * per + i];
        const int ci = (int)(i % cin), tap = (int)((i / cin) % taps), co = (int)(i / ((size_t)cin * taps));
        dw[((size_t)co * cin + ci) * taps + tap] = (float)(a * inv);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// conv1 (7x7 / 2, pad 3, the image as NHWC4): the same product with 64 couts, columns (tap, channel) = 196 (147 real: the NHWC4 slot is written as
// zero) padded to 13 fragments of 16, gathered from the unpadded image with border masks.  A workgroup owns STEM16_CHUNK output pixels and all columns;
// wave w owns couts 16 w .. 16 w + 15 x 13 column fragments (2 x 13 accumulators).  Partials in stem_wgrad_kernel's [split][64][147] layout.
// ------------------------------------------------------------------------------------------------------------------------------------------------
constexpr int STEM16_CHUNK = 1024, STEM16_FRAGS = 13, STEM16_COLS = STEM16_FRAGS * 16, STEM16_ITEMS = 16 * 49, STEM16_RPT = (STEM16_ITEMS + 255) / 256;

__global__ __launch_bounds__(256) void stem_wgrad_split16_kernel(const float *__restrict__ img, const float *__restrict__ dz, const float *simg, const float *sdzp,
                                                                 float *__restrict__ part, int S, int M) {
    __shared__ __attribute__((aligned(16))) u16 sA[2][64 * RS], sB[2][STEM16_COLS * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4, So = S / 2;
    const int m_begin = blockIdx.x * STEM16_CHUNK, m_end = min(m_begin + STEM16_CHUNK, M);
    const float sx = *simg, sdz = *sdzp;
    const int pp = lane & 15, c4 = ((lane >> 4) + 4 * wave) * 4;
    for (int i = tid; i < 2 * (STEM16_COLS - 196) * RS; i += 256)                    // columns 196 .. 207: never staged
        sB[i / ((STEM16_COLS - 196) * RS)][196 * RS + i % ((STEM16_COLS - 196) * RS)] = 0;
    f32x4 hh[STEM16_FRAGS], xx[STEM16_FRAGS];
#pragma unroll
    for (int j = 0; j < STEM16_FRAGS; ++j) hh[j] = xx[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = m_begin; m0 < m_end; m0 += 32) {
        f32x4 ra[2], rb[STEM16_RPT][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + 2 * pp + i;
            ra[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (m < m_end) ra[i] = *reinterpret_cast<const f32x4 *>(dz + (size_t)m * 64 + c4);
        }
#pragma unroll
        for (int r = 0; r < STEM16_RPT; ++r) {     // item = (tap, pixel pair): pixel pairs fastest
            const int it = tid + 256 * r, ip = it & 15, tap = it >> 4, kh = tap / 7, kw = tap % 7;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + 2 * ip + i;
                rb[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (it < STEM16_ITEMS && m < m_end) {
                    const int ox = m % So, t = m / So, oy = t % So, n = t / So;
                    const int iy = 2 * oy + kh - 3, ix = 2 * ox + kw - 3;
                    if ((unsigned)iy < (unsigned)S && (unsigned)ix < (unsigned)S) rb[r][i] = *reinterpret_cast<const f32x4 *>(img + (((size_t)n * S + iy) * S + ix) * 4);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned h, l;
            split_pair(ra[0][e] * sdz, ra[1][e] * sdz, h, l);
            *reinterpret_cast<unsigned *>(&sA[0][(c4 + e) * RS + 2 * pp]) = h;
            *reinterpret_cast<unsigned *>(&sA[1][(c4 + e) * RS + 2 * pp]) = l;
        }
#pragma unroll
        for (int r = 0; r < STEM16_RPT; ++r) {
            const int it = tid + 256 * r, ip = it & 15, tap = it >> 4;
            if (it < STEM16_ITEMS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned h = 0u, l = 0u;
                    if (e < 3) split_pair(rb[r][0][e] * sx, rb[r][1][e] * sx, h, l);
                    *reinterpret_cast<unsigned *>(&sB[0][(tap * 4 + e) * RS + 2 * ip]) = h;
                    *reinterpret_cast<unsigned *>(&sB[1][(tap * 4 + e) * RS + 2 * ip]) = l;
                }
            }
        }
        __syncthreads();
        const int ar = (wave * 16 + fr) * RS + fq * 8;
        const f16x8 ah = *reinterpret_cast<const f16x8 *>(&sA[0][ar]), al = *reinterpret_cast<const f16x8 *>(&sA[1][ar]);
#pragma unroll
        for (int j = 0; j < STEM16_FRAGS; ++j) {
            const int br = (j * 16 + fr) * RS + fq * 8;
            const f16x8 bh = *reinterpret_cast<const f16x8 *>(&sB[0][br]), bl = *reinterpret_cast<const f16x8 *>(&sB[1][br]);
            hh[j] = mfma_h(ah, bh, hh[j]);
            xx[j] = mfma_h(ah, bl, xx[j]);
            xx[j] = mfma_h(al, bh, xx[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < STEM16_FRAGS; ++j) {
        const int col = j * 16 + fr, tap = col >> 2, c = col & 3;
        if (c < 3 && tap < 49)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[((size_t)blockIdx.x * 64 + wave * 16 + fq * 4 + r) * 147 + c * 49 + tap] = hh[j][r] + xx[j][r] * CROSS;
    }
}

__global__ __launch_bounds__(256) void stem_wgrad_split16_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, const float *sx, const float *sdz,
                                                                        int nsplit) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * 147) return;
    const double inv = (1.0 / (double)*sx) * (1.0 / (double)*sdz);
    double a = 0.0;
    for (int s = 0; s < nsplit; ++s) a += (double)part[(size_t)s * (64 * 147) + i];
    dw[i] = (float)(a * inv);
}

namespace {

struct Plan16 { int M, ho, wo, ci_tiles, co_tiles, chunk, nsplit; };
// pvr_op_conv_wgrad's tiles and split: about 1024 workgroups per launch (measured against 512 and 2048: fewer leave the latency of a workgroup's
// chain exposed, more cost the reduction more partials than they hide), a pixel range of at least 64 (a multiple of the 32-pixel step)
Plan16 plan16(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    Plan16 g;
    g.ho = (h + 2 * pad - k) / stride + 1; g.wo = (w + 2 * pad - k) / stride + 1;
    g.M = n * g.ho * g.wo;
    g.ci_tiles = (cin + 63) / 64; g.co_tiles = (cout + 63) / 64;
    const int tiles = g.ci_tiles * g.co_tiles * k * k;
    const int want = std::max(1, std::min(1024 / tiles, (g.M + 63) / 64));
    g.chunk = ((g.M + want - 1) / want + 31) / 32 * 32;
    g.nsplit = (g.M + g.chunk - 1) / g.chunk;
    return g;
}
pvr_status check16(int n, int h, int w, int cin, int cout, int k, int stride, int pad) {
    PVR_REQUIRE(n > 0 && h > 0 && w > 0, "conv_wgrad_split16: empty input");
    PVR_REQUIRE((k == 1 || k == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad < k, "conv_wgrad_split16: k %d stride %d pad %d (k 1 or 3, stride 1 or 2, pad < k)",
                k, stride, pad);
    PVR_REQUIRE(cin % 32 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "conv_wgrad_split16: cin %d must be a multiple of 32 and cout %d of 4", cin, cout);
    PVR_REQUIRE(h + 2 * pad >= k && w + 2 * pad >= k, "conv_wgrad_split16: the %d x %d input is smaller than the filter", h, w);
    PVR_REQUIRE((int64_t)n * h * w * std::max(cin, cout) < (1ll << 31), "conv_wgrad_split16: operand of 2^31 elements or more (use a smaller batch)");
    return PVR_OK;
}
int blocks_for(size_t work) {
    const size_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}
// the scale kernels: a block ends with one atomic on one word, so few blocks of long loops (1024 float4s per thread-block round of four loads)
int absmax_blocks(size_t count) {
    const size_t b = (count / 4 + 1023) / 1024;
    return (int)(b < 1 ? 1 : b > 256 ? 256 : b);
}

}  // namespace
}  // namespace pvr

using namespace pvr;

extern "C" {

pvr_status pvr_op_absmax_scale(const float *x, int64_t count, float *scale, void *stream) {
    PVR_REQUIRE(x && scale, "pvr_op_absmax_scale: null argument");
    PVR_REQUIRE(count >= 0, "pvr_op_absmax_scale: count %lld", (long long)count);
    hipStream_t st = (hipStream_t)stream;
    PVR_HIP_TRY(hipMemsetAsync(scale, 0, 4, st));
    if (count > 0) hipLaunchKernelGGL(absmax_bits_kernel, dim3(absmax_blocks((size_t)count)), dim3(256), 0, st, x, (size_t)count, (unsigned *)scale);
    hipLaunchKernelGGL(absmax_to_scale_kernel, dim3(1), dim3(1), 0, st, (unsigned *)scale);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

pvr_status pvr_op_absmax_scale_pair(const float *x0, int64_t count0, float *scale0, const float *x1, int64_t count1, float *scale1, uint32_t *aux,
                                    void *stream) {
    PVR_REQUIRE(x0 && scale0 && aux, "pvr_op_absmax_scale_pair: null argument");
    PVR_REQUIRE(count0 >= 0 && count1 >= 0 && (x1 == nullptr) == (scale1 == nullptr), "pvr_op_absmax_scale_pair: the second tensor and its scale go together");
    AbsMaxJob a{x0, (size_t)count0, (unsigned *)scale0, aux, absmax_blocks((size_t)count0)};
    AbsMaxJob b{x1, (size_t)count1, (unsigned *)scale1, aux + 2, x1 ? absmax_blocks((size_t)count1) : 0};
    hipLaunchKernelGGL(absmax_pair_kernel, dim3(a.blocks + b.blocks), dim3(256), 0, (hipStream_t)stream, a, b);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

int64_t pvr_op_conv_wgrad_split16_scratch_floats(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad) {
    if (check16(n, h, w, cin, cout, k, stride, pad)) return 0;
    return (int64_t)plan16(n, h, w, cin, cout, k, stride, pad).nsplit * cout * k * k * cin;
}

pvr_status pvr_op_conv_wgrad_split16(const float *x, const float *dz, float *dw, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t k,
                                     int32_t stride, int32_t pad, const float *x_scale, const float *dz_scale, float *scratch, int64_t scratch_floats,
                                     void *stream) {
    PVR_REQUIRE(x && dz && dw && scratch, "pvr_op_conv_wgrad_split16: null argument");
    PVR_REQUIRE(x_scale && dz_scale, "pvr_op_conv_wgrad_split16: null scale (pvr_op_absmax_scale writes one per operand)");
    pvr_status s;
    if ((s = check16(n, h, w, cin, cout, k, stride, pad))) return s;
    const Plan16 g = plan16(n, h, w, cin, cout, k, stride, pad);
    const int64_t need = (int64_t)g.nsplit * cout * k * k * cin;
    PVR_REQUIRE(scratch_floats >= need, "pvr_op_conv_wgrad_split16: scratch of %lld floats, pvr_op_conv_wgrad_split16_scratch_floats asks for %lld",
                (long long)scratch_floats, (long long)need);
    WGradS p{x, dz, x_scale, dz_scale, scratch, n, h, w, cin, g.ho, g.wo, cout, k, stride, pad, g.M, g.chunk, g.ci_tiles, g.co_tiles};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv_wgrad_split16_kernel, dim3(g.ci_tiles * g.co_tiles * k * k, g.nsplit), dim3(256), 0, st, p);
    hipLaunchKernelGGL(wgrad_split16_reduce_kernel, dim3(blocks_for((size_t)cout * k * k * cin)), dim3(256), 0, st, scratch, dw, x_scale, dz_scale, g.nsplit, cout,
                       k * k, cin);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

int64_t pvr_op_stem_wgrad_split16_scratch_floats(int32_t n, int32_t S) {
    if (n <= 0 || S <= 0 || (S & 1)) return 0;
    const long long M = (long long)n * (S / 2) * (S / 2);
    return (M + STEM16_CHUNK - 1) / STEM16_CHUNK * 64 * 147;
}

pvr_status pvr_op_stem_wgrad_split16(const float *img, const float *dz, float *dw, int32_t n, int32_t S, const float *img_scale, const float *dz_scale,
                                     float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(img && dz && dw && scratch, "pvr_op_stem_wgrad_split16: null argument");
    PVR_REQUIRE(img_scale && dz_scale, "pvr_op_stem_wgrad_split16: null scale (pvr_op_absmax_scale writes one per operand)");
    PVR_REQUIRE(n > 0 && S > 0 && S % 2 == 0, "pvr_op_stem_wgrad_split16: %d frames of %d x %d (an even size)", n, S, S);
    const long long M = (long long)n * (S / 2) * (S / 2);
    PVR_REQUIRE(M * 64 < (1ll << 31), "pvr_op_stem_wgrad_split16: %d frames are more than one launch takes", n);
    const long long nsplit = (M + STEM16_CHUNK - 1) / STEM16_CHUNK;
    PVR_REQUIRE(scratch_floats >= nsplit * 64 * 147, "pvr_op_stem_wgrad_split16: scratch of %lld floats, pvr_op_stem_wgrad_split16_scratch_floats asks for %lld",
                (long long)scratch_floats, nsplit * 64 * 147);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stem_wgrad_split16_kernel, dim3((unsigned)nsplit), dim3(256), 0, st, img, dz, img_scale, dz_scale, scratch, S, (int)M);
    hipLaunchKernelGGL(stem_wgrad_split16_reduce_kernel, dim3((64 * 147 + 255) / 256), dim3(256), 0, st, scratch, dw, img_scale, dz_scale, (int)nsplit);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

}  // extern "C"
