// fp32 attention core of the ViT plans' reference-precision mode (dtype PVR_F32): fp32 qkv in, fp32 out, both matrix products on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32 = an exact fp32 fma chain), scores, maximum, exp2, normaliser and P in fp32 - nothing is rounded
// to 16 bits.  The transposed-score form of vit.hip's 16-bit kernel carries over: a D tile of S^T = K Q^T holds keys 4*(lane>>4)+r for
// query lane&15 in register r, which is the B operand (k-slot lane>>4) of k-step r of O^T = V^T P^T when V^T's A operand takes its
// k-slot from the same key, 16*nt + 4*(lane>>4) + r: P never leaves its registers.
//
// One workgroup = 64 queries (one 16-query tile per wave) of one (image, head), grid (heads, images, ceil(T / 64)).  fp32 K and V of 288 keys x
// 80 do not both fit in LDS (96 KB each), so the workgroup stages K, keeps its query tile's scores in registers, and stages V into the same
// buffer.  Keys are padded to TK = 16 ceil(T / 16): rows behind T are filled with zeros (never read from memory) and score -inf.
// No atomics and a fixed order of every sum: run-to-run and batch-composition bit identity.
#include "encoder_internal.h"

namespace pvr {

template <int HD, int MAXNT>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float *__restrict__ qkv, float *__restrict__ out, int T, int W) {
    constexpr int LD = HD + 4, CH = HD / 4, G = HD / 16, MT = HD / 16;   // LD: 4 LD = 16 (mod 64) banks and LD = 4 (mod 16): both read patterns below are conflict-free
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *S = reinterpret_cast<float *>(smem);                          // [TK][LD]: K, then V
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int hd = blockIdx.x, b = blockIdx.y, qt = blockIdx.z * 4 + wave;
    const int NT = (T + 15) / 16, TK = NT * 16;
    const size_t rs = (size_t)3 * W;
    const float *base = qkv + (size_t)b * T * rs + hd * HD;
    // out-of-range rows take an offset past num_records and read zeros: branch-free loads, and nothing behind row T - 1 is touched
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (unsigned)((size_t)T * rs * 4), 0x00020000);
    constexpr int OOB = 0x7ffffff0;
    // which = 1: K, 2: V.  A thread moves 16-byte chunks, four loads in flight
    auto fill = [&](int which) {
        const int items = TK * CH;
        for (int i0 = 0; i0 < items; i0 += 1024) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = i0 + u * 256 + tid, row = idx / CH, ch = idx % CH;
                const int off = (idx < items && row < T) ? (int)(((size_t)row * rs + (size_t)which * W + ch * 4) * 4) : OOB;
                v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = i0 + u * 256 + tid, row = idx / CH, ch = idx % CH;
                if (idx < items) *reinterpret_cast<f32x4 *>(S + row * LD + ch * 4) = v[u];
            }
        }
    };
    fill(1);
    const bool active = qt * 16 < T;                               // wave-uniform
    const int query = qt * 16 + fr;
    // B operand of S^T = K Q^T: Q[query = fr][d]; k-step 4 g + j sums over d = 16 g + 4 fq + j for both operands (one 16-byte read each)
    f32x4 qf[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int off = (active && query < T) ? (int)(((size_t)query * rs + g * 16 + fq * 4) * 4) : OOB;
        qf[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
    }
    __syncthreads();
    f32x4 s[MAXNT];
    float inv = 0.f;
    if (active) {
#pragma unroll
        for (int nt = 0; nt < MAXNT; ++nt) {
            s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (nt < NT) {
                const float *kr = S + (nt * 16 + fr) * LD + fq * 4;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const f32x4 kf = *reinterpret_cast<const f32x4 *>(kr + g * 16);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j], qf[g][j], s[nt], 0, 0, 0);
                }
            }
        }
        // s[nt][r] = S^T[key = nt*16 + 4*fq + r][query = fr]; softmax over keys in the log2 domain (scale * log2(e) in one multiply)
        const float scale = (HD == 64 ? 0.125f : 1.0f / sqrtf((float)HD)) * 1.44269504088896341f;
        float mx = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < MAXNT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = nt * 16 + fq * 4 + r;
                const float v = (nt < NT && key < T) ? s[nt][r] * scale : -INFINITY;
                s[nt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < MAXNT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(s[nt][r] - mx);    // 2^(-inf) = 0 for padded keys
                s[nt][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        inv = 1.0f / sum;
    }
    __syncthreads();                                               // every wave is done with K
    fill(2);
    __syncthreads();
    if (!active) return;
    // O^T = V^T P^T: k-step (nt, r), k-slot fq <-> key 16 nt + 4 fq + r for both operands
    f32x4 o[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) o[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < MAXNT; ++nt) {
        if (nt < NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *vr = S + (nt * 16 + fq * 4 + r) * LD + fr;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[mt * 16], s[nt][r], o[mt], 0, 0, 0);
            }
        }
    }
    // o[mt][r] = O[query = fr][d = 16 mt + 4 fq + r]
    if (query < T) {
        float *orow = out + ((size_t)b * T + query) * W + hd * HD + fq * 4;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            *reinterpret_cast<f32x4 *>(orow + mt * 16) = f32x4{o[mt][0] * inv, o[mt][1] * inv, o[mt][2] * inv, o[mt][3] * inv};
    }
}

template <int HD, int MAXNT>
static pvr_status launch_attention_f32_inst(const float *qkv, float *out, int T, int W, int heads, int nb, hipStream_t st) {
    const size_t lds = (size_t)((T + 15) / 16 * 16) * (HD + 4) * 4;   // <= 288 * 84 * 4 = 96768
    static DeviceOnce attr_done;          // per device: a second GPU of the process needs the attribute too
    if (attr_done.needed()) {
        PVR_HIP_TRY(hipFuncSetAttribute((const void *)attention_f32_kernel<HD, MAXNT>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr_done.mark();
    }
    hipLaunchKernelGGL((attention_f32_kernel<HD, MAXNT>), dim3(heads, nb, (T + 63) / 64), dim3(256), lds, st, qkv, out, T, W);
    PVR_LAUNCH_CHECK();
    return PVR_OK;
}

// key-tile instantiations: 4 (T <= 64: CLIP B/32's 50), 13 (T <= 208: the /16 plans' 197), 18 (T <= 288: MAE H/14's 257)
pvr_status launch_attention_f32(const float *qkv, float *out, int T, int W, int heads, int nb, hipStream_t st) {
    PVR_REQUIRE(qkv && out, "attention: null pointer");
    PVR_REQUIRE(T > 0 && T <= 288 && heads > 0 && nb > 0 && nb <= 65535 && W > 0, "attention: %d tokens (1..288), %d heads, %d images not built", T, heads, nb);
    const int hd = W / heads, nt = (T + 15) / 16;
    PVR_REQUIRE(W == heads * hd && (hd == 64 || hd == 80), "attention: head dim %d not built", hd);
    if (hd == 64) {
        if (nt <= 4) return launch_attention_f32_inst<64, 4>(qkv, out, T, W, heads, nb, st);
        if (nt <= 13) return launch_attention_f32_inst<64, 13>(qkv, out, T, W, heads, nb, st);
        return launch_attention_f32_inst<64, 18>(qkv, out, T, W, heads, nb, st);
    }
    if (nt <= 4) return launch_attention_f32_inst<80, 4>(qkv, out, T, W, heads, nb, st);
    if (nt <= 13) return launch_attention_f32_inst<80, 13>(qkv, out, T, W, heads, nb, st);
    return launch_attention_f32_inst<80, 18>(qkv, out, T, W, heads, nb, st);
}

}  // namespace pvr
