// Frozen-encoder plan: ResNet50 family (conv5 / l4-compressed / l3-compressed) as a static list of
// fused launches over a pre-allocated HBM workspace.
//
// Replaces: reference src/embeddings.py:386-402 (EmbeddingNet.forward), the model construction at
// src/vision_models/moco.py:6-113 and resnet.py:6-104 (topology edits), and torchvision's
// ResNet._forward_impl.  Weight names are torchvision's (SURVEY 8a "State-dict keys").
//
// The launch plan itself is made in pvr_encoder_create (encoder_plan.hip: host arithmetic on the desc and the switches).  pvr_encoder_finalize does what needs
// weights and a device: stem, finalize_conv per convolution, prepare_weights (the packed images the planned launches read), workspace, zero page.
//
// Host-side work done once in finalize():
//   * BN eval fold:  scale = gamma / sqrt(var + 1e-5),  W' = W*scale,  b' = beta - mean*scale (+ scale*conv_bias)
//   * stem: Normalize + /255 folded into conv1 (see stem.hip), K laid out (kh, kw[8], c[4])
//   * OIHW fp32 -> [cout_pad][kh][kw][cin_pad] 16-bit (bf16 or f16), zero padded
#include "encoder_internal.h"

namespace pvr {

pvr_status launch_split16_pack(const float *w, void *out, int rows, int K, hipStream_t stream);
pvr_status launch_conv_split16(const float *in, const void *wsp, const float *bias, const float *res, float *out, int n, int h, int w, int cin,
                               int cout, int k, int stride, int pad, int relu, hipStream_t stream, float *out2 = nullptr, int n1 = 0, void *out16 = nullptr,
                               int terms = 3);

// every environment switch of the encoder path (PlanSwitches), read ONCE per encoder in pvr_encoder_create (never on the forward path)
void read_switches(PlanSwitches &sw) {
    auto get = [](const char *name, int def) { const char *v = getenv(name); return v ? atoi(v) : def; };
    sw.pool_fuse = get("PVR_POOL_FUSE", 1);
    sw.stem_u8 = get("PVR_STEM_U8", 1);
    sw.stem_lds = get("PVR_STEM_LDS", 1);
    sw.stem_regpool = get("PVR_STEM_REGPOOL", 1);
    sw.frame_front1 = get("PVR_FRAME_FRONT1", 1);
    sw.frame_next1 = get("PVR_FRAME_NEXT1", 0);
    sw.frame_bneck = get("PVR_FRAME_BNECK", 1);
    sw.bneck_stagger = get("PVR_FRAME_STAGGER", 0);
    sw.dual_ds = get("PVR_DUAL_DS", 1);
    sw.chain_ds = get("PVR_CHAIN_DS", 1);
    sw.chain_blocked = get("PVR_CHAIN_BLOCKED", 1);
    sw.chain_halo = get("PVR_CHAIN_HALO", 1);
    sw.chain_ds_occ = get("PVR_CHAIN_DS_OCC", 3);
    sw.chain_pfk = get("PVR_CHAIN_PFK", 12);
    sw.chain_cfg = get("PVR_CHAIN_CFG", 12);
    sw.chain_wave = get("PVR_CHAIN_WAVE", 1);
    sw.chain_wave_halo = get("PVR_CHAIN_WAVE_HALO", 1);
    sw.chain_wave_128 = get("PVR_CHAIN_WAVE_128", 1);
    sw.strided_y = get("PVR_STRIDED_Y", 1);
    sw.splitk = get("PVR_SPLITK", 1);
    sw.smallk_div = get("PVR_SMALLK_DIV", 4);
    if (sw.smallk_div < 1) sw.smallk_div = 1;
    sw.frame_min_n = get("PVR_FRAME_MIN_N", 128);
    sw.frame_run = get("PVR_FRAME_RUN", 0);       // (measured equal to one launch per bottleneck: opt-in, profiles/experiments/r06_bneck_frame_run.txt)
    sw.frame_stagger = get("PVR_FRAME_RUN_STAGGER", 0);
    sw.split16 = get("PVR_SPLIT16", 1);
    sw.stem_conv1 = get("PVR_STEM_CONV1", 1);
    sw.resid32 = get("PVR_RESID32", 1);
    sw.tail_f32 = get("PVR_TAIL_F32", 1);
    sw.fuse = get("PVR_FUSE", 1);
    sw.conv_algo = get("PVR_CONV_ALGO", -1);
    sw.conv_halo = get("PVR_CONV_HALO", 1);
    sw.conv_expand = get("PVR_CONV_EXPAND", 1);
    sw.conv_wfrag = get("PVR_CONV_WFRAG", 1);
    sw.wfrag_ko = get("PVR_WFRAG_KO", 0);
    sw.igemm_nk4 = get("PVR_IGEMM_NK4", 1);
    sw.igemm_bm64 = get("PVR_IGEMM_BM64", 0);
    sw.pp_bm224 = get("PVR_PP_BM224", 1);
    sw.pp_persist = get("PVR_PP_PERSIST", 384);
}

PlanSwitches &op_switches() {
    static PlanSwitches sw = [] { PlanSwitches v; read_switches(v); return v; }();
    return sw;
}

// f16 range validation (pvr_encoder_check_range): any inf / NaN among the first `n` 16-bit (or fp32) values of a launch's output -> flags[idx] = 1
template <bool F32>
__global__ __launch_bounds__(256) void range_flag_kernel(const void *x, size_t n8, int dtype, int *flags, int idx) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        if constexpr (F32) {
            const u32x4 a = reinterpret_cast<const u32x4 *>(x)[2 * i], b = reinterpret_cast<const u32x4 *>(x)[2 * i + 1];
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= (a[e] & 0x7f800000u) == 0x7f800000u || (b[e] & 0x7f800000u) == 0x7f800000u;
        } else {
            const u32x4 a = reinterpret_cast<const u32x4 *>(x)[i];
            const unsigned em = dtype == PVR_F16 ? 0x7c00u : 0x7f80u;          // exponent field all ones: inf or NaN
#pragma unroll
            for (int e = 0; e < 4; ++e) bad |= ((a[e] & em) == em) || (((a[e] >> 16) & em) == em);
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flags + idx, 1);
}

// ... of a PVR_F32S plan: the next convolution rounds the high part of its fp32 operand to f16, so a finite activation above 65504 becomes inf there (and its low
// part NaN) - flagged here, on the fp32 value, together with inf / NaN (both compare above 65504 as magnitudes of the bit pattern)
__global__ __launch_bounds__(256) void range_flag_split_kernel(const float *x, size_t n4, int *flags, int idx) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const u32x4 a = reinterpret_cast<const u32x4 *>(x)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= (a[e] & 0x7fffffffu) > 0x477fe000u;      // 65504.0f
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(flags + idx, 1);
}
static void launch_range_flag_split(const void *x, size_t elems, int *flags, int idx, hipStream_t st) {
    const size_t n4 = elems / 4;
    hipLaunchKernelGGL(range_flag_split_kernel, dim3((unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048)), dim3(256), 0, st, (const float *)x, n4, flags, idx);
}

const HostTensor *enc_find(pvr_encoder *e, const std::string &name) {
    auto it = e->weights.find(name);
    return it == e->weights.end() ? nullptr : &it->second;
}

pvr_status enc_need(pvr_encoder *e, const std::string &name, const HostTensor **out, size_t numel) {
    const HostTensor *t = enc_find(e, name);
    if (!t) { set_error("missing weight: %s", name.c_str()); return PVR_ERR_MISSING_WEIGHT; }
    if (t->data.size() != numel) {
        set_error("weight %s has %zu elements, expected %zu", name.c_str(), t->data.size(), numel);
        return PVR_ERR_INVALID;
    }
    *out = t;
    return PVR_OK;
}

static pvr_status bn_fold(pvr_encoder *e, const std::string &bn, int c, std::vector<float> &scale,
                          std::vector<float> &shift) {
    const HostTensor *g, *b, *m, *v;
    pvr_status s;
    if ((s = enc_need(e, bn + ".weight", &g, c))) return s;
    if ((s = enc_need(e, bn + ".bias", &b, c))) return s;
    if ((s = enc_need(e, bn + ".running_mean", &m, c))) return s;
    if ((s = enc_need(e, bn + ".running_var", &v, c))) return s;
    scale.resize(c); shift.resize(c);
    for (int i = 0; i < c; ++i) {
        scale[i] = g->data[i] / sqrtf(v->data[i] + 1e-5f);
        shift[i] = b->data[i] - m->data[i] * scale[i];
    }
    return PVR_OK;
}


static pvr_status finalize_conv(pvr_encoder *e, ConvOp &op) {
    const int k = op.k, cr = op.cin_real, cor = op.cout_real;
    const HostTensor *w;
    pvr_status s;
    if ((s = enc_need(e, op.conv + ".weight", &w, (size_t)cor * cr * k * k))) return s;
    std::vector<float> scale, shift;
    if ((s = bn_fold(e, op.bn, cor, scale, shift))) return s;
    if (const HostTensor *cb = enc_find(e, op.conv + ".bias")) {
        if ((int)cb->data.size() != cor) { set_error("bad bias size for %s", op.conv.c_str()); return PVR_ERR_INVALID; }
        for (int i = 0; i < cor; ++i) shift[i] += scale[i] * cb->data[i];
    }
    const int cout_pad = (op.cout + 63) / 64 * 64;
    const size_t K = (size_t)k * k * op.cin;
    std::vector<u16> hw(cout_pad * K, 0);
    for (int co = 0; co < cor; ++co)
        for (int ci = 0; ci < cr; ++ci)
            for (int a = 0; a < k; ++a)
                for (int b = 0; b < k; ++b) {
                    const float v = w->data[(((size_t)co * cr + ci) * k + a) * k + b] * scale[co];
                    hw[co * K + ((size_t)a * k + b) * op.cin + ci] = f32_to_h(v, e->desc.dtype);
                }
    std::vector<float> hb(cout_pad, 0.f);
    for (int co = 0; co < cor; ++co) hb[co] = shift[co];
    if (stores_f32(e->desc.dtype) || op.f32op || op.from32) {   // reference-precision modes / fp32 head of a 16-bit plan / a 16-bit conv reading fp32: same layout, fp32 values
        std::vector<float> hf(cout_pad * K, 0.f);
        for (int co = 0; co < cor; ++co)
            for (int ci = 0; ci < cr; ++ci)
                for (int a = 0; a < k; ++a)
                    for (int b = 0; b < k; ++b)
                        hf[co * K + ((size_t)a * k + b) * op.cin + ci] = w->data[(((size_t)co * cr + ci) * k + a) * k + b] * scale[co];
        if ((s = enc_upload(&op.d_wf, hf))) return s;
        if (op.split16) {
            // the fp32 stage / head of the parity plan (every convolution of a PVR_F32S plan) on the 16-bit matrix pipe: (hi, lo) f16 pairs of the same fp32 weights (conv_split16.hip); for a from32
            // convolution only the hi half is used: f16(w), the 16-bit plan's own weight.  (d_wf stays until prepare_weights has made the head's pair image)
            PVR_HIP_TRY(hipMalloc((void **)&op.d_wsp, (size_t)cout_pad * K * 4));
            if ((s = launch_split16_pack(op.d_wf, op.d_wsp, cout_pad, (int)K, nullptr))) return s;
        }
        if (op.from32 && !op.split16) { set_error("%s: a convolution that reads the fp32 stream needs the conv_split16 weight image (cin %d, cout %d)", op.conv.c_str(), op.cin, op.cout); return PVR_ERR_INVALID; }
        op.h_b = hb;
        return enc_upload(&op.d_b, hb);
    }
    if ((s = enc_upload(&op.d_w, hw))) return s;
    op.h_w = std::move(hw);
    op.h_b = hb;
    return enc_upload(&op.d_b, hb);
}

static pvr_status pack_wfb(ConvOp &o) {          // d_wfb: the fragment-blocked copy of d_w (bneck_frame.hip, conv_wfrag.hip)
    if (o.d_wfb) return PVR_OK;
    const size_t K = (size_t)o.k * o.k * o.cin;
    PVR_HIP_TRY(hipMalloc((void **)&o.d_wfb, (size_t)o.cout * K * 2));
    return launch_pack_frag_weights(o.d_w, o.d_wfb, o.cout, (int)K, nullptr);
}

// The device images the plan's launches read besides d_w / d_b (the plan itself is made at create: encoder_plan.hip): per launch of the fused schedule,
// exactly what its role needs.
static pvr_status prepare_weights(pvr_encoder *e) {
    pvr_status s;
    for (ConvOp &op : e->ops)                    // frame members and the stand-alone launches conv_wfrag may take (either schedule)
        if (op.wfrag && (s = pack_wfb(op))) return s;
    for (const Launch &l : e->sched_fused) {
        if (l.form == LF_CHAIN) {
            // a chain: b3 + b_downsample when the downsample runs inside, row-permuted copies of its 1x1 weights
            ConvOp &o3 = e->ops[l.conv3];
            if (l.ds >= 0) {
                std::vector<float> bs(o3.h_b);
                for (size_t c = 0; c < bs.size(); ++c) bs[c] += e->ops[l.ds].h_b[c];
                if ((s = enc_upload(&o3.d_bsum, bs))) return s;
            }
            for (int which = 0; which < 3; ++which) {
                const int oi = which == 0 ? l.conv3 : which == 1 ? l.next1 : l.ds;
                if (oi < 0) continue;
                ConvOp &o = e->ops[oi];
                if (o.d_wp) continue;
                const size_t K = (size_t)o.cin;
                std::vector<u16> hp((size_t)o.cout * K);
                for (int r = 0; r < o.cout; ++r) memcpy(&hp[(size_t)r * K], &o.h_w[(size_t)chain_row_source(r) * K], K * 2);
                if ((s = enc_upload(&o.d_wp, hp))) return s;
                if (which != 1) {                        // W3 / Wd once more, in the blocked layout the wave form reads its L2-resident pieces in
                    std::vector<u16> hb(hp.size());
                    for (int r = 0; r < o.cout; ++r)
                        for (size_t c = 0; c < K; ++c) hb[(((size_t)(r >> 4) * (K / 8) + (c >> 3)) * 16 + (r & 15)) * 8 + (c & 7)] = hp[(size_t)r * K + c];
                    if ((s = enc_upload(&o.d_wpb, hb))) return s;
                }
            }
        } else if (l.form == LF_DUAL) {
            // the two-operand launch: [W3 | W_downsample] rows, b3 + b_downsample
            ConvOp &o3 = e->ops[l.conv2];
            const ConvOp &od = e->ops[l.ds];
            const size_t K1 = (size_t)o3.cin, K2 = (size_t)od.cin, cp = ((size_t)o3.cout + 63) / 64 * 64;
            std::vector<u16> wc(cp * (K1 + K2), 0);
            for (int r = 0; r < o3.cout; ++r) {
                memcpy(&wc[(size_t)r * (K1 + K2)], &o3.h_w[(size_t)r * K1], K1 * 2);
                memcpy(&wc[(size_t)r * (K1 + K2) + K1], &od.h_w[(size_t)r * K2], K2 * 2);
            }
            std::vector<float> bs(cp, 0.f);
            for (int c = 0; c < o3.cout; ++c) bs[c] = o3.h_b[c] + od.h_b[c];
            if ((s = enc_upload(&o3.d_wcat, wc)) || (s = enc_upload(&o3.d_bsum, bs))) return s;
        } else if (l.form == LF_PAIR) {
            // the conv_split16 pair: [W1 ; Wd] (128 couts) as one split weight image, both biases
            ConvOp &op = e->ops[l.conv2];
            const ConvOp &od = e->ops[l.pair];
            const size_t K = (size_t)op.k * op.k * op.cin;
            float *cat = nullptr;
            PVR_HIP_TRY(hipMalloc((void **)&cat, 128 * K * 4));
            PVR_HIP_TRY(hipMemcpy(cat, op.d_wf, 64 * K * 4, hipMemcpyDeviceToDevice));
            PVR_HIP_TRY(hipMemcpy(cat + 64 * K, od.d_wf, 64 * K * 4, hipMemcpyDeviceToDevice));
            PVR_HIP_TRY(hipMalloc((void **)&op.d_wsp_pair, 128 * K * 4));
            s = launch_split16_pack(cat, op.d_wsp_pair, 128, (int)K, nullptr);
            PVR_HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(cat);
            if (s) return s;
            std::vector<float> bb(128, 0.f);
            for (int c = 0; c < 64; ++c) { bb[c] = op.h_b[c]; bb[64 + c] = od.h_b[c]; }
            if ((s = enc_upload(&op.d_b_pair, bb))) return s;
        }
    }
    if (e->stem_c1 >= 0) {                               // layer1.0.conv1 inside the fused stem: its weights as the stem's fragment image
        std::vector<u16> img(64 * 64);
        stem_c1_pack(e->ops[e->stem_c1].h_w.data(), img.data());
        if ((s = enc_upload(&e->d_stem_c1w, img))) return s;
    }
    return PVR_OK;
}

// conv_name (cout_real, 3, ks, ks) with ks = 7 (torchvision) or 3 (CLIP: stride 2, pad 1 == the centre 3x3 taps of a 7x7 / pad 3)
static pvr_status finalize_stem(pvr_encoder *e, const std::string &conv_name = "conv1.weight", const std::string &bn_name = "bn1",
                                int cout_real = 64, int ks = 7) {
    const HostTensor *w;
    pvr_status s;
    if ((s = enc_need(e, conv_name, &w, (size_t)cout_real * 3 * ks * ks))) return s;
    std::vector<float> scale, shift;
    if ((s = bn_fold(e, bn_name, cout_real, scale, shift))) return s;
    scale.resize(64, 0.f); shift.resize(64, 0.f);
    const int t0 = (7 - ks) / 2;
    auto wat = [&](int co, int c, int a, int b) -> double {       // 7x7 view of the (possibly smaller) filter
        const int aa = a - t0, bb = b - t0;
        if (co >= cout_real || aa < 0 || aa >= ks || bb < 0 || bb >= ks) return 0.0;
        return (double)w->data[(((size_t)co * 3 + c) * ks + aa) * ks + bb];
    };
    if (e->desc.dtype == PVR_F32) {               // normalisation stays a separate fp32 kernel, exactly as torch applies it
        std::vector<float> hf(64 * 49 * 4, 0.f);
        for (int co = 0; co < 64; ++co)
            for (int c = 0; c < 3; ++c)
                for (int t = 0; t < 49; ++t) hf[((size_t)co * 49 + t) * 4 + c] = (float)wat(co, c, t / 7, t % 7) * scale[co];
        if ((s = enc_upload(&e->d_stem_wf, hf))) return s;
        return enc_upload(&e->d_stem_b, shift);
    }
    if (e->desc.dtype == PVR_F32S) {              // the same folded fp32 weights in the 16-bit stem's K order (a 8 + b) 4 + c, as the split image stem_split16.hip reads
        std::vector<float> hf(64 * 224, 0.f);
        for (int co = 0; co < 64; ++co)
            for (int c = 0; c < 3; ++c)
                for (int t = 0; t < 49; ++t) hf[(size_t)co * 224 + ((t / 7) * 8 + t % 7) * 4 + c] = (float)wat(co, c, t / 7, t % 7) * scale[co];
        float *d_hf = nullptr;
        if ((s = enc_upload(&d_hf, hf))) return s;
        PVR_HIP_TRY(hipMalloc((void **)&e->d_stem_w, 64 * 224 * 4));
        s = launch_split16_pack(d_hf, e->d_stem_w, 64, 224, nullptr);
        PVR_HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(d_hf);
        if (s) return s;
        return enc_upload(&e->d_stem_b, shift);
    }
    std::vector<u16> hw(64 * 224, 0);
    for (int co = 0; co < 64; ++co)
        for (int a = 0; a < 7; ++a)
            for (int b = 0; b < 7; ++b) {
                double vsum = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double wv = wat(co, c, a, b) * scale[co];
                    // (x/255 - mean)/std with x = xc + 128:  xc/(255 std) + (128 - 255 mean)/(255 std)
                    hw[co * 224 + (a * 8 + b) * 4 + c] = f32_to_h((float)(wv / (255.0 * e->desc.std_[c])), e->desc.dtype);
                    vsum += wv * (128.0 - 255.0 * e->desc.mean[c]) / (255.0 * e->desc.std_[c]);
                }
                hw[co * 224 + (a * 8 + b) * 4 + 3] = f32_to_h((float)vsum, e->desc.dtype);
            }
    if ((s = enc_upload(&e->d_stem_w, hw))) return s;
    return enc_upload(&e->d_stem_b, shift);
}

// CLIP AttentionPool2d parameters: q/k/v projections concatenated row-wise (one GEMM), c_proj, positional embedding
static pvr_status finalize_attnpool(pvr_encoder *e) {
    const int C = 2048, O = 1024, dt = e->desc.dtype;
    const std::string a = "visual.attnpool.";
    pvr_status s;
    std::vector<u16> wq((size_t)3 * C * C);
    std::vector<float> bq((size_t)3 * C);
    const char *nm[3] = {"q_proj", "k_proj", "v_proj"};
    for (int i = 0; i < 3; ++i) {
        const HostTensor *w, *b;
        if ((s = enc_need(e, a + nm[i] + ".weight", &w, (size_t)C * C))) return s;
        if ((s = enc_need(e, a + nm[i] + ".bias", &b, (size_t)C))) return s;
        for (size_t k = 0; k < (size_t)C * C; ++k) wq[(size_t)i * C * C + k] = f32_to_h(w->data[k], dt);
        for (int k = 0; k < C; ++k) bq[(size_t)i * C + k] = b->data[k];
    }
    const HostTensor *wc, *bc, *pos;
    if ((s = enc_need(e, a + "c_proj.weight", &wc, (size_t)O * C))) return s;
    if ((s = enc_need(e, a + "c_proj.bias", &bc, (size_t)O))) return s;
    if ((s = enc_need(e, a + "positional_embedding", &pos, (size_t)50 * C))) return s;
    std::vector<u16> wch((size_t)O * C);
    for (size_t k = 0; k < wch.size(); ++k) wch[k] = f32_to_h(wc->data[k], dt);
    if ((s = enc_upload(&e->ap_wqkv, wq)) || (s = enc_upload(&e->ap_bqkv, bq)) || (s = enc_upload(&e->ap_wc, wch)) ||
        (s = enc_upload(&e->ap_bc, bc->data)) || (s = enc_upload(&e->ap_pos, pos->data))) return s;
    PVR_HIP_TRY(hipMalloc((void **)&e->ap_out, (size_t)e->desc.chunk * O * sizeof(float) * PVR_MAX_LANES));
    return PVR_OK;
}

}  // namespace pvr

using Lane = pvr_encoder::Lane;

static void *bufp(const Lane &L, int id) { return id == B_STEM ? (void *)L.d_stem : L.buf[id]; }

// The low-latency plan's scratch, for every lane that has a workspace: allocated when the plan is switched on (pvr_encoder_set_low_latency), at
// finalize when it was switched on before, and when a lane's workspace is first made - never inside a forward (no allocation on the
// forward path after finalize).
static pvr_status lane_smallk(pvr_encoder *enc, Lane &L) {
    if (enc->low_latency && !L.d_smallk) PVR_HIP_TRY(hipMalloc((void **)&L.d_smallk, SMALLK_BYTES));
    return PVR_OK;
}
static pvr_status ensure_smallk(pvr_encoder *enc) {
    if (enc->vit || enc->rnd || enc->host) return PVR_OK;
    pvr_status s;
    for (Lane &L : enc->lanes)
        if (L.valid && (s = lane_smallk(enc, L))) return s;
    return PVR_OK;
}

// activation workspace of one lane (ResNet50 family)
static pvr_status alloc_workspace(pvr_encoder *enc, Lane &L) {
    const int C = enc->desc.chunk, crop = enc->desc.crop;
    const bool f32 = stores_f32(enc->desc.dtype);
    const size_t esz = f32 ? 4 : 2;                               // activation element size
    const size_t img = (size_t)C * (crop + 6) * (crop + 8) * 4;
    PVR_HIP_TRY(hipMalloc((void **)&L.d_img, img * 2));
    PVR_HIP_TRY(hipMemset(L.d_img, 0, img * 2));            // zero border = conv1 padding, written once
    PVR_HIP_TRY(hipMalloc((void **)&L.d_stem, (size_t)C * 112 * 112 * 64 * esz));
    if (enc->desc.dtype == PVR_F32S) {                         // the normalised image in d_img's zero-bordered layout: border written once, here
        PVR_HIP_TRY(hipMalloc((void **)&L.d_imgf, img * sizeof(float)));
        PVR_HIP_TRY(hipMemset(L.d_imgf, 0, img * sizeof(float)));
    } else if (f32) PVR_HIP_TRY(hipMalloc((void **)&L.d_imgf, (size_t)C * crop * crop * 4 * sizeof(float)));
    for (int b = 0; b < B_COUNT; ++b) {
        size_t bytes = enc->buf_elems * esz;
        if (b == B_F32) bytes = (size_t)C * enc->final_hw * enc->final_c * 4;
        if ((b == B_Y0 || b == B_Y1) && !enc->resid32) continue;             // fp32 residual stream: parity plan of the compressed PVRs only
        PVR_HIP_TRY(hipMalloc(&L.buf[b], bytes));
    }
    return PVR_OK;
}
static pvr_status alloc_zero_page(pvr_encoder *enc) {          // padding rows, and the all-zero bias of split-K launches (one per handle)
    PVR_HIP_TRY(hipMalloc((void **)&enc->d_zero, PVR_ZERO_BYTES));
    PVR_HIP_TRY(hipMemset(enc->d_zero, 0, PVR_ZERO_BYTES));
    return PVR_OK;
}
static void lane_free(Lane &L) {                               // whatever of the lane exists (a failed first use, pvr_encoder_destroy)
    for (void *q : L.buf) if (q) (void)hipFree(q);
    for (void *q : {(void *)L.d_img, (void *)L.d_stem, (void *)L.d_imgf, (void *)L.d_smallk}) if (q) (void)hipFree(q);
    if (L.done) (void)hipEventDestroy(L.done);
    L = Lane();
}
// The lane a forward runs on.  First use (lane 0: finalize) allocates it off the hot path, into a local Lane that enters the array only when every
// allocation succeeded (a ~3 GB workspace can fail): the other lanes are never touched, so the encoder stays usable.  The memsets run on the null
// stream and forwards on the caller's (torch's current stream need not be ordered against it), so the device is drained once here.
static pvr_status get_lane(pvr_encoder *enc, int lane, Lane **out) {
    Lane &slot = enc->lanes[lane];
    if (!slot.valid) {
        Lane L;
        pvr_status s = alloc_workspace(enc, L);
        if (!s) s = lane_smallk(enc, L);
        if (!s && hipDeviceSynchronize() != hipSuccess) { set_error("get_lane: device sync failed"); s = PVR_ERR_HIP; }
        if (s) { lane_free(L); return s; }
        if (enc->ap_out) L.ap_rows = enc->ap_out + (size_t)lane * enc->desc.chunk * 1024;
        L.valid = true;
        slot = L;
    }
    *out = &slot;
    return PVR_OK;
}

extern "C" {

pvr_status pvr_encoder_create(const pvr_encoder_desc *desc, pvr_encoder **out) {
    PVR_REQUIRE(desc && out, "pvr_encoder_create: null argument");
    PVR_REQUIRE(desc->arch >= PVR_ARCH_RESNET50 && desc->arch <= PVR_ARCH_RESNET34, "unknown arch %d", desc->arch);
    const bool resnet = desc->arch <= PVR_ARCH_RESNET50_L3 || desc->arch == PVR_ARCH_RESNET18 || desc->arch == PVR_ARCH_RESNET34;
    const bool vit_arch = desc->arch >= PVR_ARCH_CLIP_VIT_B32 && desc->arch <= PVR_ARCH_MAE_VIT_H14 && desc->arch != PVR_ARCH_RANDOM5;
    PVR_REQUIRE(desc->dtype == PVR_BF16 || desc->dtype == PVR_F16 || (stores_f32(desc->dtype) && resnet) || (desc->dtype == PVR_F32 && vit_arch),
                "dtype must be PVR_BF16 or PVR_F16 (PVR_F32 is built for the torchvision ResNet family - ResNet50, its _l3 / _l4 variants, ResNet18 / 34 - and for the "
                "CLIP ViT / MAE ViT encoders; PVR_F32S for the ResNet family only)");
    PVR_REQUIRE(desc->max_batch > 0, "max_batch must be positive");
    PVR_REQUIRE(desc->crop == 224, "crop must be 224 (reference embeddings.py:82; CLIP input_resolution 224)");
    PVR_REQUIRE(desc->resize >= desc->crop, "resize must be >= crop");
    pvr_encoder *e = new pvr_encoder();
    e->desc = *desc;
    read_switches(e->sw);
    if (e->desc.chunk <= 0 || e->desc.chunk > e->desc.max_batch) e->desc.chunk = e->desc.max_batch;
    if (e->desc.arch == PVR_ARCH_RANDOM5) {
        random5_create(e);
    } else if (e->desc.arch == PVR_ARCH_CLIP_RN50) {
        plan_encoder(e);
        resizer_create(e);
    } else if (e->desc.arch >= PVR_ARCH_CLIP_VIT_B32 && e->desc.arch <= PVR_ARCH_MAE_VIT_H14) {
        pvr_status s = vit_create(e);
        if (s) { delete e; return s; }
    } else {
        plan_encoder(e);                                        // the whole launch plan (encoder_plan.hip): finalize only prepares weights and workspace
        if (e->desc.dtype == PVR_F32S)                          // every convolution runs on conv_split16: a shape it cannot take fails here, not at launch
            for (const ConvOp &op : e->ops)
                if (!op.is_conv() || !conv_split16_supported(op.cin, op.cout, op.k)) {
                    set_error("PVR_F32S: %s (cin %d, cout %d, k %d) is not a conv_split16 shape", op.conv.c_str(), op.cin, op.cout, op.k);
                    delete e;
                    return PVR_ERR_INVALID;
                }
    }
    *out = e;
    return PVR_OK;
}

pvr_status pvr_encoder_load_weights(pvr_encoder *enc, const char *name, const float *host_data, const int64_t *shape,
                                    int32_t ndim) {
    PVR_REQUIRE(enc && name && host_data, "pvr_encoder_load_weights: null argument");
    PVR_REQUIRE(!enc->finalized, "encoder already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host_data, host_data + n);
    enc->weights[name] = std::move(t);
    return PVR_OK;
}

pvr_status pvr_encoder_set_host_backend(pvr_encoder *enc, int32_t on) {
    PVR_REQUIRE(enc, "null encoder");
    PVR_REQUIRE(!enc->finalized, "pvr_encoder_set_host_backend: call between create and finalize");
    PVR_REQUIRE(!on || enc->desc.dtype != PVR_F32S, "pvr_encoder_set_host_backend: the CPU plan is fp32; create the encoder with dtype PVR_F32, not PVR_F32S");
    enc->host = on != 0;
    if (!enc->vit && !enc->rnd) resolve_kinds(enc);             // (the switches of a host handle skip it)
    return PVR_OK;
}

pvr_status pvr_encoder_finalize(pvr_encoder *enc) {
    PVR_REQUIRE(enc, "null encoder");
    PVR_REQUIRE(!enc->finalized, "encoder already finalized");
    pvr_status s;
    if (enc->host) return host_finalize(enc);                   // CPU plan: no HIP call
    if (enc->vit || enc->rnd) {
        if ((s = enc->vit ? vit_finalize(enc) : random5_finalize(enc))) return s;
        PVR_HIP_TRY(hipDeviceSynchronize());
        enc->weights.clear();
        enc->finalized = true;
        return PVR_OK;
    }
    const bool rn50c = enc->desc.arch == PVR_ARCH_CLIP_RN50;
    if ((s = rn50c ? finalize_stem(enc, "visual.conv1.weight", "visual.bn1", 32, 3) : finalize_stem(enc))) return s;
    if (rn50c && (s = finalize_attnpool(enc))) return s;
    for (auto &op : enc->ops)
        if (op.is_conv() && (s = finalize_conv(enc, op))) return s;
    if ((s = prepare_weights(enc))) return s;
    PVR_HIP_TRY(hipDeviceSynchronize());                        // (the weight-packing launches above)
    for (auto &op : enc->ops) {
        op.h_w.clear(); op.h_w.shrink_to_fit(); op.h_b.clear(); op.h_b.shrink_to_fit();
        if (op.split16 && op.d_wf) { (void)hipFree(op.d_wf); op.d_wf = nullptr; }     // fp32 weights that were only the source of a split image
    }
    Lane *lane0;
    if ((s = get_lane(enc, 0, &lane0))) return s;               // (with the low-latency scratch when the plan was switched on before)
    if ((s = alloc_zero_page(enc))) return s;
    PVR_HIP_TRY(hipDeviceSynchronize());                        // (its memset runs on the null stream, forwards on the caller's: see get_lane)
    enc->weights.clear();                                       // host copies no longer needed
    enc->finalized = true;
    return PVR_OK;
}

int32_t pvr_encoder_out_size(const pvr_encoder *enc) { return enc ? enc->out_size : 0; }

}  // extern "C"

// One chunk of the CLIP RN50 tower: Resize(224, bicubic, antialias) + CenterCrop -> stem image -> conv1 (stem kernel) -> plan
// (convolutions and 2x2 average pools) -> attention pool (tokens, fused q/k/v GEMM, attention core, c_proj of token 0).

static pvr_status clip_rn50_chunk(pvr_encoder *enc, Lane &L, int lane, const uint8_t *fr, int nb, int h, int w, float *out, int64_t out_stride, hipStream_t st) {
    const int dt = enc->desc.dtype, crop = enc->desc.crop;
    pvr_status s;
    const uint8_t *u8; int oh, ow;
    if ((s = resizer_run(enc, lane, fr, nb, h, w, st, &u8, &oh, &ow))) return s;
    // short side == crop here, so this only centre-crops and converts to the stem's centred 4-channel image
    if ((s = launch_preprocess(u8, nb, oh, ow, enc->desc.resize, crop, L.d_img, dt, st))) return s;
    enc->last_n = nb;
    if (enc->stop_after == "pre") return PVR_OK;
    if ((s = launch_stem(L.d_img, enc->d_stem_w, enc->d_stem_b, L.d_stem, nb, crop, dt, st))) return s;
    for (const ConvOp &op : enc->ops) {
        if (op.role == R_AVGPOOL2) s = launch_avgpool2(bufp(L, op.in_buf), bufp(L, op.out_buf), nb, op.h, op.w, op.cin, dt, st);
        else s = launch_conv(enc->sw, bufp(L, op.in_buf), op.d_w, op.d_b, op.res_buf == B_NONE ? nullptr : bufp(L, op.res_buf), bufp(L, op.out_buf),
                             enc->d_zero, nb, op.h, op.w, op.cin, op.cout, op.k, op.k, op.stride, op.pad, op.relu, op.out_f32, dt, st);
        if (s) return s;
        if (!enc->stop_after.empty() && op.tap == enc->stop_after) return PVR_OK;
    }
    // AttentionPool2d(7, 2048, 32 heads, 1024)
    const int C = 2048, T = 50;
    if ((s = launch_attnpool_tokens((const float *)L.buf[B_F32], enc->ap_pos, L.buf[B_T1], nb, 49, C, dt, st))) return s;
    if ((s = launch_conv(enc->sw, L.buf[B_T1], enc->ap_wqkv, enc->ap_bqkv, nullptr, L.buf[B_X0], enc->d_zero, nb * T, 1, 1, C, 3 * C, 1, 1, 1, 0, 0, 0, dt, st))) return s;
    if ((s = launch_attention(L.buf[B_X0], L.buf[B_T2], T, C, 32, nb, dt, st))) return s;
    // c_proj of token 0 only: a 1x1 "convolution" over (n, T, 1) with stride T picks row 0 of every image; fp32 out
    float *dense = L.ap_rows;
    if ((s = launch_conv(enc->sw, L.buf[B_T2], enc->ap_wc, enc->ap_bc, nullptr, dense, enc->d_zero, nb, T, 1, C, 1024, 1, 1, T, 0, 0, 1, dt, st))) return s;
    PVR_HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * 4, dense, 1024 * 4, 1024 * 4, nb, hipMemcpyDeviceToDevice, st));
    return PVR_OK;
}

// Per-call inputs of a forward that only the instrumented entry points set
struct ForwardArgs {
    std::vector<hipEvent_t> *ev = nullptr;        // pvr_encoder_profile: one event before the first launch and one after every launch of the FIRST chunk
    int rec_first = -1, rec_last = -1;            // pvr_encoder_profile_span: only these two marks are recorded, the others are placeholders
    int *bad_flags = nullptr;                     // pvr_encoder_check_range: per-launch "output holds inf / NaN" flags of this forward
};
static pvr_status mark_launch(const ForwardArgs &fa, hipStream_t st) {
    if (fa.ev) {
        hipEvent_t e;
        PVR_HIP_TRY(hipEventCreate(&e));
        const int idx = (int)fa.ev->size();
        if (fa.rec_first < 0 || idx == fa.rec_first || idx == fa.rec_last) PVR_HIP_TRY(hipEventRecord(e, st));
        fa.ev->push_back(e);
    }
    return PVR_OK;
}

// One chunk of the reference-precision plans: integer transforms (exact, via the bf16 image) -> fp32 /255, Normalize ->
// fp32 conv1 -> fp32 maxpool -> fp32 implicit-GEMM convs -> fp32 pool / flatten.  PVR_F32: every product on the f32-input MFMA;
// PVR_F32S: the same launches with every product as the exact split product on the 16-bit MFMA (the normalised image zero-bordered for stem_split16)
static pvr_status f32_chunk(pvr_encoder *enc, Lane &L, const uint8_t *fr, int nb, int h, int w, float *out, int64_t out_stride, hipStream_t st, const ForwardArgs &fa) {
    const int dt = enc->desc.dtype;
    pvr_status s;
    auto mark = [&] { return mark_launch(fa, st); };
    const int crop = enc->desc.crop;
    const bool split = dt == PVR_F32S;
    if ((s = launch_preprocess(fr, nb, h, w, enc->desc.resize, crop, L.d_img, PVR_BF16, st, enc->crop_pos))) return s;
    if ((s = launch_normalize_nhwc4(L.d_img, L.d_imgf, nb, crop, enc->desc.mean, enc->desc.std_, PVR_BF16, st, split))) return s;
    if ((s = mark())) return s;
    if (split) s = launch_stem_split16(L.d_imgf, enc->d_stem_w, enc->d_stem_b, (float *)L.d_stem, nb, crop, st);
    else s = launch_stem_f32(L.d_imgf, enc->d_stem_wf, enc->d_stem_b, (float *)L.d_stem, nb, crop, st);
    if (s) return s;
    if (fa.bad_flags) launch_range_flag_split(L.d_stem, (size_t)nb * 112 * 112 * 64, fa.bad_flags, (int)enc->sched_plain.size(), st);   // (check_range: PVR_F32S only)
    if ((s = mark())) return s;
    if ((s = launch_maxpool_f32((const float *)L.d_stem, (float *)L.buf[B_X0], nb, 112, 112, 64, st))) return s;
    if ((s = mark())) return s;
    enc->last_n = nb;
    for (auto &op : enc->ops) {
        const float *res = op.res_buf == B_NONE ? nullptr : (const float *)L.buf[op.res_buf];
        if (split) s = launch_conv_split16((const float *)L.buf[op.in_buf], op.d_wsp, op.d_b, res, (float *)L.buf[op.out_buf], nb,
                                           op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, op.relu, st);
        else s = launch_conv_f32((const float *)L.buf[op.in_buf], op.d_wf, op.d_b, res, (float *)L.buf[op.out_buf], nb,
                                 op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, op.relu, st);
        if (s) return s;
        if (fa.bad_flags)                   // pvr_encoder_check_range: the launch's output, all of it
            launch_range_flag_split(L.buf[op.out_buf], (size_t)nb * op.ho() * op.wo() * op.cout, fa.bad_flags, (int)(&op - enc->ops.data()), st);
        if ((s = mark())) return s;
    }
    if (pooled_head(enc))
        s = launch_avgpool(L.buf[B_F32], out, out_stride, nb, enc->final_hw, enc->final_c, 1, dt, st);
    else
        s = launch_nhwc_to_chw((const float *)L.buf[B_F32], out, out_stride, nb, enc->final_hw, enc->final_c,
                               enc->final_creal, st);
    if (s) return s;
    return mark();
}

// One chunk of the 16-bit plans (ResNet50 family).  stopped: a debug stop (pvr_encoder_debug_stop_after) ended it - the forward ends there too
static pvr_status h16_chunk(pvr_encoder *enc, Lane &L, const uint8_t *fr, int nb, int h, int w, float *out, int64_t out_stride, hipStream_t st, const ForwardArgs &fa,
                            bool &stopped) {
    const int dt = enc->desc.dtype;
    pvr_status s;
    auto mark = [&] { return mark_launch(fa, st); };
    // frames that need no resize (the bench configuration: 256 x 256 frames, Resize(256) is the identity): the fused stem reads the
    // uint8 frames itself - no preprocess launch, no padded 16-bit image in HBM
    int fused_u8 = 0;
    // layer1.0.conv1 has no launch in the fused schedule (encoder_plan.hip: plan_stem_c1): the stem's register-pooling form runs it
    const bool c1_pending = enc->fuse && enc->stem_c1 >= 0;
    const bool c1_in_stem = c1_pending && enc->stop_after.empty() && stem_conv1_capable(enc->sw);
    if (enc->sw.stem_u8 && enc->sw.stem_lds && enc->stop_after.empty() && enc->desc.crop == 224 && enc->crop_pos >= 0 && enc->crop_pos <= 4) {
        int rn = 1, top = 0, left = 0;
        preprocess_geometry(h, w, enc->desc.resize, enc->desc.crop, enc->crop_pos, &rn, &top, &left);
        if (!rn && stem_pool_u8_ok(fr, h, w, top, left)) {
            if ((s = mark())) return s;                  // (launch index of the preprocess stays: pvr_encoder_profile)
            if ((s = launch_stem_pool_u8(enc->sw, fr, nb, h, w, top, left, enc->d_stem_w, enc->d_stem_b, L.buf[B_X0], dt, st, c1_in_stem ? enc->d_stem_c1w : nullptr,
                                         c1_in_stem ? enc->ops[enc->stem_c1].d_b : nullptr, c1_in_stem ? L.buf[B_T1] : nullptr, enc->stem_c1_blk))) return s;
            fused_u8 = 1;
        }
    }
    if (!fused_u8) {
        if ((s = launch_preprocess(fr, nb, h, w, enc->desc.resize, enc->desc.crop, L.d_img, dt, st, enc->crop_pos))) return s;
        if ((s = mark())) return s;
    }
    enc->last_n = nb;
    if (enc->stop_after == "pre") { stopped = true; return PVR_OK; }
    if (enc->stop_after == "stem") {             // debug tap of the un-pooled conv1 output: unfused kernel
        if ((s = launch_stem(L.d_img, enc->d_stem_w, enc->d_stem_b, L.d_stem, nb, enc->desc.crop, dt, st))) return s;
        stopped = true;
        return PVR_OK;
    }
    // conv1 + bn1 + relu + maxpool fused: the 112x112x64 activation stays in LDS
    if (!fused_u8 && (s = launch_stem_pool(enc->sw, L.d_img, enc->d_stem_w, enc->d_stem_b, L.buf[B_X0], nb, enc->desc.crop, dt, st, c1_in_stem ? enc->d_stem_c1w : nullptr,
                                           c1_in_stem ? enc->ops[enc->stem_c1].d_b : nullptr, c1_in_stem ? L.buf[B_T1] : nullptr, enc->stem_c1_blk))) return s;
    if (fa.bad_flags) {                      // pvr_encoder_check_range: the pooled stem output (flag slot behind the plan's launches)
        const size_t n8 = (size_t)nb * 56 * 56 * 64 / 8;
        hipLaunchKernelGGL(range_flag_kernel<false>, dim3(2048), dim3(256), 0, st, L.buf[B_X0], n8, dt, fa.bad_flags, (int)cur_plan(enc).size());
    }
    if ((s = mark())) return s;
    if ((s = mark())) return s;                  // (keeps the launch indices of pvr_encoder_profile stable)
    if (enc->stop_after == "pool") { stopped = true; return PVR_OK; }
    bool t1_blocked = false;                     // t1_blocked: the conv1 launch in front of layer1's first tail wrote t1 in the blocked layout
    if (c1_in_stem) t1_blocked = enc->stem_c1_blk != 0;
    else if (c1_pending && enc->stop_after != "pool") {
        // ... or, where that stem form did not run (debug stops, PVR_STEM_REGPOOL=0, PVR_STEM_LDS=0), as its own launch in front of the plan - blocked t1 when the tail wants it
        const ConvOp &c1 = enc->ops[enc->stem_c1];
        if (enc->stem_c1_blk && enc->sw.conv_algo == -1 && conv_expand_supported(enc->sw, (int64_t)nb * c1.h * c1.w, c1.h, c1.w, c1.cin, c1.cout, 1, 1, 1, 0, c1.relu, 0, false)) {
            s = launch_conv_expand(L.buf[c1.in_buf], c1.d_w, c1.d_b, nullptr, L.buf[c1.out_buf], nb, c1.h, c1.w, c1.cin, c1.cout, 1, c1.relu, dt, st, 1);
            t1_blocked = true;
        } else
            s = launch_conv(enc->sw, L.buf[c1.in_buf], c1.d_w, c1.d_b, nullptr, L.buf[c1.out_buf], enc->d_zero, nb, c1.h, c1.w, c1.cin, c1.cout, 1, 1, 1, 0, c1.relu, 0, dt, st);
        if (s) return s;
    }
    bool pooled = false;                         // the plan's last convolution wrote the average pool itself (conv_wfrag's pooled form)
    const std::vector<Launch> &plan_ = cur_plan(enc);
    const uint8_t *kinds = enc->kinds.data() + (size_t)(nb - 1) * plan_.size();
    float *smallk = L.d_smallk;
    // the pooled epilogue stores 16-byte pieces of the caller's rows: a property of this call's arguments, not of the plan
    const bool pool_args_ok = enc->stop_after.empty() && out_stride % 4 == 0 && ((size_t)out & 15) == 0;
    int launch_idx = 0;                          // debug: stop_after = "#k" ends the forward after conv launch k of the plan
    const bool run_ok = enc->stop_after.empty() && !fa.bad_flags;
    const int stop_idx = enc->stop_after.size() > 1 && enc->stop_after[0] == '#' ? atoi(enc->stop_after.c_str() + 1) : -1;
    // a member convolution of a launch that runs as its members (small forwards): split-K in the low-latency plan, else the shape's kernel
    auto member = [&](const ConvOp &o, const void *in, const void *r_, void *out_) -> pvr_status {
        if (const int ks = small_batch_ksplit(enc, o, nb)) {
            if (!smallk) { set_error("low-latency plan without its scratch (pvr_encoder_set_low_latency allocates it)"); return PVR_ERR_STATE; }
            return launch_conv_splitk(in, o.d_w, o.d_b, r_, out_, enc->d_zero, smallk, ks, nb, o.h, o.w, o.cin, o.cout, o.k, o.k, o.stride, o.pad, o.relu, o.out_f32, dt, st);
        }
        return launch_conv(enc->sw, in, o.d_w, o.d_b, r_, out_, enc->d_zero, nb, o.h, o.w, o.cin, o.cout, o.k, o.k, o.stride, o.pad, o.relu, o.out_f32, dt, st);
    };
    for (size_t li = 0; li < plan_.size(); ++li) {
        const Launch &l = plan_[li];
        const ConvOp &op = enc->ops[l.out_op()];
        const void *res = op.res_buf == B_NONE ? nullptr : L.buf[op.res_buf];
        int kind = kinds[li];
        if (kind == LK_WFRAG_POOL && !pool_args_ok) kind = resolve_kind(enc, plan_, li, nb, false);
        if ((kind == LK_FRAME_RUN || kind == LK_FRAME_RUN_TAIL) && !run_ok) kind = LK_FRAME_FRONT1;     // (taps, debug stops, range validation: one launch per bottleneck)
        if (kind == LK_CHAIN_YS2 && !run_ok) kind = LK_CHAIN;                                           // (... and all of y)
        if (kind == LK_CONV_YS2 && !run_ok) kind = LK_CONV;
        switch (kind) {
        case LK_FRAME_RUN: {
            BFBlk blks[6];
            int nblk = 0;
            for (size_t t = li; t < plan_.size() && nblk < 6 && (t == li || kinds[t] == LK_FRAME_RUN_TAIL); ++t, ++nblk) {
                const Launch &lt = plan_[t];
                const ConvOp &o3 = enc->ops[lt.conv3], &o2 = enc->ops[lt.conv2], &o1 = enc->ops[lt.conv1];
                blks[nblk] = BFBlk{(const u16 *)o1.d_wfb, (const u16 *)o2.d_wfb, (const u16 *)o3.d_wfb, (const u16 *)L.buf[o3.res_buf], o1.d_b, o2.d_b, o3.d_b,
                                   (u16 *)L.buf[o3.out_buf]};
            }
            s = launch_bneck_frame_run(blks, nblk, nb, dt, st, enc->sw.frame_stagger);
            break;
        }
        case LK_FRAME_RUN_TAIL:
            s = PVR_OK;                                   // (inside the run's launch)
            break;
        case LK_FRAME_FRONT1: {
            const ConvOp &c2 = enc->ops[l.conv2], &cf = enc->ops[l.conv1];
            s = launch_bneck_frame(enc->sw, nullptr, c2.d_wfb, c2.d_b, op.d_wfb, op.d_b, res, L.buf[op.out_buf], nullptr, nb, 3 | 8, dt, st,
                                   nullptr, nullptr, nullptr, nullptr, cf.d_wfb, cf.d_b);
            break;
        }
        case LK_FRAME: {
            const ConvOp &c2 = enc->ops[l.conv2];
            const ConvOp *c1 = l.next1 >= 0 ? &enc->ops[l.next1] : nullptr;
            s = launch_bneck_frame(enc->sw, L.buf[l.t1_in], c2.d_wfb, c2.d_b, op.d_wfb, op.d_b, res, L.buf[op.out_buf], nullptr, nb, c1 ? 7 : 3, dt, st,
                                   nullptr, c1 ? c1->d_wfb : nullptr, c1 ? c1->d_b : nullptr, c1 ? L.buf[l.t1_out] : nullptr);
            break;
        }
        case LK_FRAME_MEMBERS: {
            // t2 goes to the t1 buffer this launch does not read
            const ConvOp &c2 = enc->ops[l.conv2];
            const ConvOp *c1 = l.next1 >= 0 ? &enc->ops[l.next1] : nullptr;
            const ConvOp *cf = l.conv1 >= 0 ? &enc->ops[l.conv1] : nullptr;
            const int t2b = l.t1_in == B_T1 ? B_T2 : B_T1;
            s = PVR_OK;
            if (cf) s = member(*cf, L.buf[cf->in_buf], nullptr, L.buf[l.t1_in]);
            if (!s) s = member(c2, L.buf[l.t1_in], nullptr, L.buf[t2b]);
            if (!s) s = member(op, L.buf[t2b], res, L.buf[op.out_buf]);
            if (!s && c1) s = member(*c1, L.buf[op.out_buf], nullptr, L.buf[l.t1_out]);
            break;
        }
        case LK_DUAL: {
            // conv3 & downsample as one two-operand launch (layer3.0 / layer4.0)
            const ConvOp &cd = enc->ops[l.ds];
            s = launch_conv_pp256(enc->sw, L.buf[op.in_buf], op.d_wcat, op.d_bsum, nullptr, L.buf[op.out_buf], nb, op.h, op.w, op.cin, op.cout, 1, 1, 1, 0,
                                  op.relu, 0, 0, dt, 224, st, L.buf[cd.in_buf], cd.h, cd.w, cd.cin, cd.stride);
            break;
        }
        case LK_DUAL_MEMBERS: {
            const ConvOp &cd = enc->ops[l.ds];
            s = member(cd, L.buf[cd.in_buf], nullptr, L.buf[cd.out_buf]);
            if (!s) s = member(op, L.buf[op.in_buf], res, L.buf[op.out_buf]);
            break;
        }
        case LK_CHAIN:
        case LK_CHAIN_YS2: {
            const ConvOp &c2 = enc->ops[l.conv2];
            const ConvOp *c1 = l.next1 >= 0 ? &enc->ops[l.next1] : nullptr;
            const ConvOp *cd = l.ds >= 0 ? &enc->ops[l.ds] : nullptr;
            s = launch_bottleneck_chain(enc->sw, L.buf[l.t1_in], c2.d_w, c2.d_b, op.d_wp, cd ? op.d_bsum : op.d_b, res, L.buf[op.out_buf],
                                        c1 ? c1->d_wp : nullptr, c1 ? c1->d_b : nullptr, c1 ? L.buf[l.t1_out] : nullptr, nb,
                                        c2.h, c2.w, c2.cout, c1 ? c1->cout : 0, c2.stride, dt, st,
                                        cd ? L.buf[cd->in_buf] : nullptr, cd ? cd->d_wp : nullptr, op.d_wpb, cd ? cd->d_wpb : nullptr,
                                        l.wave, cd ? (l.in_blk && t1_blocked) : l.in_blk, l.out_blk, kind == LK_CHAIN_YS2);
            t1_blocked = false;
            break;
        }
        case LK_CONV_YS2:
            // the 1 x 1 stride-2 reader of a y_s2 tail: stride 1 over the (n, h / 2, w / 2, cin) tensor in the front of the same buffer
            s = launch_conv_expand(L.buf[op.in_buf], op.d_w, op.d_b, nullptr, L.buf[op.out_buf], nb, op.h / 2, op.w / 2, op.cin, op.cout, 1, op.relu, dt, st);
            break;
        case LK_CAST:
            s = launch_f32_to_h((const float *)L.buf[op.in_buf], L.buf[op.out_buf], (size_t)nb * op.h * op.w * op.cin, dt, st);
            break;
        case LK_F32:
            s = launch_conv_f32((const float *)L.buf[op.in_buf], op.d_wf, op.d_b, (const float *)res, (float *)L.buf[op.out_buf], nb,
                                op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, op.relu, st);
            break;
        case LK_SPLIT16:
            s = launch_conv_split16((const float *)L.buf[op.in_buf], op.d_wsp, op.d_b, (const float *)res, (float *)L.buf[op.out_buf], nb,
                                    op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, op.relu, st);
            break;
        case LK_SPLIT16_PAIR: {
            const ConvOp &od = enc->ops[l.pair];
            s = launch_conv_split16((const float *)L.buf[op.in_buf], op.d_wsp_pair, op.d_b_pair, nullptr, (float *)L.buf[op.out_buf], nb, op.h, op.w, op.cin,
                                    128, op.k, op.stride, op.pad, 1, st, (float *)L.buf[od.out_buf], 64);
            break;
        }
        case LK_SPLIT16_IN32:
            // a 16-bit convolution whose operand is the fp32 residual stream (rounded to f16 in the kernel's staging pass): t1 leaves 16-bit, a downsample fp32
            s = launch_conv_split16((const float *)L.buf[op.in_buf], op.d_wsp, op.d_b, nullptr, (op.out_f32 & 1) ? (float *)L.buf[op.out_buf] : nullptr, nb,
                                    op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, op.relu, st, nullptr, 0, (op.out_f32 & 1) ? nullptr : L.buf[op.out_buf], 1);
            break;
        case LK_SPLITK_SMALL:
            // low-latency plan: the few pixel tiles of a <= 4-frame forward share each K loop between `ks` blocks
            s = member(op, L.buf[op.in_buf], res, L.buf[op.out_buf]);
            break;
        case LK_SPLITK:
            s = launch_conv_splitk(L.buf[op.in_buf], op.d_w, op.d_b, res, L.buf[op.out_buf], enc->d_zero, (float *)L.buf[op.ks_buf],
                                   op.ksplit, nb, op.h, op.w, op.cin, op.cout, op.k, op.k, op.stride, op.pad, op.relu, op.out_f32, dt, st);
            break;
        case LK_EXPAND_BLOCKED:
            // layer1.0.conv1 in front of a wave-form tail: t1 in the blocked layout
            s = launch_conv_expand(L.buf[op.in_buf], op.d_w, op.d_b, nullptr, L.buf[op.out_buf], nb, op.h, op.w, op.cin, op.cout, 1, op.relu, dt, st, 1);
            t1_blocked = true;
            break;
        case LK_WFRAG_POOL:
            // the trunk's last conv3 + identity + ReLU with AdaptiveAvgPool2d(1) in its epilogue: the (n,7,7,2048) fp32 activation is never written
            s = launch_conv_wfrag(enc->sw, L.buf[op.in_buf], op.d_wfb, op.d_b, res, nullptr, nb, op.h, op.w, op.cin, op.cout, 1, 1, 1, 0, 1, 1, dt, st,
                                  out, out_stride);
            pooled = true;
            break;
        case LK_WFRAG:
            // few pixels, deep K (layer4 at batch 256): 112 x 256 tiles, weights as L2 fragments
            s = launch_conv_wfrag(enc->sw, L.buf[op.in_buf], op.d_wfb, op.d_b, res, L.buf[op.out_buf], nb, op.h, op.w, op.cin, op.cout, op.k, op.k,
                                  op.stride, op.pad, op.relu, op.out_f32, dt, st);
            break;
        default:
            s = launch_conv(enc->sw, L.buf[op.in_buf], op.d_w, op.d_b, res, L.buf[op.out_buf], enc->d_zero, nb, op.h, op.w,
                            op.cin, op.cout, op.k, op.k, op.stride, op.pad, op.relu, op.out_f32, dt, st);
        }
        if (s) return s;
        if (fa.bad_flags && kind != LK_WFRAG_POOL) {         // pvr_encoder_check_range: the launch's output, all of it
            const size_t n8 = (size_t)nb * op.ho() * op.wo() * op.cout / 8;
            const int blocks = (int)((n8 + 255) / 256 < 2048 ? (n8 + 255) / 256 : 2048);
            if ((op.out_f32 & 1) || op.f32op) hipLaunchKernelGGL(range_flag_kernel<true>, dim3(blocks), dim3(256), 0, st, L.buf[op.out_buf], n8, dt, fa.bad_flags, (int)li);
            else hipLaunchKernelGGL(range_flag_kernel<false>, dim3(blocks), dim3(256), 0, st, L.buf[op.out_buf], n8, dt, fa.bad_flags, (int)li);
        }
        if ((s = mark())) return s;
        if (!enc->stop_after.empty() && op.tap == enc->stop_after) { stopped = true; break; }
        if (launch_idx++ == stop_idx) { stopped = true; break; }
    }
    enc->last_pooled = pooled;
    if (stopped) return PVR_OK;
    if (pooled)
        s = PVR_OK;                               // (the last launch wrote the pooled rows)
    else if (pooled_head(enc))
        s = launch_avgpool(L.buf[B_F32], out, out_stride, nb, enc->final_hw, enc->final_c, 1, dt, st);
    else
        s = launch_nhwc_to_chw((const float *)L.buf[B_F32], out, out_stride, nb, enc->final_hw, enc->final_c,
                               enc->final_creal, st);
    if (s) return s;
    return mark();
}

static pvr_status forward_impl(pvr_encoder *enc, int lane, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                               int64_t out_stride, void *hip_stream, const ForwardArgs &fa) {
    PVR_REQUIRE(enc && frames && out, "pvr_encoder_forward: null argument");
    if (!enc->finalized) { set_error("encoder not finalized"); return PVR_ERR_STATE; }
    PVR_REQUIRE(n > 0 && n <= enc->desc.max_batch, "n=%d outside 1..max_batch=%d", n, enc->desc.max_batch);
    PVR_REQUIRE(out_stride >= enc->out_size, "out_stride %lld < out_size %d", (long long)out_stride, enc->out_size);
    hipStream_t st = (hipStream_t)hip_stream;
    pvr_status s;
    if (enc->rnd) return random5_forward(enc, frames, n, h, w, out, out_stride, st);
    enc->last_lane = lane;
    if (enc->vit) return vit_forward(enc, lane, frames, n, h, w, out, out_stride, st);
    Lane *L;
    if ((s = get_lane(enc, lane, &L))) return s;
    ForwardArgs ca = fa;                             // (events: the first chunk only)
    for (int f0 = 0; f0 < n; f0 += enc->desc.chunk, ca.ev = nullptr) {
        const int nb = (n - f0 < enc->desc.chunk) ? n - f0 : enc->desc.chunk;
        const uint8_t *fr = frames + (size_t)f0 * h * w * 3;
        float *o = out + (size_t)f0 * out_stride;
        bool stopped = false;
        if ((s = mark_launch(ca, st))) return s;
        if (stores_f32(enc->desc.dtype)) s = f32_chunk(enc, *L, fr, nb, h, w, o, out_stride, st, ca);
        else if (enc->desc.arch == PVR_ARCH_CLIP_RN50) s = clip_rn50_chunk(enc, *L, lane, fr, nb, h, w, o, out_stride, st);
        else s = h16_chunk(enc, *L, fr, nb, h, w, o, out_stride, st, ca, stopped);
        if (s || stopped) return s;
    }
    return PVR_OK;
}

// Same-lane forwards issued on DIFFERENT streams are ordered here, not by the caller: every forward records the lane's event on its
// stream and the next forward on that lane waits for it first (a device-side event wait, no host synchronisation), so a lane's
// workspace is never shared by two forwards in flight.  Different lanes stay independent.
static pvr_status lane_wait(pvr_encoder *enc, int lane, void *hip_stream) {
    const Lane &L = enc->lanes[lane];
    hipStream_t st = (hipStream_t)hip_stream;
    if (L.done && L.stream != st) PVR_HIP_TRY(hipStreamWaitEvent(st, L.done, 0));
    return PVR_OK;
}
static pvr_status lane_mark(pvr_encoder *enc, int lane, void *hip_stream) {
    Lane &L = enc->lanes[lane];
    hipStream_t st = (hipStream_t)hip_stream;
    if (!L.done) PVR_HIP_TRY(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    PVR_HIP_TRY(hipEventRecord(L.done, st));
    L.stream = st;
    return PVR_OK;
}
static pvr_status lane_forward(pvr_encoder *enc, int lane, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                               int64_t out_stride, void *hip_stream) {
    if (!enc->finalized) { set_error("encoder not finalized"); return PVR_ERR_STATE; }
    PVR_REQUIRE(lane == 0 || !enc->rnd, "pvr_encoder_forward_lane: the 'random' PVR plan has a single workspace");
    pvr_status s = lane_wait(enc, lane, hip_stream);
    if (!s) s = forward_impl(enc, lane, frames, n, h, w, out, out_stride, hip_stream, ForwardArgs());
    if (!s) s = lane_mark(enc, lane, hip_stream);
    return s;
}

extern "C" {

#define PVR_NO_HOST(enc_, what_) PVR_REQUIRE(!((enc_) && (enc_)->host), what_ ": not available on a host-backend encoder")

pvr_status pvr_encoder_forward(pvr_encoder *enc, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                               int64_t out_stride, void *hip_stream) {
    if (enc && enc->host) {
        PVR_REQUIRE(enc->finalized, "encoder not finalized");
        PVR_REQUIRE(n <= enc->desc.max_batch, "n=%d exceeds max_batch=%d", n, enc->desc.max_batch);
        return host_forward(enc, frames, n, h, w, out, out_stride);
    }
    PVR_REQUIRE(enc, "pvr_encoder_forward: null encoder");
    TraceScope trace("pvr_encoder_forward");
    return lane_forward(enc, 0, frames, n, h, w, out, out_stride, hip_stream);
}

pvr_status pvr_encoder_forward_lane(pvr_encoder *enc, int32_t lane, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                                    int64_t out_stride, void *hip_stream) {
    if (enc && enc->host) return pvr_encoder_forward(enc, frames, n, h, w, out, out_stride, hip_stream);
    PVR_REQUIRE(enc, "pvr_encoder_forward_lane: null encoder");
    TraceScope trace(lane == 0 ? "pvr_encoder_forward_lane 0" : "pvr_encoder_forward_lane 1+");
    PVR_REQUIRE(lane >= 0 && lane < PVR_MAX_LANES, "pvr_encoder_forward_lane: lane must be 0..%d", PVR_MAX_LANES - 1);
    return lane_forward(enc, lane, frames, n, h, w, out, out_stride, hip_stream);
}

// Instrumented forward of ONE chunk: HIP events between launches on the caller's stream (synchronises).
// op_ms[i] = duration of launch i, op_flops[i] = its algorithmic FLOPs (2*M*K_real*Cout_real; 0 for byte kernels),
// launch order: preprocess, stem, maxpool, conv ops..., pool/flatten.
pvr_status pvr_encoder_profile(pvr_encoder *enc, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                               int64_t out_stride, void *hip_stream, float *op_ms, double *op_flops, int32_t cap,
                               int32_t *n_ops) {
    PVR_REQUIRE(enc && op_ms && op_flops && n_ops, "pvr_encoder_profile: null argument");
    PVR_NO_HOST(enc, "pvr_encoder_profile");
    PVR_REQUIRE(n <= enc->desc.chunk, "profile: n=%d must fit one chunk (%d)", n, enc->desc.chunk);
    std::vector<hipEvent_t> ev;
    ForwardArgs fa;
    fa.ev = &ev;
    pvr_status s = lane_wait(enc, 0, hip_stream);
    if (!s) s = forward_impl(enc, 0, frames, n, h, w, out, out_stride, hip_stream, fa);
    if (!s && hipStreamSynchronize((hipStream_t)hip_stream) != hipSuccess) { set_error("profile: sync failed"); s = PVR_ERR_HIP; }
    const int nl = (int)ev.size() - 1;
    if (!s && nl > cap) { set_error("profile: %d launches > cap %d", nl, cap); s = PVR_ERR_INVALID; }
    if (!s) {
        for (int i = 0; i < nl; ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            op_ms[i] = ms;
            op_flops[i] = 0.0;
        }
        // stem: 118.0 MMAC/frame = 112*112*64*147
        if (nl > 1) op_flops[1] = 2.0 * n * 112.0 * 112.0 * 64.0 * 147.0;
        if (nl > 1 && enc->fuse && enc->stem_c1 >= 0 && !stores_f32(enc->desc.dtype)) op_flops[1] += 2.0 * n * 56.0 * 56.0 * 64.0 * 64.0;   // layer1.0.conv1 runs inside the stem
        int i = 3;
        auto flops = [&](int oi) {
            if (oi < 0) return 0.0;
            const ConvOp &op = enc->ops[oi];
            return 2.0 * n * op.ho() * op.ho() * (double)op.cout_real * op.k * op.k * op.cin_real;
        };
        for (const Launch &l : cur_plan(enc)) {
            if (i >= nl) break;
            op_flops[i++] = flops(l.conv1) + flops(l.conv2) + flops(l.conv3) + flops(l.next1) + flops(l.ds) + flops(l.pair);
        }
        *n_ops = nl;
    }
    for (auto e : ev) (void)hipEventDestroy(e);
    return s;
}

// Time from the start of launch first_op to the end of launch last_op (indices as pvr_encoder_profile reports them) of ONE forward that
// carries only those two events: an event between two launches costs a few microseconds of dispatch serialisation, so the sum of
// pvr_encoder_profile's per-launch durations overstates a family of 38 launches by ~4 % against rocprofv3's kernel durations.
pvr_status pvr_encoder_profile_span(pvr_encoder *enc, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out, int64_t out_stride,
                                    void *hip_stream, int32_t first_op, int32_t last_op, float *span_ms) {
    PVR_REQUIRE(enc && span_ms, "pvr_encoder_profile_span: null argument");
    PVR_NO_HOST(enc, "pvr_encoder_profile_span");
    PVR_REQUIRE(n <= enc->desc.chunk, "profile: n=%d must fit one chunk (%d)", n, enc->desc.chunk);
    PVR_REQUIRE(first_op >= 0 && last_op >= first_op, "pvr_encoder_profile_span: bad launch range %d..%d", first_op, last_op);
    std::vector<hipEvent_t> ev;
    ForwardArgs fa;
    fa.ev = &ev; fa.rec_first = first_op; fa.rec_last = last_op + 1;
    pvr_status s = lane_wait(enc, 0, hip_stream);
    if (!s) s = forward_impl(enc, 0, frames, n, h, w, out, out_stride, hip_stream, fa);
    if (!s && hipStreamSynchronize((hipStream_t)hip_stream) != hipSuccess) { set_error("profile: sync failed"); s = PVR_ERR_HIP; }
    if (!s && last_op + 1 >= (int)ev.size()) { set_error("profile_span: launch %d past the plan's %d launches", last_op, (int)ev.size() - 1); s = PVR_ERR_INVALID; }
    if (!s && hipEventElapsedTime(span_ms, ev[first_op], ev[last_op + 1]) != hipSuccess) { set_error("profile_span: elapsed time failed"); s = PVR_ERR_HIP; }
    for (auto e : ev) (void)hipEventDestroy(e);
    return s;
}

pvr_status pvr_encoder_set_crop_position(pvr_encoder *enc, int32_t pos) {
    PVR_REQUIRE(enc, "null encoder");
    PVR_REQUIRE(pos >= 0 && pos <= 4, "crop position %d outside 0..4", pos);
    PVR_REQUIRE(pos == 0 || (!enc->vit && !enc->rnd && enc->desc.arch != PVR_ARCH_CLIP_RN50), "corner crops are built for the ResNet50 family only");
    enc->crop_pos = pos;
    return PVR_OK;
}

pvr_status pvr_encoder_set_low_latency(pvr_encoder *enc, int32_t on) {
    PVR_REQUIRE(enc, "null encoder");
    enc->low_latency = on != 0;
    if (enc->vit || enc->rnd || enc->host) return PVR_OK;
    resolve_kinds(enc);
    if (!enc->finalized) return PVR_OK;                         // (finalize allocates when the plan was asked for earlier)
    return ensure_smallk(enc);                                  // the plan's split-K scratch, here and not in a forward
}

pvr_status pvr_encoder_debug_set_fusion(pvr_encoder *enc, int32_t on) {
    PVR_REQUIRE(enc, "null encoder");
    enc->fuse = on != 0;
    if (!enc->vit && !enc->rnd && !enc->host) resolve_kinds(enc);
    return PVR_OK;
}

// The switches of a finalized encoder that do not shape its plan (PlanSwitches, "live"): pool_fuse, stem_u8, frame_min_n, frame_run, frame_stagger,
// conv_algo, stem_regpool.  The A/B tests flip them between two forwards of ONE handle; everything else is fixed by the environment at
// pvr_encoder_create.
pvr_status pvr_encoder_debug_set_switch(pvr_encoder *enc, const char *name, int32_t value) {
    PVR_REQUIRE(enc && name, "pvr_encoder_debug_set_switch: null argument");
    const std::string nm = name;
    if (nm == "pool_fuse") enc->sw.pool_fuse = value;
    else if (nm == "stem_u8") enc->sw.stem_u8 = value;
    else if (nm == "frame_min_n") enc->sw.frame_min_n = value;
    else if (nm == "frame_run") enc->sw.frame_run = value;
    else if (nm == "frame_stagger") enc->sw.frame_stagger = value;
    else if (nm == "conv_algo") enc->sw.conv_algo = value;
    else if (nm == "stem_regpool") enc->sw.stem_regpool = value;
    else {
        set_error("pvr_encoder_debug_set_switch: '%s' is not a live switch (pool_fuse, stem_u8, frame_min_n, frame_run, frame_stagger, conv_algo, "
                  "stem_regpool); plan switches are read from the environment at create", name);
        return PVR_ERR_INVALID;
    }
    if (!enc->vit && !enc->rnd && !enc->host) resolve_kinds(enc);
    return PVR_OK;
}

// Range validation of the 16-bit storage types (f16: 5 exponent bits).  A non-finite EMBEDDING is caught by the callers' finite check, but an activation that
// overflows INSIDE the network need not reach the output: +inf times a negative weight is -inf, -inf or NaN through fmaxf(v, 0) is 0 - a wrong, finite
// embedding.  This runs ONE forward of the unfused plan (every convolution's output exists in HBM and is bit-identical to what the fused launches compute
// internally) and checks every launch's output for inf / NaN; *first_bad = index of the first such launch (pvr_encoder_launch_name's numbering of the
// UNFUSED plan, 3 = the first convolution) or -1.  Synchronises; allocates and frees its flag buffer: a load-time check, not part of the forward path.
pvr_status pvr_encoder_check_range(pvr_encoder *enc, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out, int64_t out_stride, void *hip_stream,
                                   int32_t *first_bad) {
    PVR_REQUIRE(enc && frames && out && first_bad, "pvr_encoder_check_range: null argument");
    PVR_NO_HOST(enc, "pvr_encoder_check_range");
    PVR_REQUIRE(enc->finalized && !enc->vit && !enc->rnd && enc->desc.arch != PVR_ARCH_CLIP_RN50 && enc->desc.dtype != PVR_F32,
                "pvr_encoder_check_range: built for the 16-bit and PVR_F32S plans of the torchvision ResNet family (PVR_F32 has the full fp32 range)");
    PVR_REQUIRE(n > 0 && n <= enc->desc.chunk, "pvr_encoder_check_range: n=%d must fit one chunk (%d)", n, enc->desc.chunk);
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t nl = enc->sched_plain.size();
    pvr_status s = lane_wait(enc, 0, hip_stream);
    if (s) return s;
    int *flags = nullptr;
    PVR_HIP_TRY(hipMalloc((void **)&flags, (nl + 1) * sizeof(int)));
    if (hipMemsetAsync(flags, 0, (nl + 1) * sizeof(int), st) != hipSuccess) { (void)hipFree(flags); set_error("check_range: memset failed"); return PVR_ERR_HIP; }
    const bool fuse0 = enc->fuse;
    enc->fuse = false; resolve_kinds(enc);
    ForwardArgs fa;
    fa.bad_flags = flags;
    s = forward_impl(enc, 0, frames, n, h, w, out, out_stride, hip_stream, fa);
    enc->fuse = fuse0; resolve_kinds(enc);
    std::vector<int> hf(nl + 1, 0);
    if (!s && hipMemcpyAsync(hf.data(), flags, (nl + 1) * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) { set_error("check_range: copy failed"); s = PVR_ERR_HIP; }
    if (!s && hipStreamSynchronize(st) != hipSuccess) { set_error("check_range: sync failed"); s = PVR_ERR_HIP; }
    (void)hipFree(flags);
    if (s) return s;
    *first_bad = hf[nl] ? 1 : -1;                               // 1 = "stem" (conv1 + bn1 + relu + maxpool)
    for (size_t i = 0; i < nl && *first_bad < 0; ++i) if (hf[i]) *first_bad = (int32_t)i + 3;
    return lane_mark(enc, 0, hip_stream);
}

pvr_status pvr_encoder_debug_stop_after(pvr_encoder *enc, const char *tap) {
    PVR_REQUIRE(enc, "null encoder");
    enc->stop_after = tap ? tap : "";
    return PVR_OK;
}

pvr_status pvr_encoder_tap(pvr_encoder *enc, const char *name, float *out, int64_t cap, int64_t *count, void *hip_stream) {
    PVR_REQUIRE(enc && name && out && count, "pvr_encoder_tap: null argument");
    PVR_NO_HOST(enc, "pvr_encoder_tap");
    if (!enc->finalized || enc->last_n == 0) { set_error("no forward has run"); return PVR_ERR_STATE; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (enc->vit) return vit_tap(enc, name, out, cap, count, st);
    const int n = enc->last_n, crop = enc->desc.crop;
    const Lane &L = enc->lanes[enc->last_lane];
    const std::string nm = name;
    const void *src = nullptr;
    size_t elems = 0;
    int f32 = 0;
    if (nm == "pre") { src = L.d_img; elems = (size_t)n * (crop + 6) * (crop + 8) * 4; }
    else if (nm == "stem") { src = L.d_stem; elems = (size_t)n * 112 * 112 * 64; }
    else if (nm == "pool") { src = L.buf[B_X0]; elems = (size_t)n * 56 * 56 * 64; }
    else if (nm.compare(0, 3, "buf") == 0 && nm.find(':') != std::string::npos) {   // debug: "buf<b>:<elems>" = raw workspace buffer b
        const int b = atoi(nm.c_str() + 3);
        PVR_REQUIRE(b >= 0 && b < B_F32, "tap %s: 16-bit workspace buffers are 0..%d", name, B_F32 - 1);
        src = L.buf[b]; elems = (size_t)atoll(nm.c_str() + nm.find(':') + 1);
    } else {
        auto it = enc->taps.find(nm);
        PVR_REQUIRE(it != enc->taps.end(), "unknown tap %s", name);
        // taps alias ping-pong buffers: only the LAST layer's tap is guaranteed intact after a full forward - and not even that one when
        // the forward pooled inside its last convolution (conv_wfrag's pooled form: the (n,7,7,2048) activation was never written)
        const auto &g = it->second.second;
        if (it->second.first == B_F32 && enc->last_pooled) {
            set_error("tap %s: the last forward averaged inside its last convolution and never wrote this activation; run the forward with "
                      "pvr_encoder_debug_stop_after(enc, \"%s\") or pvr_encoder_debug_set_switch(enc, \"pool_fuse\", 0) first", name, name);
            return PVR_ERR_STATE;
        }
        src = L.buf[it->second.first];
        elems = (size_t)n * g[0] * g[1] * g[2];
        f32 = g[3];
    }
    PVR_REQUIRE((int64_t)elems <= cap, "tap %s needs %zu elements, cap %lld", name, elems, (long long)cap);
    *count = (int64_t)elems;
    const bool img16 = nm == "pre";                     // the transformed image stays 16-bit in every mode
    if (f32 || (stores_f32(enc->desc.dtype) && !img16)) {
        PVR_HIP_TRY(hipMemcpyAsync(out, src, elems * 4, hipMemcpyDeviceToDevice, st));
        return PVR_OK;
    }
    return launch_h_to_f32(src, out, elems, stores_f32(enc->desc.dtype) ? PVR_BF16 : enc->desc.dtype, st);
}

void pvr_encoder_destroy(pvr_encoder *enc) {
    if (!enc) return;
    if (enc->hplan) host_destroy(enc);
    if (enc->vit) vit_destroy(enc);
    if (enc->rnd) random5_destroy(enc);
    for (auto &op : enc->ops) { if (op.d_w) (void)hipFree(op.d_w); if (op.d_wp) (void)hipFree(op.d_wp); if (op.d_wpb) (void)hipFree(op.d_wpb); if (op.d_wfb) (void)hipFree(op.d_wfb); if (op.d_wcat) (void)hipFree(op.d_wcat); if (op.d_wf) (void)hipFree(op.d_wf); if (op.d_wsp) (void)hipFree(op.d_wsp); if (op.d_wsp_pair) (void)hipFree(op.d_wsp_pair); if (op.d_b_pair) (void)hipFree(op.d_b_pair); if (op.d_b) (void)hipFree(op.d_b); if (op.d_bsum) (void)hipFree(op.d_bsum); }
    if (enc->d_stem_wf) (void)hipFree(enc->d_stem_wf);
    if (enc->d_stem_c1w) (void)hipFree(enc->d_stem_c1w);
    for (Lane &L : enc->lanes) lane_free(L);
    if (enc->d_stem_w) (void)hipFree(enc->d_stem_w);
    if (enc->d_stem_b) (void)hipFree(enc->d_stem_b);
    if (enc->d_zero) (void)hipFree(enc->d_zero);
    resizer_destroy(enc);
    for (void *q : {(void *)enc->ap_wqkv, (void *)enc->ap_wc, (void *)enc->ap_bqkv, (void *)enc->ap_bc, (void *)enc->ap_pos, (void *)enc->ap_out}) if (q) (void)hipFree(q);
    delete enc;
}

}  // extern "C"
