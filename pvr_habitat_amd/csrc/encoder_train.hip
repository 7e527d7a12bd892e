// Trainable ResNet encoder (include/pvr_train.h): EmbeddingNet(..., train=True) of the reference (src/embeddings.py:323-326, :396-398) for the torchvision
// trunks resnet18 / 34 / 50 in fp32.  The executor walks plan_encoder's op list (convolution + BN [+ residual] [+ ReLU], the in_buf / out_buf / res_buf
// dataflow f32_chunk walks) with ONE saved pre-BN and one post-BN tensor per op instead of the reused workspace buffers, and walks it backwards for the
// gradients.  The device code of the backward pass is train_kernels.hip; every product of a convolution, data gradient or weight gradient runs on the
// f32-input MFMA (conv_f32.hip / conv_wgrad_kernel), BatchNorm statistics are two-pass, and every split reduction is summed in a fixed order.
// pvr_trainer_set_wgrad_split16 moves the weight gradients, and nothing else, to the exact-split f16 products of wgrad_split16.hip;
// pvr_trainer_set_conv_split16 moves the forward convolutions and the data gradients of layer1 .. layer4 to those of conv_split16_scaled.hip.
// pvr_trainer_set_train_from makes conv1 / bn1 and the layers below a stage a frozen prefix: eval-mode BatchNorm, tensors from a liveness pool, in fp32
// one fused launch per op (conv_f32.hip: launch_conv_bn_frozen_f32), and a backward that stops at the first trained op.
#include "encoder_internal.h"
#include "train_internal.h"
#include "../../include/pvr_train.h"

namespace {

struct Slot {
    std::string name;
    int64_t off, numel, shape[4];
};

struct TrainOp {
    std::string conv, bn;
    int in_src = -3, res_src = -2;              // producer of the input / residual: op index, -1 the max pool's output, -2 none
    int h, w, cin, cout, k, stride, pad, relu, ho, wo;
    int64_t w_off, g_off, b_off, rm_off, rv_off, nbt_off;   // params (floats) / buffer block (4-byte slots)
    float *z = nullptr, *y = nullptr, *dy = nullptr, *mean = nullptr, *rstd = nullptr;
};

struct Timed {
    std::string name;
    double flops;
    float ms;
};

struct EventPair {
    hipEvent_t e0, e1;
};

}  // namespace

struct pvr_trainer {
    pvr_encoder_desc desc;
    int out_size = 0, final_hw = 0, final_c = 0;
    TrainOp stem;                                // conv1 / bn1 (7x7 / 2 on the NHWC4 image; in_src unused)
    std::vector<TrainOp> ops;
    std::vector<Slot> params, buffers;
    int64_t n_params = 0, n_buf_slots = 0;
    // device (made by the first forward, sized for max_batch)
    void *arena = nullptr;
    u16 *d_img = nullptr;
    float *d_imgf = nullptr, *pool = nullptr, *dpool = nullptr, *dz = nullptr, *dil = nullptr, *wpack = nullptr, *stem_wpack = nullptr, *wg_scratch = nullptr,
          *bn_scratch = nullptr, *zero_bias = nullptr;
    int64_t wg_floats = 0, bn_floats = 0;
    int fwd_n = 0;                               // frames of the forward whose activations are held (0: none - a backward is PVR_ERR_STATE)
    bool bn_frozen = false;                      // BatchNorm normalises with its running statistics (pvr_trainer_set_bn_frozen)
    bool wgrad_split16 = false;                  // weight gradients as exact-split f16 products (pvr_trainer_set_wgrad_split16); fixed once the arena exists
    bool conv_split16 = false;                   // forward convolutions and data gradients of the op list as exact-split f16 products
                                                 // (pvr_trainer_set_conv_split16); fixed once the arena exists
    float *scales = nullptr;                     // split modes: one absmax scale per saved tensor (index src + 1), the image (ops + 1), dz (ops + 2),
                                                 // then pvr_op_absmax_scale_pair's four aux words (zeroed with the workspace); conv_split16: one more
                                                 // slot behind them, the scale of the weights of the convolution at hand
    int train_from = 0;                          // pvr_trainer_set_train_from: 0 everything trains; s: layer{s} .. layer4 train, conv1 / bn1 and the ops
    int first_trained = 0;                       // [0, first_trained) are the frozen prefix; fixed once the arena exists
    int prefix_ops() const { return train_from > 0 ? first_trained : 0; }
    bool in_prefix(int src) const { return train_from > 0 && src < first_trained; }       // (src: an op index, or -1 the max pool's output)
    size_t scale_slots() const { return ops.size() + 3 + 4 + (conv_split16 ? 1 : 0); }
    int boundary_src = -2;                       // train_from > 0: the ONE prefix tensor a trained op reads (an op index, or -1 the max pool's output)
    float *ext_boundary = nullptr;               // pvr_trainer_forward_boundary: the caller's memory the held forward's boundary tensor lives in (else the arena's)
    bool prefix_fused = false;                   // pvr_trainer_set_prefix_fused: with conv_split16 a prefix op is scale + ONE launch, no z; fixed once the arena exists
    bool fused_prefix() const { return prefix_fused && conv_split16 && train_from > 0; }
    bool timing = false;
    std::vector<Timed> times;                    // launch i of a step is bracketed by events[i]
    std::vector<EventPair> events;               // made once each, on demand; destroyed with the trainer (no error path leaves one behind)
};

namespace {

constexpr int S_IMG = 224;

int64_t add_slot(std::vector<Slot> &v, int64_t &total, const std::string &name, std::initializer_list<int64_t> shape, int64_t slots_per_elem = 1) {
    Slot s;
    s.name = name; s.off = total; s.numel = 1;
    int i = 0;
    for (int64_t d : shape) { s.shape[i++] = d; s.numel *= d; }
    for (; i < 4; ++i) s.shape[i] = 0;
    total += s.numel * slots_per_elem;
    v.push_back(s);
    return s.off;
}

void add_params(pvr_trainer *t, TrainOp &op) {
    op.w_off = add_slot(t->params, t->n_params, op.conv + ".weight", {op.cout, op.cin == 4 ? 3 : op.cin, op.k, op.k});
    op.g_off = add_slot(t->params, t->n_params, op.bn + ".weight", {op.cout});
    op.b_off = add_slot(t->params, t->n_params, op.bn + ".bias", {op.cout});
    op.rm_off = add_slot(t->buffers, t->n_buf_slots, op.bn + ".running_mean", {op.cout});
    op.rv_off = add_slot(t->buffers, t->n_buf_slots, op.bn + ".running_var", {op.cout});
}

size_t out_elems(const TrainOp &op, int n) { return (size_t)n * op.ho * op.wo * op.cout; }

struct Carver {                                  // sizes, then pointers, of one arena (256-byte aligned pieces)
    char *base = nullptr;
    size_t used = 0;
    template <typename T> void take(T **p, size_t count) {
        if (base) *p = (T *)(base + used);
        used += (count * sizeof(T) + 255) / 256 * 256;
    }
};

// The frozen prefix (train_from > 0) keeps no tensor but what a trained op reads.  Its z / y tensors (and the max pool's output) come from a small pool of
// buffers assigned by liveness over in_src / res_src: a tensor's buffer is free again after its last consumer has run; a tensor a trained op reads (the
// boundary tensor) gets a piece of its own.  Prefix ops get no dy and no mean / rstd slots, and no z where the op is one fused launch.
void carve_prefix(pvr_trainer *t, Carver &c) {
    const int B = t->desc.max_batch, P = t->first_trained;
    const bool need_z = t->conv_split16 && !t->prefix_fused;      // (fp32, or prefix_fused: a prefix op is ONE launch, convolution + BatchNorm, and has no z)
    std::vector<int> last(P + 1, -1);             // last consumer (op index) of tensor src (index src + 1)
    for (int i = 0; i < (int)t->ops.size(); ++i) {
        const TrainOp &op = t->ops[i];
        if (op.in_src < P) last[op.in_src + 1] = i;
        if (op.res_src != -2 && op.res_src < P) last[op.res_src + 1] = i;
    }
    struct Buf { size_t cap; bool busy; };
    std::vector<Buf> bufs;
    std::vector<std::pair<float **, int>> uses;   // (pointer to set, buffer)
    auto get = [&](float **p, size_t need) {      // the smallest free buffer that holds `need`, else the largest free one (grown), else a new one
        int best = -1;
        for (int b = 0; b < (int)bufs.size(); ++b)
            if (!bufs[b].busy && bufs[b].cap >= need && (best < 0 || bufs[b].cap < bufs[best].cap)) best = b;
        if (best < 0)
            for (int b = 0; b < (int)bufs.size(); ++b)
                if (!bufs[b].busy && (best < 0 || bufs[b].cap > bufs[best].cap)) best = b;
        if (best < 0) { bufs.push_back(Buf{need, false}); best = (int)bufs.size() - 1; }
        bufs[best].cap = std::max(bufs[best].cap, need);
        bufs[best].busy = true;
        uses.push_back({p, best});
        return best;
    };
    std::vector<int> held(P + 1, -1);             // buffer of tensor src (index src + 1); -1: a piece of its own
    TrainOp &sm = t->stem;
    sm.dy = sm.mean = sm.rstd = nullptr;
    const int sz = get(&sm.z, out_elems(sm, B)), sy = get(&sm.y, out_elems(sm, B));
    if (last[0] >= P) c.take(&t->pool, (size_t)B * 56 * 56 * 64);
    else held[0] = get(&t->pool, (size_t)B * 56 * 56 * 64);
    bufs[sz].busy = bufs[sy].busy = false;
    for (int i = 0; i < P; ++i) {
        TrainOp &op = t->ops[i];
        op.z = op.dy = op.mean = op.rstd = nullptr;
        const int zb = need_z ? get(&op.z, out_elems(op, B)) : -1;
        if (last[i + 1] >= P) c.take(&op.y, out_elems(op, B));
        else held[i + 1] = get(&op.y, out_elems(op, B));
        if (zb >= 0) bufs[zb].busy = false;
        for (int s = 0; s <= i + 1; ++s)           // (a tensor nobody reads - there is none - is free at once)
            if (held[s] >= 0 && last[s] <= i) { bufs[held[s]].busy = false; held[s] = -1; }
    }
    std::vector<float *> ptr(bufs.size(), nullptr);
    for (size_t b = 0; b < bufs.size(); ++b) c.take(&ptr[b], bufs[b].cap);
    if (c.base)
        for (auto &u : uses) *u.first = ptr[u.second];
}

void carve(pvr_trainer *t, Carver &c) {
    const int B = t->desc.max_batch, P = t->prefix_ops();
    const bool part = t->train_from > 0;          // (off: not a byte of the workspace changes)
    c.take(&t->d_img, (size_t)B * (S_IMG + 6) * (S_IMG + 8) * 4);
    c.take(&t->d_imgf, (size_t)B * S_IMG * S_IMG * 4);
    size_t dz_max = part ? 1 : out_elems(t->stem, B), dil_max = 1, w_max = 1;
    int64_t wg_max = part ? 1 : pvr_op_stem_wgrad_scratch_floats(B, S_IMG), bn_max = part ? 1 : pvr_op_bn_scratch_floats((int64_t)B * t->stem.ho * t->stem.wo, 64);
    int c_max = 64;
    auto take_op = [&](TrainOp &op) {
        c.take(&op.z, out_elems(op, B));
        c.take(&op.y, out_elems(op, B));
        c.take(&op.dy, out_elems(op, B));
        c.take(&op.mean, op.cout);
        c.take(&op.rstd, op.cout);
    };
    if (part) carve_prefix(t, c);
    else {
        take_op(t->stem);
        c.take(&t->pool, (size_t)B * 56 * 56 * 64);
        c.take(&t->dpool, (size_t)B * 56 * 56 * 64);
    }
    for (int i = 0; i < (int)t->ops.size(); ++i) {
        TrainOp &op = t->ops[i];
        if (i < P) {                              // a prefix op: its weights are packed and its channels take the zero bias; nothing of a backward
            w_max = std::max(w_max, (size_t)std::max((op.cout + 63) / 64 * 64 * op.cin, (op.cin + 63) / 64 * 64 * op.cout) * op.k * op.k);
            c_max = std::max(c_max, std::max(op.cin, op.cout));
            continue;
        }
        take_op(op);
        dz_max = std::max(dz_max, out_elems(op, B));
        if (op.stride == 2 && !t->in_prefix(op.in_src)) dil_max = std::max(dil_max, (size_t)B * op.h * op.w * op.cout);
        w_max = std::max(w_max, (size_t)std::max((op.cout + 63) / 64 * 64 * op.cin, (op.cin + 63) / 64 * 64 * op.cout) * op.k * op.k);
        for (int n = 1; n <= B; ++n)               // (the number of pixel ranges is not monotone in the batch: the range length is rounded to 32)
            wg_max = std::max(wg_max, pvr_op_conv_wgrad_scratch_floats(n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad));
        if (t->wgrad_split16)
            for (int n = 1; n <= B; ++n)
                wg_max = std::max(wg_max, pvr_op_conv_wgrad_split16_scratch_floats(n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad));
        bn_max = std::max(bn_max, pvr_op_bn_scratch_floats((int64_t)B * op.ho * op.wo, op.cout));
        c_max = std::max(c_max, std::max(op.cin, op.cout));
    }
    c.take(&t->dz, dz_max);
    c.take(&t->dil, dil_max);
    c.take(&t->wpack, w_max);
    c.take(&t->stem_wpack, (size_t)64 * 49 * 4);
    if (t->wgrad_split16 && !part) wg_max = std::max(wg_max, pvr_op_stem_wgrad_split16_scratch_floats(B, S_IMG));
    // (both modes off: not a byte of the workspace changes.  The split weights of conv_split16 take wpack as they are: two f16 per value)
    if (t->wgrad_split16 || t->conv_split16) c.take(&t->scales, t->scale_slots());
    c.take(&t->wg_scratch, (size_t)wg_max);
    c.take(&t->bn_scratch, (size_t)bn_max);
    c.take(&t->zero_bias, (size_t)c_max);
    t->wg_floats = wg_max; t->bn_floats = bn_max;
}

// first forward: the whole workspace as one allocation; the image's zero border and the zero bias are written once, here (null stream: drained before
// the caller's stream goes on, as encoder.hip: get_lane)
pvr_status ensure_workspace(pvr_trainer *t) {
    if (t->arena) return PVR_OK;
    Carver size;
    carve(t, size);
    void *a = nullptr;
    PVR_HIP_TRY(hipMalloc(&a, size.used));
    Carver c;
    c.base = (char *)a;
    carve(t, c);
    const size_t img_bytes = (size_t)t->desc.max_batch * (S_IMG + 6) * (S_IMG + 8) * 4 * 2;
    const size_t zero_bytes = (size_t)((char *)a + size.used - (char *)t->zero_bias);      // (the arena's last piece)
    if (hipMemset(t->d_img, 0, img_bytes) != hipSuccess || hipMemset(t->zero_bias, 0, zero_bytes) != hipSuccess ||
        (t->scales && hipMemset(t->scales, 0, t->scale_slots() * sizeof(float)) != hipSuccess) || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(a);
        set_error("pvr_trainer: workspace initialisation failed");
        return PVR_ERR_HIP;
    }
    t->arena = a;
    return PVR_OK;
}

struct Tick {                                    // per-launch timing: an event pair around every launch when pvr_trainer_debug_set_timing is on
    pvr_trainer *t;
    hipStream_t st;
    pvr_status begin(const std::string &name, double flops) {
        if (!t->timing) return PVR_OK;
        const size_t i = t->times.size();
        if (i == t->events.size()) {
            EventPair p;
            PVR_HIP_TRY(hipEventCreate(&p.e0));
            if (hipEventCreate(&p.e1) != hipSuccess) {
                (void)hipEventDestroy(p.e0);
                set_error("pvr_trainer: hipEventCreate failed");
                return PVR_ERR_HIP;
            }
            t->events.push_back(p);
        }
        PVR_HIP_TRY(hipEventRecord(t->events[i].e0, st));
        t->times.push_back(Timed{name, flops, 0.f});
        return PVR_OK;
    }
    pvr_status end() {
        if (!t->timing) return PVR_OK;
        PVR_HIP_TRY(hipEventRecord(t->events[t->times.size() - 1].e1, st));
        return PVR_OK;
    }
};
pvr_status collect_times(pvr_trainer *t, size_t from, hipStream_t st) {
    if (!t->timing) return PVR_OK;
    PVR_HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = from; i < t->times.size(); ++i)
        PVR_HIP_TRY(hipEventElapsedTime(&t->times[i].ms, t->events[i].e0, t->events[i].e1));
    return PVR_OK;
}

#define TR_RUN(name_, flops_, call_)                \
    do {                                            \
        if ((s = tick.begin(name_, flops_))) return s; \
        if ((s = (call_))) return s;                \
        if ((s = tick.end())) return s;             \
    } while (0)

pvr_status memset_floats(float *p, int64_t count, hipStream_t st) {
    PVR_HIP_TRY(hipMemsetAsync(p, 0, (size_t)count * sizeof(float), st));
    return PVR_OK;
}

// tensor `src` of the forward at hand: the caller's memory for the boundary tensor of a pvr_trainer_forward_boundary pass, else the arena's piece
float *tensor_of(const pvr_trainer *t, int src) {
    if (t->ext_boundary && src == t->boundary_src) return t->ext_boundary;
    return src == -1 ? t->pool : t->ops[src].y;
}
float *grad_of(pvr_trainer *t, int src) { return src == -1 ? t->dpool : t->ops[src].dy; }

}  // namespace

extern "C" {

pvr_status pvr_trainer_create(const pvr_encoder_desc *desc, pvr_trainer **out) {
    PVR_REQUIRE(desc && out, "pvr_trainer_create: null argument");
    const char *scope = "trainable encoders: the torchvision ResNet trunks resnet18 / resnet34 / resnet50 (arch PVR_ARCH_RESNET18 / _RESNET34 / _RESNET50) "
                        "with dtype PVR_F32";
    PVR_REQUIRE(desc->arch == PVR_ARCH_RESNET50 || desc->arch == PVR_ARCH_RESNET18 || desc->arch == PVR_ARCH_RESNET34,
                "pvr_trainer_create: arch %d is not trainable (%s; the compressed *_l3 / *_l4 variants, CLIP, MAE and 'random' run frozen)", desc->arch, scope);
    PVR_REQUIRE(desc->dtype == PVR_F32, "pvr_trainer_create: dtype %d is not trainable (%s: fp32 storage, every product on the f32-input MFMA)", desc->dtype, scope);
    PVR_REQUIRE(desc->crop == S_IMG, "pvr_trainer_create: crop %d: the trainer's stem, workspace and pools are built for the %d-pixel crop of the reference's "
                "transforms", desc->crop, S_IMG);
    pvr_encoder_desc d = *desc;
    d.chunk = 0;                                  // batch statistics cannot be chunked: a forward is one pass over all its frames
    pvr_encoder *enc = nullptr;
    pvr_status s = pvr_encoder_create(&d, &enc);  // plans the op list from the desc alone (encoder_plan.hip); no weights, no device
    if (s) return s;
    pvr_trainer *t = new pvr_trainer();
    t->desc = d;
    t->out_size = enc->out_size; t->final_hw = enc->final_hw; t->final_c = enc->final_c;
    TrainOp &st = t->stem;
    st.conv = "conv1"; st.bn = "bn1";
    st.h = st.w = S_IMG; st.cin = 4; st.cout = 64; st.k = 7; st.stride = 2; st.pad = 3; st.relu = 1; st.ho = st.wo = S_IMG / 2;
    add_params(t, st);
    int writer[B_COUNT + 1];
    for (int &x : writer) x = -3;
    writer[B_X0] = -1;                            // the max pool's output
    bool ok = true;
    for (const ConvOp &op : enc->ops) {
        TrainOp o;
        o.conv = op.conv; o.bn = op.bn;
        o.h = op.h; o.w = op.w; o.cin = op.cin; o.cout = op.cout; o.k = op.k; o.stride = op.stride; o.pad = op.pad; o.relu = op.relu;
        o.ho = op.ho(); o.wo = op.wo();
        o.in_src = writer[op.in_buf];
        o.res_src = op.res_buf == B_NONE ? -2 : writer[op.res_buf];
        ok = ok && op.is_conv() && o.in_src >= -1 && o.res_src >= -2 && op.cin % 32 == 0 && op.cout % 64 == 0 && (op.k == 1 || op.k == 3) &&
             (op.stride == 1 || (op.stride == 2 && op.h % 2 == 0 && op.w % 2 == 0)) && op.pad == op.k / 2 && op.cin == op.cin_real && op.cout == op.cout_real;
        writer[op.out_buf] = (int)t->ops.size();
        add_params(t, o);
        t->ops.push_back(o);
    }
    pvr_encoder_destroy(enc);
    if (!ok || t->ops.empty()) {
        delete t;
        set_error("pvr_trainer_create: the plan of arch %d holds an operation the trainer has no backward for", desc->arch);
        return PVR_ERR_INVALID;
    }
    // the convolution launches address an operand with 32-bit byte offsets (conv_f32: "operand larger than 2 GiB"), and no kernel of the trainer has run
    // on a larger tensor: refuse, here and by name, a max_batch at which a tensor of the workspace (an activation, its gradient, the zero-filled grid
    // of a stride-2 data gradient) would pass 2 GiB, instead of failing inside the first forward or backward
    int64_t per_frame = std::max((int64_t)S_IMG * S_IMG * 4, (int64_t)st.ho * st.wo * st.cout);
    for (const TrainOp &o : t->ops)
        per_frame = std::max(per_frame, std::max((int64_t)o.h * o.w * std::max(o.cin, o.stride == 2 ? o.cout : 0), (int64_t)o.ho * o.wo * o.cout));
    const int64_t frames_max = (0x7ffffff0ll - 1) / (per_frame * 4);
    if (d.max_batch > frames_max) {
        delete t;
        set_error("pvr_trainer_create: max_batch %d: the largest tensor of this trunk's training workspace takes %.1f MB per frame and a launch addresses at "
                  "most 2 GiB of one: the largest max_batch is %lld frames", d.max_batch, per_frame * 4 / 1048576.0, (long long)frames_max);
        return PVR_ERR_INVALID;
    }
    if (t->n_buf_slots & 1) ++t->n_buf_slots;     // (never: every BatchNorm adds 2 c slots) the int64 counters are 8-byte aligned
    st.nbt_off = add_slot(t->buffers, t->n_buf_slots, st.bn + ".num_batches_tracked", {1}, 2);
    for (TrainOp &o : t->ops) o.nbt_off = add_slot(t->buffers, t->n_buf_slots, o.bn + ".num_batches_tracked", {1}, 2);
    *out = t;
    return PVR_OK;
}

void pvr_trainer_destroy(pvr_trainer *t) {
    if (!t) return;
    if (t->arena) (void)hipFree(t->arena);
    for (EventPair &p : t->events) {
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    delete t;
}

int32_t pvr_trainer_out_size(const pvr_trainer *t) { return t ? t->out_size : 0; }
int64_t pvr_trainer_param_count(const pvr_trainer *t) { return t ? t->n_params : 0; }
int64_t pvr_trainer_buffer_count(const pvr_trainer *t) { return t ? t->n_buf_slots : 0; }

int64_t pvr_trainer_workspace_bytes(const pvr_trainer *t) {
    if (!t) return 0;
    pvr_trainer sizing = *t;                      // (carve also notes the scratch sizes on its handle: size a copy, never its device pointers)
    sizing.arena = nullptr;
    Carver c;
    carve(&sizing, c);
    return (int64_t)c.used;
}

int32_t pvr_trainer_param_name(const pvr_trainer *t, int32_t index, char *buf, int32_t cap) {
    if (!t || index < 0 || index >= (int32_t)t->params.size() || !buf || cap <= 0) return 0;
    snprintf(buf, (size_t)cap, "%s", t->params[index].name.c_str());
    return (int32_t)t->params[index].name.size();
}

static int64_t slot_offset(const std::vector<Slot> &v, const char *name, int64_t *numel, int64_t *shape) {
    if (!name) return -1;
    for (const Slot &s : v)
        if (s.name == name) {
            if (numel) *numel = s.numel;
            if (shape) for (int i = 0; i < 4; ++i) shape[i] = s.shape[i];
            return s.off;
        }
    return -1;
}
int64_t pvr_trainer_param_offset(const pvr_trainer *t, const char *name, int64_t *numel, int64_t *shape) {
    return t ? slot_offset(t->params, name, numel, shape) : -1;
}
int64_t pvr_trainer_buffer_offset(const pvr_trainer *t, const char *name, int64_t *numel) { return t ? slot_offset(t->buffers, name, numel, nullptr) : -1; }

pvr_status pvr_trainer_debug_set_timing(pvr_trainer *t, int32_t on) {
    PVR_REQUIRE(t, "null trainer");
    t->timing = on != 0;
    t->times.clear();
    return PVR_OK;
}
int32_t pvr_trainer_launch_time(const pvr_trainer *t, int32_t index, char *name, int32_t cap, float *ms, double *flops) {
    if (!t || index < 0 || index >= (int32_t)t->times.size()) return 0;
    const Timed &x = t->times[index];
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s", x.name.c_str());
    if (ms) *ms = x.ms;
    if (flops) *flops = x.flops;
    return (int32_t)x.name.size();
}

}  // extern "C"

namespace {

// pvr_trainer_forward (boundary == nullptr) and pvr_trainer_forward_boundary: the arguments have passed the callers' checks.  boundary: where this pass's
// boundary tensor lives instead of the arena's piece - the producing launch writes it there and every reader goes through tensor_of.  reuse: it holds the
// tensor already, and the pass starts at the first trained op.  prefix_only (pvr_trainer_prefix_forward): the pass ends behind the last prefix op - the
// same launches up to there, nothing written but the boundary tensor and the prefix's own buffers, and no forward is held.  windows
// (pvr_trainer_forward_windows): n x (top, left) on the device - the image is each frame's window instead of the centre crop, made by one launch.
// color, gray_sums (pvr_trainer_forward_augmented, with windows): n x (float b, c, s, int32 order) and n uint32 of the caller's scratch - the window's
// uint8 values are colour-jittered before /255 and Normalize, by two launches in place of that one.  rects (pvr_trainer_forward_rects, without windows):
// n x (top, left, height, width) on the device - the image is each frame's own rectangle resized to crop x crop (no Resize before it), by one launch, or
// with color by the two colour launches reading that source.  blur, staged (pvr_trainer_forward_staged, with windows or rects): n x (float sigma, int32
// gray) and (n, crop, crop, 4) uint8 of the caller's scratch - the source's uint8 values (after the colour ops, with color) are staged and then grayed,
// blurred and normalised per frame: "stage image" and "blur normalize" stand where the image launch stood, behind "colour stats" with color.
pvr_status forward_pass(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *boundary, bool reuse,
                        float *out, int64_t out_stride, void *stream, bool prefix_only = false, const int32_t *windows = nullptr, const void *color = nullptr,
                        uint32_t *gray_sums = nullptr, const int32_t *rects = nullptr, const void *blur = nullptr, void *staged = nullptr) {
    hipStream_t st = (hipStream_t)stream;
    pvr_status s;
    if ((s = ensure_workspace(t))) return s;
    t->fwd_n = 0;                                 // the held activations are being overwritten
    t->ext_boundary = boundary;
    if (t->timing) t->times.clear();
    Tick tick{t, st};
    float *bufs = (float *)bn_buffers;
    const int P = t->prefix_ops();
    const bool part = t->train_from > 0;
    auto bn = [&](TrainOp &op, const float *res, int64_t rows, bool prefix, float *y_prefix = nullptr) {
        if (prefix)                               // a frozen module in eval: running statistics whatever the handle's BatchNorm mode; nothing kept for a backward
            return launch_bn_frozen_apply(op.z, res, params + op.g_off, params + op.b_off, bufs + op.rm_off, bufs + op.rv_off, y_prefix ? y_prefix : op.y, nullptr,
                                          nullptr, rows, op.cout, op.relu, st);
        if (t->bn_frozen)                         // running statistics, read only: neither they nor num_batches_tracked are touched
            return pvr_op_bn_frozen_forward(op.z, res, params + op.g_off, params + op.b_off, bufs + op.rm_off, bufs + op.rv_off, op.y, op.mean, op.rstd, rows,
                                            op.cout, op.relu, st);
        return pvr_op_bn_train_forward(op.z, res, params + op.g_off, params + op.b_off, bufs + op.rm_off, bufs + op.rv_off, (int64_t *)(bufs + op.nbt_off), op.y,
                                       op.mean, op.rstd, rows, op.cout, op.relu, t->bn_scratch, t->bn_floats, st);
    };
    if (!reuse) {
        if (blur) {                               // grayscale and blur per frame: the uint8 image is staged, then filtered and normalised
            if (color)
                TR_RUN("colour stats", 0,
                       launch_staged_color_stats(frames, n, h, w, t->desc.resize, t->desc.crop, windows, rects, color, gray_sums, staged, st));
            TR_RUN("stage image", 0, launch_stage_image(frames, n, h, w, t->desc.resize, t->desc.crop, windows, rects, color, gray_sums, staged, st));
            TR_RUN("blur normalize", 0, launch_blur_normalize(staged, n, t->desc.crop, t->desc.mean, t->desc.std_, blur, t->d_imgf, st));
        } else if (rects && color) {              // a random resized crop and a colour jitter per frame: the colour pair on the rectangle's pixels
            TR_RUN("colour stats", 0, launch_color_stage_rects(0, frames, n, h, w, t->desc.crop, t->desc.mean, t->desc.std_, rects, color, gray_sums, t->d_imgf, st));
            TR_RUN("preprocess colour", 0,
                   launch_color_stage_rects(1, frames, n, h, w, t->desc.crop, t->desc.mean, t->desc.std_, rects, color, gray_sums, t->d_imgf, st));
        } else if (rects) {                       // a random resized crop per frame: the frame's rectangle resized to the crop, /255 and Normalize
            TR_RUN("preprocess rects", 0, launch_preprocess_rects(frames, n, h, w, t->desc.crop, t->desc.mean, t->desc.std_, rects, t->d_imgf, st));
        } else if (windows && color) {                   // a window and a colour jitter per frame: the gray sums contrast needs, then the image
            TR_RUN("colour stats", 0, launch_color_stage(0, frames, n, h, w, t->desc.resize, t->desc.crop, t->desc.mean, t->desc.std_, windows, color, gray_sums,
                                                         t->d_imgf, st));
            TR_RUN("preprocess colour", 0, launch_color_stage(1, frames, n, h, w, t->desc.resize, t->desc.crop, t->desc.mean, t->desc.std_, windows, color,
                                                              gray_sums, t->d_imgf, st));
        } else if (windows) {                     // a window per frame: the same d_imgf bits as the two launches below at that window
            TR_RUN("preprocess windows", 0,
                   launch_preprocess_windows(frames, n, h, w, t->desc.resize, t->desc.crop, t->desc.mean, t->desc.std_, windows, t->d_imgf, st));
        } else {
            TR_RUN("preprocess", 0, launch_preprocess(frames, n, h, w, t->desc.resize, t->desc.crop, t->d_img, PVR_BF16, st, 0));
            TR_RUN("normalize", 0, launch_normalize_nhwc4(t->d_img, t->d_imgf, n, t->desc.crop, t->desc.mean, t->desc.std_, PVR_BF16, st, false));
        }
        TrainOp &sm = t->stem;
        TR_RUN("conv1 pack", 0, launch_pack_stem_weights(params + sm.w_off, t->stem_wpack, st));
        TR_RUN("conv1", 2.0 * n * 112 * 112 * 64 * 147, launch_stem_f32(t->d_imgf, t->stem_wpack, nullptr, sm.z, n, S_IMG, st, true));
        TR_RUN("bn1", 0, bn(sm, nullptr, (int64_t)n * 112 * 112, part));
        TR_RUN("maxpool", 0, launch_maxpool_f32(sm.y, tensor_of(t, -1), n, 112, 112, 64, st));
    }
    // conv_split16: a tensor's scale is computed once per forward, in the launch of its first consumer, next to that convolution's weight scale; the
    // slots stay valid for the backward (the saved activations do not change)
    std::vector<char> scaled(t->ops.size() + 1, 0);
    float *w_scale = t->conv_split16 ? t->scales + t->ops.size() + 7 : nullptr;
    uint32_t *scale_aux = t->conv_split16 ? (uint32_t *)(t->scales + t->ops.size() + 3) : nullptr;
    const bool fused = t->fused_prefix();
    const int end = prefix_only ? P : (int)t->ops.size();
    for (int i = reuse ? P : 0; i < end; ++i) {
        TrainOp &op = t->ops[i];
        const int64_t rows = (int64_t)n * op.ho * op.wo;
        float *y = tensor_of(t, i);               // (op.y, or the caller's memory when this op writes the boundary tensor)
        if (t->conv_split16) {
            const float *x = tensor_of(t, op.in_src);
            float *x_scale = t->scales + op.in_src + 1;
            const bool first = !scaled[op.in_src + 1];
            TR_RUN(op.conv + " scale", 0,
                   pvr_op_absmax_scale_pair(params + op.w_off, (int64_t)op.cout * op.cin * op.k * op.k, w_scale, first ? x : nullptr,
                                            (int64_t)n * op.h * op.w * op.cin, first ? x_scale : nullptr, scale_aux, st));
            scaled[op.in_src + 1] = 1;
            if (fused && i < P) {                 // a frozen prefix op: the split convolution with the frozen BatchNorm in its epilogue, no z
                TR_RUN(op.conv + " split16 bn frozen", 2.0 * rows * op.cout * op.cin * op.k * op.k,
                       launch_conv_bn_frozen_split16(x, params + op.w_off, params + op.g_off, params + op.b_off, bufs + op.rm_off, bufs + op.rv_off,
                                                     op.res_src == -2 ? nullptr : tensor_of(t, op.res_src), y, n, op.h, op.w, op.cin, op.cout, op.k, op.stride,
                                                     op.pad, op.relu, x_scale, w_scale, t->wpack, st));
                continue;
            }
            TR_RUN(op.conv + " split16", 2.0 * rows * op.cout * op.cin * op.k * op.k,
                   launch_conv_fwd_split16(x, params + op.w_off, op.z, n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, x_scale, w_scale, t->wpack, st));
            TR_RUN(op.bn, 0, bn(op, op.res_src == -2 ? nullptr : tensor_of(t, op.res_src), rows, i < P, y));
            continue;
        }
        TR_RUN(op.conv + " pack", 0, launch_pack_conv_weights(params + op.w_off, t->wpack, op.cout, op.cin, op.k, false, st));
        if (i < P) {                              // a frozen prefix op: convolution and BatchNorm on the running statistics as one launch, no z
            TR_RUN(op.conv + " bn frozen", 2.0 * rows * op.cout * op.cin * op.k * op.k,
                   launch_conv_bn_frozen_f32(tensor_of(t, op.in_src), t->wpack, params + op.g_off, params + op.b_off, bufs + op.rm_off, bufs + op.rv_off,
                                             op.res_src == -2 ? nullptr : tensor_of(t, op.res_src), y, n, op.h, op.w, op.cin, op.cout, op.k, op.stride,
                                             op.pad, op.relu, st));
            continue;
        }
        TR_RUN(op.conv, 2.0 * rows * op.cout * op.cin * op.k * op.k,
               launch_conv_f32(tensor_of(t, op.in_src), t->wpack, t->zero_bias, nullptr, op.z, n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, 0, st));
        TR_RUN(op.bn, 0, bn(op, op.res_src == -2 ? nullptr : tensor_of(t, op.res_src), rows, i < P));
    }
    if (prefix_only) {                            // nothing of a forward is held: the caller's memory is not remembered either
        t->ext_boundary = nullptr;
        return collect_times(t, 0, st);
    }
    TR_RUN("avgpool", 0, launch_avgpool(t->ops.back().y, out, out_stride, n, t->final_hw, t->final_c, 1, PVR_F32, st));
    t->fwd_n = n;
    return collect_times(t, 0, st);
}

}  // namespace

extern "C" {

pvr_status pvr_trainer_forward(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w, float *out,
                               int64_t out_stride, void *stream) {
    PVR_REQUIRE(t && params && bn_buffers && frames && out, "pvr_trainer_forward: null argument");
    if (t->bn_frozen)
        PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward: %d frames, the workspace holds max_batch = %d (with frozen BatchNorm the frames are "
                    "independent: run them as passes of at most max_batch and accumulate with pvr_trainer_backward_acc)", n, t->desc.max_batch);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward: %d frames, the workspace holds max_batch = %d (BatchNorm takes the whole batch of a forward "
                "together: it is not chunked)", n, t->desc.max_batch);
    TraceScope ts("pvr_trainer_forward");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, nullptr, false, out, out_stride, stream);
}

int64_t pvr_trainer_boundary_floats(const pvr_trainer *t) {
    if (!t || t->train_from <= 0) return 0;
    if (t->boundary_src == -1) return (int64_t)56 * 56 * 64;
    const TrainOp &op = t->ops[t->boundary_src];
    return (int64_t)op.ho * op.wo * op.cout;
}

pvr_status pvr_trainer_forward_boundary(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                        float *boundary, int32_t reuse, float *out, int64_t out_stride, void *stream) {
    PVR_REQUIRE(t && params && bn_buffers && out, "pvr_trainer_forward_boundary: null argument");
    if (t->train_from <= 0) {
        set_error("pvr_trainer_forward_boundary: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "keep; use pvr_trainer_forward");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(boundary, "pvr_trainer_forward_boundary: null boundary_dev (n x pvr_trainer_boundary_floats = %lld floats of device memory)",
                (long long)pvr_trainer_boundary_floats(t));
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_forward_boundary: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward_boundary: %d frames, the workspace holds max_batch = %d (run the frames as passes of at most "
                "max_batch, each on its own rows of the boundary cache)", n, t->desc.max_batch);
    PVR_REQUIRE(reuse || frames, "pvr_trainer_forward_boundary: null frames_dev with reuse == 0 (only a reuse pass, which starts at the first trained op, reads no "
                "frames)");
    TraceScope ts("pvr_trainer_forward_boundary");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, boundary, reuse != 0, out, out_stride, stream);
}

pvr_status pvr_trainer_forward_windows(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                       const int32_t *windows, float *boundary, int32_t reuse, float *out, int64_t out_stride, void *stream) {
    if (!windows || (boundary && reuse))          // no window is read: the centre-crop entry points, with their own refusals
        return boundary ? pvr_trainer_forward_boundary(t, params, bn_buffers, frames, n, h, w, boundary, reuse, out, out_stride, stream)
                        : pvr_trainer_forward(t, params, bn_buffers, frames, n, h, w, out, out_stride, stream);
    PVR_REQUIRE(t && params && bn_buffers && frames && out, "pvr_trainer_forward_windows: null argument (only a reuse pass, which starts at the first trained "
                "op, reads no frames)");
    PVR_REQUIRE(((uintptr_t)windows & 3) == 0, "pvr_trainer_forward_windows: windows_dev %p is not 4-byte aligned (n x (top, left) int32)", (const void *)windows);
    if (boundary && t->train_from <= 0) {
        set_error("pvr_trainer_forward_windows: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "keep; pass a null boundary_dev");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_forward_windows: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward_windows: %d frames, the workspace holds max_batch = %d (with frozen BatchNorm run the "
                "frames as passes of at most max_batch, each with its own rows of the windows; batch statistics take the whole batch together)", n,
                t->desc.max_batch);
    PVR_REQUIRE(h > 0 && w > 0, "pvr_trainer_forward_windows: bad frame size h=%d w=%d", h, w);
    int rh, rw;
    resized_size(h, w, t->desc.resize, &rh, &rw);
    PVR_REQUIRE(rh >= t->desc.crop && rw >= t->desc.crop, "pvr_trainer_forward_windows: resized frame %dx%d (of %dx%d) smaller than crop %d", rh, rw, h, w,
                t->desc.crop);
    TraceScope ts("pvr_trainer_forward_windows");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, boundary, false, out, out_stride, stream, false, windows);
}

pvr_status pvr_trainer_forward_augmented(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                         const int32_t *windows, const void *color, uint32_t *gray_sums, float *boundary, int32_t reuse, float *out,
                                         int64_t out_stride, void *stream) {
    if (!color || (boundary && reuse))            // no colour parameter is read: the windows entry point, with its own refusals
        return pvr_trainer_forward_windows(t, params, bn_buffers, frames, n, h, w, windows, boundary, reuse, out, out_stride, stream);
    PVR_REQUIRE(t && params && bn_buffers && frames && out, "pvr_trainer_forward_augmented: null argument (only a reuse pass, which starts at the first "
                "trained op, reads no frames)");
    PVR_REQUIRE(windows, "pvr_trainer_forward_augmented: color_dev without windows_dev (the jitter acts on a frame's window: pass the centre window, "
                "nearbyint((resized size - crop) / 2), for every frame where no random crop is wanted)");
    PVR_REQUIRE(((uintptr_t)windows & 3) == 0, "pvr_trainer_forward_augmented: windows_dev %p is not 4-byte aligned (n x (top, left) int32)",
                (const void *)windows);
    PVR_REQUIRE(((uintptr_t)color & 3) == 0, "pvr_trainer_forward_augmented: color_dev %p is not 4-byte aligned (n x (float b, float c, float s, int32 "
                "order))", color);
    PVR_REQUIRE(gray_sums && ((uintptr_t)gray_sums & 3) == 0, "pvr_trainer_forward_augmented: gray_sums_dev %p is null or not 4-byte aligned (n uint32 of "
                "device scratch, the caller's)", (void *)gray_sums);
    if (boundary && t->train_from <= 0) {
        set_error("pvr_trainer_forward_augmented: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "keep; pass a null boundary_dev");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_forward_augmented: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward_augmented: %d frames, the workspace holds max_batch = %d (with frozen BatchNorm run the "
                "frames as passes of at most max_batch, each with its own rows of the windows and colour parameters; batch statistics take the whole batch "
                "together)", n, t->desc.max_batch);
    PVR_REQUIRE(h > 0 && w > 0, "pvr_trainer_forward_augmented: bad frame size h=%d w=%d", h, w);
    int rh, rw;
    resized_size(h, w, t->desc.resize, &rh, &rw);
    PVR_REQUIRE(rh >= t->desc.crop && rw >= t->desc.crop, "pvr_trainer_forward_augmented: resized frame %dx%d (of %dx%d) smaller than crop %d", rh, rw, h, w,
                t->desc.crop);
    PVR_REQUIRE(t->desc.crop <= 256, "pvr_trainer_forward_augmented: crop %d (at most 256: the gray mean is exact while 255 crop^2 < 2^24)", t->desc.crop);
    TraceScope ts("pvr_trainer_forward_augmented");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, boundary, false, out, out_stride, stream, false, windows, color, gray_sums);
}

pvr_status pvr_trainer_forward_rects(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                     const int32_t *rects, const void *color, uint32_t *gray_sums, float *boundary, int32_t reuse, float *out,
                                     int64_t out_stride, void *stream) {
    if (!rects || (boundary && reuse))            // no rectangle is read: the augmented entry point with null windows, with its own refusals
        return pvr_trainer_forward_augmented(t, params, bn_buffers, frames, n, h, w, nullptr, color, gray_sums, boundary, reuse, out, out_stride, stream);
    PVR_REQUIRE(t && params && bn_buffers && frames && out, "pvr_trainer_forward_rects: null argument (only a reuse pass, which starts at the first trained "
                "op, reads no frames)");
    PVR_REQUIRE(((uintptr_t)rects & 3) == 0, "pvr_trainer_forward_rects: rects_dev %p is not 4-byte aligned (n x (top, left, height, width) int32)",
                (const void *)rects);
    if (color) {
        PVR_REQUIRE(((uintptr_t)color & 3) == 0, "pvr_trainer_forward_rects: color_dev %p is not 4-byte aligned (n x (float b, float c, float s, int32 order))",
                    color);
        PVR_REQUIRE(gray_sums && ((uintptr_t)gray_sums & 3) == 0, "pvr_trainer_forward_rects: gray_sums_dev %p is null or not 4-byte aligned (n uint32 of "
                    "device scratch, the caller's)", (void *)gray_sums);
        PVR_REQUIRE(t->desc.crop <= 256, "pvr_trainer_forward_rects: crop %d (at most 256: the gray mean is exact while 255 crop^2 < 2^24)", t->desc.crop);
    }
    if (boundary && t->train_from <= 0) {
        set_error("pvr_trainer_forward_rects: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "keep; pass a null boundary_dev");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_forward_rects: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward_rects: %d frames, the workspace holds max_batch = %d (with frozen BatchNorm run the "
                "frames as passes of at most max_batch, each with its own rows of the rectangles and colour parameters; batch statistics take the whole batch "
                "together)", n, t->desc.max_batch);
    PVR_REQUIRE(h > 0 && w > 0, "pvr_trainer_forward_rects: bad frame size h=%d w=%d", h, w);       // (no Resize on this path: a frame may be smaller than the crop)
    TraceScope ts("pvr_trainer_forward_rects");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, boundary, false, out, out_stride, stream, false, nullptr, color, gray_sums, rects);
}

pvr_status pvr_trainer_forward_staged(pvr_trainer *t, const float *params, void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                      const int32_t *windows, const int32_t *rects, const void *color, uint32_t *gray_sums, const void *blur, void *staged,
                                      float *boundary, int32_t reuse, float *out, int64_t out_stride, void *stream) {
    if (!blur || (boundary && reuse))             // no blur parameter is read: the rectangle or the window entry point, with its own refusals
        return rects ? pvr_trainer_forward_rects(t, params, bn_buffers, frames, n, h, w, rects, color, gray_sums, boundary, reuse, out, out_stride, stream)
                     : pvr_trainer_forward_augmented(t, params, bn_buffers, frames, n, h, w, windows, color, gray_sums, boundary, reuse, out, out_stride,
                                                     stream);
    PVR_REQUIRE(t && params && bn_buffers && frames && out, "pvr_trainer_forward_staged: null argument (only a reuse pass, which starts at the first trained "
                "op, reads no frames)");
    PVR_REQUIRE((windows != nullptr) != (rects != nullptr), "pvr_trainer_forward_staged: blur_dev with %s (exactly one pixel source: pass the centre window, "
                "nearbyint((resized size - crop) / 2), for every frame where no random crop is wanted)", windows ? "both windows_dev and rects_dev"
                : "neither windows_dev nor rects_dev");
    PVR_REQUIRE(((uintptr_t)windows & 3) == 0 && ((uintptr_t)rects & 3) == 0, "pvr_trainer_forward_staged: windows_dev %p / rects_dev %p is not 4-byte "
                "aligned (int32 rows)", (const void *)windows, (const void *)rects);
    PVR_REQUIRE(((uintptr_t)blur & 3) == 0, "pvr_trainer_forward_staged: blur_dev %p is not 4-byte aligned (n x (float sigma, int32 gray))", blur);
    PVR_REQUIRE(staged && ((uintptr_t)staged & 15) == 0, "pvr_trainer_forward_staged: staged_dev %p is null or not 16-byte aligned ((n, crop, crop, 4) uint8 "
                "of device scratch, the caller's)", staged);
    if (color) {
        PVR_REQUIRE(((uintptr_t)color & 3) == 0, "pvr_trainer_forward_staged: color_dev %p is not 4-byte aligned (n x (float b, float c, float s, int32 "
                    "order))", color);
        PVR_REQUIRE(gray_sums && ((uintptr_t)gray_sums & 3) == 0, "pvr_trainer_forward_staged: gray_sums_dev %p is null or not 4-byte aligned (n uint32 of "
                    "device scratch, the caller's)", (void *)gray_sums);
    }
    PVR_REQUIRE(t->desc.crop >= 12 && t->desc.crop <= 256, "pvr_trainer_forward_staged: crop %d (12 .. 256: a reflect padding of 11, and the gray mean is "
                "exact while 255 crop^2 < 2^24)", t->desc.crop);
    if (boundary && t->train_from <= 0) {
        set_error("pvr_trainer_forward_staged: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "keep; pass a null boundary_dev");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_forward_staged: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_forward_staged: %d frames, the workspace holds max_batch = %d (with frozen BatchNorm run the "
                "frames as passes of at most max_batch, each with its own rows of the parameter arrays; batch statistics take the whole batch together)", n,
                t->desc.max_batch);
    PVR_REQUIRE(h > 0 && w > 0, "pvr_trainer_forward_staged: bad frame size h=%d w=%d", h, w);
    if (windows) {
        int rh, rw;
        resized_size(h, w, t->desc.resize, &rh, &rw);
        PVR_REQUIRE(rh >= t->desc.crop && rw >= t->desc.crop, "pvr_trainer_forward_staged: resized frame %dx%d (of %dx%d) smaller than crop %d", rh, rw, h, w,
                    t->desc.crop);
    }
    TraceScope ts("pvr_trainer_forward_staged");
    return forward_pass(t, params, bn_buffers, frames, n, h, w, boundary, false, out, out_stride, stream, false, windows, color, gray_sums, rects, blur, staged);
}

pvr_status pvr_trainer_prefix_forward(pvr_trainer *t, const float *params, const void *bn_buffers, const uint8_t *frames, int32_t n, int32_t h, int32_t w,
                                      float *boundary, void *stream) {
    PVR_REQUIRE(t && params && bn_buffers && frames && boundary, "pvr_trainer_prefix_forward: null argument (boundary_dev takes n x "
                "pvr_trainer_boundary_floats floats of device memory)");
    if (t->train_from <= 0) {
        set_error("pvr_trainer_prefix_forward: everything trains (pvr_trainer_set_train_from stage 0): there is no frozen prefix and no boundary tensor to "
                  "compute ahead of a step");
        return PVR_ERR_STATE;
    }
    PVR_REQUIRE(((uintptr_t)boundary & 15) == 0, "pvr_trainer_prefix_forward: boundary_dev %p is not 16-byte aligned (the launches move it as float4s)",
                (void *)boundary);
    PVR_REQUIRE(n > 0 && n <= t->desc.max_batch, "pvr_trainer_prefix_forward: %d frames, the workspace holds max_batch = %d (fill a cache in blocks of at most "
                "max_batch frames, each into its own rows)", n, t->desc.max_batch);
    TraceScope ts("pvr_trainer_prefix_forward");
    // (the prefix reads the BatchNorm buffers only: every BatchNorm of a prefix pass is the frozen-apply launch, whatever the handle's mode)
    return forward_pass(t, params, const_cast<void *>(bn_buffers), frames, n, h, w, boundary, false, nullptr, 0, stream, true);
}

}  // extern "C"

namespace {

// the backward of the held forward into `grads` (fully overwritten); the caller has checked that a forward is held
pvr_status backward_into(pvr_trainer *t, const float *params, const float *dout, int64_t dout_stride, float *grads, hipStream_t st) {
    const int n = t->fwd_n;
    t->fwd_n = 0;
    pvr_status s;
    Tick tick{t, st};
    const size_t first_time = t->times.size();
    const auto bn_bwd = t->bn_frozen ? pvr_op_bn_frozen_backward : pvr_op_bn_train_backward;      // (the same arguments: mean / rstd are the slots the forward wrote)
    std::vector<char> have(t->ops.size() + 1, 0);  // gradient of tensor src (index src + 1) holds a value already: the next contribution accumulates
    const int last = (int)t->ops.size() - 1;
    // split mode: the scale of a saved activation is computed once per backward, by its first consumer; dz's right after the BatchNorm backward
    // conv_split16: the forward left every saved activation's scale in its slot, so the launch takes dz and the convolution's weights instead
    const bool split = t->wgrad_split16, csplit = t->conv_split16;
    std::vector<char> scaled(t->ops.size() + 1, csplit ? 1 : 0);
    float *dz_scale = split || csplit ? t->scales + t->ops.size() + 2 : nullptr;
    uint32_t *scale_aux = split || csplit ? (uint32_t *)(t->scales + t->ops.size() + 3) : nullptr;
    float *w_scale = csplit ? t->scales + t->ops.size() + 7 : nullptr;
    // one launch per convolution: dz, and the input tensor when this is its first consumer of the backward (x == nullptr: scaled already)
    auto scales_of = [&](const std::string &conv, size_t dz_count, const float *x, size_t x_count, float *x_slot) -> pvr_status {
        TR_RUN(conv + " scale", 0, pvr_op_absmax_scale_pair(t->dz, (int64_t)dz_count, dz_scale, x, (int64_t)x_count, x ? x_slot : nullptr, scale_aux, st));
        return PVR_OK;
    };
    TR_RUN("avgpool bwd", 0, pvr_op_avgpool_backward(dout, dout_stride, t->ops[last].dy, n, t->final_hw, t->final_c, st));
    have[last + 1] = 1;
    const int P = t->prefix_ops();                // the walk stops at the first trained op: the frozen prefix has no backward
    for (int i = last; i >= P; --i) {
        TrainOp &op = t->ops[i];
        const bool x_frozen = t->in_prefix(op.in_src);      // reads the boundary tensor: a weight gradient and no data gradient
        PVR_REQUIRE(have[i + 1], "pvr_trainer_backward: %s has no consumer", op.conv.c_str());
        const int64_t rows = (int64_t)n * op.ho * op.wo;
        float *dres = op.res_src == -2 || t->in_prefix(op.res_src) ? nullptr : grad_of(t, op.res_src);
        TR_RUN(op.bn + " bwd", 0,
               bn_bwd(op.z, op.y, op.dy, params + op.g_off, op.mean, op.rstd, t->dz, dres, dres ? have[op.res_src + 1] : 0, grads + op.g_off, grads + op.b_off,
                      rows, op.cout, op.relu, t->bn_scratch, t->bn_floats, st));
        if (dres) have[op.res_src + 1] = 1;
        const double fl = 2.0 * rows * op.cout * op.cin * op.k * op.k;
        if (csplit && (split || !x_frozen))
            TR_RUN(op.conv + " bwd scale", 0,
                   pvr_op_absmax_scale_pair(t->dz, (int64_t)out_elems(op, n), dz_scale, params + op.w_off, (int64_t)op.cout * op.cin * op.k * op.k, w_scale,
                                            scale_aux, st));
        if (split) {
            float *x_scale = t->scales + op.in_src + 1;
            if (!csplit && (s = scales_of(op.conv, out_elems(op, n), scaled[op.in_src + 1] ? nullptr : tensor_of(t, op.in_src), (size_t)n * op.h * op.w * op.cin, x_scale)))
                return s;
            scaled[op.in_src + 1] = 1;
            TR_RUN(op.conv + " wgrad", fl,
                   pvr_op_conv_wgrad_split16(tensor_of(t, op.in_src), t->dz, grads + op.w_off, n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, x_scale,
                                             dz_scale, t->wg_scratch, t->wg_floats, st));
        } else
            TR_RUN(op.conv + " wgrad", fl,
                   pvr_op_conv_wgrad(tensor_of(t, op.in_src), t->dz, grads + op.w_off, n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad, t->wg_scratch,
                                     t->wg_floats, st));
        if (x_frozen) continue;
        if (csplit)
            TR_RUN(op.conv + " dgrad split16", fl,
                   launch_conv_dgrad_split16(t->dz, params + op.w_off, grad_of(t, op.in_src), have[op.in_src + 1], n, op.h, op.w, op.cin, op.cout, op.k, op.stride,
                                             op.pad, dz_scale, w_scale, t->wpack, t->dil, st));
        else
            TR_RUN(op.conv + " dgrad", fl,
                   launch_conv_dgrad(t->dz, params + op.w_off, grad_of(t, op.in_src), have[op.in_src + 1], n, op.h, op.w, op.cin, op.cout, op.k, op.stride, op.pad,
                                     t->wpack, t->dil, t->zero_bias, st));
        have[op.in_src + 1] = 1;
    }
    if (t->train_from > 0) {                      // grads stays fully overwritten: the prefix's span is one leading run of zeros
        TR_RUN("prefix grads zero", 0, memset_floats(grads, t->ops[P].w_off, st));
        return collect_times(t, first_time, st);
    }
    PVR_REQUIRE(have[0], "pvr_trainer_backward: the max pool's output has no consumer");
    TrainOp &sm = t->stem;
    TR_RUN("maxpool bwd", 0, pvr_op_maxpool_backward(sm.y, t->dpool, sm.dy, n, 112, 112, 64, st));
    TR_RUN("bn1 bwd", 0,
           bn_bwd(sm.z, sm.y, sm.dy, params + sm.g_off, sm.mean, sm.rstd, t->dz, nullptr, 0, grads + sm.g_off, grads + sm.b_off, (int64_t)n * 112 * 112, 64, 1,
                  t->bn_scratch, t->bn_floats, st));
    if (split) {
        float *img_scale = t->scales + t->ops.size() + 1;
        if ((s = scales_of("conv1", (size_t)n * 112 * 112 * 64, t->d_imgf, (size_t)n * S_IMG * S_IMG * 4, img_scale))) return s;
        TR_RUN("conv1 wgrad", 2.0 * n * 112 * 112 * 64 * 147,
               pvr_op_stem_wgrad_split16(t->d_imgf, t->dz, grads + sm.w_off, n, S_IMG, img_scale, dz_scale, t->wg_scratch, t->wg_floats, st));
    } else
        TR_RUN("conv1 wgrad", 2.0 * n * 112 * 112 * 64 * 147, pvr_op_stem_wgrad(t->d_imgf, t->dz, grads + sm.w_off, n, S_IMG, t->wg_scratch, t->wg_floats, st));
    return collect_times(t, first_time, st);
}

pvr_status no_forward_held(const char *what) {
    set_error("%s: no forward's activations are held (one backward per pvr_trainer_forward, right after it)", what);
    return PVR_ERR_STATE;
}

}  // namespace

extern "C" {

pvr_status pvr_trainer_backward(pvr_trainer *t, const float *params, const float *dout, int64_t dout_stride, float *grads, void *stream) {
    PVR_REQUIRE(t && params && dout && grads, "pvr_trainer_backward: null argument");
    if (t->fwd_n <= 0) return no_forward_held("pvr_trainer_backward");
    TraceScope ts("pvr_trainer_backward");
    return backward_into(t, params, dout, dout_stride, grads, (hipStream_t)stream);
}

pvr_status pvr_trainer_backward_acc(pvr_trainer *t, const float *params, const float *dout, int64_t dout_stride, float *grads, int32_t accumulate,
                                    float *scratch, int64_t scratch_floats, void *stream) {
    PVR_REQUIRE(t && params && dout && grads, "pvr_trainer_backward_acc: null argument");
    if (t->fwd_n <= 0) return no_forward_held("pvr_trainer_backward_acc");
    TraceScope ts("pvr_trainer_backward_acc");
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) return backward_into(t, params, dout, dout_stride, grads, st);
    // (checked before the held forward is spent: a refused call leaves it in place)
    PVR_REQUIRE(scratch && scratch_floats >= t->n_params, "pvr_trainer_backward_acc: accumulate needs a scratch of pvr_trainer_param_count = %lld floats, got %lld",
                (long long)t->n_params, (long long)(scratch ? scratch_floats : 0));
    pvr_status s;
    if ((s = backward_into(t, params, dout, dout_stride, scratch, st))) return s;
    return launch_grad_add(grads, scratch, t->n_params, st);
}

pvr_status pvr_trainer_set_bn_frozen(pvr_trainer *t, int32_t on) {
    PVR_REQUIRE(t, "pvr_trainer_set_bn_frozen: null trainer");
    t->bn_frozen = on != 0;
    t->fwd_n = 0;                                 // a held forward was made in the other mode: its mean / rstd slots mean something else
    return PVR_OK;
}

pvr_status pvr_trainer_set_wgrad_split16(pvr_trainer *t, int32_t on) {
    PVR_REQUIRE(t, "pvr_trainer_set_wgrad_split16: null trainer");
    if (t->arena && (on != 0) != t->wgrad_split16) {
        set_error("pvr_trainer_set_wgrad_split16: the workspace of this handle exists already (the first forward made it for the %s weight gradients): choose "
                  "the mode before the first forward", t->wgrad_split16 ? "split-f16" : "fp32");
        return PVR_ERR_STATE;
    }
    t->wgrad_split16 = on != 0;
    return PVR_OK;
}

pvr_status pvr_trainer_set_conv_split16(pvr_trainer *t, int32_t on) {
    PVR_REQUIRE(t, "pvr_trainer_set_conv_split16: null trainer");
    if (t->arena && (on != 0) != t->conv_split16) {
        set_error("pvr_trainer_set_conv_split16: the workspace of this handle exists already (the first forward made it for the %s convolutions): choose "
                  "the mode before the first forward", t->conv_split16 ? "split-f16" : "fp32");
        return PVR_ERR_STATE;
    }
    t->conv_split16 = on != 0;
    return PVR_OK;
}

pvr_status pvr_trainer_set_train_from(pvr_trainer *t, int32_t stage) {
    PVR_REQUIRE(t, "pvr_trainer_set_train_from: null trainer");
    PVR_REQUIRE(stage >= 0 && stage <= 4, "pvr_trainer_set_train_from: stage %d (0: everything trains; 1 .. 4: layer<stage> .. layer4 train, conv1 / bn1 and "
                "the layers below are frozen)", stage);
    if (t->arena && stage != t->train_from) {
        set_error("pvr_trainer_set_train_from: the workspace of this handle exists already (the first forward made it for train_from stage %d): choose "
                  "the stage before the first forward", t->train_from);
        return PVR_ERR_STATE;
    }
    int first = 0;
    if (stage > 0) {
        const std::string pre = "layer" + std::to_string(stage) + ".";
        first = -1;
        for (int i = 0; i < (int)t->ops.size() && first < 0; ++i)
            if (t->ops[i].conv.compare(0, pre.size(), pre) == 0) first = i;
        PVR_REQUIRE(first >= 0, "pvr_trainer_set_train_from: this trunk has no %s", pre.c_str());
        for (int i = first; i < (int)t->ops.size(); ++i)       // (op order is layer order: the prefix is one leading span of the parameters)
            PVR_REQUIRE(t->ops[i].in_src >= -1 && t->ops[i].w_off >= t->ops[first].w_off, "pvr_trainer_set_train_from: the ops of %s do not end the plan", pre.c_str());
    }
    // the boundary: for these trunks the trained ops read exactly ONE tensor of the prefix (carve_prefix's "piece of its own")
    int bsrc = -2;
    if (stage > 0)
        for (int i = first; i < (int)t->ops.size(); ++i)
            for (int src : {t->ops[i].in_src, t->ops[i].res_src}) {
                if (src == -2 || src >= first) continue;
                PVR_REQUIRE(bsrc == -2 || bsrc == src, "pvr_trainer_set_train_from: the trained ops of stage %d read more than one tensor of the prefix", stage);
                bsrc = src;
            }
    PVR_REQUIRE(stage == 0 || bsrc != -2, "pvr_trainer_set_train_from: no trained op of stage %d reads the prefix", stage);
    if (stage != t->train_from) t->fwd_n = 0;     // (only before the arena exists: no forward is held)
    t->train_from = stage;
    t->first_trained = first;
    t->boundary_src = bsrc;
    return PVR_OK;
}

pvr_status pvr_trainer_set_prefix_fused(pvr_trainer *t, int32_t on) {
    PVR_REQUIRE(t, "pvr_trainer_set_prefix_fused: null trainer");
    if (t->arena && (on != 0) != t->prefix_fused) {
        set_error("pvr_trainer_set_prefix_fused: the workspace of this handle exists already (the first forward made it for the %s prefix ops): choose "
                  "the mode before the first forward", t->prefix_fused ? "fused" : "unfused");
        return PVR_ERR_STATE;
    }
    t->prefix_fused = on != 0;
    return PVR_OK;
}
int32_t pvr_trainer_train_from(const pvr_trainer *t) { return t ? t->train_from : 0; }
int64_t pvr_trainer_trained_offset(const pvr_trainer *t) { return t && t->train_from > 0 ? t->ops[t->first_trained].w_off : 0; }

}  // extern "C"
