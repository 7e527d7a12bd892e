// The ResNet family's launch plan: the op list, split-K, both launch schedules and the per-batch-size kernel table.  Pure host code: every decision is a
// function of pvr_encoder_desc (arch, dtype, chunk), PlanSwitches, low_latency and fuse - no weight value, no device pointer and no HIP call enters it, so
// pvr_encoder_create builds the plan and a handle that was never finalized answers pvr_encoder_launch_name / pvr_encoder_launch_kernel.  What the plan needs
// on the device (packed weight images, workspace) is made by pvr_encoder_finalize (encoder.hip: prepare_weights).
#include "encoder_internal.h"

namespace pvr {

const char *launch_kind_name(int k) {
    static const char *nm[] = {"conv", "bneck_frame(front1)", "bneck_frame", "bneck_frame(run)", "(in the run)", "frame_members", "conv_pp256(dual)", "dual_members", "chain", "cast",
                               "conv_f32", "conv_split16", "conv_split16(pair)", "conv_split16(in32)", "splitk(small)", "splitk", "conv_expand(blocked)",
                               "conv_wfrag(pool)", "conv_wfrag", "chain(y_s2)", "conv_expand(y_s2)"};
    static_assert(sizeof nm / sizeof nm[0] == LK_COUNT, "one name per LaunchKind");
    return k >= 0 && k < LK_COUNT ? nm[k] : "?";
}

// The builders emit ops by role: the role gives the state-dict names behind the block's prefix `p`.  Returns the op's index.
static int add_conv(pvr_encoder *e, OpRole role, const std::string &p, int in_buf, int out_buf, int res_buf, int hw, int cin, int cin_real, int cout,
                    int cout_real, int k, int stride, int relu, int out_f32 = 0) {
    static const char *const name[][2] = {{".conv1", ".bn1"}, {".conv2", ".bn2"}, {".conv3", ".bn3"}, {".downsample.0", ".downsample.1"}, {".conv1", ".bn1"},
                                          {".downsample.0", ".downsample.1"}, {".conv2", ".bn2"}, {".conv2", ".bn2"}, {".conv3", ".bn3"}};
    static_assert(sizeof name / sizeof name[0] == R_AVGPOOL2, "one pair of names per convolution role");
    ConvOp op;
    op.role = role; op.conv = p + name[role][0]; op.bn = p + name[role][1]; op.in_buf = in_buf; op.out_buf = out_buf; op.res_buf = res_buf;
    op.h = hw; op.w = hw; op.cin = cin; op.cin_real = cin_real; op.cout = cout; op.cout_real = cout_real;
    op.k = k; op.stride = stride; op.pad = k / 2; op.relu = relu; op.out_f32 = out_f32;
    e->ops.push_back(op);
    return (int)e->ops.size() - 1;
}

static int add_cast(pvr_encoder *e, int in_buf, int out_buf, int hw, int c) {
    ConvOp op;
    op.role = R_CAST; op.conv = "cast"; op.in_buf = in_buf; op.out_buf = out_buf; op.res_buf = B_NONE;
    op.h = hw; op.w = hw; op.cin = op.cout = op.cout_real = c; op.cin_real = 0; op.k = 1; op.stride = 1; op.pad = 0; op.relu = 0; op.out_f32 = 0;
    e->ops.push_back(op);
    return (int)e->ops.size() - 1;
}

// the last op of a stage's last block is the stage's tap "layer<stage + 1>"
static void tap_stage(pvr_encoder *e, int stage, int buf, int hw, int c, int f32) {
    const std::string tn = "layer" + std::to_string(stage + 1);
    e->ops.back().tap = tn;
    e->taps[tn] = {buf, {hw, hw, c, f32}};
}

// torchvision resnet50 v1.5: layers [3,4,6,3], stride on the 3x3 (conv2), downsample on block 0
//
// Parity plan of the compressed PVRs (resid32: *_l3 / *_l4 in f16 storage).  These variants have no final average pool, so the
// trunk's accumulated storage rounding reaches the output element by element (measured 1.09e-3 / 9.6e-4 rel-L2 with every
// activation in f16).  From layer3 on the residual stream y is therefore kept in fp32 (conv3 adds an fp32 identity / fp32
// downsample output and writes fp32; a 16-bit copy feeds the next block's convolutions), and the compression head - three
// small 3x3 convolutions over K = 9216 / 18432 - runs from that fp32 stream with fp32 weights on the f32-input MFMA
// (conv_f32.hip).  layer3 / layer4 are MFMA-bound at 14x14 / 7x7, so the extra fp32 bytes cost little.  PVR_RESID32=0 restores
// the all-16-bit plan (A/B).
static void build_resnet50(pvr_encoder *e) {
    const int arch = e->desc.arch;
    const int stages = arch == PVR_ARCH_RESNET50_L3 ? 3 : 4;
    const int nblk[4] = {3, 4, 6, 3};
    e->resid32 = e->desc.dtype == PVR_F16 && arch != PVR_ARCH_RESNET50 && e->sw.resid32 != 0;
    // Round 3: the fp32 residual stream alone left *_l3 at 9.75e-4 of a 1e-3 bound, and CPU emulation over three weight seeds
    // (scripts/emulate_l3_rounding.py) puts that plan at 8.6e-4 ... 1.01e-3: one seed from red.  What gives real margin is the LAST
    // trunk stage entirely in fp32 (fp32 weights, fp32 operands: conv_f32.hip, the kernels of the PVR_F32 mode) with the fp32
    // residual stream starting at layer2: 5.6e-4 ... 6.4e-4 on the same seeds for *_l3, 6.3e-4 ... 6.7e-4 for *_l4 (16-bit weights alone cost ~6e-4
    // at layer3, whatever the activations do).  That stage is 36 % (layer3) / 20 % (layer4) of the trunk's FLOPs at the f32-MFMA
    // rate: the parity mode of the compressed PVRs pays for its margin in throughput (DESIGN.md section 2 has the numbers);
    // PVR_TAIL_F32=0 restores round 2's plan, bf16 (the throughput mode) never uses either.
    e->tail32 = e->resid32 && e->sw.tail_f32 != 0;
    const int r32_from = e->tail32 ? 1 : 2;             // fp32 residual stream from layer2 on (emulated: *_l3 5.6e-4 ... 6.4e-4, *_l4 6.3e-4 ... 6.7e-4)
    // Round 6: with conv_split16 the convolutions that consume the fp32 stream as a 16-bit operand (the next block's conv1, a stage's downsample) read it
    // themselves and round it in their staging pass (ConvOp::from32): no fp32 -> 16-bit copy launches (3 x 0.11 ms in *_l3, 4 x 0.11 + 5 x 0.05 ms in *_l4)
    const bool in32 = e->resid32 && e->sw.split16 != 0;
    bool x_is_32 = false;                               // the block input exists as fp32 only (the previous block wrote y32 and no 16-bit copy)
    int hw = 56, inpl = 64, x = B_X0, x32 = B_NONE;
    for (int li = 0; li < stages; ++li) {
        const int planes = 64 << li;
        const bool nested = (arch == PVR_ARCH_RESNET50_L4 && li == 3) || (arch == PVR_ARCH_RESNET50_L3 && li == 2);
        const bool r32 = e->resid32 && li >= r32_from;
        const bool f32stage = e->tail32 && li == stages - 1;
        for (int bi = 0; bi < nblk[li]; ++bi) {
            char pfx[64];
            if (nested) snprintf(pfx, sizeof pfx, "layer%d.0.%d", li + 1, bi);
            else snprintf(pfx, sizeof pfx, "layer%d.%d", li + 1, bi);
            const std::string p = pfx;
            const int stride = (bi == 0 && li > 0) ? 2 : 1;
            const int ohw = hw / stride;
            const int y = x == B_X0 ? B_X1 : B_X0;
            const int y32 = x32 == B_Y0 ? B_Y1 : B_Y0;
            const bool last = (li == stages - 1 && bi == nblk[li] - 1), stage_end = bi == nblk[li] - 1;
            Block b{BK_BOTTLENECK, li, bi};
            if (f32stage) {
                // every tensor of the block is fp32 (the 16-bit ping-pong buffers are large enough: the stage's activations are
                // 1/4 ... 1/16 of layer1's elements); the block reads the fp32 stream directly
                b.conv1 = add_conv(e, R_CONV1, p, x32, B_T1, B_NONE, hw, inpl, inpl, planes, planes, 1, 1, 1);
                b.conv2 = add_conv(e, R_CONV2, p, B_T1, B_T2, B_NONE, hw, planes, planes, planes, planes, 3, stride, 1);
                if (bi == 0) b.ds = add_conv(e, R_DOWNSAMPLE, p, x32, B_DS, B_NONE, hw, inpl, inpl, planes * 4, planes * 4, 1, stride, 0, 1);
                b.conv3 = add_conv(e, R_CONV3, p, B_T2, y32, bi == 0 ? B_DS : x32, ohw, planes, planes, planes * 4, planes * 4, 1, 1, 1, 1 | 2);
                for (int i = b.conv1; i <= b.conv3; ++i) e->ops[i].f32op = true;
                if (stage_end) tap_stage(e, li, y32, ohw, planes * 4, 1);
                x32 = y32;
            } else {
                b.conv1 = add_conv(e, R_CONV1, p, x_is_32 ? x32 : x, B_T1, B_NONE, hw, inpl, inpl, planes, planes, 1, 1, 1);
                e->ops.back().from32 = x_is_32;
                b.conv2 = add_conv(e, R_CONV2, p, B_T1, B_T2, B_NONE, hw, planes, planes, planes, planes, 3, stride, 1);
                if (bi == 0) {
                    b.ds = add_conv(e, R_DOWNSAMPLE, p, x_is_32 ? x32 : x, B_DS, B_NONE, hw, inpl, inpl, planes * 4, planes * 4, 1, stride, 0, r32 ? 1 : 0);
                    e->ops.back().from32 = x_is_32;
                }
                const int res = bi == 0 ? B_DS : r32 ? x32 : x;
                if (r32) {
                    b.conv3 = add_conv(e, R_CONV3, p, B_T2, y32, res, ohw, planes, planes, planes * 4, planes * 4, 1, 1, 1, 1 | 2);
                    // the 16-bit copy feeds the next block's convolutions - unless that block is fp32 (it reads the stream itself), as the head does
                    const bool next_f32 = e->tail32 && li == stages - 2 && stage_end;
                    if (!last && !next_f32 && !in32) b.cast = add_cast(e, y32, y, ohw, planes * 4);
                    if (stage_end) tap_stage(e, li, y32, ohw, planes * 4, 1);
                    x32 = y32;
                    x_is_32 = in32;
                } else {
                    // the trunk's last block feeds avgpool: keep fp32 (conv5 variant only)
                    const int f32 = (last && arch == PVR_ARCH_RESNET50) ? 1 : 0;
                    b.conv3 = add_conv(e, R_CONV3, p, B_T2, f32 ? B_F32 : y, res, ohw, planes, planes, planes * 4, planes * 4, 1, 1, 1, f32);
                    if (stage_end) tap_stage(e, li, f32 ? B_F32 : y, ohw, planes * 4, f32);
                }
                x = y;
            }
            e->blocks.push_back(b);
            hw = ohw; inpl = planes * 4;
        }
    }
    if (arch == PVR_ARCH_RESNET50) {
        e->out_size = 2048; e->final_hw = 49; e->final_c = 2048; e->final_creal = 2048;
        return;
    }
    // compression head: BasicBlock(C -> c) with a conv3x3(+bias)+BN downsample (moco.py:35-50 / 79-94)
    const int cin = arch == PVR_ARCH_RESNET50_L3 ? 1024 : 2048;
    const int c = arch == PVR_ARCH_RESNET50_L3 ? 11 : 42;
    const std::string p = arch == PVR_ARCH_RESNET50_L3 ? "layer3.1" : "layer4.1";
    const int hx = e->resid32 ? x32 : x;
    Block b{BK_HEAD, stages - 1, 1};
    b.conv1 = add_conv(e, R_HEAD_CONV1, p, hx, B_T1, B_NONE, hw, cin, cin, 64, c, 3, 1, 1);
    b.ds = add_conv(e, R_HEAD_DOWNSAMPLE, p, hx, B_DS, B_NONE, hw, cin, cin, 64, c, 3, 1, 0);
    b.conv2 = add_conv(e, R_HEAD_CONV2, p, B_T1, B_F32, B_DS, hw, 64, c, 64, c, 3, 1, 1, 1);
    if (e->resid32) for (int i = b.conv1; i <= b.conv2; ++i) e->ops[i].f32op = true;
    e->blocks.push_back(b);
    e->out_size = c * hw * hw; e->final_hw = hw * hw; e->final_c = 64; e->final_creal = c;
}

// torchvision resnet18 / resnet34 (reference embeddings.py:112-117): BasicBlock = conv3x3(stride) bn relu, conv3x3 bn, (+ identity
// or 1x1(stride)+bn downsample), relu; layers [2,2,2,2] / [3,4,6,3], widths 64..512, global average pool -> 512
static void build_basic_resnet(pvr_encoder *e) {
    const int nb18[4] = {2, 2, 2, 2}, nb34[4] = {3, 4, 6, 3};
    const int *nblk = e->desc.arch == PVR_ARCH_RESNET18 ? nb18 : nb34;
    int hw = 56, inpl = 64, x = B_X0;
    for (int li = 0; li < 4; ++li) {
        const int planes = 64 << li;
        for (int bi = 0; bi < nblk[li]; ++bi) {
            char pfx[64];
            snprintf(pfx, sizeof pfx, "layer%d.%d", li + 1, bi);
            const std::string p = pfx;
            const int stride = (bi == 0 && li > 0) ? 2 : 1;
            const int ohw = hw / stride;
            const int y = x == B_X0 ? B_X1 : B_X0;
            const bool last = (li == 3 && bi == nblk[li] - 1);
            Block b{BK_BASIC, li, bi};
            b.conv1 = add_conv(e, R_CONV1, p, x, B_T1, B_NONE, hw, inpl, inpl, planes, planes, 3, stride, 1);
            if (stride > 1 || inpl != planes) b.ds = add_conv(e, R_DOWNSAMPLE, p, x, B_DS, B_NONE, hw, inpl, inpl, planes, planes, 1, stride, 0);
            b.conv2 = add_conv(e, R_CONV2, p, B_T1, last ? B_F32 : y, b.ds >= 0 ? B_DS : x, ohw, planes, planes, planes, planes, 3, 1, 1, last ? 1 : 0);
            if (bi == nblk[li] - 1) tap_stage(e, li, last ? B_F32 : y, ohw, planes, last ? 1 : 0);
            e->blocks.push_back(b);
            x = y; hw = ohw; inpl = planes;
        }
    }
    e->out_size = 512; e->final_hw = 49; e->final_c = 512; e->final_creal = 512;
}

// openai/CLIP ModifiedResNet-50 (reference embeddings.py:305-306): stem conv1 (3x3/2, run by the stem kernel as a 7x7 with only
// its centre taps set) is not in the list; conv2 / conv3 of the stem, AvgPool2d(2), then Bottlenecks whose convolutions all have
// stride 1 - the stride is an AvgPool2d after conv2 and in front of the downsample convolution.  Channels 32 are padded to 64.
static void add_pool(pvr_encoder *e, int in_buf, int out_buf, int h, int c) {
    ConvOp op;
    op.role = R_AVGPOOL2; op.conv = "avgpool2"; op.in_buf = in_buf; op.out_buf = out_buf; op.res_buf = B_NONE;
    op.h = h; op.w = h; op.cin = op.cin_real = op.cout = op.cout_real = c; op.k = 2; op.stride = 2; op.pad = 0; op.relu = 0; op.out_f32 = 0;
    e->ops.push_back(op);
}

static void build_clip_rn50(pvr_encoder *e) {
    add_conv(e, R_STEM_CONV2, "visual", B_STEM, B_X0, B_NONE, 112, 64, 32, 64, 32, 3, 1, 1);
    add_conv(e, R_STEM_CONV3, "visual", B_X0, B_X1, B_NONE, 112, 64, 32, 64, 64, 3, 1, 1);
    add_pool(e, B_X1, B_X0, 112, 64);
    e->ops.back().tap = "stem3";
    e->taps["stem3"] = {B_X0, {56, 56, 64, 0}};
    const int nblk[4] = {3, 4, 6, 3};
    int hw = 56, inpl = 64, x = B_X0;
    for (int li = 0; li < 4; ++li) {
        const int planes = 64 << li;
        for (int bi = 0; bi < nblk[li]; ++bi) {
            char pfx[64];
            snprintf(pfx, sizeof pfx, "visual.layer%d.%d", li + 1, bi);
            const std::string p = pfx;
            const int stride = (bi == 0 && li > 0) ? 2 : 1;
            const int ohw = hw / stride;
            const int y = x == B_X0 ? B_X1 : B_X0;
            const bool last = (li == 3 && bi == nblk[li] - 1);
            Block b{BK_BOTTLENECK, li, bi};
            b.conv1 = add_conv(e, R_CONV1, p, x, B_T1, B_NONE, hw, inpl, inpl, planes, planes, 1, 1, 1);
            b.conv2 = add_conv(e, R_CONV2, p, B_T1, B_T2, B_NONE, hw, planes, planes, planes, planes, 3, 1, 1);
            int c3_in = B_T2, res = x;
            if (stride > 1) { add_pool(e, B_T2, B_T1, hw, planes); c3_in = B_T1; }
            if (stride > 1 || inpl != planes * 4) {
                int ds_in = x;
                if (stride > 1) { add_pool(e, x, B_T2, hw, inpl); ds_in = B_T2; }
                b.ds = add_conv(e, R_DOWNSAMPLE, p, ds_in, B_DS, B_NONE, ohw, inpl, inpl, planes * 4, planes * 4, 1, 1, 0);
                res = B_DS;
            }
            b.conv3 = add_conv(e, R_CONV3, p, c3_in, last ? B_F32 : y, res, ohw, planes, planes, planes * 4, planes * 4, 1, 1, 1, last ? 1 : 0);
            if (bi == nblk[li] - 1) tap_stage(e, li, last ? B_F32 : y, ohw, planes * 4, last ? 1 : 0);
            e->blocks.push_back(b);
            x = y; hw = ohw; inpl = planes * 4;
        }
    }
    e->out_size = 1024; e->final_hw = 49; e->final_c = 2048; e->final_creal = 2048;
}

// Split-K plan (conv_igemm.hip::launch_conv_splitk): long narrow convolutions (K >= 16384 against Cout <= 64: the 3x3 compression
// head of the *_l4 PVRs, 98 pixel tiles of 288 K-slices; the *_l3 head has 392 tiles and is bound by its im2col reads instead,
// measured) get 8 K ranges and, as scratch for the fp32 partial planes, a 16-bit ping-pong buffer that is
// dead at that point of the plan (not read by this or any later op before it is overwritten).  PVR_SPLITK=0 turns it off.
static void plan_splitk(pvr_encoder *e) {
    if (!e->sw.splitk || stores_f32(e->desc.dtype)) return;
    const int n = (int)e->ops.size();
    for (int i = 0; i < n; ++i) {
        ConvOp &op = e->ops[i];
        if (!op.is_conv() || op.f32op || op.from32 || op.cout > 64 || op.k * op.k * op.cin < 16384 || (op.out_f32 & 2)) continue;
        const size_t need = (size_t)8 * e->desc.chunk * op.ho() * op.ho() * op.cout * sizeof(float);
        if (need > e->buf_elems * 2) continue;
        for (int b = 0; b < B_F32 && op.ks_buf == B_NONE; ++b) {      // (16-bit ping-pong buffers only)
            if (b == op.in_buf || b == op.out_buf || b == op.res_buf) continue;
            bool dead = true;
            for (int j = i + 1; j < n; ++j) {
                if (e->ops[j].in_buf == b || e->ops[j].res_buf == b) { dead = false; break; }
                if (e->ops[j].out_buf == b) break;
            }
            if (dead) { op.ks_buf = b; op.ksplit = 8; }
        }

    }
}

// a convolution with 16-bit operands, a 16-bit output and no padded channel: what the fused 16-bit kernels take
static bool plain16(const ConvOp &o) { return o.is_conv() && !o.f32op && !o.from32 && !o.out_f32 && o.cin_real == o.cin && o.cout_real == o.cout; }

// How a block's tail (conv2 -> conv3 + residual) can run fused: only a bottleneck whose every convolution is plain16 - not the fp32 stage or the fp32
// residual stream of the parity plan, not the block that writes the trunk's fp32 output, no basic block, not the head.  The kernels' widths are disjoint:
// per-frame launches take layer3's stride-1 blocks (bneck_frame_supported), chains take widths 64 / 128 (chain_supported).
static LaunchForm tail_form(const pvr_encoder *e, const Block &b) {
    if (b.type != BK_BOTTLENECK) return LF_SINGLE;
    const ConvOp &c2 = e->ops[b.conv2], &c3 = e->ops[b.conv3];
    if (!plain16(e->ops[b.conv1]) || !plain16(c2) || !plain16(c3) || (b.ds >= 0 && !plain16(e->ops[b.ds]))) return LF_SINGLE;
    if (b.ds < 0 && bneck_frame_supported(e->sw, e->desc.chunk, c2.h, c2.w, c2.cout, c3.cout, c2.stride)) return LF_FRAME;
    return chain_supported(c2.cout, 0) ? LF_CHAIN : LF_SINGLE;
}

// Block `b` feeds the next block's conv1 directly - no cast in between - and that block's tail runs in the same form, so it knows where to find the t1 that
// a fused launch of `b` leaves for it.  Returns that conv1, or -1.
static int next_conv1(const pvr_encoder *e, size_t b, LaunchForm form) {
    if (b + 1 >= e->blocks.size() || e->blocks[b + 1].conv1 != e->blocks[b].conv3 + 1 || tail_form(e, e->blocks[b + 1]) != form) return -1;
    return e->blocks[b + 1].conv1;
}

static Launch &push(pvr_encoder *e, LaunchForm form, int op) {
    Launch l; l.form = form; l.conv2 = op;
    e->sched_fused.push_back(l);
    return e->sched_fused.back();
}

// An op as a launch of its own.  A convolution with few pixels and a deep K (layer3 / layer4's 1 x 1 and 3 x 3 at 14 x 14 and 7 x 7): conv_wfrag.hip may
// take it at run time (conv_wfrag_preferred: by the batch) - it reads the fragment-blocked copy of the weights
static void push_single(pvr_encoder *e, int i) {
    if (i < 0) return;
    ConvOp &op = e->ops[i];
    push(e, LF_SINGLE, i);
    if (op.is_conv() && !op.f32op && !op.from32 && op.h == op.w && op.h <= 14 && op.cout_real == op.cout && (int64_t)op.k * op.k * op.cin >= 512 &&
        conv_wfrag_supported(1, 1, op.cin, op.cout, op.k, op.k, op.pad, op.relu, op.out_f32))
        op.wfrag = true;
}

// Pass 1, per block.  A bottleneck of width 64 / 128 (layer1, layer2) runs as
// [conv1 unless the previous chain already produced it] [downsample] [chain: conv2 -> conv3 (+res) -> next conv1]; layer3's stride-1 bottlenecks as
// per-frame launches; layer3.0 / layer4.0's conv3 & downsample as one two-operand launch; the compression head's conv1 & downsample as one
// conv_split16 pair; everything else as a launch of its own.  ConvOp::wfrag marks the ops whose launches read the fragment-blocked weight image.
static void plan_blocks(pvr_encoder *e) {
    int cur_t1 = B_T1;                                          // where the next chain finds its t1: chains read one t1 buffer while they write the next conv1's to the other
    bool conv1_done = false;                                    // the previous block's launch ran this block's conv1
    int conv1_frame_out = -1;                                   // t1 buffer the previous per-frame launch wrote that conv1's output to
    for (size_t bi = 0; bi < e->blocks.size(); ++bi) {
        const Block &b = e->blocks[bi];
        const LaunchForm form = tail_form(e, b);
        const bool own_conv1 = !conv1_done;
        conv1_done = false;
        if (b.type == BK_HEAD) {
            // conv1 (+ ReLU) and the downsample convolution read the SAME fp32 tensor with the same geometry: one conv_split16 launch over
            // [W1 ; Wd] (128 couts), two outputs - the 205 / 103 MB input is read once
            const ConvOp &c1 = e->ops[b.conv1], &cd = e->ops[b.ds];
            if (c1.f32op && c1.split16 && cd.f32op && cd.split16) push(e, LF_PAIR, b.conv1).pair = b.ds;
            else { push_single(e, b.conv1); push_single(e, b.ds); }
            push_single(e, b.conv2);
        } else if (b.type == BK_BASIC) {
            for (int oi : {b.conv1, b.ds, b.conv2}) push_single(e, oi);
        } else if (form == LF_FRAME && own_conv1 && e->sw.frame_front1 && !e->sw.frame_next1) {
            // layer3's stride-1 bottlenecks as ONE launch per block: conv1 -> conv2 -> conv3 + identity of one 14 x 14 image per workgroup
            // (bneck_frame.hip with the block's own conv1 in front; PVR_FRAME_FRONT1=0: conv1 keeps its launch)
            Launch &l = push(e, LF_FRAME, b.conv2);
            l.conv1 = b.conv1; l.conv3 = b.conv3; l.t1_in = e->ops[b.conv1].out_buf;
            for (int oi : {l.conv1, l.conv2, l.conv3}) e->ops[oi].wfrag = true;
        } else {
            if (own_conv1) { push_single(e, b.conv1); cur_t1 = B_T1; }
            if (form == LF_FRAME) {
                // conv2 -> conv3 + residual of one 14 x 14 image per workgroup (bneck_frame.hip); with PVR_FRAME_NEXT1=1 the next block's conv1 rides in
                // the same launch (it then reads / writes the two t1 buffers in turns, as the layer1 / layer2 chains do)
                Launch &l = push(e, LF_FRAME, b.conv2);
                l.conv3 = b.conv3; l.t1_in = conv1_frame_out >= 0 ? conv1_frame_out : e->ops[b.conv2].in_buf;
                conv1_frame_out = -1;
                if (e->sw.frame_next1 && (l.next1 = next_conv1(e, bi, LF_FRAME)) >= 0) {
                    conv1_frame_out = l.t1_out = l.t1_in == B_T1 ? B_T2 : B_T1;
                    conv1_done = true;
                }
                for (int oi : {l.conv2, l.conv3, l.next1}) if (oi >= 0) e->ops[oi].wfrag = true;
            } else if (form == LF_CHAIN) {
                // The next block's conv1 rides in this chain only if that block is a chain itself: the chain leaves t1' in the OTHER of the two
                // t1 buffers (it reads one while it writes the next), which only a following chain knows to read (l.t1_in); a plain conv2 launch
                // reads its own in_buf.  (Round 3: with the fp32 residual stream of the compressed PVRs' parity plan starting at layer2, layer1's
                // last chain is followed by plain launches.)
                const ConvOp &c2 = e->ops[b.conv2];
                int next1 = next_conv1(e, bi, LF_CHAIN);
                if (next1 >= 0 && !chain_supported(c2.cout, e->ops[next1].cout)) next1 = -1;
                // layer1's block 0: its 64-channel stride-1 downsample is accumulated inside the chain's conv3 (PVR_CHAIN_DS=0: own launch) - in the instance
                // that carries a next conv1, so only with one; otherwise the downsample launches first
                const bool ds_inside = b.ds >= 0 && next1 >= 0 && e->sw.chain_ds && c2.stride == 1 &&
                                       chain_ds_supported(c2.cout, e->ops[next1].cout, e->ops[b.ds].cin, e->ops[b.ds].stride);
                if (!ds_inside) push_single(e, b.ds);
                Launch &l = push(e, LF_CHAIN, b.conv2);
                l.conv3 = b.conv3; l.t1_in = cur_t1; l.next1 = next1;
                if (ds_inside) l.ds = b.ds;
                if (next1 >= 0) {
                    cur_t1 = l.t1_out = cur_t1 == B_T1 ? B_T2 : B_T1;
                    conv1_done = true;
                }
            } else {
                push_single(e, b.conv2);
                // A stride-2 bottleneck outside the chains (layer3.0, layer4.0): its 1 x 1 downsample and the conv3 that adds it run as ONE two-operand
                // launch (conv_pp256 DUAL: K = conv3's channels, then the block input's) - the identity branch is accumulated in fp32 and never exists in
                // HBM (- 2 x 103 MB at layer3.0, - 2 x 51 MB at layer4.0 per 256 frames, one launch less).  PVR_DUAL_DS=0: separate launches.
                if (b.ds >= 0 && e->sw.dual_ds && plain16(e->ops[b.ds]) && plain16(e->ops[b.conv3])) push(e, LF_DUAL, b.conv3).ds = b.ds;
                else { push_single(e, b.ds); push_single(e, b.conv3); }
            }
        }
        push_single(e, b.cast);
    }
}

// Pass 2: which tails run on the wave form (chain_wave.hip)
static void plan_wave_forms(pvr_encoder *e) {
    for (Launch &l : e->sched_fused)
        if (l.form == LF_CHAIN) {
            const ConvOp &c2 = e->ops[l.conv2];
            l.wave = chain_uses_wave_form(e->sw, c2.cout, l.next1 >= 0 ? e->ops[l.next1].cout : 0, c2.stride, l.ds >= 0);
        }
}

// Pass 3: two consecutive wave-form tails hand y (the second one's residual) and t1' (its conv2 input) over in the blocked layout
// (chain_wave.hip): only when nothing else reads those two buffers in between - no tap, no other launch - and the geometry allows it.
static void plan_blocked_handoffs(pvr_encoder *e) {
    for (size_t a = 0; a + 1 < e->sched_fused.size(); ++a) {
        Launch &A = e->sched_fused[a], &B = e->sched_fused[a + 1];
        if (A.form != LF_CHAIN || B.form != LF_CHAIN || A.next1 < 0 || B.ds >= 0) continue;
        const ConvOp &a2 = e->ops[A.conv2], &a3 = e->ops[A.conv3], &b2 = e->ops[B.conv2], &b3 = e->ops[B.conv3];
        const int a_cmn = e->ops[A.next1].cout;
        if (!e->sw.chain_blocked) continue;
        if (B.t1_in != A.t1_out || b3.res_buf != a3.out_buf || !a3.tap.empty() || b2.h != a2.h / a2.stride || b2.w != a2.w / a2.stride || b2.stride != 1) continue;
        if (!A.wave && !B.wave) {
            // two block-form tails (layer2): y = the next residual travels blocked (16-byte accesses of a lane land in 512-byte runs);
            // t1' stays NHWC (the halo DMA wants contiguous pixel rows)
            if ((b2.h * b2.w) % 16 == 0) { A.out_blk = 1; B.in_blk = 1; }
            continue;
        }
        if (!A.wave || !B.wave) continue;
        if (!chain_wave_blocked_ok(a_cmn, a2.h, a2.w)) continue;
        A.out_blk = 1; B.in_blk = 1;
        // ... and when A is layer1's first tail (downsample inside), its conv2 input t1 can arrive blocked too: from conv1's own launch,
        // which directly precedes it (conv_expand.hip writes either layout; whether THAT kernel runs is known per forward: batch size)
        if (A.ds >= 0 && a > 0 && a2.w == 56 && e->sw.chain_wave_halo) {   // (the downsample tail reads a blocked t1 through the halo form only)
            Launch &C = e->sched_fused[a - 1];
            if (C.form == LF_SINGLE) {
                const ConvOp &c1 = e->ops[C.conv2];
                if (c1.is_conv() && !c1.f32op && c1.k == 1 && c1.stride == 1 && c1.out_buf == A.t1_in && c1.tap.empty() && c1.res_buf == B_NONE && !c1.out_f32 &&
                    c1.ksplit <= 1) { C.out_blk = 1; A.in_blk = 1; }
            }
        }
    }
}

// Pass 4: layer1.0.conv1 (1 x 1, 64 -> 64 on the pooled stem output) inside the fused stem (stem.hip, StemC1; round 6): the launch leaves the fused schedule; the
// forward hands the stem its weights, or - where the stem's register-pooling form does not run - launches the convolution itself in front of the plan
static void plan_stem_c1(pvr_encoder *e) {
    if (!e->sw.stem_conv1 || e->sched_fused.empty() || !(e->desc.arch == PVR_ARCH_RESNET50 || e->desc.arch == PVR_ARCH_RESNET50_L3 || e->desc.arch == PVR_ARCH_RESNET50_L4)) return;
    const Launch &L0 = e->sched_fused[0];
    if (L0.form != LF_SINGLE || L0.conv2 != 0) return;
    const ConvOp &c1 = e->ops[0];
    if (c1.role == R_CONV1 && !c1.f32op && !c1.from32 && c1.k == 1 && c1.stride == 1 && c1.cin == 64 && c1.cout == 64 && c1.cin_real == 64 && c1.cout_real == 64 && c1.relu == 1 &&
        c1.in_buf == B_X0 && c1.out_buf == B_T1 && c1.res_buf == B_NONE && !c1.out_f32 && c1.tap.empty() && c1.ksplit <= 1 && c1.h == 56) {
        e->stem_c1 = 0; e->stem_c1_blk = L0.out_blk;
        e->sched_fused.erase(e->sched_fused.begin());
    }
}

// Pass 5: a wave-form tail that carries the next block's conv1 and whose y has ONE other reader, a 1 x 1 stride-2 convolution (layer1.2 -> layer2.0's
// downsample): three quarters of y are never read.  The tail may store only the (even row, even column) pixels, compacted into the front of
// the same buffer, and the reader then runs at stride 1 over them (y_s2).  Whether a forward does so is decided per batch size (resolve_kinds:
// the reader must be conv_expand at both strides - the same K order, bit-identical) and per call (taps, debug stops and range checks see full y).
static void plan_y_s2(pvr_encoder *e) {
    if (!e->sw.strided_y) return;
    std::vector<Launch> &sc = e->sched_fused;
    for (size_t a = 0; a < sc.size(); ++a) {
        Launch &A = sc[a];
        if (A.form != LF_CHAIN || A.wave != 1 || A.next1 < 0 || A.ds >= 0) continue;
        const ConvOp &a2 = e->ops[A.conv2], &a3 = e->ops[A.conv3];
        if (a2.stride != 1 || !chain_wave_y_s2_ok(a2.cout, e->ops[A.next1].cout, a2.h, a2.w, A.out_blk)) continue;   // (a tap on y: forwards that stop there run LK_CHAIN)
        const int yb = a3.out_buf;
        int reader = -1, readers = 0;
        for (size_t b = a + 1; b < sc.size(); ++b) {       // every later read of yb until a launch writes it again
            const Launch &B = sc[b];
            bool writes = false;
            if (B.t1_in == yb) ++readers;
            for (int oi : {B.conv1, B.conv2, B.ds, B.conv3, B.next1, B.pair}) {   // (members in launch order: a read behind the write is the launch's own y)
                if (oi < 0) continue;
                const ConvOp &o = e->ops[oi];
                if (!writes && (o.in_buf == yb || o.res_buf == yb)) { ++readers; reader = (int)b; }
                writes |= o.out_buf == yb;
            }
            if (writes) break;
        }
        if (readers != 1) continue;
        const Launch &R = sc[reader];
        const ConvOp &r = e->ops[R.conv2];
        if (R.form != LF_SINGLE || R.out_blk || !r.is_conv() || r.f32op || r.from32 || r.k != 1 || r.stride != 2 || r.pad != 0 ||
            r.in_buf != yb || r.res_buf != B_NONE || r.out_f32 || r.ksplit > 1 || !r.tap.empty() || r.h != a2.h || r.w != a2.w || r.cin != a3.cout)
            continue;
        A.y_s2 = reader;
    }
}

// Both launch schedules: one launch per op, and the fused one (the passes above, in this order).
static void build_schedules(pvr_encoder *e) {
    const int n = (int)e->ops.size();
    for (int i = 0; i < n; ++i) { Launch l; l.conv2 = i; e->sched_plain.push_back(l); }
    if (stores_f32(e->desc.dtype) || e->desc.arch == PVR_ARCH_CLIP_RN50) { e->sched_fused = e->sched_plain; return; }   // (CLIP: pools between the convolutions)
    plan_blocks(e);
    plan_wave_forms(e);
    plan_blocked_handoffs(e);
    plan_stem_c1(e);
    plan_y_s2(e);
}

bool pooled_head(const pvr_encoder *enc) {   // global average pool of the fp32 last activation (vs C-major flatten of the compression heads)
    return enc->desc.arch == PVR_ARCH_RESNET50 || enc->desc.arch == PVR_ARCH_RESNET18 || enc->desc.arch == PVR_ARCH_RESNET34;
}

// Low-latency plan (pvr_encoder_set_low_latency; the online pattern of EmbeddingWrapper: N = 2 frames per environment step).
// A forward of <= 4 frames has 1-7 pixel tiles in layer3 / layer4, so every deep convolution is a handful of blocks each
// walking its whole K range alone: 21 such launches x 27 us were 65 % of a 0.88 ms N = 2 forward (rocprofv3,
// profiles/r02_small_batch_kernel_stats.csv).  Here K is cut into ranges of ~4 slices over blockIdx.y (conv_igemm split-K: fp32
// partial planes + a fixed-order reduce with bias / residual / ReLU).  The split depends on the layer's K only, so results do
// not depend on N within the plan; against the unsplit plan they differ by fp32 regrouping (<= 1 ulp of the storage type), which
// is why the plan is opt-in and batch-size independence of the default plan stays bit-exact.
int small_batch_ksplit(const pvr_encoder *enc, const ConvOp &op, int nb) {
    if (!enc->low_latency || nb > 4 || !op.is_conv() || op.f32op || op.from32 || op.ksplit > 1 || op.relu > 1 || (op.out_f32 & 2)) return 0;
    const int K = op.k * op.k * op.cin, nk = K / 64;
    if (nk < 8) return 0;                                        // K < 512: nothing to share
    const long long M = (long long)nb * op.ho() * op.ho(), blocks = ((M + 127) / 128) * ((op.cout + 127) / 128);
    if (blocks > 64) return 0;
    const int div = enc->sw.smallk_div;                          // K slices per block (PVR_SMALLK_DIV, read at create)
    int ks = nk / div;
    if (ks > (div >= 4 ? 16 : 32)) ks = div >= 4 ? 16 : 32;
    if ((size_t)ks * M * op.cout * sizeof(float) > SMALLK_BYTES) return 0;
    return ks;
}

// Which kernel launch `li` of the plan runs as for a forward of nb frames (allow_pool = false: the caller's output rows cannot take the
// pooled epilogue's 16-byte stores).  A pure function of the plan, the switches and nb: tabulated by resolve_kinds, off the hot path.
uint8_t resolve_kind(const pvr_encoder *enc, const std::vector<Launch> &plan, size_t li, int nb, bool allow_pool) {
    const Launch &l = plan[li];
    const ConvOp &op = enc->ops[l.out_op()];
    if (enc->desc.dtype == PVR_F32S) return LK_SPLIT16;          // one launch per convolution, whatever the batch: no fused plan, no split-K, no frame kernels
    const bool ll = enc->low_latency && nb <= 4;                 // (the low-latency plan covers forwards of <= 4 frames: small_batch_ksplit)
    const bool autoalgo = enc->sw.conv_algo == -1;
    switch (l.form) {
    case LF_FRAME:
        // small batches (a frame per workgroup leaves most CUs idle): the member convolutions as their own launches - bit-identical
        if (nb >= enc->sw.frame_min_n && !enc->low_latency) return l.conv1 >= 0 ? LK_FRAME_FRONT1 : LK_FRAME;
        return LK_FRAME_MEMBERS;
    case LF_DUAL: return (!ll && autoalgo) ? LK_DUAL : LK_DUAL_MEMBERS;
    case LF_CHAIN: return LK_CHAIN;
    case LF_PAIR: return LK_SPLIT16_PAIR;
    case LF_SINGLE: break;
    }
    if (op.role == R_CAST) return LK_CAST;
    if (op.f32op) return op.split16 ? LK_SPLIT16 : LK_F32;
    if (op.from32) return LK_SPLIT16_IN32;
    if (small_batch_ksplit(enc, op, nb)) return LK_SPLITK_SMALL;
    if (op.ksplit > 1) return LK_SPLITK;
    const int ho = op.ho(), wo = op.wo();
    if (l.out_blk && autoalgo && op.cin == 64 &&                 // (blocked output: the cin = 64 instances of conv_expand only)
        conv_expand_supported(enc->sw, (int64_t)nb * op.h * op.w, op.h, op.w, op.cin, op.cout, 1, 1, 1, 0, op.relu, 0, false))
        return LK_EXPAND_BLOCKED;
    if (allow_pool && enc->sw.pool_fuse && li + 1 == plan.size() && op.wfrag && pooled_head(enc) && enc->final_hw == 49 && op.h == 7 && op.w == 7 && op.k == 1 &&
        op.stride == 1 && op.relu == 1 && (op.out_f32 & 1) && !(op.out_f32 & 2) && op.res_buf != B_NONE && op.out_buf == B_F32 && enc->final_c == op.cout &&
        autoalgo && !ll)
        return LK_WFRAG_POOL;
    if (op.wfrag && autoalgo && !ll && conv_wfrag_preferred(enc->sw, (int64_t)nb * ho * wo, op.cin, op.cout, op.k, op.k) &&
        conv_wfrag_supported((int64_t)nb * ho * wo, (int64_t)nb * op.h * op.w * op.cin * 2, op.cin, op.cout, op.k, op.k, op.pad, op.relu, op.out_f32))
        return LK_WFRAG;
    return LK_CONV;
}

const std::vector<Launch> &cur_plan(const pvr_encoder *enc) { return enc->fuse ? enc->sched_fused : enc->sched_plain; }

// kinds[(nb - 1) * launches + i] for nb = 1 .. chunk: rebuilt whenever something it depends on changes (create, set_low_latency,
// debug_set_fusion, debug_set_switch, set_host_backend, check_range around its forward), so the table is always the current plan's
void resolve_kinds(pvr_encoder *enc) {
    const std::vector<Launch> &plan = cur_plan(enc);
    const int chunk = enc->desc.chunk;
    enc->kinds.assign((size_t)chunk * plan.size(), enc->desc.dtype == PVR_F32S ? LK_SPLIT16 : LK_CONV);
    if (stores_f32(enc->desc.dtype) || enc->desc.arch == PVR_ARCH_CLIP_RN50 || enc->vit || enc->rnd || enc->host) return;
    for (int nb = 1; nb <= chunk; ++nb)
        for (size_t i = 0; i < plan.size(); ++i) enc->kinds[(size_t)(nb - 1) * plan.size() + i] = resolve_kind(enc, plan, i, nb);
    // a tail that stores y only at its stride-2 reader's pixels (Launch::y_s2): where that reader runs on conv_expand at stride 2 and would at stride 1
    // over the compacted tensor - the two instances differ only in the address of a pixel, so the output is bit-identical
    for (int nb = 1; nb <= chunk; ++nb) {
        uint8_t *k = enc->kinds.data() + (size_t)(nb - 1) * plan.size();
        for (size_t i = 0; i < plan.size(); ++i) {
            const int j = plan[i].y_s2;
            if (j < 0 || k[i] != LK_CHAIN || k[j] != LK_CONV || enc->sw.conv_algo != -1) continue;
            const ConvOp &r = enc->ops[plan[j].conv2];
            const int64_t M = (int64_t)nb * (r.h / 2) * (r.w / 2);
            if (conv_expand_supported(enc->sw, M, r.h, r.w, r.cin, r.cout, 1, 1, 2, 0, r.relu, 0, false) &&
                conv_expand_supported(enc->sw, M, r.h / 2, r.w / 2, r.cin, r.cout, 1, 1, 1, 0, r.relu, 0, false)) {
                k[i] = LK_CHAIN_YS2;
                k[j] = LK_CONV_YS2;
            }
        }
    }
    // consecutive whole-bottleneck frame launches, each reading its predecessor's output (layer3.1 .. 3.5): one launch for the run (bneck_frame.hip RUN)
    if (enc->sw.frame_run)
        for (int nb = 1; nb <= chunk; ++nb) {
            uint8_t *k = enc->kinds.data() + (size_t)(nb - 1) * plan.size();
            for (size_t i = 0; i + 1 < plan.size(); ++i) {
                if (k[i] != LK_FRAME_FRONT1) continue;
                size_t j = i;
                while (j + 1 < plan.size() && j + 1 - i < 6 && k[j + 1] == LK_FRAME_FRONT1 &&
                       enc->ops[plan[j + 1].conv3].res_buf == enc->ops[plan[j].conv3].out_buf && enc->ops[plan[j + 1].conv1].in_buf == enc->ops[plan[j].conv3].out_buf) ++j;
                if (j > i) { k[i] = LK_FRAME_RUN; for (size_t t = i + 1; t <= j; ++t) k[t] = LK_FRAME_RUN_TAIL; }
                i = j;
            }
        }
}

// The whole plan of a handle, in pvr_encoder_create: ops, split-K, both schedules, the kinds table.
void plan_encoder(pvr_encoder *e) {
    if (e->desc.arch == PVR_ARCH_RESNET18 || e->desc.arch == PVR_ARCH_RESNET34) build_basic_resnet(e);
    else if (e->desc.arch == PVR_ARCH_CLIP_RN50) build_clip_rn50(e);
    else build_resnet50(e);
    e->buf_elems = (size_t)e->desc.chunk * 56 * 56 * 256;         // largest activation (layer1 output)
    for (ConvOp &op : e->ops)                                     // the fp32 stage / head of the parity plan and the readers of its fp32 stream, on the 16-bit MFMA
        op.split16 = e->desc.dtype == PVR_F32S ? op.is_conv()                  // the fp32-parity mode on the 16-bit MFMA: every convolution (pvr_encoder_create refuses a plan with a shape conv_split16 cannot take)
                                               : (op.f32op || op.from32) && e->desc.dtype == PVR_F16 && e->sw.split16 && conv_split16_supported(op.cin, op.cout, op.k);
    plan_splitk(e);
    build_schedules(e);
    e->fuse = e->sw.fuse != 0;
    resolve_kinds(e);
}

}  // namespace pvr

extern "C" {

// name of the kernel family launch `index` (the order pvr_encoder_profile reports) runs as in a forward of n frames; returns its length, 0 past the end
// (the plan exists from pvr_encoder_create on: a handle need not be finalized)
int32_t pvr_encoder_launch_kernel(const pvr_encoder *enc, int32_t n, int32_t index, char *buf, int32_t cap) {
    if (!enc || !buf || cap <= 0 || index < 3 || enc->vit || enc->rnd || enc->host || n < 1) return 0;
    const std::vector<Launch> &plan = cur_plan(enc);
    const int i = index - 3;
    if (i >= (int)plan.size()) return 0;
    const int nb = n < enc->desc.chunk ? n : enc->desc.chunk;
    const int kind = enc->kinds[(size_t)(nb - 1) * plan.size() + i];   // the forward's own table: whatever changes the plan or a switch rebuilds it (resolve_kinds)
    const char *nm = enc->desc.dtype == PVR_F32 ? "conv_f32" : launch_kind_name(kind);
    if (enc->desc.dtype != PVR_F32 && (kind == LK_CHAIN || kind == LK_CHAIN_YS2)) nm = plan[i].wave ? "chain_wave" : "bottleneck_chain";
    snprintf(buf, (size_t)cap, "%s", nm);
    return (int32_t)strlen(nm);
}

// name of launch `index` of the current plan (the order pvr_encoder_profile reports); returns the name's length, 0 past the end
int32_t pvr_encoder_launch_name(const pvr_encoder *enc, int32_t index, char *buf, int32_t cap) {
    if (!enc || !buf || cap <= 0 || index < 0) return 0;
    std::string nm;
    static const char *head[3] = {"preprocess", "stem", "maxpool"};
    if (index < 3) nm = head[index];
    else {
        const std::vector<Launch> &sc = cur_plan(enc);
        const int i = index - 3;
        if (i < (int)sc.size()) {
            nm = enc->ops[sc[i].conv1 >= 0 ? sc[i].conv1 : sc[i].conv2].conv;
            if (sc[i].conv1 >= 0) nm += "+conv2";
            if (sc[i].conv3 >= 0) nm += "+conv3";
            if (sc[i].ds >= 0 || sc[i].pair >= 0) nm += "&downsample";
            if (sc[i].next1 >= 0) nm += "+" + enc->ops[sc[i].next1].conv;
        } else if (i == (int)sc.size() && !enc->vit && !enc->rnd) nm = "pool/flatten";
    }
    snprintf(buf, (size_t)cap, "%s", nm.c_str());
    return (int32_t)nm.size();
}

}  // extern "C"
