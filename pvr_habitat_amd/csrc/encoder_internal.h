// Internal declarations shared by encoder.hip (ResNet50 family), vit.hip (CLIP ViT) and the kernel files whose launchers take the encoder's switches.
#pragma once
#include <map>
#include <string>
#include <vector>
#include <cmath>
#include "common.h"
#include "chain_params.h"

namespace pvr {

// Every A/B switch of the encoder path, read from the environment ONCE per encoder (pvr_encoder_create: read_switches) - never on the forward path, and
// nowhere else: the planner and the launchers take their choices from here (launchers: `sw`).  The ones marked (live) can be changed on a finalized encoder
// with pvr_encoder_debug_set_switch; the others shape the plan or its launches and are fixed at create.  The pvr_op_* entry points have no handle: they
// share one process-level instance, op_switches().
struct PlanSwitches {
    int pool_fuse = 1;        // PVR_POOL_FUSE (live): the pooled form of conv_wfrag for the trunk's last launch
    int stem_u8 = 1;          // PVR_STEM_U8 (live): the fused stem reads uint8 frames itself when no resize is needed
    int stem_lds = 1;         // PVR_STEM_LDS: the round-3 forms of the fused stem (0: round 2's stem_pool_kernel - no uint8 form, no conv1 inside)
    int stem_regpool = 1;     // PVR_STEM_REGPOOL (live): the stem's max pool in registers (0: the LDS-tile pooling of rounds 3-5; bit-identical)
    int frame_front1 = 1;     // PVR_FRAME_FRONT1: layer3's per-frame launches carry their own conv1
    int frame_next1 = 0;      // PVR_FRAME_NEXT1: ... carry the NEXT block's conv1 instead (measured slower)
    int frame_bneck = 1;      // PVR_FRAME_BNECK: layer3's per-frame launches (bneck_frame.hip) at all
    int bneck_stagger = 0;    // PVR_FRAME_STAGGER (EXPERIMENTS=1 builds only): odd workgroups of a single bottleneck's frame launch start late
    int dual_ds = 1;          // PVR_DUAL_DS: conv3 & downsample of layer3.0 / layer4.0 as one two-operand launch
    int chain_ds = 1;         // PVR_CHAIN_DS: layer1.0's downsample inside the chain
    int chain_blocked = 1;    // PVR_CHAIN_BLOCKED: blocked hand-off between consecutive tails
    int chain_halo = 1;       // PVR_CHAIN_HALO: the block form's phase A through the LDS halo (0: per-tap global loads; bit-identical)
    int chain_ds_occ = 3;     // PVR_CHAIN_DS_OCC: blocks per CU of the block form's downsample instance (3: capped at 168 VGPRs, else 2)
    int chain_pfk = 12;       // PVR_CHAIN_PFK: slice of phase A at which the Cm = 128 block form issues phase B's first prefetch (-1: in front of phase A)
    int chain_cfg = 12;       // PVR_CHAIN_CFG: 10 * RD + OCC of the block form's Cm = 64 instances
    int chain_wave = 1;       // PVR_CHAIN_WAVE: the wave forms of the tails at all (0: every tail on the block form; bit-identical)
    int chain_wave_halo = 1;  // PVR_CHAIN_WAVE_HALO: the wave form reads blocked inputs through the halo registers (0: the per-K-step load ring)
    int chain_wave_128 = 1;   // PVR_CHAIN_WAVE_128: the wave form for layer1's last tail (next conv1 128 wide)
    int strided_y = 1;        // PVR_STRIDED_Y: a tail whose y is read only by a 1x1 stride-2 downsample stores just those pixels (layer1.2 -> layer2.0; bit-identical)
    int splitk = 1;           // PVR_SPLITK: planned split-K of the *_l4 head
    int smallk_div = 4;       // PVR_SMALLK_DIV: K slices per block of the low-latency plan
    int frame_run = 0;        // PVR_FRAME_RUN (live, opt-in: measured equal): consecutive whole-bottleneck frame launches (layer3.1 .. 3.5) as one launch
    int frame_stagger = 0;    // PVR_FRAME_RUN_STAGGER (live): odd workgroups of that launch start this many x 8128 cycles late
    int frame_min_n = 128;    // PVR_FRAME_MIN_N (live): frames per forward from which layer3's per-frame launches run as such
    int stem_conv1 = 1;       // PVR_STEM_CONV1: layer1.0.conv1 runs inside the fused stem (no launch of its own; round 6)
    int split16 = 1;          // PVR_SPLIT16: the fp32 stage / head of the compressed PVRs' parity plan on the 16-bit MFMA (0: f32-input MFMA)
    int resid32 = 1;          // PVR_RESID32: fp32 residual stream of that plan (0: all-16-bit plan)
    int tail_f32 = 1;         // PVR_TAIL_F32: its last trunk stage entirely in fp32
    int fuse = 1;             // PVR_FUSE: the fused schedule (0: one launch per convolution; also pvr_encoder_debug_set_fusion)
    int conv_algo = -1;       // PVR_CONV_ALGO (live): launch_conv's kernel: -1 auto by shape, 0 conv_igemm only, 1 / 2 / 3 conv_pp256 with 256- / 128- / 224-pixel tiles
    int conv_halo = 1;        // PVR_CONV_HALO: the 3x3 stride-1 convolutions on conv3x3_halo.hip (0: conv_igemm; bit-identical)
    int conv_expand = 1;      // PVR_CONV_EXPAND: the 1x1 convolutions conv_expand.hip accepts on it (0: conv_igemm / conv_pp256; bit-identical)
    int conv_wfrag = 1;       // PVR_CONV_WFRAG: the few-pixel deep-K launches on conv_wfrag.hip (2: every launch it accepts)
    int wfrag_ko = 0;         // PVR_WFRAG_KO (EXPERIMENTS=1 builds only): timing knock-out instance of conv_wfrag
    int igemm_nk4 = 1;        // PVR_IGEMM_NK4: conv_igemm's four-slice instance for the K = 256 1x1 convolutions with residual (bit-identical)
    int igemm_bm64 = 0;       // PVR_IGEMM_BM64: 64-pixel tiles for those convolutions (experiment)
    int pp_bm224 = 1;         // PVR_PP_BM224: conv_pp256's 224-pixel tile where it needs fewer CU-rounds (0 off, 2 round 2's rows-only rule)
    int pp_persist = 384;     // PVR_PP_PERSIST: tiles per launch from which conv_pp256 runs persistent (0 never)
};
void read_switches(PlanSwitches &sw);
PlanSwitches &op_switches();   // the pvr_op_* entry points' instance: read_switches on first use; pvr_debug_set_conv_algo changes it

pvr_status launch_preprocess(const uint8_t *, int, int, int, int, int, void *, int, hipStream_t, int crop_pos = 0);
void resized_size(int h, int w, int size, int *rh, int *rw);     // torchvision resize(int size): smaller edge -> size
// frames -> Resize -> a window per frame (windows: n x (top, left) int32 on the device, clamped in the kernel) -> the dense fp32 NHWC4 image, one launch
pvr_status launch_preprocess_windows(const uint8_t *frames, int n, int h, int w, int resize, int crop, const float *mean, const float *std_,
                                     const int32_t *windows, float *out, hipStream_t stream);
// the same with colour jitter per frame (color: n x (float b, c, s, int32 order); gray_sums: n uint32 of scratch), as two launches: stage 0 zeroes the
// sums and adds every frame's gray values before contrast, stage 1 writes the image; each checks every argument before it launches
pvr_status launch_color_stage(int stage, const uint8_t *frames, int n, int h, int w, int resize, int crop, const float *mean, const float *std_,
                              const int32_t *windows, const void *color, uint32_t *gray_sums, float *out, hipStream_t stream);
// frames -> each frame's own rectangle (rects: n x (top, left, height, width) int32 on the device, in the h x w frame, clamped in the kernel) resized to
// crop x crop -> the dense fp32 NHWC4 image, one launch; and the same with colour jitter, as launch_color_stage's two launches
pvr_status launch_preprocess_rects(const uint8_t *frames, int n, int h, int w, int crop, const float *mean, const float *std_, const int32_t *rects,
                                   float *out, hipStream_t stream);
pvr_status launch_color_stage_rects(int stage, const uint8_t *frames, int n, int h, int w, int crop, const float *mean, const float *std_,
                                    const int32_t *rects, const void *color, uint32_t *gray_sums, float *out, hipStream_t stream);
// the staged image path (grayscale and blur): "colour stats" as above with either source, "stage image" - the source's uint8 pixels after the colour ops,
// 4 bytes per pixel, into the caller's (n, crop, crop, 4) scratch - and "blur normalize" - grayscale, GaussianBlur(23, sigma), /255 and Normalize per
// frame by blur: n x (float sigma, int32 gray).  Exactly one of windows and rects is non-null
pvr_status launch_staged_color_stats(const uint8_t *frames, int n, int h, int w, int resize, int crop, const int32_t *windows, const int32_t *rects,
                                     const void *color, uint32_t *gray_sums, void *staged, hipStream_t stream);
pvr_status launch_stage_image(const uint8_t *frames, int n, int h, int w, int resize, int crop, const int32_t *windows, const int32_t *rects,
                              const void *color, uint32_t *gray_sums, void *staged, hipStream_t stream);
pvr_status launch_blur_normalize(const void *staged, int n, int crop, const float *mean, const float *std_, const void *blur, float *out,
                                 hipStream_t stream);
pvr_status launch_stem(const void *, const void *, const float *, void *, int, int, int, hipStream_t);
pvr_status launch_maxpool(const void *, void *, int, int, int, int, int, hipStream_t);
// (c1_*: layer1.0.conv1 inside the stem - stem.hip, StemC1; only when stem_conv1_capable(sw))
pvr_status launch_stem_pool(const PlanSwitches &sw, const void *, const void *, const float *, void *, int, int, int, hipStream_t, const void *c1_w = nullptr,
                            const float *c1_b = nullptr, void *c1_t1 = nullptr, int c1_blk = 0);
bool stem_pool_u8_ok(const void *, int, int, int, int);   // geometry only; the PVR_STEM_U8 / PVR_STEM_LDS switches live in PlanSwitches
pvr_status launch_stem_pool_u8(const PlanSwitches &sw, const uint8_t *, int, int, int, int, int, const void *, const float *, void *, int, hipStream_t,
                               const void *c1_w = nullptr, const float *c1_b = nullptr, void *c1_t1 = nullptr, int c1_blk = 0);
bool stem_conv1_capable(const PlanSwitches &sw);
void stem_c1_pack(const u16 *w, u16 *img);
void preprocess_geometry(int h, int w, int resize, int crop, int crop_pos, int *resize_needed, int *top, int *left);
pvr_status launch_avgpool(const void *, float *, int64_t, int, int, int, int, int, hipStream_t);
pvr_status launch_nhwc_to_chw(const float *, float *, int64_t, int, int, int, int, hipStream_t);
pvr_status launch_h_to_f32(const void *, float *, size_t, int, hipStream_t);
pvr_status launch_f32_to_h(const float *, void *, size_t, int, hipStream_t);
pvr_status launch_conv_splitk(const void *, const void *, const float *, const void *, void *, const void *, float *, int, int, int, int, int, int,
                              int, int, int, int, int, int, int, hipStream_t);
pvr_status launch_conv(const PlanSwitches &sw, const void *, const void *, const float *, const void *, void *, const void *, int, int, int, int,
                       int, int, int, int, int, int, int, int, hipStream_t);

// conv_expand.hip: persistent weight-stationary 1x1 convolutions (out_blk: blocked output layout for chain_wave.hip)
bool conv_expand_supported(const PlanSwitches &sw, int64_t M, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, int relu, int out_f32, bool has_res);
pvr_status launch_conv_expand(const void *in, const void *wgt, const float *bias, const void *res, void *out, int n, int h, int w, int cin,
                              int cout, int stride, int relu, int dtype, hipStream_t stream, int out_blk = 0);

// conv_pp256.hip: 256x256-tile ping-pong kernel for deep-K convolutions / linear layers
bool pp256_supported(int64_t M, int cin, int cout, int kh, int kw, int64_t in_bytes, int64_t w_bytes, int64_t out_bytes, int64_t res_bytes);
pvr_status launch_conv_pp256(const PlanSwitches &sw, const void *in, const void *wgt, const float *bias, const void *res, void *out, int n, int h, int w, int cin,
                             int cout, int kh, int kw, int stride, int pad, int act, int out_f32, int res_f32, int dtype, int bm, hipStream_t stream,
                             const void *in2 = nullptr, int h2 = 0, int w2 = 0, int cin2 = 0, int stride2 = 1);

// bneck_frame.hip: per-frame fused tail of the layer3 bottlenecks (conv2 -> conv3 + residual [-> the next block's conv1]); weights in the fragment-blocked layout
bool bneck_frame_supported(const PlanSwitches &sw, int n, int h, int w, int cm, int cout, int stride);
pvr_status launch_pack_frag_weights(const void *w, void *out, int rows, int K, hipStream_t stream);
pvr_status launch_bneck_frame(const PlanSwitches &sw, const void *t1, const void *w2p, const float *b2, const void *w3p, const float *b3, const void *res, void *y,
                              void *t2_out, int n, int phases, int dtype, hipStream_t stream, unsigned long long *stamps = nullptr,
                              const void *w1np = nullptr, const float *b1n = nullptr, void *t1n = nullptr, const void *w1fp = nullptr, const float *b1f = nullptr);
// round 6: consecutive whole bottlenecks of the stage per frame in ONE launch (blocks[k + 1].res == blocks[k].y); odd workgroups start `stagger` x 8128 cycles late
struct BFBlk {
    const unsigned short *w1f, *w2, *w3, *res;
    const float *b1f, *b2, *b3;
    unsigned short *y;
};
pvr_status launch_bneck_frame_run(const BFBlk *blocks, int nblk, int n, int dtype, hipStream_t stream, int stagger);

// conv_wfrag.hip: implicit GEMM in 112-pixel x 256-cout tiles with the weights read from L2 as MFMA fragments (layer4 at batch 256)
bool conv_wfrag_supported(int64_t M, int64_t in_bytes, int cin, int cout, int kh, int kw, int pad, int act, int out_f32);
bool conv_wfrag_preferred(const PlanSwitches &sw, int64_t M, int cin, int cout, int kh, int kw);
pvr_status launch_conv_wfrag(const PlanSwitches &sw, const void *in, const void *wp, const float *bias, const void *res, void *out, int n, int h, int w, int cin, int cout,
                             int kh, int kw, int stride, int pad, int act, int out_f32, int dtype, hipStream_t stream, float *pool_out = nullptr,
                             int64_t pool_stride = 0);

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// the two fp32-storage compute types: PVR_F32 multiplies on the f32-input MFMA, PVR_F32S on the 16-bit MFMA as exact (hi, lo) split products (conv_split16.hip,
// stem_split16.hip).  Workspace, weights layout, schedule, taps and profiling are the same for both
inline bool stores_f32(int dtype) { return dtype == PVR_F32 || dtype == PVR_F32S; }

constexpr int PVR_MAX_LANES = 4;
// B_Y0 / B_Y1: fp32 residual stream of the compressed PVRs' parity plan (allocated only for that plan); B_STEM: the lane's d_stem (112x112x64), not in buf[]
enum BufId { B_NONE = -1, B_X0 = 0, B_X1, B_T1, B_T2, B_DS, B_F32, B_Y0, B_Y1, B_COUNT, B_STEM = B_COUNT };

// What an op of the plan is: set by the builder that emits it (encoder_plan.hip).  The convolutions come first (ConvOp::is_conv).
enum OpRole : uint8_t {
    R_CONV1, R_CONV2, R_CONV3, R_DOWNSAMPLE,        // of a bottleneck or a basic block
    R_HEAD_CONV1, R_HEAD_DOWNSAMPLE, R_HEAD_CONV2,  // of the compression head (*_l3 / *_l4)
    R_STEM_CONV2, R_STEM_CONV3,                     // CLIP ModifiedResNet's second and third stem convolution
    R_AVGPOOL2,                                     // AvgPool2d(2) on NHWC 16-bit (CLIP ModifiedResNet; cin = channels)
    R_CAST,                                         // fp32 -> 16-bit copy
};

inline int conv_out_size(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

struct ConvOp {
    std::string conv, bn;          // state_dict prefixes (weights, launch names): the plan never parses them
    OpRole role = R_CONV1;
    int in_buf, out_buf, res_buf;
    int h, w, cin, cin_real, cout, cout_real, k, stride, pad, relu, out_f32;
    bool is_conv() const { return role < R_AVGPOOL2; }
    int ho() const { return conv_out_size(h, k, stride, pad); }
    int wo() const { return conv_out_size(w, k, stride, pad); }
    bool f32op = false;            // convolution on fp32 buffers with fp32 weights on the f32-input MFMA (conv_f32.hip) inside a 16-bit plan
    bool from32 = false;           // a 16-bit convolution (16-bit weights, one MFMA per product) whose INPUT is the fp32 residual stream: conv_split16's single-term
                                   // form rounds the operand in its staging pass - the fp32 -> 16-bit copy launch of the stream is gone (round 6)
    // plan facts, set by the planner at create (encoder_plan.hip) - finalize makes the device images they call for
    bool split16 = false;          // an f32op / from32 convolution of an f16 plan, or any convolution of a PVR_F32S plan: runs on conv_split16.hip (d_wsp)
    bool wfrag = false;            // a per-frame launch's member, or a stand-alone launch conv_wfrag.hip may take by the batch: reads d_wfb
    u16 *d_w = nullptr;
    u16 *d_wp = nullptr;           // row-permuted copy for the fused bottleneck chain (bottleneck_chain.hip)
    u16 *d_wfb = nullptr;          // fragment-blocked copy of d_w for the per-frame layer3 tail (bneck_frame.hip: launch_pack_frag_weights)
    u16 *d_wpb = nullptr;          // ... and that copy in the blocked layout [row >> 4][cin >> 3][row & 15][8] (chain_wave.hip reads W3 / Wd pieces from L2)
    std::vector<u16> h_w;          // host copy, kept until finalize has built the packed copies (prepare_weights)
    float *d_wf = nullptr;         // fp32 weights (PVR_F32 mode; PVR_F32S: only until finalize has packed d_wsp from them)
    u16 *d_wsp_pair = nullptr;     // compression head: [conv1 ; downsample] rows as ONE split weight image (both read the same fp32 input: one launch, round 6)
    float *d_b_pair = nullptr;
    u16 *d_wsp = nullptr;          // fp32 weights as (hi, lo) f16 fragment pairs (conv_split16.hip: the f32op convolutions of an f16 plan)
    float *d_b = nullptr;
    std::vector<float> h_b;        // host copy of the bias (same lifetime as h_w)
    float *d_bsum = nullptr;       // conv3 of a block whose downsample runs inside the chain / the two-operand launch: b3 + b_downsample
    u16 *d_wcat = nullptr;         // conv3 of a two-operand launch (conv_pp256 DUAL): [W3 | W_downsample] rows, (cout_pad, cin + cin_downsample)
    std::string tap;               // non-empty: output of this op is the named tap
    int ksplit = 0, ks_buf = B_NONE;   // split-K launch (conv_igemm.hip): number of K ranges, workspace buffer that is dead at this op
};

// A residual block as its builder emitted it: indices into ops, -1 where the block has no such op.  The planner schedules blocks (encoder_plan.hip: plan_blocks).
enum BlockType : uint8_t { BK_BOTTLENECK, BK_BASIC, BK_HEAD };   // conv1 1x1 -> conv2 3x3 -> conv3 1x1; conv1 3x3 -> conv2 3x3; the compression head
struct Block {
    BlockType type;
    int stage, index;                           // layer`stage + 1`.`index`
    int conv1 = -1, conv2 = -1, ds = -1, conv3 = -1;
    int cast = -1;                              // the fp32 -> 16-bit copy of the block's output, when one follows it
};

// one launch of the forward plan
enum LaunchForm : uint8_t {
    LF_SINGLE,   // ops[conv2] alone, whatever its role
    LF_CHAIN,    // fused bottleneck tail: conv2 3x3 -> conv3 1x1 + residual [-> the next block's conv1 1x1] (bottleneck_chain.hip, chain_wave.hip)
    LF_FRAME,    // per-frame form (bneck_frame.hip, layer3): [conv1 ->] conv2 -> conv3 + residual [-> next1] of one 14 x 14 image per workgroup
    LF_DUAL,     // ops[conv2] is a conv3 that runs as conv_pp256's two-operand launch with the block's downsample ops[ds] (layer3.0 / layer4.0)
    LF_PAIR,     // conv_split16 pair: ops[conv2] and ops[pair] read the same fp32 input and run as one launch (the compression head)
};
struct Launch {
    LaunchForm form = LF_SINGLE;
    int conv2 = -1, conv3 = -1, next1 = -1;   // indices into ops; conv3 / next1: chain and frame members
    int ds = -1;                              // chain: the block's downsample convolution, accumulated inside conv3 (no launch of its own); dual: see LF_DUAL
    int t1_in = B_NONE, t1_out = B_NONE;      // chain, frame: buffer holding conv2's input / receiving the next block's conv1 output
    int wave = 0;                             // chain: 1 the wave form runs it (chain_wave.hip), 0 the block form
    int conv1 = -1;                           // frame: the block's own conv1 runs in front, inside the launch (the launch reads the block input)
    int pair = -1;                            // pair: the second convolution
    int in_blk = 0, out_blk = 0;              // chain, wave form: t1 + residual / y + t1' travel in the blocked layout between two such launches (chain_wave.hip);
                                              // block form: out_blk 1 = y blocked (t1' stays NHWC)
    int y_s2 = -1;                            // chain, wave form: index of the plan's only other reader of y, a 1 x 1 stride-2 convolution - plain forwards store
                                              // just the (even row, even column) pixels of y, compacted to (n, h / 2, w / 2, c), and that launch reads them at stride 1
    int out_op() const { return form == LF_CHAIN || form == LF_FRAME ? conv3 : conv2; }   // the op whose output (and residual) the launch writes
};

// What one launch of the plan runs as for a forward of nb frames: resolved off the hot path (resolve_kinds: create, set_low_latency,
// debug_set_fusion, debug_set_switch), one byte per (nb, launch); the forward is a switch over these.
enum LaunchKind : uint8_t {
    LK_CONV = 0,          // launch_conv (conv_igemm.hip picks igemm / pp256 / expand / halo by shape)
    LK_FRAME_FRONT1,      // bneck_frame: conv1 -> conv2 -> conv3 + identity of one 14 x 14 image per workgroup
    LK_FRAME,             // bneck_frame: conv2 -> conv3 + identity [-> next conv1]
    LK_FRAME_RUN,         // round 6: the first of >= 2 consecutive LK_FRAME_FRONT1 launches - ONE launch takes every frame through all of them
    LK_FRAME_RUN_TAIL,    //          ... and the others (no launch of their own)
    LK_FRAME_MEMBERS,     // the member convolutions of a per-frame launch as their own launches (small forwards)
    LK_DUAL,              // conv_pp256 two-operand launch: conv3 & the stride-2 downsample
    LK_DUAL_MEMBERS,      // ... as two launches (low-latency plan, PVR_CONV_ALGO)
    LK_CHAIN,             // bottleneck_chain / chain_wave: conv2 -> conv3 (+ residual / downsample) -> next conv1
    LK_CAST,              // fp32 -> 16-bit copy
    LK_F32,               // conv_f32: fp32 operands on the f32-input MFMA
    LK_SPLIT16,           // conv_split16: fp32 operands as 16-bit (hi, lo) pairs on the 16-bit MFMA
    LK_SPLIT16_PAIR,      // ... two convolutions of the same input in one launch (the compression head's conv1 & downsample)
    LK_SPLIT16_IN32,      // ... single-term form: a 16-bit convolution that reads the fp32 residual stream itself
    LK_SPLITK_SMALL,      // low-latency plan: split-K over the lane's scratch
    LK_SPLITK,            // planned split-K (the *_l4 compression head)
    LK_EXPAND_BLOCKED,    // conv_expand writing the blocked layout in front of a wave-form tail
    LK_WFRAG_POOL,        // conv_wfrag with AdaptiveAvgPool2d(1) in the epilogue
    LK_WFRAG,             // conv_wfrag
    LK_CHAIN_YS2,         // LK_CHAIN storing y only at the pixels its stride-2 reader takes (Launch::y_s2; plain forwards: no tap, stop or range check)
    LK_CONV_YS2,          // ... and that reader: conv_expand at stride 1 over the compacted y
    LK_COUNT
};
const char *launch_kind_name(int k);


// Resize(resize_to, bicubic) + CenterCrop(res) of uint8 frames (vit.hip): the resampling tables, the frame size they were built for and the per-lane
// temporaries.  A ViT plan has one, a CLIP RN50 encoder has one.  aa_prepare rebuilds it when the frame size changes.
struct Resizer {
    int res = 224, resize_to = 224;
    int h = 0, w = 0, rh = 0, rw = 0, maxk_h = 0, maxk_w = 0;   // frame size of the tables (0: none yet), size after Resize, taps per output index
    int *xmin = nullptr, *xsize = nullptr, *ymin = nullptr, *ysize = nullptr;
    float *wx = nullptr, *wy = nullptr;
    struct Tmp { float *tmp = nullptr; uint8_t *u8 = nullptr; } lane[PVR_MAX_LANES];   // horizontal pass (fp32), resized crop (uint8)
};

}  // namespace pvr

using namespace pvr;

namespace pvr { struct HostPlan; }

struct pvr_encoder {
    pvr_encoder_desc desc;
    std::map<std::string, HostTensor> weights;
    std::vector<ConvOp> ops;
    std::vector<Block> blocks;                      // the residual blocks of ops, in order (the ops outside them: CLIP's stem convolutions and pools)
    std::vector<Launch> sched_plain, sched_fused;   // one launch per op / with the layer1-layer2 bottleneck tails fused
    bool fuse = true;                               // PVR_FUSE=0 or pvr_encoder_debug_set_fusion(enc, 0) selects sched_plain
    bool low_latency = false;                       // pvr_encoder_set_low_latency: split-K plan for forwards of <= 4 frames
    PlanSwitches sw;                                // environment switches, read once in pvr_encoder_create
    int stem_c1 = -1;                               // fused schedule: ops[stem_c1] = layer1.0.conv1 has no launch - the stem runs it (stem.hip, StemC1) or, where that
    int stem_c1_blk = 0;                            // form does not apply, the forward launches it in front of the plan; _blk: the tail behind it reads t1 blocked
    u16 *d_stem_c1w = nullptr;                      // its weights as the stem's fragment image (stem_c1_pack)
    std::vector<uint8_t> kinds;                     // LaunchKind of launch i for a forward of nb frames: kinds[(nb - 1) * plan.size() + i] (resolve_kinds)
    bool last_pooled = false;                       // the last forward wrote the pooled rows from the last convolution: the B_F32 tap does not exist
    bool tail32 = false;                            // round 3: + the last trunk stage entirely in fp32 (conv_f32.hip), fp32 stream one stage earlier
    bool resid32 = false;                           // compressed PVRs, f16: fp32 residual stream from layer3 on + fp32 compression head
    bool finalized = false;
    int out_size = 0;
    int final_hw = 0, final_c = 0, final_creal = 0;   // geometry of the last activation
    // device
    u16 *d_stem_w = nullptr, *d_zero = nullptr;
    float *d_stem_b = nullptr, *d_stem_wf = nullptr;   // fp32 mode: [64][49][4] stem weights (PVR_F32S: d_stem_w holds the split image of the [64][7][8][4] weights)
    size_t buf_elems = 0;
    // Everything that exists once per lane (pvr_encoder_forward_lane keeps up to PVR_MAX_LANES batches in flight, each on its own activation workspace).  A forward
    // is given its lane (encoder.hip: get_lane); lane 0 is made at finalize, the others on first use.  The ViT plans keep their workspaces in vit.hip (pvr_vit::Ws)
    // and the 'random' PVR has a single one: of a Lane they use the event and the stream only.
    struct Lane {
        u16 *d_img = nullptr, *d_stem = nullptr;       // zero-bordered 16-bit image (border = conv1 padding, written once at allocation); 112x112x64 stem output
        float *d_imgf = nullptr;                       // fp32 modes: normalised NHWC4 image (PVR_F32S: zero-bordered (crop + 6, crop + 8), border written once at allocation)
        void *buf[B_COUNT] = {nullptr};
        float *d_smallk = nullptr;                     // the low-latency plan's fp32 partial planes (pvr_encoder_set_low_latency / finalize / first use of the lane: never in a forward)
        float *ap_rows = nullptr;                      // CLIP RN50: this lane's rows of ap_out (not owned)
        hipEvent_t done = nullptr;                     // recorded after each forward on the lane; the next forward on it waits
        hipStream_t stream = nullptr;                  // stream of that forward (no wait when the stream is the same)
        bool valid = false;                            // the workspace exists
    } lanes[PVR_MAX_LANES];
    int last_lane = 0;                               // the lane the last forward ran on: the taps read its workspace, with that forward's last_n
    int crop_pos = 0;                                // 0 centre (reference), 1..4 corner crops (pvr_encoder_set_crop_position)
    int last_n = 0;
    std::string stop_after;                                          // debug: end the forward after this tap
    std::map<std::string, std::pair<int, std::vector<int>>> taps;   // name -> (buf, {h,w,c,is_f32})
    // CLIP RN50 (clip_rn50.hip): antialiased-bicubic resizer, attention-pool parameters
    Resizer resizer;
    u16 *ap_wqkv = nullptr, *ap_wc = nullptr;
    float *ap_bqkv = nullptr, *ap_bc = nullptr, *ap_pos = nullptr, *ap_out = nullptr;
    struct pvr_vit *vit = nullptr;                                   // CLIP ViT plan (vit.hip) when arch >= PVR_ARCH_CLIP_VIT_B32
    bool host = false;                                               // pvr_encoder_set_host_backend: CPU plan (host_encoder.hip), host pointers in / out
    struct pvr::HostPlan *hplan = nullptr;
    struct pvr_random5 *rnd = nullptr;                               // 'random' 5-conv PVR (random_pvr.hip)
};


namespace pvr {
// encoder_plan.hip: the ResNet family's launch plan - ops, split-K, both schedules, the kinds table.  Host arithmetic on the desc and the switches only (no
// weights, no device), so pvr_encoder_create calls it; pvr_encoder_finalize prepares what the plan's launches read (encoder.hip: prepare_weights).
void plan_encoder(pvr_encoder *e);
void resolve_kinds(pvr_encoder *enc);                          // again after low_latency, fuse or a live switch changed
uint8_t resolve_kind(const pvr_encoder *enc, const std::vector<Launch> &plan, size_t li, int nb, bool allow_pool = true);
const std::vector<Launch> &cur_plan(const pvr_encoder *enc);
bool pooled_head(const pvr_encoder *enc);
constexpr size_t SMALLK_BYTES = (size_t)32 << 20;               // the low-latency plan's fp32 partial planes, per lane
int small_batch_ksplit(const pvr_encoder *enc, const ConvOp &op, int nb);
bool conv_split16_supported(int cin, int cout, int k);         // conv_split16.hip
const HostTensor *enc_find(pvr_encoder *e, const std::string &name);
pvr_status enc_need(pvr_encoder *e, const std::string &name, const HostTensor **out, size_t numel);
template <typename T>
pvr_status enc_upload(T **dptr, const std::vector<T> &h) {
    PVR_HIP_TRY(hipMalloc((void **)dptr, h.size() * sizeof(T)));
    PVR_HIP_TRY(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return PVR_OK;
}
// conv_f32.hip (PVR_F32 reference-precision mode) and the fp32 normaliser of random_pvr.hip
pvr_status launch_conv_f32(const float *, const float *, const float *, const float *, float *, int, int, int, int, int, int, int, int, int, hipStream_t);
// (raw: the convolution alone, no bias and no ReLU - the trainable encoder's conv1, encoder_train.hip)
pvr_status launch_stem_f32(const float *, const float *, const float *, float *, int, int, hipStream_t, bool raw = false);
pvr_status launch_maxpool_f32(const float *, float *, int, int, int, int, hipStream_t);
// (padded: the output in the zero-bordered (n, crop + 6, crop + 8, 4) layout stem_split16.hip reads, border untouched)
pvr_status launch_normalize_nhwc4(const void *img_h, float *out, int n, int crop, const float *mean, const float *std_, int dtype, hipStream_t, bool padded = false);
// stem_split16.hip (PVR_F32S: conv1 as the exact split product on the 16-bit MFMA)
pvr_status launch_stem_split16(const float *img_padded, const void *wsp, const float *bias, float *out, int n, int S, hipStream_t);
long long stem_split16_launches();
// random_pvr.hip
pvr_status random5_create(pvr_encoder *e);
pvr_status random5_finalize(pvr_encoder *e);
pvr_status random5_forward(pvr_encoder *e, const uint8_t *frames, int n, int h, int w, float *out, int64_t out_stride, hipStream_t st);
void random5_destroy(pvr_encoder *e);
// host_encoder.hip (CPU plan behind the same ABI)
pvr_status host_finalize(pvr_encoder *e);
pvr_status host_forward(pvr_encoder *e, const uint8_t *frames, int n, int h, int w, float *out, int64_t out_stride);
void host_destroy(pvr_encoder *e);
// vit.hip
pvr_status vit_create(pvr_encoder *e);
pvr_status vit_finalize(pvr_encoder *e);
// vit.hip pieces shared with the CLIP RN50 plan: Resize(224, bicubic, antialias) + CenterCrop into a (res,res,3) uint8 image, attention core
pvr_status resizer_create(pvr_encoder *e);
pvr_status resizer_run(pvr_encoder *e, int lane, const uint8_t *frames, int nb, int h, int w, hipStream_t st, const uint8_t **u8, int *oh, int *ow);
void resizer_destroy(pvr_encoder *e);
pvr_status launch_attention(const void *qkv, void *out, int T, int W, int heads, int nb, int dtype, hipStream_t st);   // dtype PVR_F32: vit_f32.hip
// vit_f32.hip: the fp32 attention core (fp32 qkv rows [q | k | v] in, fp32 out, f32-input MFMA), head dim 64 / 80, 1..288 tokens
pvr_status launch_attention_f32(const float *qkv, float *out, int T, int W, int heads, int nb, hipStream_t st);
// vit.hip launch dispatchers the ViT forward and the pvr_op_* test entry points share (width 768 / 1024 / 1280, f16 / bf16 - and PVR_F32 with the fp32 output only; anything else is refused)
pvr_status launch_layernorm(const float *x, const float *patch_emb, const float *cls, const float *pos, const float *gamma, const float *beta,
                            float *out_f32, void *out_h, int rows, int T, int W, float eps, int normalize, int dtype, hipStream_t st);
pvr_status launch_cls_head(const float *x, const float *gamma, const float *beta, const float *proj, float *out, int64_t out_stride, int nb, int T, int W,
                           int out_dim, float eps, hipStream_t st);
// clip_rn50.hip
pvr_status launch_avgpool2(const void *in, void *out, int n, int h, int w, int c, int dtype, hipStream_t st);
pvr_status launch_attnpool_tokens(const float *x, const float *pos, void *tokens, int n, int hw, int c, int dtype, hipStream_t st);
pvr_status vit_forward(pvr_encoder *e, int lane, const uint8_t *frames, int n, int h, int w, float *out, int64_t out_stride, hipStream_t st);
void vit_destroy(pvr_encoder *e);
pvr_status vit_tap(pvr_encoder *e, const char *name, float *out, int64_t cap, int64_t *count, hipStream_t st);
}  // namespace pvr
