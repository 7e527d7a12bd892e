// Launchers of train_kernels.hip that the trainable encoder (encoder_train.hip) calls next to the pvr_op_* entry points of include/pvr_train.h.
#pragma once
#include "common.h"

namespace pvr {
// torch's (cout, cin, k, k) weights -> launch_conv_f32's K-major (cout_pad, k*k*cin) matrix (K index (kh*k + kw)*cin + c; rows past cout zero).
// flip: the data gradient's operand instead, (cin_pad, k*k*cout) with out[ci][(kh*k + kw)*cout + co] = w[co][ci][k-1-kh][k-1-kw]
pvr_status launch_pack_conv_weights(const float *w, float *out, int cout, int cin, int k, bool flip, hipStream_t st);
// torch's (64, 3, 7, 7) conv1 weights -> stem_f32_kernel's [64][49][4] (slot 3 zero)
pvr_status launch_pack_stem_weights(const float *w, float *out, hipStream_t st);
// pvr_op_conv_dgrad with its scratch as separate pieces: wflip (cin_pad * k*k * cout floats), dil (n*h*w*cout floats, stride 2 only), zero_bias (>= cin zeros)
pvr_status launch_conv_dgrad(const float *dz, const float *w, float *dx, int accumulate, int n, int h, int wd, int cin, int cout, int k, int stride, int pad,
                             float *wflip, float *dil, const float *zero_bias, hipStream_t st);
// grads[i] += pass[i] over n floats: one fp32 addition per element (gradient accumulation over the passes of a chunked step)
pvr_status launch_grad_add(float *grads, const float *pass, int64_t n, hipStream_t st);
// pvr_op_bn_frozen_forward's launch (same refusals); mean_out / rstd_out may both be null: nothing is kept for a backward
pvr_status launch_bn_frozen_apply(const float *z, const float *res, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                  float *y, float *mean_out, float *rstd_out, int64_t rows, int c, int relu, hipStream_t st);
// conv_f32.hip: convolution (wpack: launch_pack_conv_weights' plain matrix) + frozen BatchNorm [+ residual] [ReLU] -> y in one launch; no z is written
pvr_status launch_conv_bn_frozen_f32(const float *in, const float *wpack, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                     const float *res, float *out, int n, int h, int w, int cin, int cout, int k, int stride, int pad, int relu, hipStream_t st);
// dz (n, h/2, w/2, c) -> the even pixels of a zeroed (n, h, w, c) grid: the stride-2 data gradients' input
pvr_status launch_dilate2(const float *dz, float *out, int n, int h, int w, int c, hipStream_t st);
// conv_split16_scaled.hip: the forward and the data gradient of a convolution as exact-split f16 products with per-tensor scales read from the device
// (sx / sdz / sw: one float each, pvr_op_absmax_scale's rule).  w: torch's (cout, cin, k, k).  wpack / wflip: the split weights, rows_pad * k*k * cols floats
// as launch_pack_conv_weights; dil: n*h*w*cout floats (stride 2 only).  Refusals as pvr_op_conv_fwd_split16 / pvr_op_conv_dgrad_split16.
pvr_status launch_conv_fwd_split16(const float *x, const float *w, float *z, int n, int h, int wd, int cin, int cout, int k, int stride, int pad, const float *sx,
                                   const float *sw, float *wpack, hipStream_t st);
// launch_conv_fwd_split16 with the frozen BatchNorm [+ residual] [ReLU] in the convolution's epilogue (the BNF instance): pack + ONE launch -> y, the bits of
// launch_conv_fwd_split16 followed by launch_bn_frozen_apply; no z is written
pvr_status launch_conv_bn_frozen_split16(const float *x, const float *w, const float *gamma, const float *beta, const float *run_mean, const float *run_var,
                                         const float *res, float *y, int n, int h, int wd, int cin, int cout, int k, int stride, int pad, int relu, const float *sx,
                                         const float *sw, float *wpack, hipStream_t st);
pvr_status launch_conv_dgrad_split16(const float *dz, const float *w, float *dx, int accumulate, int n, int h, int wd, int cin, int cout, int k, int stride, int pad,
                                     const float *sdz, const float *sw, float *wflip, float *dil, hipStream_t st);
}  // namespace pvr
