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
}  // namespace pvr
