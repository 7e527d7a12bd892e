"""References for the prefix_once mode (pvr_trainer_forward_boundary, pvr_trainer_set_prefix_fused; HipTrainableResNet(..., train_from=...,
prefix_once=True)): the boundary tensor's size per trunk and stage, and - for the split prefix op as one launch
(pvr_op_conv_bn_frozen_forward_split16) - a float64 reference, the elementwise bound and an fp32 emulation with the classic mistakes as mutants, built
from tests/conv_split16_refs.py (the split product) and tests/train_from_refs.py (the frozen BatchNorm epilogue, families and geometries).
tests/test_prefix_once_cpu.py shows that the emulation passes the bound and every mutant exceeds it; tests/test_gpu_prefix_once_kernels.py holds the
kernel to the same bound and to the bits of the two-launch form.

The op.  y = relu(((z - m) * rstd) * gamma + beta + res) with z = conv(x, w) as conv_split16_refs' exact-split product (both operands scaled by a power
of two, hi * hi in one fp32 accumulator, the two cross terms in a second one that is scaled by 2^-11 once, the scales undone exactly) and the epilogue of
train_from_refs: m = running_mean, rstd = 1 / sqrt(running_var + 1e-5) in fp32 per channel.  First order in u = 2^-24:
  * the convolution: |dz| <= B_z = (K + 20) u S + 2^-27 (A_x sum|w| + A_w sum|x|), conv_split16_refs' bound of pvr_op_conv_fwd_split16.  The epilogue
    multiplies z by gamma * rstd, so it reaches y as |gamma rstd| B_z.
  * the epilogue is train_from_refs', rounding for rounding: 8 u |gamma rstd (z - m)| + 2 u (|beta| + |pre| + |res|).
  BOUND = |gamma rstd| B_z + 8 u |gamma rstd (z - m)| + 2 u (|beta| + |pre| + |res|).

Mutants, each with a residual and the ReLU on, and the family each is shown in.  'no_eps' and 'batch_statistics' and 'relu_before_residual' are
train_from_refs' ('no_eps' in 'large_mean', where its 1e-4 relative error of rstd acts on |z - m| = 100).  'scale_not_undone' leaves the product
multiplied by s_x s_w, and 'cross_dropped' keeps hi * hi alone (a relative error near 2^-12 per product that grows with sqrt(K), against a bound
that grows with K): both are mistakes of the convolution, shown in 'spread', where |z - m| is of order 1 and the convolution's term carries the
bound - in 'large_mean' the epilogue's 8 u |gamma rstd 100| would hide a dropped cross term."""
import unittest.mock as mock

import torch

import conv_split16_refs as cs
import train_from_refs as tf
import train_refs as tr

U32 = tr.U32
FAMILIES = tf.FAMILIES
GEOMETRIES = tf.GEOMETRIES
# mutant -> (train_from_refs' epilogue mutant, conv_split16_refs' product mutant, the families it is shown in)
MUTANTS = {'no_eps': ('no_eps', None, ('large_mean',)),
           'batch_statistics': ('batch_statistics', None, FAMILIES),
           'relu_before_residual': ('relu_before_residual', None, FAMILIES),
           'scale_not_undone': (None, 'scale_not_undone', FAMILIES),
           'cross_dropped': (None, 'lo_dropped', ('spread',))}

# floats per frame of the boundary tensor at stages 1 .. 4: the max pool's output or the last prefix op's y
BOUNDARY_FLOATS = {'resnet50': (56 * 56 * 64, 56 * 56 * 256, 28 * 28 * 512, 14 * 14 * 1024),
                   'resnet18': (56 * 56 * 64, 56 * 56 * 64, 28 * 28 * 128, 14 * 14 * 256)}


def fused_split_reference(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p):
    """-> (float64 reference y, elementwise bound); res may be None"""
    k = wt.shape[2]
    y, _ = tf.fused_reference(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p)
    z, bz = cs.fwd_reference(x, wt, k, s, p)
    g, b, m, v = gamma.double(), beta.double(), run_mean.double(), run_var.double()
    rstd = 1.0 / torch.sqrt(v + tr.BN_EPS)
    gx = (z - m) * rstd * g
    r = res.double() if res is not None else None
    pre = gx + b + (r if r is not None else 0.0)
    bound = (g * rstd).abs() * bz + 8 * U32 * gx.abs() + 2 * U32 * (b.abs() + pre.abs() + (r.abs() if r is not None else 0.0))
    return y, bound


def fused_split_emulate(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p, mutant=None):
    """the kernel's arithmetic in fp32: conv_split16_refs' emulation of the split product, then train_from_refs' emulation of the epilogue (which
    takes its z from train_from_refs.conv: handed the split product's z here) -> y as a float32 tensor"""
    bn_mutant, conv_mutant, _ = MUTANTS[mutant] if mutant else (None, None, None)
    z = cs.fwd_emulate(x, wt, wt.shape[2], s, p, mutant=conv_mutant).float().contiguous()
    with mock.patch.object(tf, 'conv', lambda *a: z):
        return tf.fused_emulate(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p, mutant=bn_mutant)


def scales(x, wt):
    """(s_x, s_w): pvr_op_absmax_scale's rule on the host"""
    return cs.ws.scale_rule(x), cs.ws.scale_rule(wt)
