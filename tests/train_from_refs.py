"""References for partial fine-tuning (pvr_trainer_set_train_from of include/pvr_train.h; EmbeddingNet(..., train=True, train_from='layer3')): torch's
recipe restated on tests/train_refs.py - the frozen prefix's modules in eval with requires_grad False, the trained stages on batch or running
statistics - and, for the fused prefix op (pvr_op_conv_bn_frozen_forward), a float64 reference, an fp32 emulation with switches for the classic
mistakes and the elementwise error bound.  tests/test_train_from_cpu.py shows that the emulation passes the bound and every mutant exceeds it;
tests/test_gpu_train_from_kernels.py holds the kernel to the same bound.

The fused op.  y = relu(((z - m) * rstd) * gamma + beta + res), z = conv(x, w) one chain of K = k*k*cin fp32 fmas, m = running_mean,
rstd = 1 / sqrt(running_var + 1e-5) evaluated in fp32 per channel; all inputs are exact fp32 values.  First order in u = 2^-24:
  * the convolution.  A sum of K fp32 products in ANY order is within K u S of the exact sum, S = sum |x| |w| over the K terms of the element
    (train_refs' rule, with its + 2 for the final roundings): dz <= (K + 2) u S.  The epilogue multiplies z by gamma * rstd, so this part of the
    error reaches y as |gamma rstd| (K + 2) u S.
  * the epilogue is frozen_bn_refs' forward, rounding for rounding: rstd is within 4 u of its value; the subtraction, the two products and the error
    of rstd put at most 8 u on |gamma rstd (z - m)|; adding beta and the residual costs at most u (|gamma xhat| + |beta|) and u |pre|, pre the
    value in front of the ReLU (which is exact) - taken, as there, as 2 u (|beta| + |pre| + |res|).
  BOUND = |gamma rstd| (K + 2) u S + 8 u |gamma rstd (z - m)| + 2 u (|beta| + |pre| + |res|).
An fma contraction of the last product and the addition of beta removes a rounding and stays inside.

Families.  'spread': running_mean within +-0.3 of z's level, so |z - m| is of order 1 and the convolution's term carries the bound.  'large_mean':
running_mean +-100 away (random sign per channel), so |z - m| is about 100, the epilogue's term carries the bound, and half of the channels sit far
below zero in front of the ReLU.  running_var is drawn from [0.01, 0.05] in both - a trained trunk's small variances, where eps matters most:
leaving eps out moves rstd by eps / (2 v) = 1e-4 .. 5e-4 relative.

Mutants (each exceeds the bound, with a residual and the ReLU on): 'batch_statistics' normalises with z's own mean and variance; 'no_eps' (shown in
'large_mean', where its 1e-4 relative error acts on |z - m| = 100; in 'spread' it is of the size of the convolution's own bound and proves
nothing); 'relu_before_residual' adds the residual behind the ReLU; 'gamma_on_residual' scales the residual as well."""
import numpy as np
import torch
import torch.nn.functional as F

import frozen_bn_refs as fr
import train_refs as tr

U32, BN_EPS = tr.U32, tr.BN_EPS
FAMILIES = ('spread', 'large_mean')
MUTANTS = ('batch_statistics', 'no_eps', 'relu_before_residual', 'gamma_on_residual')
# (n, h, cin, cout, k, stride, pad) next to train_refs.CONV_GEOMETRIES: fewer pixels than one 64-pixel tile; cout past one 64-wide tile and no multiple
# of 64; a stride-2 1 x 1 on an odd size
EXTRA_GEOMETRIES = [(1, 7, 32, 64, 3, 1, 1), (2, 8, 32, 132, 1, 1, 0), (2, 9, 32, 64, 1, 2, 0)]
GEOMETRIES = tr.CONV_GEOMETRIES + EXTRA_GEOMETRIES
STAGES = {'layer1': 1, 'layer2': 2, 'layer3': 3, 'layer4': 4}


# ------------------------------------------------------------------------------------------------------------------
# the fused prefix op
# ------------------------------------------------------------------------------------------------------------------
def fused_inputs(family, geo, seed=41):
    """fp32 tensors of a geometry: x (n,h,h,ci), wt (co,ci,k,k), gamma, beta, run_mean, run_var (co), res (n,ho,ho,co)"""
    n, h, ci, co, k, s, p = geo
    x, _, wt = tr.conv_inputs(*geo)
    r = np.random.default_rng(seed + 17 * h + ci + 3 * co + k + s + (1000 if family == 'large_mean' else 0))
    ho = tr.out_size(h, k, s, p)
    mean = r.uniform(-0.3, 0.3, co)
    if family == 'large_mean':
        mean = mean + 100.0 * r.choice([-1.0, 1.0], co)
    d = dict(gamma=r.uniform(0.5, 1.5, co) * r.choice([-1.0, 1.0], co), beta=r.uniform(-0.5, 0.5, co), run_mean=mean, run_var=r.uniform(0.01, 0.05, co),
             res=r.standard_normal((n, ho, ho, co)))
    out = {kk: torch.from_numpy(np.ascontiguousarray(v.astype(np.float32))) for kk, v in d.items()}
    out.update(x=x, wt=wt)
    return out


def conv(x, wt, s, p):
    """z (n,ho,wo,co) = conv(x (n,h,w,ci), wt (co,ci,k,k)) in the dtype of its inputs"""
    return F.conv2d(x.permute(0, 3, 1, 2), wt, None, s, p).permute(0, 2, 3, 1).contiguous()


def fused_reference(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p):
    """-> (float64 reference y, elementwise bound); res may be None"""
    d = lambda t: None if t is None else t.double()
    x, wt, gamma, beta, run_mean, run_var, res = d(x), d(wt), d(gamma), d(beta), d(run_mean), d(run_var), d(res)
    K = wt.shape[1] * wt.shape[2] * wt.shape[3]
    z, S = conv(x, wt, s, p), conv(x.abs(), wt.abs(), s, p)
    rstd = 1.0 / torch.sqrt(run_var + BN_EPS)
    gx = (z - run_mean) * rstd * gamma
    pre = gx + beta + (res if res is not None else 0.0)
    y = torch.relu(pre) if relu else pre
    bound = (gamma * rstd).abs() * (K + 2) * U32 * S + 8 * U32 * gx.abs() + 2 * U32 * (beta.abs() + pre.abs() + (res.abs() if res is not None else 0.0))
    return y, bound


def fused_emulate(x, wt, gamma, beta, run_mean, run_var, res, relu, s, p, mutant=None):
    """the kernel's arithmetic in fp32 (numpy float32 for the epilogue; the convolution is torch's fp32 one - another order of the same K products,
    which the bound allows) -> y as a float32 tensor"""
    f = np.float32
    z = conv(x.float(), wt.float(), s, p).numpy()
    g, b, m, v = (t.float().numpy() for t in (gamma, beta, run_mean, run_var))
    if mutant == 'batch_statistics':
        zz = z.reshape(-1, z.shape[-1])
        m = zz.mean(0, dtype=f)
        v = ((zz - m) ** 2).mean(0, dtype=f)
    eps = f(0.0) if mutant == 'no_eps' else f(BN_EPS)
    rstd = (f(1.0) / np.sqrt(v + eps)).astype(f)
    r = None if res is None else res.float().numpy()
    if mutant == 'gamma_on_residual' and r is not None:
        t = (((z - m) * rstd + r) * g + b).astype(f)
        r = None
    else:
        t = ((z - m) * rstd * g + b).astype(f)
    if mutant == 'relu_before_residual' and relu:
        t = np.maximum(t, f(0.0))
        relu = 0
    if r is not None:
        t = (t + r).astype(f)
    if relu:
        t = np.maximum(t, f(0.0))
    return torch.from_numpy(np.ascontiguousarray(t))


# ------------------------------------------------------------------------------------------------------------------
# the network: torch's partial fine-tuning step.  The frozen prefix (conv1 / bn1 and the layers below `stage`) runs in eval with requires_grad
# False; the trained stages run on batch statistics (bn_frozen False) or on their running statistics (bn_frozen True).
# ------------------------------------------------------------------------------------------------------------------
def is_trained(name, stage):
    """does the parameter / buffer `name` belong to layer{stage} .. layer4 ? (stage 0: everything)"""
    return stage == 0 or any(name.startswith('layer%d.' % s) for s in range(stage, 5))


def features(sd, x, variant, stage, bn_frozen):
    """train_refs.features with the training flag per module: False in the prefix, `not bn_frozen` in the trained stages"""
    mode = lambda name: (not bn_frozen) and is_trained(name + '.', stage)
    x = F.max_pool2d(F.relu(tr._cbn(sd, 'conv1', 'bn1', x, 2, 3, mode('conv1'))), 3, 2, 1)
    for li in range(4):
        for bi in range(tr.LAYERS[variant][li]):
            p, stride = 'layer%d.%d' % (li + 1, bi), 2 if (bi == 0 and li > 0) else 1
            t = mode(p)
            if variant == 'conv5':
                out = F.relu(tr._cbn(sd, p + '.conv1', p + '.bn1', x, 1, 0, t))
                out = F.relu(tr._cbn(sd, p + '.conv2', p + '.bn2', out, stride, 1, t))
                out = tr._cbn(sd, p + '.conv3', p + '.bn3', out, 1, 0, t)
            else:
                out = F.relu(tr._cbn(sd, p + '.conv1', p + '.bn1', x, stride, 1, t))
                out = tr._cbn(sd, p + '.conv2', p + '.bn2', out, 1, 1, t)
            idn = x
            if (p + '.downsample.0.weight') in sd:
                idn = tr._cbn(sd, p + '.downsample.0', p + '.downsample.1', x, stride, 0, t)
            x = F.relu(out + idn)
    return F.adaptive_avg_pool2d(x, 1)


def partial_step(state_dict, x, dout, variant, stage, dtype, bn_frozen):
    """one forward + backward of sum(out * dout) in `dtype` -> (out (N, C), {trained param: grad}, {buffer: running statistic after the step})"""
    sd = tr.to_tensors(state_dict, dtype, grad=False)
    for k, v in sd.items():
        if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked')) and is_trained(k, stage):
            v.requires_grad_(True)
    out = features(sd, x.to(dtype), variant, stage, bn_frozen).flatten(1)
    (out * dout.to(dtype)).sum().backward()
    grads = {k: v.grad.detach() for k, v in sd.items() if v.requires_grad}
    bufs = {k: v.detach() for k, v in sd.items() if k.endswith(('running_mean', 'running_var'))}
    return out.detach(), grads, bufs


def cat(d, keys):
    return fr.cat(d, keys)
