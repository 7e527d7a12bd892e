"""References for BatchNorm on its running statistics (frozen BatchNorm: pvr_op_bn_frozen_forward / _backward of include/pvr_train.h): float64
references, fp32 emulations with switches for the classic mistakes, and elementwise error bounds, in the manner of tests/train_refs.py (whose input
families, `ratio` and constants they share).  tests/test_frozen_bn_cpu.py shows that the fp32 emulation passes every bound and that every mutant
exceeds one; tests/test_gpu_frozen_bn_kernels.py holds the kernels to the same bounds.

Bounds, first order in u = 2^-24; m = running_mean, v = running_var, eps = 1e-5, all inputs exact fp32 values.

Forward.  rstd = 1 / sqrt(v + eps) is evaluated in fp32: the addition (u, halved by the square root), the square root (u), the division (u) and the
fp32 value of eps (below u / 2 relative to v + eps) - within 3 u, taken as 4 u:
    drstd = 4 u rstd                              (the slot the backward reads; the mean slot is a copy of m: exact)
y = relu(((z - m) * rstd) * gamma + beta + res): the subtraction, two products and the error of rstd put at most 7 u on |gamma xhat|, the addition of
beta at most u (|gamma xhat| + |beta|), the residual's at most u |pre| with pre the value before the ReLU, which is exact:
    dy <= 8 u |gamma xhat| + u |beta| + u |pre|,  taken as  8 u |gamma xhat| + 2 u (|beta| + |pre| + |res|)
The running buffers must come back bit-identical: their bound is 0.

Backward.  mean and rstd are INPUTS (the fp32 slots the forward wrote; the reference reads the same values), g = dy where (relu == 0 or y > 0) else 0.
The two column sums keep the discipline of bn_reduce_kernel - per-thread fp32 chains, a tree over the row lanes, the blocks' partials in float64 - with
a chain of at most 128 additions and a 4-step tree where that kernel has 256 and 3, so train_refs' A = 260 roundings bound them too:
    ddbeta  = (A + 2) u sum|g|,   ddgamma = (A + 5) u sum|g xhat|      (xhat = (z - mean) * rstd: 2 roundings, the product g * xhat: 1)
dz = (gamma * rstd) * g is two roundings (there are no mean terms: the statistics are constants), taken as 3; dres = g is exact, and one rounding of
the sum when it is added to what dres held:
    ddz = 3 u |gamma rstd g|,   ddres = 0  or  u (|prev| + |prev + g|)
"""
import torch

import train_refs as tr

U32, BN_A, BN_EPS = tr.U32, tr.BN_A, tr.BN_EPS

SHAPES = [(98, 64), (2049, 32), (6272, 256)]     # no multiple of any tile; one row past a 2048-row block; several blocks
FAMILIES = ('spread', 'large_mean')              # train_refs.bn_inputs: every family but 'large_mean' is the spread one
FORWARD_MUTANTS = ('batch_statistics', 'running_updated', 'no_eps')
BACKWARD_MUTANTS = ('mean_terms', 'mask_pre_residual')


def forward(z, res, gamma, beta, run_mean, run_var, relu, mutant=None):
    """-> dict(y, mean, rstd, run_mean, run_var) in the dtype of z (mean / rstd: the slots for the backward; run_*: the buffers after the call)"""
    eps = 0.0 if mutant == 'no_eps' else BN_EPS
    if mutant == 'batch_statistics':
        mean, var = z.mean(0), ((z - z.mean(0)) ** 2).mean(0)
    else:
        mean, var = run_mean, run_var
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (z - mean) * rstd * gamma + beta
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    out_mean, out_var = run_mean, run_var
    if mutant == 'running_updated':
        M = z.shape[0]
        bm = z.mean(0)
        out_mean = (1 - tr.MOMENTUM) * run_mean + tr.MOMENTUM * bm
        out_var = (1 - tr.MOMENTUM) * run_var + tr.MOMENTUM * ((z - bm) ** 2).sum(0) / max(M - 1, 1)
    return dict(y=y, mean=mean.clone(), rstd=rstd, run_mean=out_mean.clone(), run_var=out_var.clone())


def forward_ref(z, res, gamma, beta, run_mean, run_var, relu):
    """-> (ref, bound): dicts of float64 tensors with the keys of `forward`"""
    d = lambda t: None if t is None else t.double()
    z, res, gamma, beta, run_mean, run_var = d(z), d(res), d(gamma), d(beta), d(run_mean), d(run_var)
    ref = forward(z, res, gamma, beta, run_mean, run_var, relu)
    gx = ((z - run_mean) * ref['rstd'] * gamma).abs()
    r = res.abs() if res is not None else 0.0
    pre = (z - run_mean) * ref['rstd'] * gamma + beta + (res if res is not None else 0.0)
    zero = torch.zeros_like(run_mean)
    bound = dict(y=8 * U32 * gx + 2 * U32 * (beta.abs() + pre.abs() + r), mean=zero, rstd=4 * U32 * ref['rstd'], run_mean=zero, run_var=zero)
    return ref, bound


def backward(z, y, dy, gamma, mean, rstd, relu, prev=None, res=None, mutant=None):
    """-> dict(dz, dres, dgamma, dbeta).  y is the forward's output (post residual, post ReLU).  mutants: 'mean_terms' the batch-statistics dz,
    'mask_pre_residual' the ReLU mask from y - res"""
    M = z.shape[0]
    g = dy
    if relu:
        g = dy * (((y - res) if mutant == 'mask_pre_residual' else y) > 0).to(dy.dtype)
    xh = (z - mean) * rstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    dz = gamma * rstd * g
    if mutant == 'mean_terms':
        dz = gamma * rstd * (g - s0 / M - xh * (s1 / M))
    return dict(dz=dz, dres=g if prev is None else prev + g, dgamma=s1, dbeta=s0)


def backward_ref(z, y, dy, gamma, mean, rstd, relu, prev=None):
    d = lambda t: None if t is None else t.double()
    z, y, dy, gamma, mean, rstd, prev = d(z), d(y), d(dy), d(gamma), d(mean), d(rstd), d(prev)
    ref = backward(z, y, dy, gamma, mean, rstd, relu, prev)
    g = dy * (y > 0).double() if relu else dy
    xh = (z - mean) * rstd
    bound = dict(dz=3 * U32 * ref['dz'].abs(), dres=torch.zeros_like(g) if prev is None else U32 * (prev.abs() + ref['dres'].abs()),
                 dgamma=(BN_A + 5) * U32 * (g * xh).abs().sum(0), dbeta=(BN_A + 2) * U32 * g.abs().sum(0))
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------
# the network: torch's frozen-BatchNorm step (train mode, every BatchNorm in eval: train_refs.features(..., training=False) with autograd)
# ------------------------------------------------------------------------------------------------------------------
def frozen_step(state_dict, x, dout, variant, dtype):
    """one frozen-BatchNorm forward + backward of sum(out * dout) in `dtype` -> (out (N, C), {param: grad})"""
    sd = tr.to_tensors(state_dict, dtype, grad=True)
    out = tr.features(sd, x.to(dtype), variant, False).flatten(1)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), {k: v.grad.detach() for k, v in sd.items() if v.requires_grad}


def cat(d, keys):
    return torch.cat([d[k].double().flatten() for k in keys])
