"""References for the trainable encoder (include/pvr_train.h): a train-mode torch restatement of the ResNet trunks, and for every kernel of
csrc/train_kernels.hip a float64 reference, an elementwise error bound derived from the float64 magnitudes (in the manner of
oracle/vit_kernel_refs.py), input families, and a CPU emulation with switches for the classic mistakes.  tests/test_train_refs_cpu.py shows
that the fp32 emulation passes every bound and every mutant exceeds its bound; tests/test_gpu_train_kernels.py holds the kernels to the same
bounds.

Bounds are first order in u = 2^-24.  A sum of L fp32 products in ANY order is within L u sum|a_i b_i| of the exact sum; the convolution-type
kernels (weight gradient, data gradient, conv1's weight gradient) take that with L + 2 (the final rounding, the sum of the accumulator sets).
BatchNorm: the kernel's statistics are chains of at most 256 additions per thread, 3 tree steps over the row lanes and a float64 sum of the
partials, A = 260 roundings in all:
    dmean  = (A + 1) u mean|z|
    dvar   = (A + 4) u var + dmean^2            (sum (z - m')^2 / M = var + (m - m')^2 exactly)
    drstd  = rstd (dvar / (2 (var + eps)) + 2 u)
    dy     = |gamma| rstd dmean + |gamma xhat| (drstd / rstd + 6 u) + 2 u (|beta| + |y| + |res|)
and for the backward, whose mean / rstd are INPUTS (the reference reads the same fp32 values), with g the masked dy:
    ddbeta = (A + 2) u sum|g|,  ddgamma = (A + 5) u sum|g xhat|
    ddz    = |gamma| rstd ((A + 4) u (sum|g| + |xhat| sum|g xhat|) / M + 8 u (|g| + |sum g| / M + |xhat sum g xhat| / M)) + 3 u |dz|
"""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
BN_A = 260
BN_EPS = 1e-5
MOMENTUM = 0.1


def ratio(got, ref, bound):
    """largest |got - ref| / bound (inf when anything is not finite; an element whose bound is 0 must be exact)"""
    got, ref, bound = (torch.as_tensor(t).double() for t in (got, ref, bound))
    if not torch.isfinite(got).all():
        return float('inf')
    err = (got - ref).abs()
    return float((err / bound.clamp_min(1e-300)).max())


def _rng(seed):
    return np.random.default_rng(seed)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ------------------------------------------------------------------------------------------------------------------
# convolution gradients.  x (n,h,w,ci) NHWC, dz (n,ho,wo,co), weights torch's (co,ci,k,k).  The same function is the float64 reference
# (dtype of its inputs), the fp32 emulation and - on |x|, |dz| - the magnitude sum of the bound.
# ------------------------------------------------------------------------------------------------------------------
CONV_GEOMETRIES = [  # (n, h, cin, cout, k, stride, pad)
    (2, 8, 32, 64, 3, 1, 1), (2, 8, 64, 64, 3, 2, 1), (2, 8, 64, 128, 1, 2, 0),
    (3, 7, 256, 64, 1, 1, 0),        # 147 pixels: no multiple of a tile
    (1, 14, 64, 64, 3, 1, 1),        # 196 pixels: split over more than one workgroup's pixel range
]
# the data gradient (and the forward convolutions) run one fma chain over K = k * k * cout products: layer4's 3x3 has K = 4608, the longest of these trunks
DGRAD_LONG_K = (1, 4, 64, 512, 3, 1, 1)
WGRAD_MUTANTS = ('tap_shifted', 'stride_dropped', 'last_row_dropped')


def out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def conv_inputs(n, h, ci, co, k, s, p, seed=3):
    r = _rng(seed + 131 * h + ci + 7 * co + k + s)
    ho = out_size(h, k, s, p)
    x = r.standard_normal((n, h, h, ci)).astype(np.float32)
    dz = (r.standard_normal((n, ho, ho, co)) * 0.1).astype(np.float32)
    wt = (r.standard_normal((co, ci, k, k)) / np.sqrt(ci * k * k)).astype(np.float32)
    return _t(x), _t(dz), _t(wt)


def wgrad(x, dz, k, s, p, mutant=None):
    n, h, w, ci = x.shape
    _, ho, wo, co = dz.shape
    st = 1 if mutant == 'stride_dropped' else s
    xp = F.pad(x.permute(0, 3, 1, 2), (p + 1, p + 1, p + 1, p + 1))
    rows = ho - 1 if mutant == 'last_row_dropped' else ho
    dw = torch.zeros((co, ci, k, k), dtype=x.dtype)
    for kh in range(k):
        for kw in range(k):
            ys, xs = 1 + kh + (1 if mutant == 'tap_shifted' else 0), 1 + kw
            patch = xp[:, :, ys:ys + st * (ho - 1) + 1:st, xs:xs + st * (wo - 1) + 1:st]
            dw[:, :, kh, kw] = torch.einsum('nyxo,ncyx->oc', dz[:, :rows], patch[:, :, :rows])
    return dw


def wgrad_ref(x, dz, k, s, p):
    ref = wgrad(x.double(), dz.double(), k, s, p)
    L = dz.shape[0] * dz.shape[1] * dz.shape[2]
    return ref, (L + 2) * U32 * wgrad(x.double().abs(), dz.double().abs(), k, s, p)


def dgrad(dz, wt, h, k, s, p, mutant=None):
    n, ho, wo, co = dz.shape
    ci = wt.shape[1]
    dxp = torch.zeros((n, h + 2 * p, h + 2 * p, ci), dtype=dz.dtype)
    for kh in range(k):
        for kw in range(k):
            wk = wt[:, :, k - 1 - kh, k - 1 - kw] if mutant == 'not_rotated' else wt[:, :, kh, kw]
            dxp[:, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s] += dz @ wk
    return dxp[:, p:p + h, p:p + h].contiguous()


def dgrad_ref(dz, wt, h, k, s, p, prev=None):
    ref = dgrad(dz.double(), wt.double(), h, k, s, p)
    bound = (k * k * dz.shape[3] + 2) * U32 * dgrad(dz.double().abs(), wt.double().abs(), h, k, s, p)
    if prev is not None:
        ref = ref + prev.double()
        bound = bound + U32 * (prev.double().abs() + ref.abs())
    return ref, bound


def stem_inputs(n, S, seed=5):
    r = _rng(seed)
    img = np.zeros((n, S, S, 4), np.float32)
    img[..., :3] = r.standard_normal((n, S, S, 3))
    dz = (r.standard_normal((n, S // 2, S // 2, 64)) * 0.1).astype(np.float32)
    return _t(img), _t(dz)


def stem_wgrad_ref(img, dz):
    return wgrad_ref(img[..., :3], dz, 7, 2, 3)


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm2d, training mode, over (rows, C)
# ------------------------------------------------------------------------------------------------------------------
BN_SHAPES = [(98, 64), (6272, 64), (50, 2048)]
BN_FAMILIES = ('unit', 'large_mean')


def bn_inputs(family, rows, C, seed=9):
    r = _rng(seed + rows + C)
    z = r.standard_normal((rows, C))
    if family == 'large_mean':
        z = 100.0 + 0.1 * z
    else:
        z = z * r.uniform(0.2, 3.0, (1, C)) + r.uniform(-2.0, 2.0, (1, C))
    d = dict(z=z, res=r.standard_normal((rows, C)), gamma=r.uniform(0.5, 1.5, C) * r.choice([-1.0, 1.0], C), beta=r.uniform(-0.5, 0.5, C),
             run_mean=r.uniform(-0.3, 0.3, C), run_var=r.uniform(0.5, 1.5, C), dy=r.standard_normal((rows, C)), prev=r.standard_normal((rows, C)))
    return {k: _t(v.astype(np.float32)) for k, v in d.items()}


def bn_forward(z, res, gamma, beta, run_mean, run_var, relu, mutant=None):
    """-> dict(y, mean, rstd, run_mean, run_var) in the dtype of z.  mutants: 'naive_variance' E[x^2] - E[x]^2, 'biased_running_var'"""
    M = z.shape[0]
    mean = z.mean(0)
    var = (z * z).mean(0) - mean * mean if mutant == 'naive_variance' else ((z - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    y = (z - mean) * rstd * gamma + beta
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    unb = var if mutant == 'biased_running_var' else var * (M / (M - 1.0))
    return dict(y=y, mean=mean, rstd=rstd, run_mean=(1 - MOMENTUM) * run_mean + MOMENTUM * mean, run_var=(1 - MOMENTUM) * run_var + MOMENTUM * unb)


def bn_forward_ref(z, res, gamma, beta, run_mean, run_var, relu):
    """-> (ref, bound): dicts of float64 tensors with the keys of bn_forward"""
    d = lambda t: None if t is None else t.double()
    z, res, gamma, beta, run_mean, run_var = d(z), d(res), d(gamma), d(beta), d(run_mean), d(run_var)
    M = z.shape[0]
    ref = bn_forward(z, res, gamma, beta, run_mean, run_var, relu)
    mean, rstd = ref['mean'], ref['rstd']
    var = ((z - mean) ** 2).mean(0)
    dmean = (BN_A + 1) * U32 * z.abs().mean(0)
    dvar = (BN_A + 4) * U32 * var + dmean ** 2
    drel = dvar / (2 * (var + BN_EPS)) + 2 * U32
    xh = (z - mean) * rstd
    pre = xh * gamma + beta + (res if res is not None else 0.0)
    dy = gamma.abs() * rstd * dmean + (gamma * xh).abs() * (drel + 6 * U32) + 2 * U32 * (beta.abs() + pre.abs() + (res.abs() if res is not None else 0.0))
    unb = var * (M / (M - 1.0))
    bound = dict(y=dy, mean=dmean + U32 * mean.abs(), rstd=rstd * drel + U32 * rstd,
                 run_mean=MOMENTUM * dmean + 4 * U32 * (run_mean.abs() + mean.abs()),
                 run_var=MOMENTUM * dvar * (M / (M - 1.0)) + 4 * U32 * (run_var.abs() + unb))
    return ref, bound


def bn_backward(z, y, dy, gamma, mean, rstd, relu, prev=None, res=None, mutant=None):
    """-> dict(dz, dres, dgamma, dbeta).  y is the forward's output (post residual, post ReLU); mutant 'mask_pre_residual' takes the ReLU mask
    from y - res instead"""
    M = z.shape[0]
    g = dy
    if relu:
        g = dy * (((y - res) if mutant == 'mask_pre_residual' else y) > 0).to(dy.dtype)
    xh = (z - mean) * rstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    dz = gamma * rstd * (g - s0 / M - xh * (s1 / M))
    return dict(dz=dz, dres=g if prev is None else prev + g, dgamma=s1, dbeta=s0)


def bn_backward_ref(z, y, dy, gamma, mean, rstd, relu, prev=None):
    d = lambda t: None if t is None else t.double()
    z, y, dy, gamma, mean, rstd, prev = d(z), d(y), d(dy), d(gamma), d(mean), d(rstd), d(prev)
    M = z.shape[0]
    ref = bn_backward(z, y, dy, gamma, mean, rstd, relu, prev)
    g = dy * (y > 0).double() if relu else dy
    xh = (z - mean) * rstd
    sg, sgx = g.abs().sum(0), (g * xh).abs().sum(0)
    s0, s1 = ref['dbeta'], ref['dgamma']
    ddz = gamma.abs() * rstd * ((BN_A + 4) * U32 * (sg + xh.abs() * sgx) / M + 8 * U32 * (g.abs() + s0.abs() / M + (xh * s1).abs() / M)) + 3 * U32 * ref['dz'].abs()
    bound = dict(dz=ddz, dres=torch.zeros_like(g) if prev is None else U32 * (prev.abs() + ref['dres'].abs()), dgamma=(BN_A + 5) * U32 * sgx,
                 dbeta=(BN_A + 2) * U32 * sg)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------
# pools
# ------------------------------------------------------------------------------------------------------------------
def maxpool_inputs(n=2, h=8, c=64, seed=21):
    """post-ReLU-like input with planted ties (a window whose maximum appears twice, at its first and at a later position) and all-zero windows"""
    r = _rng(seed)
    x = np.maximum(r.standard_normal((n, h, h, c)), 0.0).astype(np.float32)
    x[0, 0:3, 0:3, :] = 0.0                      # all-zero windows (also the padded corner window)
    x[1, 4:8, 4:8, ::2] = 0.0
    x[0, 3, 5, :] = 7.0; x[0, 4, 6, :] = 7.0      # the same maximum twice inside windows (oy 2, ox 3): first in scan order wins
    x[1, 1, 1, :] = 5.0; x[1, 1, 2, :] = 5.0; x[1, 2, 1, :] = 5.0
    dy = r.standard_normal((n, h // 2, h // 2, c)).astype(np.float32)
    return _t(x), _t(dy)


def maxpool_backward_ref(x, dy):
    """torch's own float64 MaxPool2d(3, 2, 1) backward (its tie rule is the specification); bound: <= 4 contributions summed in fp32"""
    xx = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xx, 3, 2, 1).backward(dy.double().permute(0, 3, 1, 2).contiguous())
    xa = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(xa, 3, 2, 1).backward(dy.double().abs().permute(0, 3, 1, 2).contiguous())
    return xx.grad.permute(0, 2, 3, 1).contiguous(), 3 * U32 * xa.grad.permute(0, 2, 3, 1).contiguous()


def maxpool_backward_emulate(x, dy, mutant=None):
    """the kernel's gather in fp32: per input pixel, the windows that cover it and whose first maximum it is.  mutant 'last_max': ties to the last"""
    n, h, w, c = x.shape
    ho, wo = dy.shape[1:3]
    dx = torch.zeros_like(x)
    for oy in range(ho):
        for ox in range(wo):
            best = torch.full((n, c), -float('inf'))
            by = torch.zeros((n, c), dtype=torch.long); bx = torch.zeros((n, c), dtype=torch.long)
            for yy in range(max(2 * oy - 1, 0), min(2 * oy + 2, h)):
                for xx in range(max(2 * ox - 1, 0), min(2 * ox + 2, w)):
                    v = x[:, yy, xx, :]
                    take = (v >= best) if mutant == 'last_max' else (v > best)
                    best = torch.where(take, v, best); by = torch.where(take, torch.tensor(yy), by); bx = torch.where(take, torch.tensor(xx), bx)
            ni, ci = torch.meshgrid(torch.arange(n), torch.arange(c), indexing='ij')
            dx.index_put_((ni, by, bx, ci), dy[:, oy, ox, :], accumulate=True)
    return dx


def avgpool_backward_ref(dout, hw):
    ref = (dout.double() / hw)[:, None, :].expand(-1, hw, -1).contiguous()
    return ref, 2 * U32 * ref.abs()


# ------------------------------------------------------------------------------------------------------------------
# the network: torchvision resnet18 / 34 / 50 trunks as a function of a {name: tensor} dict, train or eval mode (any float dtype).
# With training=False it is oracle.encoder_oracle.resnet50_features operation for operation.
# ------------------------------------------------------------------------------------------------------------------
LAYERS = {'r18': (2, 2, 2, 2), 'r34': (3, 4, 6, 3), 'conv5': (3, 4, 6, 3)}


def _cbn(sd, conv, bn, x, stride, pad, training):
    x = F.conv2d(x, sd[conv + '.weight'], None, stride, pad)
    return F.batch_norm(x, sd[bn + '.running_mean'], sd[bn + '.running_var'], sd[bn + '.weight'], sd[bn + '.bias'], training, MOMENTUM if training else 0.0, BN_EPS)


def features(sd, x, variant, training):
    """sd: tensors under torchvision names (running statistics are updated in place when training); x (N,3,224,224) normalised.  -> (N, C, 1, 1)"""
    x = F.max_pool2d(F.relu(_cbn(sd, 'conv1', 'bn1', x, 2, 3, training)), 3, 2, 1)
    for li in range(4):
        for bi in range(LAYERS[variant][li]):
            p, stride = 'layer%d.%d' % (li + 1, bi), 2 if (bi == 0 and li > 0) else 1
            if variant == 'conv5':
                out = F.relu(_cbn(sd, p + '.conv1', p + '.bn1', x, 1, 0, training))
                out = F.relu(_cbn(sd, p + '.conv2', p + '.bn2', out, stride, 1, training))
                out = _cbn(sd, p + '.conv3', p + '.bn3', out, 1, 0, training)
            else:
                out = F.relu(_cbn(sd, p + '.conv1', p + '.bn1', x, stride, 1, training))
                out = _cbn(sd, p + '.conv2', p + '.bn2', out, 1, 1, training)
            idn = x
            if (p + '.downsample.0.weight') in sd:
                idn = _cbn(sd, p + '.downsample.0', p + '.downsample.1', x, stride, 0, training)
            x = F.relu(out + idn)
    return F.adaptive_avg_pool2d(x, 1)


def to_tensors(state_dict, dtype=torch.float32, grad=False):
    """a numpy / tensor state_dict -> {name: tensor}: floating tensors in `dtype` (parameters with requires_grad when asked), counters as they are"""
    out = {}
    for k, v in state_dict.items():
        t = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))).detach().clone()
        if k.endswith('num_batches_tracked'):
            out[k] = t
            continue
        t = t.to(dtype)
        if grad and not k.endswith(('running_mean', 'running_var')):
            t.requires_grad_(True)
        out[k] = t
    return out


def train_step(state_dict, x, dout, variant, dtype):
    """one training forward + backward of sum(out * dout) in `dtype` -> (out (N, C), {param: grad}, {buffer: updated running statistic})"""
    sd = to_tensors(state_dict, dtype, grad=True)
    out = features(sd, x.to(dtype), variant, True).flatten(1)
    (out * dout.to(dtype)).sum().backward()
    grads = {k: v.grad.detach() for k, v in sd.items() if v.requires_grad}
    bufs = {k: v.detach() for k, v in sd.items() if k.endswith(('running_mean', 'running_var'))}
    return out.detach(), grads, bufs


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def max_rel(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
