"""References for the split-f16 forward convolutions and data gradients (csrc/conv_split16_scaled.hip; pvr_op_conv_fwd_split16,
pvr_op_conv_dgrad_split16): float64 references, the elementwise error bound, a CPU emulation of the kernel's arithmetic with both behaviours of f16
subnormal operands, five input families and the classic mistakes as mutants.  The scale rule, the split and the geometries are those of
tests/wgrad_split16_refs.py and tests/train_refs.py.  tests/test_conv_split16_cpu.py shows that the emulation passes the bound and every mutant exceeds
it; tests/test_gpu_conv_split16_kernels.py holds the kernel to the same bound.

The product.  z = sum over K = k*k*cin products of x * w per output element (the data gradient: K = k*k*cout products of dz * w; a stride-2 data
gradient reads a zero-filled grid whose zeros are exact and contribute nothing).  Both tensors are first multiplied by a power of two
s = 2^(14 - floor(log2 max|t|)) (exact; the scaled maximum A' lies in [2^14, 2^15)), each scaled value a' is split into hi = f16(a') and
lo = f16(2^11 (a' - hi)) (the difference is exact in fp32), and the kernel accumulates hi*hi in one fp32 accumulator and lo*hi + hi*lo in a second one,
adds the second times 2^-11 to the first and multiplies by 1 / s_x and by 1 / s_w (exact).  The accumulate form of the data gradient then adds what dx
held, one fp32 addition.

The bound is wgrad_split16_refs' with the K products in the place of the L pixels; first order in u = 2^-24, every term an absolute error of one output
element, S = sum |x| |w| over its K terms:
  * split.  |a' - hi| <= 2^-11 |a'|, so |lo| <= |a'| and rounding lo to f16 leaves a' = hi + 2^-11 lo + e with |e| <= 2^-22 |a'|.  A product a' b'
    differs from the three kept terms by e_a b' + a' e_b + 2^-22 lo_a lo_b: at most 3 * 2^-22 |a' b'| = 12 u |a' b'|.  Summed: 12 u S.
  * accumulation.  hi and lo have 11-bit significands, so every product is exact in fp32; a sum of K such terms in ANY order is within K u of the sum
    of their magnitudes, which is <= S (1 + 2^-10); the cross accumulator carries the weight 2^-11 and its rounding is below u S.  The scaling of the
    cross sum and its addition are two more roundings; undoing the scales is exact.  (K + 3) u S.
  * f16's subnormal range.  A scaled value below 2^-14 has a subnormal hi - or, if the matrix unit flushes subnormal operands, none: an absolute error
    below 2^-14 <= 2^-28 A' per element, and below 2^-25 for a flushed lo.  Per output element at most 2^-27 (A_x sum|w| + A_w sum|x|) over its terms
    (border terms and the grid's zeros contribute nothing: their x is an exact 0).  Which of the two the chip does is not assumed.
  * the accumulate form: one more rounding, u (|previous| + |result|) as train_refs.dgrad_ref.
  BOUND = (K + 20) u S + 2^-27 (A_x sum|w| + A_w sum|x|) [+ u (|previous| + |result|)].

K grows the bound linearly while a dropped low part's error grows with sqrt(K): the mutants are shown at the geometries of CONV_GEOMETRIES."""
import numpy as np
import torch
import torch.nn.functional as F

import train_refs as tr
import wgrad_split16_refs as ws

FAMILIES = ws.FAMILIES + ('large', 'small_w')
MUTANTS = ws.MUTANTS
GEOMETRIES = tr.CONV_GEOMETRIES + [tr.DGRAD_LONG_K] + ws.EXTRA_GEOMETRIES


def inputs(family, geo):
    """x (n,h,h,ci), dz (n,ho,ho,co), wt (co,ci,k,k) fp32 tensors of a geometry.  'unit' / 'tiny' / 'wide' are wgrad_split16_refs' families with the
    weights in the place of its first operand for the data gradient (dz is the tiny / wide gradient) and in the place of its second for the forward;
    'large': activations and gradients near 1e6, past f16's 65504; 'small_w': weights near 1e-6, inside f16's subnormal range"""
    x, dz, wt = tr.conv_inputs(*geo)
    seed = 3000 + geo[1] + geo[2]
    if family in ws.FAMILIES:
        _, dz = ws._family(family, wt, dz, seed)
        x, wt = ws._family(family, x, wt, seed + 1)
    elif family == 'large':
        x, dz = (x.double() * 1e6).float(), (dz.double() * 1e7).float()
    else:
        assert family == 'small_w'
        wt = (wt.double() * 1e-5).float()
    return x, dz, wt


def fwd(x, wt, k, s, p):
    """z (n,ho,wo,co) = conv(x (n,h,w,ci), wt (co,ci,k,k)) in the dtype of its inputs"""
    return F.conv2d(x.permute(0, 3, 1, 2), wt, None, s, p).permute(0, 2, 3, 1).contiguous()


def _bound(K, S, sum_w, sum_a, a_max, w_max):
    return (K + 20) * tr.U32 * S + 2.0 ** -27 * (a_max * sum_w + w_max * sum_a)


def fwd_reference(x, wt, k, s, p):
    """-> (float64 reference, elementwise bound)"""
    xd, wd = x.double(), wt.double()
    ref = fwd(xd, wd, k, s, p)
    S = fwd(xd.abs(), wd.abs(), k, s, p)
    sum_w = fwd(torch.ones_like(xd), wd.abs(), k, s, p)        # over the terms whose x exists (border terms are exact zeros)
    sum_x = fwd(xd.abs(), torch.ones_like(wd), k, s, p)
    return ref, _bound(k * k * x.shape[3], S, sum_w, sum_x, float(xd.abs().max()), float(wd.abs().max()))


def dgrad_reference(dz, wt, h, k, s, p, prev=None):
    dd, wd = dz.double(), wt.double()
    ref = tr.dgrad(dd, wd, h, k, s, p)
    S = tr.dgrad(dd.abs(), wd.abs(), h, k, s, p)
    sum_w = tr.dgrad(torch.ones_like(dd), wd.abs(), h, k, s, p)
    sum_d = tr.dgrad(dd.abs(), torch.ones_like(wd), h, k, s, p)
    bound = _bound(k * k * dz.shape[3], S, sum_w, sum_d, float(dd.abs().max()), float(wd.abs().max()))
    if prev is not None:
        ref = ref + prev.double()
        bound = bound + tr.U32 * (prev.double().abs() + ref.abs())
    return ref, bound


def _emulate(a, wt, product, flush, mutant, prev):
    """the kernel's arithmetic on the CPU: `product(a, w)` in fp32 (torch's order; the bound holds for any), the cross accumulator scaled once, the scales
    undone in fp32, then the optional fp32 addition"""
    sa, sw = (1.0, 1.0) if mutant == 'no_prescale' else (ws.scale_rule(a), ws.scale_rule(wt))
    with np.errstate(over='ignore'):                  # (the 'no_prescale' mutant overflows f16 on the 'large' family: that is what it is shown on)
        ah, al = ws.split(a, sa, flush)
        wh, wl = ws.split(wt, sw, flush)
    hh = product(ah, wh)
    if mutant == 'lo_dropped':
        acc = hh
    else:
        cross = product(al, wh)
        if mutant != 'one_cross':
            cross = cross + product(ah, wl)
        acc = hh + cross * np.float32(1.0 if mutant == 'cross_unscaled' else 2.0 ** -11)
    out = acc.float()
    if mutant != 'scale_not_undone':
        out = (out * np.float32(1.0 / sa)) * np.float32(1.0 / sw)
    return out if prev is None else out + prev


def fwd_emulate(x, wt, k, s, p, flush=False, mutant=None):
    return _emulate(x, wt, lambda a, w: fwd(a, w, k, s, p), flush, mutant, None)


def dgrad_emulate(dz, wt, h, k, s, p, flush=False, mutant=None, prev=None):
    return _emulate(dz, wt, lambda a, w: tr.dgrad(a, w, h, k, s, p), flush, mutant, prev)


def prev_of(geo, seed=77):
    """what dx holds before an accumulating data gradient: of the size of the result of the 'unit' family"""
    n, h, ci = geo[0], geo[1], geo[2]
    return torch.from_numpy((np.random.default_rng(seed + h + ci).standard_normal((n, h, h, ci)) * 0.1).astype(np.float32))
