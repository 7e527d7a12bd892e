"""References for the split-f16 weight gradients (csrc/wgrad_split16.hip; pvr_op_absmax_scale, pvr_op_conv_wgrad_split16, pvr_op_stem_wgrad_split16):
the scale rule, a CPU emulation of the kernels' arithmetic with both behaviours of f16 subnormal operands, the elementwise error bound, three input
families and the classic mistakes as mutants.  The float64 reference, the geometries and the helpers are those of tests/train_refs.py.
tests/test_wgrad_split16_cpu.py shows that the emulation passes the bound and every mutant exceeds it; tests/test_gpu_wgrad_split16_kernels.py holds
the kernels to the same bound.

The product.  dW = sum over L pixels of dz * x, per output element.  Both tensors are first multiplied by a power of two s = 2^(14 - floor(log2 max|t|))
(exact; the scaled maximum A' lies in [2^14, 2^15)), each scaled value a' is split into hi = f16(a') and lo = f16(2^11 (a' - hi)) (the difference is exact
in fp32), and the kernel accumulates hi*hi in one fp32 accumulator and lo*hi + hi*lo in a second one, adds the second times 2^-11 to the first, sums the
workgroups' partials in double and multiplies by 1 / (s_x s_dz) (exact).

The bound, first order in u = 2^-24, every term an absolute error of one output element, S = sum |dz| |x| over its L terms:
  * split.  |a' - hi| <= 2^-11 |a'| (f16 has 11 significant bits), so |lo| <= |a'| and rounding lo to f16 leaves a' = hi + 2^-11 lo + e with
    |e| <= 2^-11 2^-11 |lo| <= 2^-22 |a'|.  A product a' b' then differs from the three kept terms by e_a b' + a' e_b + 2^-22 lo_a lo_b: at most
    3 * 2^-22 |a' b'| = 12 u |a' b'|.  Summed: 12 u S.
  * accumulation.  hi and lo have 11-bit significands, so every product is exact in fp32; a sum of L such terms in ANY order is within L u of the sum of
    their magnitudes, which is <= S (1 + 2^-10) for the hi*hi terms; the cross accumulator carries the weight 2^-11 and its rounding is below u S.  The
    scaling of the cross sum, its addition, and the final rounding to fp32 are three more roundings.  (L + 4) u S.
  * f16's subnormal range.  A scaled value below 2^-14 has a subnormal hi (absolute rounding error 2^-25, which lo picks up) - or, if the matrix unit
    flushes subnormal operands, no hi at all: an absolute error below 2^-14 <= 2^-28 A' per element, and below 2^-25 for a flushed lo.  Per output element
    at most 2^-27 (A_x sum|dz| + A_dz sum|x|) over its L terms (zero-filled border terms contribute nothing: their x is an exact 0).  With subnormals kept
    the term is about 2^-50; which of the two the chip does is not assumed, so the bound takes the safe form.
  BOUND = (L + 20) u S + 2^-27 (A_x sum|dz| + A_dz sum|x|).

L grows the bound linearly while a dropped low part's error grows with sqrt(L): the mutants are shown at the geometries of CONV_GEOMETRIES (L <= 196),
and the kernel tests use those geometries."""
import numpy as np
import torch

import train_refs as tr

FAMILIES = ('unit', 'tiny', 'wide')
MUTANTS = ('lo_dropped', 'one_cross', 'cross_unscaled', 'no_prescale', 'scale_not_undone')
F16_MIN_NORMAL = 2.0 ** -14
# next to train_refs.CONV_GEOMETRIES: several tiles both ways at once, and a last cin tile that is half empty (160 = 64 + 64 + 32), at 36 pixels
EXTRA_GEOMETRIES = [(1, 6, 128, 128, 3, 1, 1), (1, 6, 160, 192, 1, 1, 0)]
GEOMETRIES = tr.CONV_GEOMETRIES + EXTRA_GEOMETRIES


def scale_rule(t):
    """the per-tensor scale of pvr_op_absmax_scale as a Python float: 2^(14 - floor(log2 max|t|)), read off the exponent field of the maximum's bit
    pattern; zero (or an empty tensor) and a non-finite maximum give 1; the exponent is clamped to [-126, 126] (a subnormal maximum takes 126)"""
    a = np.abs(np.asarray(t, dtype=np.float32)).ravel()
    if a.size == 0:
        return 1.0
    bits = int(a.view(np.uint32).max())               # (an integer max over the patterns: a NaN's pattern is above Inf's)
    E = bits >> 23
    if bits == 0 or E == 255:
        return 1.0
    return 2.0 ** int(np.clip(141 - E, -126, 126))


def inputs(family, geo):
    """x (n,h,h,ci), dz (n,ho,ho,co) fp32 tensors of a CONV_GEOMETRIES entry"""
    x, dz, _ = tr.conv_inputs(*geo)
    return _family(family, x, dz, 1000 + geo[1] + geo[2])


def stem_inputs(family, n, S):
    img, dz = tr.stem_inputs(n, S)
    return _family(family, img, dz, 2000 + S)


def _family(family, x, dz, seed):
    if family == 'unit':
        return x, dz
    if family == 'tiny':
        return x, (dz.double() * 1e-9).float()
    assert family == 'wide'
    r = np.random.default_rng(seed)
    fx = 2.0 ** r.integers(-20, 12, tuple(x.shape))    # 2^-20 .. 2^11
    fd = 2.0 ** r.integers(-40, 1, tuple(dz.shape))    # 2^-40 .. 1
    return (x.double() * torch.from_numpy(fx)).float(), (dz.double() * torch.from_numpy(fd)).float()


def _f16(a, flush):
    """fp32 -> the value the matrix unit reads: round to nearest even to f16; flush: subnormal operands read as zero"""
    h = a.numpy().astype(np.float16).astype(np.float32)
    if flush:
        h = np.where(np.abs(h) < F16_MIN_NORMAL, np.float32(0), h)
    return torch.from_numpy(h)


def split(a, scale, flush=False):
    """-> (hi, lo) fp32 tensors holding f16 values.  lo is computed from the UNflushed hi, as the staging pass does (a flush happens at the operand read)"""
    s = (a * np.float32(scale)).float()
    hi = torch.from_numpy(s.numpy().astype(np.float16).astype(np.float32))
    lo = (s - hi) * 2048.0
    return (_f16(hi, flush), _f16(lo, flush))


def emulate(x, dz, k, s, p, flush=False, mutant=None):
    """the kernels' arithmetic on the CPU: fp32 accumulation (torch's order; the bound holds for any), then the double reduction's scale"""
    sx, sdz = (1.0, 1.0) if mutant == 'no_prescale' else (scale_rule(x), scale_rule(dz))
    xh, xl = split(x, sx, flush)
    dh, dl = split(dz, sdz, flush)
    hh = tr.wgrad(xh, dh, k, s, p)
    if mutant == 'lo_dropped':
        acc = hh
    else:
        cross = tr.wgrad(xl, dh, k, s, p)
        if mutant != 'one_cross':
            cross = cross + tr.wgrad(xh, dl, k, s, p)
        acc = hh + cross * (1.0 if mutant == 'cross_unscaled' else 2.0 ** -11)
    out = acc.double()
    if mutant != 'scale_not_undone':
        out = out * (1.0 / sx) * (1.0 / sdz)
    return out.float()


def reference(x, dz, k, s, p):
    """-> (float64 reference, elementwise bound)"""
    xd, dd = x.double(), dz.double()
    ref = tr.wgrad(xd, dd, k, s, p)
    L = dz.shape[0] * dz.shape[1] * dz.shape[2]
    S = tr.wgrad(xd.abs(), dd.abs(), k, s, p)
    sum_dz = tr.wgrad(torch.ones_like(xd), dd.abs(), k, s, p)     # over the terms whose x exists (border terms are exact zeros)
    sum_x = tr.wgrad(xd.abs(), torch.ones_like(dd), k, s, p)
    bound = (L + 20) * tr.U32 * S + 2.0 ** -27 * (float(xd.abs().max()) * sum_dz + float(dd.abs().max()) * sum_x)
    return ref, bound


def stem_reference(img, dz):
    return reference(img[..., :3].contiguous(), dz, 7, 2, 3)


def stem_emulate(img, dz, flush=False, mutant=None):
    return emulate(img[..., :3].contiguous(), dz, 7, 2, 3, flush, mutant)
