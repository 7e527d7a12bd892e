"""float64 references, derived error bounds, input families and CPU emulations for the ResNet-side kernels: the implicit-GEMM convolution
(csrc/conv_igemm.hip, and through it every kernel that is pinned to it bit for bit), its split-K form, the stem and its fused pooled forms
(csrc/stem.hip), the max / average pools and the layout and format kernels - test infrastructure, CPU only.

Same rules as oracle/vit_kernel_refs.py, whose helpers this module reuses: a reference takes the inputs the kernel takes (already rounded to the
16-bit storage type, or fp32) and evaluates the operation in float64; every bound is elementwise and derived from the kernel's arithmetic, never
measured; the emulations restate that arithmetic in fp32 / 16-bit torch with switches for the classic mistakes, and
tests/test_resnet_kernel_refs_cpu.py shows that every emulation passes its bound on every family and that every mutant fails on a named one.

Notation: u32 = 2^-24, u = unit roundoff of the storage type (f16 2^-11, bf16 2^-8), SUB16 = half its smallest subnormal.

Instruction accuracies.  The kernel guides of this project give rates, not accuracies, for the transcendental instructions; the figures used here are
the ones AMD's CDNA instruction set reference states - V_RCP_F32 and V_EXP_F32: 1 ulp, i.e. a relative error of at most 2^-23 = 2 u32 - and the
ones the code itself documents: `v_rcp_f32 (1 ulp)` in the QuickGELU epilogue of conv_igemm.hip / conv_pp256.hip, and Abramowitz & Stegun 7.1.26
(|error| <= 1.5e-7 in erf) for gelu_erf in common.h.  __expf(x) is v_exp_f32(x * log2(e)).  Neither instruction returns subnormals; an absolute
term F32_TINY covers results that small.
"""
import numpy as np
import torch
import torch.nn.functional as F

from pvr_habitat_amd import synth
from .vit_kernel_refs import U32, U16, SUB16, TORCH_DT, round_to, ratio   # noqa: F401  (re-exported: the tests take them from here)

F32_TINY = 2.0 ** -119                 # 128 * the smallest normal fp32: |x| * (a flushed factor) for every |x| <= 128
QGELU_LIP = 1.1                        # sup |d/dv v sigmoid(1.702 v)| = 1.0998 (test_activation_lipschitz_constants checks both on a grid)
GELU_LIP = 1.13                        # sup |d/dv gelu(v)| = 1.1290
AS_ERF = 1.5e-7                        # Abramowitz & Stegun 7.1.26
_AS_P = 0.3275911
_AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def dt_of(t):
    return 'f16' if t.dtype == torch.float16 else 'bf16'


# ------------------------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------------------------
def out_hw(h, w, kh, kw, stride, pad):
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


def pack_weights(wt):
    """(cout, kh, kw, cin) -> the kernels' (cout_pad, kh*kw*cin) matrix, K index (kh*KW + kw)*cin + c, cout_pad = cout rounded up to 64 (zero rows)"""
    cout = wt.shape[0]
    wk = torch.zeros(((cout + 63) // 64 * 64, wt[0].numel()), dtype=wt.dtype)
    wk[:cout] = wt.reshape(cout, -1)
    return wk


def pad_bias(b):
    bp = torch.zeros((b.numel() + 63) // 64 * 64, dtype=torch.float32)
    bp[:b.numel()] = b
    return bp


def _conv64(x, wt, stride, pad):
    """x (n,h,w,cin), wt (cout,kh,kw,cin), float64 -> (n,ho,wo,cout)"""
    if wt.shape[1] == 1 and wt.shape[2] == 1 and pad == 0:
        return x[:, ::stride, ::stride, :] @ wt[:, 0, 0, :].t()
    return F.conv2d(x.permute(0, 3, 1, 2), wt.permute(0, 3, 1, 2), stride=stride, padding=pad).permute(0, 2, 3, 1)


def quickgelu64(v):
    return v * torch.sigmoid(1.702 * v)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.special.erf(v * 0.7071067811865476))


def _act_bound(pre, E, act):
    """reference and error bound behind the activation, given the pre-activation value and its bound E (float64 tensors).

    act 0 / 1: the identity and ReLU are 1-Lipschitz and exact in fp32: E.

    act 2, QuickGELU as coded, v * rcp(1 + __expf(-1.702f * v)).  With z = -1.702 v, e = exp(z): the argument of v_exp_f32 carries four roundings
    relative to z (the constants 1.702f and log2(e), two products): the relative error of e is 4 |z| u32 plus the instruction's 2 u32.  It enters
    1 + e damped by e / (1 + e) = sigmoid(z); the addition, v_rcp_f32 (2 u32) and the final product add 1 + 2 + 1.  The input error E passes through
    the function's Lipschitz constant:  QGELU_LIP E + |f| u32 ((4 |z| + 2) sigmoid(z) + 4) + F32_TINY.  No cancellation: the form never subtracts.

    act 3, gelu_erf (common.h): x = |v| / sqrt2 (2 roundings), t = rcp(1 + p x) (relative error <= 4 px / (1 + px) + 1 + 2 <= 7 u32),
    poly(t) by Horner (nine operations and five rounded coefficients: 10 u32 sum_i |a_i| t^i, plus |poly'(t)| times t's error), e2 = __expf(-x x)
    (argument: 2 * 2 + 1 roundings, then constant and product: relative error (7 x^2 + 2) u32), erfc = poly e2 (1), the approximation itself
    (AS_ERF, absolute), erf = 1 - erfc (1), s = 1 +- erf (1), f = (0.5 v) s (1):
        ds = e2 dpoly + erfc (7 x^2 + 3) u32 + AS_ERF + u32 erf + u32 |s|,      df = 0.5 |v| ds + u32 |f| + GELU_LIP E + F32_TINY.
    For v < 0, s = 1 - erf cancels: ds stays of the order of AS_ERF while s itself goes to zero, so the error is ABSOLUTE, 0.5 |v| ds, not
    relative to the (tiny) result - which is why the term is kept apart from u32 |f|.
    """
    if act == 0:
        return pre, E
    if act == 1:
        return pre.clamp_min(0.0), E
    if act == 2:
        z = -1.702 * pre
        f = quickgelu64(pre)
        return f, QGELU_LIP * E + f.abs() * U32 * ((4.0 * z.abs() + 2.0) * torch.sigmoid(z) + 4.0) + F32_TINY
    assert act == 3
    av = pre.abs()
    x = av * 0.7071067811865476
    t = 1.0 / (1.0 + _AS_P * x)
    a = _AS_A
    ptil = t * (abs(a[0]) + t * (abs(a[1]) + t * (abs(a[2]) + t * (abs(a[3]) + t * abs(a[4])))))
    dpoly_dt = a[0] + t * (2 * a[1] + t * (3 * a[2] + t * (4 * a[3] + t * 5 * a[4])))
    dpoly = 10.0 * U32 * ptil + dpoly_dt.abs() * 7.0 * U32 * t
    e2 = torch.exp(-x * x)
    erfc = torch.special.erfc(x)
    erf = 1.0 - erfc
    s = torch.where(pre < 0, erfc, 1.0 + erf)
    ds = e2 * dpoly + erfc * (7.0 * x * x + 3.0) * U32 + AS_ERF + U32 * erf + U32 * s
    f = gelu64(pre)
    return f, GELU_LIP * E + 0.5 * av * ds + U32 * f.abs() + F32_TINY


def _store_bound(ref, E, out_dt):
    """the final rounding: to the 16-bit storage type u (|ref| + E) + SUB16 (below the normal range the rounding error is absolute: a kernel that
    flushes subnormal outputs is off by more), u32 (|ref| + E) for an fp32 output"""
    if out_dt:
        return E + U16[out_dt] * (ref.abs() + E) + SUB16[out_dt]
    return E + U32 * (ref.abs() + E)


def conv_ref(x, wt, b, res=None, act=0, stride=1, pad=0, out_dt=None, extra=None):
    """x: (n,h,w,cin) 16-bit, wt: (cout,kh,kw,cin) 16-bit, b: (cout) fp32, res: (n,ho,wo,cout) 16-bit or fp32 or None, act 0 none / 1 ReLU / 2 QuickGELU /
    3 erf-GELU, out_dt: 'f16' / 'bf16' for a 16-bit output, None for fp32.  extra = (x2, w2, stride2): a second pixel operand appended along K
    (the two-operand form: + w2 (cout, cin2) . x2[:, ::stride2, ::stride2]).  Returns (ref, bound), float64 (n,ho,wo,cout).

    Bound, with s = sum x w, S = sum |x w| over the K = kh kw cin (+ cin2) products of one output:
      * products of two f16 or two bf16 values are exact in fp32 (11 + 11 and 8 + 8 significand bits; the exponent range of fp32 holds them);
      * fp32 accumulation of K terms in an unknown order - the MFMA's own sum over its k-block, the K-slice loop, split-K planes added afterwards:
        every term passes through at most K - 1 additions, gamma_{K-1} S <= K u32 S (K^2 u32 <= 1: K <= 4096);
      * epilogue: one fp32 rounding for + bias, one for + residual (u32 times the magnitude of each rounded sum), then the activation (_act_bound);
      * the final rounding (_store_bound).
    Nothing in between is rounded to 16 bits, so the bound has no u term except the last."""
    xd, wd = x.double(), wt.double()
    s = _conv64(xd, wd, stride, pad)
    S = _conv64(xd.abs(), wd.abs(), stride, pad)
    K = wt[0].numel()
    if extra is not None:
        x2, w2, s2 = extra
        x2d, w2d = x2.double()[:, ::s2, ::s2, :], w2.double()
        s = s + x2d @ w2d.t()
        S = S + x2d.abs() @ w2d.abs().t()
        K += w2.shape[1]
    assert K * K * U32 <= 1.0
    E = K * U32 * S
    pre = s + b.double()
    E = E + U32 * (pre.abs() + E)
    if res is not None:
        pre = pre + res.double()
        E = E + U32 * (pre.abs() + E)
    ref, E = _act_bound(pre, E, act)
    return ref, _store_bound(ref, E, out_dt)


CONV_MUTANTS = ('round_per_tap', 'bias_16bit', 'relu_before_residual', 'bias_by_tile', 'pad_wraps_row', 'origin_without_pad', 'drop_last_k_slice',
                'residual_16bit', 'quickgelu_1p7', 'gelu_tanh')


def _quickgelu32(v, c=1.702):
    return v * (1.0 / (1.0 + torch.exp(-np.float32(c) * v)))


def _gelu_erf32(v):
    """gelu_erf of common.h in fp32 torch"""
    f = np.float32
    x = v.abs() * f(0.70710678118654752)
    t = 1.0 / (1.0 + f(_AS_P) * x)
    a = [f(c) for c in _AS_A]
    poly = t * (a[0] + t * (a[1] + t * (a[2] + t * (a[3] + t * a[4]))))
    erf_abs = 1.0 - poly * torch.exp(-x * x)
    return f(0.5) * v * (1.0 + torch.where(v < 0, -erf_abs, erf_abs))


def _gelu_tanh32(v):
    return np.float32(0.5) * v * (1.0 + torch.tanh(np.float32(0.7978845608028654) * (v + np.float32(0.044715) * v * v * v)))


def conv_emulate(x, wt, b, res=None, act=0, stride=1, pad=0, out_dt=None, mutant=None, extra=None, ksplit=0, tile=64):
    """The kernels' arithmetic on the CPU: exact products, fp32 accumulation tap by tap and K slice by K slice (ksplit > 1: into that many fp32 planes
    of ceil(slices / ksplit) consecutive 64-wide K slices, added in plane order), fp32 bias, fp32 residual, activation, one rounding to the output type.
    mutant: one of CONV_MUTANTS or None.  tile: the cout tile of bias_by_tile."""
    assert mutant is None or mutant in CONV_MUTANTS
    sdt = x.dtype
    n, h, w, cin = x.shape
    cout, kh, kw, _ = wt.shape
    ho, wo = out_hw(h, w, kh, kw, stride, pad)
    xz = torch.cat([x.float().reshape(n, h * w, cin), torch.zeros(n, 1, cin)], dim=1)          # row h*w: the zero every padded tap reads
    wf = wt.float()
    origin = 0 if mutant == 'origin_without_pad' else pad
    nslice = kh * kw * (cin // 64) + (extra[1].shape[1] // 64 if extra is not None else 0)
    per_plane = (nslice + ksplit - 1) // ksplit if ksplit > 1 else nslice
    planes = [torch.zeros(n, ho * wo, cout) for _ in range((nslice + per_plane - 1) // per_plane)]
    q = 0
    for a in range(kh):
        for bb in range(kw):
            hi = torch.arange(ho) * stride + a - origin
            wi = torch.arange(wo) * stride + bb - origin
            flat = hi[:, None] * w + wi[None, :]
            ok_h = ((hi >= 0) & (hi < h))[:, None]
            if mutant == 'pad_wraps_row':                                                     # the column is not checked: the flat index lands in a neighbouring row
                ok = ok_h & (flat >= 0) & (flat < h * w)
            else:
                ok = ok_h & ((wi >= 0) & (wi < w))[None, :]
            patch = xz[:, torch.where(ok, flat, torch.full_like(flat, h * w)).reshape(-1), :]  # (n, ho*wo, cin)
            for cs in range(cin // 64):
                if mutant == 'drop_last_k_slice' and extra is None and q == nslice - 1:
                    break
                p = planes[q // per_plane]
                p += patch[:, :, cs * 64:cs * 64 + 64] @ wf[:, a, bb, cs * 64:cs * 64 + 64].t()
                q += 1
            if mutant == 'round_per_tap':
                planes[0] = planes[0].to(sdt).float()
    if extra is not None:
        x2, w2, s2 = extra
        x2f, w2f = x2.float()[:, ::s2, ::s2, :].reshape(n, ho * wo, -1), w2.float()
        for cs in range(w2.shape[1] // 64):
            p = planes[q // per_plane]
            p += x2f[:, :, cs * 64:cs * 64 + 64] @ w2f[:, cs * 64:cs * 64 + 64].t()
            q += 1
    acc = planes[0]
    for p in planes[1:]:
        acc = acc + p
    acc = acc.reshape(n, ho, wo, cout)
    bias = b.float()
    if mutant == 'bias_16bit':
        bias = bias.to(sdt).float()
    if mutant == 'bias_by_tile':
        bias = bias[torch.arange(cout) % tile]
    v = acc + bias
    relu_done = False
    if res is not None:
        r = res.to(sdt).float() if mutant == 'residual_16bit' else res.float()
        if mutant == 'relu_before_residual':
            v, relu_done = v.clamp_min(0.0) + r, True
        else:
            v = v + r
    if act == 1 and not relu_done:
        v = v.clamp_min(0.0)
    elif act == 2:
        v = _quickgelu32(v, 1.7 if mutant == 'quickgelu_1p7' else 1.702)
    elif act == 3:
        v = _gelu_tanh32(v) if mutant == 'gelu_tanh' else _gelu_erf32(v)
    return v.to(TORCH_DT[out_dt]) if out_dt else v


CONV_FAMILIES = ('unit', 'exact', 'cancel', 'bias_dominant', 'relu_edge', 'tiny', 'large')
EXACT_LIMIT = {'f16': 2048.0, 'bf16': 256.0}          # integers up to here are representable: 11 / 8 significand bits


def _signed(seed, name, shape):
    """values of magnitude in [0.5, 1.5) with a random sign: never near zero, so that a scaled copy has no subnormal element"""
    u = synth.uniform(seed, name, shape, -1.0, 1.0)
    return torch.from_numpy(np.where(u < 0, u - 0.5, u + 0.5).astype(np.float32))


def conv_inputs(family, shape, dt, res=None, seed=23):
    """shape = (n, h, w, cin, cout, kh, kw, stride, pad); res: None, 'h' (16-bit residual) or 'f32'.  Returns (x, wt, b, r): x (n,h,w,cin) and wt
    (cout,kh,kw,cin) in the storage type, b fp32 (cout), r (n,ho,wo,cout) in the storage type or fp32, or None.  Families:
    unit           x ~ N(0,1), w ~ N(0, 2/K), b ~ U(-0.5, 0.5), r ~ N(0,1)
    exact          x[n,y,x,c] = (3y + 5x + n + c) mod 7 - 3: an integer that differs between horizontal and vertical neighbours (a wrong tap or padding
                   decision changes a value); six non-zero weights of +-1 / +-2 per output channel at scattered (tap, channel) places, integer bias in
                   [-4, 4] and residual in [-8, 8]: sum |x w| + |b| + |r| <= 48, every partial sum in any order is a small integer, exact in fp32 and in
                   both storage types - the kernel must return the float64 result bit for bit (test_exact_family_precondition asserts the limit)
    cancel         x = 8 + N(0,1)/4, weights antisymmetric tap against the centre-mirrored tap, and K half against K half in the centre tap (the only
                   tap of a 1x1), up to a small random part: the partial sums are far above the result, which leaves the accumulation term of the
                   bound on its own
    bias_dominant  products scaled to 2^-10, bias U(0.5, 1.5) with a full fp32 significand: not representable in 16 bits
    relu_edge      the residual is -(conv + bias) rounded to storage, moved by -2 .. 2 ulp: the pre-activation sits within a few ulp of zero, on both sides
    tiny           |x| in [0.5, 1.5) 2^-9, |w| in [0.5, 1.5) 2^-6 / sqrt(K), b ~ 2^-18 N(0,1): no operand is subnormal, the f16 outputs are (|out| ~ 1e-5
                   against the smallest normal 6.1e-5); a kernel that flushes them is wrong by more than SUB16
    large          x, w > 0 with conv ~ 3e4; with a residual b ~ +5e4 and r ~ -5e4, so that conv + bias is above the f16 range while the result is inside
    """
    n, h, w, cin, cout, kh, kw, stride, pad = shape
    ho, wo = out_hw(h, w, kh, kw, stride, pad)
    K = kh * kw * cin
    tag = 'conv_%s_%s' % (family, '_'.join(str(v) for v in shape))
    nrm = lambda nm, shp: torch.from_numpy(synth.normal(seed, tag + nm, shp))
    r = None
    if family == 'exact':
        yy, xx, nn, cc = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(n), torch.arange(cin), indexing='ij')
        x = (((3 * yy + 5 * xx + nn + cc) % 7) - 3).permute(2, 0, 1, 3).float()
        bits = synth.bits(seed, tag + 'w', cout * 6).astype(np.int64).reshape(cout, 6)
        wt = torch.zeros(cout, K)
        pos = torch.from_numpy((bits >> 8) % K)
        val = torch.from_numpy(np.array([1.0, -1.0, 2.0, -2.0], np.float32)[(bits >> 3) % 4])
        wt.scatter_(1, pos, val)                                            # (a place drawn twice keeps one value: at most six non-zeros)
        wt = wt.reshape(cout, kh, kw, cin)
        b = torch.from_numpy((synth.bits(seed, tag + 'b', cout) % np.uint64(9)).astype(np.float32) - 4.0)
        if res:
            r = torch.from_numpy((synth.bits(seed, tag + 'r', n * ho * wo * cout) % np.uint64(17)).astype(np.float32) - 8.0).reshape(n, ho, wo, cout)
    elif family == 'cancel':
        x = 8.0 + 0.25 * nrm('x', (n, h, w, cin))
        w0 = nrm('w', (cout, kh, kw, cin)) * K ** -0.5
        wa = (w0 - w0.flip(1, 2)) * 0.5                                     # tap against the centre-mirrored tap: a tap's own sum is large
        if kh % 2 == 1 and kw % 2 == 1:                                     # the centre tap is its own mirror: K half against K half there
            wa[:, kh // 2, kw // 2, :cin // 2] = w0[:, kh // 2, kw // 2, :cin // 2]
            wa[:, kh // 2, kw // 2, cin // 2:] = -w0[:, kh // 2, kw // 2, :cin // 2]
        wt = wa + 2.0 ** -6 * nrm('d', (cout, kh, kw, cin)) * K ** -0.5
        b = torch.from_numpy(synth.uniform(seed, tag + 'b', (cout,), -0.5, 0.5))
        if res:
            r = nrm('r', (n, ho, wo, cout))
    elif family == 'bias_dominant':
        x = nrm('x', (n, h, w, cin))
        wt = 2.0 ** -10 * nrm('w', (cout, kh, kw, cin)) * K ** -0.5
        b = torch.from_numpy(synth.uniform(seed, tag + 'b', (cout,), 0.5, 1.5))
        if res:
            r = 2.0 ** -10 * nrm('r', (n, ho, wo, cout))
    elif family == 'tiny':
        x = 2.0 ** -9 * _signed(seed, tag + 'x', (n, h, w, cin))
        wt = 2.0 ** -6 * K ** -0.5 * _signed(seed, tag + 'w', (cout, kh, kw, cin))
        b = 2.0 ** -18 * torch.from_numpy(synth.normal(seed, tag + 'b', (cout,)))
        if res:
            r = 2.0 ** -13 * _signed(seed, tag + 'r', (n, ho, wo, cout))         # the smallest normal f16 magnitudes: the sums straddle the subnormal range
    elif family == 'large':
        x = _signed(seed, tag + 'x', (n, h, w, cin)).abs()
        wt = _signed(seed, tag + 'w', (cout, kh, kw, cin)).abs() * (3.0e4 / K)
        b = torch.from_numpy(synth.uniform(seed, tag + 'b', (cout,), -100.0, 100.0))
        if res:
            b = b + 5.0e4
            r = -5.0e4 + 1.0e3 * nrm('r', (n, ho, wo, cout))
    else:
        assert family in ('unit', 'relu_edge')
        x = nrm('x', (n, h, w, cin))
        wt = nrm('w', (cout, kh, kw, cin)) * (2.0 / K) ** 0.5
        b = torch.from_numpy(synth.uniform(seed, tag + 'b', (cout,), -0.5, 0.5))
        if res:
            r = nrm('r', (n, ho, wo, cout))
    x, wt = round_to(x, dt), round_to(wt, dt)
    if family == 'relu_edge':
        assert res, 'relu_edge needs a residual'
        pre = _conv64(x.double(), wt.double(), stride, pad) + b.double()
        k = torch.from_numpy((synth.bits(seed, tag + 'k', pre.numel()) % np.uint64(5)).astype(np.float64) - 2.0).reshape(pre.shape)
        r = (-pre * (1.0 + 2.0 * U16[dt] * k)).float()                      # (2 u |v| is one ulp at the top of a binade, two at the bottom)
    if r is not None and res == 'h':
        r = round_to(r, dt)
    return x, wt, b.float().contiguous(), r


# mutant -> (family, shape, res, act, 16-bit output?) of the configuration that must catch it in both storage types.  fp32 output for the four mutants whose
# error is a fraction of one 16-bit rounding (of the bias, of the residual, ~3e-4 of the result, <= 5e-4 absolute): the rounding of a 16-bit output
# covers most of that and they leave the bound by a factor of 1.5 .. 7 only, where the fp32 output shows them at 5 .. 10^4 times the bound.
S_SMALL = (1, 5, 7, 64, 64, 3, 3, 1, 1)
S_NK4 = (2, 9, 8, 256, 128, 1, 1, 1, 0)
S_ACT = (1, 150, 1, 128, 256, 1, 1, 1, 0)
CONV_CAUGHT_BY = {
    'round_per_tap': ('cancel', S_SMALL, None, 0, True),
    'bias_16bit': ('bias_dominant', S_SMALL, None, 0, False),
    'relu_before_residual': ('relu_edge', S_NK4, 'h', 1, True),
    'bias_by_tile': ('unit', (3, 7, 7, 64, 128, 1, 1, 1, 0), None, 1, True),
    'pad_wraps_row': ('exact', S_SMALL, None, 0, True),
    'origin_without_pad': ('exact', S_SMALL, None, 0, True),
    'drop_last_k_slice': ('unit', S_NK4, 'h', 1, True),
    'residual_16bit': ('unit', S_ACT, 'f32', 0, False),
    'quickgelu_1p7': ('unit', S_ACT, None, 2, False),
    'gelu_tanh': ('unit', S_ACT, None, 3, False),
}


# ------------------------------------------------------------------------------------------------------------------
# stem: conv1 7x7/2 + folded BN + ReLU on the padded image (+ maxpool 3x3/2 pad 1 in the fused forms)
# ------------------------------------------------------------------------------------------------------------------
STEM_PH, STEM_PW, STEM_O, STEM_PO = 230, 232, 112, 56


def _stem_conv(img, wgt, dtype):
    """sum_{a<7, b<8, c<4} W[co,a,b,c] img[n, 2ho+a, 2wo+b, c] -> (n,112,112,64), image by image as one matrix product over the 224 taps"""
    wm = wgt.to(dtype).reshape(64, 224).t().contiguous()
    out = []
    for k in range(img.shape[0]):
        im = img[k].to(dtype).contiguous()
        patches = im.as_strided((STEM_O, STEM_O, 7, 32), (2 * STEM_PW * 4, 8, STEM_PW * 4, 1)).reshape(STEM_O * STEM_O, 224)
        out.append((patches @ wm).reshape(STEM_O, STEM_O, 64))
    return torch.stack(out)


def _pool64(t):
    return F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def stem_ref(img, wgt, b, pool=False):
    """img: (n,230,232,4) 16-bit, wgt: (64,7,8,4) 16-bit, b: (64) fp32.  out = relu(b[co] + sum W[co,a,b,c] img[n,2ho+a,2wo+b,c]) (n,112,112,64); pool: followed by
    the 3x3/2 pad-1 max pool (n,56,56,64).  Returns (ref, bound) float64.

    Bound: K = 224 exact products accumulated in fp32 (seven MFMAs of 32 terms, in any order): 224 u32 S; one rounding for + bias; ReLU; the rounding to
    storage u (|ref| + E) + SUB16.  The pooled forms take the maximum of the ROUNDED values.  Rounding is monotone, so that is the rounded maximum, and
    |max_i a_i - max_i b_i| <= max_i |a_i - b_i|: the reference is the maximum of the window's references and the bound the largest bound in the window
    (the padding is -inf for both, which is harmless after ReLU: test_pool_padding_is_harmless_after_relu)."""
    dt = dt_of(img)
    s = _stem_conv(img, wgt, torch.float64)
    S = _stem_conv(img.double().abs(), wgt.double().abs(), torch.float64)
    E = 224 * U32 * S
    pre = s + b.double()
    E = E + U32 * (pre.abs() + E)
    ref = pre.clamp_min(0.0)
    bound = _store_bound(ref, E, dt)
    if pool:
        ref, bound = _pool64(ref), _pool64(bound)
    return ref, bound


STEM_MUTANTS = ('tap7_dropped', 'row_origin_off_by_one', 'validity_ignored', 'pool_pads_with_zero', 'pool_window_2x2')
# pool_pads_with_zero is wrong only for a form without ReLU: it stays in the table to document why the kernels' zero identity is harmless
STEM_CAUGHT_BY = {'tap7_dropped': 'generic', 'row_origin_off_by_one': 'impulse', 'validity_ignored': 'uint8', 'pool_pads_with_zero': None,
                  'pool_window_2x2': 'generic'}


def stem_emulate(img, wgt, b, pool=False, mutant=None):
    """fp32 accumulation of the exact products, fp32 bias, ReLU, one rounding to storage, then the max pool on the rounded values"""
    assert mutant is None or mutant in STEM_MUTANTS
    sdt = img.dtype
    imgf, wf = img.float(), wgt.float()
    if mutant == 'tap7_dropped':
        wf = wf.clone(); wf[:, :, 7, :] = 0
    if mutant == 'validity_ignored':
        wf = wf.clone(); wf[:, :, :, 3] = 0
    if mutant == 'row_origin_off_by_one':
        imgf = torch.cat([imgf[:, 1:], torch.zeros_like(imgf[:, :1])], dim=1)
    o = (_stem_conv(imgf, wf, torch.float32) + b.float()).clamp_min(0.0).to(sdt)
    if not pool:
        return o
    of = o.float().permute(0, 3, 1, 2)
    if mutant == 'pool_window_2x2':
        p = F.max_pool2d(of, 2, 2, 0)
    elif mutant == 'pool_pads_with_zero':
        p = F.max_pool2d(F.pad(of, (1, 1, 1, 1), value=0.0), 3, 2, 0)
    else:
        p = F.max_pool2d(of, 3, 2, 1)
    return p.permute(0, 2, 3, 1).to(sdt)


STEM_FAMILIES = ('uint8', 'generic', 'impulse')
# impulse positions on the padded image (row, column): the four corners, the four edge midpoints, one interior pixel - more than 8 apart, so that no
# output sees two of them
STEM_IMPULSES = ((0, 0), (0, 231), (229, 0), (229, 231), (0, 116), (229, 116), (115, 0), (115, 231), (101, 77))


def stem_weights(family, dt, seed=29):
    """(64,7,8,4) weights in the storage type and the fp32 bias.  uint8: the production contract (fold_stem in encoder.hip): small image weights (the
    normalisation's 1 / (255 std) inside), larger weights on the validity channel (it carries -sum w mean / std), tap column 7 zero.  generic and impulse:
    every weight N(0, 1/224), column 7 and channel 3 included; impulse has a zero bias, so that its outputs are weights exactly."""
    tag = 'stem_%s' % family
    w = torch.from_numpy(synth.normal(seed, tag + 'w', (64, 7, 8, 4)))
    if family == 'uint8':
        w[..., :3] *= 0.002
        w[..., 3] *= 0.05
        w[:, :, 7, :] = 0
    else:
        w *= 224 ** -0.5
    b = torch.zeros(64) if family == 'impulse' else torch.from_numpy(synth.uniform(seed, tag + 'b', (64,), -0.5, 0.5))
    return round_to(w, dt), b


def stem_frames(n, h=224, w=224, seed=31):
    """uint8 (n,h,w,3) frames for the uint8 family; frame i does not depend on n"""
    return torch.cat([torch.from_numpy(synth.frames(seed, 1, h, w, 'stemu8_%d' % i)) for i in range(n)])


def stem_image_from_frames(frames, top, left, dt):
    """what the preprocess kernel writes for frames that need no resize: pixel (y,x) of the 224 x 224 window at [y+3][x+3], channels (R-128, G-128, B-128, 1),
    zero border - exact in both storage types"""
    n = frames.shape[0]
    img = torch.zeros(n, STEM_PH, STEM_PW, 4)
    img[:, 3:227, 3:227, :3] = frames[:, top:top + 224, left:left + 224, :].float() - 128.0
    img[:, 3:227, 3:227, 3] = 1.0
    return round_to(img, dt)


def stem_image(family, n, dt, seed=31):
    """(n,230,232,4) in the storage type; image i does not depend on n (a reference can be shared between batch sizes).  generic: N(0,1) everywhere, border
    included (the forms that read the padded image take any image); impulse: a single 1 at each of STEM_IMPULSES, in channel (j + i) mod 4 for impulse j
    of image i, zero elsewhere; uint8: stem_image_from_frames of stem_frames."""
    if family == 'uint8':
        return stem_image_from_frames(stem_frames(n, seed=seed), 0, 0, dt)
    if family == 'generic':
        return round_to(torch.stack([torch.from_numpy(synth.normal(seed, 'stem_generic_%d' % i, (STEM_PH, STEM_PW, 4))) for i in range(n)]), dt)
    assert family == 'impulse'
    img = torch.zeros(n, STEM_PH, STEM_PW, 4)
    for j, (y, x) in enumerate(STEM_IMPULSES):
        for i in range(n):
            img[i, y, x, (j + i) % 4] = 1.0
    return round_to(img, dt)


def stem_c1_inputs(dt, seed=37):
    """layer1.0.conv1 inside the fused stem: (64,1,1,64) weights in the storage type, fp32 bias"""
    w = torch.from_numpy(synth.normal(seed, 'stem_c1w', (64, 1, 1, 64))) * (2.0 / 64) ** 0.5
    return round_to(w, dt), torch.from_numpy(synth.uniform(seed, 'stem_c1b', (64,), -0.5, 0.5))


# ------------------------------------------------------------------------------------------------------------------
# pools, layout and format kernels
# ------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """x: (n,h,w,c) 16-bit -> (n,ho,wo,c) in the same type, 3x3 stride 2 pad 1 with -inf padding: the maximum of representable values is one of them, so
    the comparison is exact (as values: the sign of a zero that wins against the other zero is not defined).  NaN: the kernel's fmaxf drops a NaN
    (fmaxf(NaN, x) = x), torch.max_pool2d propagates it; the encoder never pools a NaN that it would not already have failed on, so the difference is
    documented here and not asserted."""
    return F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(x.dtype)


def maxpool_inputs(n, h, w, c, dt, seed=41):
    """N(0,1) (negative values in every window), a block of zeros of both signs, a constant window of a negative value, one image row of the most negative
    finite value (the -inf padding must not win against it)"""
    x = torch.from_numpy(synth.normal(seed, 'mp_%d_%d_%d_%d' % (n, h, w, c), (n, h, w, c)))
    x[0, :min(3, h), :min(3, w), :] = 0.0
    x[0, 0, 0, ::2] = -0.0
    x[-1, max(h - 3, 0):, max(w - 3, 0):, :] = -1.5
    x = round_to(x, dt)
    if h <= 3 or h >= 7:                                                    # (not across the marked blocks of a 5-row image)
        x[n // 2, h // 2, :, :] = torch.finfo(TORCH_DT[dt]).min
    return x


def avgpool_ref(x):
    """x: (n,hw,c) 16-bit or fp32 -> fp32 mean over hw, (ref, bound) float64 (n,c).  fp32 sum of hw exact values in some order (the hw = 49 form adds a tree,
    the generic loop runs in sequence): hw u32 sum |x|; the division by hw: one rounding."""
    xd = x.double()
    hw = x.shape[1]
    ref = xd.mean(dim=1)
    E = hw * U32 * xd.abs().sum(dim=1) / hw
    return ref, E + U32 * (ref.abs() + E)


def avgpool2_ref(x):
    """x: (n,h,w,c) 16-bit -> AvgPool2d(2) in the storage type: three fp32 additions (3 u32 sum |x|), an exact * 0.25, the rounding to storage"""
    dt = dt_of(x)
    n, h, w, c = x.shape
    xd = x.double().reshape(n, h // 2, 2, w // 2, 2, c)
    ref = xd.sum(dim=(2, 4)) * 0.25
    E = 3 * U32 * xd.abs().sum(dim=(2, 4)) * 0.25
    return ref, _store_bound(ref, E, dt)


def attnpool_tokens_ref(x, pos, dt):
    """x: (n,hw,c) fp32, pos: (hw+1,c) fp32 -> tokens (n,hw+1,c): token 0 = mean_p x[p] + pos[0] (sequential fp32 sum: hw u32 sum |x| / hw, the division, the
    addition), token 1+p = x[p] + pos[1+p] (one fp32 addition), each rounded to storage"""
    xd, pd = x.double(), pos.double()
    hw = x.shape[1]
    m = xd.mean(dim=1)
    Em = hw * U32 * xd.abs().mean(dim=1)
    Em = Em + U32 * (m.abs() + Em)
    t0 = m + pd[0]
    E0 = Em + U32 * (t0.abs() + Em)
    tp = xd + pd[1:]
    ref = torch.cat([t0[:, None], tp], dim=1)
    E = torch.cat([E0[:, None], U32 * tp.abs()], dim=1)
    return ref, _store_bound(ref, E, dt)


def nhwc_to_chw_ref(x, creal):
    """x: (n,hw,cpad) fp32 -> (n, creal*hw): out[b, ch*hw + i] = x[b, i, ch], an exact copy"""
    return x[:, :, :creal].permute(0, 2, 1).reshape(x.shape[0], -1).contiguous()


POOL_MUTANTS = ('avg_divides_by_hw_plus_1', 'avg_skips_last', 'chw_uses_creal_stride')


def avgpool_emulate(x, mutant=None):
    xf = x.float()
    hw = x.shape[1]
    s = torch.zeros(x.shape[0], x.shape[2])
    for i in range(hw - 1 if mutant == 'avg_skips_last' else hw):
        s = s + xf[:, i]
    return s / np.float32(hw + 1 if mutant == 'avg_divides_by_hw_plus_1' else hw)


def nhwc_to_chw_emulate(x, creal, mutant=None):
    n, hw, cpad = x.shape
    stride = creal if mutant == 'chw_uses_creal_stride' else cpad
    flat = x.reshape(n, -1)
    idx = (torch.arange(hw)[None, :] * stride + torch.arange(creal)[:, None]).reshape(-1)
    return flat[:, idx]


# ------------------------------------------------------------------------------------------------------------------
# the grids of tests/test_gpu_resnet_kernels.py (tests/test_resnet_kernel_refs_cpu.py runs the emulations over the same tables, before any GPU is involved)
# ------------------------------------------------------------------------------------------------------------------
_STD = ((None, 1, True), ('h', 1, True), ('f32', 0, False))           # (residual, activation, 16-bit output?)
_ACTS = ((None, 2, True), (None, 3, True), ('f32', 2, False), ('f32', 3, False))
# (shape (n,h,w,cin,cout,kh,kw,stride,pad), configurations, what it reaches)
CONV_GRID = [
    ((1, 5, 7, 64, 64, 3, 3, 1, 1), _STD, 'M = 35 below one tile, the <128,64> instance, all four borders in one tile; conv3x3_halo under auto'),
    ((1, 9, 11, 64, 72, 3, 3, 1, 1), _STD, 'cout tail'),
    ((3, 7, 7, 64, 128, 1, 1, 1, 0), _STD, 'K = 64: single stage; ragged M = 147'),
    ((2, 8, 8, 256, 128, 1, 1, 1, 0), (('h', 1, True), (None, 0, False)), 'the NK4 instance, exact tile'),
    ((2, 9, 8, 256, 128, 1, 1, 1, 0), (('h', 1, True), (None, 0, False)), 'the NK4 instance, ragged tile'),
    ((2, 9, 9, 128, 128, 3, 3, 2, 1), _STD, 'stride 2, odd size'),
    ((2, 8, 8, 128, 128, 3, 3, 2, 1), _STD, 'stride 2, even size'),
    ((1, 6, 6, 64, 64, 1, 1, 2, 0), _STD, 'strided 1x1'),
    ((2, 6, 6, 64, 64, 3, 3, 1, 0), _STD, 'no padding'),
    ((1, 150, 1, 128, 256, 1, 1, 1, 0), _ACTS, 'QuickGELU and erf-GELU epilogues'),
    ((1, 6, 7, 64, 72, 1, 3, 1, 1), _STD, 'a 1 x 3 filter: right or refused'),
    ((1, 7, 6, 64, 72, 3, 1, 1, 1), _STD, 'a 3 x 1 filter: right or refused'),
]
SPLITK_SHAPES = [(2, 7, 7, 128, 64, 3, 3, 1, 1), (2, 7, 7, 64, 136, 3, 3, 1, 1)]
SPLITK_KSPLITS = (2, 4, 5, 9)
SPLITK_CONFIGS = (('h', 1, True), (None, 0, False))
WFRAG_CASES = [((1, 7, 7, 64, 256, 3, 3, 1, 1), None), ((3, 7, 7, 128, 256, 1, 1, 1, 0), 'h'), ((2, 14, 14, 64, 256, 3, 3, 2, 1), None)]
DUAL_CASES = [(2, 7, 64, 64, 1, 64, 2), (2, 5, 64, 72, 3, 128, 2)]    # (n, ho, cin, cout, k, cin2, stride2)
MAXPOOL_GRID = [(2, 7, 9, 8), (1, 8, 6, 8), (3, 5, 5, 64), (2, 12, 10, 16), (1, 1, 3, 8)]
AVGPOOL_HW = (1, 7, 49, 50, 196)
AVGPOOL_C = (8, 64, 2048, 2056)
AVGPOOL2_GRID = [(2, 4, 6, 8), (1, 2, 2, 64), (3, 6, 4, 72)]
ATTNPOOL_GRID = [(1, 1, 8), (3, 9, 264), (2, 49, 2048)]               # (n, hw, c)
CHW_GRID = [(3, 49, 64, 42), (2, 196, 64, 11), (1, 5, 8, 8)]          # (n, hw, cpad, creal)


def conv_families(res, act):
    """the families a configuration can run: relu_edge needs a residual; exact and large state facts about the linear part (act 0 / 1)"""
    return tuple(f for f in CONV_FAMILIES if not (f == 'relu_edge' and not res) and not (f in ('exact', 'large') and act > 1))


def dual_inputs(case, dt, seed=43):
    """the two-operand form: x (n,ho,ho,cin), x2 (n,h2,h2,cin2) with h2 = ho*s2 - (s2-1), wt (cout,k,k,cin), w2 (cout,cin2), b"""
    n, ho, cin, cout, k, cin2, s2 = case
    tag = 'dual_%s' % '_'.join(str(v) for v in case)
    h2 = ho * s2 - (s2 - 1)
    K = k * k * cin + cin2
    nrm = lambda nm, shp: torch.from_numpy(synth.normal(seed, tag + nm, shp))
    x, x2 = round_to(nrm('x', (n, ho, ho, cin)), dt), round_to(nrm('y', (n, h2, h2, cin2)), dt)
    wt, w2 = round_to(nrm('w', (cout, k, k, cin)) * (2.0 / K) ** 0.5, dt), round_to(nrm('v', (cout, cin2)) * (2.0 / K) ** 0.5, dt)
    return x, x2, wt, w2, torch.from_numpy(synth.uniform(seed, tag + 'b', (cout,), -0.5, 0.5))


def pooled_conv_ref(x, wt, b, res):
    """conv_wfrag's pooled form: relu(1x1 conv + bias + 16-bit residual) in fp32, averaged over each frame's 49 pixels in fp32: the convolution's bound
    (before any output rounding) averaged, plus the fp32 sum of 49 terms and the division"""
    ref, bound = conv_ref(x, wt, b, res, 1, 1, 0, None)
    n, cout = x.shape[0], wt.shape[0]
    ref, bound = ref.reshape(n, 49, cout), bound.reshape(n, 49, cout)
    m = ref.mean(dim=1)
    E = bound.mean(dim=1) + 49 * U32 * (ref.abs() + bound).mean(dim=1)
    return m, E + U32 * (m.abs() + E)


def pool_inputs(shape, dt, name, seed=47):
    """N(0,1) + 0.5 of the given shape: dt 'f32' keeps fp32, else rounded to storage"""
    x = 0.5 + torch.from_numpy(synth.normal(seed, '%s_%s' % (name, '_'.join(str(v) for v in shape)), shape))
    return x if dt == 'f32' else round_to(x, dt)
