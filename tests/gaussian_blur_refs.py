"""References of the gaussian_blur and random_grayscale modes (tests/test_gaussian_blur_cpu.py, tests/test_gpu_gaussian_blur_kernels.py,
tests/test_gpu_gaussian_blur.py).

The arithmetic, three times:
  * torchvision's functional_tensor.gaussian_blur and rgb_to_grayscale restated LITERALLY in torch ops on uint8 CHW tensors (torchvision itself is not a
    dependency): the 1-D weights from torch.linspace, the 2-D kernel as their outer product in float32, reflect padding, one grouped conv2d in float32,
    torch.round and .to(uint8);
  * the EXACT blur: the same weights and the same sum in float64, not rounded to uint8 - the value the criterion is stated on;
  * an fp32 emulation of the separable kernel of csrc/preprocess.hip (blur_normalize_kernel): weights from a float32 exp and a float32 division, a
    horizontal and a vertical chain of float32 fmas in tap order, rintf.
and mutants of the emulation, which the criterion must reject: replicate padding, zero padding, taps shifted by one, sigma used as the variance, rounding
to uint8 between the passes, truncation instead of round-half-even, grayscale after the blur.

The criterion (blur_verdict): a uint8 result may differ from round-half-even of the exact value by at most ONE step anywhere, and must equal it wherever
the exact value is farther than DELTA from a .5 tie; the pixels DELTA leaves undecided may be at most 2 % of the image.

DELTA is a first-order bound on |fp32 separable sum - exact sum|, u = 2^-24 the unit roundoff of float32, values up to 255, weights that sum to 1:
  * the sums: each pass is a chain of 23 fmas, one rounding each of a partial sum of at most 255 -> 23 u 255 per pass; the vertical pass hands the
    horizontal pass's error on with weights that sum to 1, so the two add: 2 * 23 * 255 u;
  * the weights: pdf_i = exp(a_i), a_i = -0.5 (i / sigma)^2.  t = i / sigma is one correctly rounded division, relative error at most u; its square
    carries 2 u and the product's own rounding adds u (the halving is exact): a relative error of at most 3 u in a_i, so |a_i| 3 u pdf_i <= 3 u / e in
    pdf_i, since x exp(-x) <= 1 / e; tap 0 is 1 by definition, 22 taps remain; the sum of the pdfs is at least 1, so this is at most 22 * 3 u / e on
    the normalised weights of a pass together.  Relative to each weight: the device's expf, documented at 1 ulp = 2 u (HIP math API, single
    precision: expf, maximum error 1 ULP), the float32 sum of the 12 distinct positive pdfs, 12 u, and the division by it, correctly rounded
    (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt), u: 15 u.  A pixel moves by at most 255 times the summed weight error, and the 2-D
    weight is a product of two 1-D ones: 2 * 255 u (22 * 3 / e + 15).
DELTA = 255 u (46 + 2 (66 / e + 15)) = 1.89e-3.  It is not fitted to any result: on random uint8 images of 12 .. 224 pixels at sigma 0.5 .. 2, 0.7 % of
the pixels lie within 2e-3 of a tie, and the emulation below deviates from the exact value by less than 2e-4 (tests/test_gaussian_blur_cpu.py
asserts both)."""
import math

import numpy as np
import torch

from color_jitter_refs import MEAN, STD, normalize_nhwc4  # noqa: F401  (the tests take them from here)

KSIZE, R = 23, 11
U = 2.0 ** -24
DELTA = 255.0 * U * (2 * KSIZE + 2 * (22 * 3 / math.e + 15))
# the same bound for ONE fp32 sum of all 529 products (torchvision's conv2d, whatever its order): 529 roundings in place of 2 * 23
DELTA_2D = 255.0 * U * (KSIZE * KSIZE + 2 * (22 * 3 / math.e + 15))
MAX_SHARE = 0.02
SIGMA_MAX = 16.0


# ----------------------------------------------------------------------------------------------------------------------
# torchvision's functions, literally
# ----------------------------------------------------------------------------------------------------------------------
def _get_gaussian_kernel1d(kernel_size, sigma):
    ksize_half = (kernel_size - 1) * 0.5
    x = torch.linspace(-ksize_half, ksize_half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def _get_gaussian_kernel2d(kernel_size, sigma, dtype):
    kernel1d_x = _get_gaussian_kernel1d(kernel_size[0], sigma[0]).to(dtype=dtype)
    kernel1d_y = _get_gaussian_kernel1d(kernel_size[1], sigma[1]).to(dtype=dtype)
    return torch.mm(kernel1d_y[:, None], kernel1d_x[None, :])


def gaussian_blur(img, kernel_size, sigma):
    """img: (C, H, W) uint8"""
    kernel = _get_gaussian_kernel2d(kernel_size, sigma, dtype=torch.float32)
    kernel = kernel.expand(img.shape[-3], 1, kernel.shape[0], kernel.shape[1])
    x = img.unsqueeze(0).to(torch.float32)
    padding = [kernel_size[0] // 2, kernel_size[0] // 2, kernel_size[1] // 2, kernel_size[1] // 2]
    x = torch.nn.functional.pad(x, padding, mode='reflect')
    x = torch.nn.functional.conv2d(x, kernel, groups=x.shape[-3])
    return torch.round(x).to(torch.uint8).squeeze(0)


def rgb_to_grayscale3(img):
    """rgb_to_grayscale(img, num_output_channels=3) on a (3, H, W) uint8 tensor"""
    r, g, b = img.unbind(dim=-3)
    l_img = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype)
    return l_img.unsqueeze(dim=-3).expand(img.shape).contiguous()


def literal(hwc, sigma, gray):
    """one frame's uint8 (H, W, 3) image through RandomGrayscale's and GaussianBlur's functions as torchvision applies them (sigma 0: no blur)"""
    img = torch.from_numpy(np.ascontiguousarray(hwc)).permute(2, 0, 1).contiguous()
    if gray:
        img = rgb_to_grayscale3(img)
    if sigma > 0:
        img = gaussian_blur(img, [KSIZE, KSIZE], [float(sigma), float(sigma)])
    return img.permute(1, 2, 0).contiguous().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# what the kernel makes of a frame's two words
# ----------------------------------------------------------------------------------------------------------------------
def harden(sigma, gray):
    """a NaN or non-positive sigma is no blur, sigma is at most 16; any non-zero gray word is 1"""
    s = np.float32(sigma)
    s = float(min(s, np.float32(SIGMA_MAX))) if s > 0 else 0.0
    return s, int(int(gray) != 0)


def pack_params(rows):
    """rows (sigma, gray) -> the (n, 2) int32 array the device reads"""
    out = np.zeros((len(rows), 2), np.int32)
    for i, (sigma, gray) in enumerate(rows):
        out[i, 0] = np.array([sigma], np.float32).view(np.int32)[0]
        out[i, 1] = np.int64(gray).astype(np.int32)
    return out


def gray3(hwc):
    """gray_u8 of csrc/preprocess.hip on all three channels: trunc(((0.2989 r) + (0.587 g)) + (0.114 b)) in float32"""
    f = hwc.astype(np.float32)
    g = ((np.float32(0.2989) * f[..., 0] + np.float32(0.587) * f[..., 1]).astype(np.float32) + np.float32(0.114) * f[..., 2]).astype(np.float32)
    return np.repeat(np.trunc(g).astype(np.uint8)[..., None], 3, axis=-1)


# ----------------------------------------------------------------------------------------------------------------------
# the exact blur and the emulation with its mutants
# ----------------------------------------------------------------------------------------------------------------------
def _pad(a, mode):
    pad = ((R, R), (R, R)) + ((0, 0),) * (a.ndim - 2)
    if mode == 'zero':
        return np.pad(a, pad, mode='constant')
    return np.pad(a, pad, mode={'reflect': 'reflect', 'replicate': 'edge'}[mode])


def exact(hwc, sigma):
    """the exact blurred values, float64 (H, W, 3), not rounded: weights exp(-0.5 (i / sigma)^2) / sum in float64 from the float32 sigma"""
    s = float(np.float32(sigma))
    i = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 * (i / s) ** 2)
    w /= w.sum()
    p = _pad(hwc.astype(np.float64), 'reflect')
    H, W = hwc.shape[:2]
    h = sum(w[k] * p[:, k:k + W] for k in range(KSIZE))
    return sum(w[k] * h[k:k + H] for k in range(KSIZE))


def _fma(a, b, c):
    """fp32 fma of fp32 arrays (the product is exact in float64; the double rounding of the sum is far below what the criterion resolves)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel_weights(sigma, variance=False):
    """the 23 normalised float32 weights as blur_normalize_kernel makes them: tap 0 is 1, exp in float32, the 11 pdfs summed from the outermost
    inwards, doubled, plus tap 0, one division each"""
    f32 = np.float32
    s = f32(sigma)
    with np.errstate(over='ignore', under='ignore'):
        t = np.arange(R + 1, dtype=f32) / s
        arg = (f32(-0.5) * ((t * t).astype(f32) if not variance else (np.arange(R + 1, dtype=f32) ** 2 / s).astype(f32))).astype(f32)
        pdf = np.exp(arg).astype(f32)
    pdf[0] = f32(1)
    total = f32(0)
    for i in range(R, 0, -1):
        total = f32(total + pdf[i])
    total = f32(f32(2) * total + pdf[0])
    half = (pdf / total).astype(f32)
    return np.concatenate([half[:0:-1], half])


def emulate_values(hwc, sigma, pad='reflect', shift=0, variance=False, round_between=False):
    """the separable fp32 blur of one uint8 (H, W, 3) image -> the float32 sums before the final rounding.  The keywords are the mutants: pad
    'replicate' or 'zero', shift 1 (every tap reads one pixel further right and down), variance (exp(-0.5 i^2 / sigma)), round_between (uint8 between
    the passes)"""
    w = kernel_weights(sigma, variance)
    p = _pad(hwc.astype(np.float32), pad)
    if shift:
        p = np.roll(p, (-shift, -shift), axis=(0, 1))
    H, W = hwc.shape[:2]
    h = np.zeros((H + 2 * R, W, 3), np.float32)
    for k in range(KSIZE):
        h = _fma(w[k], p[:, k:k + W], h)
    if round_between:
        h = np.rint(h).astype(np.float32)
    v = np.zeros((H, W, 3), np.float32)
    for k in range(KSIZE):
        v = _fma(w[k], h[k:k + H], v)
    return v


def emulate(hwc, sigma, final='rint', **mutant):
    """emulate_values rounded to uint8 as the kernel rounds: rint (half to even), or the mutant final 'trunc'"""
    v = emulate_values(hwc, sigma, **mutant)
    v = np.rint(v) if final == 'rint' else np.trunc(v)
    return np.clip(v, 0, 255).astype(np.uint8)


def augment(hwc, sigma, gray, gray_after=False, **mutant):
    """one frame as the kernel treats it: harden, grayscale if flagged, blur if sigma > 0 (gray_after: the mutant order)"""
    sigma, gray = harden(sigma, gray)
    img = hwc
    if gray and not gray_after:
        img = gray3(img)
    if sigma > 0:
        img = emulate(img, sigma, **mutant)
    if gray and gray_after:
        img = gray3(img)
    return img


def exact_augmented(hwc, sigma, gray):
    """the exact value of a frame's augmented image: float64, integers where no blur acts"""
    sigma, gray = harden(sigma, gray)
    img = gray3(hwc) if gray else hwc
    return exact(img, sigma) if sigma > 0 else img.astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# the criterion
# ----------------------------------------------------------------------------------------------------------------------
def blur_verdict(got_u8, exact_values, delta=DELTA):
    """-> dict(max_step, undecided: the share of values within delta of a .5 tie, wrong: the number of decided values that differ from round-half-even
    of the exact value, ok)"""
    want = np.rint(exact_values)
    tie = np.abs(exact_values - np.floor(exact_values) - 0.5) <= delta
    diff = np.abs(got_u8.astype(np.int64) - want.astype(np.int64))
    v = dict(max_step=int(diff.max()), undecided=float(tie.mean()), wrong=int(((diff != 0) & ~tie).sum()))
    v['ok'] = v['max_step'] <= 1 and v['wrong'] == 0 and v['undecided'] <= MAX_SHARE
    return v


# ----------------------------------------------------------------------------------------------------------------------
# inputs and the way back from the normalised image
# ----------------------------------------------------------------------------------------------------------------------
def families(size, seed=0):
    """the input families at one size: name -> uint8 (size, size, 3)"""
    rng = np.random.default_rng(seed + size)
    # 7 .. 241: a blurred integer ramp meets exact .5 ties by symmetry wherever neighbours differ by an odd step; with these ends the exact reference
    # keeps the tied values of every size and sigma the tests use below the criterion's 2 % (0 .. 255 puts one channel column of the 12 x 12 ramp, 2.8 %,
    # on a tie)
    ramp = np.round(np.linspace(7, 241, size)).astype(np.uint8)
    corner = np.zeros((size, size, 3), np.uint8)
    corner[0, 0] = (255, 200, 90)
    return {'random': rng.integers(0, 256, (size, size, 3), dtype=np.uint8),
            'constant255': np.full((size, size, 3), 255, np.uint8),
            'corner': corner,
            'ramp_x': np.ascontiguousarray(np.broadcast_to(ramp[None, :, None], (size, size, 3)) // np.array([1, 2, 3], np.uint8)),
            'ramp_y': np.ascontiguousarray(np.broadcast_to(ramp[:, None, None], (size, size, 3)) // np.array([3, 1, 2], np.uint8))}


def recover_u8(image):
    """the fp32 NHWC4 image -> the uint8 values (…, 3) it normalises: (v / 255 - mean) / std is strictly increasing in v, so every value is looked up in
    the table of the 256 possible ones; a value that is in no table is an AssertionError"""
    table = (np.arange(256, dtype=np.float32)[:, None] / np.float32(255.0) - MEAN) / STD           # (256, 3)
    out = np.zeros(image.shape[:-1] + (3,), np.uint8)
    assert (image[..., 3] == 0).all()
    for c in range(3):
        idx = np.clip(np.searchsorted(table[:, c], image[..., c]), 0, 255)
        assert np.array_equal(table[idx, c], image[..., c]), 'channel %d holds values that no uint8 normalises to' % c
        out[..., c] = idx
    return out
