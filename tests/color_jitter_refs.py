"""References of the color_jitter mode (tests/test_color_jitter_cpu.py, tests/test_gpu_color_jitter_kernels.py, tests/test_gpu_color_jitter.py).

The arithmetic: torchvision's four tensor functions (functional_tensor.rgb_to_grayscale, _blend, adjust_brightness / adjust_contrast /
adjust_saturation) restated LITERALLY in torch ops on uint8 CHW tensors - torchvision itself is not a dependency.  On a uint8 tensor
`0.2989 * r` is a float32 product, every `+` a float32 sum, nothing is fused, and `.to(uint8)` truncates.  Three mutants of it, which the bit-exact
comparisons must reject: a fused multiply-add in the blend, rounding instead of truncation, and contrast's mean taken before the preceding ops.

The draw: Philox-4x32-10 and csrc/sample_rng.h's color_params restated in numpy with integer arithmetic and an exactly rounded fma.

The resize: preprocess_windows_f32_kernel's tap order in numpy, copied from tests/test_random_crop_cpu.py (which proves it equal to the oracle)."""
import numpy as np
import torch

from pvr_habitat_amd import embeddings as E

# order code -> the frame's ops: the permutations of (brightness, contrast, saturation) in lexicographic order
PERMS = ('bcs', 'bsc', 'cbs', 'csb', 'sbc', 'scb')
MEAN, STD = np.array(E.IMAGENET_MEAN, np.float32), np.array(E.IMAGENET_STD, np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# torchvision's functions, literally
# ----------------------------------------------------------------------------------------------------------------------
def rgb_to_grayscale(img):
    r, g, b = img.unbind(dim=-3)
    l_img = (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype)
    return l_img.unsqueeze(dim=-3)


def _blend(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).to(img1.dtype)


def adjust_brightness(img, factor):
    return _blend(img, torch.zeros_like(img), factor)


def adjust_contrast(img, factor):
    mean = torch.mean(rgb_to_grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
    return _blend(img, mean, factor)


def adjust_saturation(img, factor):
    return _blend(img, rgb_to_grayscale(img), factor)


# ----------------------------------------------------------------------------------------------------------------------
# the mutants' blends
# ----------------------------------------------------------------------------------------------------------------------
def _blend_fma(img1, img2, ratio):
    """ratio * img1 + round32((1 - ratio) * img2) as ONE rounding: the float64 sum of an exact product and a float32 value, rounded to float32"""
    ratio = float(ratio)
    second = ((1.0 - ratio) * img2).to(torch.float32).to(torch.float64)
    fused = (ratio * img1.to(torch.float64) + second).to(torch.float32)
    return fused.clamp(0, 255).to(img1.dtype)


def _blend_round(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255).round().to(img1.dtype)


def harden(b, c, s, order):
    """what the kernels make of a frame's four words: a NaN factor is 1, a factor is clamped to [0, 4], an order outside 0 .. 5 is 0"""
    f = [1.0 if np.isnan(x) else float(min(max(np.float32(x), np.float32(0)), np.float32(4))) for x in (b, c, s)]
    return f[0], f[1], f[2], (int(order) if 0 <= int(order) <= 5 else 0)


def jitter(window_hwc, b, c, s, order, mutant=None):
    """one frame's uint8 (crop, crop, 3) window through its three ops -> uint8 (crop, crop, 3).  mutant: None, 'fma', 'round' or 'mean_first'"""
    b, c, s, order = harden(b, c, s, order)
    img = torch.from_numpy(np.ascontiguousarray(window_hwc)).permute(2, 0, 1).contiguous()
    assert img.dtype == torch.uint8
    blend = {None: _blend, 'mean_first': _blend, 'fma': _blend_fma, 'round': _blend_round}[mutant]
    first_mean = torch.mean(rgb_to_grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
    for op in PERMS[order]:
        if op == 'b':
            img = blend(img, torch.zeros_like(img), b)
        elif op == 's':
            img = blend(img, rgb_to_grayscale(img), s)
        else:
            mean = first_mean if mutant == 'mean_first' else torch.mean(rgb_to_grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
            img = blend(img, mean, c)
        assert img.dtype == torch.uint8
    return img.permute(1, 2, 0).contiguous().numpy()


def jitter_literal(window_hwc, b, c, s, order):
    """the same through the adjust_* functions themselves (the unmutated path of jitter must equal it)"""
    img = torch.from_numpy(np.ascontiguousarray(window_hwc)).permute(2, 0, 1).contiguous()
    fn = {'b': (adjust_brightness, b), 'c': (adjust_contrast, c), 's': (adjust_saturation, s)}
    for op in PERMS[order]:
        img = fn[op][0](img, fn[op][1])
    return img.permute(1, 2, 0).contiguous().numpy()


def normalize_nhwc4(u8):
    """(n, crop, crop, 3) uint8 -> the fp32 NHWC4 image: (v / 255 - mean) / std in float32, one rounding per operation; channel 3 = 0"""
    out = np.zeros(u8.shape[:3] + (4,), np.float32)
    out[..., :3] = (u8.astype(np.float32) / np.float32(255.0) - MEAN) / STD
    assert out.dtype == np.float32
    return out


def windows_of(resized, windows, crop):
    """(n, rh, rw, 3) resized uint8 frames, (n, 2) in-range windows -> (n, crop, crop, 3)"""
    return np.stack([resized[i, t:t + crop, l:l + crop] for i, (t, l) in enumerate(np.asarray(windows).tolist())])


def jittered_windows(resized, windows, params, crop, mutant=None):
    """every frame's window through its own parameters; params: rows (b, c, s, order)"""
    win = windows_of(resized, windows, crop)
    return np.stack([jitter(win[i], *params[i], mutant=mutant) for i in range(len(win))])


def pack_params(rows):
    """rows (b, c, s, order) -> the (n, 4) int32 array the device reads: three float32 bit patterns and the order"""
    out = np.zeros((len(rows), 4), np.int32)
    for i, (b, c, s, order) in enumerate(rows):
        out[i, :3] = np.array([b, c, s], np.float32).view(np.int32)
        out[i, 3] = order
    return out


def unpack_params(structured):
    """E.color_params' structured array -> rows (b, c, s, order) of Python numbers that hold the float32 values exactly"""
    return [(float(r['b']), float(r['c']), float(r['s']), int(r['order'])) for r in structured]


# ----------------------------------------------------------------------------------------------------------------------
# the draw
# ----------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, k0, k1):
    """(n, 4) uint32 counters, two 32-bit key words -> (n, 4) uint32 after ten rounds"""
    c = [counter[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(c, axis=1).astype(np.uint32)


def fma32(a, b, c):
    """the correctly rounded float32 fma of float32 arrays.  a * b is exact in float64; its sum with c is rounded to float64 TO ODD (the TwoSum error
    says whether and where the exact sum lies off the float64 one), after which the rounding to float32 is the rounding of the exact value"""
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    r = p + c64
    t = r - p
    err = (p - (r - t)) + (c64 - t)                             # exact: r + err = p + c64
    even = (r.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    r = np.where((err != 0) & even, np.nextafter(r, toward), r)
    return r.astype(np.float32)


def color_params(seed, call, n, strengths, first_frame=0):
    """sample_rng.h's color_params for frames first_frame .. first_frame + n -> (b, c, s) float32 (n, 3) and order int32 (n,)"""
    f32 = np.float32
    frame = np.arange(first_frame, first_frame + n, dtype=np.uint64)
    counter = np.stack([frame & _M32, frame >> np.uint64(32), np.full(n, call & 0xFFFFFFFF, np.uint64), np.full(n, call >> 32, np.uint64)],
                       axis=1).astype(np.uint32)
    bits = philox4x32_10(counter, seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ 0x434F4C52)
    factors = np.zeros((n, 3), f32)
    for j, s in enumerate(strengths):
        s = f32(s)
        lo, hi = max(f32(0), f32(1) - s), f32(1) + s
        u = ((bits[:, j] >> np.uint32(9)).astype(f32) + f32(0.5)) * f32(1.0 / 8388608.0)       # exact: 23 bits + a half, times 2^-23
        factors[:, j] = fma32(np.full(n, f32(hi - lo), f32), u, np.full(n, lo, f32))
    order = ((bits[:, 3].astype(np.uint64) * np.uint64(6)) >> np.uint64(32)).astype(np.int32)
    return factors, order


# ----------------------------------------------------------------------------------------------------------------------
# the resize (tests/test_random_crop_cpu.py: _resize_as_the_kernel)
# ----------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma of fp32 arrays: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resize_as_the_kernel(fr, size=256):
    """preprocess_windows_f32_kernel's resize of whole (n, h, w, 3) uint8 frames in numpy float32: src = fma(scale, dst + 0.5, -0.5) clamped at 0, every
    two-tap sum w0 a + w1 b as fma(w0, a, round(w1 b)), along x and then along y, rint"""
    f32 = np.float32
    n, h, w, _ = fr.shape
    rh, rw = E.resized_size(h, w, size)
    if (rh, rw) == (h, w):
        return fr.copy()

    def axis(insz, outsz):
        scale = np.full(outsz, f32(insz) / f32(outsz), f32)
        src = np.maximum(_fma(scale, np.arange(outsz, dtype=f32) + f32(0.5), np.full(outsz, -0.5, f32)), f32(0))
        i0 = src.astype(np.int32)
        lam = (src - i0.astype(f32)).astype(f32)
        return i0, i0 + (i0 < insz - 1), lam, (f32(1) - lam).astype(f32)
    y0, y1, ly, hy = axis(h, rh)
    x0, x1, lx, hx = axis(w, rw)
    F = fr.astype(f32)
    wx = lambda v: np.broadcast_to(v.reshape(1, 1, -1, 1), (n, rh, rw, 3))
    wy = lambda v: np.broadcast_to(v.reshape(1, -1, 1, 1), (n, rh, rw, 3))
    two = lambda w0, a, w1, b: _fma(w0, a, (w1 * b).astype(f32))
    top = two(wx(hx), F[:, y0][:, :, x0], wx(lx), F[:, y0][:, :, x1])
    bottom = two(wx(hx), F[:, y1][:, :, x0], wx(lx), F[:, y1][:, :, x1])
    return np.rint(two(wy(hy), top, wy(ly), bottom)).astype(np.uint8)
