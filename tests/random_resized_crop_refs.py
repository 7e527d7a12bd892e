"""References of the random_resized_crop mode (tests/test_random_resized_crop_cpu.py, tests/test_gpu_random_resized_crop_kernels.py,
tests/test_gpu_random_resized_crop.py).

The draw: torchvision's RandomResizedCrop.get_params restated in numpy with its own continuous log-uniform ratio and numpy's generator - the
DISTRIBUTION the library's Philox draw is held to, not its bits.

The image, twice.  The oracle form is what torchvision's resized_crop does to a uint8 tensor: F.interpolate(bilinear, align_corners=False) of the
cropped array, .round(), uint8.  The kernel form restates rect_pixel (csrc/preprocess.hip) in numpy float32 with an exactly rounded fma: per axis
scale = (float)size / (float)crop, src = fma(scale, dst + 0.5, -0.5) clamped at 0, taps clamped to the RECTANGLE's last row and column and offset by
(top, left), every two-tap sum w0 a + w1 b as fma(w0, a, round(w1 b)) along x and then along y, rint.  Two mutants of the kernel form, which the
bit-exact comparisons must reject: 'frame_clamp' clamps the second tap to the frame's last row and column instead of the rectangle's (it reads the
pixels next to the rectangle), 'swapped' takes (top, left) as (left, top)."""
import numpy as np
import torch
import torch.nn.functional as F

from color_jitter_refs import fma32

RATIO = (3.0 / 4.0, 4.0 / 3.0)


# ----------------------------------------------------------------------------------------------------------------------
# the draw
# ----------------------------------------------------------------------------------------------------------------------
def get_params(rng, n, h, w, scale, ratio=RATIO):
    """n independent draws of torchvision's RandomResizedCrop.get_params on an (h, w) frame -> ((n, 4) int64 (top, left, height, width), the share of
    draws that took the fallback).  Ten tries of area = h w U(scale), log r = U(log ratio), width = round(sqrt(area r)), height = round(sqrt(area / r))
    (Python's round: half to even), accepted if 0 < width <= w and 0 < height <= h, with top = randint(0, h - height) and left likewise; then the
    fallback: the whole frame if w / h lies in the ratio range, else the centred rectangle of the nearest bound"""
    out = np.zeros((n, 4), np.int64)
    done = np.zeros(n, bool)
    for _ in range(10):
        area = h * w * rng.uniform(scale[0], scale[1], n)
        r = np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1]), n))
        cw, ch = np.rint(np.sqrt(area * r)).astype(np.int64), np.rint(np.sqrt(area / r)).astype(np.int64)
        top = np.floor(rng.random(n) * (h - ch + 1)).astype(np.int64)
        left = np.floor(rng.random(n) * (w - cw + 1)).astype(np.int64)
        ok = ~done & (0 < cw) & (cw <= w) & (0 < ch) & (ch <= h)
        out[ok] = np.stack([top, left, ch, cw], axis=1)[ok]
        done |= ok
    out[~done] = fallback(h, w, ratio)
    return out, float((~done).mean())


def fallback(h, w, ratio=RATIO):
    """get_params' last lines, literally"""
    in_ratio = float(w) / float(h)
    if in_ratio < min(ratio):
        cw = w
        ch = int(round(cw / min(ratio)))
    elif in_ratio > max(ratio):
        ch = h
        cw = int(round(ch * max(ratio)))
    else:
        cw, ch = w, h
    return [(h - ch) // 2, (w - cw) // 2, ch, cw]


# ----------------------------------------------------------------------------------------------------------------------
# the image
# ----------------------------------------------------------------------------------------------------------------------
def clamp_rect(rect, h, w):
    """what rect_pixel makes of a frame's four words: height in [1, h], width in [1, w], top in [0, h - height], left in [0, w - width]"""
    top, left, rh, rw = (int(v) for v in rect)
    rh, rw = min(max(rh, 1), h), min(max(rw, 1), w)
    return min(max(top, 0), h - rh), min(max(left, 0), w - rw), rh, rw


def oracle_resized_crop(frame, rect, crop):
    """(h, w, 3) uint8, an in-range rectangle -> (crop, crop, 3) uint8: the oracle form"""
    top, left, rh, rw = (int(v) for v in rect)
    assert 0 <= top and 0 <= left and rh >= 1 and rw >= 1 and top + rh <= frame.shape[0] and left + rw <= frame.shape[1], rect
    x = torch.from_numpy(np.ascontiguousarray(frame[top:top + rh, left:left + rw])).permute(2, 0, 1)[None].float()
    y = F.interpolate(x, size=(crop, crop), mode='bilinear', align_corners=False)
    return y.round().to(torch.uint8)[0].permute(1, 2, 0).contiguous().numpy()


def kernel_resized_crop(frame, rect, crop, mutant=None):
    """(h, w, 3) uint8, any four words -> (crop, crop, 3) uint8: the kernel form.  mutant: None, 'frame_clamp' or 'swapped'"""
    f32 = np.float32
    h, w = frame.shape[:2]
    top, left, rh, rw = clamp_rect(rect, h, w)
    if mutant == 'swapped':
        top, left = min(left, h - rh), min(top, w - rw)
    if rh == crop and rw == crop:
        return frame[top:top + crop, left:left + crop].copy()

    def axis(size, off, frame_size):
        scale = np.full(crop, f32(size) / f32(crop), f32)
        src = np.maximum(fma32(scale, np.arange(crop, dtype=f32) + f32(0.5), np.full(crop, -0.5, f32)), f32(0))
        i0 = np.minimum(src.astype(np.int32), size - 1)
        lam = (src - i0.astype(f32)).astype(f32)
        last = frame_size - 1 - off if mutant == 'frame_clamp' else size - 1
        return i0 + off, i0 + (i0 < last) + off, lam, (f32(1) - lam).astype(f32)
    y0, y1, ly, hy = axis(rh, top, h)
    x0, x1, lx, hx = axis(rw, left, w)
    img = frame.astype(f32)
    wx = lambda v: np.ascontiguousarray(np.broadcast_to(v.reshape(1, -1, 1), (crop, crop, 3)))
    wy = lambda v: np.ascontiguousarray(np.broadcast_to(v.reshape(-1, 1, 1), (crop, crop, 3)))
    two = lambda w0, a, w1, b: fma32(w0, a, (w1 * b).astype(f32))
    upper = two(wx(hx), img[y0][:, x0], wx(lx), img[y0][:, x1])
    lower = two(wx(hx), img[y1][:, x0], wx(lx), img[y1][:, x1])
    return np.rint(two(wy(hy), upper, wy(ly), lower)).astype(np.uint8)


def resized_crops(frames, rects, crop, form=oracle_resized_crop, **kw):
    """every frame's rectangle -> (n, crop, crop, 3) uint8"""
    return np.stack([form(frames[i], rects[i], crop, **kw) for i in range(len(frames))])
