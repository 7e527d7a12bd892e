"""The kernels of the random_resized_crop mode on the GPU: pvr_op_crop_rects against pvr_host_crop_rects, and pvr_op_preprocess_rects (uint8 frames ->
each frame's own rectangle resized to crop x crop -> [brightness, contrast, saturation per frame] -> the normalised fp32 NHWC4 image) against the
oracle form of tests/random_resized_crop_refs.py - F.interpolate on the cropped array, .round(), uint8 - followed by / 255 and Normalize in torch
fp32, and with colour by tests/color_jitter_refs.py's literal restatement of torchvision's functions on the oracle's uint8 image.

Everything is compared with array_equal on the fp32 image.  5 frames of 64 x 64 and 2 of 300 x 260 (smooth frames, one of each size with noise), run
once per rectangle set: every frame of a size gets the set's rectangle k in run k."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_jitter_refs as R
import random_resized_crop_refs as RR
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

PVR_ERR_INVALID = 1
CROP = 224
# (top, left, height, width), five per run on the 64 x 64 frames: the four corners' single pixels; a row and a column; the whole frame; 37 x 29 ending
# at the last row and column; and, for the taps at the rectangle's edge to have neighbours in the frame, 28 x 28, 37 x 29 and 25 x 33 inside it
SMALL = [[(0, 0, 1, 1), (0, 63, 1, 1), (63, 0, 1, 1), (63, 63, 1, 1), (5, 0, 1, 64)],
         [(0, 9, 64, 1), (0, 0, 64, 64), (27, 35, 37, 29), (3, 30, 28, 28), (11, 7, 25, 33)]]
# two per run on the 300 x 260 frames: 224 x 224 (a plain copy) and 260 x 230 (down-scale); the whole frame and 37 x 29 inside
LARGE = [[(76, 36, 224, 224), (20, 15, 260, 230)], [(0, 0, 300, 260), (100, 200, 37, 29)]]
# (brightness, contrast, saturation, order): contrast is not the identity in any frame, every order occurs
PARAMS = [(2.0, 1.7, 1.0, 0), (1.0, 0.5, 0.3, 1), (0.6, 1.4, 1.8, 2), (1.3, 0.5, 0.0, 3), (1.2, 2.0, 2.0, 4), (0.9, 0.0, 1.5, 5), (1.1, 1.3, 0.7, 2)]
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _frames(h, w, n):
    """n frames of (h, w), the last one noise: on the host and on the device, once per size"""
    if (h, w) not in _cache:
        fr = synth.smooth_frames(11, n, h, w)
        fr[n - 1] = np.random.default_rng(2).integers(0, 256, fr[0].shape, dtype=np.uint8)
        _cache[(h, w)] = (fr, torch.from_numpy(fr).cuda())
    return _cache[(h, w)]


def _run(dev, rects, crop=CROP, packed=None, out=None):
    n, h, w, _ = dev.shape
    rc = torch.from_numpy(np.ascontiguousarray(rects, np.int32)).cuda()
    out = torch.full((n, crop, crop, 4), float('nan'), device='cuda') if out is None else out
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    col = None if packed is None else torch.from_numpy(packed).cuda()
    sums = None if packed is None else torch.full((n + 1,), 123456789, dtype=torch.int32, device='cuda')     # stale scratch: the entry point zeroes what it uses
    _lib.check(_lib.lib().pvr_op_preprocess_rects(vp(dev), n, h, w, crop, mean, std, vp(rc), vp(col), vp(sums), vp(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert sums is None or int(sums[n]) == 123456789            # n sums and nothing else
    return out.cpu().numpy()


def _normalize_in_torch(u8):
    """the oracle's uint8 image -> / 255 -> Normalize in torch fp32 -> NHWC4 with channel 3 = 0"""
    x = torch.from_numpy(u8).float() / 255.0
    x = (x - torch.tensor(E.IMAGENET_MEAN, dtype=torch.float32)) / torch.tensor(E.IMAGENET_STD, dtype=torch.float32)
    assert x.dtype == torch.float32
    return torch.cat([x, torch.zeros(u8.shape[:3] + (1,))], dim=-1).numpy()


CASES = [('64x64', 64, 64, 5, SMALL[0]), ('64x64', 64, 64, 5, SMALL[1]), ('300x260', 300, 260, 2, LARGE[0]), ('300x260', 300, 260, 2, LARGE[1])]
IDS = ['64x64_pixels_and_row', '64x64_column_whole_and_inside', '300x260_copy_and_downscale', '300x260_whole_and_inside']


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_preprocess_rects_against_the_oracle_form(case):
    _, h, w, n, rects = case
    fr, dev = _frames(h, w, n)
    got = _run(dev, rects)
    want = _normalize_in_torch(RR.resized_crops(fr, rects, CROP))
    assert np.isfinite(got).all() and (got[..., 3] == 0).all()
    for i in range(n):
        bad = got[i] != want[i]
        print('[preprocess rects %dx%d] frame %d, rectangle %s: %d of %d values differ' % (h, w, i, rects[i], int(bad.sum()), bad.size))
    assert np.array_equal(got, want)
    # the comparison is sharp enough to tell the mutants from the kernel, wherever a mutant can differ at all
    for mutant in ('frame_clamp', 'swapped'):
        differs = [not np.array_equal(RR.kernel_resized_crop(fr[i], rects[i], CROP, mutant=mutant), RR.oracle_resized_crop(fr[i], rects[i], CROP))
                   for i in range(n)]
        wrong = _normalize_in_torch(RR.resized_crops(fr, rects, CROP, form=RR.kernel_resized_crop, mutant=mutant))
        assert any(differs) == (not np.array_equal(wrong, got)), mutant
        _cache.setdefault(('rejected', mutant), set()).update((h, w, rects[i]) for i in range(n) if differs[i])


def test_the_cases_reject_both_mutants():
    """(after the cases above) frame_clamp shows on the up-scaled rectangles inside their frames, swapped wherever top != left"""
    for case in CASES:
        if not all(('rejected', m) in _cache for m in ('frame_clamp', 'swapped')):
            test_preprocess_rects_against_the_oracle_form(case)
    assert {(64, 64, (3, 30, 28, 28)), (64, 64, (11, 7, 25, 33)), (300, 260, (100, 200, 37, 29))} <= _cache[('rejected', 'frame_clamp')]
    assert {(64, 64, (0, 63, 1, 1)), (64, 64, (5, 0, 1, 64)), (64, 64, (27, 35, 37, 29)), (300, 260, (20, 15, 260, 230)),
            (300, 260, (76, 36, 224, 224))} <= _cache[('rejected', 'swapped')]


def test_a_crop_that_is_no_multiple_of_the_tile():
    """crop 37: the last block of a row and of a column is partly outside the image.  The reference here is the numpy restatement of the kernel's
    rounding order, not the oracle form: the order was matched to ATen's at the trainer's 224 x 224, and at 37 x 37 ATen's host kernel sums one value
    of these frames differently (rectangle (7, 9, 48, 53) of frame 0, output (11, 21), channel 2: exactly 203.4999943, 203 there and a 203.5 tie,
    so 204, in the restated order)"""
    fr, dev = _frames(64, 64, 5)
    rects = [tuple(r) for r in E.crop_rects(4, 1, 5, 64, 64, (0.2, 1.0)).tolist()]
    got = _run(dev, rects, crop=37)
    want = RR.resized_crops(fr, rects, 37, form=RR.kernel_resized_crop)
    assert np.array_equal(got, _normalize_in_torch(want))
    assert int((want != RR.resized_crops(fr, rects, 37)).sum()) <= 1


def test_hostile_rectangles_give_the_clamped_rectangles_image():
    fr, dev = _frames(64, 64, 5)
    big = 2 ** 31 - 1
    wild = [(-5, -1, 20, 30), (50, 60, 40, 40), (3, 4, 0, 0), (-big - 1, big, -7, big), (big, -big, big, -big - 1)]
    tame = [RR.clamp_rect(r, 64, 64) for r in wild]
    assert tame == [(0, 0, 20, 30), (24, 24, 40, 40), (3, 4, 1, 1), (0, 0, 1, 64), (0, 0, 64, 1)]
    a, b = _run(dev, wild), _run(dev, tame)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(b, _normalize_in_torch(RR.resized_crops(fr, tame, CROP)))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_preprocess_rects_with_colour_against_the_reference(case):
    _, h, w, n, rects = case
    fr, dev = _frames(h, w, n)
    params = PARAMS[:n]
    assert all(p[1] != 1.0 for p in params)
    u8 = RR.resized_crops(fr, rects, CROP)
    want_u8 = np.stack([R.jitter(u8[i], *params[i]) for i in range(n)])
    got = _run(dev, rects, packed=R.pack_params(params))
    assert np.isfinite(got).all() and np.array_equal(got, _normalize_in_torch(want_u8))
    assert np.array_equal(_normalize_in_torch(want_u8), R.normalize_nhwc4(want_u8))            # the two statements of / 255 and Normalize agree
    for mutant in ('fma', 'round', 'mean_first'):               # the colour reference's own mutants stay rejected on this source
        assert not np.array_equal(_normalize_in_torch(np.stack([R.jitter(u8[i], *params[i], mutant=mutant) for i in range(n)])), got), mutant
    for mutant in ('frame_clamp', 'swapped'):                   # and the resize's mutants wherever they can differ at all
        wrong = RR.resized_crops(fr, rects, CROP, form=RR.kernel_resized_crop, mutant=mutant)
        assert (not np.array_equal(wrong, u8)) == (not np.array_equal(_normalize_in_torch(np.stack([R.jitter(wrong[i], *params[i]) for i in range(n)])),
                                                                      got)), mutant
    # identity factors in any order: the bits of the launch without colour
    ones = R.pack_params([(1.0, 1.0, 1.0, k % 6) for k in range(n)])
    assert np.array_equal(_run(dev, rects, packed=ones).view(np.uint32), _run(dev, rects).view(np.uint32))


def test_two_runs_give_the_same_bits():
    fr, dev = _frames(64, 64, 5)
    packed = R.pack_params(PARAMS[:5])
    for kw in ({}, {'packed': packed}):
        a, b = _run(dev, SMALL[1], **kw), _run(dev, SMALL[1], **kw)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_leave_out_untouched():
    L = _lib.lib()
    fr, dev = _frames(64, 64, 5)
    n = 5
    rc, col = torch.from_numpy(np.array(SMALL[1], np.int32)).cuda(), torch.from_numpy(R.pack_params(PARAMS[:n])).cuda()
    sums = torch.zeros((n + 1,), dtype=torch.int32, device='cuda')
    out = torch.full((n, CROP, CROP, 4), float('nan'), device='cuda')
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    ok = dict(frames=vp(dev), n=n, h=64, w=64, crop=CROP, mean=mean, std=std, rects=vp(rc), color=vp(col), sums=vp(sums), out=vp(out))
    order = ('frames', 'n', 'h', 'w', 'crop', 'mean', 'std', 'rects', 'color', 'sums', 'out')
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    for change, word in ((dict(frames=None), 'null argument'), (dict(rects=None), 'null rects_dev'), (dict(sums=None), 'without gray_sums_dev'),
                         (dict(color=off(col, 2)), 'color_dev'), (dict(sums=off(sums, 1)), 'gray_sums_dev'), (dict(rects=off(rc, 2)), 'rects_dev'),
                         (dict(rects=off(rc, 2), color=None, sums=None), 'rects_dev'), (dict(out=off(out, 8)), '16-byte aligned'),
                         (dict(out=off(out, 8), color=None, sums=None), '16-byte aligned'), (dict(n=0), 'bad shape'), (dict(w=0, color=None), 'bad shape'),
                         (dict(crop=257), 'crop 257'), (dict(n=65536, color=None), '65535')):
        assert L.pvr_op_preprocess_rects(*[dict(ok, **change)[x] for x in order], _lib.stream_ptr()) == PVR_ERR_INVALID, change
        assert word in _lib.last_error(), (change, _lib.last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not bool(sums.any())


@pytest.mark.parametrize('h,w', [(64, 64), (48, 80), (256, 256)], ids=lambda v: str(v))
def test_device_rectangles_equal_host_rectangles(h, w):
    n = 2000
    for first, scale in ((0, (0.2, 1.0)), (1000003, (0.2, 1.0)), ((1 << 33) + 5, (0.08, 0.5)), (0, (1.0, 1.0))):
        dev = torch.full((n + 1, 4), -7, dtype=torch.int32, device='cuda')
        _lib.check(_lib.lib().pvr_op_crop_rects((7 << 32) | 11, 5, first, n, h, w, scale[0], scale[1], vp(dev), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        want = E.crop_rects((7 << 32) | 11, 5, n, h, w, scale, first_frame=first)
        assert np.array_equal(got[:n], want), (first, scale, int((got[:n] != want).any(axis=1).sum()))
        assert (got[n] == -7).all()                             # n rows and nothing else
    # a long frame at the whole area: every row is the fallback, on the device too
    dev = torch.full((8, 4), -7, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().pvr_op_crop_rects(1, 0, 0, 8, 20, 100, 1.0, 1.0, vp(dev), _lib.stream_ptr()))
    assert (dev.cpu().numpy() == np.array([0, 36, 20, 27], np.int32)).all()
