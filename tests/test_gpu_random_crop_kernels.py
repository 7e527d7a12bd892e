"""The kernels of the random_crop mode on the GPU: pvr_op_preprocess_windows (uint8 frames -> Resize -> a window per frame -> the normalised fp32
NHWC4 image, one launch) against oracle.encoder_oracle.resize_u8 sliced at the window, and pvr_op_crop_windows against pvr_host_crop_windows.

Frames as tests/test_gpu_encoder.py's preprocess test makes them (synth.smooth_frames, seed 11).  Per shape the resized uint8 frames are computed once.
Every frame is cropped at both extreme corners, the centre, an interior point of its own and the out-of-range pair (-5, 1000), which must behave as
its clamped value (0, max_left).

Exact: rint((out * std + mean) * 255) is the oracle's uint8 window everywhere and channel 3 is 0.  The kernel sums the four taps in the rounding order
of ATen's host kernel (tests/test_random_crop_cpu.py restates it), so .5 ties of the bilinear sum land where the oracle's do at every scale.
Values: |out - ((u8 / 255 - mean) / std in numpy float32)| <= 3 * 2^-24 / min(std): three fp32 roundings (the quotient, the difference, the
second quotient) of magnitudes <= 1, divided by std >= 0.224 - about 8e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import encoder_oracle as eo
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

RESIZE, CROP = 256, 224
MEAN, STD = np.array(E.IMAGENET_MEAN, np.float32), np.array(E.IMAGENET_STD, np.float32)
# (h, w) -> n: x4 upscale; non-square, non-integer scale, max_top != max_left; the no-resize branch; downscale
SHAPES = {(64, 64): 3, (96, 72): 2, (256, 256): 2, (300, 260): 1}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr())


def _case(h, w):
    if (h, w) not in _cache:
        n = SHAPES[(h, w)]
        fr = synth.smooth_frames(11, n, h, w)
        resized = eo.resize_u8(torch.from_numpy(fr).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous().numpy()       # (n, rh, rw, 3) uint8
        _cache[(h, w)] = (fr, torch.from_numpy(fr).cuda(), resized)
    return _cache[(h, w)]


def _run(frames_dev, h, w, windows):
    n = frames_dev.shape[0]
    win = torch.from_numpy(np.ascontiguousarray(windows, np.int32)).cuda()
    out = torch.full((n, CROP, CROP, 4), float('nan'), device='cuda')
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    _lib.check(_lib.lib().pvr_op_preprocess_windows(vp(frames_dev), n, h, w, RESIZE, CROP, mean, std, vp(win), vp(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _window_sets(n, max_top, max_left):
    """name -> ((n, 2) windows handed to the kernel, (n, 2) windows it must behave as)"""
    rng = np.random.default_rng(5)
    interior = np.stack([rng.integers(1, max(max_top, 2), n), rng.integers(1, max(max_left, 2), n)], axis=1)
    interior = np.minimum(interior, [max_top, max_left])
    same = lambda t, l: np.tile(np.array([[t, l]]), (n, 1))
    return {'top_left': (same(0, 0), same(0, 0)), 'bottom_right': (same(max_top, max_left), same(max_top, max_left)),
            'centre': (same(int(round(max_top / 2.0)), int(round(max_left / 2.0))),) * 2, 'interior': (interior, interior),
            'out_of_range': (same(-5, 1000), same(0, max_left))}


@pytest.mark.parametrize('h,w', list(SHAPES), ids=['%dx%d' % s for s in SHAPES])
def test_preprocess_windows_against_the_oracle(h, w):
    fr, dev, resized = _case(h, w)
    n, rh, rw = resized.shape[:3]
    assert (rh, rw) == E.resized_size(h, w, RESIZE)
    max_top, max_left = rh - CROP, rw - CROP
    assert (max_top, max_left) == {(64, 64): (32, 32), (96, 72): (117, 32), (256, 256): (32, 32), (300, 260): (71, 32)}[(h, w)]
    bound = 3 * 2.0 ** -24 / float(STD.min())
    inexact, outside = [], []
    for name, (given, acts_as) in _window_sets(n, max_top, max_left).items():
        out = _run(dev, h, w, given)
        want = np.stack([resized[i, t:t + CROP, l:l + CROP] for i, (t, l) in enumerate(acts_as)])
        assert want.shape == (n, CROP, CROP, 3)
        assert np.isfinite(out).all() and (out[..., 3] == 0).all(), name
        got_u8 = np.rint((out[..., :3].astype(np.float64) * STD + MEAN) * 255.0)
        wrong = got_u8 != want
        print('\n[preprocess windows %dx%d %s] windows %s: %d of %d values differ from the oracle\'s uint8 (largest |difference| %d)'
              % (h, w, name, given.tolist(), int(wrong.sum()), wrong.size, int(np.abs(got_u8 - want).max())))
        if wrong.any():
            inexact.append((name, int(wrong.sum()), np.argwhere(wrong)[:4].tolist()))
        ref = (want.astype(np.float32) / np.float32(255.0) - MEAN) / STD                  # numpy float32 throughout
        assert ref.dtype == np.float32
        err = float(np.abs(out[..., :3] - ref)[~wrong].max())                             # (a value of another uint8 is counted above, once)
        print('[preprocess windows %dx%d %s] largest |out - float32 reference| %.3e (bound %.3e)' % (h, w, name, err, bound))
        if not err <= bound:
            outside.append((name, err))
    assert not inexact, inexact                               # every window has been measured and printed
    assert not outside, (outside, bound)


@pytest.mark.parametrize('h,w', [(64, 64), (256, 256)], ids=['64x64', '256x256'])
def test_two_runs_give_equal_bits(h, w):
    fr, dev, resized = _case(h, w)
    n = dev.shape[0]
    win = E.crop_windows(3, 1, n, resized.shape[1] - CROP, resized.shape[2] - CROP)
    a, b = _run(dev, h, w, win), _run(dev, h, w, win)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('n', [1000, 3])
def test_device_windows_equal_host_windows(n):
    for max_top, max_left in ((32, 32), (85, 32), (0, 0)):
        dev = torch.full((n + 1, 2), -7, dtype=torch.int32, device='cuda')
        _lib.check(_lib.lib().pvr_op_crop_windows(11, 5, 7, n, max_top, max_left, vp(dev), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        assert np.array_equal(got[:n], E.crop_windows(11, 5, n, max_top, max_left, first_frame=7))
        assert (got[n] == -7).all()                           # n pairs and nothing else
