"""The kernels of the color_jitter mode on the GPU: pvr_op_color_params against pvr_host_color_params, and pvr_op_preprocess_color (uint8 frames ->
Resize -> a window per frame -> brightness, contrast, saturation per frame -> the normalised fp32 NHWC4 image; two launches) against the reference
of tests/color_jitter_refs.py: torchvision's functions restated literally in torch, on the resize in the kernel's tap order.

Everything is compared with array_equal on the fp32 image: the jitter yields uint8 values, and (v / 255 - mean) / std is three correctly rounded
float32 operations on either side.  Seven frames per shape (smooth frames, the last two with noise in them), hand-written parameters: all six orders,
factors 0, 1 and 2, a contrast-only and a saturation-only frame, windows at both extreme corners, at the centre, inside, and one out-of-range pair that
must behave as its clamped value."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_jitter_refs as R
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

PVR_ERR_INVALID = 1
# (h, w, resize, crop): no resize; the two exact power-of-two resizes; non-square and no power of two; a small shape whose crop is no multiple of 64 or 4
SHAPES = [(256, 256, 256, 224), (64, 64, 256, 224), (128, 128, 256, 224), (96, 80, 256, 224), (20, 27, 40, 37)]
# (brightness, contrast, saturation, order)
PARAMS = [(2.0, 1.0, 1.0, 0),        # b c s: brightness alone, factor 2 - values clamp at 255
          (1.0, 1.7, 1.0, 1),        # b s c: contrast alone
          (1.0, 1.0, 0.3, 2),        # c b s: saturation alone
          (0.6, 1.4, 1.8, 3),        # c s b
          (1.3, 0.5, 0.0, 4),        # s b c: saturation 0 - gray first
          (1.2, 2.0, 2.0, 5),        # s c b
          (0.9, 0.0, 1.5, 2)]        # contrast 0: every value becomes the truncated mean
N = len(PARAMS)
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr())


def _case(shape):
    """(frames on the device, resized uint8 frames, (given windows, the windows they act as)): once per shape"""
    if shape not in _cache:
        h, w, resize, crop = shape
        fr = synth.smooth_frames(11, N, h, w)
        noise = np.random.default_rng(2).integers(0, 256, fr.shape, dtype=np.uint8)
        fr[5] = (fr[5] // 2 + noise[5] // 2).astype(np.uint8)
        fr[6] = noise[6]
        resized = R.resize_as_the_kernel(fr, resize)
        rh, rw = resized.shape[1:3]
        assert (rh, rw) == E.resized_size(h, w, resize)
        mt, ml = rh - crop, rw - crop
        assert mt >= 3 and ml >= 3
        given = np.array([[0, 0], [mt, ml], [-5, 1000], [mt, 0], [int(round(mt / 2.0)), int(round(ml / 2.0))], [1, ml - 2], [mt - 1, 2]], np.int32)
        acts_as = np.clip(given, 0, [mt, ml])
        assert acts_as[2].tolist() == [0, ml]
        _cache[shape] = (torch.from_numpy(fr).cuda(), resized, (given, acts_as))
    return _cache[shape]


def _run(dev, shape, windows, packed, op='color', out=None):
    h, w, resize, crop = shape
    n = dev.shape[0]
    win = torch.from_numpy(np.ascontiguousarray(windows, np.int32)).cuda()
    out = torch.full((n, crop, crop, 4), float('nan'), device='cuda') if out is None else out
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    if op == 'windows':
        _lib.check(_lib.lib().pvr_op_preprocess_windows(vp(dev), n, h, w, resize, crop, mean, std, vp(win), vp(out), _lib.stream_ptr()))
    else:
        col = torch.from_numpy(packed).cuda()
        sums = torch.full((n + 1,), 123456789, dtype=torch.int32, device='cuda')             # stale scratch: the entry point zeroes what it uses
        _lib.check(_lib.lib().pvr_op_preprocess_color(vp(dev), n, h, w, resize, crop, mean, std, vp(win), vp(col), vp(sums), vp(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert int(sums[n]) == 123456789                       # n sums and nothing else
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d_resize%d_crop%d' % s for s in SHAPES])
def test_preprocess_color_against_the_reference(shape):
    dev, resized, (given, acts_as) = _case(shape)
    crop = shape[3]
    assert {p[3] for p in PARAMS} == set(range(6)) and {0.0, 1.0, 2.0} <= {f for p in PARAMS for f in p[:3]}
    want_u8 = R.jittered_windows(resized, acts_as, PARAMS, crop)
    plain = R.windows_of(resized, acts_as, crop)
    # the cases do what they are there for: brightness 2 clamps at 255, and the contrast-only and saturation-only frames change their window
    assert ((plain[0].astype(np.int32) * 2 > 255) & (want_u8[0] == 255)).any()
    assert not np.array_equal(want_u8[1], plain[1]) and not np.array_equal(want_u8[2], plain[2])
    assert len(np.unique(want_u8[6][..., 0])) <= 3              # contrast 0 first: one value per channel, then brightness and saturation of a flat image
    got = _run(dev, shape, given, R.pack_params(PARAMS))
    want = R.normalize_nhwc4(want_u8)
    assert np.isfinite(got).all() and (got[..., 3] == 0).all()
    for i in range(N):
        bad = got[i] != want[i]
        print('[preprocess colour %s] frame %d, window %s, parameters %s: %d of %d values differ' % (shape, i, given[i].tolist(), PARAMS[i], int(bad.sum()),
                                                                                                   bad.size))
    assert np.array_equal(got, want)
    if shape == SHAPES[0]:                                      # the comparison is sharp enough to tell the mutants from the kernel
        for mutant in ('fma', 'round', 'mean_first'):
            assert not np.array_equal(R.normalize_nhwc4(R.jittered_windows(resized, acts_as, PARAMS, crop, mutant=mutant)), got), mutant


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[3], SHAPES[4]], ids=['256x256', '96x80', '20x27'])
def test_identity_factors_give_the_bits_of_preprocess_windows_and_two_runs_agree(shape):
    dev, resized, (given, _) = _case(shape)
    ones = R.pack_params([(1.0, 1.0, 1.0, order) for order in (0, 1, 2, 3, 4, 5, 17)])
    a = _run(dev, shape, given, ones)
    assert np.array_equal(a.view(np.uint32), _run(dev, shape, given, None, op='windows').view(np.uint32))
    jit = R.pack_params(PARAMS)
    b, c = _run(dev, shape, given, jit), _run(dev, shape, given, jit)
    assert np.array_equal(b.view(np.uint32), c.view(np.uint32)) and not np.array_equal(a, b)


def test_hardened_parameters_give_the_bits_of_their_clamped_values():
    shape = SHAPES[1]
    dev, resized, (given, _) = _case(shape)
    nan, inf = float('nan'), float('inf')
    wild = [(nan, -1.0, 9.0, 17), (9.0, nan, -0.0, -1), (-inf, 1.5, nan, 6), (inf, inf, inf, 5), (1.5, -3.0, 4.5, 2 ** 31 - 1), (nan, nan, nan, -2 ** 31),
            (0.5, 4.0, 0.0, 3)]
    tame = [(1.0, 0.0, 4.0, 0), (4.0, 1.0, 0.0, 0), (0.0, 1.5, 1.0, 0), (4.0, 4.0, 4.0, 5), (1.5, 0.0, 4.0, 0), (1.0, 1.0, 1.0, 0), (0.5, 4.0, 0.0, 3)]
    assert [R.harden(*p) for p in wild] == tame
    a, b = _run(dev, shape, given, R.pack_params(wild)), _run(dev, shape, given, R.pack_params(tame))
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_leave_out_untouched():
    L = _lib.lib()
    shape = SHAPES[4]
    h, w, resize, crop = shape
    dev, resized, (given, _) = _case(shape)
    win, col = torch.from_numpy(given).cuda(), torch.from_numpy(R.pack_params(PARAMS)).cuda()
    sums = torch.zeros((N + 1,), dtype=torch.int32, device='cuda')
    out = torch.full((N, crop, crop, 4), float('nan'), device='cuda')
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    ok = dict(frames=vp(dev), n=N, h=h, w=w, resize=resize, crop=crop, mean=mean, std=std, windows=vp(win), color=vp(col), sums=vp(sums), out=vp(out))
    order = ('frames', 'n', 'h', 'w', 'resize', 'crop', 'mean', 'std', 'windows', 'color', 'sums', 'out')
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)
    for change, word in ((dict(color=None), 'null color_dev'), (dict(sums=None), 'null gray_sums_dev'), (dict(color=off(col, 2)), 'color_dev'),
                         (dict(sums=off(sums, 1)), 'gray_sums_dev'), (dict(windows=None), 'null argument'), (dict(windows=off(win, 2)), 'windows_dev'),
                         (dict(out=off(out, 8)), '16-byte aligned'), (dict(crop=64), 'smaller than crop 64'), (dict(n=0), 'bad shape')):
        assert L.pvr_op_preprocess_color(*[dict(ok, **change)[x] for x in order], _lib.stream_ptr()) == PVR_ERR_INVALID, change
        assert word in _lib.last_error(), (change, _lib.last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and not bool(sums.any())


@pytest.mark.parametrize('n,first', [(1, 0), (257, 0), (257, 1000003)])
def test_device_parameters_equal_host_parameters(n, first):
    for strengths in ((0.4, 0.4, 0.4), (0.0, 1.0, 2.5)):
        dev = torch.full((n + 1, 4), -7, dtype=torch.int32, device='cuda')
        _lib.check(_lib.lib().pvr_op_color_params((7 << 32) | 11, 5, first, n, *strengths, vp(dev), _lib.stream_ptr()))
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        want = E.color_params((7 << 32) | 11, 5, n, strengths, first_frame=first)
        assert np.array_equal(got[:n].view(np.uint8).reshape(n, 16), want.view(np.uint8).reshape(n, 16))
        assert (got[n] == -7).all()                           # n rows and nothing else
