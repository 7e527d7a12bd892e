"""The random_crop mode (pvr_op_crop_windows / pvr_host_crop_windows, pvr_trainer_forward_windows, pvr_op_preprocess_windows;
EmbeddingNet(..., train=True, random_crop=True, crop_seed=...); --embedding_random_crop) without a GPU: the new symbols, the window draw on the host
(range, determinism, slice invariance, coverage and mean at the trainer's range of 33 x 33 offsets), the rounding order of the kernel's bilinear sum
restated in numpy against the oracle, the keyword and flag refusals, and the refusals of the entry points that launch nothing."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pvr_op_crop_windows', 'pvr_host_crop_windows', 'pvr_trainer_forward_windows', 'pvr_op_preprocess_windows')
PVR_ERR_INVALID, PVR_ERR_STATE = 1, 4
MAX = 32                                                       # 256 - 224: the trainer's range for square frames


def test_the_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pvr_train.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGS, s
        assert re.search(r'\b%s\s*\(' % s, header), s


# ------------------------------------------------------------------------------------------------------------------
# the window draw
# ------------------------------------------------------------------------------------------------------------------
def test_windows_lie_in_range_and_are_a_function_of_their_arguments():
    w = E.crop_windows(5, 3, 4096, MAX, MAX)
    assert w.shape == (4096, 2) and w.dtype == np.int32
    assert w.min() >= 0 and w.max() <= MAX
    assert np.array_equal(w, E.crop_windows(5, 3, 4096, MAX, MAX))
    assert not np.array_equal(w, E.crop_windows(5, 4, 4096, MAX, MAX))          # another call
    assert not np.array_equal(w, E.crop_windows(6, 3, 4096, MAX, MAX))          # another seed
    assert not np.array_equal(w[:, 0], w[:, 1])                                  # top and left come from different words


def test_slice_invariance():
    """rows lo:hi of one draw equal a draw with first_frame = lo: a step cut into passes sees the windows of the whole step"""
    w = E.crop_windows(1, 9, 100, MAX, MAX)
    for lo, hi in ((0, 100), (7, 8), (33, 64), (99, 100)):
        assert np.array_equal(w[lo:hi], E.crop_windows(1, 9, hi - lo, MAX, MAX, first_frame=lo)), (lo, hi)
    out = np.full((3, 2), -1, np.int32)                         # the raw entry point writes n pairs and nothing else
    _lib.lib().pvr_host_crop_windows(1, 9, 7, 2, MAX, MAX, out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out[:2], w[7:9]) and (out[2] == -1).all()


def test_every_offset_occurs_and_the_mean_is_central():
    """n = 4096 at 33 x 33 offsets: a value is missed with probability below 66 (32/33)^4096 < 1e-52; the mean of the tops is 16 with a standard
    error of sqrt((33^2 - 1) / 12 / 4096) = 0.15"""
    w = E.crop_windows(1, 0, 4096, MAX, MAX)
    assert sorted(set(w[:, 0].tolist())) == list(range(MAX + 1))
    assert sorted(set(w[:, 1].tolist())) == list(range(MAX + 1))
    assert abs(float(w[:, 0].mean()) - 16.0) <= 1.0


def test_a_range_of_one_value_gives_zeros():
    assert not E.crop_windows(1, 0, 50, 0, 0).any()
    w = E.crop_windows(1, 0, 200, 0, 5)                         # max_top != max_left
    assert not w[:, 0].any() and w[:, 1].max() == 5 and w[:, 1].min() == 0
    assert E.crop_windows(1, 0, 0, MAX, MAX).shape == (0, 2)


def test_resized_size_is_torchvisions():
    assert E.resized_size(64, 64, 256) == (256, 256) and E.resized_size(256, 256, 256) == (256, 256)
    assert E.resized_size(96, 72, 256) == (341, 256) and E.resized_size(72, 96, 256) == (256, 341)
    assert E.resized_size(300, 260, 256) == (295, 256) and E.resized_size(256, 300, 256) == (256, 300)


# ------------------------------------------------------------------------------------------------------------------
# the rounding order of the kernel's bilinear sum
# ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fp32 fma of fp32 arrays: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _resize_as_the_kernel(fr, size=256):
    """preprocess_windows_f32_kernel's resize of whole (n, h, w, 3) uint8 frames in numpy float32: src = fma(scale, dst + 0.5, -0.5) clamped at 0, every
    two-tap sum w0 a + w1 b as fma(w0, a, round(w1 b)), along x and then along y, rint"""
    f32 = np.float32
    n, h, w, _ = fr.shape
    rh, rw = E.resized_size(h, w, size)

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


@pytest.mark.parametrize('h,w,n', [(96, 72, 2), (300, 260, 1), (64, 64, 1), (37, 53, 2)], ids=lambda v: str(v))
def test_the_kernels_rounding_order_gives_the_oracles_uint8_on_whole_frames(h, w, n):
    """why the kernel sums its taps as it does: in this order every value of the whole resized frame is the oracle's (ATen's host kernel), .5 ties
    included - smooth frames (the GPU test's) and noise; with every product and sum rounded by itself, preprocess_kernel's order, two values of the
    96 x 72 frames (float64 194.49999999999997 and 183.5) land one step away"""
    import torch
    from oracle import encoder_oracle as eo
    from pvr_habitat_amd import synth
    for fr in (synth.smooth_frames(11, n, h, w), np.random.default_rng(1).integers(0, 256, (n, h, w, 3), dtype=np.uint8)):
        want = eo.resize_u8(torch.from_numpy(fr).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
        got = _resize_as_the_kernel(fr)
        assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())


# ------------------------------------------------------------------------------------------------------------------
# keywords and flags
# ------------------------------------------------------------------------------------------------------------------
def test_keyword_refusals():
    """before anything needs a GPU"""
    with pytest.raises(ValueError, match='random_crop is a mode of the trainable encoder .train=True.: a frozen encoder embeds the centre crop'):
        E.EmbeddingNet('resnet18', pretrained=False, random_crop=True)
    with pytest.raises(ValueError, match='random_crop with prefix_cache.*ONE window per frame.*prefix_once.*compatible'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, train_from='layer3', prefix_cache=True, random_crop=True)
    with pytest.raises(ValueError, match='random_crop with prefix_cache.*ONE window per frame.*prefix_once'):
        E.check_random_crop(True, True)
    for what in ('build_prefix_cache', 'forward_cached'):
        with pytest.raises(ValueError, match='random_crop with %s.*ONE window per frame.*prefix_once' % what):
            E.check_random_crop(True, True, what)
    E.check_random_crop(True, False)
    E.check_random_crop(False, True)
    with pytest.raises(NotImplementedError, match='resnet18'):               # what the trainer refuses stays refused
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, random_crop=True)


def test_flag_refusals_and_help():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_random_crop is False
    f = make_parser().parse_args(['--train_embedding', '--embedding_random_crop', '--embedding_train_from', 'layer3', '--embedding_prefix_once'])
    assert f.embedding_random_crop is True and Fz.check_random_crop_flag(f) is True
    assert Fz.workspace_modes(f) == {'train_from': 'layer3', 'prefix_once': True}      # the mode adds nothing to the workspace
    text = ' '.join(make_parser().format_help().split())
    assert '--embedding_random_crop' in text and 'ONE window per frame' in text and '--embedding_prefix_once is the compatible mode' in text
    with pytest.raises(ValueError, match='--embedding_random_crop needs --train_embedding.*centre crop'):
        Fz.run(make_parser().parse_args(['--embedding_random_crop']))
    with pytest.raises(ValueError, match='--embedding_random_crop with --embedding_prefix_cache.*ONE window per frame.*--embedding_prefix_once'):
        Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--embedding_prefix_cache', '--embedding_random_crop']))
    assert Fz.check_random_crop_flag(argparse.Namespace()) is False


# ------------------------------------------------------------------------------------------------------------------
# library refusals that launch nothing
# ------------------------------------------------------------------------------------------------------------------
def test_crop_windows_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    for args, word in (((1, 0, 0, 4, MAX, MAX, None), 'null windows_dev'), ((1, 0, 0, 4, MAX, MAX, p(258)), '4-byte aligned'),
                       ((1, 0, 0, 0, MAX, MAX, p(256)), 'n = 0'), ((1, 0, -1, 4, MAX, MAX, p(256)), 'first_frame = -1'),
                       ((1, 0, 0, 4, -1, MAX, p(256)), 'max_top = -1'), ((1, 0, 0, 4, MAX, -2, p(256)), 'max_left = -2')):
        assert L.pvr_op_crop_windows(*args, None) == PVR_ERR_INVALID, args
        assert 'pvr_op_crop_windows' in _lib.last_error() and word in _lib.last_error(), (args, _lib.last_error())


def test_preprocess_windows_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    ok = dict(frames=p(256), n=1, h=64, w=64, resize=256, crop=224, mean=mean, std=std, windows=p(512), out=p(1024))
    order = ('frames', 'n', 'h', 'w', 'resize', 'crop', 'mean', 'std', 'windows', 'out')
    call = lambda **k: L.pvr_op_preprocess_windows(*[dict(ok, **k)[x] for x in order], None)
    for change, word in ((dict(frames=None), 'null argument'), (dict(windows=None), 'null argument'), (dict(out=None), 'null argument'),
                         (dict(mean=None), 'null argument'), (dict(n=0), 'bad shape'), (dict(h=0), 'bad shape'), (dict(n=65536), '65535'),
                         (dict(resize=200), 'smaller than crop 224'), (dict(h=64, w=32, resize=128), 'smaller than crop 224'),
                         (dict(windows=p(514)), '4-byte aligned'), (dict(out=p(1032)), '16-byte aligned')):
        assert call(**change) == PVR_ERR_INVALID, change
        assert 'preprocess windows' in _lib.last_error().replace('_', ' ') and word in _lib.last_error(), (change, _lib.last_error())


def test_forward_windows_refusals():
    L = _lib.lib()
    d = _lib.EncoderDesc(arch=10, dtype=_lib.PVR_F32, max_batch=4, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert L.pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    try:
        one = C.c_void_p(16)
        def call(params=one, bufs=one, frames=one, n=1, hw=(64, 64), windows=one, boundary=None, reuse=0, out=one):
            return L.pvr_trainer_forward_windows(h, params, bufs, frames, n, hw[0], hw[1], windows, boundary, reuse, out, 512, None)
        name = 'pvr_trainer_forward_windows'
        for kw, word in ((dict(params=None), 'null argument'), (dict(frames=None), 'null argument'), (dict(out=None), 'null argument'),
                         (dict(windows=C.c_void_p(18)), 'not 4-byte aligned'), (dict(n=0), 'max_batch = 4'), (dict(n=5), 'max_batch = 4'),
                         (dict(hw=(0, 64)), 'bad frame size'), (dict(hw=(64, -3)), 'bad frame size')):
            assert call(**kw) == PVR_ERR_INVALID, kw
            assert name in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
        assert call(boundary=one) == PVR_ERR_STATE and name in _lib.last_error() and 'no frozen prefix' in _lib.last_error()     # stage 0
        # without windows the entry point is the centre-crop one, refusals included
        assert call(windows=None, frames=None) == PVR_ERR_INVALID and 'pvr_trainer_forward: null argument' in _lib.last_error()
        assert call(windows=None, boundary=one) == PVR_ERR_STATE and 'pvr_trainer_forward_boundary' in _lib.last_error()
        assert L.pvr_trainer_set_train_from(h, 3) == 0
        assert call(boundary=C.c_void_p(20)) == PVR_ERR_INVALID and name in _lib.last_error() and 'not 16-byte aligned' in _lib.last_error()
        assert call(boundary=one, frames=None) == PVR_ERR_INVALID and name in _lib.last_error() and 'null argument' in _lib.last_error()
        assert call(windows=None, boundary=one, n=9, reuse=1) == PVR_ERR_INVALID and 'pvr_trainer_forward_boundary' in _lib.last_error()
        # nothing was launched and nothing is held
        assert L.pvr_trainer_backward(h, one, one, 512, one, None) == PVR_ERR_STATE and 'no forward' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)
