"""The color_jitter mode (pvr_op_color_params / pvr_host_color_params, pvr_op_preprocess_color, pvr_trainer_forward_augmented;
EmbeddingNet(..., train=True, color_jitter=(b, c, s), color_seed=...); --embedding_color_jitter B C S) without a GPU: the new symbols, the reference
arithmetic and its mutants (tests/color_jitter_refs.py), the draw on the host against a numpy Philox restatement (bits, slice invariance, ranges, means,
order frequencies, the crop windows untouched), the keyword and flag refusals, and the refusals of the entry points that launch nothing."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import color_jitter_refs as R
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pvr_op_color_params', 'pvr_host_color_params', 'pvr_op_preprocess_color', 'pvr_trainer_forward_augmented')
PVR_ERR_INVALID, PVR_ERR_STATE = 1, 4
BIG_SEED = (7 << 32) | 5                                         # both key words in use


def test_the_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pvr_train.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGS, s
        assert re.search(r'\b%s\s*\(' % s, header), s


# ------------------------------------------------------------------------------------------------------------------
# the reference arithmetic
# ------------------------------------------------------------------------------------------------------------------
def _window(seed=3, crop=48):
    smooth = synth.smooth_frames(seed, 1, crop, crop)[0]
    noise = np.random.default_rng(seed).integers(0, 256, (crop, crop, 3), dtype=np.uint8)
    return smooth, noise


def test_the_reference_is_the_literal_functions_and_the_identity_keeps_the_bits():
    for img in _window():
        for order in range(6):
            assert np.array_equal(R.jitter(img, 1.0, 1.0, 1.0, order), img)              # 1 * a + 0 * b = a
            got = R.jitter(img, 1.5, 0.25, 2.0, order)
            assert np.array_equal(got, R.jitter_literal(img, 1.5, 0.25, 2.0, order)) and got.dtype == np.uint8
        assert np.array_equal(R.jitter(img, 0.0, 1.0, 1.0, 0), np.zeros_like(img))       # brightness 0: black
        gray = R.rgb_to_grayscale(torch.from_numpy(img).permute(2, 0, 1))[0].numpy()
        assert np.array_equal(R.jitter(img, 1.0, 1.0, 0.0, 4), np.repeat(gray[:, :, None], 3, axis=2))     # saturation 0: gray in every channel
    assert len(set(R.PERMS)) == 6 and list(R.PERMS) == sorted(R.PERMS) and all(sorted(p) == ['b', 'c', 's'] for p in R.PERMS)


def test_the_gray_mean_is_one_division_of_an_exact_integer_sum():
    """what makes a parallel reduction bit-reproducible: torch.mean of the float32 gray plane equals float32(S) / float32(pixels) with S the integer
    sum, at the trainer's window size and at an odd one"""
    rng = np.random.default_rng(0)
    for hw in (224, 37):
        for k in range(6):
            g = rng.integers(0, 256 if k else 1, (1, hw, hw), dtype=np.uint8)
            if k == 5:
                g[:] = 255                                       # the largest sum: 255 * 224^2 < 2^24
            S = int(g.astype(np.int64).sum())
            assert S < 2 ** 24
            want = np.float32(S) / np.float32(hw * hw)
            got = torch.mean(torch.from_numpy(g).to(torch.float32), dim=(-3, -2, -1), keepdim=True).numpy().reshape(())
            assert got.dtype == np.float32 and got == want, (hw, k, float(got), float(want))


@pytest.mark.parametrize('mutant', ['fma', 'round', 'mean_first'])
def test_the_bit_exact_comparison_rejects_the_mutants(mutant):
    """each mutant differs from the reference on the windows the GPU tests use (smooth frames), so array_equal against the reference tells them apart"""
    img = synth.smooth_frames(11, 1, 256, 256)[0, 16:240, 16:240]
    rows = [(1.3, 0.7, 1.6, order) for order in range(6)]
    differs = [not np.array_equal(R.jitter(img, *r), R.jitter(img, *r, mutant=mutant)) for r in rows]
    if mutant == 'mean_first':                                   # the mean is the first op's own where contrast comes first
        assert differs == [True, True, False, False, True, True], differs
    else:
        assert all(differs), differs


# ------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------
def test_the_exact_fma_helper_rounds_once():
    """(1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 tie; +- 2^-60 decides it, and the float64 sum cannot hold that term: rounding the float64 sum
    to nearest and then to float32 gives 1 + 2^-11 (to even) both times"""
    f32 = np.float32
    a = np.full(3, 1 + 2.0 ** -12, f32)
    c = np.array([2.0 ** -60, -2.0 ** -60, 0.0], f32)
    want = np.array([1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11, 1 + 2.0 ** -11], f32)
    assert np.array_equal(R.fma32(a, a, c), want)
    naive = (a.astype(np.float64) * a.astype(np.float64) + c.astype(np.float64)).astype(f32)
    assert naive[0] != want[0]                                   # what the helper is for


@pytest.mark.parametrize('seed,call,first,n,strengths', [(1, 0, 0, 2000, (0.4, 0.4, 0.4)), (BIG_SEED, (3 << 32) | 9, 5, 1000, (0.2, 1.0, 2.5)),
                                                         (5, 7, (1 << 32) - 3, 8, (1e-3, 0.0, 0.999))])
def test_host_draw_equals_the_numpy_philox_restatement(seed, call, first, n, strengths):
    got = E.color_params(seed, call, n, strengths, first_frame=first)
    assert got.dtype == E.COLOR_DTYPE and got.shape == (n,) and got.itemsize == 16
    factors, order = R.color_params(seed, call, n, strengths, first_frame=first)
    for j, name in enumerate('bcs'):
        assert np.array_equal(got[name].view(np.uint32), factors[:, j].view(np.uint32)), name
    assert np.array_equal(got['order'], order)


def test_slice_invariance_and_dependence_on_seed_call_and_frame():
    s = (0.4, 0.3, 0.2)
    p = E.color_params(1, 9, 100, s)
    for lo, hi in ((0, 100), (7, 8), (33, 64), (99, 100)):
        assert np.array_equal(p[lo:hi], E.color_params(1, 9, hi - lo, s, first_frame=lo)), (lo, hi)
    assert np.array_equal(p, E.color_params(1, 9, 100, s))
    assert not np.array_equal(p, E.color_params(1, 10, 100, s)) and not np.array_equal(p, E.color_params(2, 9, 100, s))
    assert len({tuple(r) for r in p.tolist()}) == 100            # every frame its own row
    assert not np.array_equal(p['b'], p['c']) and not np.array_equal(p['c'], p['s'])       # the factors come from different words
    out = np.full((3, 4), -1, np.int32)                          # the raw entry point writes n rows and nothing else
    _lib.lib().pvr_host_color_params(1, 9, 7, 2, 0.4, 0.3, 0.2, out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out[:2].view(np.uint8), p[7:9].view(np.uint8).reshape(2, 16)) and (out[2] == -1).all()
    _lib.lib().pvr_host_color_params(1, 9, 7, 2, 0.4, 0.3, 0.2, None)                    # a null pointer: nothing written, no fault
    assert E.color_params(1, 0, 0, s).shape == (0,)


def test_the_crop_windows_keep_their_bits():
    """the colour stream has a key of its own: the windows of the same (seed, call) are what they were, and no window word shows up as a colour word"""
    for seed, call in ((9, 0), (BIG_SEED, 5)):
        before = E.crop_windows(seed, call, 500, 32, 32)
        E.color_params(seed, call, 500, 0.4)
        assert np.array_equal(E.crop_windows(seed, call, 500, 32, 32), before)
    # pinned: the first windows of (9, 0), the draw of tests/test_gpu_random_crop.py, as the commit before the colour stream drew them
    assert E.crop_windows(9, 0, 4, 32, 32).tolist() == [[27, 17], [14, 16], [7, 17], [31, 25]]
    # and the colour words are not the windows' words: the top 23 bits of word 0 of either stream, 2000 frames
    top = E.crop_windows(9, 0, 2000, (1 << 23) - 1, 0)[:, 0].astype(np.int64)
    u = E.color_params(9, 0, 2000, (1.0, 0, 0))['b'].astype(np.float64) / 2      # lo = 0, hi = 2: b = 2 u with u = (those 23 bits + 0.5) 2^-23
    assert (np.floor(u * 2 ** 23).astype(np.int64) != top).mean() > 0.99


def test_strength_zero_gives_exactly_one():
    p = E.color_params(3, 1, 1000, (0.0, 0.5, 0.0))
    assert (p['b'].view(np.uint32) == np.float32(1).view(np.uint32)).all() and (p['s'] == 1).all() and not (p['c'] == 1).all()
    q = E.color_params(3, 1, 1000, 0)                            # the mode off: all three
    assert (q['b'] == 1).all() and (q['c'] == 1).all() and (q['s'] == 1).all() and set(q['order'].tolist()) == set(range(6))


def test_ranges_means_and_order_frequencies_of_60000_frames():
    """a fixed seed (4, call 2), so these are conditions that either hold or do not, not a random test: every factor in [max(0, 1 - s), 1 + s]; the mean
    of a factor within 5 standard errors of the interval's centre, which is 1 for s <= 1 (a uniform on an interval of width d has standard deviation
    d / sqrt(12)); each of the six orders within 5 binomial standard deviations sqrt(n / 6 * 5 / 6) of n / 6"""
    n = 60000
    for strengths in ((0.4, 1.0, 2.5), (0.05, 0.8, 0.3)):
        p = E.color_params(4, 2, n, strengths)
        for name, s in zip('bcs', strengths):
            lo, hi = max(0.0, 1.0 - s), 1.0 + s
            f = p[name].astype(np.float64)
            assert np.float32(lo) <= p[name].min() and p[name].max() <= np.float32(hi), (name, s)
            se = (hi - lo) / np.sqrt(12.0) / np.sqrt(n)
            centre = 1.0 if s <= 1 else (lo + hi) / 2
            print('[colour draw] strength %g: mean %.6f, centre %g, standard error %.2e' % (s, f.mean(), centre, se))
            assert abs(f.mean() - centre) <= 5 * se, (name, s, f.mean())
        counts = np.bincount(p['order'], minlength=6)
        sd = np.sqrt(n * (1 / 6) * (5 / 6))
        print('[colour draw] order counts %s, expected %.0f, standard deviation %.1f' % (counts.tolist(), n / 6, sd))
        assert len(counts) == 6 and (np.abs(counts - n / 6) <= 5 * sd).all(), counts


# ------------------------------------------------------------------------------------------------------------------
# keywords and flags
# ------------------------------------------------------------------------------------------------------------------
def test_strengths_of_the_keyword():
    assert E.color_strengths(None) is None and E.color_strengths(0) is None and E.color_strengths((0, 0, 0)) is None and E.color_strengths(0.0) is None
    assert E.color_strengths(0.5) == (0.5, 0.5, 0.5) and E.color_strengths([0.25, 0, 2]) == (0.25, 0.0, 2.0)
    assert E.color_strengths(0.4) == (float(np.float32(0.4)),) * 3                        # the fp32 values the library receives
    for bad in (-0.1, (0.4, -1, 0), float('nan'), (0.1, float('inf'), 0.1)):
        with pytest.raises(ValueError, match='color_jitter=.*a strength is a finite number, 0 or above'):
            E.color_strengths(bad)
    for bad in ((0.1, 0.2), (0.1, 0.2, 0.3, 0.4), 'abc'):
        with pytest.raises(ValueError, match='color_jitter=.*one strength for all.*or the three of them .hue is not offered.'):
            E.color_strengths(bad)


def test_keyword_refusals():
    """before anything needs a GPU"""
    with pytest.raises(ValueError, match='color_jitter is a mode of the trainable encoder .train=True.: a frozen encoder embeds the un-jittered centre crop'):
        E.EmbeddingNet('resnet18', pretrained=False, color_jitter=0.4)
    with pytest.raises(ValueError, match='a strength is a finite number, 0 or above'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, color_jitter=(0.4, -0.4, 0))
    with pytest.raises(ValueError, match='a strength is a finite number, 0 or above'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, color_jitter=float('inf'))
    with pytest.raises(ValueError, match='color_jitter with prefix_cache.*ONE image per frame.*prefix_once.*compatible'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, train_from='layer3', prefix_cache=True, color_jitter=0.4)
    for what in ('prefix_cache', 'build_prefix_cache', 'forward_cached'):
        with pytest.raises(ValueError, match='color_jitter with %s.*ONE image per frame.*prefix_once' % what):
            E.check_color_jitter((0.4, 0.4, 0.4), True, what)
    E.check_color_jitter((0.4, 0.4, 0.4), False)
    E.check_color_jitter(None, True)
    with pytest.raises(NotImplementedError, match='resnet18'):               # what the trainer refuses stays refused
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, color_jitter=0.4)
    assert 'Hue is not offered' in E.HipTrainableResNet.__doc__


def test_flag_refusals_and_help():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_color_jitter is None
    assert Fz.check_color_jitter_flag(make_parser().parse_args([])) is None
    f = make_parser().parse_args(['--train_embedding', '--embedding_color_jitter', '0.4', '0', '0.25', '--embedding_train_from', 'layer3',
                                  '--embedding_prefix_once', '--embedding_random_crop'])
    assert f.embedding_color_jitter == [0.4, 0.0, 0.25]
    assert Fz.check_color_jitter_flag(f) == (float(np.float32(0.4)), 0.0, 0.25) and Fz.check_random_crop_flag(f) is True
    assert Fz.workspace_modes(f) == {'train_from': 'layer3', 'prefix_once': True}      # the mode adds nothing to the workspace
    assert Fz.check_color_jitter_flag(make_parser().parse_args(['--embedding_color_jitter', '0', '0', '0'])) is None     # zeros: off, nothing to refuse
    with pytest.raises(SystemExit):
        make_parser().parse_args(['--embedding_color_jitter', '0.4'])        # three floats
    text = ' '.join(make_parser().format_help().split())
    assert '--embedding_color_jitter B C S' in text and 'ONE image per frame' in text and 'hue is not offered' in text
    with pytest.raises(ValueError, match='--embedding_color_jitter needs --train_embedding.*un-jittered centre crop'):
        Fz.run(make_parser().parse_args(['--embedding_color_jitter', '0.4', '0.4', '0.4']))
    with pytest.raises(ValueError, match='--embedding_color_jitter with --embedding_prefix_cache.*ONE image per frame.*--embedding_prefix_once'):
        Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--embedding_prefix_cache', '--embedding_color_jitter',
                                         '0.4', '0.4', '0.4']))
    for bad in ('-0.5', 'nan', 'inf'):
        with pytest.raises(ValueError, match='--embedding_color_jitter: .*a strength is a finite number, 0 or above'):
            Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_color_jitter', '0.4', bad, '0.4']))
    assert Fz.check_color_jitter_flag(argparse.Namespace()) is None


def test_color_params_needs_no_gpu():
    """host arithmetic: usable where no device is visible (this test runs without one)"""
    p = E.color_params(1, 0, 3, (0.4, 0.4, 0.4))
    assert p.shape == (3,) and np.isfinite(p['b']).all() and p['order'].min() >= 0 and p['order'].max() <= 5
    assert E.color_params(1, 0, 3, 0.4).tolist() == p.tolist()   # a scalar means all three


# ------------------------------------------------------------------------------------------------------------------
# library refusals that launch nothing
# ------------------------------------------------------------------------------------------------------------------
def test_color_params_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    nan, inf = float('nan'), float('inf')
    for args, word in (((1, 0, 0, 4, 0.4, 0.4, 0.4, None), 'null color_dev'), ((1, 0, 0, 4, 0.4, 0.4, 0.4, p(258)), '4-byte aligned'),
                       ((1, 0, 0, 0, 0.4, 0.4, 0.4, p(256)), 'n = 0'), ((1, 0, -1, 4, 0.4, 0.4, 0.4, p(256)), 'first_frame = -1'),
                       ((1, 0, 0, 4, -0.1, 0.4, 0.4, p(256)), 'strengths -0.1'), ((1, 0, 0, 4, 0.4, nan, 0.4, p(256)), 'finite, 0 or above'),
                       ((1, 0, 0, 4, 0.4, 0.4, inf, p(256)), 'finite, 0 or above')):
        assert L.pvr_op_color_params(*args, None) == PVR_ERR_INVALID, args
        assert 'pvr_op_color_params' in _lib.last_error() and word in _lib.last_error(), (args, _lib.last_error())


def test_preprocess_color_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    ok = dict(frames=p(256), n=1, h=64, w=64, resize=256, crop=224, mean=mean, std=std, windows=p(512), color=p(768), sums=p(1536), out=p(1024))
    order = ('frames', 'n', 'h', 'w', 'resize', 'crop', 'mean', 'std', 'windows', 'color', 'sums', 'out')
    call = lambda **k: L.pvr_op_preprocess_color(*[dict(ok, **k)[x] for x in order], None)
    for change, word in ((dict(frames=None), 'null argument'), (dict(windows=None), 'null argument'), (dict(out=None), 'null argument'),
                         (dict(mean=None), 'null argument'), (dict(color=None), 'null color_dev'), (dict(sums=None), 'null gray_sums_dev'),
                         (dict(n=0), 'bad shape'), (dict(h=0), 'bad shape'), (dict(n=65536), '65535'),
                         (dict(resize=200), 'smaller than crop 224'), (dict(h=64, w=32, resize=128), 'smaller than crop 224'),
                         (dict(windows=p(514)), 'windows_dev 0x202 is not 4-byte aligned'), (dict(out=p(1032)), '16-byte aligned'),
                         (dict(color=p(770)), 'color_dev 0x302 is not 4-byte aligned'), (dict(sums=p(1537)), 'gray_sums_dev 0x601 is not 4-byte aligned'),
                         (dict(resize=300, crop=257, h=300, w=300), 'crop 257')):
        assert call(**change) == PVR_ERR_INVALID, change
        assert 'preprocess colour' in _lib.last_error().replace('_color', ' colour').replace('_', ' ') and word in _lib.last_error(), \
            (change, _lib.last_error())


def test_forward_augmented_refusals():
    L = _lib.lib()
    d = _lib.EncoderDesc(arch=10, dtype=_lib.PVR_F32, max_batch=4, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert L.pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    try:
        one = C.c_void_p(16)
        def call(params=one, bufs=one, frames=one, n=1, hw=(64, 64), windows=one, color=one, sums=one, boundary=None, reuse=0, out=one):
            return L.pvr_trainer_forward_augmented(h, params, bufs, frames, n, hw[0], hw[1], windows, color, sums, boundary, reuse, out, 512, None)
        name = 'pvr_trainer_forward_augmented'
        for kw, word in ((dict(params=None), 'null argument'), (dict(frames=None), 'null argument'), (dict(out=None), 'null argument'),
                         (dict(windows=None), 'color_dev without windows_dev'), (dict(windows=C.c_void_p(18)), 'windows_dev 0x12 is not 4-byte aligned'),
                         (dict(color=C.c_void_p(18)), 'color_dev 0x12 is not 4-byte aligned'), (dict(sums=None), 'gray_sums_dev'),
                         (dict(sums=C.c_void_p(18)), 'gray_sums_dev 0x12 is null or not 4-byte aligned'), (dict(n=0), 'max_batch = 4'),
                         (dict(n=5), 'max_batch = 4'), (dict(hw=(0, 64)), 'bad frame size'), (dict(hw=(64, -3)), 'bad frame size')):
            assert call(**kw) == PVR_ERR_INVALID, kw
            assert name in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
        assert call(boundary=one) == PVR_ERR_STATE and name in _lib.last_error() and 'no frozen prefix' in _lib.last_error()     # stage 0
        # without colour parameters the entry point is the windows one, and without windows too the centre-crop one, refusals included
        assert call(color=None, frames=None) == PVR_ERR_INVALID and 'pvr_trainer_forward_windows: null argument' in _lib.last_error()
        assert call(color=None, windows=C.c_void_p(18)) == PVR_ERR_INVALID and 'pvr_trainer_forward_windows: windows_dev' in _lib.last_error()
        assert call(color=None, windows=None, frames=None) == PVR_ERR_INVALID and 'pvr_trainer_forward: null argument' in _lib.last_error()
        assert call(color=None, windows=None, boundary=one) == PVR_ERR_STATE and 'pvr_trainer_forward_boundary' in _lib.last_error()
        assert L.pvr_trainer_set_train_from(h, 3) == 0
        assert call(boundary=C.c_void_p(20)) == PVR_ERR_INVALID and name in _lib.last_error() and 'not 16-byte aligned' in _lib.last_error()
        assert call(boundary=one, frames=None) == PVR_ERR_INVALID and name in _lib.last_error() and 'null argument' in _lib.last_error()
        # a reuse pass reads neither array: the boundary entry point's own refusal
        assert call(boundary=one, n=9, reuse=1, color=C.c_void_p(18), windows=None) == PVR_ERR_INVALID and 'pvr_trainer_forward_boundary' in _lib.last_error()
        # nothing was launched and nothing is held
        assert L.pvr_trainer_backward(h, one, one, 512, one, None) == PVR_ERR_STATE and 'no forward' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)
