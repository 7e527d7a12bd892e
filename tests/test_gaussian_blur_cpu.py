"""The gaussian_blur and random_grayscale modes (pvr_op_blur_params / pvr_host_blur_params, pvr_op_preprocess_staged, pvr_op_blur_normalize,
pvr_trainer_forward_staged; EmbeddingNet(..., train=True, gaussian_blur=(p, lo, hi), random_grayscale=p, blur_seed=...); --embedding_gaussian_blur P LO
HI, --embedding_random_grayscale P) without a GPU: the new symbols, the references and the blur criterion with its mutants
(tests/gaussian_blur_refs.py), the draw on the host (bits against a numpy Philox restatement, the row-slice rule, p = 0 and p = 1, the share of blurred
frames, the sigma range, the other draws untouched), the keyword and flag refusals, the wording of the documents, and the refusals of the entry points
that launch nothing."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

import color_jitter_refs as CR
import gaussian_blur_refs as R
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('pvr_op_blur_params', 'pvr_host_blur_params', 'pvr_op_preprocess_staged', 'pvr_op_blur_normalize', 'pvr_trainer_forward_staged')
PVR_ERR_INVALID = 1
BIG_SEED = (7 << 32) | 5                                         # both key words in use
MOCO = (0.5, 0.1, 2.0)
SIZES, SIGMAS = (12, 24, 40), (0.5, 1.0, 2.0)
_cache = {}


def test_the_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pvr_train.h')).read(), flags=re.S)
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGS, s
        assert re.search(r'\b%s\s*\(' % s, header), s
    for name in ('blur_params', 'blur_spec', 'gray_prob', 'check_gaussian_blur', 'BLUR_DTYPE'):
        assert hasattr(E, name), name


# ------------------------------------------------------------------------------------------------------------------
# the criterion, the emulation and the mutants
# ------------------------------------------------------------------------------------------------------------------
def _exact(size, family, sigma, gray=0):
    key = (size, family, sigma, gray)
    if key not in _cache:
        _cache[key] = R.exact_augmented(R.families(size)[family], sigma, gray)
    return _cache[key]


def test_delta_is_the_derived_bound():
    assert abs(R.DELTA - 255 * 2.0 ** -24 * (46 + 2 * (66 / np.e + 15))) < 1e-12 and 1.8e-3 < R.DELTA < 2e-3
    assert R.DELTA < R.DELTA_2D < 1e-2


@pytest.mark.parametrize('size', SIZES + (224,))
def test_the_emulation_passes_the_criterion(size):
    """every family at every sigma, with and without grayscale first; the emulation's own distance from the exact value is far below DELTA"""
    fams = R.families(size)
    for name in (fams if size < 224 else ['random']):
        for sigma in SIGMAS:
            for gray in ((0, 1) if name == 'random' and size < 224 else (0,)):
                got = R.augment(fams[name], sigma, gray)
                v = R.blur_verdict(got, _exact(size, name, sigma, gray))
                print('[emulation] %3d %-11s sigma %.1f gray %d: max step %d, undecided %.4f, wrong %d' % (size, name, sigma, gray, v['max_step'],
                                                                                                       v['undecided'], v['wrong']))
                assert v['ok'], (size, name, sigma, gray, v)
    assert np.array_equal(R.augment(fams['constant255'], 2.0, 0), fams['constant255'])             # 255 stays exactly 255


def test_a_tiny_sigma_is_the_identity_and_no_value_is_near_a_tie():
    img = R.families(24)['random']
    for sigma in (0.1, 1e-30):
        assert np.array_equal(R.augment(img, sigma, 0), img)
    ex = R.exact(img, 0.1)
    assert np.abs(ex - img).max() < 1e-9 and R.blur_verdict(img, ex)['undecided'] == 0.0
    w = R.kernel_weights(1e-30)
    assert w[R.R] == 1.0 and w.sum() == 1.0 and np.isfinite(w).all()


def test_near_tie_shares_of_random_images_and_the_distance_of_the_emulation():
    """what the criterion leaves undecided: at most 0.7 % within 2e-3 and 1.6 % within 4e-3 of a tie; and the fp32 sums of the emulation, before
    their rounding, lie within 2e-4 of the exact values - a tenth of DELTA, which bounds the worst case"""
    for size in SIZES + (224,):
        img = R.families(size)['random']
        for sigma in SIGMAS:
            ex = _exact(size, 'random', sigma)
            for delta, most in ((2e-3, 0.007), (4e-3, 0.016)):
                share = float((np.abs(ex - np.floor(ex) - 0.5) <= delta).mean())
                assert share <= most, (size, sigma, delta, share)
            dev = float(np.abs(R.emulate_values(img, sigma).astype(np.float64) - ex).max())
            print('[emulation] %3d sigma %.1f: largest distance from the exact value %.2e' % (size, sigma, dev))
            assert dev < 2e-4 < R.DELTA, (size, sigma, dev)


def test_the_literal_restatement_agrees_with_the_exact_value():
    """torchvision's own arithmetic (one fp32 sum of 529 products) under the same criterion with the bound for that sum"""
    for size in (12, 40):
        img = R.families(size)['random']
        for sigma in (0.5, 2.0):
            v = R.blur_verdict(R.literal(img, sigma, 0), _exact(size, 'random', sigma), delta=R.DELTA_2D)
            assert v['max_step'] <= 1 and v['wrong'] == 0, (size, sigma, v)
    assert np.array_equal(R.literal(img, 0, 1), R.gray3(img))                                     # the grayscale: bit for bit
    assert np.array_equal(R.literal(img, 0, 0), img)


MUTANTS = {'replicate_padding': dict(pad='replicate'), 'zero_padding': dict(pad='zero'), 'taps_shifted': dict(shift=1), 'sigma_as_variance': dict(variance=True),
           'rounded_between_the_passes': dict(round_between=True), 'truncated': dict(final='trunc'), 'gray_after_blur': dict(gray_after=True)}


@pytest.mark.parametrize('mutant', list(MUTANTS))
def test_the_criterion_rejects_the_mutants(mutant):
    gray = 1 if mutant == 'gray_after_blur' else 0
    failed = []
    for size in (12, 24):
        for name, img in R.families(size).items():
            for sigma in (0.5, 2.0):
                v = R.blur_verdict(R.augment(img, sigma, gray, **MUTANTS[mutant]), _exact(size, name, sigma, gray))
                if not v['ok']:
                    failed.append((size, name, sigma))
    print('[mutant %s] fails on %s' % (mutant, failed))
    assert failed, mutant


def test_hardening_of_the_two_words():
    nan, inf = float('nan'), float('inf')
    assert [R.harden(s, g) for s, g in ((nan, 0), (-1.0, 2), (0.0, -5), (inf, 1), (1e30, 0), (-inf, 0), (16.5, 1), (0.3, 0))] == \
        [(0.0, 0), (0.0, 1), (0.0, 1), (16.0, 1), (16.0, 0), (0.0, 0), (16.0, 1), (float(np.float32(0.3)), 0)]
    img = R.families(24)['random']
    assert np.array_equal(R.recover_u8(R.normalize_nhwc4(img[None]))[0], img)
    with pytest.raises(AssertionError):
        R.recover_u8(R.normalize_nhwc4(img[None]) + np.float32(1e-3) * np.array([1, 1, 1, 0], np.float32))


# ------------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------------
def _numpy_draw(seed, call, n, p_blur, lo, hi, p_gray, first=0):
    f32 = np.float32
    frame = np.arange(first, first + n, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    counter = np.stack([frame & m32, frame >> np.uint64(32), np.full(n, call & 0xFFFFFFFF, np.uint64), np.full(n, call >> 32, np.uint64)],
                       axis=1).astype(np.uint32)
    bits = CR.philox4x32_10(counter, seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ 0x424C5552)
    u = ((bits >> np.uint32(9)).astype(f32) + f32(0.5)) * f32(1.0 / 8388608.0)
    sigma = CR.fma32(np.full(n, f32(hi) - f32(lo), f32), u[:, 1], np.full(n, f32(lo), f32))
    return np.where(u[:, 0] < f32(p_blur), sigma, f32(0)).astype(f32), (u[:, 2] < f32(p_gray)).astype(np.int32)


@pytest.mark.parametrize('seed,call,first,n', [(1, 0, 0, 300), (BIG_SEED, (3 << 32) | 9, (1 << 32) + 5, 300)])
def test_host_draw_equals_the_numpy_philox_restatement(seed, call, first, n):
    got = E.blur_params(seed, call, n, MOCO, 0.2, first_frame=first)
    sigma, gray = _numpy_draw(seed, call, n, 0.5, 0.1, 2.0, 0.2, first)
    assert got.dtype == E.BLUR_DTYPE and got.itemsize == 8
    assert np.array_equal(got['sigma'].view(np.uint32), sigma.view(np.uint32)) and np.array_equal(got['gray'], gray)


def test_row_slices_p0_p1_and_dependence_on_seed_call_and_frame():
    whole = E.blur_params(BIG_SEED, 4, 500, MOCO, 0.2)
    assert np.array_equal(E.blur_params(BIG_SEED, 4, 100, MOCO, 0.2, first_frame=250), whole[250:350])
    for other in (E.blur_params(BIG_SEED + 1, 4, 500, MOCO, 0.2), E.blur_params(BIG_SEED, 5, 500, MOCO, 0.2),
                  E.blur_params(BIG_SEED ^ (1 << 40), 4, 500, MOCO, 0.2)):
        assert not np.array_equal(other, whole)
    always = E.blur_params(BIG_SEED, 4, 5000, (1.0, 0.1, 2.0), 1.0)
    assert (always['sigma'] > 0).all() and (always['gray'] == 1).all()
    never = E.blur_params(BIG_SEED, 4, 5000, (0.0, 0.1, 2.0), 0.0)
    assert (never['sigma'] == 0).all() and (never['gray'] == 0).all()
    assert (E.blur_params(BIG_SEED, 4, 5000, None, None).view(np.uint8) == 0).all()
    # the sigma of a frame does not depend on p: the frames blurred at p = 0.5 have the sigma they have at p = 1
    half = E.blur_params(BIG_SEED, 4, 5000, MOCO, 1.0)
    on = half['sigma'] > 0
    assert np.array_equal(half['sigma'][on], always['sigma'][on]) and 0.4 < on.mean() < 0.6
    fixed = E.blur_params(BIG_SEED, 4, 100, (1.0, 0.7, 0.7), None)
    assert (fixed['sigma'] == np.float32(0.7)).all()


def test_shares_and_the_sigma_range_of_100000_frames():
    n = 100000
    for p_blur, p_gray in ((0.5, 0.2), (0.1, 0.9)):
        got = E.blur_params(3, 11, n, (p_blur, 0.1, 2.0), p_gray)
        on = got['sigma'] > 0
        for share, p in ((on.mean(), p_blur), (got['gray'].mean(), p_gray)):
            assert abs(share - p) <= 4 * np.sqrt(p * (1 - p) / n), (share, p)
        s = got['sigma'][on]
        assert s.min() >= np.float32(0.1) and s.max() <= np.float32(2.0) and abs(s.mean() - 1.05) < 0.02
        assert set(np.unique(got['gray'])) == {0, 1}
        # blur and grayscale are decided by different words
        both = (on & (got['gray'] == 1)).mean()
        assert abs(both - p_blur * p_gray) < 0.01


def test_the_other_draws_keep_their_bits():
    """windows, rectangles and colour parameters of the same (seed, call) are what they were, and the blur stream is none of them"""
    w = E.crop_windows(BIG_SEED, 4, 64, 32, 32)
    c = E.color_params(BIG_SEED, 4, 64, (0.4, 0.4, 0.4))
    r = E.crop_rects(BIG_SEED, 4, 64, 64, 64, (0.2, 1.0))
    factors, order = CR.color_params(BIG_SEED, 4, 64, (0.4, 0.4, 0.4))
    assert np.array_equal(np.stack([c['b'], c['c'], c['s']], axis=1), factors) and np.array_equal(c['order'], order)
    b = E.blur_params(BIG_SEED, 4, 64, (1.0, 0.6, 1.4), 0.5)
    assert not np.array_equal(b['sigma'], c['b'].astype(np.float32)) and w.shape == (64, 2) and r.shape == (64, 4)


# ------------------------------------------------------------------------------------------------------------------
# keywords, flags, documents
# ------------------------------------------------------------------------------------------------------------------
def test_the_keywords():
    f = lambda x: float(np.float32(x))
    assert E.blur_spec(None) is None and E.blur_spec(False) is None and E.blur_spec((0, 0.1, 2.0)) is None
    assert E.blur_spec(MOCO) == (0.5, f(0.1), 2.0) and E.blur_spec([1, 1, 1]) == (1.0, 1.0, 1.0)
    assert E.gray_prob(None) is None and E.gray_prob(0) is None and E.gray_prob(0.2) == f(0.2) and E.gray_prob(1) == 1.0
    for bad in (0.5, (0.5, 0.1), 'abc', (0.5, 0.1, 2.0, 3.0)):
        with pytest.raises(ValueError, match='gaussian_blur=.*three numbers .p, lo, hi.'):
            E.blur_spec(bad)
    for bad in ((-0.1, 0.1, 2.0), (1.5, 0.1, 2.0), (float('nan'), 0.1, 2.0)):
        with pytest.raises(ValueError, match='gaussian_blur=.*probability.*finite number in .0, 1.'):
            E.blur_spec(bad)
    for bad in ((0.5, 0.0, 2.0), (0.5, -1.0, 2.0), (0.5, 2.0, 0.1), (0.5, 0.1, float('inf')), (0.5, float('nan'), 2.0), (0.5, 1e-60, 2.0)):
        with pytest.raises(ValueError, match='gaussian_blur=.*sigma range.*finite with 0 < lo <= hi'):
            E.blur_spec(bad)
    for bad in (-0.1, 1.01, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='random_grayscale=.*finite number in .0, 1.'):
            E.gray_prob(bad)
    with pytest.raises(ValueError, match='random_grayscale=.*one number'):
        E.gray_prob('abc')


def test_keyword_refusals():
    """before anything needs a GPU"""
    with pytest.raises(ValueError, match='gaussian_blur is a mode of the trainable encoder .train=True.: a frozen encoder embeds the plain centre crop'):
        E.EmbeddingNet('resnet18', pretrained=False, gaussian_blur=MOCO)
    with pytest.raises(ValueError, match='random_grayscale is a mode of the trainable encoder .train=True.'):
        E.EmbeddingNet('resnet18', pretrained=False, random_grayscale=0.2)
    with pytest.raises(ValueError, match='sigma range'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, gaussian_blur=(0.5, 2.0, 0.1))
    with pytest.raises(ValueError, match='finite number in .0, 1.'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, random_grayscale=1.5)
    for kw, name in ((dict(gaussian_blur=MOCO), 'gaussian_blur'), (dict(random_grayscale=0.2), 'random_grayscale')):
        with pytest.raises(ValueError, match='%s with prefix_cache.*ONE image per frame.*prefix_once.*compatible' % name):
            E.EmbeddingNet('resnet18', pretrained=False, train=True, train_from='layer3', prefix_cache=True, **kw)
    for what in ('prefix_cache', 'build_prefix_cache', 'forward_cached'):
        with pytest.raises(ValueError, match='gaussian_blur with %s.*ONE image per frame.*prefix_once' % what):
            E.check_gaussian_blur(MOCO, None, True, what)
        with pytest.raises(ValueError, match='random_grayscale with %s.*ONE image per frame.*prefix_once' % what):
            E.check_gaussian_blur(None, 0.2, True, what)
    E.check_gaussian_blur(MOCO, 0.2, False)
    E.check_gaussian_blur(None, None, True)
    with pytest.raises(NotImplementedError, match='resnet18'):               # what the trainer refuses stays refused
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, gaussian_blur=MOCO, random_grayscale=0.2)
    doc = E.HipTrainableResNet.__doc__
    assert 'gaussian_blur' in doc and 'random_grayscale' in doc and 'kernel size is fixed at 23' in doc and 'Hue is not offered' in doc


def test_flag_refusals_and_help():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    none = make_parser().parse_args([])
    assert none.embedding_gaussian_blur is None and none.embedding_random_grayscale is None and Fz.check_gaussian_blur_flags(none) == (None, None)
    f = make_parser().parse_args(['--train_embedding', '--embedding_gaussian_blur', '0.5', '0.1', '2.0', '--embedding_random_grayscale', '0.2',
                                  '--embedding_train_from', 'layer3', '--embedding_prefix_once', '--embedding_random_resized_crop', '0.2', '1',
                                  '--embedding_color_jitter', '0.4', '0.4', '0.4'])
    assert f.embedding_gaussian_blur == [0.5, 0.1, 2.0] and f.embedding_random_grayscale == 0.2
    assert Fz.check_gaussian_blur_flags(f) == ((0.5, float(np.float32(0.1)), 2.0), float(np.float32(0.2)))
    assert Fz.workspace_modes(f) == {'train_from': 'layer3', 'prefix_once': True}      # the modes add nothing to the trainer's workspace
    zero = make_parser().parse_args(['--embedding_gaussian_blur', '0', '0.1', '2', '--embedding_random_grayscale', '0'])
    assert Fz.check_gaussian_blur_flags(zero) == (None, None)                           # probability 0: off, nothing to refuse
    with pytest.raises(SystemExit):
        make_parser().parse_args(['--embedding_gaussian_blur', '0.5'])       # three floats
    text = ' '.join(make_parser().format_help().split())
    assert '--embedding_gaussian_blur P LO HI' in text and '--embedding_random_grayscale P' in text and 'kernel size is fixed at 23' in text
    assert 'hue is not offered' in text
    for flag in (['--embedding_gaussian_blur', '0.5', '0.1', '2.0'], ['--embedding_random_grayscale', '0.2']):
        with pytest.raises(ValueError, match='%s needs --train_embedding.*plain centre crop' % flag[0]):
            Fz.run(make_parser().parse_args(flag))
        with pytest.raises(ValueError, match='%s with --embedding_prefix_cache.*ONE image per frame.*--embedding_prefix_once' % flag[0]):
            Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--embedding_prefix_cache'] + flag))
    for bad in (['1.5', '0.1', '2'], ['0.5', '0', '2'], ['0.5', '2', '0.1'], ['0.5', '0.1', 'inf'], ['nan', '0.1', '2']):
        with pytest.raises(ValueError, match='--embedding_gaussian_blur: .*(probability|sigma range)'):
            Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_gaussian_blur'] + bad))
    for bad in ('-0.5', 'nan', '2'):
        with pytest.raises(ValueError, match='--embedding_random_grayscale: .*finite number in .0, 1.'):
            Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_random_grayscale', bad]))
    assert Fz.check_gaussian_blur_flags(argparse.Namespace()) == (None, None)


def test_the_documents():
    readme = ' '.join(open(os.path.join(ROOT, 'README.md')).read().split())
    design = ' '.join(open(os.path.join(ROOT, 'DESIGN.md')).read().split())
    for text in (readme, design):
        assert '--embedding_gaussian_blur' in text and '--embedding_random_grayscale' in text and 'blur normalize' in text and 'stage image' in text
    assert 'gaussian_blur_step_times' in readme and 'grayscale, blur' not in design
    assert re.search(r'[Hh]ue is not offered', readme) and re.search(r'[Hh]ue', design)
    assert '60096' in design                                    # the LDS bytes of the blur kernel are stated


def test_blur_params_needs_no_gpu():
    """host arithmetic: usable where no device is visible (this test runs without one)"""
    p = E.blur_params(1, 0, 3, MOCO, 0.2)
    assert p.shape == (3,) and np.isfinite(p['sigma']).all() and set(p['gray'].tolist()) <= {0, 1}


# ------------------------------------------------------------------------------------------------------------------
# library refusals that launch nothing
# ------------------------------------------------------------------------------------------------------------------
def test_blur_params_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    nan, inf = float('nan'), float('inf')
    ok = (1, 0, 0, 4, 0.5, 0.1, 2.0, 0.2, p(256))
    def change(**kw):
        names = ('seed', 'call', 'first', 'n', 'p_blur', 'lo', 'hi', 'p_gray', 'out')
        return tuple(kw.get(k, v) for k, v in zip(names, ok))
    for args, word in ((change(out=None), 'null blur_dev'), (change(out=p(258)), '4-byte aligned'), (change(n=0), 'n = 0'),
                       (change(first=-1), 'first_frame = -1'), (change(p_blur=-0.1), 'probabilities -0.1'), (change(p_blur=1.5), 'in [0, 1]'),
                       (change(p_gray=nan), 'in [0, 1]'), (change(p_gray=inf), 'in [0, 1]'), (change(lo=0.0), 'sigma range (0'),
                       (change(lo=-1.0), '0 < lo <= hi'), (change(lo=3.0), '0 < lo <= hi'), (change(hi=inf), '0 < lo <= hi'),
                       (change(lo=nan), '0 < lo <= hi')):
        assert L.pvr_op_blur_params(*args, None) == PVR_ERR_INVALID, args
        assert 'pvr_op_blur_params' in _lib.last_error() and word in _lib.last_error(), (args, _lib.last_error())
    L.pvr_host_blur_params(1, 0, 0, 4, 0.5, 0.1, 2.0, 0.2, None)              # writes nothing through a null pointer
    a, b = np.zeros(4, E.BLUR_DTYPE), E.blur_params(1, 0, 4, (0.5, 1.0, 1.0), 0.2)
    L.pvr_host_blur_params(1, 0, 0, 4, 0.5, nan, 2.0, 0.2, a.ctypes.data_as(C.c_void_p))      # a bad range counts as (1, 1)
    assert np.array_equal(a, b)


def test_preprocess_staged_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    ok = dict(frames=p(256), n=1, h=64, w=64, resize=256, crop=224, windows=p(512), rects=None, color=None, sums=None, staged=p(1024))
    order = ('frames', 'n', 'h', 'w', 'resize', 'crop', 'windows', 'rects', 'color', 'sums', 'staged')
    call = lambda **k: L.pvr_op_preprocess_staged(*[dict(ok, **k)[x] for x in order], None)
    for kw, word in ((dict(frames=None), 'null frames_dev'), (dict(staged=None), 'null staged_dev'), (dict(windows=None), 'exactly one pixel source'),
                     (dict(rects=p(512)), 'exactly one pixel source'), (dict(staged=p(1032)), '16-byte aligned'), (dict(n=0), 'bad shape'),
                     (dict(n=65536), '65535'), (dict(resize=200), 'smaller than crop 224'), (dict(windows=p(514)), 'windows_dev 0x202 is not 4-byte aligned'),
                     (dict(windows=None, rects=p(514)), 'rects_dev 0x202 is not 4-byte aligned'), (dict(windows=None, rects=p(512), h=0), 'bad shape'),
                     (dict(color=p(768)), 'color_dev without gray_sums_dev'), (dict(color=p(770), sums=p(1536)), 'color_dev 0x302 is not 4-byte aligned'),
                     (dict(color=p(768), sums=p(1537)), 'gray_sums_dev 0x601'), (dict(color=p(768), sums=p(1536), resize=300, crop=257, h=300, w=300), 'crop 257')):
        assert call(**kw) == PVR_ERR_INVALID, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())


def test_blur_normalize_op_refusals():
    L = _lib.lib()
    p = C.c_void_p
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    ok = dict(staged=p(1024), n=1, crop=224, mean=mean, std=std, blur=p(512), out=p(2048))
    order = ('staged', 'n', 'crop', 'mean', 'std', 'blur', 'out')
    call = lambda **k: L.pvr_op_blur_normalize(*[dict(ok, **k)[x] for x in order], None)
    for kw, word in ((dict(staged=None), 'null argument'), (dict(mean=None), 'null argument'), (dict(out=None), 'null argument'),
                     (dict(blur=None), 'null blur_dev'), (dict(staged=p(1032)), 'staged_dev 0x408 is not 16-byte aligned'),
                     (dict(out=p(2056)), 'out_dev 0x808 is not 16-byte aligned'), (dict(blur=p(514)), 'blur_dev 0x202 is not 4-byte aligned'),
                     (dict(n=0), 'bad shape'), (dict(n=65536), '65535'), (dict(crop=11), 'crop 11 (at least 12'), (dict(crop=257), 'crop 257 (at most 256')):
        assert call(**kw) == PVR_ERR_INVALID, kw
        assert 'blur normalize' in _lib.last_error().replace('_', ' ') and word in _lib.last_error(), (kw, _lib.last_error())


def test_forward_staged_refusals():
    L = _lib.lib()
    d = _lib.EncoderDesc(arch=10, dtype=_lib.PVR_F32, max_batch=4, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert L.pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    try:
        one = C.c_void_p(16)
        def call(params=one, bufs=one, frames=one, n=1, hw=(64, 64), windows=one, rects=None, color=None, sums=None, blur=one, staged=one, boundary=None,
                 reuse=0, out=one):
            return L.pvr_trainer_forward_staged(h, params, bufs, frames, n, hw[0], hw[1], windows, rects, color, sums, blur, staged, boundary, reuse, out,
                                                512, None)
        name = 'pvr_trainer_forward_staged'
        for kw, word in ((dict(params=None), 'null argument'), (dict(frames=None), 'null argument'), (dict(out=None), 'null argument'),
                         (dict(windows=None), 'neither windows_dev nor rects_dev'), (dict(rects=one), 'both windows_dev and rects_dev'),
                         (dict(windows=C.c_void_p(18)), 'is not 4-byte aligned'), (dict(blur=C.c_void_p(18)), 'blur_dev 0x12 is not 4-byte aligned'),
                         (dict(staged=None), 'staged_dev'), (dict(staged=C.c_void_p(24)), 'staged_dev 0x18 is null or not 16-byte aligned'),
                         (dict(color=C.c_void_p(18), sums=one), 'color_dev 0x12 is not 4-byte aligned'), (dict(color=one), 'gray_sums_dev'),
                         (dict(n=0), 'max_batch = 4'), (dict(n=5), 'max_batch = 4'), (dict(hw=(0, 64)), 'bad frame size'),
                         (dict(boundary=one), 'everything trains')):
            assert call(**kw) != 0, kw
            assert name in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
        # without blur parameters the entry point is the one it extends, refusals included
        assert call(blur=None, windows=None, color=one, sums=one) == PVR_ERR_INVALID and 'pvr_trainer_forward_augmented' in _lib.last_error()
        assert call(blur=None, windows=None, rects=C.c_void_p(18)) == PVR_ERR_INVALID and 'pvr_trainer_forward_rects' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)
