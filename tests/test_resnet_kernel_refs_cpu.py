"""The float64 references and bounds of oracle/resnet_kernel_refs.py can tell a right ResNet kernel from a subtly wrong one (CPU only): an fp32 / 16-bit
emulation of each kernel's arithmetic passes its bound on every input family and configuration tests/test_gpu_resnet_kernels.py uses, and every mutant
of that emulation fails on its named family - while the norm limits of tests/test_gpu_encoder.py::test_conv2d_matches_torch let two of them through."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet_kernel_refs as kr
from pvr_habitat_amd import synth

DTS = ('f16', 'bf16')


@functools.lru_cache(maxsize=None)
def _conv_case(family, shape, dt, res):
    return kr.conv_inputs(family, shape, dt, res)


def _conv_ratio(family, shape, dt, res, act, out16, mutant=None, **kw):
    x, wt, b, r = _conv_case(family, shape, dt, res)
    od = dt if out16 else None
    ref, bound = kr.conv_ref(x, wt, b, r, act, shape[7], shape[8], od)
    got = kr.conv_emulate(x, wt, b, r, act, shape[7], shape[8], od, mutant=mutant, **kw)
    return kr.ratio(got, ref, bound), got, ref


# ------------------------------------------------------------------------------------------------------------------
# convolution
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('entry', kr.CONV_GRID, ids=lambda e: 'x'.join(str(v) for v in e[0]))
def test_conv_emulation_within_bound(entry, dt):
    shape, configs, _ = entry
    worst = {}
    for res, act, out16 in configs:
        for family in kr.conv_families(res, act):
            r, got, ref = _conv_ratio(family, shape, dt, res, act, out16)
            worst[family] = max(worst.get(family, 0.0), r)
            assert r <= 1.0, (shape, family, res, act, out16, r)
            if family == 'exact':
                assert torch.equal(got.double(), ref), 'the exact family must come out bit for bit'
    print('\n[conv emulation %s %s] error / bound %s' % (shape, dt, {k: '%.2f' % v for k, v in worst.items()}))


@pytest.mark.parametrize('dt', DTS)
def test_exact_family_precondition(dt):
    """sum |x w| + |b| + |r| stays below the largest integer up to which every integer is representable, so every partial sum in any order is exact"""
    shapes = [e[0] for e in kr.CONV_GRID] + kr.SPLITK_SHAPES + [c[0] for c in kr.WFRAG_CASES]
    for shape in shapes:
        x, wt, b, r = _conv_case('exact', shape, dt, 'h')
        for t in (x, wt, b, r):
            assert torch.equal(t.float(), t.float().round()), 'integers only'
        S = kr._conv64(x.double().abs(), wt.double().abs(), shape[7], shape[8])
        total = S + b.double().abs() + r.double().abs()
        assert float(total.max()) <= kr.EXACT_LIMIT[dt], (shape, float(total.max()))
        assert float(S.max()) >= 6.0 and int((wt != 0).sum(dim=(1, 2, 3)).min()) >= 1, 'the weights are too sparse to see anything'
        # pixel values code position: horizontal and vertical neighbours differ everywhere
        if shape[2] > 1:
            assert (x[:, :, 1:] != x[:, :, :-1]).all()
        if shape[1] > 1:
            assert (x[:, 1:] != x[:, :-1]).all()


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('mutant', kr.CONV_MUTANTS)
def test_conv_mutant_fails(mutant, dt):
    family, shape, res, act, out16 = kr.CONV_CAUGHT_BY[mutant]
    honest, _, _ = _conv_ratio(family, shape, dt, res, act, out16)
    r, _, _ = _conv_ratio(family, shape, dt, res, act, out16, mutant)
    print('\n[conv mutant %s on %s %s %s] honest %.2f mutant %.2f' % (mutant, family, shape, dt, honest, r))
    assert honest <= 1.0
    assert r > 1.0, 'mutant %s passes %s at %s %s (ratio %.2f): the inputs are too weak' % (mutant, family, shape, dt, r)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape', kr.SPLITK_SHAPES)
def test_splitk_emulation_within_bound(shape, dt):
    for res, act, out16 in kr.SPLITK_CONFIGS:
        for family in kr.conv_families(res, act):
            for ks in kr.SPLITK_KSPLITS:
                r, got, ref = _conv_ratio(family, shape, dt, res, act, out16, ksplit=ks)
                assert r <= 1.0, (shape, family, ks, r)
                if family == 'exact':
                    assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', kr.WFRAG_CASES, ids=lambda c: 'x'.join(str(v) for v in c[0]))
def test_wfrag_shapes_emulation_within_bound(case, dt):
    shape, res = case
    for act, out16 in ((1, True), (0, False)):
        for family in kr.conv_families(res, act):
            r, got, ref = _conv_ratio(family, shape, dt, res, act, out16)
            assert r <= 1.0, (shape, family, act, out16, r)
            if family == 'exact':
                assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [1, 3])
def test_pooled_conv_emulation_and_mutants(n, dt):
    """the pooled epilogue: the fp32 activation averaged over 49 pixels; rounding it to storage first, or averaging 48 pixels, leaves the bound"""
    shape = (n, 7, 7, 64, 256, 1, 1, 1, 0)
    for family in ('unit', 'exact', 'cancel', 'relu_edge', 'large'):
        x, wt, b, r = _conv_case(family, shape, dt, 'h')
        ref, bound = kr.pooled_conv_ref(x, wt, b, r)
        y = kr.conv_emulate(x, wt, b, r, 1, 1, 0, None).reshape(n, 49, 256)
        assert kr.ratio(kr.avgpool_emulate(y), ref, bound) <= 1.0, family
        if family in ('unit', 'large'):
            assert kr.ratio(kr.avgpool_emulate(y.to(kr.TORCH_DT[dt])), ref, bound) > 1.0, family
            assert kr.ratio(kr.avgpool_emulate(y, 'avg_skips_last') * (49.0 / 48.0), ref, bound) > 1.0, family


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', kr.DUAL_CASES)
def test_dual_emulation_within_bound(case, dt):
    x, x2, wt, w2, b = kr.dual_inputs(case, dt)
    k, s2 = case[4], case[6]
    ref, bound = kr.conv_ref(x, wt, b, None, 1, 1, k // 2, dt, extra=(x2, w2, s2))
    assert kr.ratio(kr.conv_emulate(x, wt, b, None, 1, 1, k // 2, dt, extra=(x2, w2, s2)), ref, bound) <= 1.0
    shifted = kr.conv_emulate(x, wt, b, None, 1, 1, k // 2, dt, extra=(x2.roll(1, dims=2), w2, s2))      # the second operand read one column off
    assert kr.ratio(shifted, ref, bound) > 1.0


def test_activation_lipschitz_constants():
    """the constants of _act_bound against the derivatives on a fine grid; and where the tanh form differs from the erf form"""
    v = torch.linspace(-12.0, 12.0, 2400001, dtype=torch.float64, requires_grad=True)
    for fn, lip, sup in ((kr.quickgelu64, kr.QGELU_LIP, 1.0998), (kr.gelu64, kr.GELU_LIP, 1.1290)):
        g, = torch.autograd.grad(fn(v).sum(), v)
        assert float(g.abs().max()) <= lip
        assert abs(float(g.abs().max()) - sup) < 1e-3


@pytest.mark.parametrize('act', [2, 3])
def test_activation_emulation_within_bound_on_a_line(act):
    """the epilogue alone: exact pre-activation values (E = 0) from -30 to 30, the negative tail included"""
    v = torch.cat([torch.linspace(-30.0, 30.0, 600001), -torch.logspace(-30, 1.4, 2000), torch.logspace(-30, 1.4, 2000)]).float()
    ref, bound = kr._act_bound(v.double(), torch.zeros_like(v, dtype=torch.float64), act)
    got = kr._quickgelu32(v) if act == 2 else kr._gelu_erf32(v)
    r = kr.ratio(got, ref, bound + kr.U32 * ref.abs())
    print('\n[activation %d alone] error / bound %.2f' % (act, r))
    assert r <= 1.0
    wrong = kr._quickgelu32(v, 1.7) if act == 2 else kr._gelu_tanh32(v)
    assert kr.ratio(wrong, ref, bound + kr.U32 * ref.abs()) > 1.0


def _relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)), float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', [(2, 56, 56, 64, 64, 3, 1, 1, 0, 0), (3, 14, 14, 512, 512, 3, 2, 1, 0, 0), (1, 7, 7, 2048, 512, 1, 1, 1, 0, 0)])
def test_norm_limits_of_the_torch_comparison_pass_two_mutants(case, dt):
    """Why this suite exists.  tests/test_gpu_encoder.py::test_conv2d_matches_torch compares rel-L2 and max-norm errors against torch fp32 at
    8e-4 / 6e-3.  On that test's own inputs a kernel that rounds its accumulator to the storage type after every filter tap, and one that rounds its bias
    to 16 bits, both pass those limits in both storage types; the elementwise bounds above catch both (test_conv_mutant_fails)."""
    n, h, w, cin, cout, k, stride, relu, res, out_f32 = case
    tdt = kr.TORCH_DT[dt]
    pad = k // 2
    x = torch.from_numpy(synth.normal(3, 'cx%s' % (case,), (n, h, w, cin))).to(tdt)
    wt = torch.from_numpy(synth.normal(3, 'cw%s' % (case,), (cout, cin, k, k), std=float(np.sqrt(2.0 / (cin * k * k))))).to(tdt)
    b = torch.from_numpy(synth.uniform(3, 'cb%s' % (case,), (cout,), -0.5, 0.5))
    ref = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), wt.float(), b, stride, pad).permute(0, 2, 3, 1))
    tol = 6e-3 if dt == 'bf16' else 8e-4
    figures = {}
    for mutant in (None, 'round_per_tap', 'bias_16bit'):
        got = kr.conv_emulate(x, wt.permute(0, 2, 3, 1).contiguous(), b, None, 1, stride, pad, dt, mutant=mutant)
        l2, mx = _relerr(got.float().numpy(), ref.numpy())
        figures[mutant or 'honest'] = '%.1e / %.1e' % (l2, mx)
        assert l2 < tol and mx < 2 * tol + 1e-3, (mutant, l2, mx)
    print('\n[norm limits %s %s] rel-L2 / max-norm %s' % (case, dt, figures))


# ------------------------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_case(family, dt, pool):
    img = kr.stem_image(family, 2, dt)
    wgt, b = kr.stem_weights(family, dt)
    return (img, wgt, b) + kr.stem_ref(img, wgt, b, pool)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('family', kr.STEM_FAMILIES)
def test_stem_emulation_within_bound(family, pool, dt):
    img, wgt, b, ref, bound = _stem_case(family, dt, pool)
    got = kr.stem_emulate(img, wgt, b, pool)
    r = kr.ratio(got, ref, bound)
    print('\n[stem emulation %s pool %d %s] error / bound %.2f' % (family, pool, dt, r))
    assert r <= 1.0
    if family == 'impulse':
        assert torch.equal(got.double(), ref), 'the impulse outputs are weights: exact'
        assert int((ref > 0).sum()) >= 9 * 64 // 4, 'too few outputs see an impulse'


def test_uint8_family_is_the_production_contract():
    img = kr.stem_image('uint8', 1, 'bf16').float()
    wgt, _ = kr.stem_weights('uint8', 'bf16')
    assert (img[:, 3:227, 3:227, 3] == 1).all() and (img[..., :3] == img[..., :3].round()).all() and float(img[..., :3].abs().max()) <= 128
    border = img.clone(); border[:, 3:227, 3:227] = 0
    assert (border == 0).all() and (wgt[:, :, 7, :] == 0).all()
    frames = kr.stem_frames(1, 256, 320)
    crop = kr.stem_image_from_frames(frames, 32, 96, 'f16').float()
    assert torch.equal(crop[0, 3, 3, :3], frames[0, 32, 96].float() - 128.0) and torch.equal(crop[0, 226, 226, :3], frames[0, 255, 319].float() - 128.0)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('mutant', [m for m in kr.STEM_MUTANTS if kr.STEM_CAUGHT_BY[m]])
def test_stem_mutant_fails(mutant, dt):
    family = kr.STEM_CAUGHT_BY[mutant]
    for pool in ((True,) if mutant.startswith('pool_') else (False, True)):
        img, wgt, b, ref, bound = _stem_case(family, dt, pool)
        r = kr.ratio(kr.stem_emulate(img, wgt, b, pool, mutant), ref, bound)
        assert r > 1.0, 'mutant %s passes %s (pool %d, %s, ratio %.2f): the inputs are too weak' % (mutant, family, pool, dt, r)


def test_tap7_is_invisible_under_the_production_contract():
    """why the generic family exists: with weight column 7 zero a kernel that drops tap 7 computes the same function"""
    img, wgt, b, ref, bound = _stem_case('uint8', 'f16', False)
    assert torch.equal(kr.stem_emulate(img, wgt, b, False, 'tap7_dropped'), kr.stem_emulate(img, wgt, b, False))


@pytest.mark.parametrize('dt', DTS)
def test_pool_padding_is_harmless_after_relu(dt):
    """the fused kernels start their maximum from 0, torch pads with -inf: the same function on post-ReLU values (pool_pads_with_zero of the table)"""
    assert kr.STEM_CAUGHT_BY['pool_pads_with_zero'] is None
    for family in kr.STEM_FAMILIES:
        img, wgt, b, _, _ = _stem_case(family, dt, True)
        assert torch.equal(kr.stem_emulate(img, wgt, b, True, 'pool_pads_with_zero'), kr.stem_emulate(img, wgt, b, True))
    x = kr.maxpool_inputs(2, 7, 9, 8, dt)                                      # ... and not on signed values: the general max pool must pad with -inf
    zero_pad = F.max_pool2d(F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1)
    assert not torch.equal(zero_pad, kr.maxpool_ref(x).float())


# ------------------------------------------------------------------------------------------------------------------
# pools and layout kernels
# ------------------------------------------------------------------------------------------------------------------
def test_maxpool_inputs_have_the_edge_values():
    for dt in DTS:
        for n, h, w, c in kr.MAXPOOL_GRID:
            x = kr.maxpool_inputs(n, h, w, c, dt)
            xf = x.float()
            ref = kr.maxpool_ref(x)
            assert ref.shape == (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c) and torch.isfinite(ref.float()).all()
            if h >= 5:
                zeros = xf[xf == 0]
                assert (xf < 0).any() and torch.signbit(zeros).any() and not torch.signbit(zeros).all()
                assert (xf[-1, h - 3:, w - 3:] == -1.5).all(), 'a constant window'
            if h <= 3:
                assert float(ref.float().min()) == float(torch.finfo(kr.TORCH_DT[dt]).min), 'the most negative value must win against the padding'


@pytest.mark.parametrize('dt', DTS + ('f32',))
def test_avgpool_emulation_and_mutants(dt):
    worst = 0.0
    for hw in kr.AVGPOOL_HW:
        for c in (8, 2056):
            x = kr.pool_inputs((3, hw, c), dt, 'avg')
            ref, bound = kr.avgpool_ref(x)
            r = kr.ratio(kr.avgpool_emulate(x), ref, bound)
            worst = max(worst, r)
            assert r <= 1.0, (hw, c, r)
            assert kr.ratio(kr.avgpool_emulate(x, 'avg_divides_by_hw_plus_1'), ref, bound) > 1.0
            if hw > 1:
                assert kr.ratio(kr.avgpool_emulate(x, 'avg_skips_last'), ref, bound) > 1.0
    print('\n[avgpool emulation %s] largest error / bound %.2f' % (dt, worst))


@pytest.mark.parametrize('dt', DTS)
def test_avgpool2_and_attnpool_tokens_emulation(dt):
    tdt = kr.TORCH_DT[dt]
    for shape in kr.AVGPOOL2_GRID:
        x = kr.pool_inputs(shape, dt, 'avg2')
        n, h, w, c = shape
        ref, bound = kr.avgpool2_ref(x)
        xf = x.float().reshape(n, h // 2, 2, w // 2, 2, c)
        got = (((xf[:, :, 0, :, 0] + xf[:, :, 0, :, 1]) + xf[:, :, 1, :, 0]) + xf[:, :, 1, :, 1]) * 0.25
        assert kr.ratio(got.to(tdt), ref, bound) <= 1.0
        assert kr.ratio((xf[:, :, 0, :, 0] * 1.0).to(tdt), ref, bound) > 1.0          # the top-left pixel alone
    for n, hw, c in kr.ATTNPOOL_GRID:
        x, pos = kr.pool_inputs((n, hw, c), 'f32', 'apx'), kr.pool_inputs((hw + 1, c), 'f32', 'app')
        ref, bound = kr.attnpool_tokens_ref(x, pos, dt)
        got = torch.cat([(kr.avgpool_emulate(x) + pos[0])[:, None], x + pos[1:]], dim=1).to(tdt)
        assert kr.ratio(got, ref, bound) <= 1.0
        if hw > 1:
            off = torch.cat([(kr.avgpool_emulate(x) + pos[0])[:, None], x + pos[:-1]], dim=1).to(tdt)   # positional rows off by one
            assert kr.ratio(off, ref, bound) > 1.0


def test_nhwc_to_chw_emulation_and_mutant():
    for n, hw, cpad, creal in kr.CHW_GRID:
        x = kr.pool_inputs((n, hw, cpad), 'f32', 'chw')
        ref = kr.nhwc_to_chw_ref(x, creal)
        assert torch.equal(kr.nhwc_to_chw_emulate(x, creal), ref)
        assert torch.equal(ref.reshape(n, creal, hw)[:, 3 % creal, hw - 1], x[:, hw - 1, 3 % creal])
        if creal != cpad:
            assert not torch.equal(kr.nhwc_to_chw_emulate(x, creal, 'chw_uses_creal_stride'), ref)


def test_every_mutant_of_the_table_is_exercised():
    assert set(kr.CONV_CAUGHT_BY) == set(kr.CONV_MUTANTS)
    assert set(kr.STEM_CAUGHT_BY) == set(kr.STEM_MUTANTS)
    assert set(kr.CONV_MUTANTS) == {'round_per_tap', 'bias_16bit', 'relu_before_residual', 'bias_by_tile', 'pad_wraps_row', 'origin_without_pad',
                                    'drop_last_k_slice', 'residual_16bit', 'quickgelu_1p7', 'gelu_tanh'}
    assert set(kr.STEM_MUTANTS) == {'tap7_dropped', 'row_origin_off_by_one', 'validity_ignored', 'pool_pads_with_zero', 'pool_window_2x2'}
    assert set(kr.POOL_MUTANTS) == {'avg_divides_by_hw_plus_1', 'avg_skips_last', 'chw_uses_creal_stride'}
    families = {kr.CONV_CAUGHT_BY[m][0] for m in kr.CONV_MUTANTS}
    assert families <= set(kr.CONV_FAMILIES)
