"""The float64 references and bounds of oracle/vit_kernel_refs.py can tell a right ViT kernel from a subtly wrong one (CPU only):
an fp32 / 16-bit emulation of each kernel's arithmetic passes its bound on every input family tests/test_gpu_vit_kernels.py uses,
and every mutant of that emulation fails on at least one named family."""
import functools

import pytest
import torch

from oracle import vit_kernel_refs as kr

# (T, heads, head dim): ragged, tile-exact and full key counts of both head dims - a subset of the GPU grid, same generators
ATT_SHAPES = [(1, 1, 64), (17, 2, 64), (50, 2, 64), (101, 1, 64), (197, 2, 64), (257, 1, 64), (288, 1, 64), (50, 2, 80), (101, 2, 80), (257, 2, 80)]
DTS = ('f16', 'bf16')


@functools.lru_cache(maxsize=None)
def _att_case(family, T, heads, hd, dt):
    qkv = kr.attention_inputs(family, T, heads, hd, 2, dt)
    return (qkv,) + kr.attention_ref(qkv, heads)


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('family', kr.ATT_FAMILIES)
def test_attention_emulation_within_bound(family, dt):
    worst = 0.0
    for T, heads, hd in ATT_SHAPES:
        qkv, ref, bound = _att_case(family, T, heads, hd, dt)
        r = kr.ratio(kr.attention_emulate(qkv, heads), ref, bound)
        worst = max(worst, r)
        assert r <= 1.0, (family, dt, T, heads, hd, r)
    print('\n[attention emulation %s %s] largest error / bound %.2f' % (family, dt, worst))


# mutant -> the family that must catch it, in both storage types (no_max: f16 only - P in bf16 has fp32's exponent range, where the peaked
# logits do not overflow and the mutant is the same function)
ATT_CAUGHT_BY = {'drop_last_key': 'dominant', 'count_padded_key': 'negative', 'scale_hd80': 'peaked', 'no_max': 'peaked', 'v_shift': 'dominant'}


@pytest.mark.parametrize('mutant,dt', [(m, dt) for m in kr.ATT_MUTANTS for dt in DTS if (m, dt) != ('no_max', 'bf16')])
def test_attention_mutant_fails(mutant, dt):
    family = ATT_CAUGHT_BY[mutant]
    worst = 0.0
    for T, heads, hd in ATT_SHAPES:
        if mutant == 'scale_hd80' and hd != 80:
            continue
        if mutant == 'count_padded_key' and T % 32 == 0:
            continue
        if mutant in ('drop_last_key', 'v_shift') and T == 1:
            continue
        if mutant == 'no_max' and T < 50:                           # too few keys for one of them to reach the overflow threshold
            continue
        qkv, ref, bound = _att_case(family, T, heads, hd, dt)
        r = kr.ratio(kr.attention_emulate(qkv, heads, mutant), ref, bound)
        worst = max(worst, r)
        assert r > 1.0, 'mutant %s passes %s at T %d hd %d %s (ratio %.2f): the inputs are too weak' % (mutant, family, T, hd, dt, r)
    print('\n[attention mutant %s on %s %s] caught at every shape' % (mutant, family, dt))


def test_padded_key_is_invisible_on_unit_inputs():
    """why the 'negative' family exists: on N(0,1) inputs the padded-key mutant stays inside the bound at the production token counts"""
    for T in (197, 257):
        qkv, ref, bound = _att_case('unit', T, 2 if T == 197 else 1, 64, 'bf16')
        assert kr.ratio(kr.attention_emulate(qkv, 2 if T == 197 else 1, 'count_padded_key'), ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------------------------
LN_W = (768, 1024, 1280)


def _ln_plain(family, W, eps, out_dt, mutant=None):
    x = kr.layernorm_rows(family, 5, W)
    g, b = kr.layernorm_params(W)
    ref, bound = kr.layernorm_ref(x, g, b, eps, out_dt=out_dt)
    return kr.ratio(kr.layernorm_emulate(x, None, None, None, g, b, 1, eps, out_dt=out_dt, mutant=mutant), ref, bound)


def _ln_assembly(T, W, normalize, out_dt, mutant=None):
    pe, cls, pos = kr.assembly_inputs(3, T, W)
    g, b = kr.layernorm_params(W)
    ref, bound = kr.layernorm_ref(kr.assemble(pe.double(), cls.double(), pos.double(), T), g, b, 1e-5, normalize, out_dt, assembled=True)
    return kr.ratio(kr.layernorm_emulate(None, pe, cls, pos, g, b, T, 1e-5, normalize, out_dt, mutant), ref, bound)


@pytest.mark.parametrize('out_dt', (None,) + DTS)
@pytest.mark.parametrize('W', LN_W)
def test_layernorm_emulation_within_bound(W, out_dt):
    worst = 0.0
    for family in kr.LN_FAMILIES:
        for eps in (1e-5, 1e-6):
            r = _ln_plain(family, W, eps, out_dt)
            worst = max(worst, r)
            assert r <= 1.0, (family, W, eps, out_dt, r)
    for T in (2, 50, 197):
        for normalize in (1, 0):
            r = _ln_assembly(T, W, normalize, out_dt)
            worst = max(worst, r)
            assert r <= 1.0, ('assembly', T, W, normalize, out_dt, r)
    print('\n[layernorm emulation W %d %s] largest error / bound %.2f' % (W, out_dt or 'f32', worst))


def test_constant_row_gives_beta_exactly():
    for W in LN_W:
        g, b = kr.layernorm_params(W)
        out = kr.layernorm_emulate(kr.layernorm_rows('constant', 3, W), None, None, None, g, b, 1, 1e-5)
        assert torch.equal(out, b.expand(3, W))


@pytest.mark.parametrize('W', LN_W)
@pytest.mark.parametrize('mutant,family', [('eps_swapped', 'small_var'), ('divisor_w_minus_1', 'unit'), ('one_pass_variance', 'offset')])
def test_layernorm_numeric_mutant_fails(mutant, family, W):
    for eps in (1e-5, 1e-6):
        r = _ln_plain(family, W, eps, None, mutant)
        assert r > 1.0, 'mutant %s passes %s at W %d eps %g (ratio %.2f): the inputs are too weak' % (mutant, family, W, eps, r)
    if mutant == 'eps_swapped':                                      # 4 % of the output: visible in both 16-bit outputs too
        for dt in DTS:
            assert _ln_plain(family, W, 1e-5, dt, mutant) > 1.0


@pytest.mark.parametrize('W', LN_W)
@pytest.mark.parametrize('mutant', ['pos_by_row', 'cls_last'])
def test_layernorm_assembly_mutant_fails(mutant, W):
    for T in (2, 50):
        for normalize in (1, 0):
            for out_dt in (None,) + DTS:
                r = _ln_assembly(T, W, normalize, out_dt, mutant)
                assert r > 1.0, 'mutant %s passes the assembly family at T %d W %d (ratio %.2f)' % (mutant, T, W, r)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W', LN_W)
@pytest.mark.parametrize('out_dim', [512, 0])
def test_cls_head_emulation_and_mutants(W, out_dim):
    g, b = kr.layernorm_params(W)
    for T in (1, 50):
        x, proj = kr.cls_head_inputs(3, T, W, out_dim)
        for eps in (1e-5, 1e-6):
            ref, bound = kr.cls_head_ref(x, g, b, proj, T, eps)
            r = kr.ratio(kr.cls_head_emulate(x, g, b, proj, T, eps), ref, bound)
            assert r <= 1.0, (W, out_dim, T, eps, r)
        if T > 1:
            assert kr.ratio(kr.cls_head_emulate(x, g, b, proj, T, eps, 'token_1'), ref, bound) > 1.0
        if proj is not None:
            assert kr.ratio(kr.cls_head_emulate(x, g, b, proj, T, eps, 'proj_transposed'), ref, bound) > 1.0


def test_every_mutant_of_the_table_is_exercised():
    assert set(ATT_CAUGHT_BY) == set(kr.ATT_MUTANTS)
    assert set(kr.LN_MUTANTS) == {'eps_swapped', 'divisor_w_minus_1', 'one_pass_variance', 'pos_by_row', 'cls_last'}
    assert set(kr.CLS_MUTANTS) == {'token_1', 'proj_transposed'}
