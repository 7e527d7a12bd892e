"""The split-f16 weight gradients where no GPU is needed: the CPU emulation of tests/wgrad_split16_refs.py stays inside the derived bound at every
geometry, family and subnormal behaviour while each classic mistake exceeds it; the scale rule; what the new entry points refuse; the mode setter on a
fresh handle; the Python surface and the driver flag."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_refs as tr
import wgrad_split16_refs as ws
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

_refs = {}


def case(family, geo):
    """inputs, float64 reference and bound of one (family, geometry), computed once and left unchanged"""
    if (family, geo) not in _refs:
        x, dz = ws.inputs(family, geo)
        _refs[(family, geo)] = (x, dz) + ws.reference(x, dz, *geo[4:])
    return _refs[(family, geo)]


@pytest.mark.parametrize('geo', ws.GEOMETRIES)
@pytest.mark.parametrize('family', ws.FAMILIES)
@pytest.mark.parametrize('flush', [False, True])
def test_the_emulation_is_inside_the_bound(geo, family, flush):
    x, dz, ref, bound = case(family, geo)
    r = tr.ratio(ws.emulate(x, dz, *geo[4:], flush=flush), ref, bound)
    print('\n[split16 emulation %s %s flush %d] error / bound %.3f' % (geo, family, flush, r))
    assert r <= 1.0


# where each mistake is shown: the smallest and the largest L of CONV_GEOMETRIES; a missing pre-scale only shows on gradients of f16's subnormal size
MUTANT_CASES = [(m, f, g) for m in ('lo_dropped', 'one_cross', 'cross_unscaled', 'scale_not_undone') for f in ('unit', 'wide')
                for g in (tr.CONV_GEOMETRIES[1], tr.CONV_GEOMETRIES[4])] + [('no_prescale', 'tiny', g) for g in tr.CONV_GEOMETRIES]


@pytest.mark.parametrize('mutant,family,geo', MUTANT_CASES)
def test_every_mutant_exceeds_the_bound(mutant, family, geo):
    x, dz, ref, bound = case(family, geo)
    r = tr.ratio(ws.emulate(x, dz, *geo[4:], mutant=mutant), ref, bound)
    print('\n[split16 mutant %s %s %s] error / bound %.3g' % (mutant, geo, family, r))
    assert r > 1.0


def test_the_stem_emulation_is_inside_the_bound():
    for family in ('unit', 'tiny'):
        img, dz = ws.stem_inputs(family, 2, 32)
        ref, bound = ws.stem_reference(img, dz)
        for flush in (False, True):
            assert tr.ratio(ws.stem_emulate(img, dz, flush), ref, bound) <= 1.0
        assert tr.ratio(ws.stem_emulate(img, dz, mutant='lo_dropped'), ref, bound) > 1.0


def test_the_scale_rule():
    r = np.random.default_rng(2)
    for family in ws.FAMILIES:
        for t in ws.inputs(family, tr.CONV_GEOMETRIES[0]):
            s, a = ws.scale_rule(t), float(t.abs().max())
            assert np.log2(s) == int(np.log2(s)) and 2.0 ** 14 <= a * s < 2.0 ** 15, (family, s, a)
    for a in (1.0, 2.0, 1.9999999, 65504.0, 1e-6, 3e-20, float(r.uniform(0.1, 10.0))):
        s = ws.scale_rule(np.float32([0.0, -a, a / 3]))
        assert 2.0 ** 14 <= float(np.float32(a)) * s < 2.0 ** 15
    assert ws.scale_rule(np.zeros(7, np.float32)) == 1.0 and ws.scale_rule(np.zeros(0, np.float32)) == 1.0
    assert ws.scale_rule(np.float32([1.0, np.inf])) == 1.0 and ws.scale_rule(np.float32([np.nan, 1.0])) == 1.0
    tiny_normal = float(np.finfo(np.float32).tiny)
    for a in (2.0 ** -140, 3e38):                       # a subnormal and a near-maximal maximum: s and 1 / s stay normal fp32 numbers
        s = ws.scale_rule(np.float32([a]))
        assert np.float32(s) == s and np.float32(1.0 / s) == 1.0 / s and s >= tiny_normal and 1.0 / s >= tiny_normal, (a, s)
    assert ws.scale_rule(np.float32([2.0 ** -140])) == 2.0 ** 126 and ws.scale_rule(np.float32([3e38])) == 2.0 ** (14 - 127)


def test_the_new_entry_points_refuse_what_they_are_not_built_for():
    L = _lib.lib()
    one = (C.c_float * 1)()
    p = C.cast(one, C.c_void_p)
    big = 1 << 30
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 64, 64, 5, 1, 2, p, p, p, big, None) == 1 and 'k 5' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16_scratch_floats(2, 8, 8, 64, 64, 5, 1, 2) == 0
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 48, 64, 3, 1, 1, p, p, p, big, None) == 1 and 'cin' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 64, 62, 3, 1, 1, p, p, p, big, None) == 1 and 'cout' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 64, 64, 3, 1, 1, p, p, p, 16, None) == 1 and 'scratch' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 64, 64, 3, 1, 1, None, p, p, big, None) == 1 and 'scale' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16(p, p, p, 2, 8, 8, 64, 64, 3, 1, 1, p, None, p, big, None) == 1 and 'scale' in _lib.last_error()
    assert L.pvr_op_conv_wgrad_split16(p, None, p, 2, 8, 8, 64, 64, 3, 1, 1, p, p, p, big, None) == 1 and 'null' in _lib.last_error()
    assert L.pvr_op_stem_wgrad_split16(p, p, p, 2, 33, p, p, p, big, None) == 1 and 'even' in _lib.last_error()
    assert L.pvr_op_stem_wgrad_split16_scratch_floats(2, 33) == 0
    assert L.pvr_op_stem_wgrad_split16(p, p, p, 2, 32, p, p, p, 16, None) == 1 and 'scratch' in _lib.last_error()
    assert L.pvr_op_stem_wgrad_split16(p, p, p, 2, 32, None, p, p, big, None) == 1 and 'scale' in _lib.last_error()
    assert L.pvr_op_absmax_scale(None, 4, p, None) == 1 and 'null' in _lib.last_error()
    assert L.pvr_op_absmax_scale(p, 4, None, None) == 1 and 'null' in _lib.last_error()
    assert L.pvr_op_absmax_scale_pair(p, 4, p, p, 4, p, None, None) == 1 and 'null' in _lib.last_error()
    assert L.pvr_op_absmax_scale_pair(p, 4, p, p, 4, None, p, None) == 1 and 'together' in _lib.last_error()
    for geo in ws.GEOMETRIES:                             # whole pixel ranges of (cout, taps, cin) partials
        n, h, ci, co, k, s, pad = geo
        floats = L.pvr_op_conv_wgrad_split16_scratch_floats(n, h, h, ci, co, k, s, pad)
        assert floats > 0 and floats % (co * k * k * ci) == 0
    assert L.pvr_op_stem_wgrad_split16_scratch_floats(2, 32) == 64 * 147


def _create(arch=10, max_batch=4):
    d = _lib.EncoderDesc(arch=arch, dtype=_lib.PVR_F32, max_batch=max_batch, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    return h


@pytest.mark.parametrize('arch', [10, 0])
def test_the_mode_setter_on_a_fresh_handle(arch):
    L = _lib.lib()
    h = _create(arch)
    try:
        off = L.pvr_trainer_workspace_bytes(h)
        assert L.pvr_trainer_set_wgrad_split16(h, 1) == 0, _lib.last_error()
        on = L.pvr_trainer_workspace_bytes(h)
        assert off < on <= off + (128 << 20)                # the scale slots, and the partials of the split kernels' own pixel ranges
        assert L.pvr_trainer_set_bn_frozen(h, 1) == 0 and L.pvr_trainer_workspace_bytes(h) == on          # legal in both BatchNorm modes
        assert L.pvr_trainer_set_wgrad_split16(h, 0) == 0
        assert L.pvr_trainer_workspace_bytes(h) == off      # off: to the byte what it was
        assert L.pvr_trainer_set_wgrad_split16(None, 1) == 1 and 'null' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)


def test_trainer_workspace_bytes_takes_the_mode():
    off, on = E.trainer_workspace_bytes('resnet18', 4), E.trainer_workspace_bytes('resnet18', 4, wgrad_split16=True)
    assert off == E.trainer_workspace_bytes('resnet18', 4, wgrad_split16=False) and off < on <= off + (128 << 20)
    assert E.trainer_workspace_bytes('resnet18', 669, wgrad_split16=True) is None


def test_embeddingnet_refuses_the_mode_without_train():
    with pytest.raises(ValueError, match='wgrad_split16'):
        E.EmbeddingNet('resnet18', pretrained=False, wgrad_split16=True)
    with pytest.raises(NotImplementedError, match='resnet18'):
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, wgrad_split16=True)


def test_the_driver_flag():
    import argparse
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_wgrad_split16 is False
    f = make_parser().parse_args(['--train_embedding', '--embedding_wgrad_split16', '--freeze_embedding_bn'])
    assert f.embedding_wgrad_split16 is True and f.freeze_embedding_bn is True
    assert '--embedding_wgrad_split16' in make_parser().format_help()
    # the memory guard sizes the workspace of the mode
    import unittest.mock as mock
    gb = 1 << 30
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (64 * gb, 256 * gb)):
        base = dict(embedding_name='resnet18', unroll_length=2, batch_size=2, freeze_embedding_bn=False, embedding_chunk=None)
        assert Fz.check_workspace_fits(argparse.Namespace(embedding_wgrad_split16=True, **base), 2) == E.trainer_workspace_bytes('resnet18', 8, True)
        assert Fz.check_workspace_fits(argparse.Namespace(**base), 2) == E.trainer_workspace_bytes('resnet18', 8)
        fz = argparse.Namespace(embedding_wgrad_split16=True, **dict(base, freeze_embedding_bn=True, embedding_chunk=3))
        assert Fz.check_workspace_fits(fz, 2) == E.trainer_workspace_bytes('resnet18', 3, True) and fz.embedding_chunk == 3
