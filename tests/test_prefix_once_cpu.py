"""The prefix_once mode (pvr_trainer_forward_boundary, pvr_trainer_set_prefix_fused; EmbeddingNet(..., train=True, train_from=..., prefix_once=True);
--embedding_prefix_once) without a GPU: the new symbols, the boundary tensor's size, the workspace of the fused split prefix, keyword and flag
validation, the memory guards with the boundary cache, and the fused split op's references - the fp32 emulation of tests/prefix_once_refs.py passes
its bound at every geometry and every mutant exceeds it."""
import argparse
import ctypes as C
import unittest.mock as mock

import pytest
import torch

import prefix_once_refs as po
import train_from_refs as tf
import train_refs as tr
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

ARCH = {'resnet18': 10, 'resnet50': 0}
SYMBOLS = ('pvr_trainer_boundary_floats', 'pvr_trainer_forward_boundary', 'pvr_trainer_set_prefix_fused', 'pvr_op_conv_bn_frozen_forward_split16',
           'pvr_op_conv_bn_frozen_forward_split16_scratch_floats')


def _create(name, max_batch=8):
    d = _lib.EncoderDesc(arch=ARCH[name], dtype=_lib.PVR_F32, max_batch=max_batch, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    return h


def test_the_symbols_are_exported():
    L = _lib.lib()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib._SIGS, s


@pytest.mark.parametrize('name', list(ARCH))
def test_boundary_floats(name):
    L = _lib.lib()
    h = _create(name)
    try:
        assert L.pvr_trainer_boundary_floats(h) == 0 and L.pvr_trainer_boundary_floats(None) == 0
        for stage in range(1, 5):
            assert L.pvr_trainer_set_train_from(h, stage) == 0, _lib.last_error()
            assert L.pvr_trainer_boundary_floats(h) == po.BOUNDARY_FLOATS[name][stage - 1], stage
            assert E.trainer_boundary_bytes(name, 'layer%d' % stage) == 4 * po.BOUNDARY_FLOATS[name][stage - 1]
        assert L.pvr_trainer_set_train_from(h, 0) == 0 and L.pvr_trainer_boundary_floats(h) == 0
        assert E.trainer_boundary_bytes(name, None) == 0
    finally:
        L.pvr_trainer_destroy(h)


@pytest.mark.parametrize('name', list(ARCH))
def test_set_prefix_fused_and_the_workspace(name):
    L = _lib.lib()
    h, fresh = _create(name), _create(name)
    try:
        assert L.pvr_trainer_set_prefix_fused(None, 1) == 1 and 'null' in _lib.last_error()
        plain = L.pvr_trainer_workspace_bytes(fresh)
        assert L.pvr_trainer_set_prefix_fused(h, 1) == 0 and L.pvr_trainer_workspace_bytes(h) == plain       # stage 0: equal on and off
        assert L.pvr_trainer_set_train_from(h, 3) == 0 and L.pvr_trainer_set_train_from(fresh, 3) == 0
        assert L.pvr_trainer_workspace_bytes(h) == L.pvr_trainer_workspace_bytes(fresh)                      # without conv_split16: equal on and off
        assert L.pvr_trainer_set_wgrad_split16(h, 1) == 0 and L.pvr_trainer_set_wgrad_split16(fresh, 1) == 0
        assert L.pvr_trainer_workspace_bytes(h) == L.pvr_trainer_workspace_bytes(fresh)                      # (wgrad_split16 is not conv_split16)
        assert L.pvr_trainer_set_conv_split16(h, 1) == 0 and L.pvr_trainer_set_conv_split16(fresh, 1) == 0
        assert L.pvr_trainer_workspace_bytes(h) < L.pvr_trainer_workspace_bytes(fresh)                       # stage 3 with conv_split16: strictly below
        assert L.pvr_trainer_set_prefix_fused(h, 0) == 0
        assert L.pvr_trainer_workspace_bytes(h) == L.pvr_trainer_workspace_bytes(fresh)                      # off again: the untouched handle's value
        assert L.pvr_trainer_set_prefix_fused(h, 1) == 0 and L.pvr_trainer_set_train_from(h, 0) == 0 and L.pvr_trainer_set_train_from(fresh, 0) == 0
        assert L.pvr_trainer_workspace_bytes(h) == L.pvr_trainer_workspace_bytes(fresh)                      # stage 0 with conv_split16: equal
    finally:
        L.pvr_trainer_destroy(h)
        L.pvr_trainer_destroy(fresh)


def test_forward_boundary_at_stage_0_is_a_state_error_before_anything_touches_the_device():
    L = _lib.lib()
    h = _create('resnet18')
    try:
        one = C.c_void_p(16)                          # (never dereferenced: the refusal comes first)
        assert L.pvr_trainer_forward_boundary(h, one, one, one, 1, 64, 64, one, 0, one, 512, None) == 4       # PVR_ERR_STATE
        assert 'pvr_trainer_forward_boundary' in _lib.last_error() and 'no frozen prefix' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)


def test_trainer_workspace_bytes_takes_the_keyword():
    from pvr_habitat_amd import main_bc_finetune as Fz
    off = E.trainer_workspace_bytes('resnet18', 8, False, True, train_from='layer3')
    assert E.trainer_workspace_bytes('resnet18', 8, False, True, train_from='layer3', prefix_once=False) == off
    assert E.trainer_workspace_bytes('resnet18', 8, False, True, train_from='layer3', prefix_once=True) < off
    assert E.trainer_workspace_bytes('resnet18', 8, train_from='layer3', prefix_once=True) == E.trainer_workspace_bytes('resnet18', 8, train_from='layer3')
    with pytest.raises(ValueError, match='no frozen prefix to keep'):
        E.trainer_workspace_bytes('resnet18', 8, prefix_once=True)
    free = E.trainer_workspace_bytes('resnet50', 40, False, True, train_from='layer3')
    assert Fz.largest_fitting_frames('resnet50', 300, free, False, True, 'layer3') == 40 \
        < Fz.largest_fitting_frames('resnet50', 300, free, False, True, 'layer3', prefix_once=True)


def test_keyword_validation():
    with pytest.raises(ValueError, match='no frozen prefix to keep'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, prefix_once=True)
    with pytest.raises(ValueError, match='train=True.*no frozen prefix to keep'):
        E.EmbeddingNet('resnet18', pretrained=False, train_from=None, prefix_once=True)
    with pytest.raises(ValueError, match='train=True'):
        E.EmbeddingNet('resnet18', pretrained=False, train_from='layer3', prefix_once=True)
    with pytest.raises(NotImplementedError, match='resnet18'):
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, train_from='layer3', prefix_once=True)


def test_the_driver_flag():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_prefix_once is False
    f = make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--freeze_embedding_bn', '--embedding_prefix_once'])
    assert f.embedding_prefix_once is True and Fz.workspace_modes(f) == {'train_from': 'layer3', 'prefix_once': True}
    assert '--embedding_prefix_once' in make_parser().format_help()
    with pytest.raises(ValueError, match='--embedding_prefix_once needs --embedding_train_from'):
        Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_prefix_once']))
    with pytest.raises(ValueError, match='--embedding_prefix_once needs --embedding_train_from'):
        Fz.workspace_modes(argparse.Namespace(embedding_prefix_once=True))
    gb = 1 << 30
    base = dict(embedding_name='resnet18', unroll_length=100, batch_size=16, freeze_embedding_bn=True, embedding_chunk=None, embedding_train_from='layer2')
    frames = 100 * 16 * 2
    cache = frames * E.trainer_boundary_bytes('resnet18', 'layer2')
    assert cache == frames * 4 * 56 * 56 * 64 and Fz.boundary_cache_bytes(argparse.Namespace(**base), frames) == 0
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (8 * gb, 256 * gb)):       # the guard and the default chunk count the cache
        off, on = argparse.Namespace(**base), argparse.Namespace(embedding_prefix_once=True, **base)
        need_off, need_on = Fz.check_workspace_fits(off, 2), Fz.check_workspace_fits(on, 2)
        assert 1 <= on.embedding_chunk < off.embedding_chunk                     # the cache takes its part of the nine tenths
        assert need_off == E.trainer_workspace_bytes('resnet18', off.embedding_chunk, train_from='layer2')
        assert need_on == E.trainer_workspace_bytes('resnet18', on.embedding_chunk, train_from='layer2', prefix_once=True) + cache <= 8 * gb // 10 * 9
        given = argparse.Namespace(embedding_prefix_once=True, **dict(base, embedding_chunk=off.embedding_chunk))
        with pytest.raises(RuntimeError, match='boundary cache of --embedding_prefix_once for 3200 frames'):    # the message names both sizes
            Fz.check_workspace_fits(given, 2)
        whole = argparse.Namespace(embedding_prefix_once=True, **dict(base, freeze_embedding_bn=False, unroll_length=2, batch_size=2))
        assert Fz.check_workspace_fits(whole, 2) == E.trainer_workspace_bytes('resnet18', 8, train_from='layer2', prefix_once=True) \
            + 8 * E.trainer_boundary_bytes('resnet18', 'layer2')
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (2 * gb, 256 * gb)):       # a cache that alone passes the nine tenths
        with pytest.raises(RuntimeError, match='chunk of one frame.*boundary cache of --embedding_prefix_once'):
            Fz.check_workspace_fits(argparse.Namespace(embedding_prefix_once=True, **base), 2)


# ------------------------------------------------------------------------------------------------------------------
# the fused split prefix op's references
# ------------------------------------------------------------------------------------------------------------------
def _run(geo, family, with_res, relu, mutant=None):
    d = tf.fused_inputs(family, geo)
    res = d['res'] if with_res else None
    args = (d['x'], d['wt'], d['gamma'], d['beta'], d['run_mean'], d['run_var'], res, relu, geo[5], geo[6])
    ref, bound = po.fused_split_reference(*args)
    return tr.ratio(po.fused_split_emulate(*args, mutant=mutant), ref, bound)


@pytest.mark.parametrize('geo', po.GEOMETRIES, ids=str)
def test_the_emulation_passes_the_bound_and_every_mutant_exceeds_it(geo):
    worst = 0.0
    for family in po.FAMILIES:
        for with_res in (False, True):
            for relu in (0, 1):
                worst = max(worst, _run(geo, family, with_res, relu))
    print('\n[fused split prefix op, emulation %s] largest error / bound %.3f' % (geo, worst))
    assert worst <= 1.0, worst
    for mutant, (_, _, families) in po.MUTANTS.items():
        for family in families:
            r = _run(geo, family, True, 1, mutant)
            assert r > 1.0, (mutant, family, r)
