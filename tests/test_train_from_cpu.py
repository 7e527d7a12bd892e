"""Partial fine-tuning (pvr_trainer_set_train_from; EmbeddingNet(..., train=True, train_from='layer3'); --embedding_train_from) without a GPU: the new
symbols, the handle's arithmetic of workspace and offsets, keyword and flag validation, and the fused prefix op's references - the fp32 emulation of
tests/train_from_refs.py passes its bound at every geometry and every mutant exceeds it."""
import argparse
import ctypes as C
import unittest.mock as mock

import pytest
import torch

import train_from_refs as tf
import train_refs as tr
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

ARCH = {'resnet18': 10, 'resnet50': 0}
SYMBOLS = ('pvr_trainer_set_train_from', 'pvr_trainer_train_from', 'pvr_trainer_trained_offset', 'pvr_op_conv_bn_frozen_forward',
           'pvr_op_conv_bn_frozen_forward_scratch_floats')


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
def test_stage_validation_workspace_and_offsets(name):
    L = _lib.lib()
    h, fresh = _create(name), _create(name)
    try:
        assert L.pvr_trainer_train_from(h) == 0 and L.pvr_trainer_trained_offset(h) == 0
        for bad in (5, -1):
            assert L.pvr_trainer_set_train_from(h, bad) == 1 and 'stage %d' % bad in _lib.last_error()      # PVR_ERR_INVALID, nothing changed
            assert L.pvr_trainer_train_from(h) == 0
        assert L.pvr_trainer_set_train_from(None, 1) == 1 and 'null' in _lib.last_error()
        names, buf = [], C.create_string_buffer(128)
        while L.pvr_trainer_param_name(h, len(names), buf, 128):
            names.append(buf.value.decode())
        numel = C.c_int64()
        sizes = []
        for stage in range(5):
            assert L.pvr_trainer_set_train_from(h, stage) == 0, _lib.last_error()
            assert L.pvr_trainer_train_from(h) == stage
            sizes.append(L.pvr_trainer_workspace_bytes(h))
            if stage:
                first = 'layer%d.0.conv1.weight' % stage
                off = L.pvr_trainer_param_offset(h, first.encode(), None, None)
                assert off > 0 and L.pvr_trainer_trained_offset(h) == off
                below = 0                             # parameters are laid out in op order: the prefix is the one leading span
                for n in names[:names.index(first)]:
                    assert L.pvr_trainer_param_offset(h, n.encode(), C.byref(numel), None) == below, n
                    below += numel.value
                assert below == off
                assert all(not tf.is_trained(n, stage) for n in names[:names.index(first)])
                assert all(tf.is_trained(n, stage) for n in names[names.index(first):])
        assert all(a > b for a, b in zip(sizes, sizes[1:])), sizes        # strictly decreasing in the stage
        assert sizes[0] == L.pvr_trainer_workspace_bytes(fresh)           # stage 0 after a set(0): the untouched handle's value to the byte
        for setter in (L.pvr_trainer_set_wgrad_split16, L.pvr_trainer_set_conv_split16):
            assert setter(h, 1) == 0 and setter(fresh, 1) == 0
            assert L.pvr_trainer_set_train_from(h, 3) == 0 and L.pvr_trainer_workspace_bytes(h) < L.pvr_trainer_workspace_bytes(fresh)
            assert L.pvr_trainer_set_train_from(h, 0) == 0 and L.pvr_trainer_workspace_bytes(h) == L.pvr_trainer_workspace_bytes(fresh)
            assert setter(h, 0) == 0 and setter(fresh, 0) == 0
            assert L.pvr_trainer_workspace_bytes(h) == sizes[0]
        assert L.pvr_trainer_set_bn_frozen(h, 1) == 0 and L.pvr_trainer_set_train_from(h, 2) == 0       # legal in both BatchNorm modes
        assert L.pvr_trainer_workspace_bytes(h) == sizes[2]
    finally:
        L.pvr_trainer_destroy(h)
        L.pvr_trainer_destroy(fresh)


def test_trainer_workspace_bytes_and_largest_fitting_frames_take_the_keyword():
    from pvr_habitat_amd import main_bc_finetune as Fz
    full = E.trainer_workspace_bytes('resnet18', 8)
    assert E.trainer_workspace_bytes('resnet18', 8, train_from=None) == full
    sizes = [full] + [E.trainer_workspace_bytes('resnet18', 8, train_from=s) for s in E.TRAIN_FROM]
    assert all(a > b for a, b in zip(sizes, sizes[1:]))
    assert E.trainer_workspace_bytes('resnet18', 8, True, True, train_from='layer3') < E.trainer_workspace_bytes('resnet18', 8, True, True)
    with pytest.raises(ValueError, match="'layer1', 'layer2', 'layer3', 'layer4'"):
        E.trainer_workspace_bytes('resnet18', 8, train_from='layer5')
    assert E.trainer_workspace_bytes('resnet18', 669, train_from='layer4') is None        # the 2 GiB refusals of create stay as they are
    free = E.trainer_workspace_bytes('resnet50', 40)
    for name in ('resnet18', 'resnet50'):
        plain = Fz.largest_fitting_frames(name, 300, free)
        part = Fz.largest_fitting_frames(name, 300, free, train_from='layer4')
        assert part >= plain and Fz.largest_fitting_frames(name, 300, free, train_from=None) == plain
    assert Fz.largest_fitting_frames('resnet50', 300, free) == 40 < Fz.largest_fitting_frames('resnet50', 300, free, train_from='layer4')


def test_keyword_validation():
    with pytest.raises(ValueError, match='train=True'):
        E.EmbeddingNet('resnet18', pretrained=False, train_from='layer3')
    for bad in ('layer0', 'layer5', 'conv1', 3, ''):
        with pytest.raises(ValueError, match="'layer1', 'layer2', 'layer3', 'layer4'"):
            E.EmbeddingNet('resnet18', pretrained=False, train=True, train_from=bad)
    with pytest.raises(NotImplementedError, match='resnet18'):
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, train_from='layer3')
    assert [E.train_stage(s) for s in (None,) + E.TRAIN_FROM] == [0, 1, 2, 3, 4]


def test_the_driver_flag():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_train_from is None
    f = make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--freeze_embedding_bn'])
    assert f.embedding_train_from == 'layer3'
    assert '--embedding_train_from' in make_parser().format_help()
    with pytest.raises(SystemExit):
        make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer5'])
    with pytest.raises(ValueError, match='--embedding_train_from layer4 needs --train_embedding'):
        Fz.run(make_parser().parse_args(['--embedding_train_from', 'layer4']))
    gb = 1 << 30
    base = dict(embedding_name='resnet18', unroll_length=10, batch_size=4, freeze_embedding_bn=True, embedding_chunk=None)
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (2 * gb, 256 * gb)):        # the guard and the default chunk use the flag
        plain, part = argparse.Namespace(**base), argparse.Namespace(embedding_train_from='layer4', **base)
        need = Fz.check_workspace_fits(part, 2)
        Fz.check_workspace_fits(plain, 2)
        assert part.embedding_chunk > plain.embedding_chunk                      # a partial run gets a larger chunk by itself
        assert need == E.trainer_workspace_bytes('resnet18', part.embedding_chunk, train_from='layer4') <= 2 * gb // 10 * 9
        whole = argparse.Namespace(embedding_train_from='layer3', **dict(base, freeze_embedding_bn=False, unroll_length=2, batch_size=2))
        assert Fz.check_workspace_fits(whole, 2) == E.trainer_workspace_bytes('resnet18', 8, train_from='layer3')


# ------------------------------------------------------------------------------------------------------------------
# the fused prefix op's references
# ------------------------------------------------------------------------------------------------------------------
def _run(geo, family, with_res, relu, mutant=None):
    d = tf.fused_inputs(family, geo)
    res = d['res'] if with_res else None
    args = (d['x'], d['wt'], d['gamma'], d['beta'], d['run_mean'], d['run_var'], res, relu, geo[5], geo[6])
    ref, bound = tf.fused_reference(*args)
    return tr.ratio(tf.fused_emulate(*args, mutant=mutant), ref, bound)


@pytest.mark.parametrize('geo', tr.CONV_GEOMETRIES + tf.EXTRA_GEOMETRIES, ids=str)
def test_the_emulation_passes_the_bound_and_every_mutant_exceeds_it(geo):
    worst = 0.0
    for family in tf.FAMILIES:
        for with_res in (False, True):
            for relu in (0, 1):
                worst = max(worst, _run(geo, family, with_res, relu))
    print('\n[fused prefix op, emulation %s] largest error / bound %.3f' % (geo, worst))
    assert worst <= 1.0, worst
    for mutant in tf.MUTANTS:
        families = ('large_mean',) if mutant == 'no_eps' else tf.FAMILIES      # (train_from_refs: what 'spread' can and cannot show)
        for family in families:
            r = _run(geo, family, True, 1, mutant)
            assert r > 1.0, (mutant, family, r)
