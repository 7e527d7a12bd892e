"""Frozen BatchNorm where no GPU is needed: the fp32 emulation of tests/frozen_bn_refs.py passes every bound and every mutant exceeds one (so the
bounds the GPU kernels are held to can tell the classic mistakes apart), the C surface (symbols, argument counts, state errors, refused shapes), the
two driver flags and the driver's chunk guard."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch

import frozen_bn_refs as fr
import train_refs as tr
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

CPU_SHAPES = fr.SHAPES[:2]
MODES = [(False, False), (False, True), (True, False), (True, True)]          # (with_res, relu)


def _forward_ratios(d, with_res, relu, mutant=None):
    res = d['res'] if with_res else None
    ref, bound = fr.forward_ref(d['z'], res, d['gamma'], d['beta'], d['run_mean'], d['run_var'], relu)
    got = fr.forward(d['z'], res, d['gamma'], d['beta'], d['run_mean'], d['run_var'], relu, mutant)
    return {k: tr.ratio(got[k], ref[k], bound[k]) for k in ref}


def _backward_ratios(d, with_res, relu, accumulate, mutant=None):
    res = d['res'] if with_res else None
    fwd = fr.forward(d['z'], res, d['gamma'], d['beta'], d['run_mean'], d['run_var'], relu)
    prev = d['prev'] if accumulate else None
    ref, bound = fr.backward_ref(d['z'], fwd['y'], d['dy'], d['gamma'], fwd['mean'], fwd['rstd'], relu, prev)
    got = fr.backward(d['z'], fwd['y'], d['dy'], d['gamma'], fwd['mean'], fwd['rstd'], relu, prev, res=res, mutant=mutant)
    return {k: tr.ratio(got[k], ref[k], bound[k]) for k in ref}


@pytest.mark.parametrize('rows,C_', CPU_SHAPES)
@pytest.mark.parametrize('family', fr.FAMILIES)
def test_the_fp32_emulation_passes_every_bound(family, rows, C_):
    d = tr.bn_inputs(family, rows, C_)
    for with_res, relu in MODES:
        worst = _forward_ratios(d, with_res, relu)
        assert max(worst.values()) <= 1.0, ('forward', with_res, relu, worst)
        for accumulate in (False, True):
            worst = _backward_ratios(d, with_res, relu, accumulate)
            assert max(worst.values()) <= 1.0, ('backward', with_res, relu, accumulate, worst)


@pytest.mark.parametrize('rows,C_', CPU_SHAPES)
@pytest.mark.parametrize('family', fr.FAMILIES)
@pytest.mark.parametrize('mutant', fr.FORWARD_MUTANTS)
def test_every_forward_mutant_exceeds_a_bound(mutant, family, rows, C_):
    worst = _forward_ratios(tr.bn_inputs(family, rows, C_), True, True, mutant)
    key = {'batch_statistics': 'y', 'running_updated': 'run_mean', 'no_eps': 'rstd'}[mutant]
    assert worst[key] > 1.0, worst
    if mutant == 'no_eps':
        assert worst['y'] > 1.0, worst
    if mutant == 'running_updated':
        assert worst['run_var'] > 1.0 and worst['y'] <= 1.0, worst


@pytest.mark.parametrize('rows,C_', CPU_SHAPES)
@pytest.mark.parametrize('family', fr.FAMILIES)
@pytest.mark.parametrize('mutant', fr.BACKWARD_MUTANTS)
def test_every_backward_mutant_exceeds_a_bound(mutant, family, rows, C_):
    worst = _backward_ratios(tr.bn_inputs(family, rows, C_), True, True, True, mutant)
    assert worst['dz'] > 1.0, worst
    if mutant == 'mask_pre_residual':
        assert worst['dres'] > 1.0 and worst['dbeta'] > 1.0, worst
    else:                                           # the mean terms touch dz only
        assert max(worst['dres'], worst['dgamma'], worst['dbeta']) <= 1.0, worst


def test_the_frozen_and_the_batch_statistics_reference_differ_by_order_one():
    d = tr.bn_inputs('spread', 98, 64)
    a = fr.forward(d['z'].double(), None, d['gamma'].double(), d['beta'].double(), d['run_mean'].double(), d['run_var'].double(), False)['y']
    b = tr.bn_forward(d['z'].double(), None, d['gamma'].double(), d['beta'].double(), d['run_mean'].double(), d['run_var'].double(), False)['y']
    assert tr.rel_l2(a, b) > 0.1


# ------------------------------------------------------------------------------------------------------------------
# the C surface
# ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {'pvr_trainer_set_bn_frozen': 2, 'pvr_trainer_backward_acc': 9, 'pvr_op_bn_frozen_forward': 13, 'pvr_op_bn_frozen_backward': 17}


def test_exported_symbols_and_declared_argument_counts():
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pvr_train.h')).read()
    for name, count in NEW_SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_lib._SIGS[name][1]) == count, name
        decl = re.search(r'pvr_status\s+%s\(([^)]*)\);' % name, header)
        assert decl is not None, name
        assert len(decl.group(1).split(',')) == count, (name, decl.group(1))


def _create(arch=10, max_batch=4):
    d = _lib.EncoderDesc(arch=arch, dtype=_lib.PVR_F32, max_batch=max_batch, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    return h


def test_the_mode_switch_and_the_accumulating_backward_on_a_fresh_handle():
    L = _lib.lib()
    h = _create()
    try:
        before = L.pvr_trainer_workspace_bytes(h)
        assert L.pvr_trainer_set_bn_frozen(h, 1) == 0
        assert L.pvr_trainer_workspace_bytes(h) == before          # the accumulation scratch is the caller's: the workspace does not move
        one = (C.c_float * 4)()
        for accumulate in (0, 1):
            assert L.pvr_trainer_backward_acc(h, one, one, 512, one, accumulate, one, 4, None) == 4      # PVR_ERR_STATE, before anything touches the device
            assert 'forward' in _lib.last_error()
        assert L.pvr_trainer_backward(h, one, one, 512, one, None) == 4
        assert L.pvr_trainer_set_bn_frozen(h, 0) == 0
        assert L.pvr_trainer_set_bn_frozen(None, 1) == 1
    finally:
        L.pvr_trainer_destroy(h)


def test_unit_entry_points_refuse_unsupported_shapes():
    L = _lib.lib()
    one = (C.c_float * 1)()
    p = C.cast(one, C.c_void_p)
    assert L.pvr_op_bn_frozen_forward(p, None, p, p, p, p, p, p, p, 8, 30, 0, None) == 1 and 'c % 4' in _lib.last_error()
    assert L.pvr_op_bn_frozen_backward(p, p, p, p, p, p, p, None, 0, p, p, 8, 30, 1, p, 1 << 20, None) == 1 and 'c % 4' in _lib.last_error()
    assert L.pvr_op_bn_frozen_forward(p, None, p, p, p, p, p, p, p, 0, 64, 0, None) == 1 and 'rows' in _lib.last_error()
    assert L.pvr_op_bn_frozen_backward(p, p, p, p, p, p, p, None, 0, p, p, 8, 64, 1, p, 16, None) == 1 and 'scratch' in _lib.last_error()
    assert L.pvr_op_bn_frozen_forward(p, None, p, p, None, p, p, p, p, 8, 64, 0, None) == 1 and 'null' in _lib.last_error()


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
def test_the_parser_accepts_the_two_flags():
    from pvr_habitat_amd.arguments import make_parser
    f = make_parser().parse_args([])
    assert f.freeze_embedding_bn is False and f.embedding_chunk is None
    f = make_parser().parse_args(['--train_embedding', '--freeze_embedding_bn', '--embedding_chunk', '320'])
    assert f.freeze_embedding_bn is True and f.embedding_chunk == 320
    text = make_parser().format_help()
    assert '--freeze_embedding_bn' in text and '--embedding_chunk' in text


def _flags(**kw):
    base = dict(embedding_name='resnet18', unroll_length=10, batch_size=4, freeze_embedding_bn=True, embedding_chunk=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_the_guard_in_frozen_mode_names_a_chunk_that_fits(monkeypatch):
    from pvr_habitat_amd import main_bc_finetune as Fz
    gb = 1 << 30
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **k: (gb, 256 * gb))
    with pytest.raises(RuntimeError, match='largest --embedding_chunk that fits is') as e:
        Fz.check_workspace_fits(_flags(embedding_chunk=80), 2)                       # 80 frames of resnet18: about 2.4 GB
    fit = int(str(e.value).split('that fits is ')[1].split()[0])
    assert 0 < fit < 80
    assert E.trainer_workspace_bytes('resnet18', fit) <= gb < E.trainer_workspace_bytes('resnet18', fit + 1)
    # a chunk that fits passes, whatever unroll_length x batch_size x frames is, and is never above it
    f = _flags(embedding_chunk=fit, unroll_length=100, batch_size=16)
    assert Fz.check_workspace_fits(f, 2) == E.trainer_workspace_bytes('resnet18', fit) and f.embedding_chunk == fit
    f = _flags(embedding_chunk=fit, unroll_length=1, batch_size=2)
    Fz.check_workspace_fits(f, 2)
    assert f.embedding_chunk == 4
    # the default: the largest chunk whose workspace fits nine tenths of the free memory
    f = _flags(unroll_length=100, batch_size=16)
    need = Fz.check_workspace_fits(f, 2)
    assert 0 < f.embedding_chunk <= fit and need == E.trainer_workspace_bytes('resnet18', f.embedding_chunk) <= gb // 10 * 9
    assert E.trainer_workspace_bytes('resnet18', f.embedding_chunk + 1) > gb // 10 * 9


def test_the_guard_in_frozen_mode_keeps_the_trainers_own_limit(monkeypatch):
    from pvr_habitat_amd import main_bc_finetune as Fz
    gb = 1 << 30
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **k: (1024 * gb, 1024 * gb))
    with pytest.raises(RuntimeError, match='largest --embedding_chunk that fits is 668'):
        Fz.check_workspace_fits(_flags(embedding_chunk=700, unroll_length=100, batch_size=16), 2)
    f = _flags(unroll_length=100, batch_size=16)
    Fz.check_workspace_fits(f, 2)
    assert f.embedding_chunk == 668
    # without the flag the guard is the batch-statistics one, message and all
    with pytest.raises(RuntimeError, match='largest unroll_length x batch_size x frames that fits is 668'):
        Fz.check_workspace_fits(_flags(freeze_embedding_bn=False, unroll_length=100, batch_size=16), 2)


def test_freeze_bn_belongs_to_the_trainable_encoder():
    with pytest.raises(ValueError, match='train=True'):
        E.EmbeddingNet('resnet18', pretrained=False, train=False, freeze_bn=True, disable_cuda=True)
