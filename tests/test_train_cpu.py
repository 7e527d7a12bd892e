"""The trainable encoder's surface where no GPU is needed: what pvr_trainer_create accepts and refuses, the layout of the flat parameter and
BatchNorm-buffer blocks against the state_dict, and what EmbeddingNet(..., train=True) keeps refusing."""
import ctypes as C

import numpy as np
import pytest

from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E

ARCH = {'conv5': 0, 'r18': 10, 'r34': 11}


def _create(arch, dtype=_lib.PVR_F32, max_batch=4):
    d = _lib.EncoderDesc(arch=arch, dtype=dtype, max_batch=max_batch, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    return _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)), h


@pytest.mark.parametrize('variant', ['conv5', 'r18', 'r34'])
def test_create_and_flat_layout_match_the_state_dict(variant):
    L = _lib.lib()
    status, h = _create(ARCH[variant])
    assert status == 0, _lib.last_error()
    try:
        assert L.pvr_trainer_out_size(h) == E.OUT_SIZE[variant]
        sd = synth.resnet50_state_dict(3, variant)
        assert set(sd) == set(synth.resnet50_state_dict(3, variant, keys_only=True))
        params = {k: v for k, v in sd.items() if not k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))}
        assert L.pvr_trainer_param_count(h) == sum(int(np.prod(v.shape)) for v in params.values())
        numel, shape, spans = C.c_int64(), (C.c_int64 * 4)(), []
        for k, v in params.items():
            o = L.pvr_trainer_param_offset(h, k.encode(), C.byref(numel), shape)
            assert o >= 0, k
            assert tuple(x for x in shape if x > 0) == tuple(v.shape) and numel.value == v.size, k
            spans.append((o, o + numel.value))
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == L.pvr_trainer_param_count(h)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), 'parameters overlap or leave holes'
        names, buf, i = [], C.create_string_buffer(128), 0
        while L.pvr_trainer_param_name(h, i, buf, 128) > 0:
            names.append(buf.value.decode())
            i += 1
        assert set(names) == set(params)
        assert L.pvr_trainer_param_offset(h, b'fc.weight', None, None) == -1
        # BatchNorm buffers: fp32 statistics, then 8-byte aligned int64 counters
        bspans = []
        for k, v in sd.items():
            if k.endswith(('running_mean', 'running_var')):
                o = L.pvr_trainer_buffer_offset(h, k.encode(), C.byref(numel))
                assert o >= 0 and numel.value == v.size, k
                bspans.append((o, o + numel.value))
            elif k.endswith('num_batches_tracked'):
                o = L.pvr_trainer_buffer_offset(h, k.encode(), C.byref(numel))
                assert o >= 0 and o % 2 == 0 and numel.value == 1, k
                bspans.append((o, o + 2))
        bspans.sort()
        assert bspans[0][0] == 0 and bspans[-1][1] == L.pvr_trainer_buffer_count(h)
        assert all(a[1] <= b[0] for a, b in zip(bspans, bspans[1:]))
    finally:
        L.pvr_trainer_destroy(h)


@pytest.mark.parametrize('arch,what', [(1, '_l4'), (2, '_l3'), (3, 'CLIP ViT'), (5, 'MAE ViT'), (6, 'random'), (9, 'CLIP RN50')])
def test_create_refuses_other_architectures(arch, what):
    status, _ = _create(arch)
    assert status == 1, what
    assert 'resnet18' in _lib.last_error() and 'not trainable' in _lib.last_error()


def test_create_refuses_another_crop():
    d = _lib.EncoderDesc(arch=10, dtype=_lib.PVR_F32, max_batch=4, chunk=0, resize=256, crop=192)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)) == 1
    assert '224' in _lib.last_error()


@pytest.mark.parametrize('dtype', [_lib.PVR_BF16, _lib.PVR_F16, _lib.PVR_F32S])
def test_create_refuses_other_dtypes(dtype):
    status, _ = _create(0, dtype)
    assert status == 1
    assert 'PVR_F32' in _lib.last_error()


def test_a_backward_without_a_forward_is_a_state_error():
    status, h = _create(10)
    assert status == 0
    try:
        one = (C.c_float * 1)()
        assert _lib.lib().pvr_trainer_backward(h, one, one, 512, one, None) == 4      # PVR_ERR_STATE, before anything touches the device
        assert 'forward' in _lib.last_error()
    finally:
        _lib.lib().pvr_trainer_destroy(h)


def test_kernel_entry_points_refuse_unsupported_shapes():
    L = _lib.lib()
    one = (C.c_float * 1)()
    p = C.cast(one, C.c_void_p)
    assert L.pvr_op_conv_dgrad_scratch_floats(2, 7, 7, 64, 64, 3, 2, 1) == 0
    assert L.pvr_op_conv_dgrad(p, p, p, 0, 2, 7, 7, 64, 64, 3, 2, 1, p, 1 << 30, None) == 1 and 'odd' in _lib.last_error()
    assert L.pvr_op_conv_wgrad(p, p, p, 2, 8, 8, 48, 64, 3, 1, 1, p, 1 << 30, None) == 1 and 'cin' in _lib.last_error()
    assert L.pvr_op_conv_wgrad(p, p, p, 2, 8, 8, 64, 64, 5, 1, 2, p, 1 << 30, None) == 1
    assert L.pvr_op_conv_wgrad(p, p, p, 2, 8, 8, 64, 64, 3, 1, 1, p, 16, None) == 1 and 'scratch' in _lib.last_error()
    assert L.pvr_op_bn_train_forward(p, None, p, p, None, None, None, p, p, p, 1, 64, 0, p, 1 << 20, None) == 1 and 'rows' in _lib.last_error()
    assert L.pvr_op_stem_wgrad(p, p, p, 2, 33, p, 1 << 30, None) == 1
    assert L.pvr_op_bn_scratch_floats(6272, 64) == (4 + 1) * 2 * 64


@pytest.mark.parametrize('name', ['resnet50_l3', 'moco_aug_l4', 'clip_vit', 'moco_aug_uber_345', 'mae_base', 'random'])
def test_embeddingnet_train_keeps_refusing_what_is_not_trainable(name):
    with pytest.raises(NotImplementedError, match='resnet18'):
        E.EmbeddingNet(name, pretrained=False, train=True)


def test_embeddingnet_train_refusals():
    with pytest.raises(NotImplementedError, match='host backend'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, disable_cuda=True)
    with pytest.raises(ValueError, match='fp32'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, compute_dtype='f16')
    with pytest.raises(NotImplementedError, match='Requested model not available'):
        E.EmbeddingNet('nonexistent', train=True)
    with pytest.raises(NotImplementedError, match='5-crop'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, crops=5)


def test_save_embedded_obs_refuses_train_embedding(tmp_path):
    import argparse
    from pvr_habitat_amd import save_embedded_obs
    flags = argparse.Namespace(train_embedding=True, embedding_name='resnet18', data_path=str(tmp_path), env='nowhere', run_id=0, disable_cuda=True,
                               source='pickle', pretrained_embedding=False)
    with pytest.raises(NotImplementedError, match='frozen encoder'):
        save_embedded_obs.run(flags)
    (tmp_path / 'nowhere.pickle').write_bytes(b'not a scene')        # refused before the scene is opened: no index job is left behind
    with pytest.raises(NotImplementedError, match='frozen encoder'):
        save_embedded_obs.run(flags)
