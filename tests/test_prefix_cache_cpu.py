"""The prefix_cache mode (pvr_trainer_prefix_forward, pvr_op_gather_rows; HipTrainableResNet.build_prefix_cache / forward_cached,
EmbeddingNet(..., train=True, train_from=..., prefix_cache=True); DeviceDataset.rows; --embedding_prefix_cache) without a GPU: the new symbols, keyword
and flag validation, the byte arithmetic, the order of the cache's rows, every refusal of the two entry points that launches nothing, and the driver's
memory check."""
import argparse
import ctypes as C
import unittest.mock as mock

import numpy as np
import pytest
import torch

from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E

ARCH = {'resnet18': 10, 'resnet50': 0}
PVR_ERR_INVALID, PVR_ERR_STATE = 1, 4


def _create(name, max_batch=8):
    d = _lib.EncoderDesc(arch=ARCH[name], dtype=_lib.PVR_F32, max_batch=max_batch, chunk=0, resize=256, crop=224)
    d.mean[:] = E.IMAGENET_MEAN
    d.std_[:] = E.IMAGENET_STD
    h = C.c_void_p()
    assert _lib.lib().pvr_trainer_create(C.byref(d), C.byref(h)) == 0, _lib.last_error()
    return h


def test_the_symbols_are_exported():
    L = _lib.lib()
    for s in ('pvr_trainer_prefix_forward', 'pvr_op_gather_rows'):
        assert hasattr(L, s) and s in _lib._SIGS, s


# ------------------------------------------------------------------------------------------------------------------
# keywords, flag, parser help
# ------------------------------------------------------------------------------------------------------------------
def test_keyword_validation():
    with pytest.raises(ValueError, match='prefix_cache needs train_from.*no frozen prefix'):
        E.EmbeddingNet('resnet18', pretrained=False, train=True, prefix_cache=True)
    with pytest.raises(ValueError, match='prefix_cache is a mode of the trainable encoder .train=True'):
        E.EmbeddingNet('resnet18', pretrained=False, train_from=None, prefix_cache=True)
    with pytest.raises(ValueError, match='train=True'):
        E.EmbeddingNet('resnet18', pretrained=False, train_from='layer3', prefix_cache=True)
    with pytest.raises(NotImplementedError, match='resnet18'):
        E.EmbeddingNet('clip_vit', pretrained=False, train=True, train_from='layer3', prefix_cache=True)
    with pytest.raises(ValueError, match='no frozen prefix'):
        E.check_prefix_cache(True, None)
    E.check_prefix_cache(True, 'layer2')
    E.check_prefix_cache(False, None)


def test_the_driver_flag_and_the_parser_help():
    from pvr_habitat_amd.arguments import make_parser
    from pvr_habitat_amd import main_bc_finetune as Fz
    assert make_parser().parse_args([]).embedding_prefix_cache is False
    f = make_parser().parse_args(['--train_embedding', '--embedding_train_from', 'layer3', '--freeze_embedding_bn', '--embedding_prefix_cache'])
    assert f.embedding_prefix_cache is True and f.embedding_prefix_once is False
    assert Fz.workspace_modes(f) == {'train_from': 'layer3', 'prefix_once': True}          # the workspace mode is prefix_once's: the fused prefix launches
    assert Fz.boundary_cache_bytes(f, 3200) == 0                                       # no step-sized cache, with or without --embedding_prefix_once
    f.embedding_prefix_once = True
    assert Fz.boundary_cache_bytes(f, 3200) == 0
    text = ' '.join(make_parser().format_help().split())
    assert '--embedding_prefix_cache' in text and 'once per DATASET frame' in text and 'rebuilt' in text
    with pytest.raises(ValueError, match='--embedding_prefix_cache needs --embedding_train_from.*no frozen prefix'):
        Fz.run(make_parser().parse_args(['--train_embedding', '--embedding_prefix_cache']))
    with pytest.raises(ValueError, match='--embedding_prefix_cache needs --embedding_train_from'):
        Fz.check_prefix_cache_flag(argparse.Namespace(embedding_prefix_cache=True))


# ------------------------------------------------------------------------------------------------------------------
# byte arithmetic
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ARCH))
def test_prefix_cache_bytes(name):
    for stage in range(1, 5):
        layer = 'layer%d' % stage
        for n in (1, 7, 8000):
            assert E.trainer_prefix_cache_bytes(name, layer, n) == n * E.trainer_boundary_bytes(name, layer) > 0
    assert E.trainer_prefix_cache_bytes('resnet50', 'layer2', 1) == 4 * 56 * 56 * 256
    assert E.trainer_prefix_cache_bytes('resnet18', 'layer4', 8000) == 8000 * 4 * 14 * 14 * 256
    with pytest.raises(ValueError, match='no frozen prefix'):
        E.trainer_prefix_cache_bytes(name, None, 10)


# ------------------------------------------------------------------------------------------------------------------
# row order
# ------------------------------------------------------------------------------------------------------------------
def test_dataset_rows_on_the_host_backend():
    from pvr_habitat_amd.bc_data import DeviceDataset
    n, T = 7, 4
    obs = np.arange(n * 16, dtype=np.uint8).reshape(n, 16)
    ds = DeviceDataset(obs, np.arange(n), np.zeros(n, bool), device='cpu')
    starts = [0, 5, 6, 3]                                      # 5 and 6 wrap
    rows = ds.rows(starts, T)
    want = np.stack([np.mod(np.arange(i, i + T), n) for i in starts], axis=1)
    assert rows.dtype == torch.int64 and rows.shape == (T, len(starts)) and rows.device.type == 'cpu'
    assert np.array_equal(rows.numpy(), want) and want.max() == n - 1 and want[3, 2] == 2
    o, a, _ = ds.gather(starts, T)                             # the index arithmetic of gather
    assert torch.equal(o, ds.obs[rows]) and torch.equal(a, ds.action[rows])
    for bad in ([-1], [n], [0, n + 3]):
        with pytest.raises(IndexError, match='start index'):
            ds.rows(bad, T)
    with pytest.raises(ValueError, match='at least one'):
        ds.rows([], T)
    with pytest.raises(ValueError, match='at least one'):
        ds.rows([0], 0)


def test_the_row_map_is_the_order_of_split_frames():
    """frame f of sample s is cache row s * F + f: split_frames of the whole dataset, taken as one (1, n) batch, puts it there, and cache_rows of (T, B)
    sample indices names the frames split_frames gives for the gathered observations"""
    from pvr_habitat_amd.models import PolicyNetWithEncoder
    n, F, H, W = 5, 3, 2, 2
    m = argparse.Namespace(num_frames=F, device=torch.device('cpu'))
    obs = torch.arange(n * H * W * 3 * F, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(n, H, W, 3 * F)
    frames = PolicyNetWithEncoder.split_frames(m, obs.unsqueeze(0))                     # the cache's frame order
    assert frames.shape == (n * F, H, W, 3)
    for s in range(n):
        for f in range(F):
            assert torch.equal(frames[s * F + f], obs[s, :, :, 3 * f:3 * f + 3]), (s, f)
    rows = torch.tensor([[3, 0], [4, 1], [0, 2]])                                        # (T, B) sample indices, a wrap in column 0
    idx = PolicyNetWithEncoder.cache_rows(m, rows)
    assert idx.dtype == torch.int64 and idx.tolist() == [s * F + f for s in rows.reshape(-1).tolist() for f in range(F)]
    assert torch.equal(frames[idx], PolicyNetWithEncoder.split_frames(m, obs[rows]))


# ------------------------------------------------------------------------------------------------------------------
# library refusals that launch nothing
# ------------------------------------------------------------------------------------------------------------------
def test_gather_rows_refusals():
    L = _lib.lib()
    p = lambda a: C.c_void_p(a)                                  # (never dereferenced: the refusal comes first)
    ok = dict(src=p(256), n_src=3, row=8, rows=p(512), n=2, dst=p(1024))
    call = lambda **k: L.pvr_op_gather_rows(*[dict(ok, **k)[x] for x in ('src', 'n_src', 'row', 'rows', 'n', 'dst')], None)
    for change, word in ((dict(src=None), 'null argument'), (dict(rows=None), 'null argument'), (dict(dst=None), 'null argument'),
                         (dict(n=0), 'n = 0'), (dict(n=-2), 'n = -2'), (dict(n_src=0), 'n_src_rows = 0'), (dict(row=0), 'row_floats 0'),
                         (dict(row=3), 'row_floats 3'), (dict(row=6), 'row_floats 6'), (dict(row=-4), 'row_floats -4'),
                         (dict(src=p(260)), '16-byte aligned'), (dict(dst=p(1032)), '16-byte aligned'), (dict(rows=p(516)), '8-byte aligned')):
        assert call(**change) == PVR_ERR_INVALID, change
        assert 'pvr_op_gather_rows' in _lib.last_error() and word in _lib.last_error(), (change, _lib.last_error())


def test_prefix_forward_refusals():
    L = _lib.lib()
    h = _create('resnet18', max_batch=4)
    try:
        one = C.c_void_p(16)
        call = lambda params=one, bufs=one, frames=one, n=1, boundary=one: L.pvr_trainer_prefix_forward(h, params, bufs, frames, n, 64, 64, boundary, None)
        assert L.pvr_trainer_prefix_forward(None, one, one, one, 1, 64, 64, one, None) == PVR_ERR_INVALID and 'null argument' in _lib.last_error()
        assert call() == PVR_ERR_STATE                          # stage 0: there is no prefix
        assert 'pvr_trainer_prefix_forward' in _lib.last_error() and 'no frozen prefix' in _lib.last_error()
        assert L.pvr_trainer_set_train_from(h, 3) == 0
        for kw, word in ((dict(params=None), 'null argument'), (dict(bufs=None), 'null argument'), (dict(frames=None), 'null argument'),
                         (dict(boundary=None), 'null argument'), (dict(boundary=C.c_void_p(20)), 'not 16-byte aligned'),
                         (dict(n=0), 'max_batch = 4'), (dict(n=5), 'max_batch = 4'), (dict(n=-1), 'max_batch = 4')):
            assert call(**kw) == PVR_ERR_INVALID, kw
            assert 'pvr_trainer_prefix_forward' in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
        # nothing was launched and nothing is held: a backward is a state error
        assert L.pvr_trainer_backward(h, one, one, 512, one, None) == PVR_ERR_STATE and 'no forward' in _lib.last_error()
    finally:
        L.pvr_trainer_destroy(h)


# ------------------------------------------------------------------------------------------------------------------
# the driver's memory check
# ------------------------------------------------------------------------------------------------------------------
def test_the_driver_memory_check_counts_the_cache():
    from pvr_habitat_amd import main_bc_finetune as Fz
    gb = 1 << 30
    base = dict(embedding_name='resnet50', unroll_length=100, batch_size=16, freeze_embedding_bn=True, embedding_chunk=None, embedding_train_from='layer4',
                embedding_prefix_cache=True)
    n_samples, F = 4000, 2
    bb = E.trainer_boundary_bytes('resnet50', 'layer4')
    cache = E.trainer_prefix_cache_bytes('resnet50', 'layer4', n_samples * F)
    assert cache == n_samples * F * bb == 8000 * 4 * 14 * 14 * 1024
    assert Fz.prefix_cache_bytes(argparse.Namespace(**base), n_samples * F) == (cache, bb)
    assert Fz.prefix_cache_bytes(argparse.Namespace(**dict(base, embedding_prefix_cache=False)), n_samples * F) == (0, 0)
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (64 * gb, 256 * gb)):      # it fits: cache + staging + the chunk's workspace
        on, off = argparse.Namespace(**base), argparse.Namespace(**dict(base, embedding_prefix_cache=False))
        need_on, need_off = Fz.check_workspace_fits(on, F, n_samples), Fz.check_workspace_fits(off, F, n_samples)
        assert 1 <= on.embedding_chunk <= off.embedding_chunk
        ws = E.trainer_workspace_bytes('resnet50', on.embedding_chunk, train_from='layer4', prefix_once=True)
        assert need_on == ws + cache + on.embedding_chunk * bb <= 64 * gb // 10 * 9
        assert need_off == E.trainer_workspace_bytes('resnet50', off.embedding_chunk, train_from='layer4')
        whole = argparse.Namespace(**dict(base, freeze_embedding_bn=False, unroll_length=2, batch_size=2))       # one pass: the staging holds the step
        assert Fz.check_workspace_fits(whole, F, 10) == E.trainer_workspace_bytes('resnet50', 8, train_from='layer4', prefix_once=True) + (10 * F + 8) * bb
    with mock.patch.object(torch.cuda, 'mem_get_info', lambda *a, **k: (4 * gb, 256 * gb)):       # 5.98 GB of cache do not fit 4 GB
        for flags in (argparse.Namespace(**base), argparse.Namespace(**dict(base, embedding_chunk=8)),
                      argparse.Namespace(**dict(base, freeze_embedding_bn=False, unroll_length=2, batch_size=2))):
            with pytest.raises(RuntimeError) as e:
                Fz.check_workspace_fits(flags, F, n_samples)
            msg = str(e.value)
            assert '--embedding_prefix_cache' in msg and '8000 dataset frames takes %.2f GB' % (cache / gb) in msg and 'staging tensor of' in msg
            assert 'training workspace of' in msg and '4.00 GB of device memory are free' in msg
            assert 'higher stage' in msg and '--embedding_prefix_once' in msg
