"""The prefix_cache mode on the GPU (pvr_op_gather_rows, pvr_trainer_prefix_forward; HipTrainableResNet.build_prefix_cache / forward_cached;
PolicyNetWithEncoder.build_prefix_cache, HipJointRMSprop.step_cached; --embedding_prefix_cache): inputs as tests/test_gpu_prefix_once.py - resnet18 with
3 - 6 frames, resnet50 with 2, 64 x 64 frames, frozen BatchNorm.

The oracle is equality of bits.  The gather moves bits and is compared with numpy's indexing.  The cache holds what the launches of a pass write before
its first trained op, and a cached pass reads that tensor from the staging buffer, so embeddings, every trained gradient and every updated parameter
equal those of the step on the frames themselves, with prefix_once and with neither mode."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
import train_from_refs as tf
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

LAYER = {1: 'layer1', 2: 'layer2', 3: 'layer3', 4: 'layer4'}
ARITHMETICS = {'fp32': {}, 'conv_split16': {'conv_split16': True}, 'both_split16': {'conv_split16': True, 'wgrad_split16': True}}
STEM = ('preprocess', 'normalize', 'conv1', 'bn1', 'maxpool')
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _gather(src, rows, n_src=None, dst=None):
    rows_dev = torch.as_tensor(rows, dtype=torch.int64).cuda()
    dst = torch.full((len(rows), src.shape[1]), 7.0, device='cuda') if dst is None else dst
    _lib.check(_lib.lib().pvr_op_gather_rows(vp(src), src.shape[0] if n_src is None else n_src, src.shape[1], vp(rows_dev), len(rows), vp(dst),
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dst


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# pvr_op_gather_rows
# ------------------------------------------------------------------------------------------------------------------
def _random_rows(n_src, row_floats, seed):
    """fp32 rows of random BITS (NaN payloads and denormals included): the gather moves bits, it does not compute"""
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src, row_floats), generator=torch.Generator().manual_seed(seed), dtype=torch.int64).to(torch.int32)
    return bits.view(torch.float32).cuda()


@pytest.mark.parametrize('n_src,row_floats,rows', [(7, 12, [6, 0, 0, 3]), (1, 4, [0]), (3, 200704, [2, 1]), (5, 4100, [4, 4, 1]),
                                                   (40, 50176, None)], ids=['7x12', '1x4', '3x200704', '5x4100', '334_of_40x50176'])
def test_gather_against_numpy_indexing(n_src, row_floats, rows):
    """pieces: 12 floats are 3 lanes of one piece, 200704 floats 49 full pieces, 4100 floats one full piece and a tail of one lane, 50176 floats 12 full
    pieces and a tail of 256 lanes; 334 rows of them are 4342 items for a grid of at most 8192 and repeat every source row"""
    if rows is None:
        rows = np.random.default_rng(5).integers(0, n_src, 334).tolist()
        assert len(set(rows)) == n_src
    src = _random_rows(n_src, row_floats, 3)
    dst = _gather(src, rows)
    assert np.array_equal(_bits(dst), _bits(src)[np.asarray(rows)])


def test_gather_walks_more_items_than_the_grid_has_workgroups():
    """9000 rows of one lane: 9000 items on 8192 workgroups, the last 808 walked in a second round"""
    src = _random_rows(64, 4, 9)
    rows = np.random.default_rng(2).integers(0, 64, 9000)
    assert np.array_equal(_bits(_gather(src, rows.tolist())), _bits(src)[rows])


def test_gather_out_of_range_rows_are_nan_and_nothing_else_moves():
    """the source is the middle of a larger tensor whose guard rows hold a sentinel: -1 and n_src_rows would read exactly those rows"""
    n_src, row_floats, sentinel = 4, 4100, 12345.0
    big = torch.full((n_src + 2, row_floats), sentinel, device='cuda')
    big[1:-1] = _random_rows(n_src, row_floats, 4).nan_to_num(0.0, 1.0, -1.0).clamp(-100, 100)       # finite, never the sentinel
    src = big[1:-1]
    rows = [0, -1, 2, n_src, 3, -1]
    out = torch.full((len(rows) + 2, row_floats), 7.0, device='cuda')                                # guard rows around the destination too
    _gather(src, rows, n_src=n_src, dst=out[1:-1])
    dst = out[1:-1].cpu()
    for i, r in enumerate(rows):
        if 0 <= r < n_src:
            assert torch.equal(dst[i], src[r].cpu()), i
        else:
            assert np.all(_bits(dst[i]) == 0x7fc00000), i       # quiet NaNs
    assert not bool((dst == sentinel).any())
    assert bool((out[0] == 7.0).all()) and bool((out[-1] == 7.0).all())


def test_gather_64_bit_offsets():
    """an uninitialised source of 2049 rows of 2^20 floats (8.004 GiB): row 512 begins at 2 GiB, row 1024 at 4 GiB = 2^30 floats, row 2048 at 2^31
    floats = 8 GiB.  A 32-bit offset in bytes or in floats would read another row, and the rows written here are the only ones with known contents"""
    free = torch.cuda.mem_get_info()[0]
    if free < 10 * 2 ** 30:
        pytest.skip('the 8 GiB source needs 10 GiB of free device memory, %.1f GiB are free' % (free / 2 ** 30))
    row_floats, picks = 2 ** 20, [0, 511, 512, 1024, 2048]
    src = torch.empty((2049, row_floats), dtype=torch.float32, device='cuda')
    ramp = torch.arange(row_floats, dtype=torch.float32, device='cuda')
    for r in picks:
        src[r] = ramp * (r + 1) + r                           # distinct in every element but a few
    rows = picks[::-1]
    dst = _gather(src, rows)
    for i, r in enumerate(rows):
        assert torch.equal(dst[i], ramp * (r + 1) + r), r
    del src, dst
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------
# pvr_trainer_prefix_forward
# ------------------------------------------------------------------------------------------------------------------
def _inputs(variant, n):
    key = ('inputs', variant, n)
    if key not in _cache:
        sd = synth.resnet50_state_dict(3, variant)
        frames = synth.smooth_frames(11, n, 64, 64)
        dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
        _cache[key] = (sd, frames, dout)
    return _cache[key]


def _model(sd, variant, max_batch, stage, **modes):
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=True, train_from=LAYER[stage], **modes)
    m.train()
    for p in m.trained_parameters():
        p.requires_grad = True
    return m


def _launches(m):
    L = _lib.lib()
    names, buf = [], C.create_string_buffer(128)
    while L.pvr_trainer_launch_time(m._handle, len(names), buf, 128, None, None):
        names.append(buf.value.decode())
    return names


def _in_prefix(name, stage):
    return name.split()[0] in STEM or any(name.startswith('layer%d.' % s) for s in range(1, stage))


@pytest.mark.parametrize('variant,stage,arithmetic,fused', [(v, s, a, f) for v, s in (('r18', 1), ('r18', 3), ('r18', 4), ('conv5', 2))
                                                            for a, f in (('fp32', True), ('conv_split16', True), ('conv_split16', False))])
def test_prefix_forward_writes_the_bits_of_forward_boundary(variant, stage, arithmetic, fused):
    L = _lib.lib()
    n = 3 if variant == 'r18' else 2
    sd, frames, dout = _inputs(variant, n)
    m = _model(sd, variant, n, stage, **dict(ARITHMETICS[arithmetic], **({'prefix_cache': True} if fused else {})))
    _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
    fr, dd = torch.from_numpy(frames).cuda(), dout.cuda()
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    out, whole, alone = nan(n, m.out_size), nan(n, m._boundary_floats), nan(n, m._boundary_floats)
    _lib.check(L.pvr_trainer_forward_boundary(m._handle, vp(m._flat), vp(m._bufs), vp(fr), n, 64, 64, vp(whole), 0, vp(out), out.stride(0), _lib.stream_ptr()))
    first = _launches(m)
    bufs = m._bufs.clone()
    _lib.check(L.pvr_trainer_prefix_forward(m._handle, vp(m._flat), vp(m._bufs), vp(fr), n, 64, 64, vp(alone), _lib.stream_ptr()))
    pre = _launches(m)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole).all()) and np.array_equal(_bits(alone), _bits(whole))
    assert torch.equal(m._bufs, bufs)                         # the running statistics are read, never written
    assert pre[:2] == ['preprocess', 'normalize'] and all(_in_prefix(x, stage) for x in pre), pre
    assert pre == [x for x in first if _in_prefix(x, stage)] == first[:len(pre)]       # exactly the launches before the first trained op
    assert any(x.endswith(' split16 bn frozen') for x in pre) == (fused and arithmetic == 'conv_split16' and stage > 1)
    # the forward that was held is dropped: a backward is a state error
    g = nan(m._flat.numel())
    assert L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()) == 4 and 'no forward' in _lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all())


# ------------------------------------------------------------------------------------------------------------------
# the autograd step: a cache of 6 frames, rows [3, 0, 3, 1, 4] in passes of 2, 2 and 1
# ------------------------------------------------------------------------------------------------------------------
ROWS = [3, 0, 3, 1, 4]


def _grads(m, out, dout):
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}


def _frames_step(stage, prefix_once, modes):
    sd, frames, dout = _inputs('r18', 6)
    m = _model(sd, 'r18', 2, stage, **dict(modes, **({'prefix_once': True} if prefix_once else {})))
    return _grads(m, m(torch.from_numpy(frames[ROWS]).cuda()), dout[:len(ROWS)])


def _cached_step(stage, modes):
    sd, frames, dout = _inputs('r18', 6)
    m = _model(sd, 'r18', 2, stage, prefix_cache=True, **modes)
    cache = m.build_prefix_cache(torch.from_numpy(frames).cuda())
    assert cache.n_frames == 6 and cache.nbytes == 6 * m.boundary_bytes() and cache.train_from == LAYER[stage] and cache.encoder is m
    assert cache.data.shape == (6, m._boundary_floats) and bool(torch.isfinite(cache.data).all()) and cache.fill_seconds > 0
    held = cache.data.clone()
    out = m.forward_cached(cache, torch.tensor(ROWS, device='cuda'))
    assert out.requires_grad and m._staging.shape == (2, m._boundary_floats)
    res = _grads(m, out, dout[:len(ROWS)])
    assert torch.equal(cache.data, held)                      # a step reads the cache and never writes it
    return res


@pytest.mark.parametrize('arithmetic', list(ARITHMETICS))
@pytest.mark.parametrize('stage', [1, 3])
def test_cached_autograd_step_keeps_the_bits_of_the_step_on_the_frames(stage, arithmetic):
    modes = ARITHMETICS[arithmetic]
    on = _cached_step(stage, modes)
    for prefix_once in (True, False):
        off = _frames_step(stage, prefix_once, modes)
        assert torch.equal(on[0], off[0]), ('embeddings', prefix_once)
        trained = [k for k in on[1] if tf.is_trained(k, stage)]
        assert trained and 'layer%d.0.conv1.weight' % stage in trained
        for k in on[1]:
            if k in trained:
                assert on[1][k] is not None and torch.equal(on[1][k], off[1][k]), (k, prefix_once)
            else:
                assert on[1][k] is None and off[1][k] is None, k


@pytest.mark.parametrize('arithmetic', ['fp32', 'conv_split16'])
def test_a_cached_pass_starts_at_the_first_trained_op(arithmetic):
    stage = 3
    sd, frames, dout = _inputs('r18', 6)
    m = _model(sd, 'r18', 2, stage, prefix_cache=True, **ARITHMETICS[arithmetic])
    cache = m.build_prefix_cache(torch.from_numpy(frames).cuda())
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
    fr = torch.from_numpy(frames[ROWS[-1:]]).cuda()
    out = torch.empty((1, m.out_size), device='cuda')
    m._forward_pass(fr, 0, 1, out)                             # the last pass on its frame, for the list of a whole pass
    whole = _launches(m)
    m._forward_raw_cached(cache, torch.tensor(ROWS, device='cuda'))
    again = _launches(m)                                      # the list of the last cached pass
    torch.cuda.synchronize()
    assert again and again[0].startswith('layer%d.0.conv1' % stage) and not any(_in_prefix(x, stage) for x in again), again[:4]
    assert again == [x for x in whole if not _in_prefix(x, stage)]


# ------------------------------------------------------------------------------------------------------------------
# the joint optimizer: T = 2, B = 2, F = 2 (8 frames in passes of 3, 3, 2) at stage 3, a dataset of 5 samples, a wrapping start index
# ------------------------------------------------------------------------------------------------------------------
def test_two_cached_joint_steps_give_the_parameters_of_two_steps_on_the_observations():
    from pvr_habitat_amd.bc_data import DeviceDataset
    T, B, F_, n = 2, 2, 2, 5
    obs = synth.smooth_frames(7, n * F_, 64, 64).reshape(n, F_, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 3 * F_)
    rng = np.random.default_rng(1)
    ds = DeviceDataset(np.ascontiguousarray(obs), rng.integers(0, R.A, n), np.eye(1, n, 2, dtype=bool)[0], 'cuda')
    starts = ([4, 1], [3, 0])                                 # sample 4 + 1 wraps to sample 0
    results = []
    for cached in (True, False):
        enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], 1)
        enc = _model(enc_sd, 'r18', 3, 3, **({'prefix_cache': True} if cached else {}))
        m = M.PolicyNetWithEncoder(enc, R.A, True, num_frames=F_, max_unroll=T, max_batch=B)
        m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
        m.train()
        opt = M.HipJointRMSprop(m, lr=1e-3)
        start = enc._flat.clone()
        if cached:
            cache = m.build_prefix_cache(ds.obs)
            assert cache is m.prefix_cache and cache.n_frames == n * F_
            one = enc._build_prefix_cache(1, [(0, torch.from_numpy(np.ascontiguousarray(obs[3, :, :, 3:6]))[None].cuda())])
            assert torch.equal(one.data[0], cache.data[3 * F_ + 1])                        # frame f of sample s is cache row s * F + f
        for s in starts:
            if cached:
                rows = ds.rows(s, T)
                assert rows.tolist() == [[s[0], s[1]], [(s[0] + 1) % n, (s[1] + 1) % n]]
                loss, norm = opt.step_cached(rows, ds.done[rows].bool(), ds.action[rows])
            else:
                o, a, d = ds.gather(s, T)
                loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and np.isfinite(float(norm)) and not torch.equal(enc._flat, start)
        assert torch.equal(enc._flat[:enc.trained_offset], start[:enc.trained_offset])    # the prefix has not moved: the cache stays valid
        results.append((enc._flat.clone(), m.policy._flat.clone(), opt.square_avg['embedding'].clone(), opt.square_avg['policy'].clone(),
                        float(loss), float(norm)))
        m.close()
    for a, b in zip(results[0][:4], results[1][:4]):
        assert torch.equal(a, b)
    assert results[0][4:] == results[1][4:]


# ------------------------------------------------------------------------------------------------------------------
# stale and foreign caches, the Python surface
# ------------------------------------------------------------------------------------------------------------------
def test_stale_and_foreign_caches_are_refused():
    sd, frames, dout = _inputs('r18', 3)
    fr = torch.from_numpy(frames).cuda()
    rows = torch.tensor([2, 0], device='cuda')
    m3, m4, other = _model(sd, 'r18', 2, 3, prefix_cache=True), _model(sd, 'r18', 2, 4, prefix_cache=True), _model(sd, 'r18', 2, 3, prefix_cache=True)
    c3, c4 = m3.build_prefix_cache(fr), m4.build_prefix_cache(fr)
    assert m3.forward_cached(c3, rows).shape == (2, 512)
    with pytest.raises(RuntimeError, match="another stage.*'layer4'.*'layer3'"):
        m3.forward_cached(c4, rows)
    with pytest.raises(RuntimeError, match='another encoder'):
        other.forward_cached(c3, rows)
    with pytest.raises(TypeError, match='PrefixCache'):
        m3.forward_cached(c3.data, rows)
    with pytest.raises(TypeError, match='int64'):
        m3.forward_cached(c3, rows.int())
    for p in m3.trained_parameters():                         # the trained parameters moving is the normal case
        p.data.mul_(1.01)
    m3.forward_cached(c3, rows)
    m3.load_state_dict(m3.state_dict())
    with pytest.raises(RuntimeError, match='stale prefix cache.*rebuild'):
        m3.forward_cached(c3, rows)
    fresh = m3.build_prefix_cache(fr)
    out = m3.forward_cached(fresh, rows)
    wrapper = torch.nn.Sequential(m3)                         # a parent module's load_state_dict reaches the encoder too
    wrapper.load_state_dict(wrapper.state_dict())
    with pytest.raises(RuntimeError, match='stale prefix cache'):
        out.sum().backward()                                  # the backward would gather from it again
    with pytest.raises(RuntimeError, match='stale prefix cache'):
        m3.forward_cached(fresh, rows)
    m3.eval()
    with pytest.raises(RuntimeError, match='training-mode'):
        m3.forward_cached(m3.build_prefix_cache(fr), rows)


def test_the_python_surface():
    sd, frames, _ = _inputs('r18', 3)
    fr = torch.from_numpy(frames).cuda()
    with pytest.raises(ValueError, match='no frozen prefix'):
        E.HipTrainableResNet(sd, 'r18', max_batch=2, freeze_bn=True).build_prefix_cache(fr)
    late = _model(sd, 'r18', 2, 3, conv_split16=True)           # the workspace exists without the fused prefix launches
    late(fr[:2])
    with pytest.raises(RuntimeError, match='before the first forward'):
        late.build_prefix_cache(fr)
    early = _model(sd, 'r18', 2, 3, conv_split16=True)          # before the first training forward the call switches them on itself
    cache = early.build_prefix_cache(fr)
    assert early.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 2, False, True, train_from='layer3', prefix_once=True)
    assert early.forward_cached(cache, torch.tensor([1], device='cuda')).shape == (1, 512)
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, freeze_bn=True, max_batch=4, train_from='layer3', conv_split16=True, prefix_cache=True,
                         prefix_once=True)
    enc = net.embedding
    assert enc.prefix_cache and not enc.prefix_once                                  # both: prefix_cache, no step-sized boundary tensor
    assert enc.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, False, True, train_from='layer3', prefix_once=True)
    out = net(fr)                                             # a forward on frames still works and allocates no boundary tensor
    assert out.shape == (3, 512) and out.requires_grad and enc._boundary is None
    net.close()


# ------------------------------------------------------------------------------------------------------------------
# the driver: two iterations against --embedding_prefix_once
# ------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n=40):
    frames = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(frames)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, save, mode, extra, T=3, B=2):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / save), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--freeze_embedding_bn', '--embedding_chunk', '5', '--embedding_name', 'resnet18',
                                     '--disable_pretrained_embedding', '--unroll_length', str(T), '--batch_size', str(B), '--eval_frequency', '1',
                                     '--max_frames', '12', '--embedding_train_from', 'layer4', '--embedding_conv_split16', mode] + extra)


@pytest.mark.parametrize('extra', [[], ['--autograd_step']], ids=['fused', 'autograd_step'])
def test_the_driver_gives_the_stats_of_prefix_once(tmp_path, capsys, extra):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    cached = Fz.run(_args(tmp_path, 'cache', '--embedding_prefix_cache', extra))['scene']
    printed = capsys.readouterr().out
    assert '--embedding_prefix_cache' in printed and 'prefix cache: 80 frames, ' in printed and 'frames/s' in printed
    once = Fz.run(_args(tmp_path, 'once', '--embedding_prefix_once', extra))['scene']
    assert cached['frames'] == once['frames'] == [0, 0, 6]
    assert all(np.isfinite(cached['training_loss'][1:])) and all(np.isfinite(cached['gradient_norm'][1:]))
    assert cached['training_loss'][1:] == once['training_loss'][1:] and cached['gradient_norm'][1:] == once['gradient_norm'][1:]
    ck = torch.load(tmp_path / 'cache' / 'scene_emresnet18_finetuned_s1_scene.tar', weights_only=False)
    assert ck['flags']['embedding_prefix_cache'] is True and ck['flags']['embedding_train_from'] == 'layer4'
