"""The prefix_once mode on the GPU (pvr_trainer_forward_boundary, pvr_trainer_set_prefix_fused; HipTrainableResNet / EmbeddingNet(..., train_from=...,
prefix_once=True); --embedding_prefix_once): inputs as tests/test_gpu_train_from.py - resnet18 with 3 frames, resnet50 with 2, 64 x 64 frames, frozen
BatchNorm.

The oracle is equality of bits with the mode off: the boundary tensor a trained op reads is the same tensor whether it lives in the workspace or in the
caller's cache, whether this pass computed it or an earlier one did, and whether a split prefix op ran as three launches or as one.  A chunked step is
also held to torch's float64 recipe (tests/train_from_refs.py) within that file's 8 x d_t32 criterion, and the launch lists of the passes are read
through pvr_trainer_debug_set_timing."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
import train_from_refs as tf
import train_refs as tr
from oracle import encoder_oracle as eo
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

CASES = {'r18': 3, 'conv5': 2}          # variant -> frames
STATS = ('running_mean', 'running_var', 'num_batches_tracked')
LAYER = {1: 'layer1', 2: 'layer2', 3: 'layer3', 4: 'layer4'}
ARITHMETICS = {'fp32': {}, 'conv_split16': {'conv_split16': True}, 'both_split16': {'conv_split16': True, 'wgrad_split16': True}}
STEM = ('preprocess', 'normalize', 'conv1', 'bn1', 'maxpool')
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(variant, n):
    key = ('inputs', variant, n)
    if key not in _cache:
        sd = synth.resnet50_state_dict(3, variant)
        frames = synth.smooth_frames(11, n, 64, 64)
        dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
        _cache[key] = (sd, frames, dout)
    return _cache[key]


def _model(sd, variant, max_batch, stage, prefix_once, **modes):
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=True, train_from=LAYER[stage], **dict(modes, **({'prefix_once': True} if prefix_once else {})))
    m.train()
    for p in m.trained_parameters():
        p.requires_grad = True
    return m


def _lib_step(variant, n, max_batch, stage, prefix_once, **modes):
    """one autograd step -> (embeddings, {parameter: grad or None}, {buffer: value})"""
    sd, frames, dout = _inputs(variant, n)
    m = _model(sd, variant, max_batch, stage, prefix_once, **modes)
    out = m(torch.from_numpy(frames).cuda())
    assert m._boundary is None                        # the cache lives on the autograd node, as the kept frames do
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.endswith(STATS)}
    return out.detach().cpu(), grads, bufs


def _equal_steps(on, off, sd, stage):
    assert torch.equal(on[0], off[0]), 'embeddings'
    trained = [k for k in on[1] if tf.is_trained(k, stage)]
    assert trained and 'layer%d.0.conv1.weight' % stage in trained
    for k in on[1]:
        if k in trained:
            assert on[1][k] is not None and torch.equal(on[1][k], off[1][k]), k
        else:
            assert on[1][k] is None and off[1][k] is None, k
    for k, v in on[2].items():                        # frozen BatchNorm: every buffer is what was loaded
        assert torch.equal(v, torch.as_tensor(np.asarray(sd[k])).to(v.dtype).reshape(v.shape)), k


# ------------------------------------------------------------------------------------------------------------------
# one pass and chunks: the mode on against off, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('arithmetic', list(ARITHMETICS))
@pytest.mark.parametrize('variant,stage', [('r18', 1), ('r18', 3), ('r18', 4), ('conv5', 2), ('conv5', 3)])
def test_one_pass_keeps_the_bits_of_the_mode_off(variant, stage, arithmetic):
    n = CASES[variant]
    modes = ARITHMETICS[arithmetic]
    _equal_steps(_lib_step(variant, n, n, stage, True, **modes), _lib_step(variant, n, n, stage, False, **modes), _inputs(variant, n)[0], stage)


@pytest.mark.parametrize('arithmetic', list(ARITHMETICS))
@pytest.mark.parametrize('stage', [1, 3])
def test_chunked_step(stage, arithmetic):
    """resnet18, 5 frames in passes of 2, 2, 1: the recompute passes start at the first trained op on their rows of the cache"""
    modes = ARITHMETICS[arithmetic]
    sd, frames, dout = _inputs('r18', 5)
    on, off = _lib_step('r18', 5, 2, stage, True, **modes), _lib_step('r18', 5, 2, stage, False, **modes)
    _equal_steps(on, off, sd, stage)
    key = ('torch', stage)
    if key not in _cache:
        x = eo.preprocess(frames)
        _cache[key] = (tf.partial_step(sd, x, dout, 'r18', stage, torch.float64, True)[1], tf.partial_step(sd, x, dout, 'r18', stage, torch.float32, True)[1])
    g64, g32 = _cache[key]
    keys = sorted(g64)
    assert sorted(k for k in on[1] if on[1][k] is not None) == keys
    d_lib, d_t32 = tr.rel_l2(tf.cat(on[1], keys), tf.cat(g64, keys)), tr.rel_l2(tf.cat(g32, keys), tf.cat(g64, keys))
    print('\n[prefix_once chunks, stage %d, %s] trained gradient rel-L2 to float64: library %.3e, torch fp32 %.3e' % (stage, arithmetic, d_lib, d_t32))
    assert d_lib <= 8.0 * d_t32, (d_lib, d_t32)


# ------------------------------------------------------------------------------------------------------------------
# structure: the launch lists
# ------------------------------------------------------------------------------------------------------------------
def _launches(m):
    L = _lib.lib()
    names, buf = [], C.create_string_buffer(128)
    while L.pvr_trainer_launch_time(m._handle, len(names), buf, 128, None, None):
        names.append(buf.value.decode())
    return names


def _in_prefix(name, stage):
    return name.split()[0] in STEM or any(name.startswith('layer%d.' % s) for s in range(1, stage))


@pytest.mark.parametrize('arithmetic', ['fp32', 'conv_split16'])
@pytest.mark.parametrize('variant,stage', [('r18', 3), ('conv5', 2)])
def test_launch_lists(variant, stage, arithmetic):
    L = _lib.lib()
    n = CASES[variant]
    sd, frames, _ = _inputs(variant, n)
    m = _model(sd, variant, n, stage, True, **ARITHMETICS[arithmetic])
    _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
    fr = torch.from_numpy(frames).cuda()
    out = torch.empty((n, m.out_size), device='cuda')
    cache = torch.empty((n, m._boundary_floats), device='cuda')
    m._forward_pass(fr, 0, n, out, cache)
    first = _launches(m)
    m._forward_pass(fr, 0, n, out, cache, reuse=True)
    again = _launches(m)
    torch.cuda.synchronize()
    trained = 'layer%d.0.conv1' % stage
    assert first[:2] == ['preprocess', 'normalize'] and any(_in_prefix(x, stage) and x.startswith('layer') for x in first) == (stage > 1)
    assert again and again[0].startswith(trained) and not any(_in_prefix(x, stage) for x in again), again[:4]
    assert again == [x for x in first if not _in_prefix(x, stage)]                     # the trained part of the list is the same list
    prefix = [x for x in first if x.startswith('layer') and _in_prefix(x, stage)]
    if arithmetic == 'conv_split16':                  # every prefix op is scale + ONE launch, and no prefix BatchNorm launch is left
        assert len(prefix) % 2 == 0 and all(a.endswith(' scale') and b == a[:-len(' scale')] + ' split16 bn frozen' for a, b in zip(prefix[::2], prefix[1::2])), prefix
    else:
        assert all(x.endswith((' pack', ' bn frozen')) for x in prefix), prefix


# ------------------------------------------------------------------------------------------------------------------
# the handle
# ------------------------------------------------------------------------------------------------------------------
def test_the_handle():
    L = _lib.lib()
    n, stage = CASES['r18'], 3
    sd, frames, dout = _inputs('r18', n)
    m = _model(sd, 'r18', n, stage, True)
    assert L.pvr_trainer_set_prefix_fused(m._handle, 0) == 0 and L.pvr_trainer_set_prefix_fused(m._handle, 1) == 0       # before the arena: free
    fr, dd = torch.from_numpy(frames).cuda(), dout.cuda()
    bf = m._boundary_floats
    assert bf == L.pvr_trainer_boundary_floats(m._handle) == 28 * 28 * 128 and m.boundary_bytes() == 4 * bf
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')

    def step(forward):
        out, g = nan(n, m.out_size), nan(m._flat.numel())
        forward(out)
        _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return out, g

    args = lambda out: (m._handle, vp(m._flat), vp(m._bufs), vp(fr), n, 64, 64)
    plain = step(lambda out: _lib.check(L.pvr_trainer_forward(*args(out), vp(out), out.stride(0), _lib.stream_ptr())))
    cache = nan(n, bf)
    kept = step(lambda out: _lib.check(L.pvr_trainer_forward_boundary(*args(out), vp(cache), 0, vp(out), out.stride(0), _lib.stream_ptr())))
    assert torch.isfinite(cache).all() and torch.equal(kept[0], plain[0]) and torch.equal(kept[1], plain[1])
    held = cache.clone()
    reused = step(lambda out: _lib.check(L.pvr_trainer_forward_boundary(m._handle, vp(m._flat), vp(m._bufs), None, n, 64, 64, vp(cache), 1, vp(out),
                                                                        out.stride(0), _lib.stream_ptr())))      # null frames
    assert torch.equal(reused[0], plain[0]) and torch.equal(reused[1], plain[1]) and torch.equal(cache, held)
    assert L.pvr_trainer_set_prefix_fused(m._handle, 0) == 4 and 'before the first forward' in _lib.last_error()         # PVR_ERR_STATE
    assert L.pvr_trainer_set_prefix_fused(m._handle, 1) == 0
    # refusals: by name, launching nothing
    out = nan(n, m.out_size)
    call = lambda frames_, n_, cache_, reuse: L.pvr_trainer_forward_boundary(m._handle, vp(m._flat), vp(m._bufs), frames_, n_, 64, 64, cache_, reuse, vp(out),
                                                                             out.stride(0), _lib.stream_ptr())
    for frames_, n_, cache_, reuse, word in ((vp(fr), n, None, 0, 'null boundary_dev'), (vp(fr), n, C.c_void_p(cache.data_ptr() + 4), 0, '16-byte'),
                                             (vp(fr), 0, vp(cache), 0, 'max_batch'), (vp(fr), n + 1, vp(cache), 1, 'max_batch'),
                                             (None, n, vp(cache), 0, 'null frames_dev')):
        assert call(frames_, n_, cache_, reuse) == 1 and word in _lib.last_error(), word
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.equal(cache, held)
    whole = E.HipTrainableResNet(sd, 'r18', max_batch=n, freeze_bn=True)              # stage 0: there is no prefix
    assert L.pvr_trainer_forward_boundary(whole._handle, vp(whole._flat), vp(whole._bufs), vp(fr), n, 64, 64, vp(cache), 0, vp(out), out.stride(0),
                                          _lib.stream_ptr()) == 4 and 'no frozen prefix' in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.equal(cache, held)


# ------------------------------------------------------------------------------------------------------------------
# the joint optimizer: resnet18, T = 3, B = 2, F = 2 (12 frames in passes of 5, 5, 2) at stage 3
# ------------------------------------------------------------------------------------------------------------------
def _joint(prefix_once, lr, T=3, B=2, F_=2, bn=1, chunk=5):
    enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], bn)
    enc = _model(enc_sd, 'r18', chunk, 3, prefix_once)
    m = M.PolicyNetWithEncoder(enc, R.A, bool(bn), num_frames=F_, max_unroll=T, max_batch=B)
    m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
    m.train()
    return enc, m, M.HipJointRMSprop(m, lr=lr)


def test_fused_and_autograd_steps_agree_bit_for_bit():
    T, B, F_ = 3, 2, 2
    obs, done, act = R.chain_inputs(13, T, B, F_)
    enc, m, opt = _joint(True, 0.0)
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    opt.step(o, d, a)
    torch.cuda.synchronize()
    assert enc._boundary is None                      # released with the step
    ge_f = opt.grads()['embedding'].clone()
    dlogits = m.policy.last_dlogits(T, B)
    out, _ = m(dict(obs=o, done=d), m.initial_state(B))
    out['policy_logits'].backward(dlogits)
    torch.cuda.synchronize()
    compared = 0
    for (k, _), (off, n, shp) in zip(enc.named_parameters(), enc._slots):
        g = enc.get_parameter(k).grad
        if off < enc.trained_offset:
            assert g is None, k
            assert torch.equal(ge_f[off:off + n], torch.zeros_like(ge_f[off:off + n])), k
        else:
            assert torch.equal(g, ge_f[off:off + n].view(shp)), k
            compared += 1
    assert compared == len(enc._trained_slots) > 10
    m.close()


def test_three_joint_steps_give_the_parameters_of_the_mode_off():
    T, B, F_ = 3, 2, 2
    obs, done, act = R.chain_inputs(13, T, B, F_)
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    flats = []
    for prefix_once in (True, False):
        enc, m, opt = _joint(prefix_once, 1e-3)
        start = enc._flat.clone()
        for _ in range(3):
            loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and np.isfinite(float(norm)) and not torch.equal(enc._flat, start)
        flats.append((enc._flat.clone(), m.policy._flat.clone(), float(loss), float(norm)))
        m.close()
    assert torch.equal(flats[0][0], flats[1][0]) and torch.equal(flats[0][1], flats[1][1]) and flats[0][2:] == flats[1][2:]


# ------------------------------------------------------------------------------------------------------------------
# the Python surface and the driver
# ------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n=40):
    frames = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(frames)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, max_frames, prefix_once=True, T=3, B=2):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'e2e'), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--freeze_embedding_bn', '--embedding_chunk', '5', '--embedding_name', 'resnet18',
                                     '--disable_pretrained_embedding', '--unroll_length', str(T), '--batch_size', str(B), '--eval_frequency', '1',
                                     '--max_frames', str(max_frames), '--embedding_train_from', 'layer4', '--embedding_conv_split16']
                                    + (['--embedding_prefix_once'] if prefix_once else []))


def test_surface_and_driver_train_save_and_resume(tmp_path, capsys):
    from pvr_habitat_amd import main_bc_finetune as Fz
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, freeze_bn=True, max_batch=4, train_from='layer3', conv_split16=True, prefix_once=True)
    enc = net.embedding
    assert enc.prefix_once and enc.boundary_bytes() == E.trainer_boundary_bytes('resnet18', 'layer3')
    assert enc.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, False, True, train_from='layer3', prefix_once=True) \
        < E.trainer_workspace_bytes('resnet18', 4, False, True, train_from='layer3')
    out = net(torch.from_numpy(synth.smooth_frames(11, 6, 64, 64)))           # 6 frames in passes of 4 and 2
    assert out.shape == (6, 512) and out.requires_grad
    out.square().mean().backward()
    for k, p in enc.named_parameters():
        assert (p.grad is not None and bool(torch.isfinite(p.grad).all())) == tf.is_trained(k, 3), k
    net.close()
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 12))['scene']
    assert stats['frames'] == [0, 0, 6]
    assert all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    assert '--embedding_prefix_once' in capsys.readouterr().out                    # the flag is printed
    tar = tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar'
    ck = torch.load(tar, weights_only=False)
    assert ck['flags']['embedding_prefix_once'] is True and ck['flags']['embedding_train_from'] == 'layer4'
    again = Fz.run(_args(tmp_path, 18, prefix_once=False))['scene']                # a resume with the other value is allowed: the bits are the same
    assert again['frames'] == stats['frames'] + [6, 12]
    ck = torch.load(tar, weights_only=False)
    assert ck['actor_model_optimizer_state_dict']['steps'] == 4 and ck['flags']['embedding_prefix_once'] is False
