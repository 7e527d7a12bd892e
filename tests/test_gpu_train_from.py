"""Partial fine-tuning on the GPU (pvr_trainer_set_train_from; EmbeddingNet(..., train=True, train_from='layer3'); --embedding_train_from): resnet18
with 3 frames and resnet50 with 2, as tests/test_gpu_frozen_bn.py.

Two oracles.  (1) Equality of bits with the handle that trains everything: with frozen BatchNorm and conv_split16 the prefix runs the very launches of
stage 0, so the embeddings and every trained tensor's gradient must keep their bits - a weight gradient dropped at the boundary or a wrong buffer of
the liveness pool shows as a difference.  (2) Torch's recipe (tests/train_from_refs.py: the prefix modules in eval with requires_grad False) for the
fp32 arithmetic, whose prefix ops are the fused launches: embeddings within the 1e-4 rel-L2 of tests/test_gpu_train.py, the concatenated trained
gradient within 8 x the distance torch's own fp32 gradient keeps from float64 (that file's criterion), and per trained tensor the same factor against
the larger of that tensor's and the concatenated torch-fp32 distance: the ReLU masks an fp32 forward flips against float64 land in different tensors
for two fp32 evaluations in different orders, so one tensor's own torch-fp32 distance can be far below the network's; a dropped or mis-wired
gradient moves a tensor by order 1."""
import ctypes as C
import os
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
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr())


def _inputs(variant, n):
    sd = synth.resnet50_state_dict(3, variant)
    frames = synth.smooth_frames(11, n, 64, 64)
    dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
    return sd, frames, eo.preprocess(frames), dout


def _lib_step(sd, variant, frames, dout, max_batch, stage, freeze_bn=True, **modes):
    """one autograd step -> (embeddings, {parameter: grad or None}, {buffer: value})"""
    kw = dict(modes, train_from=LAYER[stage]) if stage else modes
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=freeze_bn, **kw)
    m.train()
    for p in m.trained_parameters():
        p.requires_grad = True
    out = m(torch.from_numpy(frames).cuda())
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.endswith(STATS)}
    return out.detach().cpu(), grads, bufs


def _same_buffers(bufs, sd, only=lambda k: True):
    assert sorted(bufs) == sorted(k for k in sd if k.endswith(STATS))
    for k, v in bufs.items():
        if only(k):
            want = torch.as_tensor(np.asarray(sd[k]))
            assert torch.equal(v, want.to(v.dtype).reshape(v.shape)), k


def case(variant, stage):
    """torch's references and two library runs (fp32: the fused prefix) of one (variant, stage) with frozen BatchNorm, computed once"""
    key = (variant, stage)
    if key not in _cache:
        n = CASES[variant]
        sd, frames, x, dout = _inputs(variant, n)
        _cache[key] = dict(sd=sd, f64=tf.partial_step(sd, x, dout, variant, stage, torch.float64, True),
                           f32=tf.partial_step(sd, x, dout, variant, stage, torch.float32, True),
                           lib=_lib_step(sd, variant, frames, dout, n, stage), lib2=_lib_step(sd, variant, frames, dout, n, stage))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------------
# the handle
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [1, 3])
@pytest.mark.parametrize('variant', list(CASES))
def test_the_prefix_span_of_the_gradient_is_exactly_zero(variant, stage):
    L = _lib.lib()
    n = CASES[variant]
    sd, frames, _, dout = _inputs(variant, n)
    m = E.HipTrainableResNet(sd, variant, max_batch=n, freeze_bn=True, train_from=LAYER[stage])
    m.train()
    off = m.trained_offset
    assert 0 < off == L.pvr_trainer_trained_offset(m._handle) < m._flat.numel()
    dout_dev = dout.cuda()
    grads = torch.full_like(m._flat, float('nan'))
    m._forward_raw(torch.from_numpy(frames).cuda())
    _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(grads), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(grads[:off], torch.zeros_like(grads[:off])), 'the prefix span is not exactly 0.0'
    assert torch.isfinite(grads[off:]).all(), 'a trained gradient was not written'
    assert all(bool(grads[o:o + k].abs().sum() > 0) for o, k, _ in m._trained_slots), 'a trained tensor has an all-zero gradient'
    # the accumulate form adds the zeros like everything else
    old = torch.randn(m._flat.shape, generator=torch.Generator().manual_seed(3)).cuda()
    acc, scratch = old.clone(), torch.full_like(m._flat, float('nan'))
    m._forward_raw(torch.from_numpy(frames).cuda())
    _lib.check(L.pvr_trainer_backward_acc(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(acc), 1, vp(scratch), scratch.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(scratch, grads) and torch.equal(acc, old + grads) and torch.equal(acc[:off], old[:off])


def test_the_stage_is_locked_by_the_first_forward():
    L = _lib.lib()
    sd, frames, _, _ = _inputs('r18', 2)
    m = E.HipTrainableResNet(sd, 'r18', max_batch=2, freeze_bn=True, train_from='layer3')
    m.train()
    ws = m.workspace_bytes()
    assert L.pvr_trainer_set_train_from(m._handle, 2) == 0 and L.pvr_trainer_set_train_from(m._handle, 3) == 0      # before the arena: free
    m._forward_raw(torch.from_numpy(frames).cuda())
    assert L.pvr_trainer_set_train_from(m._handle, 2) == 4 and 'before the first forward' in _lib.last_error()       # PVR_ERR_STATE
    assert L.pvr_trainer_set_train_from(m._handle, 0) == 4
    assert L.pvr_trainer_set_train_from(m._handle, 3) == 0 and L.pvr_trainer_train_from(m._handle) == 3             # the stage it has: no change
    assert m.workspace_bytes() == ws
    torch.cuda.synchronize()


@pytest.mark.parametrize('variant', list(CASES))
def test_two_runs_give_identical_bits(variant):
    a, b = case(variant, 3)['lib'], case(variant, 3)['lib2']
    assert torch.equal(a[0], b[0])
    assert all((a[1][k] is None and b[1][k] is None) or torch.equal(a[1][k], b[1][k]) for k in a[1])


# ------------------------------------------------------------------------------------------------------------------
# against the handle that trains everything: equality of bits (the unfused prefix of conv_split16)
# ------------------------------------------------------------------------------------------------------------------
def _bits_against_stage0(variant, stage, **modes):
    n = CASES[variant]
    sd, frames, _, dout = _inputs(variant, n)
    key = ('stage0', variant, tuple(sorted(modes)))
    if key not in _cache:
        _cache[key] = _lib_step(sd, variant, frames, dout, n, 0, **modes)
    full, part = _cache[key], _lib_step(sd, variant, frames, dout, n, stage, **modes)
    assert torch.equal(part[0], full[0]), 'embeddings'
    trained = [k for k in part[1] if tf.is_trained(k, stage)]
    assert trained and 'layer%d.0.conv1.weight' % stage in trained
    for k in part[1]:
        if k in trained:
            assert part[1][k] is not None and torch.equal(part[1][k], full[1][k]), k
        else:
            assert part[1][k] is None, k
    _same_buffers(part[2], sd)


@pytest.mark.parametrize('wgrad_split16', [False, True])
@pytest.mark.parametrize('variant', list(CASES))
def test_stage_3_keeps_the_bits_of_stage_0(variant, wgrad_split16):
    _bits_against_stage0(variant, 3, conv_split16=True, **({'wgrad_split16': True} if wgrad_split16 else {}))


@pytest.mark.parametrize('stage', [1, 2, 4])
def test_resnet18_keeps_the_bits_of_stage_0_at_the_other_stages(stage):
    _bits_against_stage0('r18', stage, conv_split16=True)


# ------------------------------------------------------------------------------------------------------------------
# against torch's recipe: the fp32 arithmetic with the fused prefix
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stage', [1, 3])
@pytest.mark.parametrize('variant', list(CASES))
def test_against_torch_with_the_fused_prefix(variant, stage):
    c = case(variant, stage)
    out, glib, bufs = c['lib']
    figures = dict(out_l2=tr.rel_l2(out, c['f32'][0]), out_max=tr.max_rel(out, c['f32'][0]))
    print('\n[train_from %s stage %d] embeddings vs the fp32 torch restatement: %s; torch fp32 vs float64 %.2e'
          % (variant, stage, {k: '%.2e' % v for k, v in figures.items()}, tr.rel_l2(c['f32'][0], c['f64'][0])))
    assert torch.isfinite(out).all() and max(figures.values()) < 1e-4, figures
    _same_buffers(bufs, c['sd'])                      # frozen BatchNorm: every buffer bit-identical to what was loaded
    g64, g32 = c['f64'][1], c['f32'][1]
    keys = sorted(g64)
    assert keys == sorted(k for k in glib if glib[k] is not None) == sorted(k for k in glib if tf.is_trained(k, stage))
    assert all(glib[k].shape == g64[k].shape and torch.isfinite(glib[k]).all() for k in keys)
    d_lib, d_t32 = tr.rel_l2(tf.cat(glib, keys), tf.cat(g64, keys)), tr.rel_l2(tf.cat(g32, keys), tf.cat(g64, keys))
    print('[train_from %s stage %d] concatenated trained gradient, rel-L2 to float64: library %.3e, torch fp32 %.3e (ratio %.2f)'
          % (variant, stage, d_lib, d_t32, d_lib / d_t32))
    assert d_lib <= 8.0 * d_t32, (d_lib, d_t32)
    worst = (-1.0, '')
    for k in keys:
        dk, tk = tr.rel_l2(glib[k], g64[k]), tr.rel_l2(g32[k], g64[k])
        worst = max(worst, (dk / max(tk, d_t32), k))
        assert dk <= 8.0 * max(tk, d_t32), (k, dk, tk, d_t32)
    first = ['layer%d.0.conv1.weight' % stage] + [k for k in keys if k == 'layer%d.0.downsample.0.weight' % stage]
    print('[train_from %s stage %d] worst tensor %s at %.2f of its allowance / 8; the boundary readers: %s'
          % (variant, stage, worst[1], worst[0], {k: '%.2e (torch fp32 %.2e)' % (tr.rel_l2(glib[k], g64[k]), tr.rel_l2(g32[k], g64[k])) for k in first}))


def test_split_weight_gradients_alone_on_the_fused_prefix():
    """wgrad_split16 without conv_split16 at stage 3: the forward (fused prefix included) keeps its bits, the boundary tensor is scaled by its first
    consumer of the backward, and the trained gradient holds the criterion above"""
    c = case('r18', 3)
    sd, frames, _, dout = _inputs('r18', CASES['r18'])
    out, glib, bufs = _lib_step(sd, 'r18', frames, dout, CASES['r18'], 3, wgrad_split16=True)
    assert torch.equal(out, c['lib'][0])
    keys = sorted(c['f64'][1])
    assert keys == sorted(k for k in glib if glib[k] is not None)
    d_lib, d_t32 = tr.rel_l2(tf.cat(glib, keys), tf.cat(c['f64'][1], keys)), tr.rel_l2(tf.cat(c['f32'][1], keys), tf.cat(c['f64'][1], keys))
    print('\n[train_from r18 stage 3, wgrad_split16] trained gradient rel-L2 to float64: library %.3e, torch fp32 %.3e' % (d_lib, d_t32))
    assert d_lib <= 8.0 * d_t32, (d_lib, d_t32)
    _same_buffers(bufs, sd)


@pytest.mark.parametrize('variant', list(CASES))
def test_batch_statistics_mode_leaves_the_prefix_buffers_alone(variant):
    stage, n = 3, CASES[variant]
    sd, frames, x, dout = _inputs(variant, n)
    out, glib, bufs = _lib_step(sd, variant, frames, dout, n, stage, freeze_bn=False)
    ref_out, ref_g, ref_bufs = tf.partial_step(sd, x, dout, variant, stage, torch.float32, False)
    _same_buffers(bufs, sd, only=lambda k: not tf.is_trained(k, stage))                # prefix statistics and counters: what was loaded
    moved = [k for k in ref_bufs if tf.is_trained(k, stage)]
    assert moved and all(not torch.equal(bufs[k], torch.as_tensor(np.asarray(sd[k])).float()) for k in moved)
    for k in bufs:
        if k.endswith('num_batches_tracked') and tf.is_trained(k, stage):
            assert int(bufs[k]) == int(np.asarray(sd[k])) + 1, k
    figures = dict(out_l2=tr.rel_l2(out, ref_out), out_max=tr.max_rel(out, ref_out), buf_l2=tr.rel_l2(tf.cat(bufs, moved), tf.cat(ref_bufs, moved)),
                   buf_max=tr.max_rel(tf.cat(bufs, moved), tf.cat(ref_bufs, moved)))
    print('\n[train_from %s stage %d, batch statistics] vs the fp32 torch restatement: %s' % (variant, stage, {k: '%.2e' % v for k, v in figures.items()}))
    assert max(figures.values()) < 1e-4, figures
    assert sorted(k for k in glib if glib[k] is not None) == sorted(ref_g)


# ------------------------------------------------------------------------------------------------------------------
# chunks and the joint optimizer: resnet18, 5 frames in passes of 2, 2, 1 at stage 3
# ------------------------------------------------------------------------------------------------------------------
def test_chunked_step():
    sd, frames, x, dout = _inputs('r18', 5)
    f64, f32 = tf.partial_step(sd, x, dout, 'r18', 3, torch.float64, True), tf.partial_step(sd, x, dout, 'r18', 3, torch.float32, True)
    one, chunked = _lib_step(sd, 'r18', frames, dout, 5, 3), _lib_step(sd, 'r18', frames, dout, 2, 3)
    assert torch.equal(one[0], chunked[0]), 'embeddings of passes of 2, 2, 1 and of one pass of 5'
    keys = sorted(f64[1])
    d_t32 = tr.rel_l2(tf.cat(f32[1], keys), tf.cat(f64[1], keys))
    for what, run in (('one', one), ('chunked', chunked)):
        assert sorted(k for k in run[1] if run[1][k] is not None) == keys
        d_lib = tr.rel_l2(tf.cat(run[1], keys), tf.cat(f64[1], keys))
        print('\n[train_from chunks, %s] trained gradient rel-L2 to float64: library %.3e, torch fp32 %.3e' % (what, d_lib, d_t32))
        assert d_lib <= 8.0 * d_t32, (what, d_lib, d_t32)
        _same_buffers(run[2], sd)
    print('[train_from chunks] chunked gradient vs the single pass: rel-L2 %.3e' % tr.rel_l2(tf.cat(chunked[1], keys), tf.cat(one[1], keys)))


def _joint(variant, T, B, F_, bn, chunk, lr):
    enc_sd, pol_sd = synth.resnet50_state_dict(3, variant), R.policy_params(5, F_ * E.OUT_SIZE[variant], bn)
    enc = E.HipTrainableResNet(enc_sd, variant, max_batch=chunk, freeze_bn=True, train_from='layer3')
    enc.train()
    for p in enc.trained_parameters():
        p.requires_grad = True
    m = M.PolicyNetWithEncoder(enc, R.A, bool(bn), num_frames=F_, max_unroll=T, max_batch=B)
    m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
    m.train()
    return enc_sd, enc, m, M.HipJointRMSprop(m, lr=lr)


def test_three_joint_steps_move_the_trained_stages_only():
    T, B, F_ = 3, 2, 2
    obs, done, act = R.chain_inputs(13, T, B, F_)
    enc_sd, enc, m, opt = _joint('r18', T, B, F_, 1, 5, 1e-3)                  # 12 frames in passes of 5, 5, 2
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    flat0, off = enc._flat.clone(), enc.trained_offset
    for _ in range(3):
        loss, norm = opt.step(o, d, a)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and np.isfinite(float(norm))
    assert torch.equal(enc._flat[:off], flat0[:off]), 'a prefix parameter moved'
    sq = opt.square_avg['embedding']
    assert torch.equal(sq[:off], torch.zeros_like(sq[:off])), 'square_avg of the prefix'
    for o_, n_, _ in enc._trained_slots:
        assert not torch.equal(enc._flat[o_:o_ + n_], flat0[o_:o_ + n_]), 'a trained tensor did not move'
    assert bool((sq[off:] > 0).any())
    _same_buffers({k: v.detach().cpu() for k, v in enc.state_dict().items() if k.endswith(STATS)}, enc_sd)
    m.close()


def test_fused_and_autograd_steps_agree_bit_for_bit():
    T, B, F_ = 3, 2, 2
    obs, done, act = R.chain_inputs(13, T, B, F_)
    enc_sd, enc, m, opt = _joint('r18', T, B, F_, 1, 5, 0.0)
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    opt.step(o, d, a)
    torch.cuda.synchronize()
    ge_f = opt.grads()['embedding'].clone()
    dlogits = m.policy.last_dlogits(T, B)
    out, _ = m(dict(obs=o, done=d), m.initial_state(B))
    out['policy_logits'].backward(dlogits)
    torch.cuda.synchronize()
    names = [k for k, _ in enc.named_parameters()]
    compared = 0
    for k, (off, n, shp) in zip(names, enc._slots):
        g = enc.get_parameter(k).grad
        if off < enc.trained_offset:
            assert g is None and not enc.get_parameter(k).requires_grad, k
            assert torch.equal(ge_f[off:off + n], torch.zeros_like(ge_f[off:off + n])), k
        else:
            assert torch.equal(g, ge_f[off:off + n].view(shp)), k
            compared += 1
    assert compared == len(enc._trained_slots) > 10
    m.close()


# ------------------------------------------------------------------------------------------------------------------
# the Python surface and the driver
# ------------------------------------------------------------------------------------------------------------------
def test_surface_embeddingnet_with_train_from():
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, freeze_bn=True, max_batch=4, train_from='layer3')
    enc = net.embedding
    assert net.training and enc.training and enc.train_from == 'layer3' and enc.trained_offset > 0
    frozen = E.EmbeddingNet('resnet18', pretrained=False, compute_dtype='f32', max_batch=4)
    assert list(net.state_dict()) == list(frozen.state_dict())                 # prefix parameters are in state_dict() as before
    assert enc.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, train_from='layer3') < E.trainer_workspace_bytes('resnet18', 4)
    for k, p in enc.named_parameters():
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad == tf.is_trained(k, 3), k
    assert len(enc.prefix_parameters()) + len(enc.trained_parameters()) == len(list(enc.parameters()))
    flat0 = enc._flat.clone()
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=0.01)
    out = net(torch.from_numpy(synth.smooth_frames(11, 6, 64, 64)))           # 6 frames in passes of 4 and 2
    assert out.is_cuda and out.shape == (6, 512) and out.requires_grad and out.grad_fn is not None
    out.square().mean().backward()
    for k, p in enc.named_parameters():
        if tf.is_trained(k, 3):
            assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), k
        else:
            assert p.grad is None, k
    opt.step()
    off = enc.trained_offset
    assert torch.equal(enc._flat[:off], flat0[:off]) and not torch.equal(enc._flat[off:], flat0[off:])
    net.eval()                                        # eval mode is unchanged: the frozen 'f32' plan of the current parameters
    frozen.embedding.load_state_dict(enc.state_dict())
    fr8 = torch.from_numpy(synth.smooth_frames(12, 3, 64, 64))
    assert np.array_equal(net(fr8), frozen(fr8))
    net.close()
    frozen.close()


def _scene(tmp_path, n=40):
    frames = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(frames)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, max_frames, stage='layer4', T=3, B=2):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'e2e'), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--freeze_embedding_bn', '--embedding_chunk', '5', '--embedding_name', 'resnet18',
                                     '--disable_pretrained_embedding', '--unroll_length', str(T), '--batch_size', str(B), '--eval_frequency', '1',
                                     '--max_frames', str(max_frames)] + (['--embedding_train_from', stage] if stage else []))


def test_driver_trains_saves_resumes_and_refuses_another_stage(tmp_path, capsys):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 12))['scene']
    assert stats['frames'] == [0, 0, 6]
    assert all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    assert 'layer4' in capsys.readouterr().out.splitlines()[0]                     # the run's first line names the stage
    tar = tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar'
    ck = torch.load(tar, weights_only=False)
    assert ck['flags']['embedding_train_from'] == 'layer4' and ck['flags']['embedding_chunk'] == 5
    sd = ck['actor_model_state_dict']
    init, _ = E._load_named_state_dict('resnet18', False)
    init = {k: torch.as_tensor(np.asarray(v)) for k, v in init.items()}
    for k, v in init.items():
        got = sd['embedding.' + k].cpu()
        same = torch.equal(got, v.to(got.dtype).reshape(got.shape))
        if k.endswith(STATS) or not tf.is_trained(k, 4):
            assert same, k                                                         # the prefix and every running statistic: what was loaded
        else:
            assert not same, k
    again = Fz.run(_args(tmp_path, 18))['scene']                                   # resume: to four updates
    assert again['frames'] == stats['frames'] + [6, 12]
    assert torch.load(tar, weights_only=False)['actor_model_optimizer_state_dict']['steps'] == 4
    mtime = os.path.getmtime(tar)
    for other in ('layer3', None):
        with pytest.raises(ValueError, match='--embedding_train_from layer4; resume with the same stage'):
            Fz.run(_args(tmp_path, 24, stage=other))
    assert os.path.getmtime(tar) == mtime
