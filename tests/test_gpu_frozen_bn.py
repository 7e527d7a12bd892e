"""Frozen-BatchNorm fine-tuning on the GPU (pvr_trainer_set_bn_frozen, pvr_trainer_backward_acc; EmbeddingNet(..., train=True, freeze_bn=True,
max_batch=chunk)): the network against torch's own frozen-BatchNorm step (train mode, every BatchNorm in eval: train_refs.features(...,
training=False) with autograd), the chunked step against the single pass, the Python surface, the fused and the autograd end-to-end step, and the
`main_bc_finetune --train_embedding --freeze_embedding_bn` driver.

Gradients follow the acceptance rule of tests/test_gpu_train.py: the float64 gradient, torch's fp32 gradient and the library's are computed in the
same run and dist(library, float64) <= 8 x dist(torch fp32, float64) on the concatenated gradient.  The mode itself is checked against the
batch-statistics float64 gradient of the same inputs, which lies at a relative distance of order one (1.08 for resnet18, 1.13 for resnet50)."""
import os
import pickle

import numpy as np
import pytest
import torch

import frozen_bn_refs as fr
import policy_dobs_refs as R
import train_refs as tr
from oracle import encoder_oracle as eo
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

CASES = {'r18': 3, 'conv5': 2}          # variant -> frames
_cache = {}
STATS = ('running_mean', 'running_var', 'num_batches_tracked')


def _counting(monkeypatch):
    """calls of the trainer's entry points from here on (the pattern of tests/test_gpu_policy_dobs.py)"""
    L, counts = _lib.lib(), {}
    for name in ('pvr_trainer_forward', 'pvr_trainer_backward', 'pvr_trainer_backward_acc'):
        fn = getattr(L, name)
        counts[name] = 0

        def wrapped(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(L, name, wrapped)
    return counts


def _lib_step(sd, variant, frames, dout, max_batch):
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=True)
    m.train()
    for p in m.parameters():
        p.requires_grad = True
    out = m(torch.from_numpy(frames).cuda())
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.endswith(STATS)}
    return out.detach().cpu(), grads, bufs


def _inputs(variant, n):
    sd = synth.resnet50_state_dict(3, variant)
    frames = synth.smooth_frames(11, n, 64, 64)
    dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
    return sd, frames, eo.preprocess(frames), dout


def case(variant):
    """references and two library runs of one case, computed once and shared by the tests below"""
    if variant not in _cache:
        n = CASES[variant]
        sd, frames, x, dout = _inputs(variant, n)
        _cache[variant] = dict(sd=sd, f64=fr.frozen_step(sd, x, dout, variant, torch.float64), f32=fr.frozen_step(sd, x, dout, variant, torch.float32),
                               batch64=tr.train_step(sd, x, dout, variant, torch.float64)[1],
                               lib=_lib_step(sd, variant, frames, dout, n), lib2=_lib_step(sd, variant, frames, dout, n))
    return _cache[variant]


def _forward_figures(out, ref):
    return dict(out_l2=tr.rel_l2(out, ref), out_max=tr.max_rel(out, ref))


def _gradient_figures(what, glib, g32, g64):
    keys = sorted(g64)
    assert sorted(glib) == keys
    assert all(glib[k].shape == g64[k].shape and torch.isfinite(glib[k]).all() for k in keys)
    d_lib, d_t32 = tr.rel_l2(fr.cat(glib, keys), fr.cat(g64, keys)), tr.rel_l2(fr.cat(g32, keys), fr.cat(g64, keys))
    worst_lib = max(keys, key=lambda k: tr.rel_l2(glib[k], g64[k]))
    worst_t32 = max(keys, key=lambda k: tr.rel_l2(g32[k], g64[k]))
    print('\n[frozen gradients %s] concatenated rel-L2 to float64: library %.3e, torch fp32 %.3e (ratio %.2f)' % (what, d_lib, d_t32, d_lib / d_t32))
    print('[frozen gradients %s] worst tensor: library %s %.3e, torch fp32 %s %.3e' % (what, worst_lib, tr.rel_l2(glib[worst_lib], g64[worst_lib]),
                                                                                    worst_t32, tr.rel_l2(g32[worst_t32], g64[worst_t32])))
    return d_lib, d_t32


def _same_buffers(bufs, sd):
    assert sorted(bufs) == sorted(k for k in sd if k.endswith(STATS))
    for k, v in bufs.items():
        want = torch.as_tensor(np.asarray(sd[k]))
        assert torch.equal(v, want.to(v.dtype).reshape(v.shape)), k


@pytest.mark.parametrize('variant', list(CASES))
def test_forward_and_untouched_running_statistics(variant):
    c = case(variant)
    out, _, bufs = c['lib']
    figures = _forward_figures(out, c['f32'][0])
    print('\n[frozen forward %s] vs the fp32 torch restatement: %s; torch fp32 vs float64 %.2e'
          % (variant, {k: '%.2e' % v for k, v in figures.items()}, tr.rel_l2(c['f32'][0], c['f64'][0])))
    assert torch.isfinite(out).all() and max(figures.values()) < 1e-4, figures
    _same_buffers(bufs, c['sd'])                      # running statistics and counters: bit-identical to what was loaded


@pytest.mark.parametrize('variant', list(CASES))
def test_gradients_against_float64_and_torch_fp32(variant):
    c = case(variant)
    d_lib, d_t32 = _gradient_figures(variant, c['lib'][1], c['f32'][1], c['f64'][1])
    assert d_lib <= 8.0 * d_t32, (d_lib, d_t32)


@pytest.mark.parametrize('variant', list(CASES))
def test_the_gradient_is_the_frozen_one_not_the_batch_statistics_one(variant):
    c = case(variant)
    keys = sorted(c['f64'][1])
    g, frozen, batch = fr.cat(c['lib'][1], keys), fr.cat(c['f64'][1], keys), fr.cat(c['batch64'], keys)
    to_frozen, to_batch = float((g - frozen).norm()), float((g - batch).norm())
    print('\n[frozen mode %s] |library - frozen float64| %.3e, |library - batch-statistics float64| %.3e (factor %.0f); the two references differ by %.2f '
          'relative' % (variant, to_frozen, to_batch, to_batch / to_frozen, tr.rel_l2(batch, frozen)))
    assert 100.0 * to_frozen <= to_batch, (to_frozen, to_batch)


@pytest.mark.parametrize('variant', list(CASES))
def test_two_runs_give_identical_bits(variant):
    a, b = case(variant)['lib'], case(variant)['lib2']
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1])


# ------------------------------------------------------------------------------------------------------------------
# the handle: mode switch, accumulation
# ------------------------------------------------------------------------------------------------------------------
def test_accumulation_is_one_exact_add_and_a_mode_switch_drops_the_forward():
    L = _lib.lib()
    sd, frames, _, dout = _inputs('r18', 2)
    m = E.HipTrainableResNet(sd, 'r18', max_batch=2, freeze_bn=True)
    m.train()
    fr_dev, dout_dev = torch.from_numpy(frames).cuda(), dout.cuda()
    vp = lambda t: _lib.C.c_void_p(t.data_ptr())
    plain = torch.full_like(m._flat, float('nan'))
    m._forward_raw(fr_dev)
    _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(plain), _lib.stream_ptr()))
    old = torch.randn(m._flat.shape, generator=torch.Generator().manual_seed(3)).cuda()
    grads, scratch = old.clone(), torch.full_like(m._flat, float('nan'))
    m._forward_raw(fr_dev)
    assert L.pvr_trainer_backward_acc(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(grads), 1, vp(scratch), 16, _lib.stream_ptr()) == 1
    assert 'scratch' in _lib.last_error()            # refused, and the held forward is still there:
    _lib.check(L.pvr_trainer_backward_acc(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(grads), 1, vp(scratch), scratch.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(scratch, plain), 'the pass written to the scratch is not pvr_trainer_backward\'s gradient'
    assert torch.equal(grads, old + scratch), 'grads is not old + scratch in fp32'
    # accumulate == 0 is pvr_trainer_backward
    m._forward_raw(fr_dev)
    over = old.clone()
    _lib.check(L.pvr_trainer_backward_acc(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(over), 0, None, 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(over, plain)
    # one backward per forward; switching the mode drops a held forward
    assert L.pvr_trainer_backward_acc(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(over), 0, None, 0, _lib.stream_ptr()) == 4
    m._forward_raw(fr_dev)
    m.set_bn_frozen(False)
    assert L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dout_dev), dout_dev.stride(0), vp(over), _lib.stream_ptr()) == 4
    assert not m.freeze_bn
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# chunks: resnet18, 5 frames in passes of 2, 2, 1 against one pass of 5
# ------------------------------------------------------------------------------------------------------------------
def chunk_case():
    if 'chunks' not in _cache:
        sd, frames, x, dout = _inputs('r18', 5)
        _cache['chunks'] = dict(sd=sd, f64=fr.frozen_step(sd, x, dout, 'r18', torch.float64), f32=fr.frozen_step(sd, x, dout, 'r18', torch.float32),
                                one=_lib_step(sd, 'r18', frames, dout, 5), chunked=_lib_step(sd, 'r18', frames, dout, 2),
                                chunked2=_lib_step(sd, 'r18', frames, dout, 2))
    return _cache['chunks']


def test_chunked_embeddings_and_gradients():
    c = chunk_case()
    for what in ('one', 'chunked'):
        figures = _forward_figures(c[what][0], c['f32'][0])
        print('\n[frozen chunks, %s] embeddings vs the fp32 torch restatement: %s' % (what, {k: '%.2e' % v for k, v in figures.items()}))
        assert max(figures.values()) < 1e-4, (what, figures)
        _same_buffers(c[what][2], c['sd'])
    print('[frozen chunks] embeddings of passes of 2, 2, 1 and of one pass of 5 bit-identical: %s' % torch.equal(c['one'][0], c['chunked'][0]))
    for what in ('one', 'chunked'):
        d_lib, d_t32 = _gradient_figures('r18 x 5, ' + what, c[what][1], c['f32'][1], c['f64'][1])
        assert d_lib <= 8.0 * d_t32, (what, d_lib, d_t32)
    keys = sorted(c['one'][1])
    print('[frozen chunks] chunked gradient vs the single pass: rel-L2 %.3e' % tr.rel_l2(fr.cat(c['chunked'][1], keys), fr.cat(c['one'][1], keys)))


def test_the_chunked_step_is_bit_identical_run_to_run():
    a, b = chunk_case()['chunked'], chunk_case()['chunked2']
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_passes_issued(monkeypatch):
    sd, frames, _, dout = _inputs('r18', 5)
    counts = _counting(monkeypatch)
    _lib_step(sd, 'r18', frames, dout, 5)               # a single chunk: one forward, one backward, no recompute
    assert counts == {'pvr_trainer_forward': 1, 'pvr_trainer_backward': 1, 'pvr_trainer_backward_acc': 0}
    for k in counts:
        counts[k] = 0
    _lib_step(sd, 'r18', frames, dout, 2)               # 3 passes forward; the backward recomputes all but the last
    assert counts == {'pvr_trainer_forward': 5, 'pvr_trainer_backward': 0, 'pvr_trainer_backward_acc': 3}
    m = E.HipTrainableResNet(sd, 'r18', max_batch=2)    # batch statistics: nothing changes
    m.train()
    with pytest.raises(ValueError, match='it cannot be chunked'):
        m(torch.from_numpy(frames).cuda())


# ------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------
def test_surface_embeddingnet_with_frozen_batchnorm():
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, freeze_bn=True, max_batch=4)
    assert net.training and net.embedding.training and net.embedding.freeze_bn and net.embedding.max_batch == 4
    before = {k: v.detach().cpu().clone() for k, v in net.embedding.state_dict().items() if k.endswith(STATS)}
    flat0 = net.embedding._flat.clone()
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    out = net(torch.from_numpy(synth.smooth_frames(11, 6, 64, 64)))          # 6 frames in passes of 4 and 2
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.shape == (6, 512) and out.requires_grad and out.grad_fn is not None
    out.square().mean().backward()
    for k, p in net.embedding.named_parameters():
        assert p.is_cuda and p.requires_grad and p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), k
    opt.step()
    assert not torch.equal(net.embedding._flat, flat0)
    after = {k: v.detach().cpu() for k, v in net.embedding.state_dict().items() if k.endswith(STATS)}
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
    net.set_bn_frozen(False)                          # back to batch statistics: the chunk is max_batch again
    with pytest.raises(ValueError, match='max_batch'):
        net(torch.from_numpy(synth.smooth_frames(11, 6, 64, 64)))
    net.close()


def test_fused_and_autograd_steps_agree_bit_for_bit_on_the_chunked_path():
    variant, T, B, F_, bn = 'r18', 3, 2, 2, 1
    enc_sd, pol_sd = synth.resnet50_state_dict(3, variant), R.policy_params(5, F_ * E.OUT_SIZE[variant], bn)
    obs, done, act = R.chain_inputs(13, T, B, F_)
    enc = E.HipTrainableResNet(enc_sd, variant, max_batch=5, freeze_bn=True)      # 12 frames in passes of 5, 5, 2
    enc.train()
    for p in enc.parameters():
        p.requires_grad = True
    m = M.PolicyNetWithEncoder(enc, R.A, bool(bn), num_frames=F_, max_unroll=T, max_batch=B)
    m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
    m.train()
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    opt = M.HipJointRMSprop(m, lr=0.0)
    loss, norm = opt.step(o, d, a)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and np.isfinite(float(norm))
    g = opt.grads()
    ge_f, gp_f = g['embedding'].clone(), g['policy'].clone()
    dlogits = m.policy.last_dlogits(T, B)
    out, _ = m(dict(obs=o, done=d), m.initial_state(B))
    out['policy_logits'].backward(dlogits)
    torch.cuda.synchronize()
    names = [k for k, _ in enc.named_parameters()]
    for k, (off, n, shp) in zip(names, enc._slots):
        assert torch.equal(enc.get_parameter(k).grad, ge_f[off:off + n].view(shp)), k
    pol, compared = m.policy, 0
    for k, p in pol.named_parameters():
        if p.grad is not None:
            off, shp = pol._slots[k]
            assert off < pol._n_train and torch.equal(p.grad, gp_f[off:off + int(np.prod(shp))].view(shp)), k
            compared += 1
    assert compared > 10
    _same_buffers({k: v.detach().cpu() for k, v in enc.state_dict().items() if k.endswith(STATS)}, enc_sd)
    m.close()


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n=40):
    frames = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(frames)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, max_frames, T=3, B=2):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'e2e'), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--freeze_embedding_bn', '--embedding_chunk', '5', '--embedding_name', 'resnet18',
                                     '--disable_pretrained_embedding', '--unroll_length', str(T), '--batch_size', str(B), '--eval_frequency', '1',
                                     '--max_frames', str(max_frames)])


def test_driver_trains_saves_resumes_and_keeps_the_running_statistics(tmp_path, capsys):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 12))['scene']                                   # two iterations of 3 x 2 observations = 12 frames in passes of 5, 5, 2
    assert stats['frames'] == [0, 0, 6]
    assert all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    assert sum('WARNING' in line and 'freeze_embedding_bn' in line for line in capsys.readouterr().out.splitlines()) == 1
    tar = tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar'
    ck = torch.load(tar, weights_only=False)
    assert ck['flags']['freeze_embedding_bn'] is True and ck['flags']['embedding_chunk'] == 5
    sd = ck['actor_model_state_dict']
    init, _ = E._load_named_state_dict('resnet18', False)
    init = {k: torch.as_tensor(np.asarray(v)) for k, v in init.items()}
    assert not torch.equal(sd['embedding.conv1.weight'].cpu(), init['conv1.weight'].float())
    assert not torch.equal(sd['embedding.layer4.1.bn2.weight'].cpu(), init['layer4.1.bn2.weight'].float())
    stat_keys = [k for k in init if k.endswith(STATS)]
    assert len(stat_keys) == 60                                                    # 20 BatchNorms of resnet18
    for k in stat_keys:                                                            # the saved running statistics are the initial ones
        assert torch.equal(sd['embedding.' + k].cpu(), init[k].to(sd['embedding.' + k].dtype).reshape(sd['embedding.' + k].shape)), k
    assert ck['scheduler_state_dict']['last_epoch'] == 2
    again = Fz.run(_args(tmp_path, 18))['scene']                                   # resume: to four updates
    assert again['frames'] == stats['frames'] + [6, 12]
    ck2 = torch.load(tar, weights_only=False)
    assert ck2['scheduler_state_dict']['last_epoch'] == 4 and ck2['actor_model_optimizer_state_dict']['steps'] == 4
    mtime = os.path.getmtime(tar)
    finished = Fz.run(_args(tmp_path, 12))['scene']                                # frames[-1] = 12 >= max_frames: returns without training
    assert finished['frames'] == again['frames'] and os.path.getmtime(tar) == mtime
