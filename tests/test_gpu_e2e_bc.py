"""End-to-end BC on the GPU: trainable encoder -> PolicyNet -> NLL with the gradient flowing back into the encoder (models.PolicyNetWithEncoder),
through the fused joint step (models.HipJointRMSprop) and through autograd, and the `main_bc_finetune --train_embedding` driver.

Chain gradients follow the acceptance rule of tests/test_gpu_train.py on the concatenated encoder gradient and on the concatenated policy gradient:
rel_l2(library, float64) <= 8 x rel_l2(torch fp32, float64) against the float64 chain of tests/policy_dobs_refs.py, computed once per case."""
import os
import pickle

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M
from pvr_habitat_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

# name -> (variant, T, B, F, batch_norm)
CHAIN = {'r18_bn': ('r18', 3, 2, 2, 1), 'r18_nobn': ('r18', 3, 2, 2, 0), 'conv5_bn': ('conv5', 2, 1, 2, 1)}
_cache = {}


def _model(variant, T, B, F_, bn, enc_sd, pol_sd):
    enc = E.HipTrainableResNet(enc_sd, variant, max_batch=T * B * F_)
    enc.train()
    for p in enc.parameters():
        p.requires_grad = True
    m = M.PolicyNetWithEncoder(enc, R.A, bool(bn), num_frames=F_, max_unroll=T, max_batch=B)
    m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
    m.train()
    return m


def _named(m, flat_policy, flat_encoder):
    """flat gradient buffers -> ({encoder parameter: grad}, {policy parameter: grad}) on the host"""
    pol, enc = m.policy, m.embedding
    gp = {k: flat_policy[o:o + int(np.prod(shp))].view(shp).cpu() for k, (o, shp) in pol._slots.items() if o < pol._n_train}
    names = [k for k, _ in enc.named_parameters()]
    ge = {k: flat_encoder[o:o + n].view(shp).cpu() for k, (o, n, shp) in zip(names, enc._slots)}
    return ge, gp


def case(name):
    """the float64 and fp32 chains, the fused step (learning rate 0: the parameters stay) and the autograd path on one model: once per case"""
    if name not in _cache:
        variant, T, B, F_, bn = CHAIN[name]
        enc_sd = synth.resnet50_state_dict(3, variant)
        pol_sd = R.policy_params(5, F_ * E.OUT_SIZE[variant], bn)
        obs, done, act = R.chain_inputs(13, T, B, F_)
        c = dict(f64=R.chain_grads(enc_sd, pol_sd, obs, done, act, variant, bn, torch.float64),
                 f32=R.chain_grads(enc_sd, pol_sd, obs, done, act, variant, bn, torch.float32))
        m = _model(variant, T, B, F_, bn, enc_sd, pol_sd)
        o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
        opt = M.HipJointRMSprop(m, lr=0.0)
        loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        g = opt.grads()
        c['fused'] = (float(loss), float(norm)) + _named(m, g['policy'].clone(), g['embedding'].clone())
        dlogits = m.policy.last_dlogits(T, B)                                   # what the fused step's loss kernel handed to its backward

        def autograd(upstream):
            for p in m.parameters():
                p.grad = None
            out, _ = m(dict(obs=o, done=d), m.initial_state(B))
            loss = R.nll(out['policy_logits'], a)
            if upstream is None:
                loss.backward()                                                  # the reference's lines: torch's own log_softmax / nll_loss
            else:
                out['policy_logits'].backward(upstream)
            torch.cuda.synchronize()
            ge = {k: p.grad.detach().cpu() for k, p in m.embedding.named_parameters()}
            gp = {k: p.grad.detach().cpu() for k, p in m.policy.named_parameters() if p.grad is not None}
            return (float(loss), None, ge, gp)
        c['autograd'] = autograd(None)
        c['autograd_same_upstream'] = autograd(dlogits)
        m.close()
        _cache[name] = c
    return _cache[name]


@pytest.mark.parametrize('path', ['fused', 'autograd'])
@pytest.mark.parametrize('name', list(CHAIN))
def test_chain_gradients_against_float64(name, path):
    c = case(name)
    loss64, e64, p64 = c['f64']
    _, e32, p32 = c['f32']
    loss, norm, ge, gp = c[path]
    assert sorted(ge) == sorted(e64) and sorted(gp) == sorted(p64)
    assert loss == pytest.approx(loss64, rel=1e-4)
    for what, g, g32, g64 in (('encoder', ge, e32, e64), ('policy', gp, p32, p64)):
        ok, d, d32 = R.accept(R.cat(g), R.cat(g32), R.cat(g64))
        print('\n[chain %s %s %s] concatenated rel-L2 to float64: library %.3e, torch fp32 %.3e (ratio %.2f)' % (name, path, what, d, d32, d / d32))
        assert ok, (what, d, d32)
    if norm is not None:
        want = float(torch.cat([R.cat(e64), R.cat(p64)]).norm())
        assert norm == pytest.approx(want, rel=1e-3), (norm, want)


@pytest.mark.parametrize('name', list(CHAIN))
def test_fused_and_autograd_paths_agree_bit_for_bit(name):
    """The fused step (four library calls) and the autograd path (the two torch.autograd.Functions chained by autograd) run the same kernels on the
    same buffers: on the same d(loss)/d(logits) every encoder and policy gradient agrees in every bit.  The upstream gradient is the one thing the two
    forms of an iteration compute differently - the fused step in the library's loss kernel, the reference's lines in torch's log_softmax / nll_loss,
    which round differently in the last bit (as tests/test_gpu_policy.py notes for the policy alone) - so the autograd path is given the fused step's
    own (pvr_policy_last_dlogits); with torch's loss the gradients differ by fp32 noise (measured on an MI355X: largest |difference| 3.0e-8 for resnet18
    with BatchNorm1d, 1.5e-8 without, 7.0e-7 for resnet50), which is printed and held to 1e-5 of the gradient's largest element: on identical forward bits the backward is linear in the upstream gradient, the
    two dlogits differ by about four roundings per element (u = 6e-8: exp, the subtraction, the scaling, log-sum-exp against max + log), and 1e-5 = 170 u
    leaves a factor of 40 for cancellation in the sums."""
    c = case(name)
    _, _, ge_f, gp_f = c['fused']
    _, _, ge_a, gp_a = c['autograd_same_upstream']
    assert all(torch.equal(ge_f[k], ge_a[k]) for k in ge_f), [k for k in ge_f if not torch.equal(ge_f[k], ge_a[k])][:5]
    assert all(torch.equal(gp_f[k], gp_a[k]) for k in gp_f), [k for k in gp_f if not torch.equal(gp_f[k], gp_a[k])][:5]
    _, _, ge_t, gp_t = c['autograd']
    diff = max(max(float((ge_f[k] - ge_t[k]).abs().max()) for k in ge_f), max(float((gp_f[k] - gp_t[k]).abs().max()) for k in gp_f))
    top = max(max(float(ge_f[k].abs().max()) for k in ge_f), max(float(gp_f[k].abs().max()) for k in gp_f))
    print('\n[chain %s] fused vs autograd with torch\'s loss: largest |difference| %.3e (largest element %.3e); loss %.9g vs %.9g'
          % (name, diff, top, c['fused'][0], c['autograd'][0]))
    assert diff <= 1e-5 * top, (diff, top)


def test_model_surface_state_dict_and_eval():
    variant, T, B, F_, bn = CHAIN['r18_bn']
    m = _model(variant, T, B, F_, bn, synth.resnet50_state_dict(3, variant), R.policy_params(5, F_ * 512, bn))
    keys = list(m.state_dict())
    assert any(k.startswith('embedding.') for k in keys) and any(k.startswith('policy.') for k in keys)
    assert all(k.startswith(('embedding.', 'policy.')) for k in keys)
    assert 'embedding.conv1.weight' in keys and 'policy.fc.1.weight' in keys and 'policy.core.weight_hh_l1' in keys
    obs, done, _ = R.chain_inputs(13, T, B, F_)
    o, d = torch.from_numpy(obs).cuda(), done.cuda()
    # the split: frame f of observation n is row n * F + f
    fr = m.split_frames(o)
    assert fr.shape == (T * B * F_, 64, 64, 3) and fr.is_contiguous()
    assert torch.equal(fr[3].cpu(), torch.from_numpy(obs.reshape(T * B, 64, 64, 6)[1, :, :, 3:6]))
    m.eval()
    with torch.no_grad():
        out, (h, c) = m(dict(obs=o, done=d), tuple(s.cuda() for s in m.initial_state(B)))
    assert out['policy_logits'].shape == (T, B, R.A) and out['action'].shape == (T, B) and h.shape == (2, B, 1024)
    # eval = the frozen f32 plan of the current parameters in front of the eval policy
    frozen = E.HipResNet50({k: v.detach().cpu() for k, v in m.embedding.state_dict().items()}, variant, compute_dtype='f32', max_batch=T * B * F_)
    x = frozen(fr).view(T, B, -1)
    with torch.no_grad():
        want, _ = m.policy(dict(obs=x, done=d), tuple(s.cuda() for s in m.initial_state(B)))
    assert torch.equal(out['policy_logits'], want['policy_logits'])
    with pytest.raises(RuntimeError, match='eval mode'):
        M.HipJointRMSprop(m).step(o, d, torch.zeros((T, B), dtype=torch.int64))
    with pytest.raises(NotImplementedError, match='momentum'):
        M.HipJointRMSprop(m, momentum=0.9)
    frozen.close()
    m.close()


def test_joint_optimizer_trains_and_round_trips_its_state():
    variant, T, B, F_, bn = CHAIN['r18_bn']
    enc_sd, pol_sd = synth.resnet50_state_dict(3, variant), R.policy_params(5, F_ * 512, bn)
    obs, done, act = R.chain_inputs(13, T, B, F_)
    o, d, a = torch.from_numpy(obs).cuda(), done.cuda(), act.cuda()
    m = _model(variant, T, B, F_, bn, enc_sd, pol_sd)
    opt = M.HipJointRMSprop(m, lr=1e-4, max_epochs=20)
    w0 = m.embedding._flat.clone()
    losses = []
    for _ in range(4):
        opt.scheduler_step()
        loss, norm = opt.step(o, d, a)
        losses.append(float(loss))
        assert np.isfinite(losses[-1]) and np.isfinite(float(norm))
    print('\n[joint step x4, one batch] loss %s' % ['%.4f' % v for v in losses])
    assert losses[-1] < losses[0] and not torch.equal(m.embedding._flat, w0)
    sd = opt.state_dict()
    assert sd['steps'] == 4 and sd['last_epoch'] == 4 and set(sd['square_avg']) == {'policy', 'embedding'}
    opt2 = M.HipJointRMSprop(m, lr=1e-4, max_epochs=20)
    opt2.load_state_dict(sd)
    assert opt2.steps == 4 and opt2.last_epoch == 4 and all(torch.equal(opt2.square_avg[k].cpu(), sd['square_avg'][k]) for k in sd['square_avg'])
    m.close()


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
def _scene(tmp_path, n=40):
    fr = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(fr)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, max_frames, *extra, T=3, B=2):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'e2e'), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--embedding_name', 'resnet18', '--disable_pretrained_embedding', '--unroll_length', str(T),
                                     '--batch_size', str(B), '--eval_frequency', '1', '--max_frames', str(max_frames)] + list(extra))


def test_driver_trains_saves_resumes_and_returns_early(tmp_path):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 12))['scene']                                   # two iterations of 3 x 2 observations
    assert stats['frames'] == [0, 0, 6]
    assert all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    tar = tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar'
    ck = torch.load(tar, weights_only=False)
    sd = ck['actor_model_state_dict']
    assert any(k.startswith('embedding.') for k in sd) and any(k.startswith('policy.') for k in sd)
    sq = ck['actor_model_optimizer_state_dict']['square_avg']
    assert sq['embedding'].numel() == sum(v.numel() for k, v in sd.items() if k.startswith('embedding.') and not k.endswith(('running_mean', 'running_var', 'num_batches_tracked')))
    assert sq['policy'].numel() > 0 and float(sq['policy'].abs().sum()) > 0 and float(sq['embedding'].abs().sum()) > 0
    assert ck['scheduler_state_dict']['last_epoch'] == 2
    init, _ = E._load_named_state_dict('resnet18', False)
    init = {k: torch.as_tensor(np.asarray(v)) for k, v in init.items()}
    assert sd['embedding.conv1.weight'].shape == init['conv1.weight'].shape
    assert not torch.equal(sd['embedding.conv1.weight'].cpu(), init['conv1.weight'].float())
    assert not torch.equal(sd['embedding.layer4.1.bn2.weight'].cpu(), init['layer4.1.bn2.weight'].float())
    # resume: starts at the saved frame count (the reference's range() repeats it) and runs to four updates
    again = Fz.run(_args(tmp_path, 18))['scene']
    assert again['frames'] == stats['frames'] + [6, 12]
    ck2 = torch.load(tar, weights_only=False)
    assert ck2['scheduler_state_dict']['last_epoch'] == 4 and ck2['actor_model_optimizer_state_dict']['steps'] == 4
    mtime = os.path.getmtime(tar)
    finished = Fz.run(_args(tmp_path, 12))['scene']                                # frames[-1] = 12 >= max_frames: returns without training
    assert finished['frames'] == again['frames'] and os.path.getmtime(tar) == mtime


def test_driver_autograd_step_runs_the_reference_lines(tmp_path):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 12, '--autograd_step', '--batch_norm'))['scene']
    assert stats['frames'] == [0, 0, 6] and all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    ck = torch.load(tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar', weights_only=False)
    assert len(ck['actor_model_optimizer_state_dict']['state']) > 60                # torch.optim.RMSprop over both parameter sets
    assert ck['scheduler_state_dict']['last_epoch'] == 2


def test_driver_memory_guard_names_a_size_that_fits(tmp_path, monkeypatch):
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    gb = 1 << 30
    monkeypatch.setattr(torch.cuda, 'mem_get_info', lambda *a, **k: (gb, 256 * gb))
    with pytest.raises(RuntimeError, match='largest unroll_length x batch_size x frames that fits is') as e:
        Fz.run(_args(tmp_path, 80, T=10, B=4))                                     # 80 frames of resnet18: about 2.4 GB
    fit = int(str(e.value).split('that fits is ')[1].split()[0])
    assert 0 < fit < 80
    assert E.trainer_workspace_bytes('resnet18', fit) <= gb < E.trainer_workspace_bytes('resnet18', fit + 1)
    assert not os.path.exists(tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar')
