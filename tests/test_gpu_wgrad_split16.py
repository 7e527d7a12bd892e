"""The trainer with split-f16 weight gradients (pvr_trainer_set_wgrad_split16; HipTrainableResNet / EmbeddingNet(..., wgrad_split16=True)) on the GPU:
mode on against mode off on the same inputs, against the float64 and fp32 torch steps of tests/train_refs.py and tests/frozen_bn_refs.py, the chunked
frozen-BatchNorm step, and the Python surface.

The forward, dz and the BatchNorm reductions are untouched by the mode, so embeddings, running statistics and every BatchNorm gradient keep their bits.
For the convolution weights the acceptance rule is that of tests/test_gpu_train.py - dist(library, float64) <= 8 x d_t32 on the concatenated gradient,
d_t32 = dist(torch fp32, float64) computed in the same run - and, sharper, dist(on, off) <= d_t32 over the convolution weights: the two library runs
share one forward, so no ReLU mask can flip between them, the split product differs from the fp32 one by about 2^-22 relative, and a wiring error
moves the gradient by order 1.  The arithmetic itself is held to its bound by tests/test_gpu_wgrad_split16_kernels.py."""
import numpy as np
import pytest
import torch

import frozen_bn_refs as fr
import policy_dobs_refs as R
import test_gpu_train as tg
import train_refs as tr
from oracle import encoder_oracle as eo
from pvr_habitat_amd import synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

STATS = ('running_mean', 'running_var', 'num_batches_tracked')
_cache = {}


def _lib_step(sd, variant, frames, dout, max_batch, split16, freeze_bn=False):
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=freeze_bn, wgrad_split16=split16)
    assert m.wgrad_split16 is bool(split16)
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
    """one batch-statistics case of tests/test_gpu_train.py (resnet18 x 3 frames, resnet50 x 2): its float64 step, its fp32 torch step and its
    library step with the mode off are computed once per run by that file's case() and shared with it - no second float64 network - and two
    library steps with the mode on are made here on the same inputs"""
    if variant not in _cache:
        n = tg.CASES[variant]
        sd, frames, _, dout = _inputs(variant, n)
        ref = tg.case(variant)
        _cache[variant] = dict(f64=ref['f64'], f32=ref['f32'], off=ref['lib'][:3], on=_lib_step(sd, variant, frames, dout, n, True),
                               on2=_lib_step(sd, variant, frames, dout, n, True))
    return _cache[variant]


def _conv_keys(grads):
    return sorted(k for k, v in grads.items() if v.dim() == 4)


def _same_everything_but_conv_weights(on, off):
    assert torch.equal(on[0], off[0]), 'embeddings differ'
    assert len(off[2]) > 10 and all(torch.equal(on[2][k], off[2][k]) for k in off[2]), 'BatchNorm buffers differ'
    bn_keys = sorted(k for k, v in off[1].items() if v.dim() == 1)
    assert len(bn_keys) > 10 and all(torch.equal(on[1][k], off[1][k]) for k in bn_keys), 'a BatchNorm gradient differs'
    return bn_keys


def _on_off(what, on, off, d_t32):
    keys = _conv_keys(off[1])
    assert len(keys) > 10 and all(torch.isfinite(on[1][k]).all() for k in keys)
    d = tr.rel_l2(fr.cat(on[1], keys), fr.cat(off[1], keys))
    worst = max(keys, key=lambda k: tr.rel_l2(on[1][k], off[1][k]))
    print('\n[split16 %s] convolution weights, rel-L2(on, off) %.3e (d_t32 %.3e); worst tensor %s %.3e; conv1 %.3e'
          % (what, d, d_t32, worst, tr.rel_l2(on[1][worst], off[1][worst]), tr.rel_l2(on[1]['conv1.weight'], off[1]['conv1.weight'])))
    assert any(not torch.equal(on[1][k], off[1][k]) for k in keys), 'the mode changed nothing: the split kernels did not run'
    assert d <= d_t32, (d, d_t32)


@pytest.mark.parametrize('variant', ['r18', 'conv5'])
def test_on_against_off_and_the_references(variant):
    c = case(variant)
    _same_everything_but_conv_weights(c['on'], c['off'])
    g64, g32 = c['f64'][1], c['f32'][1]
    keys = sorted(g64)
    assert sorted(c['on'][1]) == keys
    d_t32 = tr.rel_l2(fr.cat(g32, keys), fr.cat(g64, keys))
    d_on, d_off = tr.rel_l2(fr.cat(c['on'][1], keys), fr.cat(g64, keys)), tr.rel_l2(fr.cat(c['off'][1], keys), fr.cat(g64, keys))
    print('\n[split16 %s] concatenated rel-L2 to float64: mode on %.3e, mode off %.3e, torch fp32 %.3e (on / d_t32 %.2f)'
          % (variant, d_on, d_off, d_t32, d_on / d_t32))
    assert d_on <= 8.0 * d_t32, (d_on, d_t32)
    _on_off(variant, c['on'], c['off'], d_t32)


@pytest.mark.parametrize('variant', ['r18', 'conv5'])
def test_two_runs_with_the_mode_on_give_identical_bits(variant):
    a, b = case(variant)['on'], case(variant)['on2']
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_frozen_batchnorm_chunked_step_with_the_mode_on():
    sd, frames, x, dout = _inputs('r18', 5)
    f64, f32 = fr.frozen_step(sd, x, dout, 'r18', torch.float64), fr.frozen_step(sd, x, dout, 'r18', torch.float32)
    one = _lib_step(sd, 'r18', frames, dout, 5, True, freeze_bn=True)
    on = _lib_step(sd, 'r18', frames, dout, 2, True, freeze_bn=True)            # passes of 2, 2, 1
    off = _lib_step(sd, 'r18', frames, dout, 2, False, freeze_bn=True)
    assert torch.equal(on[0], one[0]), 'the embeddings of passes of 2, 2, 1 are not those of one pass of 5'
    _same_everything_but_conv_weights(on, off)
    keys = sorted(f64[1])
    d_t32 = tr.rel_l2(fr.cat(f32[1], keys), fr.cat(f64[1], keys))
    d_on = tr.rel_l2(fr.cat(on[1], keys), fr.cat(f64[1], keys))
    print('\n[split16 frozen chunks] concatenated rel-L2 to float64: mode on %.3e, mode off %.3e, torch fp32 %.3e'
          % (d_on, tr.rel_l2(fr.cat(off[1], keys), fr.cat(f64[1], keys)), d_t32))
    assert d_on <= 8.0 * d_t32, (d_on, d_t32)
    _on_off('frozen chunks', on, off, d_t32)


# ------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------
def test_surface_embeddingnet_trains_with_the_mode_on():
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, wgrad_split16=True, max_batch=4)
    assert net.training and net.embedding.wgrad_split16 and not net.embedding.freeze_bn
    assert net.embedding.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, wgrad_split16=True)
    fr_ = torch.from_numpy(synth.smooth_frames(13, 4, 64, 64))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    a = torch.randn((512,), generator=torch.Generator().manual_seed(5)).cuda() / 512 ** 0.5
    target = torch.randn((4,), generator=torch.Generator().manual_seed(6)).cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((net(fr_) @ a - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print('\n[split16 surface] loss over six Adam steps %s' % ['%.4f' % v for v in losses])
    assert all(np.isfinite(losses)) and losses[5] < losses[0], losses
    # the mode decides the workspace: after the first forward has made it, the setter refuses
    with pytest.raises(RuntimeError, match='before the first forward'):
        net.embedding.set_wgrad_split16(False)
    assert net.embedding.wgrad_split16
    net.embedding.set_wgrad_split16(True)               # (the mode it has: nothing to change)
    net.close()


def test_fused_and_autograd_steps_agree_bit_for_bit_with_the_mode_on():
    variant, T, B, F_, bn = 'r18', 2, 1, 2, 1
    enc_sd, pol_sd = synth.resnet50_state_dict(3, variant), R.policy_params(5, F_ * E.OUT_SIZE[variant], bn)
    obs, done, act = R.chain_inputs(13, T, B, F_)
    enc = E.HipTrainableResNet(enc_sd, variant, max_batch=T * B * F_, wgrad_split16=True)
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
    ge_f = opt.grads()['embedding'].clone()
    dlogits = m.policy.last_dlogits(T, B)
    out, _ = m(dict(obs=o, done=d), m.initial_state(B))
    out['policy_logits'].backward(dlogits)
    torch.cuda.synchronize()
    names = [k for k, _ in enc.named_parameters()]
    assert len(names) > 10
    for k, (off, n, shp) in zip(names, enc._slots):
        assert torch.equal(enc.get_parameter(k).grad, ge_f[off:off + n].view(shp)), k
    m.close()
