"""The trainer with split-f16 forward convolutions and data gradients (pvr_trainer_set_conv_split16; HipTrainableResNet / EmbeddingNet(...,
conv_split16=True)) on the GPU, at the cases of tests/test_gpu_train.py (resnet18 x 3 frames, resnet50 x 2): the forward and the running statistics
within the 1e-4 of the fp32 torch restatement that file asks of the fp32 path, the concatenated gradient within its 8 x dist(torch fp32, float64) of
the float64 gradient - alone, with split-f16 weight gradients, and in the chunked frozen-BatchNorm step - then the explicit off, the late switch, a
trunk whose activations pass f16's 65504, and the Python surface down to the driver's flag.  The float64 and fp32 torch steps and the fp32 library
step are test_gpu_train.py's own, computed once per run.  The arithmetic itself is held to its bound by tests/test_gpu_conv_split16_kernels.py."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frozen_bn_refs as fr
import test_gpu_train as tg
import train_refs as tr
from oracle import encoder_oracle as eo
from pvr_habitat_amd import _lib
from pvr_habitat_amd import synth
from pvr_habitat_amd import embeddings as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

STATS = ('running_mean', 'running_var')
_cache = {}


def _lib_step(sd, variant, frames, dout, max_batch, conv16=True, wgrad16=False, freeze_bn=False, explicit_off=False):
    m = E.HipTrainableResNet(sd, variant, max_batch=max_batch, freeze_bn=freeze_bn, wgrad_split16=wgrad16, conv_split16=conv16)
    if explicit_off:
        m.set_conv_split16(False)
    assert m.conv_split16 is bool(conv16 and not explicit_off) and m.wgrad_split16 is bool(wgrad16)
    m.train()
    for p in m.parameters():
        p.requires_grad = True
    out = m(torch.from_numpy(frames).cuda())
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.endswith(STATS)}
    return out.detach().cpu(), grads, bufs, m.workspace_bytes()


def _inputs(variant, n):
    """the inputs of test_gpu_train.case(variant) (the same seeds)"""
    sd = synth.resnet50_state_dict(3, variant)
    frames = synth.smooth_frames(11, n, 64, 64)
    dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
    return sd, frames, eo.preprocess(frames), dout


def case(variant):
    if variant not in _cache:
        n = tg.CASES[variant]
        sd, frames, _, dout = _inputs(variant, n)
        ref = tg.case(variant)
        _cache[variant] = dict(f64=ref['f64'], f32=ref['f32'], off=ref['lib'], on=_lib_step(sd, variant, frames, dout, n),
                               on2=_lib_step(sd, variant, frames, dout, n), both=_lib_step(sd, variant, frames, dout, n, wgrad16=True))
    return _cache[variant]


def _forward_figures(what, got, ref32):
    out, _, bufs = got[:3]
    ref_out, ref_bufs = ref32[0], ref32[2]
    keys = sorted(ref_bufs)
    figures = dict(out_l2=tr.rel_l2(out, ref_out), out_max=tr.max_rel(out, ref_out))
    if bufs is not None:
        assert sorted(bufs) == keys
        figures.update(buf_l2=tr.rel_l2(fr.cat(bufs, keys), fr.cat(ref_bufs, keys)), buf_max=tr.max_rel(fr.cat(bufs, keys), fr.cat(ref_bufs, keys)))
    print('\n[conv split16 forward %s] vs the fp32 torch restatement: %s' % (what, {k: '%.2e' % v for k, v in figures.items()}))
    assert torch.isfinite(out).all() and max(figures.values()) < 1e-4, figures


def _gradient_figures(what, g_on, g_off, g32, g64):
    keys = sorted(g64)
    assert sorted(g_on) == keys and all(g_on[k].shape == g64[k].shape and torch.isfinite(g_on[k]).all() for k in keys)
    d_t32 = tr.rel_l2(fr.cat(g32, keys), fr.cat(g64, keys))
    d_on, d_off = tr.rel_l2(fr.cat(g_on, keys), fr.cat(g64, keys)), tr.rel_l2(fr.cat(g_off, keys), fr.cat(g64, keys))
    print('\n[conv split16 gradients %s] concatenated rel-L2 to float64: mode on %.3e, fp32 path %.3e, torch fp32 %.3e (on / d_t32 %.2f, fp32 path / d_t32 %.2f)'
          % (what, d_on, d_off, d_t32, d_on / d_t32, d_off / d_t32))
    assert d_on <= 8.0 * d_t32, (d_on, d_t32)


@pytest.mark.parametrize('variant', list(tg.CASES))
@pytest.mark.parametrize('mode', ['on', 'both'])
def test_forward_and_running_statistics(variant, mode):
    c = case(variant)
    _forward_figures('%s %s' % (variant, mode), c[mode], c['f32'])
    assert not torch.equal(c[mode][0], c['off'][0]), 'the mode changed nothing: the split kernels did not run'


@pytest.mark.parametrize('variant', list(tg.CASES))
@pytest.mark.parametrize('mode', ['on', 'both'])
def test_gradients_against_float64_and_torch_fp32(variant, mode):
    c = case(variant)
    _gradient_figures('%s %s' % (variant, mode), c[mode][1], c['off'][1], c['f32'][1], c['f64'][1])


@pytest.mark.parametrize('variant', list(tg.CASES))
def test_two_runs_with_the_mode_on_give_identical_bits(variant):
    a, b = case(variant)['on'], case(variant)['on2']
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


def test_frozen_batchnorm_chunked_step_with_the_mode_on():
    sd, frames, x, dout = _inputs('r18', 5)
    f64, f32 = fr.frozen_step(sd, x, dout, 'r18', torch.float64), fr.frozen_step(sd, x, dout, 'r18', torch.float32)
    one = _lib_step(sd, 'r18', frames, dout, 5, freeze_bn=True)
    on = _lib_step(sd, 'r18', frames, dout, 2, freeze_bn=True)                  # passes of 2, 2, 1
    off = _lib_step(sd, 'r18', frames, dout, 2, conv16=False, freeze_bn=True)
    assert torch.equal(on[0], one[0]), 'the embeddings of passes of 2, 2, 1 are not those of one pass of 5'
    assert all(torch.equal(on[2][k], off[2][k]) for k in off[2]), 'frozen BatchNorm: a running statistic moved'
    _forward_figures('frozen chunks', (on[0], None, None), (f32[0], None, {}))
    _gradient_figures('frozen chunks', on[1], off[1], f32[1], f64[1])
    both = _lib_step(sd, 'r18', frames, dout, 2, wgrad16=True, freeze_bn=True)
    assert torch.equal(both[0], on[0])
    _gradient_figures('frozen chunks, split weight gradients too', both[1], off[1], f32[1], f64[1])


def test_explicit_off_is_the_handle_that_never_heard_of_the_mode():
    sd, frames, _, dout = _inputs('r18', tg.CASES['r18'])
    off = tg.case('r18')['lib']
    got = _lib_step(sd, 'r18', frames, dout, tg.CASES['r18'], explicit_off=True)
    assert torch.equal(got[0], off[0]) and all(torch.equal(got[1][k], off[1][k]) for k in off[1]) and all(torch.equal(got[2][k], off[2][k]) for k in off[2])
    assert got[3] == E.trainer_workspace_bytes('resnet18', tg.CASES['r18']) < case('r18')['on'][3]
    assert case('r18')['on'][3] == E.trainer_workspace_bytes('resnet18', tg.CASES['r18'], conv_split16=True)


def test_a_late_switch_is_a_state_error():
    sd, frames, _, _ = _inputs('r18', 2)
    m = E.HipTrainableResNet(sd, 'r18', max_batch=2)
    m.train()
    m(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    L = _lib.lib()
    assert L.pvr_trainer_set_conv_split16(m._handle, 1) == 4 and 'before the first forward' in _lib.last_error()      # PVR_ERR_STATE
    with pytest.raises(RuntimeError, match='before the first forward'):
        m.set_conv_split16(True)
    assert not m.conv_split16
    m.set_conv_split16(False)                            # (the mode it has: nothing to change)
    on = E.HipTrainableResNet(sd, 'r18', max_batch=2, conv_split16=True)
    on.train()
    on(torch.from_numpy(frames).cuda())
    assert L.pvr_trainer_set_conv_split16(on._handle, 0) == 4 and 'split-f16' in _lib.last_error()
    assert on.conv_split16


def test_a_trunk_whose_activations_pass_65504_trains():
    """layer1.0.bn1's gamma times 3e5: its output, the input of layer1.0.conv2, reaches about 1e6 - an unscaled f16 high part would be infinite"""
    sd, frames, x, dout = _inputs('r18', 3)
    sd = dict(sd)
    sd['layer1.0.bn1.weight'] = np.asarray(sd['layer1.0.bn1.weight'], dtype=np.float32) * np.float32(3e5)
    t = tr.to_tensors(sd)
    with torch.no_grad():
        x0 = F.max_pool2d(F.relu(tr._cbn(t, 'conv1', 'bn1', x, 2, 3, True)), 3, 2, 1)
        act = F.relu(tr._cbn(t, 'layer1.0.conv1', 'layer1.0.bn1', x0, 1, 1, True))
    assert float(act.max()) > 65504.0
    out, grads, bufs, _ = _lib_step(sd, 'r18', frames, dout, 3)
    ref_out, ref_grads, _ = tr.train_step(sd, x, dout, 'r18', torch.float32)
    print('\n[conv split16 range] largest activation %.3g; embeddings vs the fp32 torch restatement rel-L2 %.2e' % (float(act.max()), tr.rel_l2(out, ref_out)))
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values()) and all(torch.isfinite(b).all() for b in bufs.values())
    assert float(out.abs().max()) > 0 and all(float(g.abs().max()) > 0 for k, g in grads.items() if g.dim() == 4)


def test_surface_embeddingnet_carries_the_mode():
    with pytest.raises(ValueError, match='conv_split16'):
        E.EmbeddingNet('resnet18', pretrained=False, conv_split16=True)
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, conv_split16=True, max_batch=4)
    assert net.training and net.embedding.conv_split16 and not net.embedding.wgrad_split16 and not net.embedding.freeze_bn
    assert net.embedding.workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, conv_split16=True)
    frames = torch.from_numpy(synth.smooth_frames(13, 4, 64, 64))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    a = torch.randn((512,), generator=torch.Generator().manual_seed(5)).cuda() / 512 ** 0.5
    target = torch.randn((4,), generator=torch.Generator().manual_seed(6)).cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = ((net(frames) @ a - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print('\n[conv split16 surface] loss over six Adam steps %s' % ['%.4f' % v for v in losses])
    assert all(np.isfinite(losses)) and losses[5] < losses[0], losses
    # eval mode keeps running the frozen 'f32' plan
    frozen = E.EmbeddingNet('resnet18', pretrained=False, compute_dtype='f32', max_batch=4)
    net.eval()
    frozen.embedding.load_state_dict(net.embedding.state_dict())
    assert np.array_equal(net(frames), frozen(frames))
    net.close()
    frozen.close()


def test_the_driver_flag_reaches_the_handle(tmp_path, monkeypatch):
    from pvr_habitat_amd import main_bc_finetune as Fz
    from pvr_habitat_amd.arguments import make_parser
    n = 12
    fr_ = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(fr_)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))
    made = []
    real_init = E.HipTrainableResNet.__init__

    def recording(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(E.HipTrainableResNet, '__init__', recording)
    flags = make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'e2e'), '--env', 'scene', '--to_env', 'scene',
                                      '--train_embedding', '--embedding_name', 'resnet18', '--disable_pretrained_embedding', '--unroll_length', '2',
                                      '--batch_size', '1', '--eval_frequency', '1', '--max_frames', '4', '--embedding_conv_split16'])
    stats = Fz.run(flags)['scene']
    assert all(np.isfinite(stats['training_loss'][1:])) and all(np.isfinite(stats['gradient_norm'][1:]))
    assert len(made) == 1 and made[0].conv_split16 and not made[0].wgrad_split16 and not made[0].freeze_bn
    assert made[0].workspace_bytes() == E.trainer_workspace_bytes('resnet18', 4, conv_split16=True)
    ck = torch.load(tmp_path / 'e2e' / 'scene_emresnet18_finetuned_s1_scene.tar', weights_only=False)
    assert ck['flags']['embedding_conv_split16'] is True and ck['flags']['embedding_wgrad_split16'] is False
