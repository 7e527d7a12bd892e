"""The trainable encoder end to end (EmbeddingNet(..., train=True), include/pvr_train.h) on the GPU: forward, running statistics and gradients of
resnet18 / resnet50 against the train-mode torch restatement of tests/train_refs.py, reproducibility, and the Python surface (autograd,
state_dict, eval mode, optimizers).

Gradients have no absolute bound: a training-mode network puts many pre-activations near zero and an fp32 forward flips some ReLU masks against
float64, so torch's own fp32 gradient sits 7e-4 (resnet18, 2 frames) ... 8e-3 (resnet50, 2 frames) from its float64 gradient.  The test computes the
float64 gradient, torch's fp32 gradient and the library's in the same run and asserts dist(library, float64) <= 8 x dist(torch fp32, float64) on
the concatenated gradient - the margin tests/test_gpu_vit_f32.py gives two fp32 evaluations in different orders; a wiring error moves the
gradient by order 1.  The sharp arithmetic check is tests/test_gpu_train_kernels.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_refs as tr
from oracle import encoder_oracle as eo
from pvr_habitat_amd import synth
from pvr_habitat_amd import embeddings as E

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

CASES = {'r18': 3, 'conv5': 2}          # variant -> frames
_cache = {}


def _lib_step(sd, variant, frames, dout):
    m = E.HipTrainableResNet(sd, variant, max_batch=frames.shape[0])
    m.train()
    for p in m.parameters():
        p.requires_grad = True
    out = m(torch.from_numpy(frames).cuda())
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    bufs = {k: v.detach().cpu() for k, v in m.state_dict().items() if k.endswith(('running_mean', 'running_var'))}
    nbt = {k: int(v) for k, v in m.state_dict().items() if k.endswith('num_batches_tracked')}
    return out.detach().cpu(), grads, bufs, nbt


def case(variant):
    """references and two library runs of one case, computed once and shared by the tests below"""
    if variant not in _cache:
        n = CASES[variant]
        sd = synth.resnet50_state_dict(3, variant)
        frames = synth.smooth_frames(11, n, 64, 64)
        x = eo.preprocess(frames)
        dout = torch.randn((n, E.OUT_SIZE[variant]), generator=torch.Generator().manual_seed(17)) / n
        _cache[variant] = dict(f64=tr.train_step(sd, x, dout, variant, torch.float64), f32=tr.train_step(sd, x, dout, variant, torch.float32),
                               lib=_lib_step(sd, variant, frames, dout), lib2=_lib_step(sd, variant, frames, dout))
    return _cache[variant]


def _cat(d, keys):
    return torch.cat([d[k].double().flatten() for k in keys])


@pytest.mark.parametrize('variant', list(CASES))
def test_forward_and_running_statistics(variant):
    c = case(variant)
    out, _, bufs, nbt = c['lib']
    ref_out, _, ref_bufs = c['f32']
    keys = sorted(ref_bufs)
    assert sorted(bufs) == keys and all(v == 1 for v in nbt.values()) and len(nbt) == len(keys) // 2
    figures = dict(out_l2=tr.rel_l2(out, ref_out), out_max=tr.max_rel(out, ref_out), buf_l2=tr.rel_l2(_cat(bufs, keys), _cat(ref_bufs, keys)),
                   buf_max=tr.max_rel(_cat(bufs, keys), _cat(ref_bufs, keys)))
    print('\n[train forward %s] vs the fp32 torch restatement: %s' % (variant, {k: '%.2e' % v for k, v in figures.items()}))
    print('[train forward %s] torch fp32 vs float64: out %.2e, buffers %.2e' % (variant, tr.rel_l2(ref_out, c['f64'][0]),
                                                                                tr.rel_l2(_cat(ref_bufs, keys), _cat(c['f64'][2], keys))))
    assert torch.isfinite(out).all() and max(figures.values()) < 1e-4, figures


@pytest.mark.parametrize('variant', list(CASES))
def test_gradients_against_float64_and_torch_fp32(variant):
    c = case(variant)
    g64, g32, glib = c['f64'][1], c['f32'][1], c['lib'][1]
    keys = sorted(g64)
    assert sorted(glib) == keys
    assert all(glib[k].shape == g64[k].shape and torch.isfinite(glib[k]).all() for k in keys)
    d_lib, d_t32 = tr.rel_l2(_cat(glib, keys), _cat(g64, keys)), tr.rel_l2(_cat(g32, keys), _cat(g64, keys))
    worst_lib = max(keys, key=lambda k: tr.rel_l2(glib[k], g64[k]))
    worst_t32 = max(keys, key=lambda k: tr.rel_l2(g32[k], g64[k]))
    print('\n[train gradients %s] concatenated rel-L2 to float64: library %.3e, torch fp32 %.3e (ratio %.2f)' % (variant, d_lib, d_t32, d_lib / d_t32))
    print('[train gradients %s] worst tensor: library %s %.3e, torch fp32 %s %.3e' % (variant, worst_lib, tr.rel_l2(glib[worst_lib], g64[worst_lib]),
                                                                                   worst_t32, tr.rel_l2(g32[worst_t32], g64[worst_t32])))
    assert d_lib <= 8.0 * d_t32, (d_lib, d_t32)


@pytest.mark.parametrize('variant', list(CASES))
def test_two_runs_give_identical_bits(variant):
    a, b = case(variant)['lib'], case(variant)['lib2']
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])


# ------------------------------------------------------------------------------------------------------------------
# the Python surface
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net():
    return E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=4)


def _frames(n, seed=11):
    return torch.from_numpy(synth.smooth_frames(seed, n, 64, 64))


def test_surface_forward_and_backward(net):
    assert net.training and net.embedding.training
    out = net(_frames(3))
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.shape == (3, 512) and out.requires_grad and out.grad_fn is not None
    out.square().mean().backward()
    for k, p in net.embedding.named_parameters():
        assert p.is_cuda and p.requires_grad and p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), k
    one = net(_frames(1))
    assert one.shape == (512,) and one.requires_grad
    stale = net(_frames(2))
    net(_frames(2))
    with pytest.raises(RuntimeError, match='later training-mode forward'):
        stale.sum().backward()
    with pytest.raises(ValueError, match='max_batch'):
        net(_frames(5))


def test_surface_state_dict_and_eval(net):
    frozen = E.EmbeddingNet('resnet18', pretrained=False, compute_dtype='f32', max_batch=4)
    assert list(net.state_dict()) == list(frozen.state_dict())
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(net.state_dict().values(), frozen.state_dict().values()))
    net(_frames(3))                                   # moves the running statistics away from their start
    net.eval()
    try:
        assert not net.embedding.training
        got = net(_frames(3, seed=12))
        assert isinstance(got, np.ndarray) and got.shape == (3, 512) and got.dtype == np.float32
        frozen.embedding.load_state_dict(net.embedding.state_dict())
        assert np.array_equal(got, frozen(_frames(3, seed=12)))
    finally:
        net.train()
    assert net.embedding.training and net(_frames(2)).requires_grad


def test_a_frozen_net_in_train_mode_still_returns_checked_numpy_rows():
    """only the trainable module has a training mode: .train() on a frozen EmbeddingNet (a parent module's .train() reaches it) changes nothing"""
    frozen = E.EmbeddingNet('resnet18', pretrained=False, compute_dtype='f32', max_batch=4)
    want = frozen(_frames(2))
    frozen.train()
    assert frozen.embedding.training
    got = frozen(_frames(2))
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)


def test_surface_optimizer_steps_the_flat_buffer(net):
    fr = _frames(4, seed=13)
    opt = torch.optim.SGD(net.parameters(), lr=0.01)
    a = torch.randn((512,), generator=torch.Generator().manual_seed(5)).cuda() / 512 ** 0.5
    target = torch.randn((4,), generator=torch.Generator().manual_seed(6)).cuda()
    losses = []
    for step in range(6):
        opt.zero_grad()
        out = net(fr)
        if step == 1:                                 # the forward after one optimizer step read the stepped parameters
            want = tr.features(tr.to_tensors(sd_before_forward), eo.preprocess(fr.numpy()), 'r18', True).flatten(1)
            figures = (tr.rel_l2(out.detach().cpu(), want), tr.max_rel(out.detach().cpu(), want))
            print('\n[train after one SGD step] vs the fp32 torch restatement on the stepped parameters: rel-L2 %.2e, max-norm %.2e' % figures)
            assert max(figures) < 1e-4, figures
        loss = ((out @ a - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
        sd_before_forward = {k: v.detach().cpu().clone() for k, v in net.embedding.state_dict().items()}
    print('[train five SGD steps] loss %s' % ['%.4f' % v for v in losses])
    assert losses[5] < losses[0], losses


def test_frozen_f16_bits_do_not_depend_on_a_trainable_net_in_the_process():
    """a fresh process: the frozen f16 resnet18 before any trainable net exists, a training step, the frozen net again"""
    script = ("import torch, hashlib\n"
              "from pvr_habitat_amd import synth, embeddings as E\n"
              "fr = torch.from_numpy(synth.smooth_frames(11, 3, 64, 64))\n"
              "h = lambda: hashlib.sha256(E.EmbeddingNet('resnet18', pretrained=False, compute_dtype='f16', max_batch=4)(fr).tobytes()).hexdigest()\n"
              "before = h()\n"
              "net = E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=4)\n"
              "net(fr).sum().backward()\n"
              "torch.cuda.synchronize()\n"
              "print('SAME' if h() == before else 'DIFFERENT')\n")
    r = subprocess.run([sys.executable, '-c', script], capture_output=True, text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == 'SAME', r.stdout
