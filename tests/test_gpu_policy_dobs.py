"""d(loss)/d(obs) of the vector policy on the GPU (pvr_policy_backward_dobs, pvr_policy_backward_dlogits_dobs), its autograd bridge, and the joint
clip + RMSprop over several flat buffers (pvr_joint_apply_rmsprop).

Gradients follow the acceptance rule of tests/test_gpu_train.py: the float64 gradient, torch's fp32 gradient and the library's gradient of the same
inputs, and rel_l2(library, float64) <= 8 x rel_l2(torch fp32, float64); both figures are printed.  The references (tests/policy_dobs_refs.py) are
computed once per case and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
from pvr_habitat_amd import _lib
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

ENTRIES = ('loss', 'dlogits')
_refs, _runs = {}, {}
vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def refs(case):
    if case not in _refs:
        T, B, O, bn = case
        sd = R.policy_params(7, O, bn)
        obs, done, act = R.inputs(11 + O, T, B, O)
        _refs[case] = dict(sd=sd, obs=obs, done=done, act=act, f64=R.dobs_autograd(sd, obs, done, act, bn, torch.float64),
                           f32=R.dobs_autograd(sd, obs, done, act, bn, torch.float32))
    return _refs[case]


def _policy(case):
    T, B, O, bn = case
    m = M.PolicyNet((O,), R.A, bool(bn), max_unroll=T, max_batch=B)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in refs(case)['sd'].items()})
    m = m.to(device='cuda')
    m.train()
    m._ensure(T, B)
    return m


def _backward(m, case, entry, mode):
    """one backward through an entry point.  mode 'old': the existing call; 'null': the new call with dobs == NULL; 'dobs': the new call.
    -> (grads, dobs or None), on the host"""
    T, B, O, bn = case
    r = refs(case)
    L = M._plib()
    x = torch.flatten(r['obs'], 0, 1).cuda().contiguous()
    d = r['done'].to(torch.uint8).cuda()
    a = r['act'].cuda()
    g = torch.zeros(m._n_train, device='cuda')                   # (the flat layout pads every tensor to 4 floats: the pad slots are never written)
    dobs = torch.full((T * B, O), float('nan'), device='cuda') if mode == 'dobs' else None
    bns = m._bn_struct()
    bnp = C.byref(bns) if bns else None
    if entry == 'loss':
        if mode == 'old':
            st = L.pvr_policy_backward(m._handle, vp(m._flat), bnp, vp(x), vp(d), vp(a), T, B, vp(g), None, None, _lib.stream_ptr())
        else:
            st = L.pvr_policy_backward_dobs(m._handle, vp(m._flat), bnp, vp(x), vp(d), vp(a), T, B, vp(g), None, None, vp(dobs), _lib.stream_ptr())
    else:
        logits = m._forward_raw(x, d, None, None, T, B, True)[0].requires_grad_(True)
        R.nll(logits, a).backward()
        dl = logits.grad.contiguous()
        if mode == 'old':
            st = L.pvr_policy_backward_dlogits(m._handle, vp(m._flat), vp(x), vp(dl), T, B, vp(g), _lib.stream_ptr())
        else:
            st = L.pvr_policy_backward_dlogits_dobs(m._handle, vp(m._flat), vp(x), vp(dl), T, B, vp(g), vp(dobs), _lib.stream_ptr())
    _lib.check(st)
    torch.cuda.synchronize()
    return g.cpu(), None if dobs is None else dobs.cpu().view(T, B, O)


def runs(case, entry):
    """old call, new call with NULL, two new calls with dobs: once per (case, entry point)"""
    if (case, entry) not in _runs:
        m = _policy(case)
        _runs[(case, entry)] = {k: _backward(m, case, entry, k.rstrip('2')) for k in ('old', 'null', 'dobs', 'dobs2')}
        m.close()
    return _runs[(case, entry)]


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', R.CASES, ids=str)
def test_dobs_against_float64(case, entry):
    r = refs(case)
    g, dobs = runs(case, entry)['dobs']
    assert dobs.shape == r['f64'][0].shape and torch.isfinite(dobs).all() and torch.isfinite(g).all()
    ok, d, d32 = R.accept(dobs, r['f32'][0], r['f64'][0])
    print('\n[dobs %s %s] rel-L2 to float64: library %.3e, torch fp32 %.3e (ratio %.2f)' % (case, entry, d, d32, d / d32))
    assert ok, (d, d32)


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', [c for c in R.CASES if c[3]] + [(3, 2, 128, 0)], ids=str)
def test_asking_for_dobs_does_not_change_a_bit_of_grads(case, entry):
    r = runs(case, entry)
    assert torch.isfinite(r['old'][0]).all()
    assert torch.equal(r['dobs'][0], r['old'][0]), 'grads of the _dobs call differ from the existing call'
    assert torch.equal(r['null'][0], r['old'][0]), 'dobs == NULL through the new entry point differs from the existing call'
    assert torch.equal(r['dobs2'][0], r['dobs'][0]) and torch.equal(r['dobs2'][1], r['dobs'][1]), 'two _dobs runs differ'


def _status_both(m, T, B, O):
    """status of both new entry points on a handle that must refuse dobs (device buffers are valid; nothing is enqueued by a refusal)"""
    L = M._plib()
    dev = 'cpu' if m._host else 'cuda'
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    x = z(T * B, 64, 64, 6, dt=torch.uint8) if m._conv_frames else z(T * B, O)
    d, a, g, dobs, dl = z(T, B, dt=torch.uint8), z(T, B, dt=torch.int64), z(m._n_train), z(T * B, O), z(T, B, R.A)
    st = None if m._host else _lib.stream_ptr()
    bns = m._bn_struct()
    s1 = L.pvr_policy_backward_dobs(m._handle, vp(m._flat), C.byref(bns) if bns else None, vp(x), vp(d), vp(a), T, B, vp(g), None, None, vp(dobs), st)
    e1 = _lib.last_error()
    s2 = L.pvr_policy_backward_dlogits_dobs(m._handle, vp(m._flat), vp(x), vp(dl), T, B, vp(g), vp(dobs), st)
    e2 = _lib.last_error()
    return (s1, e1), (s2, e2)


def test_refusals():
    T, B = 3, 2
    conv = M.PolicyNetWithConv((64, 64, 6), R.A, True, max_unroll=T, max_batch=B).to(device='cuda')
    conv._ensure(T, B)
    for s, e in _status_both(conv, T, B, 256):
        assert s == 1 and 'uint8' in e and 'conv_frames' in e, (s, e)
    conv.close()
    host = M.PolicyNet((128,), R.A, True, max_unroll=T, max_batch=B).use_host_backend(True)
    host._ensure(T, B)
    for s, e in _status_both(host, T, B, 128):
        assert s == 1 and 'host' in e, (s, e)
    host.close()
    dp = M.PolicyNet((128,), R.A, True, max_unroll=T, max_batch=B).to(device='cuda')
    dp._ensure(T, B)
    calls = []
    stub = M.ALLREDUCE_FN(lambda buf, count, stream, user: calls.append(count) or 0)
    _lib.check(M._plib().pvr_policy_set_data_parallel(dp._handle, 2, 0, stub, None))
    try:
        for s, e in _status_both(dp, T, B, 128):
            assert s == 1 and 'data-parallel' in e, (s, e)
        assert not calls                                           # refused before anything was enqueued
    finally:
        _lib.check(M._plib().pvr_policy_set_data_parallel(dp._handle, 1, 0, M.ALLREDUCE_FN(), None))
        dp.close()


def _counting(monkeypatch):
    L, counts = M._plib(), {}
    for name in ('pvr_policy_backward_dlogits', 'pvr_policy_backward_dlogits_dobs'):
        fn = getattr(L, name)
        counts[name] = 0

        def wrapped(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(L, name, wrapped)
    return counts


@pytest.mark.parametrize('case', [(3, 2, 128, 1), (3, 2, 72, 0)], ids=str)
def test_autograd_bridge_returns_the_entry_points_gradient(case, monkeypatch):
    T, B, O, bn = case
    r = refs(case)
    counts = _counting(monkeypatch)
    m = _policy(case)
    obs = r['obs'].cuda().requires_grad_(True)
    done, act = r['done'].cuda(), r['act'].cuda()
    out, _ = m(dict(obs=obs, done=done), m.initial_state(B))
    logits = out['policy_logits']
    logits.retain_grad()
    R.nll(logits, act).backward()
    assert counts == {'pvr_policy_backward_dlogits': 0, 'pvr_policy_backward_dlogits_dobs': 1}
    assert obs.grad is not None and obs.grad.shape == obs.shape
    # the entry point by hand on the same upstream gradient
    L = M._plib()
    x = torch.flatten(obs.detach(), 0, 1).contiguous()
    m._forward_raw(x, done.to(torch.uint8), None, None, T, B, True)
    g, dobs = torch.empty(m._n_train, device='cuda'), torch.empty((T * B, O), device='cuda')
    _lib.check(L.pvr_policy_backward_dlogits_dobs(m._handle, vp(m._flat), vp(x), vp(logits.grad.contiguous()), T, B, vp(g), vp(dobs), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(obs.grad.view(T * B, O), dobs)
    grads_with = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    for k, (o, shp) in m._slots.items():                          # (tensor by tensor: the flat layout's pad slots are never written)
        if o < m._n_train:
            n = int(np.prod(shp))
            assert torch.equal(m._last_flat_grad[o:o + n], g[o:o + n]), k
    # without a graph on obs: today's call, and the same parameter gradient bit for bit
    for p in m.parameters():
        p.grad = None
    out, _ = m(dict(obs=obs.detach(), done=done), m.initial_state(B))
    R.nll(out['policy_logits'], act).backward()
    assert counts == {'pvr_policy_backward_dlogits': 1, 'pvr_policy_backward_dlogits_dobs': 2}     # (2: the by-hand call above)
    grads_without = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert sorted(grads_with) == sorted(grads_without) and all(torch.equal(grads_with[k], grads_without[k]) for k in grads_with)
    m.close()


def _joint_run(p0, grads, lr, alpha, eps, max_norm):
    L = M._plib()
    ps = [p.clone().cuda() for p in p0]
    vs = [torch.zeros_like(p) for p in ps]
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    counts = (C.c_int64 * len(ps))(*[p.numel() for p in ps])
    norms = []
    for gs in grads:
        gd = [g.cuda() for g in gs]
        stat = torch.zeros(1, device='cuda')
        _lib.check(L.pvr_joint_apply_rmsprop(len(ps), arr(ps), arr(vs), arr(gd), counts, lr, alpha, eps, max_norm, vp(stat), _lib.stream_ptr()))
        torch.cuda.synchronize()
        norms.append(float(stat))
    return [p.cpu() for p in ps], [v.cpu() for v in vs], norms


def test_joint_apply_rmsprop_equals_clip_grad_norm_and_torch_rmsprop():
    gen = torch.Generator().manual_seed(3)
    sizes, lr, alpha, eps, max_norm = (4000, 144), 1e-3, 0.99, 1e-5, 40.0
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    # norms about 64 x scale: above max_grad_norm, below it, above it
    grads = [[torch.randn(n, generator=gen) * s for n in sizes] for s in (2.0, 0.1, 5.0)]
    ref_p = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.RMSprop(ref_p, lr=lr, alpha=alpha, eps=eps, momentum=0)
    ref_norms = []
    for gs in grads:
        for p, g in zip(ref_p, gs):
            p.grad = g.clone()
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_(ref_p, max_norm)))
        opt.step()
    assert ref_norms[0] > max_norm > ref_norms[1] and ref_norms[2] > max_norm, ref_norms
    ps, vs, norms = _joint_run(p0, grads, lr, alpha, eps, max_norm)
    print('\n[joint rmsprop] norms %s, torch %s' % (norms, ref_norms))
    for n, rn in zip(norms, ref_norms):
        assert n == pytest.approx(rn, rel=1e-5)
    for p, rp in zip(ps, ref_p):
        np.testing.assert_allclose(p.numpy(), rp.detach().numpy(), rtol=2e-4, atol=2e-6)
    ps2, vs2, norms2 = _joint_run(p0, grads, lr, alpha, eps, max_norm)
    assert norms2 == norms and all(torch.equal(a, b) for a, b in zip(ps + vs, ps2 + vs2))


def test_joint_apply_rmsprop_refuses_bad_arguments():
    L = M._plib()
    t = torch.zeros(8, device='cuda')
    one = (C.c_void_p * 1)(t.data_ptr())
    off = (C.c_void_p * 1)(t.data_ptr() + 4)
    assert L.pvr_joint_apply_rmsprop(1, one, one, one, (C.c_int64 * 1)(6), 1e-3, 0.99, 1e-5, 40.0, None, _lib.stream_ptr()) == 1
    assert 'multiple of 4' in _lib.last_error()
    assert L.pvr_joint_apply_rmsprop(1, off, one, one, (C.c_int64 * 1)(4), 1e-3, 0.99, 1e-5, 40.0, None, _lib.stream_ptr()) == 1
    assert 'aligned' in _lib.last_error()
    assert L.pvr_joint_apply_rmsprop(9, one, one, one, (C.c_int64 * 1)(4), 1e-3, 0.99, 1e-5, 40.0, None, _lib.stream_ptr()) == 1
