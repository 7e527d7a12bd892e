"""The kernels of the trainable encoder (csrc/train_kernels.hip) one by one through their pvr_op_* entry points, against the float64 references
and derived elementwise bounds of tests/train_refs.py (pinned on the CPU by tests/test_train_refs_cpu.py), at the smallest shapes at which each
can still go wrong.  Every kernel runs twice and must give identical bits; outputs are NaN before the launch, so a value that is not written shows."""
import ctypes as C

import pytest
import torch

import train_refs as tr
from pvr_habitat_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(t):
    """a device copy; the caller keeps the reference until it has synchronised (a temporary's block would be handed to the next allocation)"""
    return None if t is None else t.contiguous().cuda()


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def scratch(floats):
    assert floats > 0
    return nans(int(floats)), int(floats)


def run_bn_forward(d, res, relu, rows, C_):
    L = _lib.lib()
    z, gamma, beta = dev(d['z']), dev(d['gamma']), dev(d['beta'])
    rm, rv = dev(d['run_mean'].clone()), dev(d['run_var'].clone())
    nbt = torch.tensor([5], dtype=torch.int64, device='cuda')
    y, mean, rstd = nans(rows, C_), nans(C_), nans(C_)
    s, sf = scratch(L.pvr_op_bn_scratch_floats(rows, C_))
    resd = dev(res)
    _lib.check(L.pvr_op_bn_train_forward(vp(z), vp(resd), vp(gamma), vp(beta), vp(rm), vp(rv), vp(nbt), vp(y), vp(mean), vp(rstd), rows, C_, int(relu),
                                         vp(s), sf, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(nbt.item()) == 6
    return dict(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu(), run_mean=rm.cpu(), run_var=rv.cpu())


@pytest.mark.parametrize('rows,C_', tr.BN_SHAPES)
@pytest.mark.parametrize('family', tr.BN_FAMILIES)
@pytest.mark.parametrize('with_res,relu', [(False, False), (False, True), (True, True)])
def test_batchnorm_forward_matches_float64(family, rows, C_, with_res, relu):
    d = tr.bn_inputs(family, rows, C_)
    res = d['res'] if with_res else None
    ref, bound = tr.bn_forward_ref(d['z'], res, d['gamma'], d['beta'], d['run_mean'], d['run_var'], relu)
    got = run_bn_forward(d, res, relu, rows, C_)
    worst = {k: tr.ratio(got[k], ref[k], bound[k]) for k in ref}
    print('\n[bn forward %s %dx%d res %d relu %d] error / bound %s' % (family, rows, C_, with_res, relu, {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    again = run_bn_forward(d, res, relu, rows, C_)
    assert all(torch.equal(got[k], again[k]) for k in got), 'two runs differ'


def run_bn_backward(d, fwd, relu, rows, C_, prev):
    L = _lib.lib()
    dz, dgamma, dbeta = nans(rows, C_), nans(C_), nans(C_)
    dres = dev(prev.clone()) if prev is not None else nans(rows, C_)
    s, sf = scratch(L.pvr_op_bn_scratch_floats(rows, C_))
    z, y, dy, gamma, mean, rstd = (dev(t) for t in (d['z'], fwd['y'], d['dy'], d['gamma'], fwd['mean'], fwd['rstd']))     # (held until the sync below)
    _lib.check(L.pvr_op_bn_train_backward(vp(z), vp(y), vp(dy), vp(gamma), vp(mean), vp(rstd),
                                          vp(dz), vp(dres), 1 if prev is not None else 0, vp(dgamma), vp(dbeta), rows, C_, int(relu), vp(s), sf,
                                          _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dict(dz=dz.cpu(), dres=dres.cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu())


@pytest.mark.parametrize('rows,C_', tr.BN_SHAPES)
@pytest.mark.parametrize('family', tr.BN_FAMILIES)
@pytest.mark.parametrize('with_res,relu', [(False, False), (False, True), (True, True)])
def test_batchnorm_backward_matches_float64(family, rows, C_, with_res, relu):
    d = tr.bn_inputs(family, rows, C_)
    fwd = tr.bn_forward(d['z'], d['res'] if with_res else None, d['gamma'], d['beta'], d['run_mean'], d['run_var'], relu)     # fp32 inputs of the backward
    prev = d['prev'] if with_res else None              # with a residual the branch gradient accumulates; without, dres is the masked dy itself
    ref, bound = tr.bn_backward_ref(d['z'], fwd['y'], d['dy'], d['gamma'], fwd['mean'], fwd['rstd'], relu, prev=prev)
    got = run_bn_backward(d, fwd, relu, rows, C_, prev)
    worst = {k: tr.ratio(got[k], ref[k], bound[k]) for k in ref}
    print('\n[bn backward %s %dx%d res %d relu %d] error / bound %s' % (family, rows, C_, with_res, relu, {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    again = run_bn_backward(d, fwd, relu, rows, C_, prev)
    assert all(torch.equal(got[k], again[k]) for k in got), 'two runs differ'


def run_wgrad(x, dz, geo):
    n, h, ci, co, k, s, p = geo
    L = _lib.lib()
    dw = nans(co, ci, k, k)
    sc, sf = scratch(L.pvr_op_conv_wgrad_scratch_floats(n, h, h, ci, co, k, s, p))
    xd, dzd = dev(x), dev(dz)
    _lib.check(L.pvr_op_conv_wgrad(vp(xd), vp(dzd), vp(dw), n, h, h, ci, co, k, s, p, vp(sc), sf, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize('geo', tr.CONV_GEOMETRIES)
def test_weight_gradient_matches_float64(geo):
    n, h, ci, co, k, s, p = geo
    x, dz, _ = tr.conv_inputs(*geo)
    ref, bound = tr.wgrad_ref(x, dz, k, s, p)
    got = run_wgrad(x, dz, geo)
    r = tr.ratio(got, ref, bound)
    print('\n[wgrad %s] error / bound %.3f' % (geo, r))
    assert r <= 1.0
    assert torch.equal(got, run_wgrad(x, dz, geo)), 'two runs differ'


def run_dgrad(dz, wt, geo, prev):
    n, h, ci, co, k, s, p = geo
    L = _lib.lib()
    dx = dev(prev.clone()) if prev is not None else nans(n, h, h, ci)
    sc, sf = scratch(L.pvr_op_conv_dgrad_scratch_floats(n, h, h, ci, co, k, s, p))
    dzd, wtd = dev(dz), dev(wt)
    _lib.check(L.pvr_op_conv_dgrad(vp(dzd), vp(wtd), vp(dx), 1 if prev is not None else 0, n, h, h, ci, co, k, s, p, vp(sc), sf, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dx.cpu()


@pytest.mark.parametrize('geo', tr.CONV_GEOMETRIES + [tr.DGRAD_LONG_K])
@pytest.mark.parametrize('accumulate', [False, True])
def test_data_gradient_matches_float64(geo, accumulate):
    n, h, ci, co, k, s, p = geo
    _, dz, wt = tr.conv_inputs(*geo)
    prev = torch.randn((n, h, h, ci), generator=torch.Generator().manual_seed(4)) if accumulate else None
    ref, bound = tr.dgrad_ref(dz, wt, h, k, s, p, prev)
    got = run_dgrad(dz, wt, geo, prev)
    r = tr.ratio(got, ref, bound)
    print('\n[dgrad %s accumulate %d] error / bound %.3f' % (geo, accumulate, r))
    assert r <= 1.0
    assert torch.equal(got, run_dgrad(dz, wt, geo, prev)), 'two runs differ'


def test_data_gradient_refuses_an_odd_size_at_stride_2():
    L = _lib.lib()
    t = nans(16)
    assert L.pvr_op_conv_dgrad_scratch_floats(2, 7, 7, 64, 64, 3, 2, 1) == 0
    assert L.pvr_op_conv_dgrad(vp(t), vp(t), vp(t), 0, 2, 7, 7, 64, 64, 3, 2, 1, vp(t), 1 << 30, _lib.stream_ptr()) == 1
    assert 'odd' in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.isnan(t).all(), 'a refused call launched something'


def test_stem_weight_gradient_matches_float64():
    n, S = 2, 32
    img, dz = tr.stem_inputs(n, S)
    ref, bound = tr.stem_wgrad_ref(img, dz)
    L = _lib.lib()

    def run():
        dw = nans(64, 3, 7, 7)
        sc, sf = scratch(L.pvr_op_stem_wgrad_scratch_floats(n, S))
        imgd, dzd = dev(img), dev(dz)
        _lib.check(L.pvr_op_stem_wgrad(vp(imgd), vp(dzd), vp(dw), n, S, vp(sc), sf, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return dw.cpu()
    got = run()
    r = tr.ratio(got, ref, bound)
    print('\n[stem wgrad] error / bound %.3f' % r)
    assert r <= 1.0
    assert torch.equal(got, run()), 'two runs differ'


def test_maxpool_backward_ties_and_zero_windows():
    x, dy = tr.maxpool_inputs()
    ref, bound = tr.maxpool_backward_ref(x, dy)

    def run():
        dx = nans(*x.shape)
        xd, dyd = dev(x), dev(dy)
        _lib.check(_lib.lib().pvr_op_maxpool_backward(vp(xd), vp(dyd), vp(dx), x.shape[0], x.shape[1], x.shape[2], x.shape[3], _lib.stream_ptr()))
        torch.cuda.synchronize()
        return dx.cpu()
    got = run()
    assert tr.ratio(got, ref, bound) <= 1.0
    assert torch.equal(got, run()), 'two runs differ'


def test_avgpool_backward():
    n, hw, c, stride = 2, 49, 512, 520                 # resnet18's pool; rows of dout 520 floats apart
    dout = torch.randn((n, stride), generator=torch.Generator().manual_seed(6))
    ref, bound = tr.avgpool_backward_ref(dout[:, :c], hw)

    def run():
        dx = nans(n, hw, c)
        doutd = dev(dout)
        _lib.check(_lib.lib().pvr_op_avgpool_backward(vp(doutd), stride, vp(dx), n, hw, c, _lib.stream_ptr()))
        torch.cuda.synchronize()
        return dx.cpu()
    got = run()
    assert tr.ratio(got, ref, bound) <= 1.0
    assert torch.equal(got, run()), 'two runs differ'
