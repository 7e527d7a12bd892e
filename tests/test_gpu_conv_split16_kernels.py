"""The split-f16 forward convolution and data gradient (csrc/conv_split16_scaled.hip) through pvr_op_conv_fwd_split16 / pvr_op_conv_dgrad_split16,
against the float64 references and the derived elementwise bound of tests/conv_split16_refs.py (pinned on the CPU by tests/test_conv_split16_cpu.py), at
train_refs.CONV_GEOMETRIES (147 pixels: no multiple of a tile, stride 2, borders), train_refs.DGRAD_LONG_K (K = 4608) and
wgrad_split16_refs.EXTRA_GEOMETRIES (several tiles both ways, partial cout tiles, a half-empty channel tile) in every family, and at three larger
geometries where the launch takes its 128-pixel tiles.  Outputs are NaN before the launch, so a value that is not written shows; every launch runs
twice and must give the same bits; a refused call must leave its output untouched."""
import ctypes as C

import pytest
import torch

import conv_split16_refs as cs
import train_refs as tr
from pvr_habitat_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

# 32768 and 33800 output pixels: at least one 128-pixel tile per compute unit, where the launch switches from its 64-pixel to its 128-pixel tiles.
# forward / data gradient run the (128 pixels x 128 rows, 128 x 64), (128 x 64, 128 x 128) and, with 3x3 borders and a pixel tail, (128 x 64, 128 x 64) kernels
BIG_GEOMETRIES = [(8, 64, 32, 128, 1, 1, 0), (8, 64, 128, 32, 1, 1, 0), (2, 130, 32, 64, 3, 1, 1)]

_refs = {}


def case(family, geo):
    """inputs, float64 references and bounds of one (family, geometry), computed once and left unchanged"""
    if (family, geo) not in _refs:
        n, h, ci, co, k, s, p = geo
        x, dz, wt = cs.inputs(family, geo)
        prev = cs.prev_of(geo)
        _refs[(family, geo)] = dict(x=x, dz=dz, wt=wt, prev=prev, fwd=cs.fwd_reference(x, wt, k, s, p), dgrad=cs.dgrad_reference(dz, wt, h, k, s, p),
                                    dgrad_acc=cs.dgrad_reference(dz, wt, h, k, s, p, prev))
    return _refs[(family, geo)]


def vp(t):
    return C.c_void_p(t.data_ptr())


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def scales_of(a_dev, w_dev):
    """the two device scales, by the one-launch pair form the trainer uses"""
    s = nans(2)
    aux = torch.zeros(4, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().pvr_op_absmax_scale_pair(vp(a_dev), a_dev.numel(), vp(s[0:1]), vp(w_dev), w_dev.numel(), vp(s[1:2]), vp(aux), _lib.stream_ptr()))
    return s


def run_fwd(x, wt, geo):
    n, h, ci, co, k, s, p = geo
    L = _lib.lib()
    ho = tr.out_size(h, k, s, p)
    z = nans(n, ho, ho, co)
    floats = int(L.pvr_op_conv_fwd_split16_scratch_floats(n, h, h, ci, co, k, s, p))
    assert floats > 0
    sc = nans(floats)
    xd, wd = x.contiguous().cuda(), wt.contiguous().cuda()
    sl = scales_of(xd, wd)
    _lib.check(L.pvr_op_conv_fwd_split16(vp(xd), vp(wd), vp(z), n, h, h, ci, co, k, s, p, vp(sl[0:1]), vp(sl[1:2]), vp(sc), floats, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return z.cpu()


def run_dgrad(dz, wt, geo, prev=None):
    n, h, ci, co, k, s, p = geo
    L = _lib.lib()
    dx = nans(n, h, h, ci) if prev is None else prev.contiguous().cuda()
    floats = int(L.pvr_op_conv_dgrad_split16_scratch_floats(n, h, h, ci, co, k, s, p))
    assert floats > 0
    sc = nans(floats)
    dzd, wd = dz.contiguous().cuda(), wt.contiguous().cuda()
    sl = scales_of(dzd, wd)
    _lib.check(L.pvr_op_conv_dgrad_split16(vp(dzd), vp(wd), vp(dx), 0 if prev is None else 1, n, h, h, ci, co, k, s, p, vp(sl[0:1]), vp(sl[1:2]), vp(sc), floats,
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    return dx.cpu()


def check_fwd(geo, family):
    c = case(family, geo)
    got = run_fwd(c['x'], c['wt'], geo)
    assert not torch.isnan(got).any(), 'z is not fully written'
    r = tr.ratio(got, *c['fwd'])
    print('\n[conv split16 forward %s %s] error / bound %.3f' % (geo, family, r))
    assert r <= 1.0
    assert torch.equal(got, run_fwd(c['x'], c['wt'], geo)), 'two runs differ'


def check_dgrad(geo, family, accumulate):
    c = case(family, geo)
    prev = c['prev'] if accumulate else None
    got = run_dgrad(c['dz'], c['wt'], geo, prev)
    assert not torch.isnan(got).any(), 'dx is not fully written'
    r = tr.ratio(got, *c['dgrad_acc' if accumulate else 'dgrad'])
    print('\n[conv split16 data gradient %s %s accumulate %d] error / bound %.3f' % (geo, family, accumulate, r))
    assert r <= 1.0
    assert torch.equal(got, run_dgrad(c['dz'], c['wt'], geo, prev)), 'two runs differ'


@pytest.mark.parametrize('geo', cs.GEOMETRIES)
@pytest.mark.parametrize('family', cs.FAMILIES)
def test_forward_matches_float64(geo, family):
    check_fwd(geo, family)


@pytest.mark.parametrize('geo', cs.GEOMETRIES)
@pytest.mark.parametrize('family', cs.FAMILIES)
@pytest.mark.parametrize('accumulate', [0, 1])
def test_data_gradient_matches_float64(geo, family, accumulate):
    check_dgrad(geo, family, accumulate)


@pytest.mark.parametrize('geo', BIG_GEOMETRIES)
@pytest.mark.parametrize('family', ['unit', 'large'])
def test_the_128_pixel_tiles(geo, family):
    check_fwd(geo, family)
    check_dgrad(geo, family, 1)


def test_the_refusals_launch_nothing():
    L = _lib.lib()
    st = _lib.stream_ptr()
    a, s, sc = torch.ones(2 * 8 * 8 * 64, device='cuda'), torch.ones(2, device='cuda'), nans(1 << 16)
    out = nans(2 * 8 * 8 * 64)
    big = sc.numel()
    for args in ((2, 8, 8, 48, 64, 3, 1, 1), (2, 8, 8, 64, 62, 3, 1, 1), (2, 8, 8, 64, 64, 5, 1, 2), (2, 8, 8, 64, 64, 3, 3, 1)):
        assert L.pvr_op_conv_fwd_split16(vp(a), vp(a), vp(out), *args, vp(s[0:1]), vp(s[1:2]), vp(sc), big, st) == 1, args
    assert L.pvr_op_conv_fwd_split16(vp(a), vp(a), vp(out), 2, 8, 8, 64, 64, 3, 1, 1, vp(s[0:1]), vp(s[1:2]), vp(sc), 16, st) == 1 and 'scratch' in _lib.last_error()
    assert L.pvr_op_conv_fwd_split16(vp(a), vp(a), vp(out), 2, 8, 8, 64, 64, 3, 1, 1, None, vp(s[1:2]), vp(sc), big, st) == 1 and 'scale' in _lib.last_error()
    for args in ((2, 8, 8, 64, 48, 3, 1, 1), (2, 8, 8, 62, 64, 3, 1, 1), (2, 8, 8, 64, 64, 3, 1, 0), (2, 7, 7, 64, 64, 3, 2, 1)):
        assert L.pvr_op_conv_dgrad_split16(vp(a), vp(a), vp(out), 0, *args, vp(s[0:1]), vp(s[1:2]), vp(sc), big, st) == 1, args
    assert L.pvr_op_conv_dgrad_split16(vp(a), vp(a), vp(out), 0, 2, 8, 8, 64, 64, 3, 2, 1, vp(s[0:1]), vp(s[1:2]), vp(sc), 64 * 9 * 64, st) == 1 \
        and 'scratch' in _lib.last_error()                              # (the weights fit, the zero-filled grid does not)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(sc).all(), 'a refused call wrote something'
