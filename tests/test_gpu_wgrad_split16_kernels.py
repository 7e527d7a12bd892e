"""The split-f16 weight-gradient kernels (csrc/wgrad_split16.hip) one by one through their pvr_op_* entry points, against the float64 reference and the
derived elementwise bound of tests/wgrad_split16_refs.py (pinned on the CPU by tests/test_wgrad_split16_cpu.py), at the geometries of
train_refs.CONV_GEOMETRIES: a pixel count that is no multiple of a tile (147), a split over more than one workgroup (196), stride 2, partial cout tiles
and borders, and wgrad_split16_refs.EXTRA_GEOMETRIES (several tiles both ways, a half-empty cin tile).  Outputs are NaN before the launch, so a value that is not written shows; every kernel runs twice and must give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_refs as tr
import wgrad_split16_refs as ws
from pvr_habitat_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def vp(t):
    return C.c_void_p(t.data_ptr())


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device='cuda')


def gpu_scale(t_dev):
    s = nans(1)
    _lib.check(_lib.lib().pvr_op_absmax_scale(vp(t_dev), t_dev.numel(), vp(s), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return float(s.item())


@pytest.mark.parametrize('family', ws.FAMILIES)
def test_absmax_scale_equals_the_cpu_rule(family):
    for t in ws.inputs(family, tr.CONV_GEOMETRIES[3]):                  # 3 x 7 x 7 x 256 and x 64: several blocks
        d = t.contiguous().cuda()
        assert gpu_scale(d) == ws.scale_rule(t), family
        assert gpu_scale(d) == ws.scale_rule(t), 'two runs differ'


def test_absmax_scale_edge_cases():
    assert gpu_scale(torch.zeros(4096, device='cuda')) == 1.0
    r = np.random.default_rng(8)
    for count in (1, 3, 255, 1003, 4097):                               # no multiple of a vector, of a block; one block and several
        t = torch.from_numpy((r.standard_normal(count + 1) * 1e-5).astype(np.float32))
        t[count - 1] = 3.0e-3                                            # the maximum in the tail
        d = t.cuda()
        assert gpu_scale(d[:count]) == ws.scale_rule(t[:count]), count
        assert gpu_scale(d[1:]) == ws.scale_rule(t[1:]), count          # a pointer that is not 16-byte aligned
    for a, want in ((2.0 ** -140, 2.0 ** 126), (3e38, 2.0 ** -113), (float('inf'), 1.0), (float('nan'), 1.0)):
        t = torch.tensor([0.5 if a != a or a == float('inf') else 0.0, -a, 0.0], dtype=torch.float32)
        assert gpu_scale(t.cuda()) == want == ws.scale_rule(t), a


def test_absmax_scale_pair_is_the_same_rule_in_one_launch():
    """the trainer's form: two tensors, one launch; the aux words are zero again afterwards, so the next launch needs no memset"""
    L = _lib.lib()
    aux = torch.zeros(4, dtype=torch.int32, device='cuda')
    for family in ws.FAMILIES:
        x, dz = ws.inputs(family, tr.CONV_GEOMETRIES[3])
        xd, dzd = x.contiguous().cuda(), dz.contiguous().cuda()
        for _ in range(2):
            s = nans(2)
            _lib.check(L.pvr_op_absmax_scale_pair(vp(dzd), dzd.numel(), vp(s[0:1]), vp(xd), xd.numel(), vp(s[1:2]), vp(aux), _lib.stream_ptr()))
            torch.cuda.synchronize()
            assert s.tolist() == [ws.scale_rule(dz), ws.scale_rule(x)], family
            assert not aux.any(), 'the aux words are not left zero'
        s = nans(2)
        _lib.check(L.pvr_op_absmax_scale_pair(vp(xd[0, 0, 0, 1:]), 255, vp(s[0:1]), None, 0, None, vp(aux), _lib.stream_ptr()))       # one tensor, unaligned
        torch.cuda.synchronize()
        assert float(s[0]) == ws.scale_rule(x[0, 0, 0, 1:]) and torch.isnan(s[1]) and not aux.any()
    z = torch.zeros(1000, device='cuda')
    s = nans(2)
    _lib.check(L.pvr_op_absmax_scale_pair(vp(z), 1000, vp(s[0:1]), vp(z), 0, vp(s[1:2]), vp(aux), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert s.tolist() == [1.0, 1.0]


def run_wgrad(x, dz, geo):
    n, h, ci, co, k, s, p = geo
    L = _lib.lib()
    dw = nans(co, ci, k, k)
    floats = int(L.pvr_op_conv_wgrad_split16_scratch_floats(n, h, h, ci, co, k, s, p))
    assert floats > 0
    sc, scales = nans(floats), nans(2)
    xd, dzd = x.contiguous().cuda(), dz.contiguous().cuda()
    st = _lib.stream_ptr()
    _lib.check(L.pvr_op_absmax_scale(vp(xd), xd.numel(), vp(scales[0:1]), st))
    _lib.check(L.pvr_op_absmax_scale(vp(dzd), dzd.numel(), vp(scales[1:2]), st))
    _lib.check(L.pvr_op_conv_wgrad_split16(vp(xd), vp(dzd), vp(dw), n, h, h, ci, co, k, s, p, vp(scales[0:1]), vp(scales[1:2]), vp(sc), floats, st))
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize('geo', ws.GEOMETRIES)
@pytest.mark.parametrize('family', ws.FAMILIES)
def test_weight_gradient_matches_float64(geo, family):
    x, dz = ws.inputs(family, geo)
    ref, bound = ws.reference(x, dz, *geo[4:])
    got = run_wgrad(x, dz, geo)
    assert not torch.isnan(got).any(), 'dw is not fully written'
    r = tr.ratio(got, ref, bound)
    print('\n[split16 wgrad %s %s] error / bound %.3f' % (geo, family, r))
    assert r <= 1.0
    assert torch.equal(got, run_wgrad(x, dz, geo)), 'two runs differ'


@pytest.mark.parametrize('family', ['unit', 'tiny'])
def test_stem_weight_gradient_matches_float64(family):
    n, S = 2, 32                                                         # L = n (S / 2)^2 = 512
    img, dz = ws.stem_inputs(family, n, S)
    ref, bound = ws.stem_reference(img, dz)
    L = _lib.lib()

    def run():
        dw = nans(64, 3, 7, 7)
        floats = int(L.pvr_op_stem_wgrad_split16_scratch_floats(n, S))
        assert floats > 0
        sc, scales = nans(floats), nans(2)
        imgd, dzd = img.contiguous().cuda(), dz.contiguous().cuda()
        st = _lib.stream_ptr()
        _lib.check(L.pvr_op_absmax_scale(vp(imgd), imgd.numel(), vp(scales[0:1]), st))
        _lib.check(L.pvr_op_absmax_scale(vp(dzd), dzd.numel(), vp(scales[1:2]), st))
        _lib.check(L.pvr_op_stem_wgrad_split16(vp(imgd), vp(dzd), vp(dw), n, S, vp(scales[0:1]), vp(scales[1:2]), vp(sc), floats, st))
        torch.cuda.synchronize()
        return dw.cpu()
    got = run()
    assert not torch.isnan(got).any(), 'dw is not fully written'
    r = tr.ratio(got, ref, bound)
    print('\n[split16 stem wgrad %s] error / bound %.3f' % (family, r))
    assert r <= 1.0
    assert torch.equal(got, run()), 'two runs differ'
