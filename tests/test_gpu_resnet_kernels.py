"""The ResNet-side kernels one by one - pvr_op_conv2d under every kernel choice, its split-K, two-operand and L2-fragment forms, the stem and its fused pooled
forms, the pools and the layout / format kernels - against the float64 references and derived elementwise bounds of oracle/resnet_kernel_refs.py.  Every
output sits between guard rows holding a sentinel and is NaN before the launch; every input is an allocation of its own, of exactly its size; every test
asserts error / bound <= 1 per family (the exact and impulse families bit for bit), finiteness, untouched guards and identical bits on a second run, and
prints its error / bound ratios."""
import ctypes as C
import functools

import pytest
import torch

from oracle import resnet_kernel_refs as kr
from pvr_habitat_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

DT = {'f16': _lib.PVR_F16, 'bf16': _lib.PVR_BF16}
DTS = ['f16', 'bf16']
SENTINEL16 = 0x5A5A                                   # guard rows of 16-bit outputs (a finite value in both types)
SENTINEL32 = 0x5A5A5A5A
NAN16 = {'f16': 0x7E00, 'bf16': 0x7FC0}
NAN32 = 0x7FC00000
GUARD = 3                                             # rows in front of and behind every output


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def dev(t):
    """a device allocation of its own, of exactly the tensor's size"""
    return t.contiguous().cuda() if t is not None else None


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _launch(fn, rows, cols, out_dt, what, dev_index=None):
    """Runs fn(out_pointer) -> status on an output of rows x cols (out_dt 'f16' / 'bf16' / None = fp32) that is NaN before the launch and sits between GUARD
    rows of a sentinel.  Returns (status, CPU tensor (rows, cols) in the output type); the guards are checked."""
    it, sent, nan, size = (torch.int16, SENTINEL16, NAN16[out_dt], 2) if out_dt else (torch.int32, SENTINEL32, NAN32, 4)
    out = torch.full((GUARD + rows + GUARD, cols), sent, dtype=it, device='cuda' if dev_index is None else 'cuda:%d' % dev_index)
    out[GUARD:GUARD + rows] = nan
    st = fn(vp(out, GUARD * cols * size))
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[:GUARD] == sent).all() and (o[GUARD + rows:] == sent).all(), '%s wrote outside its rows' % what
    return st, o[GUARD:GUARD + rows].view(kr.TORCH_DT[out_dt] if out_dt else torch.float32)


def _check(got, ref, bound, family, what, exact=False):
    assert torch.isfinite(got.float()).all(), '%s %s: a NaN survived or an output is not finite' % (what, family)
    if exact:
        assert torch.equal(got.double().reshape(ref.shape), ref), '%s %s: not bit for bit' % (what, family)
    return kr.ratio(got.reshape(ref.shape), ref, bound)


@pytest.fixture
def conv_algo():
    def _set(a):
        _lib.check(_lib.lib().pvr_debug_set_conv_algo(a))
    yield _set
    _lib.check(_lib.lib().pvr_debug_set_conv_algo(-1))


# ------------------------------------------------------------------------------------------------------------------
# pvr_op_conv2d under every kernel choice
# ------------------------------------------------------------------------------------------------------------------
def _conv_device_inputs(x, wt, b, r):
    return dev(x), dev(kr.pack_weights(wt)), dev(kr.pad_bias(b)), dev(r)


def _conv2d(d, shape, res, act, out16, dt):
    xd, wd, bd, rd = d
    n, h, w, cin, cout, kh, kw, stride, pad = shape
    ho, wo = kr.out_hw(h, w, kh, kw, stride, pad)
    flags = (0 if out16 else 1) | (2 if res == 'f32' else 0)
    fn = lambda o: _lib.lib().pvr_op_conv2d(vp(xd), vp(wd), vp(bd), vp(rd), o, n, h, w, cin, cout, kh, kw, stride, pad, act, flags, DT[dt], _lib.stream_ptr())
    return _launch(fn, n * ho * wo, cout, dt if out16 else None, 'conv2d %s' % (shape,))


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('entry', kr.CONV_GRID, ids=lambda e: 'x'.join(str(v) for v in e[0]))
def test_conv2d_matches_float64(entry, dt, conv_algo):
    shape, configs, _ = entry
    square = shape[5] == shape[6]
    worst = {}
    for res, act, out16 in configs:
        for family in kr.conv_families(res, act):
            x, wt, b, r = kr.conv_inputs(family, shape, dt, res)
            ref, bound = kr.conv_ref(x, wt, b, r, act, shape[7], shape[8], dt if out16 else None)
            d = _conv_device_inputs(x, wt, b, r)
            for algo in (0, 1, 2, 3, -1):
                conv_algo(algo)
                what = 'conv2d %s res %s act %d out16 %d algo %d' % (shape, res, act, out16, algo)
                st, got = _conv2d(d, shape, res, act, out16, dt)
                if st != 0:                                                         # a filter that is not built: refused with a message, nothing written
                    assert not square and _lib.last_error(), what
                    assert torch.isnan(got.float()).all(), '%s: a refused call launched something' % what
                    worst['refused'] = 0.0
                    continue
                key = '%s/%d' % (family, algo)
                worst[key] = max(worst.get(key, 0.0), _check(got, ref, bound, family, what, exact=family == 'exact'))
                _, again = _conv2d(d, shape, res, act, out16, dt)
                assert torch.equal(_bits(got), _bits(again)), '%s %s: two runs differ' % (what, family)
    fam = {f: max(v for k, v in worst.items() if k.split('/')[0] == f) for f in {k.split('/')[0] for k in worst}}
    print('\n[conv2d %s %s] error / bound %s' % (shape, dt, {k: '%.2f' % v for k, v in sorted(fam.items())}))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def _big_conv_case(shape, dt, res, act):
    """the unit family of a large shape with its reference"""
    x, wt, b, r = kr.conv_inputs('unit', shape, dt, res)
    return (x, wt, b, r) + kr.conv_ref(x, wt, b, r, act, shape[7], shape[8], dt)


# the smallest shapes conv_expand_supported accepts: 64 -> 64 channels needs 4 * 512 pixel tiles of 64 (one cout tile: every block of the persistent grid
# gets four), 256 -> 256 with a residual 4 * 256 tiles; one pixel more than a whole number of tiles.  (56,197,1,..): 44 x 9 = 396 tiles of 256 x 256
BIG_CASES = [
    ((56, 197, 1, 64, 2304, 1, 1, 1, 0), None, 0, 1, 'pp_persistent'),
    ((1, 2047 * 64 + 1, 1, 64, 64, 1, 1, 1, 0), None, 1, -1, 'conv_expand'),
    ((1, 1023 * 64 + 1, 1, 256, 256, 1, 1, 1, 0), 'h', 1, -1, 'conv_expand'),
]


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', BIG_CASES, ids=lambda c: '%s_cin%d' % (c[4], c[0][3]))
def test_conv2d_chosen_by_shape_matches_float64(case, dt, conv_algo):
    shape, res, act, algo, counter = case
    L = _lib.lib()
    count = {'pp_persistent': L.pvr_debug_pp_persistent_launches, 'conv_expand': L.pvr_debug_conv_expand_launches}[counter]
    x, wt, b, r, ref, bound = _big_conv_case(shape, dt, res, act)
    d = _conv_device_inputs(x, wt, b, r)
    conv_algo(algo)
    before = count()
    st, got = _conv2d(d, shape, res, act, True, dt)
    _lib.check(st)
    assert count() == before + 1, 'the launch did not take %s' % counter
    ratio = _check(got, ref, bound, 'unit', 'conv2d %s' % (shape,))
    _, again = _conv2d(d, shape, res, act, True, dt)
    assert torch.equal(_bits(got), _bits(again)), 'two runs differ'
    print('\n[conv2d %s %s %s] error / bound {unit: %.2f}' % (shape, counter, dt, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# split-K, L2-fragment and two-operand forms
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('shape', kr.SPLITK_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_conv2d_splitk_matches_float64(shape, dt):
    n, h, w, cin, cout, kh, kw, stride, pad = shape
    ho, wo = kr.out_hw(h, w, kh, kw, stride, pad)
    M = n * ho * wo
    worst = {}
    for res, act, out16 in kr.SPLITK_CONFIGS:
        for family in kr.conv_families(res, act):
            x, wt, b, r = kr.conv_inputs(family, shape, dt, res)
            ref, bound = kr.conv_ref(x, wt, b, r, act, stride, pad, dt if out16 else None)
            xd, wd, bd, rd = _conv_device_inputs(x, wt, b, r)
            for ks in kr.SPLITK_KSPLITS:
                def run():
                    scratch = torch.full((GUARD + ks * M + GUARD, cout), SENTINEL32, dtype=torch.int32, device='cuda')     # the fp32 planes, between guards too
                    fn = lambda o: _lib.lib().pvr_op_conv2d_splitk(vp(xd), vp(wd), vp(bd), vp(rd), o, vp(scratch, GUARD * cout * 4), ks, n, h, w, cin, cout, kh, kw,
                                                                   stride, pad, act, 0 if out16 else 1, DT[dt], _lib.stream_ptr())
                    st, got = _launch(fn, M, cout, dt if out16 else None, 'split-K %s' % (shape,))
                    _lib.check(st)
                    s = scratch.cpu()
                    assert (s[:GUARD] == SENTINEL32).all() and (s[GUARD + ks * M:] == SENTINEL32).all(), 'split-K wrote outside its planes'
                    return got
                got = run()
                key = '%s/%d' % (family, ks)
                worst[key] = max(worst.get(key, 0.0), _check(got, ref, bound, family, 'split-K %s ksplit %d' % (shape, ks), exact=family == 'exact'))
                assert torch.equal(_bits(got), _bits(run())), 'split-K %s %s ksplit %d: two runs differ' % (shape, family, ks)
    fam = {f: max(v for k, v in worst.items() if k.split('/')[0] == f) for f in {k.split('/')[0] for k in worst}}
    print('\n[conv2d_splitk %s %s] error / bound %s' % (shape, dt, {k: '%.2f' % v for k, v in sorted(fam.items())}))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def _pack_frag(wk):
    wp = torch.empty_like(wk)
    _lib.check(_lib.lib().pvr_op_pack_frag_weights(vp(wk), vp(wp), wk.shape[0], wk.shape[1], _lib.stream_ptr()))
    return wp


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', kr.WFRAG_CASES, ids=lambda c: 'x'.join(str(v) for v in c[0]))
def test_conv_wfrag_matches_float64(case, dt):
    shape, res = case
    n, h, w, cin, cout, kh, kw, stride, pad = shape
    ho, wo = kr.out_hw(h, w, kh, kw, stride, pad)
    L = _lib.lib()
    worst = {}
    for act, out16 in ((1, True), (0, False)):
        for family in kr.conv_families(res, act):
            x, wt, b, r = kr.conv_inputs(family, shape, dt, res)
            ref, bound = kr.conv_ref(x, wt, b, r, act, stride, pad, dt if out16 else None)
            xd, wd, bd, rd = _conv_device_inputs(x, wt, b, r)
            wp = _pack_frag(wd)
            fn = lambda o: L.pvr_op_conv_wfrag(vp(xd), vp(wp), vp(bd), vp(rd), o, n, h, w, cin, cout, kh, kw, stride, pad, act, 0 if out16 else 1, DT[dt], _lib.stream_ptr())
            before = L.pvr_debug_conv_wfrag_launches()
            st, got = _launch(fn, n * ho * wo, cout, dt if out16 else None, 'conv_wfrag %s' % (shape,))
            _lib.check(st)
            assert L.pvr_debug_conv_wfrag_launches() == before + 1
            worst[family] = max(worst.get(family, 0.0), _check(got, ref, bound, family, 'conv_wfrag %s' % (shape,), exact=family == 'exact'))
            _, again = _launch(fn, n * ho * wo, cout, dt if out16 else None, 'conv_wfrag %s' % (shape,))
            assert torch.equal(_bits(got), _bits(again)), 'conv_wfrag %s %s: two runs differ' % (shape, family)
    print('\n[conv_wfrag %s %s] error / bound %s' % (shape, dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [1, 2, 3])
def test_conv_wfrag_pool_matches_float64(n, dt):
    """the pooled form: two whole 7 x 7 frames per tile, so one frame, one full pair and a pair plus a ragged frame; output strided between guards"""
    cin, cout = 64, 256
    shape = (n, 7, 7, cin, cout, 1, 1, 1, 0)
    L = _lib.lib()
    stride_o = cout + 24
    worst = {}
    for family in ('unit', 'exact', 'cancel', 'relu_edge', 'large'):
        x, wt, b, r = kr.conv_inputs(family, shape, dt, 'h')
        ref, bound = kr.pooled_conv_ref(x, wt, b, r)
        xd, wd, bd, rd = _conv_device_inputs(x, wt, b, r)
        wp = _pack_frag(wd)
        fn = lambda o: L.pvr_op_conv_wfrag_pool(vp(xd), vp(wp), vp(bd), vp(rd), C.c_void_p(o.value + 32), stride_o, n, cin, cout, DT[dt], _lib.stream_ptr())
        st, full = _launch(fn, n, stride_o, None, 'conv_wfrag_pool n %d' % n)
        _lib.check(st)
        assert torch.isnan(full[:, :8]).all() and torch.isnan(full[:, 8 + cout:]).all(), 'conv_wfrag_pool wrote into the gap between its rows'
        got = full[:, 8:8 + cout].contiguous()
        worst[family] = _check(got, ref, bound, family, 'conv_wfrag_pool n %d' % n)
        _, again = _launch(fn, n, stride_o, None, 'conv_wfrag_pool n %d' % n)
        assert torch.equal(_bits(got), _bits(again[:, 8:8 + cout].contiguous())), 'conv_wfrag_pool %s: two runs differ' % family
    print('\n[conv_wfrag_pool n %d %s] error / bound %s' % (n, dt, {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('case', kr.DUAL_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_conv2d_dual_matches_float64(case, dt):
    n, ho, cin, cout, k, cin2, s2 = case
    pad = k // 2
    h2 = ho * s2 - (s2 - 1)
    x, x2, wt, w2, b = kr.dual_inputs(case, dt)
    ref, bound = kr.conv_ref(x, wt, b, None, 1, 1, pad, dt, extra=(x2, w2, s2))
    wcat = torch.cat([kr.pack_weights(wt), kr.pack_weights(w2.reshape(cout, 1, 1, cin2))], dim=1)          # the second operand's columns behind the first's
    xd, x2d, wd, bd = dev(x), dev(x2), dev(wcat), dev(kr.pad_bias(b))
    fn = lambda o: _lib.lib().pvr_op_conv2d_dual(vp(xd), vp(x2d), vp(wd), vp(bd), o, n, ho, ho, cin, cout, k, k, 1, pad, h2, h2, cin2, s2, 1, DT[dt], _lib.stream_ptr())
    st, got = _launch(fn, n * ho * ho, cout, dt, 'conv2d_dual %s' % (case,))
    _lib.check(st)
    ratio = _check(got, ref, bound, 'unit', 'conv2d_dual %s' % (case,))
    _, again = _launch(fn, n * ho * ho, cout, dt, 'conv2d_dual %s' % (case,))
    assert torch.equal(_bits(got), _bits(again)), 'two runs differ'
    print('\n[conv2d_dual %s %s] error / bound {unit: %.2f}' % (case, dt, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_images(family, dt, n):
    return kr.stem_image(family, n, dt)


@functools.lru_cache(maxsize=None)
def _stem_ref_one(family, dt, i, pool, crop):
    """reference and bound of image i alone (an image does not depend on the batch it is in): shared by every batch size and form"""
    wgt, b = kr.stem_weights(family, dt)
    if crop:
        img = kr.stem_image_from_frames(kr.stem_frames(i + 1, 256, 320)[i:i + 1], 32, 96, dt)
    else:
        img = _stem_images(family, dt, 37 if i >= 9 else 9)[i:i + 1]
    return kr.stem_ref(img, wgt, b, pool)


def _stem_ref(family, dt, n, pool, crop=False):
    parts = [_stem_ref_one(family, dt, i, pool, crop) for i in range(n)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [1, 3])
def test_stem_matches_float64(n, dt):
    worst = {}
    for family in kr.STEM_FAMILIES:
        wgt, b = kr.stem_weights(family, dt)
        imgd, wd, bd = dev(_stem_images(family, dt, 9)[:n]), dev(wgt.reshape(64, 224)), dev(b)
        ref, bound = _stem_ref(family, dt, n, False)
        fn = lambda o: _lib.lib().pvr_op_stem(vp(imgd), vp(wd), vp(bd), o, n, DT[dt], _lib.stream_ptr())
        st, got = _launch(fn, n * 112 * 112, 64, dt, 'stem')
        _lib.check(st)
        worst[family] = _check(got, ref, bound, family, 'stem n %d' % n, exact=family == 'impulse')
        _, again = _launch(fn, n * 112 * 112, 64, dt, 'stem')
        assert torch.equal(_bits(got), _bits(again)), 'stem %s: two runs differ' % family
    print('\n[stem n %d %s] error / bound %s' % (n, dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


def _c1_device(dt):
    """layer1.0.conv1 for the fused stem: weights as the stem's fragment image, bias; and the (64,1,1,64) weights and bias for the reference"""
    w1, b1 = kr.stem_c1_inputs(dt)
    src = w1.reshape(64, 64).contiguous().view(torch.int16)
    image = torch.empty(4096, dtype=torch.int16)
    _lib.check(_lib.lib().pvr_debug_stem_c1_pack(C.c_void_p(src.data_ptr()), C.c_void_p(image.data_ptr())))
    return w1, b1, dev(image), dev(b1)


def _check_t1(pooled, t1, n, dt, what):
    """t1 = relu(conv1x1(pooled) + b1) on the pooled output the kernel itself wrote"""
    w1, b1 = kr.stem_c1_inputs(dt)
    ref, bound = kr.conv_ref(pooled.reshape(n, 56, 56, 64), w1, b1, None, 1, 1, 0, dt)
    return _check(t1, ref, bound, 'c1', what)


def _stem_pool_case(call, n, dt, family, form, with_c1, what, crop=False):
    """call(out_ptr, c1_w, c1_b, c1_t1) -> status.  Returns the error / bound ratios of the pooled output and of t1 (or None)"""
    ref, bound = _stem_ref(family, dt, n, True, crop)
    t1_box = {}

    def run():
        if not with_c1:
            st, got = _launch(lambda o: call(o, None, None, None), n * 56 * 56, 64, dt, what)
            _lib.check(st)
            return got, None
        w1, b1, c1w, c1b = _c1_device(dt)

        def inner(t1_ptr):
            st, got = _launch(lambda o: call(o, vp(c1w), vp(c1b), t1_ptr), n * 56 * 56, 64, dt, what)
            t1_box['pooled'] = got
            return st
        st, t1 = _launch(inner, n * 56 * 56, 64, dt, what + ' (t1)')
        _lib.check(st)
        return t1_box['pooled'], t1
    got, t1 = run()
    r = _check(got, ref, bound, family, what, exact=family == 'impulse')
    r1 = _check_t1(got, t1, n, dt, what) if with_c1 else None
    again, t1_again = run()
    assert torch.equal(_bits(got), _bits(again)) and (t1 is None or torch.equal(_bits(t1), _bits(t1_again))), '%s %s: two runs differ' % (what, family)
    return r, r1


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [1, 9, 37])
@pytest.mark.parametrize('form', [0, 1, 2])
def test_stem_pool_matches_float64(form, n, dt):
    """n = 1: one image per block; 9: groups of four with a ragged last group; 37: more than four images per block on 256 CUs"""
    worst = {}
    for family in kr.STEM_FAMILIES:
        wgt, b = kr.stem_weights(family, dt)
        imgd, wd, bd = dev(_stem_images(family, dt, 37 if n > 9 else 9)[:n]), dev(wgt.reshape(64, 224)), dev(b)
        for with_c1 in ((False, True) if form == 2 else (False,)):
            call = lambda o, cw, cb, t1: _lib.lib().pvr_op_stem_pool(vp(imgd), vp(wd), vp(bd), o, n, form, cw, cb, t1, DT[dt], _lib.stream_ptr())
            r, r1 = _stem_pool_case(call, n, dt, family, form, with_c1, 'stem_pool form %d n %d' % (form, n))
            worst[family] = max(worst.get(family, 0.0), r)
            if r1 is not None:
                worst['c1/' + family] = r1
    print('\n[stem_pool form %d n %d %s] error / bound %s' % (form, n, dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('dt', DTS)
@pytest.mark.parametrize('n', [1, 9, 37])
@pytest.mark.parametrize('form', [1, 2])
def test_stem_pool_u8_matches_float64(form, n, dt):
    L = _lib.lib()
    wgt, b = kr.stem_weights('uint8', dt)
    wd, bd = dev(wgt.reshape(64, 224)), dev(b)
    worst = {}
    cases = [('224', kr.stem_frames(n), 0, 0, False)]
    if n == 9:
        cases.append(('256x320 corner', kr.stem_frames(n, 256, 320), 32, 96, True))
    for name, frames, top, left, crop in cases:
        fd = dev(frames)
        h, w = frames.shape[1], frames.shape[2]
        assert L.pvr_debug_stem_u8_geometry_ok(vp(fd), h, w, top, left) == 1
        for with_c1 in ((False, True) if form == 2 else (False,)):
            call = lambda o, cw, cb, t1: L.pvr_op_stem_pool_u8(vp(fd), n, h, w, top, left, vp(wd), vp(bd), o, form, cw, cb, t1, DT[dt], _lib.stream_ptr())
            r, r1 = _stem_pool_case(call, n, dt, 'uint8', form, with_c1, 'stem_pool_u8 form %d n %d %s' % (form, n, name), crop)
            worst[name] = max(worst.get(name, 0.0), r)
            if r1 is not None:
                worst['c1/' + name] = r1
    print('\n[stem_pool_u8 form %d n %d %s] error / bound %s' % (form, n, dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


def test_stem_forms_that_are_not_built_are_refused():
    L = _lib.lib()
    wgt, b = kr.stem_weights('uint8', 'f16')
    imgd, wd, bd, fd = dev(_stem_images('uint8', 'f16', 9)[:1]), dev(wgt.reshape(64, 224)), dev(b), dev(kr.stem_frames(1))
    _, _, c1w, c1b = _c1_device('f16')
    calls = {
        'form 3': lambda o: L.pvr_op_stem_pool(vp(imgd), vp(wd), vp(bd), o, 1, 3, None, None, None, DT['f16'], _lib.stream_ptr()),
        'conv1 without register pooling': lambda o: L.pvr_op_stem_pool(vp(imgd), vp(wd), vp(bd), o, 1, 1, vp(c1w), vp(c1b), o, DT['f16'], _lib.stream_ptr()),
        'uint8, form 0': lambda o: L.pvr_op_stem_pool_u8(vp(fd), 1, 224, 224, 0, 0, vp(wd), vp(bd), o, 0, None, None, None, DT['f16'], _lib.stream_ptr()),
        'uint8, window outside the frame': lambda o: L.pvr_op_stem_pool_u8(vp(fd), 1, 224, 224, 16, 0, vp(wd), vp(bd), o, 2, None, None, None, DT['f16'], _lib.stream_ptr()),
        'uint8, unaligned column': lambda o: L.pvr_op_stem_pool_u8(vp(fd), 1, 224, 224, 0, 1, vp(wd), vp(bd), o, 2, None, None, None, DT['f16'], _lib.stream_ptr()),
    }
    for name, fn in calls.items():
        st, got = _launch(fn, 56 * 56, 64, 'f16', name)
        assert st != 0 and _lib.last_error(), name
        assert torch.isnan(got.float()).all(), '%s: a refused call launched something' % name


def test_stem_pool_lds_form_on_a_second_device():
    """the padded-image LDS form needs its dynamic-LDS attribute on every device of the process, not only on the first one that ran it"""
    if torch.cuda.device_count() < 2:
        pytest.skip('one GPU visible')
    dt = 'f16'
    wgt, b = kr.stem_weights('generic', dt)
    img = _stem_images('generic', dt, 9)[:1]
    ref, bound = _stem_ref('generic', dt, 1, True)
    for index in (0, 1):
        with torch.cuda.device(index):
            imgd, wd, bd = (t.contiguous().cuda(index) for t in (img, wgt.reshape(64, 224), b))
            fn = lambda o: _lib.lib().pvr_op_stem_pool(vp(imgd), vp(wd), vp(bd), o, 1, 1, None, None, None, DT[dt], _lib.stream_ptr())
            st, got = _launch(fn, 56 * 56, 64, dt, 'stem_pool form 1 on device %d' % index, dev_index=index)
            _lib.check(st)
            assert _check(got, ref, bound, 'generic', 'stem_pool form 1 on device %d' % index) <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# pools, layout and format kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTS)
def test_maxpool_is_exact(dt):
    for n, h, w, c in kr.MAXPOOL_GRID:
        x = kr.maxpool_inputs(n, h, w, c, dt)
        ref = kr.maxpool_ref(x)
        xd = dev(x)
        fn = lambda o: _lib.lib().pvr_op_maxpool(vp(xd), o, n, h, w, c, DT[dt], _lib.stream_ptr())
        rows = ref.numel() // c
        st, got = _launch(fn, rows, c, dt, 'maxpool %s' % ((n, h, w, c),))
        _lib.check(st)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got.float().reshape(ref.shape), ref.float()), 'maxpool %s differs from the maximum of its window' % ((n, h, w, c),)
        _, again = _launch(fn, rows, c, dt, 'maxpool')
        assert torch.equal(_bits(got), _bits(again))
    print('\n[maxpool %s] exact on %s' % (dt, kr.MAXPOOL_GRID))


def _strided_rows(fn_of_ptr, n, cols, stride, what):
    """fp32 rows of `cols` values at a row stride, eight columns into a guarded block of n rows: returns the rows; everything else must keep its NaN"""
    st, full = _launch(lambda o: fn_of_ptr(C.c_void_p(o.value + 32)), n, stride, None, what)
    _lib.check(st)
    assert torch.isnan(full[:, :8]).all() and torch.isnan(full[:, 8 + cols:]).all(), '%s wrote into the gap between its rows' % what
    return full[:, 8:8 + cols].contiguous()


@pytest.mark.parametrize('in_dt', DTS + ['f32'])
def test_avgpool_matches_float64(in_dt):
    worst = 0.0
    cdt = DT['f16' if in_dt == 'f32' else in_dt]
    for hw in kr.AVGPOOL_HW:
        for c in kr.AVGPOOL_C:
            x = kr.pool_inputs((3, hw, c), in_dt, 'avg')
            ref, bound = kr.avgpool_ref(x)
            xd = dev(x)
            fn = lambda o: _lib.lib().pvr_op_avgpool(vp(xd), o, c + 24, 3, hw, c, 1 if in_dt == 'f32' else 0, cdt, _lib.stream_ptr())
            got = _strided_rows(fn, 3, c, c + 24, 'avgpool hw %d c %d' % (hw, c))
            r = _check(got, ref, bound, 'unit', 'avgpool hw %d c %d' % (hw, c))
            assert r <= 1.0, (hw, c, r)
            worst = max(worst, r)
            assert torch.equal(_bits(got), _bits(_strided_rows(fn, 3, c, c + 24, 'avgpool')))
    print('\n[avgpool %s in] error / bound {unit: %.2f}' % (in_dt, worst))


@pytest.mark.parametrize('dt', DTS)
def test_avgpool2_and_attnpool_tokens_match_float64(dt):
    L = _lib.lib()
    worst = {'avgpool2': 0.0, 'attnpool_tokens': 0.0}
    for shape in kr.AVGPOOL2_GRID:
        n, h, w, c = shape
        x = kr.pool_inputs(shape, dt, 'avg2')
        ref, bound = kr.avgpool2_ref(x)
        xd = dev(x)
        fn = lambda o: L.pvr_op_avgpool2(vp(xd), o, n, h, w, c, DT[dt], _lib.stream_ptr())
        st, got = _launch(fn, n * (h // 2) * (w // 2), c, dt, 'avgpool2 %s' % (shape,))
        _lib.check(st)
        worst['avgpool2'] = max(worst['avgpool2'], _check(got, ref, bound, 'unit', 'avgpool2 %s' % (shape,)))
        assert torch.equal(_bits(got), _bits(_launch(fn, n * (h // 2) * (w // 2), c, dt, 'avgpool2')[1]))
    for n, hw, c in kr.ATTNPOOL_GRID:
        x, pos = kr.pool_inputs((n, hw, c), 'f32', 'apx'), kr.pool_inputs((hw + 1, c), 'f32', 'app')
        ref, bound = kr.attnpool_tokens_ref(x, pos, dt)
        xd, pd = dev(x), dev(pos)
        fn = lambda o: L.pvr_op_attnpool_tokens(vp(xd), vp(pd), o, n, hw, c, DT[dt], _lib.stream_ptr())
        st, got = _launch(fn, n * (hw + 1), c, dt, 'attnpool_tokens %s' % ((n, hw, c),))
        _lib.check(st)
        worst['attnpool_tokens'] = max(worst['attnpool_tokens'], _check(got, ref, bound, 'unit', 'attnpool_tokens %s' % ((n, hw, c),)))
        assert torch.equal(_bits(got), _bits(_launch(fn, n * (hw + 1), c, dt, 'attnpool_tokens')[1]))
    print('\n[avgpool2 / attnpool_tokens %s] error / bound %s' % (dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    assert L.pvr_op_avgpool2(vp(xd), vp(xd), 1, 3, 4, 8, DT[dt], _lib.stream_ptr()) != 0 and _lib.last_error()       # an odd height is refused


def test_nhwc_to_chw_is_an_exact_copy():
    for n, hw, cpad, creal in kr.CHW_GRID:
        x = kr.pool_inputs((n, hw, cpad), 'f32', 'chw')
        ref = kr.nhwc_to_chw_ref(x, creal)
        xd = dev(x)
        stride = hw * creal + 24
        fn = lambda o: _lib.lib().pvr_op_nhwc_to_chw(vp(xd), o, stride, n, hw, cpad, creal, _lib.stream_ptr())
        got = _strided_rows(fn, n, hw * creal, stride, 'nhwc_to_chw %s' % ((n, hw, cpad, creal),))
        assert torch.equal(_bits(got), _bits(ref)), (n, hw, cpad, creal)


@functools.lru_cache(maxsize=None)
def _format_values(count):
    return torch.from_numpy(kr.synth.normal(53, 'f2h_%d' % count, (count,)))


@pytest.mark.parametrize('dt', DTS)
def test_format_kernels_equal_torch_casts(dt):
    """f32_to_h: round to nearest even, ties, values below the normal range, overflow to inf, both zeros; h_to_f32: exact.  The last count is past one pass
    of the kernels' grid-stride loops (8192 x 256 threads of eight values; 4096 x 256 of one)."""
    L = _lib.lib()
    tdt = kr.TORCH_DT[dt]
    for count in (8, 2056, 8192 * 256 * 8 + 8):
        x = _format_values(count).clone()
        x[:8] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-7, -3e-41, 7e4, -1e39])
        x[8:] *= torch.pow(2.0, (torch.arange(count - 8) % 61 - 40).float())
        xd = dev(x)
        fn = lambda o: L.pvr_op_f32_to_h(vp(xd), o, count, DT[dt], _lib.stream_ptr())
        st, got = _launch(fn, count // 8, 8, dt, 'f32_to_h %d' % count)
        _lib.check(st)
        assert torch.equal(_bits(got).reshape(-1), _bits(x.to(tdt))), 'f32_to_h differs from the cast at %d values' % count
    assert L.pvr_op_f32_to_h(vp(xd), vp(xd), 12, DT[dt], _lib.stream_ptr()) != 0 and _lib.last_error()              # a count that is no multiple of 8
    for count in (1, 1000, 4096 * 256 + 3):
        bits = (torch.arange(count, dtype=torch.int64) * 40503 % 65536).to(torch.int32)
        bits[(bits & 0x7FFF) > (0x7C00 if dt == 'f16' else 0x7F80)] = 0x3C00                                       # no NaN: its payload is not pinned
        h = bits.to(torch.int16).view(tdt)
        hd = dev(h)
        fn = lambda o: L.pvr_op_h_to_f32(vp(hd), o, count, DT[dt], _lib.stream_ptr())
        st, got = _launch(fn, count, 1, None, 'h_to_f32 %d' % count)
        _lib.check(st)
        assert torch.equal(_bits(got).reshape(-1), _bits(h.float())), 'h_to_f32 differs from the cast at %d values' % count
