"""The f32s compute type on the GPU (PVR_F32S: fp32 storage as PVR_F32, every product on the 16-bit matrix pipe as an exact (hi, lo) f16 split product):
the stem kernel (stem_split16.hip) against float64, whole networks against the fp32 oracle and against the PVR_F32 plan of the same weights, the bit-exact
invariances of the forward, the 65504 range check, and the Python surface.  synth weights and frames only."""
import ctypes as C

import numpy as np
import pytest
import torch

from pvr_habitat_amd import synth, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]


def _relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)), float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _max_rel(a, b):
    """the MAXIMUM relative error over EVERY element above 1 % of the reference's largest magnitude (none left out)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    big = np.abs(b) > 0.01 * np.abs(b).max()
    assert big.any()
    return float((np.abs(a - b)[big] / np.abs(b)[big]).max())


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------------------------------------
# 1. the stem kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,S', [(1, 224), (3, 30)])
def test_stem_split16_is_an_fp32_convolution(n, S):
    """pvr_op_stem_split16 against conv1 7x7/2 pad 3 + bias + ReLU in float64.  (1, 224): exactly 98 full 128-pixel tiles; (3, 30): M = 675, a ragged last
    tile, and every border pixel a large share of the image.  The bound is test_conv_split16_is_an_fp32_convolution's per-convolution bound: the same
    arithmetic at a shorter K (147 products per output)."""
    L = _lib.lib()
    So = S // 2
    x = torch.from_numpy(synth.normal(13, 'st16x%d_%d' % (n, S), (n, S, S, 3)))
    # a few tiny and a few large pixels: the low parts must survive f16's subnormal range, the high parts its 65504
    x.view(-1)[::997] *= 1e-6
    x.view(-1)[5::1013] *= 3e3
    w4 = torch.from_numpy(synth.normal(13, 'st16w', (64, 3, 7, 7), std=float(np.sqrt(2.0 / 147))))
    b = torch.from_numpy(synth.uniform(13, 'st16b', (64,), -0.5, 0.5))
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w4.double(), b.double(), 2, 3).clamp_(min=0).permute(0, 2, 3, 1)
    img = torch.zeros((n, S + 6, S + 8, 4))
    img[:, 3:3 + S, 3:3 + S, :3] = x                                   # zero border: 3 rows above / below, 3 columns left, 5 right; channel 3 zero
    wk = torch.zeros((64, 7, 8, 4))
    wk[:, :, :7, :3] = w4.permute(0, 2, 3, 1)                          # K index (a * 8 + b) * 4 + c; column 7 and channel 3 zero
    imgd, wd, bd = img.cuda(), wk.reshape(64, 224).contiguous().cuda(), b.cuda()
    wsp = torch.empty((64, 224, 2), dtype=torch.float16, device='cuda')
    _lib.check(L.pvr_op_split16_pack_weights(_vp(wd), _vp(wsp), 64, 224, _lib.stream_ptr()))
    before = L.pvr_debug_stem_split16_launches()
    y = torch.full((n, So, So, 64), float('nan'), device='cuda')
    _lib.check(L.pvr_op_stem_split16(_vp(imgd), _vp(wsp), _vp(bd), _vp(y), n, S, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert L.pvr_debug_stem_split16_launches() == before + 1
    assert torch.isfinite(y).all()
    l2, mx = _relerr(y.cpu().numpy(), ref.numpy())
    print('\n[stem_split16 n=%d S=%d] rel-L2 %.2e max-norm %.2e' % (n, S, l2, mx))
    assert l2 < 2e-6 and mx < 5e-6, (l2, mx)
    y2 = torch.full_like(y, float('nan'))
    _lib.check(L.pvr_op_stem_split16(_vp(imgd), _vp(wsp), _vp(bd), _vp(y2), n, S, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(y, y2)                                          # run to run: bit-identical (no atomics, fixed K order)
    assert L.pvr_debug_stem_split16_launches() == before + 2


def test_stem_split16_refuses_bad_arguments():
    L = _lib.lib()
    t = torch.zeros(64, device='cuda')
    assert L.pvr_op_stem_split16(_vp(t), _vp(t), _vp(t), _vp(t), 1, 31, _lib.stream_ptr()) != 0       # odd image size
    assert L.pvr_op_stem_split16(None, _vp(t), _vp(t), _vp(t), 1, 30, _lib.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------
# 2. + 3. whole networks: against the oracle, and against the PVR_F32 plan of the same weights
# ------------------------------------------------------------------------------------------------
NET_CASES = [('conv5', 64), ('conv3', 128), ('conv4', 64), ('r18', 64)]
_NET = {}


def _net_run(variant, frame):
    """one f32s and one f32 forward of 3 frames, the oracle's embedding, and what the counters saw - computed once per case, shared, never changed"""
    key = (variant, frame)
    if key not in _NET:
        from oracle import encoder_oracle as eo
        from pvr_habitat_amd.embeddings import HipResNet50
        torch.set_num_threads(8)
        L = _lib.lib()
        sd = synth.resnet50_state_dict(6, variant)
        fr = synth.smooth_frames(71, 3, frame, frame)
        d = torch.from_numpy(fr).cuda()
        ms = HipResNet50(sd, variant, compute_dtype='f32s', max_batch=4)
        kn, ops = ms.kernel_names(3), ms.op_names()
        c0, s0 = L.pvr_debug_conv_split16_launches(), L.pvr_debug_stem_split16_launches()
        out = ms(d).cpu().numpy()
        counts = (L.pvr_debug_conv_split16_launches() - c0, L.pvr_debug_stem_split16_launches() - s0)
        m32 = HipResNet50(sd, variant, compute_dtype='f32', max_batch=4)
        c1 = L.pvr_debug_conv_split16_launches()
        out32 = m32(d).cpu().numpy()
        f32_split_launches = L.pvr_debug_conv_split16_launches() - c1
        ops32, kn32 = m32.op_names(), m32.kernel_names(3)
        ms.close(); m32.close()
        _NET[key] = dict(out=out, out32=out32, ref=eo.embed(sd, fr, variant, squeeze=False), kn=kn, ops=ops, counts=counts, ops32=ops32, kn32=kn32,
                         f32_split_launches=f32_split_launches)
    return _NET[key]


@pytest.mark.parametrize('variant,frame', NET_CASES)
def test_whole_network_against_the_oracle(variant, frame):
    """rel-L2 and max-norm at the bound test_fp32_reference_precision_mode holds PVR_F32 to, and the north-star 1e-3 ELEMENT-WISE: the maximum relative error
    over every element above 1 % of the maximum (CPU emulation of the arithmetic: <= 5.4e-5, tests/test_f32s_cpu.py)."""
    r = _net_run(variant, frame)
    l2, mx = _relerr(r['out'], r['ref'])
    rel = _max_rel(r['out'], r['ref'])
    l2f, mxf = _relerr(r['out32'], r['ref'])
    print('\n[%s f32s] rel-L2 %.2e max-norm %.2e max element-wise relative error %.2e   (f32 plan: %.2e / %.2e / %.2e)'
          % (variant, l2, mx, rel, l2f, mxf, _max_rel(r['out32'], r['ref'])))
    assert r['out'].shape == r['ref'].shape and np.isfinite(r['out']).all()
    assert l2 < 1e-4 and mx < 1e-4, (l2, mx)
    assert rel < 1e-3, rel


@pytest.mark.parametrize('variant,frame', NET_CASES)
def test_against_the_f32_plan(variant, frame):
    """Same weights, same frames: both plans are fp32 convolutions of the same fp32 tensors - the bound of
    test_parity_plan_of_the_compressed_pvrs_runs_on_the_16_bit_pipe (emulated whole-net values: 1.2e-6 / 1.6e-6).  The plan says which kernels ran, the
    launch counters say they did."""
    r = _net_run(variant, frame)
    l2, mx = _relerr(r['out'], r['out32'])
    print('\n[%s] f32s vs f32 plan: rel-L2 %.2e max-norm %.2e' % (variant, l2, mx))
    assert l2 < 5e-6 and mx < 2e-5, (l2, mx)
    assert r['ops'] == r['ops32'] and len(r['kn']) == len(r['ops'])
    assert all(k.startswith('conv_split16') for k in r['kn']), r['kn']
    assert r['counts'] == (len(r['kn']), 1), (r['counts'], len(r['kn']))          # one stem launch per chunk (3 frames, one chunk)
    assert set(r['kn32']) == {'conv_f32'} and r['f32_split_launches'] == 0        # the yardstick stays on the f32-input MFMA
    assert not np.array_equal(r['out'], r['out32'])


# ------------------------------------------------------------------------------------------------
# 4. invariances, bit-exact
# ------------------------------------------------------------------------------------------------
def test_invariances_are_bit_exact():
    from pvr_habitat_amd.embeddings import HipResNet50
    L = _lib.lib()
    sd = synth.resnet50_state_dict(3, 'conv3')
    fr = torch.from_numpy(synth.smooth_frames(77, 5, 96, 128)).cuda()
    m = HipResNet50(sd, 'conv3', compute_dtype='f32s', max_batch=8)
    a = m(fr).clone()
    assert a.shape == (5, 2156) and torch.isfinite(a).all()
    assert torch.equal(m(fr[1:3]), a[1:3])                             # batch size
    out1 = torch.full_like(a, float('nan'))
    m.forward_into(fr, out1, lane=1)                                   # a second workspace (its zero border is written at ITS allocation)
    torch.cuda.synchronize()
    assert torch.equal(out1, a)
    wide = torch.full((5, 2156 + 37), float('nan'), device='cuda')     # a column block of a wider buffer (UberModel's writes)
    m.forward_into(fr, wide[:, 37:])
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 37:], a) and torch.isnan(wide[:, :37]).all()
    mc = HipResNet50(sd, 'conv3', compute_dtype='f32s', max_batch=8, chunk=3)
    s0 = L.pvr_debug_stem_split16_launches()
    b = mc(fr)
    assert L.pvr_debug_stem_split16_launches() - s0 == 2               # 5 frames in chunks of 3: one stem launch per chunk
    assert torch.equal(b, a)
    m.close(); mc.close()


# ------------------------------------------------------------------------------------------------
# 5. range: the high part of every activation is an f16
# ------------------------------------------------------------------------------------------------
def test_f32s_activation_range(monkeypatch):
    """Scaling bn1's affine by S scales every downstream activation by ~S (test_f16_activation_range).  (a) peak stage activation ~2.4e4: the parity bounds
    of test_whole_network_against_the_oracle hold and check_range is clean; (b) 16x larger: activations pass 65504, check_range names the launch and
    EmbeddingNet raises FloatingPointError on its first call, while compute_dtype='f32' (full fp32 range) embeds the same frames.  Arithmetic overflow to
    inf only: nothing here faults the device."""
    from oracle import encoder_oracle as eo
    from pvr_habitat_amd.embeddings import EmbeddingNet, HipResNet50
    torch.set_num_threads(8)
    sd = synth.resnet50_state_dict(1, 'conv5')
    fr = synth.smooth_frames(24, 2, 128, 128)
    d = torch.from_numpy(fr).cuda()
    taps = {}
    with torch.no_grad():
        eo.resnet50_features(sd, eo.preprocess(fr), 'conv5', taps=taps)
    peak = max(float(t.abs().max()) for t in taps.values())

    def scaled(S):
        s2 = dict(sd)
        s2['bn1.weight'] = sd['bn1.weight'] * S
        s2['bn1.bias'] = sd['bn1.bias'] * S
        return s2
    S = 2.4e4 / peak
    ref = eo.embed(scaled(S), fr, 'conv5', squeeze=False)
    m = HipResNet50(scaled(S), 'conv5', compute_dtype='f32s', max_batch=4)
    out = m(d).cpu().numpy()
    l2, mx = _relerr(out, ref)
    rel = _max_rel(out, ref)
    print('\n[f32s range] scale %.0f, oracle peak stage activation %.3g: rel-L2 %.2e max-norm %.2e max element-wise %.2e' % (S, peak * S, l2, mx, rel))
    assert np.isfinite(out).all() and l2 < 1e-4 and mx < 1e-4 and rel < 1e-3, (l2, mx, rel)
    assert m.check_range(d) is None
    assert torch.equal(m(d), torch.from_numpy(out).cuda())             # the check leaves the plan as it was
    m.close()
    big = scaled(16 * S)
    mo = HipResNet50(big, 'conv5', compute_dtype='f32s', max_batch=4)
    where = mo.check_range(d)
    print('[f32s range] 16x larger: first launch output outside the range: %s' % where)
    assert where is not None and (where.startswith('layer') or where.startswith('conv1'))
    mo.close()
    monkeypatch.setenv('PVR_SYNTHETIC_WEIGHTS', '1')
    net = EmbeddingNet('resnet50', pretrained=False, compute_dtype='f32s', max_batch=4)
    net.embedding.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in big.items()})
    with pytest.raises(FloatingPointError, match="compute_dtype='f32'") as ei:
        net(torch.from_numpy(fr))
    assert 'bf16' not in str(ei.value) and where.split('+')[0] in str(ei.value)
    net.close()
    net32 = EmbeddingNet('resnet50', pretrained=False, compute_dtype='f32', max_batch=4)
    net32.embedding.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in big.items()})
    o32 = net32(torch.from_numpy(fr))
    assert np.isfinite(o32).all() and _relerr(o32, eo.embed(big, fr, 'conv5', squeeze=False))[0] < 1e-4
    net32.close()
    # the PVR_F32 plan has the full range: its handle keeps refusing the check, with a message
    m32 = HipResNet50(sd, 'conv5', compute_dtype='f32', max_batch=4)
    with pytest.raises(RuntimeError, match='check_range'):
        m32.check_range(d)
    m32.close()


# ------------------------------------------------------------------------------------------------
# 6. surface
# ------------------------------------------------------------------------------------------------
def test_embeddingnet_surface(monkeypatch):
    from pvr_habitat_amd.embeddings import EmbeddingNet, stream_embed
    monkeypatch.setenv('PVR_SYNTHETIC_WEIGHTS', '1')
    fr = torch.from_numpy(synth.smooth_frames(23, 2, 64, 64))
    net = EmbeddingNet('moco_aug_uber_345', pretrained=False, compute_dtype='f32s', max_batch=4)
    assert net.out_size == 2156 + 2058 + 2048
    out = net(fr)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (2, 6262) and np.isfinite(out).all()
    assert all(m._dtype == _lib.PVR_F32S for m in net.embedding.models)
    alone = []
    for name in ('moco_aug_l3', 'moco_aug_l4', 'moco_aug'):
        one = EmbeddingNet(name, pretrained=False, compute_dtype='f32s', max_batch=4)
        alone.append(one(fr))
        one.close()
    np.testing.assert_array_equal(out, np.concatenate(alone, axis=1))
    np.testing.assert_array_equal(np.asarray(stream_embed(net, torch.cat([fr, fr, fr]), batch=4))[:2], out)
    net.close()


def test_save_embedded_obs_takes_the_mode(tmp_path, monkeypatch):
    """save_embedded_obs.run --compute_dtype f32s on a scene pickle in the reference's format: the rows of --compute_dtype f32, within the bound of
    test_against_the_f32_plan."""
    import pickle
    from pvr_habitat_amd import save_embedded_obs as S
    from pvr_habitat_amd.arguments import make_parser
    monkeypatch.setenv('PVR_SYNTHETIC_WEIGHTS', '1')
    lens = (5, 4)
    fr = synth.smooth_frames(31, 2 * sum(lens), 64, 64)
    obs_all = np.concatenate([fr[:sum(lens)], fr[sum(lens):]], axis=3)            # (N,64,64,6): frame + goal
    cuts = np.cumsum((0,) + lens)
    raw = dict(obs=[obs_all[a:b] for a, b in zip(cuts[:-1], cuts[1:])], action=[np.zeros(L, np.int64) for L in lens],
               reward=[np.zeros(L, np.float32) for L in lens], done=[np.eye(1, L, L - 1, dtype=bool)[0] for L in lens],
               true_state=[np.zeros((L, 12), np.float32) for L in lens])
    rows = {}
    for dt in ('f32s', 'f32'):
        d = tmp_path / dt
        d.mkdir()
        pickle.dump(raw, open(d / 'scene.pickle', 'wb'))
        S.run(make_parser().parse_args(['--data_path', str(d), '--env', 'scene', '--embedding_name', 'resnet50', '--source', 'pickle', '--compute_dtype', dt,
                                        '--embed_batch', '8']))
        rows[dt] = pickle.load(open(d / 'scene_resnet50.pickle', 'rb'))['obs']
    assert rows['f32s'].shape == (9, 4096) and rows['f32s'].dtype == np.float32 and np.isfinite(rows['f32s']).all()
    l2, mx = _relerr(rows['f32s'], rows['f32'])
    print('\n[save_embedded_obs f32s vs f32] rel-L2 %.2e max-norm %.2e' % (l2, mx))
    assert l2 < 5e-6 and mx < 2e-5 and not np.array_equal(rows['f32s'], rows['f32'])
