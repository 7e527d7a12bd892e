"""The fp32 reference-precision plan of the ViT encoders on the GPU (compute_dtype='f32' = PVR_F32 for CLIP ViT B/32, B/16 and MAE ViT B/16, L/16, H/14):
the fp32 attention kernel (csrc/vit_f32.hip) and conv_f32's activation epilogues against float64, whole networks against the fp32 oracle and against its
float64 restatement, the bit-exact invariances of the forward, the fp32 range, and the Python surface.  synth weights and frames only; references,
bounds and inputs are those of tests/vit_f32_refs.py (pinned on the CPU by tests/test_vit_f32_cpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_f32_refs as vr
from oracle import vit_kernel_refs as kr
from pvr_habitat_amd import synth, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SENTINEL32 = 0x5A5A5A5A
NAN32 = 0x7FC00000
GUARD = 3                                             # rows in front of and behind every output


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


# ------------------------------------------------------------------------------------------------------------------
# 1. attention
# ------------------------------------------------------------------------------------------------------------------
def _run_attention(qkv, T, heads):
    """qkv: CPU (nb, T, 3W) fp32.  One allocation holds qkv and a NaN tail of 32 ceil(T / 32) rows behind it; out sits between guard rows and is NaN
    before the launch.  Returns the CPU output (nb, T, W) after checking the guards."""
    nb, W = qkv.shape[0], qkv.shape[2] // 3
    TK = (T + 31) // 32 * 32
    buf = torch.full(((nb * T + TK) * 3 * W,), NAN32, dtype=torch.int32, device='cuda')
    buf[:nb * T * 3 * W] = qkv.view(torch.int32).reshape(-1).cuda()
    out = torch.full((GUARD + nb * T + GUARD, W), SENTINEL32, dtype=torch.int32, device='cuda')
    out[GUARD:GUARD + nb * T] = NAN32
    _lib.check(_lib.lib().pvr_op_attention(vp(buf), vp(out, GUARD * W * 4), T, W, heads, nb, _lib.PVR_F32, _lib.stream_ptr()))
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[:GUARD] == SENTINEL32).all() and (o[GUARD + nb * T:] == SENTINEL32).all(), 'attention wrote outside its rows'
    assert (buf[nb * T * 3 * W:] == NAN32).all()
    return o[GUARD:GUARD + nb * T].view(torch.float32).reshape(nb, T, W)


@pytest.mark.parametrize('T,heads,hd', vr.ATT_SHAPES)
def test_attention_f32_matches_float64(T, heads, hd):
    """every element within (2 D_q + (T + 8) u32) sum_k p_k |v_k| of the float64 result (vit_f32_refs.attention_ref_f32: fp32 arithmetic passes at <= 0.05 of
    it, P or q / k / v rounded to f16 fail by >= 4x); run to run and alone or in a batch: the same bits"""
    worst = {}
    for family in kr.ATT_FAMILIES:
        qkv = vr.attention_inputs_f32(family, T, heads, hd)
        ref, bound = vr.attention_ref_f32(qkv, heads)
        got = _run_attention(qkv, T, heads)
        assert torch.isfinite(got).all(), '%s: a NaN survived or was read (padded rows must read as zero)' % family
        worst[family] = kr.ratio(got, ref, bound)
        again = _run_attention(qkv, T, heads)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), '%s: two runs differ' % family
        alone = _run_attention(qkv[1:2].contiguous(), T, heads)                     # nb = 1: the middle item on its own
        assert torch.equal(alone[0].view(torch.int32), got[1].view(torch.int32)), '%s: the middle item alone differs from its rows in the batch' % family
    print('\n[attention f32 T %d heads %d hd %d] error / bound %s' % (T, heads, hd, {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


def test_attention_f32_refuses_what_is_not_built():
    L = _lib.lib()
    st = _lib.stream_ptr()
    a = torch.zeros(1 << 20, dtype=torch.float32, device='cuda')
    o = torch.full((1 << 18,), SENTINEL32, dtype=torch.int32, device='cuda')
    assert L.pvr_op_attention(vp(a), vp(o), 50, 64, 2, 1, _lib.PVR_F32, st) != 0                  # head dim 32
    assert L.pvr_op_attention(vp(a), vp(o), 289, 64, 1, 1, _lib.PVR_F32, st) != 0                 # more than 288 tokens
    assert L.pvr_op_attention(None, vp(o), 50, 64, 1, 1, _lib.PVR_F32, st) != 0
    assert L.pvr_op_attention(vp(a), None, 50, 64, 1, 1, _lib.PVR_F32, st) != 0
    assert L.pvr_op_attention(vp(a), vp(o), 50, 64, 1, 1, _lib.PVR_F32S, st) != 0                 # no split-product attention
    f = torch.zeros(1 << 14, dtype=torch.float32, device='cuda')
    assert L.pvr_op_layernorm(vp(f), None, None, None, vp(f), vp(f), vp(o), vp(o, 1 << 17), 4, 1, 768, 1e-5, 1, _lib.PVR_F32, st) != 0    # PVR_F32: fp32 output only
    torch.cuda.synchronize()
    assert (o == SENTINEL32).all(), 'a refused call launched something'
    assert L.pvr_op_layernorm(vp(f), None, None, None, vp(f), vp(f), vp(o), None, 4, 1, 768, 1e-5, 0, _lib.PVR_F32, st) == 0
    torch.cuda.synchronize()
    assert (o[:4 * 768] == 0).all() and (o[4 * 768:] == SENTINEL32).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. linear layer + activation (conv_f32 with k = 1)
# ------------------------------------------------------------------------------------------------------------------
LIN_CASES = [(768, 3072, 2, False), (768, 3072, 3, False), (3072, 768, 0, True), (640, 1280, 0, False)]


def _act(y, act):
    if act == 1:
        return y.clamp(min=0)
    if act == 2:
        return y * torch.sigmoid(1.702 * y)
    if act == 3:
        return torch.nn.functional.gelu(y)
    return y


def _linear_gpu(xd, wd, bd, rd, rows, cin, cout, act):
    y = torch.full((GUARD + rows + GUARD, cout), SENTINEL32, dtype=torch.int32, device='cuda')
    y[GUARD:GUARD + rows] = NAN32
    _lib.check(_lib.lib().pvr_op_conv2d_f32(vp(xd), vp(wd), vp(bd), vp(rd), vp(y, GUARD * cout * 4), rows, 1, 1, cin, cout, 1, 1, 0, act, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert (y[:GUARD] == SENTINEL32).all() and (y[GUARD + rows:] == SENTINEL32).all(), 'conv_f32 wrote outside its rows'
    return y[GUARD:GUARD + rows].view(torch.float32).cpu()


@pytest.mark.parametrize('rows', [1, 63, 65, 591])
@pytest.mark.parametrize('cin,cout,act,residual', LIN_CASES)
def test_linear_f32_with_the_vit_epilogues(cin, cout, act, residual, rows):
    """x W^T + b (+ residual), then the activation, against float64.  Yardstick: torch's fp32 evaluation of the same expression on the CPU - both are fp32
    evaluations that differ in summation order and libm only, so the kernel's max-norm and rel-L2 errors may be at most 4x torch's (an operand rounded to
    16 bits, or a 16-bit-grade exp / erf, is >= 100x off).  act 0 / 1 around it: the same bits before and after, and ReLU = max(., 0) of the plain result."""
    torch.set_num_threads(16)
    tag = 'lin32_%d_%d_%d_%d' % (cin, cout, act, rows)
    x = torch.from_numpy(synth.normal(29, tag + 'x', (rows, cin)))
    x[0::7] *= 8.0                                                                   # a few rows reach the GELU / QuickGELU tails
    x[3::11] *= -8.0
    w = torch.from_numpy(synth.normal(29, tag + 'w', (cout, cin), std=float(cin ** -0.5)))
    b = torch.from_numpy(synth.normal(29, tag + 'b', (cout,)))
    r = torch.from_numpy(synth.normal(29, tag + 'r', (rows, cout))) if residual else None
    ref = x.double() @ w.double().t() + b.double()
    y32 = x @ w.t() + b
    if residual:
        ref, y32 = ref + r.double(), y32 + r
    ref, y32 = _act(ref, act), _act(y32, act)
    xd, wd, bd, rd = x.cuda(), w.cuda(), b.cuda(), r.cuda() if residual else None
    plain = _linear_gpu(xd, wd, bd, rd, rows, cin, cout, 0)
    relu = _linear_gpu(xd, wd, bd, rd, rows, cin, cout, 1)
    got = _linear_gpu(xd, wd, bd, rd, rows, cin, cout, act)
    assert torch.isfinite(got).all()
    assert torch.equal(_linear_gpu(xd, wd, bd, rd, rows, cin, cout, 0).view(torch.int32), plain.view(torch.int32))
    assert torch.equal(_linear_gpu(xd, wd, bd, rd, rows, cin, cout, 1).view(torch.int32), relu.view(torch.int32))
    assert torch.equal(relu, plain.clamp(min=0))
    err = lambda a: (float((a.double() - ref).abs().max() / ref.abs().max()), float((a.double() - ref).norm() / ref.norm()))
    (gm, gl), (tm, tl) = err(got), err(y32)
    print('\n[linear f32 %d -> %d act %d res %d rows %d] kernel max-norm %.2e rel-L2 %.2e; torch fp32 %.2e / %.2e; ratios %.2f / %.2f'
          % (cin, cout, act, residual, rows, gm, gl, tm, tl, gm / tm, gl / tl))
    assert gm <= 4.0 * tm and gl <= 4.0 * tl, (gm, tm, gl, tl)


def test_linear_f32_refuses_an_unknown_activation():
    t = torch.zeros(64 * 64, device='cuda')
    o = torch.full((64 * 64,), SENTINEL32, dtype=torch.int32, device='cuda')
    assert _lib.lib().pvr_op_conv2d_f32(vp(t), vp(t), vp(t), None, vp(o), 4, 1, 1, 64, 64, 1, 1, 0, 4, _lib.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert (o == SENTINEL32).all()


# ------------------------------------------------------------------------------------------------------------------
# 3. whole networks
# ------------------------------------------------------------------------------------------------------------------
_NET = {}
TAPS = ('qkv0', 'att0', 'res0', 'fc0')


def _net_run(variant):
    """one f32 and one f16 forward, the fp32 oracle and its float64 restatement - computed once per case, shared, never changed"""
    if variant not in _NET:
        from pvr_habitat_amd.embeddings import HipResNet50
        torch.set_num_threads(16)
        mk_sd, mk_fr, heads, mae = vr.NET_CASES[variant]
        sd, fr = mk_sd(), mk_fr()
        taps = {}
        ref, ref64 = vr.oracle_pair(sd, fr, heads, mae, taps=taps)
        d = torch.from_numpy(fr).cuda()
        m = HipResNet50(sd, variant, compute_dtype='f32', max_batch=4)
        out = m(d).cpu().numpy()
        got_taps = {}
        if variant == 'clip_b32':
            for name in TAPS:
                m.debug_stop_after(name); m(d)
                got_taps[name] = m.tap(name, taps[name].numel()).cpu().numpy().reshape(tuple(taps[name].shape))
            m.debug_stop_after('')
            assert np.array_equal(m(d).cpu().numpy(), out)                              # the taps leave the plan as it was
        m.close()
        m16 = HipResNet50(sd, variant, compute_dtype='f16', max_batch=4)
        out16 = m16(d).cpu().numpy()
        m16.close()
        _NET[variant] = dict(out=out, out16=out16, ref=ref, ref64=ref64, taps={k: taps[k].numpy() for k in TAPS}, got_taps=got_taps)
    return _NET[variant]


@pytest.mark.parametrize('variant', sorted(vr.NET_CASES))
def test_whole_network_against_the_oracle(variant):
    """the bounds the project holds the PVR_F32 ResNets to: rel-L2 and max-norm < 1e-4, and the maximum ELEMENT-WISE relative error over every element above
    1 % of the maximum < 1e-3.  The f16 plan of the same weights is further than 1e-4 from the f32 output: the mode ran."""
    r = _net_run(variant)
    l2, mx, rel = vr.parity_figures(r['out'], r['ref'])
    d16 = vr.parity_figures(r['out16'], r['out'])[0]
    print('\n[%s f32] against the fp32 oracle: rel-L2 %.2e max-norm %.2e max element-wise %.2e;  f16 plan against f32 plan: rel-L2 %.2e' % (variant, l2, mx, rel, d16))
    assert r['out'].shape == r['ref'].shape and r['out'].dtype == np.float32 and np.isfinite(r['out']).all()
    assert l2 < 1e-4 and mx < 1e-4, (l2, mx)
    assert rel < 1e-3, rel
    assert d16 > 1e-4, d16


@pytest.mark.parametrize('variant', sorted(vr.NET_CASES))
def test_whole_network_against_float64(variant):
    """rel-L2 to the float64 restatement at most 8x the fp32 oracle's own on the same input: both are fp32 evaluations of 12 - 24 blocks in a different
    order (a random walk), while one f16 rounding class anywhere in the network costs >= 100x"""
    r = _net_run(variant)
    mine = vr.parity_figures(r['out'], r['ref64'])[0]
    oracle = vr.parity_figures(r['ref'], r['ref64'])[0]
    print('\n[%s f32] rel-L2 to float64: plan %.2e, fp32 oracle %.2e, ratio %.2f' % (variant, mine, oracle, mine / oracle))
    assert mine <= 8.0 * oracle, (mine, oracle)


def test_block0_taps_against_the_oracle():
    """clip_b32: the plan's fp32 buffers after block 0's QKV GEMM, attention, first residual and activation, every row of every image"""
    r = _net_run('clip_b32')
    errs = {}
    for name in TAPS:
        g, t = r['got_taps'][name], r['taps'][name]
        assert np.isfinite(g).all(), name
        errs[name] = float(np.abs(g.astype(np.float64) - t).max() / np.abs(t).max())
    print('\n[clip_b32 f32 taps] max-norm %s' % {k: '%.2e' % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-5, errs


# ------------------------------------------------------------------------------------------------------------------
# 4. invariances, bit-exact
# ------------------------------------------------------------------------------------------------------------------
def test_invariances_are_bit_exact():
    from pvr_habitat_amd.embeddings import HipResNet50
    sd = synth.clip_vit_state_dict(1, patch=32)
    fr = torch.from_numpy(synth.smooth_frames(41, 3, 224, 224)).cuda()
    m16a = HipResNet50(sd, 'clip_b32', compute_dtype='f16', max_batch=4)
    before = m16a(fr).clone()
    m16a.close()
    m = HipResNet50(sd, 'clip_b32', compute_dtype='f32', max_batch=4)
    a = m(fr).clone()
    assert a.shape == (3, 512) and torch.isfinite(a).all()
    assert torch.equal(m(fr[1:2]), a[1:2])                             # batch size
    out1 = torch.full_like(a, float('nan'))
    m.forward_into(fr, out1, lane=1)                                   # a second workspace
    torch.cuda.synchronize()
    assert torch.equal(out1, a)
    wide = torch.full((3, 512 + 37), float('nan'), device='cuda')      # a column block of a wider buffer (UberModel's writes)
    m.forward_into(fr, wide[:, 37:])
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 37:], a) and torch.isnan(wide[:, :37]).all()
    mc = HipResNet50(sd, 'clip_b32', compute_dtype='f32', max_batch=4, chunk=2)
    assert torch.equal(mc(fr), a)                                      # 3 frames in chunks of 2
    m.close(); mc.close()
    m16b = HipResNet50(sd, 'clip_b32', compute_dtype='f16', max_batch=4)
    assert torch.equal(m16b(fr), before)                               # the 16-bit plan is what it was, before and after an f32 handle
    assert not torch.equal(before, a)
    m16b.close()


# ------------------------------------------------------------------------------------------------------------------
# 5. range: the residual stream beyond 65504
# ------------------------------------------------------------------------------------------------------------------
def test_f32_has_the_full_range():
    """ln_pre's affine scaled until block 0's residual passes 65504 (the scale comes from the ORACLE's res0 tap): the f32 plan embeds within the network
    bounds.  Arithmetic only - nothing here faults a device; a PVR_F32 ViT handle keeps refusing check_range."""
    from oracle import vit_oracle as vo
    from pvr_habitat_amd.embeddings import HipResNet50
    torch.set_num_threads(16)
    sd = synth.clip_vit_state_dict(1, patch=32)
    fr = synth.smooth_frames(41, 2, 224, 224)
    taps = {}
    with torch.no_grad():
        vo.encode_image(sd, vo.preprocess(fr), taps=taps)
    S = 2.0 * 65504.0 / float(taps['res0'].abs().max())
    big = dict(sd)
    big['visual.ln_pre.weight'] = vo._t(sd['visual.ln_pre.weight']) * S
    big['visual.ln_pre.bias'] = vo._t(sd['visual.ln_pre.bias']) * S
    taps = {}
    with torch.no_grad():
        ref = vo.encode_image(big, vo.preprocess(fr), taps=taps).numpy()
    peak = float(taps['res0'].abs().max())
    assert peak > 65504.0, peak
    m = HipResNet50(big, 'clip_b32', compute_dtype='f32', max_batch=4)
    d = torch.from_numpy(fr).cuda()
    out = m(d).cpu().numpy()
    l2, mx, rel = vr.parity_figures(out, ref)
    print('\n[f32 range] scale %.0f, oracle block-0 residual peak %.3g: rel-L2 %.2e max-norm %.2e max element-wise %.2e' % (S, peak, l2, mx, rel))
    assert np.isfinite(out).all() and l2 < 1e-4 and mx < 1e-4 and rel < 1e-3, (l2, mx, rel)
    m.debug_stop_after('res0'); m(d)
    got = m.tap('res0', taps['res0'].numel()).cpu().numpy()
    assert np.isfinite(got).all() and float(np.abs(got).max()) > 65504.0          # the plan's own residual is out there too
    m.debug_stop_after('')
    with pytest.raises(RuntimeError, match='check_range'):
        m.check_range(d)
    m.close()


# ------------------------------------------------------------------------------------------------------------------
# 6. surface
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,out_size', [('clip_vit', 512), ('mae_base', 768)])
def test_embeddingnet_surface(name, out_size, monkeypatch):
    from pvr_habitat_amd.embeddings import EmbeddingNet, stream_embed
    monkeypatch.setenv('PVR_SYNTHETIC_WEIGHTS', '1')
    fr = torch.from_numpy(synth.smooth_frames(23, 2, 64, 64))
    net = EmbeddingNet(name, compute_dtype='f32', max_batch=4)
    assert net.out_size == out_size
    out = net(fr)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (2, out_size) and np.isfinite(out).all()
    members = [m for m in net.modules() if hasattr(m, '_dtype')]
    assert members and all(m._dtype == _lib.PVR_F32 for m in members)
    np.testing.assert_array_equal(np.asarray(stream_embed(net, torch.cat([fr, fr, fr]), batch=4))[:2], out)
    net.close()


def test_save_embedded_obs_takes_the_mode(tmp_path, monkeypatch):
    """save_embedded_obs.run --embedding_name clip_vit --compute_dtype f32 on a scene pickle in the reference's format: the rows of the same job in f16
    within 2e-3 rel-L2 (the f16 plan's own parity bound, doubled) - and not the same rows"""
    import pickle
    from pvr_habitat_amd import save_embedded_obs as S
    from pvr_habitat_amd.arguments import make_parser
    monkeypatch.setenv('PVR_SYNTHETIC_WEIGHTS', '1')
    lens = (3, 2)
    fr = synth.smooth_frames(31, 2 * sum(lens), 64, 64)
    obs_all = np.concatenate([fr[:sum(lens)], fr[sum(lens):]], axis=3)            # (N,64,64,6): frame + goal
    cuts = np.cumsum((0,) + lens)
    raw = dict(obs=[obs_all[a:b] for a, b in zip(cuts[:-1], cuts[1:])], action=[np.zeros(L, np.int64) for L in lens],
               reward=[np.zeros(L, np.float32) for L in lens], done=[np.eye(1, L, L - 1, dtype=bool)[0] for L in lens],
               true_state=[np.zeros((L, 12), np.float32) for L in lens])
    rows = {}
    for dt in ('f32', 'f16'):
        d = tmp_path / dt
        d.mkdir()
        pickle.dump(raw, open(d / 'scene.pickle', 'wb'))
        S.run(make_parser().parse_args(['--data_path', str(d), '--env', 'scene', '--embedding_name', 'clip_vit', '--source', 'pickle', '--compute_dtype', dt,
                                        '--embed_batch', '8']))
        rows[dt] = pickle.load(open(d / 'scene_clip_vit.pickle', 'rb'))['obs']
    assert rows['f32'].shape == (5, 1024) and rows['f32'].dtype == np.float32 and np.isfinite(rows['f32']).all()
    l2, mx, _ = vr.parity_figures(rows['f16'], rows['f32'])
    print('\n[save_embedded_obs clip_vit f16 vs f32] rel-L2 %.2e max-norm %.2e' % (l2, mx))
    assert l2 < 2e-3 and not np.array_equal(rows['f32'], rows['f16'])
