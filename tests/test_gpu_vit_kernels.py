"""The ViT kernels of csrc/vit.hip one by one (pvr_op_attention / pvr_op_layernorm / pvr_op_cls_head: the launch dispatchers the encoder
plans use) against the float64 references and derived elementwise bounds of oracle/vit_kernel_refs.py - every attention instantiation
with its edge token counts, every LayerNorm width and path, guards around every output."""
import ctypes as C

import pytest
import torch

from oracle import vit_kernel_refs as kr
from pvr_habitat_amd import _lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

DT = {'f16': _lib.PVR_F16, 'bf16': _lib.PVR_BF16}
SENTINEL16 = 0x5A5A                                   # guard rows of 16-bit outputs (a finite value in both types)
SENTINEL32 = 0x5A5A5A5A
NAN16 = {'f16': 0x7E00, 'bf16': 0x7FC0}
GUARD = 3                                             # rows in front of and behind every output


def vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _bits16(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------
# (T, heads, head dim): key count TK = 32 ceil(T / 32) -> instantiation
ATT_GRID = [
    (1, 1, 64), (16, 2, 64), (17, 12, 64), (32, 1, 64),                       # TK 32: runtime-NT fallback <64,18,false>
    (33, 2, 64), (50, 12, 64), (63, 1, 64), (64, 2, 64),                      # TK 64: <64,4,true>
    (65, 1, 64), (101, 12, 64), (128, 2, 64),                                 # TK 96 / 128: runtime-NT fallback
    (193, 1, 64), (197, 12, 64), (224, 2, 64),                                # TK 224: <64,14,true>
    (225, 2, 64), (257, 12, 64), (288, 1, 64),                                # TK 256 / 288: <64,18,false>, 288 with every tile full
    (257, 2, 80), (288, 2, 80),                                               # head dim 80, TK 288: <80,18,true>
    (50, 2, 80), (101, 2, 80),                                                # head dim 80, other key counts: <80,18,false>
]


def _run_attention(qkv, T, heads, dt):
    """qkv: CPU (nb, T, 3W) 16-bit.  One allocation holds qkv and a NaN tail of TK rows behind it; out sits between guard rows and is
    NaN before the launch.  Returns the CPU output (nb, T, W) after checking the guards."""
    nb, W = qkv.shape[0], qkv.shape[2] // 3
    TK = (T + 31) // 32 * 32
    buf = torch.full(((nb * T + TK) * 3 * W,), NAN16[dt], dtype=torch.int16, device='cuda')
    buf[:nb * T * 3 * W] = _bits16(qkv).reshape(-1).cuda()
    out = torch.full((GUARD + nb * T + GUARD, W), SENTINEL16, dtype=torch.int16, device='cuda')
    out[GUARD:GUARD + nb * T] = NAN16[dt]
    _lib.check(_lib.lib().pvr_op_attention(vp(buf), vp(out, GUARD * W * 2), T, W, heads, nb, DT[dt], _lib.stream_ptr()))
    torch.cuda.synchronize()
    o = out.cpu()
    assert (o[:GUARD] == SENTINEL16).all() and (o[GUARD + nb * T:] == SENTINEL16).all(), 'attention wrote outside its rows'
    assert (buf[nb * T * 3 * W:] == NAN16[dt]).all()
    return o[GUARD:GUARD + nb * T].view(kr.TORCH_DT[dt]).reshape(nb, T, W)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('T,heads,hd', ATT_GRID)
def test_attention_matches_float64(T, heads, hd, dt):
    worst = {}
    for family in kr.ATT_FAMILIES:
        qkv = kr.attention_inputs(family, T, heads, hd, 3, dt)
        ref, bound = kr.attention_ref(qkv, heads)
        got = _run_attention(qkv, T, heads, dt)
        assert torch.isfinite(got.float()).all(), '%s: a NaN survived or was read (padded rows must read as zero)' % family
        worst[family] = kr.ratio(got, ref, bound)
        again = _run_attention(qkv, T, heads, dt)
        assert torch.equal(_bits16(got), _bits16(again)), '%s: two runs differ' % family
        alone = _run_attention(qkv[1:2].contiguous(), T, heads, dt)                 # nb = 1: the middle item on its own
        assert torch.equal(_bits16(alone[0]), _bits16(got[1])), '%s: the middle item alone differs from its rows in the batch' % family
    print('\n[attention T %d heads %d hd %d %s] error / bound %s' % (T, heads, hd, dt, {k: '%.2f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------
def _run_layernorm(x, asm, g, b, rows, T, W, eps, normalize, dt, want_f32=True, want_h=True):
    """x: CPU (rows, W) fp32 or None; asm: (patch_emb, cls, pos) or None.  Returns (out_f32 or None, out_h or None) on the CPU, guards checked."""
    L = _lib.lib()
    dev = lambda t: t.contiguous().cuda() if t is not None else None
    xd, gd, bd = dev(x), dev(g), dev(b)
    ped, clsd, posd = (dev(t) for t in asm) if asm else (None, None, None)
    of = oh = None
    if want_f32:
        of = torch.full((GUARD + rows + GUARD, W), SENTINEL32, dtype=torch.int32, device='cuda')
        of[GUARD:GUARD + rows] = 0x7FC00000
    if want_h:
        oh = torch.full((GUARD + rows + GUARD, W), SENTINEL16, dtype=torch.int16, device='cuda')
        oh[GUARD:GUARD + rows] = NAN16[dt]
    _lib.check(L.pvr_op_layernorm(vp(xd), vp(ped), vp(clsd), vp(posd), vp(gd), vp(bd), vp(of, GUARD * W * 4) if want_f32 else None,
                                  vp(oh, GUARD * W * 2) if want_h else None, rows, T, W, eps, normalize, DT[dt], _lib.stream_ptr()))
    torch.cuda.synchronize()
    rf = rh = None
    if want_f32:
        o = of.cpu()
        assert (o[:GUARD] == SENTINEL32).all() and (o[GUARD + rows:] == SENTINEL32).all(), 'layernorm wrote fp32 outside its rows'
        rf = o[GUARD:GUARD + rows].view(torch.float32)
        assert torch.isfinite(rf).all()
    if want_h:
        o = oh.cpu()
        assert (o[:GUARD] == SENTINEL16).all() and (o[GUARD + rows:] == SENTINEL16).all(), 'layernorm wrote 16-bit outside its rows'
        rh = o[GUARD:GUARD + rows].view(kr.TORCH_DT[dt])
        assert torch.isfinite(rh.float()).all()
    return rf, rh


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('W', [768, 1024, 1280])
def test_layernorm_plain_matches_float64(W, dt):
    g, b = kr.layernorm_params(W)
    worst = {}
    cases = [('unit', rows, 1e-5) for rows in (1, 3, 4, 5, 9)]                       # ragged last block of four rows, guards behind it
    cases += [('small_var', 5, 1e-5), ('small_var', 5, 1e-6), ('offset', 5, 1e-6), ('outlier', 5, 1e-5), ('constant', 5, 1e-6)]
    for family, rows, eps in cases:
        x = kr.layernorm_rows(family, rows, W)
        rf, rh = _run_layernorm(x, None, g, b, rows, 1, W, eps, 1, dt)
        ref, bound = kr.layernorm_ref(x, g, b, eps)
        refh, boundh = kr.layernorm_ref(x, g, b, eps, out_dt=dt)
        key = '%s/%d/%g' % (family, rows, eps)
        worst[key] = (kr.ratio(rf, ref, bound), kr.ratio(rh, refh, boundh))
        if family == 'constant':
            assert torch.equal(rf, b.expand(rows, W)), 'a constant row must give beta exactly'
        if family == 'small_var':                                                   # each output alone: the same bits as both at once
            only_f, none_h = _run_layernorm(x, None, g, b, rows, 1, W, eps, 1, dt, want_h=False)
            none_f, only_h = _run_layernorm(x, None, g, b, rows, 1, W, eps, 1, dt, want_f32=False)
            assert none_h is None and none_f is None
            assert torch.equal(only_f, rf) and torch.equal(_bits16(only_h), _bits16(rh))
    x = kr.layernorm_rows('offset', 5, W)                                           # normalize = 0: a copy (fp32 exact, 16-bit rounded once)
    rf, rh = _run_layernorm(x, None, None, None, 5, 1, W, 1e-5, 0, dt)
    assert torch.equal(rf, x) and torch.equal(_bits16(rh), _bits16(kr.round_to(x, dt)))
    print('\n[layernorm plain W %d %s] error / bound (fp32 out, 16-bit out) %s' % (W, dt, {k: '%.2f %.2f' % v for k, v in worst.items()}))
    assert max(max(v) for v in worst.values()) <= 1.0, worst


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('W', [768, 1024, 1280])
def test_layernorm_assembly_matches_float64(W, dt):
    g, b = kr.layernorm_params(W)
    worst = {}
    for T in (2, 50, 197):
        pe, cls, pos = kr.assembly_inputs(3, T, W)
        x64 = kr.assemble(pe.double(), cls.double(), pos.double(), T)
        for normalize, eps in ((1, 1e-5), (0, 1e-6)):
            rf, rh = _run_layernorm(None, (pe, cls, pos), g, b, 3 * T, T, W, eps, normalize, dt)
            ref, bound = kr.layernorm_ref(x64, g, b, eps, normalize, assembled=True)
            refh, boundh = kr.layernorm_ref(x64, g, b, eps, normalize, out_dt=dt, assembled=True)
            worst['T%d/norm%d' % (T, normalize)] = (kr.ratio(rf, ref, bound), kr.ratio(rh, refh, boundh))
            if not normalize:                                                       # row 0 of every item is cls + pos[0], patches follow per item
                v = kr.assemble(pe, cls, pos, T)
                assert torch.equal(rf, v)
                assert torch.equal(rf.reshape(3, T, W)[:, 0], (cls + pos[0]).expand(3, W))
    print('\n[layernorm assembly W %d %s] error / bound (fp32 out, 16-bit out) %s' % (W, dt, {k: '%.2f %.2f' % v for k, v in worst.items()}))
    assert max(max(v) for v in worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------
# cls_head
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_dim', [512, 0])
@pytest.mark.parametrize('W', [768, 1024, 1280])
def test_cls_head_matches_float64(W, out_dim):
    L = _lib.lib()
    g, b = kr.layernorm_params(W)
    worst = {}
    for T, eps in ((1, 1e-5), (50, 1e-6)):
        x, proj = kr.cls_head_inputs(3, T, W, out_dim)
        od = out_dim or W                                                           # MAE: no projection, the normalised token is the output
        stride = od + 8
        out = torch.full((GUARD + 3 + GUARD, stride), SENTINEL32, dtype=torch.int32, device='cuda')
        out[GUARD:GUARD + 3, :od] = 0x7FC00000
        xd, gd, bd, pd = x.cuda(), g.cuda(), b.cuda(), proj.contiguous().cuda() if proj is not None else None
        _lib.check(L.pvr_op_cls_head(vp(xd), vp(gd), vp(bd), vp(pd), vp(out, GUARD * stride * 4), stride, 3, T, W, od, eps, _lib.stream_ptr()))
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[:GUARD] == SENTINEL32).all() and (o[GUARD + 3:] == SENTINEL32).all() and (o[:, od:] == SENTINEL32).all(), \
            'cls_head wrote outside its rows or into the gap between them'
        got = o[GUARD:GUARD + 3, :od].contiguous().view(torch.float32)
        ref, bound = kr.cls_head_ref(x, g, b, proj, T, eps)
        worst['T%d' % T] = kr.ratio(got, ref, bound)
    print('\n[cls_head W %d out_dim %s] error / bound %s' % (W, out_dim or 'none', {k: '%.3f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------
# shapes that are not built are refused before any launch
# ------------------------------------------------------------------------------------------------------------------
def test_unsupported_shapes_are_refused():
    L = _lib.lib()
    st = _lib.stream_ptr()
    a = torch.zeros(1 << 20, dtype=torch.int16, device='cuda')
    o = torch.full((1 << 18,), SENTINEL16, dtype=torch.int16, device='cuda')
    f = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    of = torch.full((1 << 16,), SENTINEL32, dtype=torch.int32, device='cuda')
    assert L.pvr_op_attention(vp(a), vp(o), 50, 64, 2, 1, DT['f16'], st) != 0                   # head dim 32
    assert L.pvr_op_attention(vp(a), vp(o), 289, 64, 1, 1, DT['f16'], st) != 0                  # more than 288 tokens
    assert L.pvr_op_attention(None, vp(o), 50, 64, 1, 1, DT['f16'], st) != 0
    assert L.pvr_op_attention(vp(a), None, 50, 64, 1, 1, DT['f16'], st) != 0
    assert L.pvr_op_layernorm(vp(f), None, None, None, vp(f), vp(f), vp(of), vp(o), 4, 1, 512, 1e-5, 1, DT['f16'], st) != 0     # width 512
    assert L.pvr_op_layernorm(None, None, None, None, vp(f), vp(f), vp(of), vp(o), 4, 1, 768, 1e-5, 1, DT['f16'], st) != 0
    assert L.pvr_op_layernorm(vp(f), None, None, None, vp(f), vp(f), None, None, 4, 1, 768, 1e-5, 1, DT['f16'], st) != 0
    assert L.pvr_op_cls_head(vp(f), vp(f), vp(f), None, vp(of), 512, 2, 1, 512, 512, 1e-5, st) != 0                           # width 512
    assert L.pvr_op_cls_head(None, vp(f), vp(f), None, vp(of), 768, 2, 1, 768, 768, 1e-5, st) != 0
    torch.cuda.synchronize()
    assert (o == SENTINEL16).all() and (of == SENTINEL32).all(), 'a refused call launched something'
