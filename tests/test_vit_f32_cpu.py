"""The fp32 reference-precision plan of the ViT encoders (compute_dtype='f32' = PVR_F32 for CLIP ViT B/32, B/16 and MAE ViT B/16, L/16, H/14), pinned on the
CPU: what pvr_encoder_create takes and keeps refusing, the attention bound of tests/test_gpu_vit_f32.py shown to pass fp32 arithmetic and to fail 16-bit
arithmetic before any GPU is involved, and the float64 restatement of the oracle the GPU test measures against."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import vit_f32_refs as vr
from oracle import vit_kernel_refs as kr
from pvr_habitat_amd import _lib

VIT_ARCHS = {'CLIP_VIT_B32': 3, 'CLIP_VIT_B16': 4, 'MAE_VIT_B16': 5, 'MAE_VIT_L16': 7, 'MAE_VIT_H14': 8}
CLIP_RN50 = 9
PVR_ERR_INVALID = 1


def _create(arch, dtype, max_batch=4):
    h = C.c_void_p()
    d = _lib.EncoderDesc(arch=arch, dtype=dtype, max_batch=max_batch, chunk=0, resize=256 if arch in (5, 7, 8) else 224, crop=224)
    return _lib.lib().pvr_encoder_create(C.byref(d), C.byref(h)), h


@pytest.mark.parametrize('arch', sorted(VIT_ARCHS))
def test_create_takes_f32_for_every_vit(arch):
    L = _lib.lib()
    st, h = _create(VIT_ARCHS[arch], _lib.PVR_F32)
    assert st == 0 and h.value, _lib.last_error()
    try:
        assert L.pvr_encoder_out_size(h) == {'CLIP_VIT_B32': 512, 'CLIP_VIT_B16': 512, 'MAE_VIT_B16': 768, 'MAE_VIT_L16': 1024, 'MAE_VIT_H14': 1280}[arch]
    finally:
        L.pvr_encoder_destroy(h)


@pytest.mark.parametrize('arch', sorted(VIT_ARCHS))
def test_f32s_stays_refused_for_every_vit(arch):
    st, h = _create(VIT_ARCHS[arch], _lib.PVR_F32S)
    assert st == PVR_ERR_INVALID and not h.value
    assert 'ResNet family' in _lib.last_error(), _lib.last_error()


def test_clip_rn50_refuses_both_fp32_types():
    for dt in (_lib.PVR_F32, _lib.PVR_F32S):
        st, h = _create(CLIP_RN50, dt)
        assert st == PVR_ERR_INVALID and not h.value
        assert 'ResNet family' in _lib.last_error(), _lib.last_error()


def test_host_backend_refuses_a_vit_handle():
    """the CPU plan is the torchvision ResNet family's: a PVR_F32 ViT handle switched to it is refused at finalize, before any weight is asked for"""
    L = _lib.lib()
    st, h = _create(VIT_ARCHS['CLIP_VIT_B32'], _lib.PVR_F32)
    assert st == 0
    try:
        assert L.pvr_encoder_set_host_backend(h, 1) == 0
        assert L.pvr_encoder_finalize(h) == PVR_ERR_INVALID
        assert 'ResNet family has a CPU plan' in _lib.last_error(), _lib.last_error()
    finally:
        L.pvr_encoder_destroy(h)
    from pvr_habitat_amd.embeddings import HipResNet50
    m = HipResNet50({}, 'clip_b32', compute_dtype='f32', max_batch=2, host=True)          # the Python surface refuses before it creates a handle
    with pytest.raises(NotImplementedError, match='CPU plan'):
        m._build()


@pytest.mark.parametrize('T,heads,hd', vr.ATT_SHAPES)
def test_attention_bound_passes_fp32_and_fails_16_bit(T, heads, hd):
    """torch's fp32 attention stays far under the bound in every family; P rounded to f16, and q / k / v rounded to f16, exceed it in the 'dominant' family
    wherever there is more than one key tile's worth of mass to round (T >= 17)"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst, mut = {}, {}
    for family in kr.ATT_FAMILIES:
        qkv = vr.attention_inputs_f32(family, T, heads, hd)
        assert not torch.equal(qkv, qkv.bfloat16().float()) and not torch.equal(qkv, qkv.half().float())
        ref, bound = vr.attention_ref_f32(qkv, heads)
        worst[family] = kr.ratio(vr.attention_emulate_f32(qkv, heads), ref, bound)
        if family == 'dominant':
            mut = {m: kr.ratio(vr.attention_emulate_f32(qkv, heads, m), ref, bound) for m in vr.ATT_MUTANTS}
    print('\n[attention bound T %d heads %d hd %d] fp32 error / bound %s; mutants (dominant) %s'
          % (T, heads, hd, {k: '%.3f' % v for k, v in worst.items()}, {k: '%.1f' % v for k, v in mut.items()}))
    assert max(worst.values()) <= 1.0, worst
    if T >= 17:
        assert min(mut.values()) > 1.0, mut


@pytest.mark.parametrize('variant', ['clip_b32', 'mae_b16'])
def test_fp32_oracle_against_its_float64_restatement(variant):
    """the yardstick of the GPU test's second bound: the fp32 oracle is within 1e-5 rel-L2 of the same code in float64"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    mk_sd, mk_fr, heads, mae = vr.NET_CASES[variant]
    ref, ref64 = vr.oracle_pair(mk_sd(), mk_fr(), heads, mae)
    l2, mx, rel = vr.parity_figures(ref, ref64)
    print('\n[%s] fp32 oracle against float64: rel-L2 %.2e max-norm %.2e max element-wise %.2e' % (variant, l2, mx, rel))
    assert ref.shape == ref64.shape and 0.0 < l2 < 1e-5, l2
