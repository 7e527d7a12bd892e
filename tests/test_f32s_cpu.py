"""The f32s compute type (PVR_F32S: fp32 storage, every product on the 16-bit matrix pipe as an exact (hi, lo) f16 split product), pinned on the CPU:
the constant and its spellings, the launch plan of a handle that was never finalized, what pvr_encoder_create / pvr_encoder_set_host_backend refuse, and the
arithmetic itself - the split product emulated through a whole network with torch on the CPU against the fp32 oracle, at the bounds the GPU test
(tests/test_gpu_f32s.py) holds the kernels to, so that those bounds are properties of the arithmetic and not of one kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pvr_habitat_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = {'RESNET50': 0, 'RESNET50_L4': 1, 'RESNET50_L3': 2, 'RESNET18': 10, 'RESNET34': 11}
CLIP_VIT_B32, CLIP_RN50 = 3, 9
PVR_ERR_INVALID = 1
MAX_BATCH = 256


def _create(arch, dtype, max_batch=MAX_BATCH):
    h = C.c_void_p()
    d = _lib.EncoderDesc(arch=arch, dtype=dtype, max_batch=max_batch, chunk=0, resize=256, crop=224)
    return _lib.lib().pvr_encoder_create(C.byref(d), C.byref(h)), h


def _names(fn, h, *front):
    out, buf, i = [], C.create_string_buffer(256), 3
    while fn(h, *front, i, buf, 256) > 0:
        out.append(buf.value.decode())
        i += 1
    return out


def test_dtype_constant_and_spellings():
    from pvr_habitat_amd.embeddings import _dtype_from_env
    assert _dtype_from_env('f32s') == _dtype_from_env('f32_split') == _lib.PVR_F32S == 3
    assert _dtype_from_env('F32S') == 3 and _dtype_from_env('f32') == _lib.PVR_F32 == 2
    with open(os.path.join(ROOT, 'include', 'pvr_hip.h')) as f:
        assert re.search(r'^#define PVR_F32S 3$', f.read(), re.M)


def test_dtype_from_the_environment(monkeypatch):
    from pvr_habitat_amd.embeddings import _dtype_from_env
    monkeypatch.setenv('PVR_DTYPE', 'f32s')
    assert _dtype_from_env() == _lib.PVR_F32S
    from pvr_habitat_amd import arguments
    p = arguments.make_parser()                               # --compute_dtype offers both fp32 modes; the default stays
    assert p.parse_args(['--compute_dtype', 'f32s']).compute_dtype == 'f32s' and p.parse_args(['--compute_dtype', 'f32']).compute_dtype == 'f32'
    assert p.parse_args([]).compute_dtype is None


@pytest.mark.parametrize('arch', sorted(ARCH))
def test_plan_of_an_unfinalized_handle(arch):
    """the same op list as the PVR_F32 handle of the architecture; every launch conv_split16, for every batch size - no fused plan, no split-K, no frame kernels"""
    L = _lib.lib()
    st, h = _create(ARCH[arch], _lib.PVR_F32S)
    assert st == 0, _lib.last_error()
    st32, h32 = _create(ARCH[arch], _lib.PVR_F32)
    assert st32 == 0, _lib.last_error()
    try:
        ops = _names(L.pvr_encoder_launch_name, h)
        assert ops == _names(L.pvr_encoder_launch_name, h32) and ops[-1] == 'pool/flatten' and len(ops) > 17
        nconv = len(ops) - 1
        for n in range(1, MAX_BATCH + 1):
            kn = _names(L.pvr_encoder_launch_kernel, h, n)
            assert len(kn) == nconv and set(kn) <= {'conv_split16', 'conv_split16(pair)'}, (arch, n, kn)
        # ... also in the low-latency plan and with the fusion switch off: the mode has one plan
        _lib.check(L.pvr_encoder_set_low_latency(h, 1))
        _lib.check(L.pvr_encoder_debug_set_fusion(h, 0))
        assert _names(L.pvr_encoder_launch_name, h) == ops
        for n in (1, 2, 4, 5, 256):
            assert set(_names(L.pvr_encoder_launch_kernel, h, n)) <= {'conv_split16', 'conv_split16(pair)'}
        assert set(_names(L.pvr_encoder_launch_kernel, h32, 3)) == {'conv_f32'}          # the yardstick keeps its kernel
    finally:
        L.pvr_encoder_destroy(h)
        L.pvr_encoder_destroy(h32)


def test_refusals():
    L = _lib.lib()
    for arch in (CLIP_RN50, CLIP_VIT_B32):
        st, h = _create(arch, _lib.PVR_F32S)
        assert st == PVR_ERR_INVALID and not h.value
        assert 'ResNet family' in _lib.last_error(), _lib.last_error()
    st, h = _create(ARCH['RESNET50'], _lib.PVR_F32S, 4)
    assert st == 0
    try:
        assert L.pvr_encoder_set_host_backend(h, 1) == PVR_ERR_INVALID
        assert 'PVR_F32' in _lib.last_error()
        assert L.pvr_encoder_set_host_backend(h, 0) == 0
    finally:
        L.pvr_encoder_destroy(h)
    st, h = _create(ARCH['RESNET50'], _lib.PVR_F32, 4)                                   # the CPU plan keeps taking PVR_F32
    assert st == 0
    try:
        assert L.pvr_encoder_set_host_backend(h, 1) == 0
    finally:
        L.pvr_encoder_destroy(h)


# ------------------------------------------------------------------------------------------------
# the arithmetic: x w = xh wh + 2^-11 (xh wl + xl wh) (+ 2^-22 xl wl, dropped), xh = f16(x), xl = f16(2^11 (x - xh)), products exact in fp32
# ------------------------------------------------------------------------------------------------
def _split(t):
    hi = t.to(torch.float16).float()
    return hi, ((t - hi) * 2048.0).to(torch.float16).float()


def split_conv_bn(eo):
    """oracle.encoder_oracle._conv_bn with the convolution as the split product of the BN-folded fp32 weights (what finalize packs)"""
    def conv_bn(sd, conv, bn, x, stride=1, pad=0, q=None):
        w = eo._t(sd[conv + '.weight'])
        b = eo._t(sd[conv + '.bias']) if (conv + '.bias') in sd else None
        scale = eo._t(sd[bn + '.weight']) / torch.sqrt(eo._t(sd[bn + '.running_var']) + eo.BN_EPS)
        shift = eo._t(sd[bn + '.bias']) - eo._t(sd[bn + '.running_mean']) * scale
        if b is not None:
            shift = shift + b * scale
        wh, wl = _split(w * scale.view(-1, 1, 1, 1))
        xh, xl = _split(x)
        y = F.conv2d(xh, wh, None, stride, pad) + (F.conv2d(xh, wl, None, stride, pad) + F.conv2d(xl, wh, None, stride, pad)) * (1.0 / 2048.0)
        return y + shift.view(1, -1, 1, 1)
    return conv_bn


def parity_figures(out, ref):
    """(rel-L2, max-norm, the MAXIMUM relative error over every element above 1 % of the reference's largest magnitude)"""
    a, b = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    big = np.abs(b) > 0.01 * np.abs(b).max()
    return (float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max()),
            float((np.abs(a - b)[big] / np.abs(b)[big]).max()))


def test_split_product_emulation_meets_the_network_bounds(monkeypatch):
    """conv4 (no average pool: every rounding reaches an output element - the worst case of the four variants), 2 frames of 64 x 64, every convolution
    replaced by the emulated split product: the bounds of test_gpu_f32s.py::test_whole_network_against_the_oracle."""
    from oracle import encoder_oracle as eo
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synth.resnet50_state_dict(6, 'conv4')
    fr = synth.smooth_frames(71, 2, 64, 64)
    ref = eo.embed(sd, fr, 'conv4', squeeze=False)
    with monkeypatch.context() as m:
        m.setattr(eo, '_conv_bn', split_conv_bn(eo))
        out = eo.embed(sd, fr, 'conv4', squeeze=False)
    l2, mx, rel = parity_figures(out, ref)
    print('\n[f32s emulation, conv4] rel-L2 %.2e max-norm %.2e max element-wise relative error (elements > 1 %% of the maximum) %.2e' % (l2, mx, rel))
    assert out.shape == (2, 2058) and not np.array_equal(out, ref)
    assert l2 < 1e-4 and mx < 1e-4 and rel < 1e-3, (l2, mx, rel)
