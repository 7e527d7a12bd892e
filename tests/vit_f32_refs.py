"""float64 references, derived bounds and inputs for the fp32 ViT plan (compute_dtype='f32' of the CLIP / MAE encoders) - shared by
tests/test_vit_f32_cpu.py and tests/test_gpu_vit_f32.py, CPU only.  Nothing here is measured on the code under test: the attention bound follows from
fp32 arithmetic (u32 = 2^-24), the whole-network yardsticks are the fp32 oracle and a float64 run of the same oracle code."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_kernel_refs as kr
from oracle import vit_oracle as vo
from pvr_habitat_amd import synth

U32 = 2.0 ** -24

# (T, heads, head dim): one token; 17 (a second, ragged key tile); CLIP B/32's 50; 64 / 65 (a full workgroup of queries, and one query more);
# the /16 plans' 197; MAE H/14's 257 at head dim 80; 288 (the most keys built, every tile full); head dim 80 with few keys
ATT_SHAPES = [(1, 1, 64), (17, 12, 64), (50, 12, 64), (64, 2, 64), (65, 1, 64), (197, 12, 64), (257, 2, 80), (288, 2, 80), (50, 2, 80)]
ATT_NB = 3


def attention_inputs_f32(family, T, heads, hd, nb=ATT_NB):
    """(nb, T, 3W) fp32: the bf16 input families of oracle/vit_kernel_refs.py plus noise of 2^-12, which populates the low bits of the significand
    (an operand rounded to 16 bits anywhere changes the values)"""
    base = kr.attention_inputs(family, T, heads, hd, nb, 'bf16').float()
    noise = synth.normal(23, 'att32_%s_%d_%d_%d_%d' % (family, T, heads, hd, nb), tuple(base.shape)).astype(np.float32)
    return (base + 2.0 ** -12 * torch.from_numpy(noise)).contiguous()


def attention_ref_f32(qkv, heads):
    """qkv: (nb, T, 3W) fp32.  Returns (ref, bound), float64 (nb, T, W), every step in float64.

    Bound per element:  (2 D_q + (T + 8) u32) sum_k p_k |v_k|,   D_q = max_k u32 ((HD + 2) (|q| . |k|) / sqrt(HD) + 4 |s_k|).
    D_q bounds the absolute error of a scaled score of query q: HD products accumulated in fp32 ((HD + 2) u32 of sum |q_d k_d|, scale included), and a few
    roundings proportional to the score itself (the scale multiply, the max subtraction, exp2's argument and result).  An absolute score error D moves
    every p_k by a relative e^D - 1 ~ D, and the normaliser by at most as much: 2 D_q.  (T + 8) u32: the fp32 accumulation of T products in P V, the
    normaliser's sum, the division and the final multiply."""
    q, k, v, hd = kr._split_heads(qkv.double(), heads)
    T = qkv.shape[1]
    s = q @ k.transpose(-1, -2) / np.sqrt(hd)
    p = torch.softmax(s, dim=-1)
    ref = p @ v
    spv = p @ v.abs()
    qk = q.abs() @ k.abs().transpose(-1, -2) / np.sqrt(hd)
    dq = (U32 * ((hd + 2) * qk + 4.0 * s.abs())).amax(dim=-1, keepdim=True)
    bound = (2.0 * dq + (T + 8) * U32) * spv
    back = lambda t: t.permute(0, 2, 1, 3).reshape(qkv.shape[0], T, -1)
    return back(ref), back(bound)


ATT_MUTANTS = ('p_f16', 'qkv_f16')


def attention_emulate_f32(qkv, heads, mutant=None):
    """fp32 attention in torch on the CPU; mutant 'p_f16': the probabilities rounded to f16 before P V, 'qkv_f16': q, k and v rounded to f16"""
    assert mutant is None or mutant in ATT_MUTANTS
    x = qkv.half().float() if mutant == 'qkv_f16' else qkv.float()
    q, k, v, hd = kr._split_heads(x, heads)
    p = torch.softmax(q @ k.transpose(-1, -2) / np.float32(np.sqrt(hd)), dim=-1)
    if mutant == 'p_f16':
        p = p.half().float()
    o = p @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], -1)


# ------------------------------------------------------------------------------------------------------------------
# whole networks: the fp32 oracle and the same code in float64
# ------------------------------------------------------------------------------------------------------------------
NET_CASES = {                       # variant: (state dict, frames, heads, mae)
    'clip_b32': (lambda: synth.clip_vit_state_dict(1, patch=32), lambda: synth.smooth_frames(41, 3, 224, 224), 12, False),
    'clip_b16': (lambda: synth.clip_vit_state_dict(1, patch=16), lambda: synth.smooth_frames(41, 2, 224, 224), 12, False),
    'mae_b16': (lambda: synth.mae_vit_state_dict(1), lambda: synth.smooth_frames(47, 2, 64, 64), 12, True),
    'mae_l16': (lambda: synth.mae_vit_state_dict(2, width=1024, layers=24), lambda: synth.smooth_frames(48, 1, 256, 256), 16, True),
}


def _ln64(x, w, b):
    return F.layer_norm(x.double(), (x.shape[-1],), vo._t(w).double(), vo._t(b).double(), 1e-5)


def oracle_pair(sd, frames, heads, mae, taps=None):
    """(fp32 oracle, float64 restatement) of the embedding of `frames`, both from the oracle's own fp32 preprocessed image: the same code, the second
    time with a float64 state dict and float64 activations (encode_image's LayerNorm is the one place the oracle casts, so it is replaced)"""
    with torch.no_grad():
        x = (vo.mae_preprocess if mae else vo.preprocess)(frames)
        sd64 = {k: vo._t(v).double() for k, v in sd.items()}
        if mae:
            ref = vo.mae_encode(sd, x, heads=heads, taps=taps)
            ref64 = vo.mae_encode(sd64, x.double(), heads=heads)
        else:
            ref = vo.encode_image(sd, x, heads=heads, taps=taps)
            keep = vo._ln
            vo._ln = _ln64
            try:
                ref64 = vo.encode_image(sd64, x.double(), heads=heads)
            finally:
                vo._ln = keep
    assert ref.dtype == torch.float32 and ref64.dtype == torch.float64
    return ref.numpy(), ref64.numpy()


def parity_figures(out, ref):
    """(rel-L2, max-norm, the MAXIMUM relative error over every element above 1 % of the reference's largest magnitude - none left out)"""
    a, b = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    big = np.abs(b) > 0.01 * np.abs(b).max()
    assert big.any()
    return (float(np.linalg.norm(a - b) / np.linalg.norm(b)), float(np.abs(a - b).max() / np.abs(b).max()),
            float((np.abs(a - b)[big] / np.abs(b)[big]).max()))
