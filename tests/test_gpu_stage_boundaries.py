"""Stage boundary layer1 -> layer2 (PVR_STRIDED_Y): layer1's last tail stores its output y only at the (even row, even column) pixels that
layer2.0's stride-2 downsample reads, compacted to (n, 28, 28, 256), and that downsample runs at stride 1 over them.  A storage property of
plain forwards: the embeddings, the downsample's output and (under a debug stop) the full layer1 output are bit-identical to the switch-off
plan.  Forwards with a tap, a '#k' stop or a range check keep the full store."""
import pytest
import torch

from pvr_habitat_amd import synth

gpu = pytest.mark.gpu
pytestmark = [gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

B_DS = 4                      # workspace buffer of the downsample outputs (encoder_internal.h: BufId)


def _pair(monkeypatch, dtype, max_batch, sd):
    """(switch on, switch off) handles of the same weights; the switch is read when the handle is created"""
    from pvr_habitat_amd.embeddings import HipResNet50
    ms = []
    for v in ('1', '0'):
        monkeypatch.setenv('PVR_STRIDED_Y', v)
        m = HipResNet50(sd, 'conv5', compute_dtype=dtype, max_batch=max_batch)
        m.kernel_names()      # (builds the handle while the variable is set)
        ms.append(m)
    monkeypatch.delenv('PVR_STRIDED_Y')
    return ms


def _compact(n):
    """a batch of n frames takes the compact form: layer2.0's downsample is conv_expand at both strides (>= 512 tiles of 64 pixels)"""
    return (n * 28 * 28 + 63) // 64 >= 512


@pytest.mark.parametrize('dtype,n', [('f16', 256), ('bf16', 256), ('f16', 1), ('bf16', 3), ('f16', 41), ('f16', 43), ('bf16', 42)])
def test_strided_y_embeddings_bit_identical(dtype, n, monkeypatch):
    sd = synth.resnet50_state_dict(3, 'conv5')
    on, off = _pair(monkeypatch, dtype, max(8, n), sd)
    kn_on, kn_off = on.kernel_names(n), off.kernel_names(n)
    assert len(kn_on) == len(kn_off) == len(on.op_names()) and on.op_names() == off.op_names()
    assert 'conv_expand(y_s2)' not in kn_off
    if _compact(n):
        k = on.op_names().index('layer2.0.downsample.0')
        assert kn_on[k] == 'conv_expand(y_s2)' and kn_on.count('conv_expand(y_s2)') == 1, kn_on
        assert kn_on[k - 1] == 'chain_wave' and on.op_names()[k - 1] == 'layer1.2.conv2+conv3+layer2.0.conv1'
        assert [a for a in kn_on if a != 'conv_expand(y_s2)'] == [b for i, b in enumerate(kn_off) if i != k]
    else:
        assert kn_on == kn_off
    fr = torch.from_numpy(synth.frames(40 + n, n, 256, 256)).cuda()
    a, b = on(fr), off(fr)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    on.close(); off.close()


def test_strided_y_plan_at_the_bench_batch(monkeypatch):
    sd = synth.resnet50_state_dict(1, 'conv5')
    on, off = _pair(monkeypatch, 'f16', 256, sd)
    kn = on.kernel_names(256)
    print('\n[PVR_STRIDED_Y=1, batch 256]', list(zip(on.op_names(), kn))[:12])
    assert kn.count('chain_wave') == 3 and kn.count('bottleneck_chain') == 4 and kn.count('conv_expand(y_s2)') == 1
    assert kn[on.op_names().index('layer2.0.downsample.0')] == 'conv_expand(y_s2)'
    assert 'conv_expand(y_s2)' not in off.kernel_names(256)
    on.close(); off.close()


@pytest.mark.parametrize('dtype,n', [('f16', 64), ('bf16', 43)])
def test_strided_y_full_layer1_and_downsample(dtype, n, monkeypatch):
    """the layer1 tap under a debug stop is the full y; the downsample output of a plain forward (its buffer is not written again when layer3.0 /
    layer4.0 run their downsample inside the two-operand launch) equals the switch-off one and that of a '#k' stop on either handle"""
    sd = synth.resnet50_state_dict(5, 'conv5')
    on, off = _pair(monkeypatch, dtype, n, sd)
    assert _compact(n) and 'conv_expand(y_s2)' in on.kernel_names(n)
    fr = torch.from_numpy(synth.frames(90 + n, n, 256, 256)).cuda()
    n_y, n_ds = n * 56 * 56 * 256, n * 28 * 28 * 512
    ds = {}
    for key, m in (('on', on), ('off', off)):
        m(fr)
        ds[key] = m.tap('buf%d:%d' % (B_DS, n_ds), n_ds).clone()
    assert torch.equal(ds['on'], ds['off'])
    k = on.op_names().index('layer2.0.downsample.0')
    y1 = {}
    for key, m in (('on', on), ('off', off)):
        m.debug_stop_after('#%d' % k)
        m(fr)
        assert torch.equal(m.tap('buf%d:%d' % (B_DS, n_ds), n_ds), ds['on']), key
        m.debug_stop_after('layer1')
        m(fr)
        y1[key] = m.tap('layer1', n_y).clone()
        m.debug_stop_after('')
    assert torch.equal(y1['on'], y1['off'])
    assert torch.isfinite(y1['on']).all() and y1['on'].abs().sum() > 0
    assert torch.equal(on(fr), off(fr))                  # (plain forwards again after the stops)
    on.close(); off.close()


def test_strided_y_two_lanes(monkeypatch):
    sd = synth.resnet50_state_dict(2, 'conv5')
    on, off = _pair(monkeypatch, 'f16', 128, sd)
    fa = torch.from_numpy(synth.frames(61, 128, 256, 256)).cuda()
    fb = torch.from_numpy(synth.frames(62, 96, 256, 256)).cuda()
    torch.cuda.synchronize()
    got = {}
    for key, m in (('on', on), ('off', off)):
        oa = torch.empty((128, m.out_size), device='cuda')
        ob = torch.empty((96, m.out_size), device='cuda')
        s1 = torch.cuda.Stream()
        m.forward_into(fa, oa, lane=0)
        with torch.cuda.stream(s1):
            m.forward_into(fb, ob, lane=1)
        torch.cuda.synchronize()
        got[key] = (oa, ob)
    assert torch.equal(got['on'][0], got['off'][0]) and torch.equal(got['on'][1], got['off'][1])
    on.close(); off.close()
