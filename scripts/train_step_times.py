"""Per-launch times of one training step (forward + backward, batch 32) of the trainable resnet18 and resnet50 encoders
(EmbeddingNet(..., train=True), include/pvr_train.h) -> profiles/train_step_times.txt.

The trainer brackets every launch with events (pvr_trainer_debug_set_timing), so the times carry a few microseconds of dispatch each; the step
total is also measured without them.  For the weight-gradient launches the fp32-equivalent TFLOP/s (2 * pixels * cout * cin * k * k / time) are
reported, and the slowest launches are named.

    python scripts/train_step_times.py [--batch 32] [--out profiles/train_step_times.txt]

--wgrad_split16 compares the two weight-gradient arithmetics (pvr_trainer_set_wgrad_split16) instead: both modes in ONE process, each warmed up, the
per-launch events of --reps steps each (minimum / median / maximum show the spread), conv1's weight gradient and the sum of all others with the
mode's scale launches counted in, and the step totals -> profiles/wgrad_split16_times.txt.

    python scripts/train_step_times.py --wgrad_split16 [--batch 32] [--reps 5] [--out profiles/wgrad_split16_times.txt]

--conv_split16 does the same for the forward convolutions and the data gradients of layer1 .. layer4 (pvr_trainer_set_conv_split16): per convolution
the fp32 launches (forward: weight pack + convolution; data gradient: its one bracket of pack [+ grid] + convolution) against the split launches with
the scale launch that serves them (forward: "<conv> scale"; backward: "<conv> bwd scale", counted with the data gradient), their sums and the step
totals -> profiles/conv_split16_times.txt.  --names picks the trunks, --append adds to the file (batch 32, then the frozen-BatchNorm pass sizes).

    python scripts/train_step_times.py --conv_split16 [--batch 32] [--names resnet18,resnet50] [--reps 5] [--append]
"""
import argparse
import ctypes as C
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvr_habitat_amd import _lib, synth  # noqa: E402
from pvr_habitat_amd import embeddings as E  # noqa: E402


def launches(handle):
    L, out, i = _lib.lib(), [], 0
    name, ms, fl = C.create_string_buffer(128), C.c_float(), C.c_double()
    while L.pvr_trainer_launch_time(handle, i, name, 128, C.byref(ms), C.byref(fl)) > 0:
        out.append((name.value.decode(), ms.value, fl.value))
        i += 1
    return out


def one(name, batch, lines):
    net = E.EmbeddingNet(name, pretrained=False, train=True, max_batch=batch)
    m = net.embedding
    fr = torch.from_numpy(synth.smooth_frames(11, batch, 64, 64)).cuda()
    dout = torch.randn((batch, net.out_size), device='cuda') / batch

    def step():
        for p in m.parameters():
            p.grad = None
        (net(fr) * dout).sum().backward()
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        step()
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) / 3
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
    step()
    torch.cuda.synchronize()
    rows = launches(m._handle)
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 0))
    lines.append('== %s, batch %d: forward + backward %.2f ms per step without per-launch events (%.1f frames/s); %d launches, %.2f ms summed with events =='
                 % (name, batch, total, batch / total * 1e3, len(rows), sum(r[1] for r in rows)))
    groups = {}
    for n, ms, fl in rows:
        kind = n.split()[-1] if n.split()[-1] in ('wgrad', 'dgrad', 'pack', 'bwd') else ('bn' if ('bn' in n or 'downsample.1' in n) else 'conv / other')
        if kind == 'bwd':
            kind = 'bn bwd' if 'pool' not in n else 'pool bwd'
        g = groups.setdefault(kind, [0.0, 0.0, 0])
        g[0] += ms; g[1] += fl; g[2] += 1
    lines.append('%-14s %8s %10s %s' % ('group', 'launches', 'ms', 'fp32-equivalent TFLOP/s'))
    for k, (ms, fl, cnt) in sorted(groups.items(), key=lambda kv: -kv[1][0]):
        lines.append('%-14s %8d %10.3f %s' % (k, cnt, ms, '%.2f' % (fl / ms / 1e9) if fl else '-'))
    lines.append('slowest launches:')
    for n, ms, fl in sorted(rows, key=lambda r: -r[1])[:12]:
        lines.append('  %-40s %8.3f ms %s' % (n, ms, '%7.2f TFLOP/s' % (fl / ms / 1e9) if fl else ''))
    lines.append('weight-gradient launches:')
    for n, ms, fl in rows:
        if n.endswith('wgrad'):
            lines.append('  %-40s %8.3f ms %7.2f TFLOP/s' % (n, ms, fl / ms / 1e9))
    lines.append('')


def measure_mode(name, batch, split16, reps, conv16=False):
    """-> (ms per step without per-launch events, [launch rows of each of `reps` steps]) of one arithmetic"""
    net = E.EmbeddingNet(name, pretrained=False, train=True, max_batch=batch, **({'wgrad_split16': True} if split16 else {}),
                         **({'conv_split16': True} if conv16 else {}))
    m = net.embedding
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(batch, device='cuda') % 64].contiguous()
    dout = torch.randn((batch, net.out_size), device='cuda', generator=torch.Generator('cuda').manual_seed(3)) / batch

    def step():
        for p in m.parameters():
            p.grad = None
        (net(fr) * dout).sum().backward()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        step()
    e1.record()
    torch.cuda.synchronize()
    total = e0.elapsed_time(e1) / 5
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
    step()                                            # (the events of a step are made on first use)
    runs = []
    for _ in range(reps):
        step()
        torch.cuda.synchronize()
        runs.append(launches(m._handle))
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 0))
    net.close()
    del step, m, net                                  # (the workspace goes with the module: the next mode's fits next to nothing)
    gc.collect()
    return total, runs


def _stat(values):
    v = sorted(values)
    return v[0], v[len(v) // 2], v[-1]


def compare(name, batch, reps, lines):
    """weight-gradient launches of both modes: per convolution the fp32 launch against the split launch plus its scale launches"""
    t_off, off = measure_mode(name, batch, False, reps)
    t_on, on = measure_mode(name, batch, True, reps)
    def per_conv(runs):                               # conv -> [ms of each rep]: the wgrad launch and the scale launches that belong to it
        out = {}
        for i, rows in enumerate(runs):
            for n, ms, fl in rows:
                w = n.split()
                if w[-1] == 'wgrad' or w[-1] == 'scale':
                    e = out.setdefault(w[0], dict(wgrad=[0.0] * len(runs), scale=[0.0] * len(runs), flops=0.0))
                    e['wgrad' if w[-1] == 'wgrad' else 'scale'][i] += ms
                    e['flops'] = max(e['flops'], fl)
        return out
    a, b = per_conv(off), per_conv(on)
    assert list(a) == list(b)
    lines.append('== %s, batch %d, %d timed steps per mode after a warm-up; ms as minimum / median / maximum ==' % (name, batch, reps))
    lines.append('forward + backward per step without per-launch events: fp32 weight gradients %.2f ms, split-f16 %.2f ms (%.2fx)' % (t_off, t_on, t_off / t_on))
    c_off = _stat(a['conv1']['wgrad'])
    c_on = _stat([w + s for w, s in zip(b['conv1']['wgrad'], b['conv1']['scale'])])
    lines.append('conv1 weight gradient: fp32 (stem_wgrad) %.3f / %.3f / %.3f ms; split-f16 with its two scale launches %.3f / %.3f / %.3f ms (of which scales %.3f); '
                 'median ratio %.1fx' % (c_off + c_on + (_stat(b['conv1']['scale'])[1], c_off[1] / c_on[1])))
    others = [k for k in a if k != 'conv1']
    s_off = _stat([sum(a[k]['wgrad'][i] for k in others) for i in range(reps)])
    s_on = _stat([sum(b[k]['wgrad'][i] + b[k]['scale'][i] for k in others) for i in range(reps)])
    s_sc = _stat([sum(b[k]['scale'][i] for k in others) for i in range(reps)])
    lines.append('all other weight gradients, summed (%d convolutions): fp32 %.3f / %.3f / %.3f ms; split-f16 with scale launches %.3f / %.3f / %.3f ms (of which '
                 'scales %.3f); median ratio %.2fx' % ((len(others),) + s_off + s_on + (s_sc[1], s_off[1] / s_on[1])))
    lines.append('%-28s %10s %12s %10s %10s %8s' % ('convolution (median ms)', 'fp32', 'fp32 TFLOP/s', 'split-f16', '+ scales', 'ratio'))
    lost = []
    for k in a:
        o, w, sc = _stat(a[k]['wgrad'])[1], _stat(b[k]['wgrad'])[1], _stat(b[k]['scale'])[1]
        lines.append('%-28s %10.3f %12.2f %10.3f %10.3f %7.2fx' % (k, o, a[k]['flops'] / o / 1e9, w, sc, o / (w + sc)))
        if w + sc > o:
            lost.append(k)
    lines.append('shapes at which the split launch with its scales is slower than the fp32 launch: %s' % (', '.join(lost) if lost else 'none'))
    lines.append('')


def compare_conv(name, batch, reps, lines):
    """forward convolutions and data gradients of layer1 .. layer4 in both modes, the scale and pack launches counted with the launch they serve"""
    t_off, off = measure_mode(name, batch, False, reps)
    t_on, on = measure_mode(name, batch, False, reps, conv16=True)

    def per_conv(runs, split):                        # conv -> {'fwd': [ms per rep], 'dgrad': [...], 'scale': [...]} (scale: part of the two sums)
        out = {}
        for i, rows in enumerate(runs):
            for n, ms, fl in rows:
                w = n.split()
                if not w[0].startswith('layer') or 'bn' in w[0] or w[0].endswith('downsample.1') or w[-1] in ('wgrad', 'bwd'):
                    continue
                tail = ' '.join(w[1:])
                part = {'': 'fwd', 'pack': 'fwd', 'split16': 'fwd', 'scale': 'fwd', 'dgrad': 'dgrad', 'dgrad split16': 'dgrad', 'bwd scale': 'dgrad'}[tail]
                e = out.setdefault(w[0], dict(fwd=[0.0] * len(runs), dgrad=[0.0] * len(runs), scale=[0.0] * len(runs), flops=0.0))
                e[part][i] += ms
                if tail.endswith('scale'):
                    e['scale'][i] += ms
                e['flops'] = max(e['flops'], fl)
        return out
    a, b = per_conv(off, False), per_conv(on, True)
    assert list(a) == list(b) and len(a) > 10
    lines.append('== %s, batch %d, %d timed steps per mode after a warm-up; ms as minimum / median / maximum ==' % (name, batch, reps))
    lines.append('forward + backward per step without per-launch events: fp32 %.2f ms, split-f16 convolutions and data gradients %.2f ms (%.2fx)'
                 % (t_off, t_on, t_off / t_on))
    sums = {}
    for part, what in (('fwd', 'forward convolutions'), ('dgrad', 'data gradients')):
        s_off = _stat([sum(a[k][part][i] for k in a) for i in range(reps)])
        s_on = _stat([sum(b[k][part][i] for k in b) for i in range(reps)])
        sums[part] = (s_off, s_on)
        lines.append('%s, summed (%d convolutions): fp32 %.3f / %.3f / %.3f ms; split-f16 with scale and pack launches %.3f / %.3f / %.3f ms; median ratio %.2fx'
                     % ((what, len(a)) + s_off + s_on + (s_off[1] / s_on[1],)))
    both_off = _stat([sum(a[k]['fwd'][i] + a[k]['dgrad'][i] for k in a) for i in range(reps)])
    both_on = _stat([sum(b[k]['fwd'][i] + b[k]['dgrad'][i] for k in b) for i in range(reps)])
    s_sc = _stat([sum(b[k]['scale'][i] for k in b) for i in range(reps)])
    gain, spreads = both_off[1] - both_on[1], (both_off[2] - both_off[0]) + (both_on[2] - both_on[0])
    lines.append('both, summed: fp32 %.3f / %.3f / %.3f ms; split-f16 %.3f / %.3f / %.3f ms (of which scale launches %.3f); median ratio %.2fx'
                 % (both_off + both_on + (s_sc[1], both_off[1] / both_on[1])))
    lines.append('criterion (the split median below the fp32 median by more than the two spreads): fp32 - split %.3f ms, spreads %.3f ms: %s'
                 % (gain, spreads, 'MET' if gain > spreads else 'NOT MET'))
    lines.append('%-26s %9s %9s %9s %7s   %9s %9s %9s %7s' % ('convolution (median ms)', 'fwd fp32', 'TFLOP/s', 'fwd split', 'ratio', 'dgr fp32', 'TFLOP/s',
                                                             'dgr split', 'ratio'))
    lost = []
    for k in a:
        fo, fs, do, ds = (_stat(d[k][p])[1] for d, p in ((a, 'fwd'), (b, 'fwd'), (a, 'dgrad'), (b, 'dgrad')))
        lines.append('%-26s %9.3f %9.2f %9.3f %6.2fx   %9.3f %9.2f %9.3f %6.2fx' % (k, fo, a[k]['flops'] / fo / 1e9, fs, fo / fs, do, a[k]['flops'] / do / 1e9, ds,
                                                                                  do / ds))
        if fs > fo or ds > do:
            lost.append(k)
    lines.append('shapes at which a split launch with its scale and pack launches is slower than the fp32 launches: %s' % (', '.join(lost) if lost else 'none'))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wgrad_split16', action='store_true', help='compare the fp32 and the split-f16 weight gradients (both modes in this process)')
    ap.add_argument('--conv_split16', action='store_true', help='compare the fp32 and the split-f16 forward convolutions and data gradients')
    ap.add_argument('--names', default='resnet18,resnet50', help='with --conv_split16: the trunks to measure')
    ap.add_argument('--append', action='store_true', help='with --conv_split16: append to --out')
    ap.add_argument('--reps', type=int, default=5, help='with --wgrad_split16 / --conv_split16: timed steps per mode')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'conv_split16_times.txt' if a.conv_split16 else 'wgrad_split16_times.txt' if a.wgrad_split16
                             else 'train_step_times.txt')
    if a.conv_split16:
        lines = ['forward-convolution and data-gradient launches of one training step, fp32 (f32-input MFMA) against split-f16 (pvr_trainer_set_conv_split16), '
                 'per-launch events (scripts/train_step_times.py --conv_split16), %s' % torch.cuda.get_device_name(0), '']
        for name in a.names.split(','):
            compare_conv(name, a.batch, a.reps, lines)
    elif a.wgrad_split16:
        lines = ['weight-gradient launches of one training step, fp32 (f32-input MFMA) against split-f16 (pvr_trainer_set_wgrad_split16), per-launch events '
                 '(scripts/train_step_times.py --wgrad_split16), %s' % torch.cuda.get_device_name(0), '']
        for name in ('resnet18', 'resnet50'):
            compare(name, a.batch, a.reps, lines)
    else:
        lines = ['per-launch times of one training step of the trainable encoders (scripts/train_step_times.py), %s' % torch.cuda.get_device_name(0), '']
        for name in ('resnet18', 'resnet50'):
            one(name, a.batch, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a' if a.conv_split16 and a.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
