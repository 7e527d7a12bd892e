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
"""
import argparse
import ctypes as C
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


def measure_mode(name, batch, split16, reps):
    """-> (ms per step without per-launch events, [launch rows of each of `reps` steps]) of one weight-gradient arithmetic"""
    net = E.EmbeddingNet(name, pretrained=False, train=True, max_batch=batch, **({'wgrad_split16': True} if split16 else {}))
    m = net.embedding
    fr = torch.from_numpy(synth.smooth_frames(11, batch, 64, 64)).cuda()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wgrad_split16', action='store_true', help='compare the fp32 and the split-f16 weight gradients (both modes in this process)')
    ap.add_argument('--reps', type=int, default=5, help='with --wgrad_split16: timed steps per mode')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'wgrad_split16_times.txt' if a.wgrad_split16 else 'train_step_times.txt')
    if a.wgrad_split16:
        lines = ['weight-gradient launches of one training step, fp32 (f32-input MFMA) against split-f16 (pvr_trainer_set_wgrad_split16), per-launch events '
                 '(scripts/train_step_times.py --wgrad_split16), %s' % torch.cuda.get_device_name(0), '']
        for name in ('resnet18', 'resnet50'):
            compare(name, a.batch, a.reps, lines)
    else:
        lines = ['per-launch times of one training step of the trainable encoders (scripts/train_step_times.py), %s' % torch.cuda.get_device_name(0), '']
        for name in ('resnet18', 'resnet50'):
            one(name, a.batch, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
