"""Per-launch times of one training step (forward + backward, batch 32) of the trainable resnet18 and resnet50 encoders
(EmbeddingNet(..., train=True), include/pvr_train.h) -> profiles/train_step_times.txt.

The trainer brackets every launch with events (pvr_trainer_debug_set_timing), so the times carry a few microseconds of dispatch each; the step
total is also measured without them.  For the weight-gradient launches the fp32-equivalent TFLOP/s (2 * pixels * cout * cin * k * k / time) are
reported, and the slowest launches are named.

    python scripts/train_step_times.py [--batch 32] [--out profiles/train_step_times.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_step_times.txt'))
    a = ap.parse_args()
    lines = ['per-launch times of one training step of the trainable encoders (scripts/train_step_times.py), %s' % torch.cuda.get_device_name(0), '']
    for name in ('resnet18', 'resnet50'):
        one(name, a.batch, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
