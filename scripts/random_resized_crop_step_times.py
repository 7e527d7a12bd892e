"""The random_resized_crop mode (pvr_trainer_forward_rects; EmbeddingNet(..., train=True, random_resized_crop=(lo, hi))) ->
profiles/random_resized_crop_step_times.txt.  Reference: the same build's paths without the mode in the same process.  Per trunk (resnet18 in passes of
640 frames, resnet50 in passes of 320), B = 16, two 64 x 64 frames per observation, frozen BatchNorm, BatchNorm1d on - the conditions of
scripts/random_crop_step_times.py:

  1. the fused step (models.HipJointRMSprop) at T = 100 x B = 16 x 2 = 3200 frames with the mode off, on, and on together with color_jitter: three
     models in one process, a warm-up step each, then --steps timed steps each, ALTERNATING so that all see the same neighbours; min, median and max
     per mode.  A mode's step counts as slower when its median exceeds the off median by more than the off runs' min - max spread;
  2. the launch "preprocess rects" against "preprocess windows" (the random_crop mode), and the pair "colour stats" + "preprocess colour" with the
     rectangle and with the window as the pixel source, at the pass size, all in that same process (pvr_trainer_debug_set_timing: an event pair around
     every launch): min, median and max of --steps forwards each.  "preprocess rects" counts as slower than "preprocess windows" when its median
     exceeds that launch's by more than that launch's own min - max spread.

    python scripts/random_resized_crop_step_times.py [--steps 5] [--T 100] [--only resnet18] [--scale 0.2 1] [--out profiles/...txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvr_habitat_amd import _lib, synth  # noqa: E402
from pvr_habitat_amd import embeddings as E  # noqa: E402
from pvr_habitat_amd import models as M  # noqa: E402

B, F_ = 16, 2
STRENGTHS = (0.4, 0.4, 0.4)


def batch(T):
    n = T * B * F_
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()
    obs = fr[torch.arange(n, device='cuda') % 64].view(T, B, F_, 64, 64, 3).permute(0, 1, 3, 4, 2, 5).reshape(T, B, 64, 64, 3 * F_)
    return obs.contiguous(), torch.zeros((T, B), dtype=torch.bool, device='cuda'), torch.randint(0, 3, (T, B), device='cuda')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ms, digits=2):
    return ('%%.%df / %%.%df / %%.%df' % ((digits,) * 3)) % (min(ms), statistics.median(ms), max(ms))


def stepper(name, T, chunk, modes):
    net = E.EmbeddingNet(name, pretrained=False, train=True, freeze_bn=True, max_batch=chunk, **modes)
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    obs, done, act = batch(T)

    def one():
        opt.scheduler_step()
        opt.step(obs, done, act)
    return one, model


def step_table(name, T, chunk, steps, scale, lines):
    n = T * B * F_
    modes = (('off', {}), ('on', {'random_resized_crop': scale, 'crop_seed': 1}),
             ('on + colour', {'random_resized_crop': scale, 'crop_seed': 1, 'color_jitter': STRENGTHS, 'color_seed': 1}))
    runs = [(how,) + stepper(name, T, chunk, kw) for how, kw in modes]
    for _, one, _ in runs:
        one()                                                  # warm-up: allocates the workspaces
    torch.cuda.synchronize()
    ms = {how: [] for how, _ in modes}
    for _ in range(steps):
        for how, one, _ in runs:
            ms[how].append(timed(one))
    passes = len(runs[0][2].embedding._passes(n))
    room = max(ms['off']) - min(ms['off'])
    cells = []
    for how, _ in modes[1:]:
        d = statistics.median(ms[how]) - statistics.median(ms['off'])
        cells.append('%s: %s  (%+.2f, %s)' % (how, spread(ms[how]), d, 'slower' if d > room else 'not slower'))
    lines.append('%-9s %5d  %6d  off: %s  (spread %.2f)   %s' % (name, chunk, passes, spread(ms['off']), room, '   '.join(cells)))
    for _, _, model in runs:
        model.close()
    del runs
    torch.cuda.empty_cache()


def launches(handle):
    L, out, i = _lib.lib(), {}, 0
    name, ms = C.create_string_buffer(128), C.c_float()
    while L.pvr_trainer_launch_time(handle, i, name, 128, C.byref(ms), None) > 0:
        out[name.value.decode()] = ms.value
        i += 1
    return out


IMAGE = ('preprocess', 'normalize', 'preprocess windows', 'preprocess rects', 'colour stats', 'preprocess colour')


def launch_table(name, chunk, steps, scale, lines):
    sd, variant = E._load_named_state_dict(name, False)
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(chunk, device='cuda') % 64].contiguous()
    kinds = (('windows', {'random_crop': True}), ('rects', {'random_resized_crop': scale}), ('windows + colour', {'color_jitter': STRENGTHS}),
             ('rects + colour', {'random_resized_crop': scale, 'color_jitter': STRENGTHS}))
    models = []
    for how, kw in kinds:
        m = E.HipTrainableResNet(sd, variant, max_batch=chunk, freeze_bn=True, **kw)
        m.train()
        m._forward_raw(fr)                                     # warm-up
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        models.append((how, m))
    rows = {how: [] for how, _ in kinds}
    for _ in range(steps):                                     # the four sources alternate
        for how, m in models:
            m._forward_raw(fr)
            torch.cuda.synchronize()
            rows[how].append({k: v for k, v in launches(m._handle).items() if k in IMAGE})
    assert sorted(rows['windows'][0]) == ['preprocess windows'] and sorted(rows['rects'][0]) == ['preprocess rects'], rows
    assert sorted(rows['windows + colour'][0]) == sorted(rows['rects + colour'][0]) == ['colour stats', 'preprocess colour'], rows
    col = lambda how, k: [r[k] for r in rows[how]]
    win, rect = col('windows', 'preprocess windows'), col('rects', 'preprocess rects')
    d, room = statistics.median(rect) - statistics.median(win), max(win) - min(win)
    lines.append('%-9s %5d  preprocess windows %s   preprocess rects %s   (%+.3f, spread of windows %.3f: %s)'
                 % (name, chunk, spread(win, 3), spread(rect, 3), d, room, 'slower' if d > room else 'not slower'))
    for k in ('colour stats', 'preprocess colour'):
        lines.append('%-9s %5d  %-17s from windows %s   from rects %s' % ('', chunk, k, spread(col('windows + colour', k), 3), spread(col('rects + colour', k), 3)))
    del models
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--scale', type=float, nargs=2, default=(0.2, 1.0))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'random_resized_crop_step_times.txt'))
    a = ap.parse_args()
    scale = tuple(a.scale)
    trunks = [(nm, ch) for nm, ch in (('resnet18', 640), ('resnet50', 320)) if a.only in (None, nm)]
    lines = ['the random_resized_crop mode (scripts/random_resized_crop_step_times.py), %s; one process, frozen BatchNorm, eager launches, BatchNorm1d on, '
             '64x64 frames, scale %g %g, colour strengths %g %g %g; a warm-up, then %d timed steps per figure, the modes alternating; every figure is '
             'min / median / max in ms' % ((torch.cuda.get_device_name(0),) + scale + STRENGTHS + (a.steps,)), '',
             '-- the fused step, T %d x B %d x %d frames = %d frames per step: the mode off, on, and on with color_jitter --' % (a.T, B, F_, a.T * B * F_),
             'trunk     chunk  passes']
    for nm, ch in trunks:
        step_table(nm, a.T, ch, a.steps, scale, lines)
    lines += ['(in brackets: median minus the off median; slower: the difference exceeds the spread, max - min, of the off runs)', '',
              '-- the image launches of one pass (per-launch events, %d forwards each, the sources alternating) --' % a.steps,
              '(per output pixel both sources read four uint8 taps of three channels and the image launches write 16 B; colour stats includes the memset of '
              'the gray sums)']
    for nm, ch in trunks:
        launch_table(nm, ch, a.steps, scale, lines)
    lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
