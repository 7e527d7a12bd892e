"""The gaussian_blur and random_grayscale modes (pvr_trainer_forward_staged; EmbeddingNet(..., train=True, gaussian_blur=(p, lo, hi),
random_grayscale=p)) -> profiles/gaussian_blur_step_times.txt.  Reference: the same build's centre-crop path in the same process.  Per trunk (resnet18
in passes of 640 frames, resnet50 in passes of 320), B = 16, two 64 x 64 frames per observation, frozen BatchNorm, BatchNorm1d on - the conditions of
scripts/color_jitter_step_times.py:

  1. the fused step (models.HipJointRMSprop) at T = 100 x B = 16 x 2 = 3200 frames with the modes off and on (MoCo v2's 0.5 0.1 2.0 and 0.2): two models
     in one process, a warm-up step each, then --steps timed steps each, ALTERNATING off and on so that both see the same neighbours; min, median and
     max per mode, next to the spread of the off runs.  No threshold is fixed: the figures are recorded;
  2. the launches "stage image" and "blur normalize" at the pass size in that same process (pvr_trainer_debug_set_timing: an event pair around every
     launch), median of --steps forwards each, with no frame blurred and every frame grayed (the branch without LDS), with MoCo v2's probabilities and
     with every frame blurred (p = 1, sigma 2), next to "blur normalize"'s byte floor - the staged bytes read (4 per pixel) plus the image bytes
     written (16 per pixel) at 6.0 TB/s, the in-order HBM sweep rate of scripts/frozen_bn_step_times.py - and to "colour stats" + "preprocess colour"
     of the color_jitter mode for scale.

    python scripts/gaussian_blur_step_times.py [--steps 5] [--T 100] [--only resnet18] [--out profiles/gaussian_blur_step_times.txt]
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
MOCO = {'gaussian_blur': (0.5, 0.1, 2.0), 'random_grayscale': 0.2, 'blur_seed': 1}
SWEEP = 6.0e12                                                  # bytes per second


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


def spread(ms):
    return 'min %.2f, median %.2f, max %.2f' % (min(ms), statistics.median(ms), max(ms))


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


def step_table(name, T, chunk, steps, lines):
    n = T * B * F_
    off, m_off = stepper(name, T, chunk, {})
    on, m_on = stepper(name, T, chunk, MOCO)
    off(), on()                                                # warm-up: allocates the workspaces
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(steps):
        ms[False].append(timed(off))
        ms[True].append(timed(on))
    passes = len(m_off.embedding._passes(n))
    d = statistics.median(ms[True]) - statistics.median(ms[False])
    room = max(ms[False]) - min(ms[False])
    lines.append('%-9s %5d  %6d  off: %-46s on: %-46s %+8.2f  %6.2f' % (name, chunk, passes, spread(ms[False]), spread(ms[True]), d, room))
    m_off.close(), m_on.close()
    del off, on, m_off, m_on
    torch.cuda.empty_cache()


def launches(handle):
    L, out, i = _lib.lib(), {}, 0
    name, ms = C.create_string_buffer(128), C.c_float()
    while L.pvr_trainer_launch_time(handle, i, name, 128, C.byref(ms), None) > 0:
        out[name.value.decode()] = ms.value
        i += 1
    return out


IMAGE = ('preprocess', 'normalize', 'colour stats', 'preprocess colour', 'stage image', 'blur normalize')


def launch_table(name, chunk, steps, lines):
    sd, variant = E._load_named_state_dict(name, False)
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(chunk, device='cuda') % 64].contiguous()
    got = {}
    for mode, kw in (('centre', {}), ('colour', {'color_jitter': (0.4, 0.4, 0.4)}), ('moco', MOCO), ('gray', {'random_grayscale': 1.0}),
                     ('all', {'gaussian_blur': (1.0, 2.0, 2.0), 'random_grayscale': 0.2}),
                     ('all+colour', {'gaussian_blur': (1.0, 2.0, 2.0), 'random_grayscale': 0.2, 'color_jitter': (0.4, 0.4, 0.4)})):
        m = E.HipTrainableResNet(sd, variant, max_batch=chunk, freeze_bn=True, **kw)
        m.train()
        m._forward_raw(fr)                                     # warm-up
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        rows = []
        for _ in range(steps):
            m.crop_call = 1                                    # the same draw in every timed forward
            m._forward_raw(fr)
            torch.cuda.synchronize()
            rows.append(launches(m._handle))
        got[mode] = {k: statistics.median(r[k] for r in rows) for k in rows[0] if k in IMAGE}
        if 'random_grayscale' in kw:
            p = E.blur_params(m.blur_seed, 1, chunk, kw.get('gaussian_blur'), kw['random_grayscale'])
            got[mode]['blurred'] = float((p['sigma'] > 0).mean())
        del m
        torch.cuda.empty_cache()
    assert sorted(got['centre']) == ['normalize', 'preprocess'] and sorted(got['colour']) == ['colour stats', 'preprocess colour'], got
    assert sorted(got['moco']) == ['blur normalize', 'blurred', 'stage image'] and 'colour stats' in got['all+colour'], got
    px = chunk * 224 * 224
    floor = px * 20 / SWEEP * 1e3
    lines.append('%-9s %5d  preprocess %.3f + normalize %.3f ms   colour stats %.3f + preprocess colour %.3f ms   byte floor of blur normalize %.3f ms (%.2f GB)'
                 % (name, chunk, got['centre']['preprocess'], got['centre']['normalize'], got['colour']['colour stats'], got['colour']['preprocess colour'],
                    floor, px * 20 / 1e9))
    for mode in ('gray', 'moco', 'all', 'all+colour'):
        g = got[mode]
        lines.append('%-9s %5d  %-10s %3.0f %% of the frames blurred: %sstage image %.3f ms, blur normalize %.3f ms = %.1f x its byte floor'
                     % (name, chunk, mode, 100 * g['blurred'], ('colour stats %.3f ms, ' % g['colour stats']) if 'colour stats' in g else '',
                        g['stage image'], g['blur normalize'], g['blur normalize'] / floor))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gaussian_blur_step_times.txt'))
    a = ap.parse_args()
    trunks = [(nm, ch) for nm, ch in (('resnet18', 640), ('resnet50', 320)) if a.only in (None, nm)]
    lines = ['the gaussian_blur and random_grayscale modes (scripts/gaussian_blur_step_times.py), %s; one process, frozen BatchNorm, eager launches, '
             'BatchNorm1d on, 64x64 frames; a warm-up, then %d timed steps per figure, the two modes alternating' % (torch.cuda.get_device_name(0), a.steps), '',
             '-- the fused step, T %d x B %d x %d frames = %d frames per step: off, and on with gaussian_blur 0.5 0.1 2.0 + random_grayscale 0.2 (ms per step) --'
             % (a.T, B, F_, a.T * B * F_),
             'trunk     chunk  passes  %-51s %-50s on - off  spread' % ('off', 'on')]
    for nm, ch in trunks:
        step_table(nm, a.T, ch, a.steps, lines)
    lines += ['(on - off: difference of the medians; spread: max - min of the off runs)', '',
              '-- the image of one pass (ms, per-launch events, median of %d forwards) --' % a.steps,
              '(byte floor of blur normalize: 4 B staged read + 16 B image written per pixel at 6.0 TB/s; moco: gaussian_blur 0.5 0.1 2.0 + random_grayscale '
              '0.2; gray: random_grayscale 1 alone, the no-LDS branch; all: every frame blurred at sigma 2, random_grayscale 0.2; colour stats includes the memset of the gray sums)']
    for nm, ch in trunks:
        launch_table(nm, ch, a.steps, lines)
    lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
