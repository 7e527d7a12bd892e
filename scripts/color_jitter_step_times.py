"""The color_jitter mode (pvr_trainer_forward_augmented; EmbeddingNet(..., train=True, color_jitter=(b, c, s))) -> profiles/color_jitter_step_times.txt.
Reference: the same build's centre-crop path in the same process.  Per trunk (resnet18 in passes of 640 frames, resnet50 in passes of 320), B = 16,
two 64 x 64 frames per observation, frozen BatchNorm, BatchNorm1d on - the conditions of scripts/random_crop_step_times.py:

  1. the fused step (models.HipJointRMSprop) at T = 100 x B = 16 x 2 = 3200 frames with the mode off and on: two models in one process, a warm-up
     step each, then --steps timed steps each, ALTERNATING off and on so that both see the same neighbours; median, min and max per mode.  The
     mode's step counts as slower when its median exceeds the off median by more than the off runs' min - max spread;
  2. the launches "colour stats" and "preprocess colour" next to "preprocess windows" (the random_crop mode) and "preprocess" + "normalize" (no mode)
     at the pass size, all in that same process (pvr_trainer_debug_set_timing: an event pair around every launch), median of --steps forwards each,
     next to the bytes they move per output pixel: 12 B read (four uint8 taps of three channels) by the stats launch, 12 B read + 16 B written by
     the image launch.  "colour stats" includes the memset of the pass's gray sums.

    python scripts/color_jitter_step_times.py [--steps 5] [--T 100] [--only resnet18] [--strengths 0.4 0.4 0.4] [--out profiles/color_jitter_step_times.txt]
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


def stepper(name, T, chunk, strengths):
    net = E.EmbeddingNet(name, pretrained=False, train=True, freeze_bn=True, max_batch=chunk,
                         **({'color_jitter': strengths, 'color_seed': 1} if strengths else {}))
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    obs, done, act = batch(T)

    def one():
        opt.scheduler_step()
        opt.step(obs, done, act)
    return one, model


def step_table(name, T, chunk, steps, strengths, lines):
    n = T * B * F_
    off, m_off = stepper(name, T, chunk, None)
    on, m_on = stepper(name, T, chunk, strengths)
    off(), on()                                                # warm-up: allocates the workspaces
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(steps):
        ms[False].append(timed(off))
        ms[True].append(timed(on))
    passes = len(m_off.embedding._passes(n))
    d = statistics.median(ms[True]) - statistics.median(ms[False])
    room = max(ms[False]) - min(ms[False])
    lines.append('%-9s %5d  %6d  off: %-46s on: %-46s %+8.2f  %6.2f  %s'
                 % (name, chunk, passes, spread(ms[False]), spread(ms[True]), d, room, 'slower' if d > room else 'not slower'))
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


IMAGE = ('preprocess', 'normalize', 'preprocess windows', 'colour stats', 'preprocess colour')


def launch_table(name, chunk, steps, strengths, lines):
    sd, variant = E._load_named_state_dict(name, False)
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(chunk, device='cuda') % 64].contiguous()
    got = {}
    for mode, kw in (('centre', {}), ('windows', {'random_crop': True}), ('colour', {'color_jitter': strengths})):
        m = E.HipTrainableResNet(sd, variant, max_batch=chunk, freeze_bn=True, **kw)
        m.train()
        m._forward_raw(fr)                                     # warm-up
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        rows = []
        for _ in range(steps):
            m._forward_raw(fr)
            torch.cuda.synchronize()
            rows.append(launches(m._handle))
        got[mode] = {k: statistics.median(r[k] for r in rows) for k in rows[0] if k in IMAGE}
        del m
        torch.cuda.empty_cache()
    assert sorted(got['centre']) == ['normalize', 'preprocess'] and sorted(got['windows']) == ['preprocess windows'], got
    assert sorted(got['colour']) == ['colour stats', 'preprocess colour'], got
    px = chunk * 224 * 224
    two = got['centre']['preprocess'] + got['centre']['normalize']
    one = got['windows']['preprocess windows']
    st, im = got['colour']['colour stats'], got['colour']['preprocess colour']
    lines.append('%-9s %5d  preprocess %.3f + normalize %.3f = %.3f ms   preprocess windows %.3f ms (%.2f GB: %.2f TB/s)   colour stats %.3f ms (%.2f GB: '
                 '%.2f TB/s) + preprocess colour %.3f ms (%.2f GB: %.2f TB/s) = %.3f ms   colour / windows %.2f'
                 % (name, chunk, got['centre']['preprocess'], got['centre']['normalize'], two, one, px * 28 / 1e9, px * 28 / one / 1e9, st, px * 12 / 1e9,
                    px * 12 / st / 1e9, im, px * 28 / 1e9, px * 28 / im / 1e9, st + im, (st + im) / one))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--strengths', type=float, nargs=3, default=(0.4, 0.4, 0.4))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'color_jitter_step_times.txt'))
    a = ap.parse_args()
    strengths = tuple(a.strengths)
    trunks = [(nm, ch) for nm, ch in (('resnet18', 640), ('resnet50', 320)) if a.only in (None, nm)]
    lines = ['the color_jitter mode (scripts/color_jitter_step_times.py), %s; one process, frozen BatchNorm, eager launches, BatchNorm1d on, 64x64 frames, '
             'strengths %g %g %g; a warm-up, then %d timed steps per figure, the two modes alternating' % ((torch.cuda.get_device_name(0),) + strengths
                                                                                                        + (a.steps,)), '',
             '-- the fused step, T %d x B %d x %d frames = %d frames per step: color_jitter off and on (ms per step) --' % (a.T, B, F_, a.T * B * F_),
             'trunk     chunk  passes  %-51s %-50s on - off  spread  verdict' % ('off', 'on')]
    for nm, ch in trunks:
        step_table(nm, a.T, ch, a.steps, strengths, lines)
    lines += ['(on - off: difference of the medians; spread: max - min of the off runs; slower: the difference exceeds that spread)', '',
              '-- the image of one pass: no mode, random_crop, color_jitter (ms, per-launch events, median of %d forwards) --' % a.steps,
              '(bytes per output pixel: colour stats 12 read; preprocess windows and preprocess colour 12 read + 16 written; the uint8 taps mostly hit in '
              'cache, so the rates are upper bounds of the HBM traffic; colour stats includes the memset of the gray sums)']
    for nm, ch in trunks:
        launch_table(nm, ch, a.steps, strengths, lines)
    lines.append('')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
