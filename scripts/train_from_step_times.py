"""Partial fine-tuning (EmbeddingNet(..., train=True, freeze_bn=True, train_from=...), pvr_trainer_set_train_from) -> profiles/train_from_step_times.txt.
One process, frozen BatchNorm, B = 16, two frames per observation, BatchNorm1d on, 64x64 frames:

  1. the fused end-to-end BC step (models.HipJointRMSprop) at T = 100 for resnet18 and resnet50 at stages 0 .. 4, all-fp32 and with both split modes:
     workspace bytes, the default chunk (main_bc_finetune.check_chunk_fits: the largest frame count whose workspace fits nine tenths of the free
     memory), passes, ms per step (a warm-up step, then --steps timed steps: median and spread) and frames/s; and whether any stage is slower than
     stage 0 of the same process by more than the two spreads (max - min);
  2. the fused prefix op's criterion: per-launch events (pvr_trainer_debug_set_timing) around the prefix ops of a stage-4 forward - "<conv> pack" +
     "<conv> bn frozen" - and around the same ops' "<conv> pack" + "<conv>" + "<bn>" launches of a stage-0 forward, a warm-up and --steps timed
     forwards each, at the frozen-BatchNorm pass sizes (320 resnet50 frames, 640 resnet18 frames) and at 32 frames: minimum, median and maximum of
     the sums, and per stage of the trunk.

--prefix_once (-> profiles/prefix_once_step_times.txt) is the leg of the prefix_once mode (pvr_trainer_forward_boundary, pvr_trainer_set_prefix_fused)
instead: for every row of the table above that has a prefix (resnet18 / resnet50, fp32 and both split modes, stages 1 .. 4) the same fused step with
the mode off and on in one process - a warm-up step and --steps timed steps each - next to the per-launch sum of the stem and the prefix of one
full pass, off and on (pvr_trainer_debug_set_timing), the predicted saving (passes - 1) x that sum of the mode-off pass, and whether the measured
saving reaches half of it; then the split prefix op as three launches against scale + ONE launch, summed over the prefix ops of a stage-4 forward at
320 resnet50 frames and 640 resnet18 frames.

    python scripts/train_from_step_times.py [--steps 5] [--T 100] [--only resnet50] [--part steps|launches] [--out profiles/train_from_step_times.txt]
    python scripts/train_from_step_times.py --prefix_once [--steps 5] [--T 100] [--only resnet50]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from pvr_habitat_amd import _lib, synth  # noqa: E402
from pvr_habitat_amd import embeddings as E  # noqa: E402
from pvr_habitat_amd import models as M  # noqa: E402
from pvr_habitat_amd import main_bc_finetune as Fz  # noqa: E402
from frozen_bn_step_times import B, F_, batch, timed, launches  # noqa: E402

STAGES = (None,) + E.TRAIN_FROM


class Lines(list):
    """the report: a line is printed as soon as it is known (a run of many steps shows where it is)"""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def mmm(v):
    return 'min %.2f, median %.2f, max %.2f' % (min(v), statistics.median(v), max(v))


def prefix_launch_ms(enc, stage, frames):
    """per-launch events around ONE full pass of `frames` frames: (ms of the stem's and the prefix's launches, ms of the prefix's layer launches alone)"""
    L = _lib.lib()
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(frames, device='cuda') % 64].contiguous()
    _lib.check(L.pvr_trainer_debug_set_timing(enc._handle, 1))
    enc._forward_raw(fr)
    enc._boundary = None
    torch.cuda.synchronize()
    rows = launches(enc._handle)
    _lib.check(L.pvr_trainer_debug_set_timing(enc._handle, 0))
    first = [n for n, _ in rows].index(stage + '.0.conv1' + (' scale' if enc.conv_split16 else ' pack'))
    return sum(t for _, t in rows[:first]), sum(t for n, t in rows[:first] if n.startswith('layer'))


def step_case(name, T, train_from, split, steps, prefix_once=False, launch_sums=False):
    n = T * B * F_
    flags = argparse.Namespace(embedding_name=name, unroll_length=T, batch_size=B, freeze_embedding_bn=True, embedding_chunk=None,
                               embedding_wgrad_split16=split, embedding_conv_split16=split, embedding_train_from=train_from,
                               embedding_prefix_once=prefix_once)
    Fz.check_workspace_fits(flags, F_)                         # the driver's default chunk of this mode
    chunk = flags.embedding_chunk
    modes = dict(wgrad_split16=True, conv_split16=True) if split else {}
    if prefix_once:
        modes['prefix_once'] = True
    net = E.EmbeddingNet(name, pretrained=False, train=True, freeze_bn=True, max_batch=chunk, **modes, **({'train_from': train_from} if train_from else {}))
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    obs, done, act = batch(T)

    def one():
        opt.scheduler_step()
        opt.step(obs, done, act)
    one()
    torch.cuda.synchronize()
    ms = timed(one, steps)
    out = (ms, net.embedding.workspace_bytes(), chunk, len(net.embedding._passes(n)))
    if launch_sums:
        out += prefix_launch_ms(net.embedding, train_from, chunk)
    model.close()
    del opt, model, net
    torch.cuda.empty_cache()
    return out


def steps_part(name, T, steps, lines):
    n = T * B * F_
    lines.append('== %s, frozen BatchNorm, fused step, T %d x B %d x %d frames = %d frames per step ==' % (name, T, B, F_, n))
    lines.append('%-10s %-8s %12s %6s %7s  %-52s %10s' % ('arithmetic', 'stage', 'workspace GB', 'chunk', 'passes', 'ms per step', 'frames/s'))
    slower = []
    for split in (False, True):
        base = None
        for tf in STAGES:
            ms, ws, chunk, passes = step_case(name, T, tf, split, steps)
            med = statistics.median(ms)
            if tf is None:
                base = ms
            elif med > statistics.median(base) + (max(ms) - min(ms)) + (max(base) - min(base)):
                slower.append((split, tf))
            lines.append('%-10s %-8s %12.2f %6d %7d  %-52s %10.1f' % ('split-f16' if split else 'fp32', tf or 'all', ws / 2 ** 30, chunk, passes, mmm(ms), n / med * 1e3))
    lines.append('stages slower than stage 0 of the same arithmetic beyond the two spreads: %s' % (slower or 'none'))
    lines.append('')


def prefix_once_part(name, T, steps, lines):
    n = T * B * F_
    lines.append('== %s, frozen BatchNorm, fused step, T %d x B %d x %d frames = %d frames per step: prefix_once off and on ==' % (name, T, B, F_, n))
    lines.append('%-10s %-7s %6s %7s %9s  %-44s %-44s %9s %9s %9s %9s  %s'
                 % ('arithmetic', 'stage', 'chunk', 'passes', 'cache GB', 'off: ms per step', 'on: ms per step', 'pass off', 'pass on', 'predicted', 'measured', 'at least half'))
    missed = []
    for split in (False, True):
        for tf in E.TRAIN_FROM:
            off = step_case(name, T, tf, split, steps, False, True)
            on = step_case(name, T, tf, split, steps, True, True)
            predicted = (off[3] - 1) * off[4]
            measured = statistics.median(off[0]) - statistics.median(on[0])
            ok = measured >= 0.5 * predicted
            if not ok:
                missed.append(('split-f16' if split else 'fp32', tf))
            lines.append('%-10s %-7s %6s %7d %9.2f  %-44s %-44s %9.2f %9.2f %9.1f %9.1f  %s'
                         % ('split-f16' if split else 'fp32', tf, '%d/%d' % (off[2], on[2]), on[3], n * E.trainer_boundary_bytes(name, tf) / 2 ** 30, mmm(off[0]),
                            mmm(on[0]), off[4], on[4], predicted, measured, 'yes' if ok else 'NO'))
    lines.append('(pass off / pass on: ms of the stem\'s and the prefix\'s launches of one full pass, per-launch events; predicted = (passes - 1) x pass off; '
                 'measured = median off - median on)')
    lines.append('rows whose measured saving is below half of the prediction: %s' % (missed or 'none'))
    lines.append('')


def fused_split_part(name, frames, steps, lines):
    """the split prefix ops of a stage-4 forward: scale + split16 + BatchNorm (off) against scale + ONE launch (on)"""
    sums = {}
    for on in (False, True):
        sd, variant = E._load_named_state_dict(name, False)
        m = E.HipTrainableResNet(sd, variant, max_batch=frames, freeze_bn=True, conv_split16=True, train_from='layer4', **({'prefix_once': True} if on else {}))
        m.train()
        prefix_launch_ms(m, 'layer4', frames)                  # warm-up: makes the workspace
        sums[on] = [prefix_launch_ms(m, 'layer4', frames)[1] for _ in range(steps)]
        del m
        torch.cuda.empty_cache()
    gain = statistics.median(sums[False]) - statistics.median(sums[True])
    lines.append('%s, %d frames, the split prefix ops of layer1 .. layer3 (ms per forward, %d timed forwards):' % (name, frames, steps))
    lines.append('   three launches (scale + split16 + BatchNorm)      %s' % mmm(sums[False]))
    lines.append('   two launches   (scale + split16 bn frozen)        %s' % mmm(sums[True]))
    lines.append('   median of three - median of two %.2f ms: %s' % (gain, 'the fused form is lower' if gain > 0 else 'NOT LOWER'))
    lines.append('')


def forward_rows(name, frames, train_from, steps):
    sd, variant = E._load_named_state_dict(name, False)
    m = E.HipTrainableResNet(sd, variant, max_batch=frames, freeze_bn=True, **({'train_from': train_from} if train_from else {}))
    m.train()
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(frames, device='cuda') % 64].contiguous()
    m._forward_raw(fr)                                         # warm-up: makes the workspace
    torch.cuda.synchronize()
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
    runs = []
    for _ in range(steps):
        m._forward_raw(fr)
        torch.cuda.synchronize()
        runs.append(launches(m._handle))
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 0))
    del m
    torch.cuda.empty_cache()
    return runs


def launches_part(name, frames, steps, lines):
    fused, plain = forward_rows(name, frames, 'layer4', steps), forward_rows(name, frames, None, steps)
    convs = [n[:-len(' bn frozen')] for n, _ in fused[0] if n.endswith(' bn frozen')]
    groups = sorted(set(c.split('.')[0] for c in convs))

    def sums(runs, width, group=None):
        out = []
        for rows in runs:
            names = [n for n, _ in rows]
            total = 0.0
            for c in convs:
                if group is None or c.startswith(group + '.'):
                    i = names.index(c + ' pack')
                    total += sum(t for _, t in rows[i:i + width])
            out.append(total)
        return out
    f, u = sums(fused, 2), sums(plain, 3)
    gain = statistics.median(u) - statistics.median(f)
    spreads = (max(f) - min(f)) + (max(u) - min(u))
    lines.append('%s, %d frames, the %d prefix ops of layer1 .. layer3 (ms per forward, %d timed forwards):' % (name, frames, len(convs), steps))
    lines.append('   fused    (pack + convolution with the BatchNorm epilogue)   %s' % mmm(f))
    lines.append('   unfused  (pack + convolution + BatchNorm launch)            %s' % mmm(u))
    lines.append('   unfused median - fused median %.2f ms, the two spreads %.2f ms: %s' % (gain, spreads, 'the fused form pays' if gain > spreads else 'NO GAIN'))
    for g in groups:
        fg, ug = sums(fused, 2, g), sums(plain, 3, g)
        lines.append('   %-8s fused %s | unfused %s' % (g, mmm(fg), mmm(ug)))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--part', default=None, choices=['steps', 'launches'])
    ap.add_argument('--prefix_once', action='store_true', help='the prefix_once leg (see the module docstring) -> profiles/prefix_once_step_times.txt')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'prefix_once_step_times.txt' if a.prefix_once else 'train_from_step_times.txt')
    lines = Lines()
    if a.prefix_once:
        lines.append('the prefix_once mode (scripts/train_from_step_times.py --prefix_once), %s; one process, frozen BatchNorm, eager launches, BatchNorm1d on, '
                     '64x64 frames; a warm-up, then %d timed steps per figure' % (torch.cuda.get_device_name(0), a.steps))
        lines.append('')
        if a.part in (None, 'launches'):
            lines.append('-- the split prefix op: three launches against two, per-launch events --')
            for name, frames in (('resnet50', 320), ('resnet18', 640)):
                if a.only in (None, name):
                    fused_split_part(name, frames, a.steps, lines)
        if a.part in (None, 'steps'):
            lines.append('-- the step by stage, the mode off and on --')
            for name in ('resnet50', 'resnet18'):
                if a.only in (None, name):
                    prefix_once_part(name, a.T, a.steps, lines)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
        return
    lines.append('partial fine-tuning (scripts/train_from_step_times.py), %s; one process, frozen BatchNorm, eager launches, BatchNorm1d on, 64x64 frames; '
                 'a warm-up, then %d timed steps per line' % (torch.cuda.get_device_name(0), a.steps))
    lines.append('')
    if a.part in (None, 'launches'):
        lines.append('-- the fused prefix op against pack + convolution + BatchNorm, per-launch events --')
        for name, chunk in (('resnet50', 320), ('resnet18', 640)):
            if a.only in (None, name):
                for frames in (chunk, 32):
                    launches_part(name, frames, a.steps, lines)
    if a.part in (None, 'steps'):
        lines.append('-- the step by stage --')
        for name in ('resnet50', 'resnet18'):
            if a.only in (None, name):
                steps_part(name, a.T, a.steps, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
