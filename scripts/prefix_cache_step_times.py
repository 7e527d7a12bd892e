"""The prefix_cache mode (pvr_trainer_prefix_forward, pvr_op_gather_rows; HipJointRMSprop.step_cached) -> profiles/prefix_cache_step_times.txt.
One process, frozen BatchNorm, T = 100, B = 16, two frames per observation, BatchNorm1d on, 64x64 frames, a synthetic dataset of 4000 samples resident
on the device (bc_data.DeviceDataset), the driver's default chunk of each mode (main_bc_finetune.check_workspace_fits).

For resnet18 and resnet50 at stages 1 .. 4, all-fp32 and with both split modes, an iteration as the driver runs it - the sampler's start indices, then
DeviceDataset.gather + HipJointRMSprop.step with prefix_once, or DeviceDataset.rows + the action / done rows + step_cached with prefix_cache - a warm-up
and --steps timed iterations each (device events), with the same start indices in every leg.  prefix_once is measured twice, in two separately built
models: the difference of the two medians is the run-to-run spread a difference between the modes is held against.  Then prefix_cache: the cache's
bytes, its fill time and frames/s, the iteration, and pvr_op_gather_rows alone on one full pass of the step's rows (device events, --reps launches):
its time and the bytes it moves (rows read + rows written) per second.  A cache that does not fit next to the workspace is reported as such.

    python scripts/prefix_cache_step_times.py [--steps 5] [--T 100] [--samples 4000] [--only resnet50] [--out profiles/prefix_cache_step_times.txt]
"""
import argparse
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from pvr_habitat_amd import synth  # noqa: E402
from pvr_habitat_amd import embeddings as E  # noqa: E402
from pvr_habitat_amd import models as M  # noqa: E402
from pvr_habitat_amd import main_bc_finetune as Fz  # noqa: E402
from pvr_habitat_amd.bc_data import DeviceDataset  # noqa: E402
from pvr_habitat_amd.utils_bc import sample_with_minimum_distance  # noqa: E402
from frozen_bn_step_times import B, F_, timed  # noqa: E402
from train_from_step_times import Lines, mmm  # noqa: E402

STREAM_TBS = 6.3                                               # a float4 copy kernel on this device (HBM3E: 8.0 TB/s peak, 6.29 TB/s measured)


def dataset(n_samples):
    """n_samples observations of F_ 64x64 frames: 64 smooth frames, rolled by the sample index so that no two samples are equal"""
    base = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()
    idx = torch.arange(n_samples * F_, device='cuda')
    fr = base[idx % 64]
    fr = (fr.to(torch.int16) + (idx // 64).view(-1, 1, 1, 1).to(torch.int16)).remainder(256).to(torch.uint8)
    obs = fr.view(n_samples, F_, 64, 64, 3).permute(0, 2, 3, 1, 4).reshape(n_samples, 64, 64, 3 * F_).contiguous()
    g = torch.Generator().manual_seed(3)
    return DeviceDataset(obs, torch.randint(0, 3, (n_samples,), generator=g).numpy(), np.zeros(n_samples, bool), 'cuda')


def flags_of(name, T, train_from, split, mode):
    return argparse.Namespace(embedding_name=name, unroll_length=T, batch_size=B, freeze_embedding_bn=True, embedding_chunk=None,
                              embedding_wgrad_split16=split, embedding_conv_split16=split, embedding_train_from=train_from,
                              embedding_prefix_once=mode == 'prefix_once', embedding_prefix_cache=mode == 'prefix_cache')


def leg(name, T, train_from, split, mode, ds, starts, steps, reps):
    """-> dict(ms=[...], chunk, passes [, cache_bytes, fill_s, gather_ms, gather_bytes])"""
    flags = flags_of(name, T, train_from, split, mode)
    Fz.check_workspace_fits(flags, F_, ds.n)                   # the driver's default chunk of this mode; RuntimeError when the cache does not fit
    chunk = flags.embedding_chunk
    modes = dict(wgrad_split16=True, conv_split16=True) if split else {}
    net = E.EmbeddingNet(name, pretrained=False, train=True, freeze_bn=True, max_batch=chunk, train_from=train_from, **modes, **{mode: True})
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    enc = net.embedding
    out = dict(chunk=chunk, passes=len(enc._passes(T * B * F_)))
    if mode == 'prefix_cache':
        cache = model.build_prefix_cache(ds.obs)
        out.update(cache_bytes=cache.nbytes, fill_s=cache.fill_seconds)
    it = iter(starts)

    def one():
        s = next(it)
        opt.scheduler_step()
        if mode == 'prefix_cache':
            rows = ds.rows(s, T)
            opt.step_cached(rows, ds.done[rows].bool(), ds.action[rows])
        else:
            o, a, d = ds.gather(s, T)
            opt.step(o, d, a)
    one()
    torch.cuda.synchronize()
    out['ms'] = timed(one, steps)
    if mode == 'prefix_cache':                                 # the gather alone: one full pass of a step's rows
        rows = model.cache_rows(ds.rows(starts[0], T))[:chunk].contiguous()
        enc._gather_pass(cache, rows, 0, rows.numel())
        torch.cuda.synchronize()
        ms = timed(lambda: enc._gather_pass(cache, rows, 0, rows.numel()), reps)
        out.update(gather_ms=ms, gather_bytes=2 * rows.numel() * enc.boundary_bytes())
    model.close()
    del opt, model, net, enc
    torch.cuda.empty_cache()
    return out


def table(name, T, steps, reps, ds, lines):
    n = T * B * F_
    random.seed(1)
    starts = [sample_with_minimum_distance(n=ds.n, k=B, d=T) for _ in range(steps + 1)]
    lines.append('== %s, frozen BatchNorm, fused step, T %d x B %d x %d frames = %d frames per step, %d samples = %d dataset frames =='
                 % (name, T, B, F_, n, ds.n, ds.n * F_))
    lines.append('%-10s %-7s %6s %7s  %-40s %-40s %7s  %-40s %7s %8s  %8s %7s %9s  %9s %8s %7s'
                 % ('arithmetic', 'stage', 'chunk', 'passes', 'prefix_once: ms per iteration', 'prefix_once again', 'spread', 'prefix_cache: ms per iteration',
                    'saved', 'slower?', 'cache GB', 'fill s', 'frames/s', 'gather ms', 'GB/s', 'of copy'))
    slower, slow_gather = [], []
    for split in (False, True):
        arith = 'split-f16' if split else 'fp32'
        for tf in E.TRAIN_FROM:
            a = leg(name, T, tf, split, 'prefix_once', ds, starts, steps, reps)
            b = leg(name, T, tf, split, 'prefix_once', ds, starts, steps, reps)
            ma, mb = statistics.median(a['ms']), statistics.median(b['ms'])
            spread = max(abs(ma - mb), max(a['ms']) - min(a['ms']), max(b['ms']) - min(b['ms']))
            try:
                c = leg(name, T, tf, split, 'prefix_cache', ds, starts, steps, reps)
            except RuntimeError as e:
                if '--embedding_prefix_cache' not in str(e):
                    raise
                lines.append('%-10s %-7s %6d %7d  %-40s %-40s %7.2f  the prefix cache does not fit: %s' % (arith, tf, a['chunk'], a['passes'], mmm(a['ms']), mmm(b['ms']), spread, e))
                continue
            mc = statistics.median(c['ms'])
            late = mc > min(ma, mb) + spread
            if late:
                slower.append((arith, tf))
            g = statistics.median(c['gather_ms'])
            rate = c['gather_bytes'] / (g * 1e-3) / 1e9
            if rate < 500 * STREAM_TBS:
                slow_gather.append((arith, tf, '%.0f GB/s' % rate))
            lines.append('%-10s %-7s %6s %7s  %-40s %-40s %7.2f  %-40s %7.1f %8s  %8.2f %7.2f %9.0f  %9.3f %8.0f %6.0f%%'
                         % (arith, tf, '%d/%d' % (a['chunk'], c['chunk']), '%d/%d' % (a['passes'], c['passes']), mmm(a['ms']), mmm(b['ms']), spread, mmm(c['ms']),
                            min(ma, mb) - mc, 'SLOWER' if late else 'no', c['cache_bytes'] / 2 ** 30, c['fill_s'], ds.n * F_ / c['fill_s'], g, rate,
                            rate / (10 * STREAM_TBS)))
    lines.append('(spread: the largest of |median - median| of the two prefix_once legs and their max - min; saved = the lower prefix_once median - the '
                 'prefix_cache median; slower: the prefix_cache median above that median + spread; gather: pvr_op_gather_rows on one full pass (chunk rows), '
                 'bytes read + written per second, next to a float4 copy kernel\'s %.1f TB/s on this device)' % STREAM_TBS)
    lines.append('rows where prefix_cache is slower than prefix_once beyond the spread: %s' % (slower or 'none'))
    lines.append('rows where the gather reaches less than half of the copy rate: %s' % (slow_gather or 'none'))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--samples', type=int, default=4000)
    ap.add_argument('--only', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prefix_cache_step_times.txt'))
    a = ap.parse_args()
    lines = Lines()
    lines.append('the prefix_cache mode (scripts/prefix_cache_step_times.py), %s; one process, frozen BatchNorm, eager launches, BatchNorm1d on, 64x64 frames; '
                 'a warm-up, then %d timed iterations per figure' % (torch.cuda.get_device_name(0), a.steps))
    lines.append('')
    ds = dataset(a.samples)
    for name in ('resnet50', 'resnet18'):
        if a.only in (None, name):
            table(name, a.T, a.steps, a.reps, ds, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
