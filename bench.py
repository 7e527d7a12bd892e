#!/usr/bin/env python3
"""Headline benchmark: frames/sec embedded by the frozen ResNet50 (MoCo-v2 layout) PVR encoder.

BASELINE.json metric "frames/sec embedded (ResNet50, 256x256)", workload = configs[1]:
ResNet50 MoCo-v2 frozen, 256x256 uint8 frames, batch 256, bf16, synthetic frames + synthetic weights
(no network).  A step = one pass of the hot path (resize/crop/normalise + 53 convs + pool) over one
batch of 256 frames that is already resident in HBM.  Frames shard across ranks with no collective
(SURVEY 8e): weak scaling, value = frames all ranks embedded / max-over-ranks time.

  python bench.py                      (N = 1, 320 timed steps ~ 1 s over a 4096-frame pool: the headline leg alone)
  python bench.py --gpus 1 --steps 20 --warmup 3
  python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR   (+ DIR/embeddings.npy: what the last timed step computed)
  python bench.py --full               (+ one-lane / bf16 / roofline / parity / CPU baseline / PNG / PCIe / e2e / 5-crop / ViT / BC legs)
  python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
  python bench.py --gpus N --steps K --warmup W        (no launcher: starts that torch.distributed.run command itself as a child process)

Without --full a run sets up, warms up, times the steps, writes --dump-outputs and prints the headline line: nothing else.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

GFLOP_PER_FRAME = 8.174           # 2 x 4.0871 GMAC, 53 convs @ 224x224
PEAK_BF16_TFLOPS = 2500.0         # MI355X dense bf16/f16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3           # f32-input MFMA (= the fp32 vector rate), reference-precision mode only


def conv_algorithmic_bytes(n, names=None):
    """Activation bytes (16-bit) the conv launches of one n-frame chunk must move: input + output (+ residual) of every
    launch of the plan `names` (HipResNet50.op_names(); a fused bottleneck tail 'a.conv2+conv3+b.conv1' reads t1 and the
    residual and writes y and the next block's t1, nothing else).  names=None: one launch per convolution."""
    def geom(layer, block):
        planes = 64 << (layer - 1)
        hw_out = 56 >> (layer - 1)
        hw_in = hw_out * 2 if (block == 0 and layer > 1) else hw_out
        inpl = (64 if layer == 1 else planes * 2) if block == 0 else planes * 4
        return planes, hw_in, hw_out, inpl
    if names is None:
        names = []
        for li, nb in enumerate((3, 4, 6, 3)):
            for bi in range(nb):
                names += ['layer%d.%d.conv1' % (li + 1, bi), 'layer%d.%d.conv2' % (li + 1, bi)]
                if bi == 0:
                    names.append('layer%d.%d.downsample.0' % (li + 1, bi))
                names.append('layer%d.%d.conv3' % (li + 1, bi))
    tot = 0
    for nm in names:
        parts = nm.split('+')
        head = parts[0].split('.')
        layer, block, kind = int(head[0][5:]), int(head[1]), head[2]
        planes, hi, ho, inpl = geom(layer, block)
        if len(parts) > 2 and kind == 'conv1' and parts[1] == 'conv2':      # the whole bottleneck per frame (bneck_frame.hip): x in (the identity is the same tensor), y out
            tot += hi * hi * inpl + ho * ho * planes * 4
        elif len(parts) > 1:                                 # conv2 -> conv3 (+ residual) [-> next conv1]
            if '&downsample' in parts[1]:                        # identity branch computed from the block input: x in, y out
                tot += hi * hi * planes + hi * hi * inpl + ho * ho * planes * 4
            else:
                tot += hi * hi * planes + 2 * ho * ho * planes * 4
            if len(parts) > 2:
                nh = parts[2].split('.')
                tot += ho * ho * geom(int(nh[0][5:]), int(nh[1]))[0]
        elif kind == 'conv1':
            tot += hi * hi * inpl + hi * hi * planes
        elif kind == 'conv2':
            tot += hi * hi * planes + ho * ho * planes
        elif kind == 'downsample':
            tot += hi * hi * inpl + ho * ho * planes * 4
        elif kind == 'conv3&downsample':                     # the two-operand launch (conv_pp256 DUAL): t2 and the strided pixels of the block input in, y out
            tot += ho * ho * planes + ho * ho * inpl + ho * ho * planes * 4
        elif kind == 'conv3':
            tot += ho * ho * planes + 2 * ho * ho * planes * 4
    return tot * 2 * n


def cpu_limits():
    """what this process may actually use: the scheduler affinity mask and the cgroup CPU quota (cpu.max: "<quota> <period>" or "max")"""
    lim = {'os_cpu_count': os.cpu_count()}
    try:
        lim['affinity_cores'] = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        lim['affinity_cores'] = None
    quota = None
    for f in ('/sys/fs/cgroup/cpu.max', '/sys/fs/cgroup/cpu/cpu.cfs_quota_us'):
        try:
            txt = open(f).read().split()
            if f.endswith('cpu.max'):
                quota = None if txt[0] == 'max' else round(int(txt[0]) / int(txt[1]), 2)
            else:
                q = int(txt[0])
                quota = None if q <= 0 else round(q / int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read()), 2)
            break
        except (OSError, ValueError, IndexError):
            continue
    lim['cgroup_cpu_quota'] = quota                       # CPUs' worth of time per period; None = unlimited
    return lim


def cpu_baseline(sd, frames_u8, budget_s=12.0):
    """The oracle (torch fp32 eager restatement of the reference path) timed on this box's host cores,
    batch 64 like the reference's 32 obs x 2 frames (save_embedded_obs.py:151-153).  `cores` = the thread count of the timed sample = the
    fastest of a sweep (torch's CPU convolutions stop scaling - and regress - at high thread counts: the sweep is in the line, next to the
    affinity mask and the cgroup quota, so that `cores` can be read against what the process was allowed to use)."""
    from oracle import encoder_oracle as eo
    lim = cpu_limits()
    avail = lim['affinity_cores'] or os.cpu_count() or 1
    if lim['cgroup_cpu_quota']:
        avail = max(1, min(avail, int(lim['cgroup_cpu_quota'])))
    sweep, best, best_t = {}, 1, float('inf')
    for th in sorted({min(avail, t) for t in (1, 4, 8, 16, 32, 64, 128, 256)}):
        torch.set_num_threads(th)
        nfr = 4 if th == 1 else 16
        eo.embed(sd, frames_u8[:min(8, nfr)], 'conv5')         # warm-up at this thread count
        t0 = time.perf_counter(); eo.embed(sd, frames_u8[:nfr], 'conv5'); dt = time.perf_counter() - t0
        sweep[str(th)] = round(nfr / dt, 2)
        if dt / nfr < best_t:
            best, best_t = th, dt / nfr
    torch.set_num_threads(best)

    def sustained(bs, budget, cap):
        done, t0 = 0, time.perf_counter()
        while True:
            eo.embed(sd, frames_u8[:bs], 'conv5')
            done += bs
            el = time.perf_counter() - t0
            if el > budget or done >= cap:
                return done, el
    # `value`: sustained over >= budget_s at the reference's batch (32 obs x 2 frames = 64).  The sweep above times ONE 16-frame batch per
    # thread count: a burst on a 4x smaller working set.  The same 16-frame batches SUSTAINED at the same thread count are timed here too, so the
    # line separates the two effects (batch size vs burst) instead of leaving two figures that do not agree.
    done, el = sustained(64, budget_s, 64 * 8)
    done16, el16 = sustained(16, budget_s / 3, 16 * 16)
    res = dict(value=round(done / el, 2), unit='frames/s', cores=torch.get_num_threads(), kind='port',
               sample='%d synthetic 256x256 frames in batches of 64, torch fp32 eager oracle, %.1f s' % (done, el),
               cpu_model=cpu_model(), box_cores=os.cpu_count(), affinity_cores=lim['affinity_cores'], cgroup_cpu_quota=lim['cgroup_cpu_quota'],
               sustained_batch16={'value': round(done16 / el16, 2), 'unit': 'frames/s', 'cores': torch.get_num_threads(),
                                  'sample': '%d frames in batches of 16, %.1f s' % (done16, el16)},
               thread_sweep_frames_per_s=sweep,
               thread_sweep_note='ONE 16-frame batch per thread count (4 frames at 1 thread) after a warm-up - a burst, used only to pick `cores` (the fastest); '
                                 '`value` is the sustained rate at the reference\'s batch of 64 (save_embedded_obs.py:151-153), `sustained_batch16` the sustained rate of the '
                                 'sweep\'s own batch size at the same thread count: value vs sustained_batch16 = the cost of the 4x larger activation working set per '
                                 'batch, sustained_batch16 vs the sweep entry = sustained vs burst (CFS quota, clocks)')
    # the reference launchers pin OMP_NUM_THREADS=1 (slurm_eo.py:13): the same oracle on ONE thread, on a smaller sample
    torch.set_num_threads(1)
    eo.embed(sd, frames_u8[:2], 'conv5')
    t0 = time.perf_counter(); eo.embed(sd, frames_u8[:8], 'conv5'); dt1 = time.perf_counter() - t0
    res['one_thread'] = dict(value=round(8 / dt1, 3), unit='frames/s', cores=1, sample='8 frames in one batch, %.1f s' % dt1)
    torch.set_num_threads(best)
    return res


def cpu_model():
    try:
        for ln in open('/proc/cpuinfo'):
            if ln.lower().startswith('model name'):
                return ln.split(':', 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


BC_GFLOP_PER_STEP = 211.4         # PolicyNet T=100,B=16,obs 4096: 3 x fwd of 22.02 MMAC x 1600
INFINITY_CACHE_GBPS = 8600.0      # MI355X_MICROARCH.md: uniformly gathered rows of a 38 MB table served from the Infinity Cache, chip-wide


def bc_bench(steps, warmup, with_cpu):
    """Second half of the BASELINE metric: BC steps/sec (main_bc_2.py:186-227 iteration, slurm_bc.py:121-128
    configuration T=100, B=16, obs 4096, BatchNorm on, RMSprop) on one GPU.
      value        the iteration alone on two batches resident in HBM (the kernel path)
      loop         what main_bc_2.run's loop delivers: Python sampler (sample_with_minimum_distance) -> device gather of the (T,B)
                   batch from the HBM-resident dataset (pvr_bc_gather) -> scheduler step -> the same iteration, 20 k samples
      roofline     the step against the f32-MFMA roof (algorithmic 211.4 GFLOP), and the LSTM recurrences against the weight stream
                   they are bound by: every one of the 2 x T recurrent launches re-reads its layer's 16.8 MB W_hh (it does not fit
                   one XCD's 4 MB L2, so it streams from the Infinity Cache), forward and again in BPTT"""
    import random
    from pvr_habitat_amd import synth
    from pvr_habitat_amd.bc_data import DeviceDataset
    from pvr_habitat_amd.models import PolicyNet, HipRMSprop
    from pvr_habitat_amd.utils_bc import sample_with_minimum_distance
    T, B, O, A = 100, 16, 4096, 3
    m = PolicyNet((O,), A, True, max_unroll=T, max_batch=B)
    sd = synth.policy_state_dict(1, O, A, True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m = m.to('cuda').train()
    opt = HipRMSprop(m, max_epochs=10 ** 6)
    obs, done, act = synth.bc_batches(1, T, B, O, A, 2)
    obs_d, done_d, act_d = torch.from_numpy(obs).cuda(), torch.from_numpy(done).cuda(), torch.from_numpy(act).cuda()
    for i in range(warmup):
        opt.scheduler_step(); opt.step(obs_d[i % 2], done_d[i % 2], act_d[i % 2])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        opt.scheduler_step(); loss, gn = opt.step(obs_d[i % 2], done_d[i % 2], act_d[i % 2])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    res = {'metric': 'BC steps/sec (PolicyNet T=100 B=16 obs=4096 BN, fp32)', 'value': round(steps / el, 2), 'unit': 'steps/s',
           'ms_per_step': round(el / steps * 1e3, 3), 'dtype': 'f32', 'final_loss': round(float(loss), 5)}
    # the loop of main_bc_2.run (bc_loop.train): sampler + device gather + step, dataset resident in HBM
    n = 20000
    data_obs = np.abs(synth.normal(2, 'bc_loop_obs', (n, O)))
    ds = DeviceDataset(data_obs, (synth.uniform(2, 'bc_loop_act', (n,)) * A).astype(np.int64).clip(0, A - 1), synth.uniform(2, 'bc_loop_done', (n,)) < 0.02)
    random.seed(1)
    for _ in range(max(warmup, 2)):
        o, a, d = ds.gather(sample_with_minimum_distance(n=n, k=B, d=T), T); opt.scheduler_step(); opt.step(o, d, a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        o, a, d = ds.gather(sample_with_minimum_distance(n=n, k=B, d=T), T)
        opt.scheduler_step(); loss, gn = opt.step(o, d, a)
    torch.cuda.synchronize()
    el_loop = time.perf_counter() - t0
    res['loop'] = {'value': round(steps / el_loop, 2), 'unit': 'steps/s', 'ms_per_step': round(el_loop / steps * 1e3, 3),
                   'what': 'sample_with_minimum_distance + pvr_bc_gather from a %d-sample dataset in HBM + scheduler + fused step '
                           '(the loop of main_bc_2.run); per step %d bytes of start indices cross PCIe' % (n, 8 * B)}
    # recurrences: an eval-mode forward of the same (T,B) is BN-apply + 2 fc GEMMs + 2 hoisted projections + 2*T recurrent launches + heads
    m.eval()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    inp = dict(obs=obs_d[0], done=done_d[0])
    with torch.no_grad():
        for _ in range(3):
            m(inp, m.initial_state(B))
        ev0.record()
        for _ in range(10):
            m(inp, m.initial_state(B))
        ev1.record()
    torch.cuda.synchronize()
    fwd_ms = ev0.elapsed_time(ev1) / 10
    whh_bytes = 2 * T * 4 * 1024 * 1024 * 4                   # 2 layers x T steps x [4H][H] fp32
    tf = BC_GFLOP_PER_STEP * steps / el / 1e3
    res['roofline'] = {'bound': 'mfma', 'achieved': round(tf, 2), 'peak': PEAK_F32_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(tf / PEAK_F32_TFLOPS, 4),
                       'traffic': None, 'kernel': 'whole iteration (f32-input MFMA GEMMs + recurrences), algorithmic %.1f GFLOP/step' % BC_GFLOP_PER_STEP,
                       'recurrence_weight_stream': {
                           'bound': 'infinity-cache', 'achieved': round(whh_bytes / (fwd_ms * 1e-3) / 1e9, 1), 'peak': INFINITY_CACHE_GBPS, 'unit': 'GB/s',
                           'frac': round(whh_bytes / (fwd_ms * 1e-3) / 1e9 / INFINITY_CACHE_GBPS, 4), 'forward_ms': round(fwd_ms, 3),
                           'note': 'W_hh bytes the %d recurrent launches of one forward re-read (%.2f GB) / wall time of that forward (incl. its '
                                   'five GEMMs): a lower bound on the rate of the recurrent launches themselves' % (2 * T, whh_bytes / 1e9)}}
    if with_cpu:
        from oracle import policy_oracle as po
        torch.set_num_threads(min(os.cpu_count() or 1, 32))
        p = po.to_params(sd)
        o = po.RMSpropState(p, max_epochs=10 ** 6)
        po.bc_step(p, o, torch.from_numpy(obs[0]), torch.from_numpy(done[0]), torch.from_numpy(act[0]), True)
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 8.0 and n < 5:
            po.bc_step(p, o, torch.from_numpy(obs[n % 2]), torch.from_numpy(done[n % 2]), torch.from_numpy(act[n % 2]), True); n += 1
        res['cpu_baseline'] = {'value': round(n / (time.perf_counter() - t0), 3), 'unit': 'steps/s', 'cores': torch.get_num_threads(),
                               'kind': 'port', 'sample': '%d oracle steps (torch fp32 autograd restatement)' % n}
    return res


def finetune_dp_bench(dist, steps, warmup):
    """BASELINE config 4 (N > 1): data-parallel finetune iteration - PolicyNetWithConv, T=100, B=16 sequences PER RANK (weak), SyncBN,
    gradient buckets all-reduced on RCCL while backward still runs.  Reports steps/s, the time of the same all-reduces issued alone
    (nothing to hide behind), and the fraction of that time the overlap hides: 1 - (t_dp - t_local) / t_allreduce."""
    from pvr_habitat_amd.models import PolicyNetWithConv, HipRMSprop, make_allreduce_fn
    T, B = 100, 16
    world, rank = dist.get_world_size(), dist.get_rank()
    torch.manual_seed(0)
    net = PolicyNetWithConv((64, 64, 6), 4, True, max_unroll=T, max_batch=B).to(device='cuda')
    opt = HipRMSprop(net, max_epochs=10 ** 6)
    g = torch.Generator().manual_seed(1 + rank)
    o = torch.randint(0, 256, (T, B, 64, 64, 6), dtype=torch.uint8, generator=g).cuda()
    d = (torch.rand((T, B), generator=g) < 0.02).cuda()
    a = torch.randint(0, 4, (T, B), generator=g).cuda()

    def timed(fn, k):
        dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize(); dist.barrier()
        return (time.perf_counter() - t0) / k

    def dp_step():
        opt.scheduler_step(); opt.step_data_parallel(o, d, a)

    def local_step():
        opt.scheduler_step(); opt.step(o, d, a)
    for _ in range(warmup):
        dp_step()
    t_dp = timed(dp_step, steps)
    # the same collectives alone: four bucket-sized all-reduces of the flat gradient, back to back, on an idle GPU
    fn, errors = make_allreduce_fn(None, 'cuda')
    grads = torch.zeros(net._n_train, dtype=torch.float32, device='cuda')
    bounds = [0, net._slots['fc.1.weight'][0], net._slots['core.weight_ih_l0'][0], net._slots['core.weight_ih_l1'][0], net._n_train]

    def comm_only():
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            if hi > lo:
                assert fn(grads.data_ptr() + 4 * lo, hi - lo, torch.cuda.current_stream().cuda_stream, None) == 0, errors
    comm_only()
    t_comm = timed(comm_only, steps)
    # uninstall the collective for the local leg: the same iteration without any all-reduce
    import pvr_habitat_amd.models as _M
    _M._lib.check(_M._plib().pvr_policy_set_data_parallel(net._handle, 1, 0, _M.ALLREDUCE_FN(), None)); net._dp_key = None
    for _ in range(2):
        local_step()
    t_local = timed(local_step, steps)
    hidden = 1.0 - max(t_dp - t_local, 0.0) / t_comm if t_comm > 0 else None
    return {'metric': 'finetune DP steps/sec (PolicyNetWithConv T=100, B=16 per rank, SyncBN, fp32, bucketed RCCL all-reduce overlapped with backward)',
            'value': round(1.0 / t_dp, 2), 'unit': 'steps/s', 'n_gpus': world, 'global_batch_sequences': B * world, 'scaling': 'weak',
            'ms_per_step': round(t_dp * 1e3, 3), 'ms_per_step_without_collectives': round(t_local * 1e3, 3),
            'allreduce_ms': round(t_comm * 1e3, 3), 'allreduce_bytes': int(net._n_train * 4), 'overlap_fraction': None if hidden is None else round(hidden, 3),
            'backend': dist.get_backend()}


def finetune_bench(steps, warmup):
    """BASELINE config 4 on one GPU: the end-to-end BC iteration of main_bc_finetune.py - PolicyNetWithConv (5 x (conv3x3 s2 + ELU) over
    every frame of the (T, B) batch, forward and backward) + the PolicyNet step; T = 100, B = 16, 64x64x6 uint8 observations, BN."""
    from pvr_habitat_amd.models import PolicyNetWithConv, HipRMSprop
    T, B = 100, 16
    torch.manual_seed(0)
    net = PolicyNetWithConv((64, 64, 6), 4, True, max_unroll=T, max_batch=B).to(device='cuda')
    opt = HipRMSprop(net, max_epochs=10 ** 6)
    g = torch.Generator().manual_seed(1)
    o = torch.randint(0, 256, (T, B, 64, 64, 6), dtype=torch.uint8, generator=g).cuda()
    d = (torch.rand((T, B), generator=g) < 0.02).cuda()
    a = torch.randint(0, 4, (T, B), generator=g).cuda()
    for _ in range(warmup):
        opt.scheduler_step(); opt.step(o, d, a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.scheduler_step(); loss, gn = opt.step(o, d, a)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    # algorithmic work of one iteration (SURVEY 8d conventions: forward MACs x 2 FLOP x 3 for forward + both backward products): the conv stack is
    # 4.02 MMAC per 64x64x3 frame x 3200 frames; the policy behind it is PolicyNet's 22.02 MMAC per sample with a 256-wide first layer
    # instead of 4096 (-3.93 MMAC) x 1600 samples
    gflop = (4.02 * T * B * 2 + (22.02 - 3.93) * T * B) * 2 * 3 / 1e3
    tf = gflop * steps / el / 1e3
    return {'metric': 'finetune steps/sec (PolicyNetWithConv T=100 B=16, 64x64x6 uint8, BN, fp32)', 'value': round(steps / el, 2), 'unit': 'steps/s',
            'ms_per_step': round(el / steps * 1e3, 3), 'frames_per_s_through_conv_stack': round(steps * T * B * 2 / el), 'dtype': 'f32',
            'final_loss': round(float(loss), 5),
            'roofline': {'bound': 'mfma', 'achieved': round(tf, 2), 'peak': PEAK_F32_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(tf / PEAK_F32_TFLOPS, 4), 'traffic': None,
                         'kernel': 'whole iteration (direct-conv forward / backward kernels + f32-input MFMA GEMMs + recurrences), algorithmic %.1f GFLOP/step; '
                                   'like the BC step it is a chain of dependent launches (T = 100 sequential BPTT steps at the launch floor), not a kernel on a roof' % gflop}}


VIT_GFLOP = {'clip_b32': 8.82, 'clip_b16': 35.13}      # per frame


def rank_spread(dist, el):
    """(slowest, fastest) of every rank's own elapsed time for the same leg: a straggler shows as max >> min (N = 1: both = el)"""
    if dist is None:
        return el, el
    t = torch.tensor([el, -el], dtype=torch.float64, device='cuda')
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t[0].item()), float(-t[1].item())


class LegGuard(object):
    """Keeps a one-sided failure inside a multi-rank leg from hanging the run: the legs are full of barriers / all-reduces, so a
    rank that raises (pin_memory out of memory, a full disk on rank 0, a FloatingPointError) would leave the others blocked in a collective
    until the launcher's time-out, and no JSON line.  A rank that fails writes its error to the rendezvous store - NOT a collective -; a watcher
    thread on every rank polls that key (and a per-leg deadline): when it fires, rank 0 prints the line it has so far with the error in it and
    every rank leaves with a non-zero exit code, promptly."""

    def __init__(self, dist, rank, get_line):
        import threading
        self.dist, self.rank, self.get_line = dist, rank, get_line
        self.deadline, self.leg = None, None
        self.store = None
        if dist is not None:
            try:
                from torch.distributed import distributed_c10d as c10d
                self.store = c10d._get_default_store()
            except Exception:
                self.store = None
            self._stop = threading.Event()
            threading.Thread(target=self._watch, name='pvr-leg-guard', daemon=True).start()

    def _abort(self, why):
        if self.rank == 0:
            line = self.get_line()
            if line is not None:
                line.setdefault('aborted', why)
                print(json.dumps(line), flush=True)
        os._exit(3)

    def _watch(self):
        while not self._stop.wait(1.0):
            if self.deadline is not None and time.time() > self.deadline:
                self._abort('leg %s did not finish within its time limit' % self.leg)
            if self.store is not None:
                try:
                    if self.store.check(['pvr_bench_abort']):
                        self._abort(self.store.get('pvr_bench_abort').decode(errors='replace'))
                except Exception:
                    pass

    def enter(self, leg, limit_s):
        self.leg, self.deadline = leg, (time.time() + limit_s if self.dist is not None else None)

    def leave(self):
        self.deadline = None

    def failed(self, leg, exc):
        """called by the rank whose leg raised (N > 1): tell the others, then leave"""
        msg = 'rank %d, leg %s: %s: %s' % (self.rank, leg, type(exc).__name__, exc)
        if self.store is not None:
            try:
                self.store.set('pvr_bench_abort', msg)
            except Exception:
                pass
        time.sleep(3.0)                      # rank 0's watcher prints the line; if THIS is rank 0 its own watcher does
        self._abort(msg)

    def close(self):
        if self.dist is not None:
            self._stop.set()


def vit_bench(variant, batch, steps, warmup, dtype, streams=None, dist=None):
    """BASELINE config 3: CLIP-layout ViT frozen, 224x224 frames resident in HBM, frames/s per GPU; at N > 1 every rank runs the leg at the same
    time (barrier on both sides): aggregate = all ranks' frames / the slowest rank's time, with the per-rank spread beside it."""
    world = dist.get_world_size() if dist is not None else 1
    from pvr_habitat_amd import synth
    from pvr_habitat_amd.embeddings import HipResNet50
    sd = synth.clip_vit_state_dict(1, patch=16 if variant == 'clip_b16' else 32)
    m = HipResNet50(sd, variant, compute_dtype=dtype, max_batch=batch)
    fr = torch.from_numpy(synth.frames(3, batch, 224, 224)).cuda()
    outs = [torch.empty((batch, 512), dtype=torch.float32, device='cuda') for _ in range(2)]
    streams = streams or [torch.cuda.Stream(), torch.cuda.Stream()]     # two batches in flight, as in the headline loop (streams shared with it)

    def run(k):
        for i in range(k):
            with torch.cuda.stream(streams[i % 2]):
                m.forward_into(fr, outs[i % 2], lane=i % 2)
    torch.cuda.synchronize()
    run(max(warmup, 2))
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    el_own = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    el, el_min = rank_spread(dist, el_own)
    assert torch.equal(outs[0], outs[1])
    fps = world * steps * batch / el
    m.close()
    res = {'metric': 'frames/sec embedded (%s, 224x224)' % variant, 'value': round(fps, 1), 'unit': 'frames/s', 'dtype': dtype,
           'ms_per_step': round(el / steps * 1e3, 3), 'batch': batch, 'tflops': round(fps * VIT_GFLOP[variant] / 1e3, 1),
           'frac_of_mfma_peak': round(fps * VIT_GFLOP[variant] / 1e3 / PEAK_BF16_TFLOPS / world, 4)}
    if world > 1:
        res.update(n_gpus=world, per_rank_ms_per_step={'min': round(el_min / steps * 1e3, 3), 'max': round(el / steps * 1e3, 3)},
                   note='all ranks at the same time, no collective in the timed region; value = all ranks\' frames / the slowest rank\'s time; frac_of_mfma_peak per GPU')
    return res


def pcie_bench(model_sd, batch, frames_np, dtype, passes=2, dist=None):
    """PCIe-inclusive rate (never the headline `value`): host-resident uint8 frames -> (pinned staging ->) H2D ->
    encoder -> D2H fp32 embeddings, overlapped on separate HIP streams (embeddings.stream_embed, the path save_embedded_obs uses).
    The whole frame pool (4096 frames = 16 batches) is streamed `passes` times per measurement, so pipeline fill / drain and the
    one-off buffer set-up are a small part of the timed region.

    dist (N > 1, round 5): every rank streams its own pool at the same time (barrier on both sides, MAX over ranks) - the ranks share the
    host's memory bandwidth, staging threads and PCIe root complexes, which is what SURVEY 8e names as the scaling limit of the
    precompute path; the aggregate is all ranks' frames over the slowest rank's time."""
    from pvr_habitat_amd.embeddings import HipResNet50, stream_embed
    world = dist.get_world_size() if dist is not None else 1

    class _Net:                                           # minimal EmbeddingNet-like holder
        pass
    net = _Net()
    net.embedding = HipResNet50(model_sd, 'conv5', compute_dtype=dtype, max_batch=batch)
    net.out_size = net.embedding.out_size
    fr = torch.from_numpy(frames_np).repeat(passes, 1, 1, 1)
    stream_embed(net, fr[:4 * batch], batch)              # warm-up (allocations, first launches, both lanes)
    res = {}
    for kind, src in (('pageable_source', fr), ('pinned_source', fr.pin_memory())):
        stream_embed(net, src, batch)                     # untimed full pass: the GPU has idled through the CPU legs before this one (clock ramp)
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        out = stream_embed(net, src, batch)
        if dist is not None:
            dist.barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device='cuda')
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        assert np.isfinite(out).all()
        res[kind] = {'value': round(world * fr.shape[0] / el, 1), 'unit': 'frames/s', 'h2d_GBps': round(world * fr.numel() / el / 1e9, 2)}
    res['frames'] = int(fr.shape[0]) * world
    res['n_gpus'] = world
    res['note'] = ('host uint8 frames (a pageable source is copied into a pinned staging ring by 8 native threads of the library (pvr_stage_copy) on a producer thread that runs ahead of the GPU work; page-locking it in place is opt-in: PVR_STREAM_REGISTER=1) -> H2D -> encode (two lanes) -> D2H fp32, '
                   'copies overlapped with compute on separate HIP streams; includes registering the source and allocating the page-locked result buffer'
                   + ('' if world == 1 else '; all %d ranks stream their own pool concurrently (barrier on both sides, max over ranks): aggregate rate' % world))
    net.embedding.close()
    return res


def png_source_bench(model_sd, batch, dtype, n_traj=48, length=250, hw=64):
    """the reference's per-frame PNG layout (save_opt_trajectories_png.py:44-58: <t>_<s>.png, <t>_goal.png, <t>.pickle;
    64x64 frames as habitat_config/nav_task.yaml renders them) read by save_embedded_obs.read_habitat_data_from_png: native threads
    read the file bytes, csrc/png_decode.hip inflates / unfilters them on the GPU, the frames go to the encoder without leaving HBM.
    A synthetic tree of n_traj x length files is written to a temporary directory first (untimed)."""
    import pickle, shutil, tempfile
    from PIL import Image
    from pvr_habitat_amd import synth, save_embedded_obs as S
    from pvr_habitat_amd.embeddings import EmbeddingNet
    d = tempfile.mkdtemp(prefix='pvr_png_bench_')
    try:
        fr = synth.smooth_frames(11, 512, hw, hw)
        for t in range(n_traj):
            for s_ in range(length):
                Image.fromarray(fr[(t * length + s_) % 512][..., ::-1]).save(os.path.join(d, '%d_%d.png' % (t, s_)), compress_level=1)
            Image.fromarray(fr[t % 512][..., ::-1]).save(os.path.join(d, '%d_goal.png' % t), compress_level=1)
            with open(os.path.join(d, '%d.pickle' % t), 'wb') as f:
                pickle.dump(dict(action=np.zeros(length, np.int64), reward=np.zeros(length), done=np.zeros(length, bool), true_state=np.zeros((length, 12))), f)
        os.environ.setdefault('PVR_SYNTHETIC_WEIGHTS', '1')
        net = EmbeddingNet('resnet50', pretrained=False, max_batch=batch, compute_dtype=dtype)
        quiet = open(os.devnull, 'w')
        import contextlib
        with contextlib.redirect_stdout(quiet):
            S.read_habitat_data_from_png(d, net, min(17, n_traj), batch=batch)       # warm-up: both decode groups' shapes, both lanes
            t0 = time.perf_counter()
            data = S.read_habitat_data_from_png(d, net, -1, batch=batch)
            el = time.perf_counter() - t0
        n = n_traj * length
        assert data['obs'].shape == (n, 2 * net.out_size) and np.isfinite(data['obs']).all()
        return {'metric': 'frames/sec embedded from the per-frame PNG tree (decode on the GPU + ResNet50)', 'value': round(n / el, 1), 'unit': 'frames/s',
                'files': n, 'frame': hw, 'dtype': dtype,
                'note': 'file bytes read by native threads, inflate + scanline filters + B,G,R packing on the GPU (bit-identical to the host decoder, '
                        'tests/test_gpu_png.py), frames stay in HBM; goal frame embedded per trajectory; includes the loop\'s host bookkeeping and the final row assembly'}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def save_obs_e2e_bench(batch, dtype, n_samples=100000, traj_len=500, hw=64, dist=None, reps=3):
    """The real driver end to end (round-3 verdict item 3c): pvr_habitat_amd.save_embedded_obs.run(flags) - the drop-in for the reference's
    behavioral_cloning/save_embedded_obs.py:96-172 - on a synthetic scene pickle of n_samples (hw, hw, 6) uint8 observations in the
    reference's per-trajectory layout (save_opt_trajectories.py:100-106).  Wall clock of run(): scene index pass, streamed unpickling into
    pinned blocks, embedding of both 3-channel planes of every row, shard file, stitch and the output pickle (protocol 5).  frames/s counts
    embedded FRAMES (2 per sample).  The scene is written to a temporary directory first (untimed).  The timed run is repeated `reps` times
    (the output removed in between) and the MEDIAN reported with all samples: one run swung 50-59 k with the leg order in round 4.

    dist (N > 1, round 5): ONE scene, every rank embeds its contiguous row range into its own shard file, rank 0 stitches (the
    host - readers, pinned memory - is what limits this path's scaling); the wall clock is barrier to barrier, MAX over ranks."""
    import contextlib, pickle, shutil, tempfile
    from pvr_habitat_amd import save_embedded_obs as S
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    d = tempfile.mkdtemp(prefix='pvr_e2e_bench_') if rank == 0 else None
    if dist is not None:
        box = [d]
        dist.broadcast_object_list(box, 0)
        d = box[0]

    def barrier():
        if dist is not None:
            dist.barrier()
    try:
        rng = np.random.default_rng(5)
        scene_bytes = 0
        if rank == 0:
            lens = [traj_len] * (n_samples // traj_len) + ([n_samples % traj_len] if n_samples % traj_len else [])
            base = rng.integers(0, 256, (traj_len, hw, hw, 6), dtype=np.uint8)
            raw = dict(obs=[], action=[], reward=[], done=[], true_state=[])
            for t, L in enumerate(lens):
                raw['obs'].append(np.roll(base[:L], t, axis=1))            # distinct trajectories, cheap to make
                raw['action'].append(rng.integers(0, 3, L)); raw['reward'].append(np.zeros(L)); raw['done'].append(np.arange(L) == L - 1)
                raw['true_state'].append(np.zeros((L, 12), np.float32))
            with open(os.path.join(d, 'scene.pickle'), 'wb') as f:
                pickle.dump(raw, f, protocol=pickle.HIGHEST_PROTOCOL)
            scene_bytes = os.path.getsize(os.path.join(d, 'scene.pickle'))
            del raw, base
            wd = os.path.join(d, 'warm'); os.makedirs(wd)
            with open(os.path.join(wd, 'scene.pickle'), 'wb') as f:
                nw = 4 * batch * world
                pickle.dump(dict(obs=[rng.integers(0, 256, (nw, hw, hw, 6), dtype=np.uint8)], action=[np.zeros(nw, np.int64)],
                                 reward=[np.zeros(nw)], done=[np.zeros(nw, bool)], true_state=[np.zeros((nw, 12), np.float32)]), f)
        barrier()
        os.environ.setdefault('PVR_SYNTHETIC_WEIGHTS', '1')
        argv = ['--data_path', d, '--env', 'scene', '--embedding_name', 'resnet50', '--disable_pretrained_embedding', '--source', 'pickle',
                '--embed_batch', str(batch), '--compute_dtype', dtype]
        out = os.path.join(d, 'scene_resnet50.pickle')
        els = []
        with contextlib.redirect_stdout(open(os.devnull, 'w')):
            # warm-up on a tiny scene of the same frame size (library load, plan, first launches, both lanes): not part of the measurement
            S.run(S.make_parser().parse_args(['--data_path', os.path.join(d, 'warm')] + argv[2:]))
            for r_ in range(reps):
                barrier()
                if rank == 0 and os.path.isfile(out):
                    os.remove(out)                          # (run() returns at once when its output exists: save_embedded_obs.py:97-101)
                barrier()
                t0 = time.perf_counter()
                S.run(S.make_parser().parse_args(argv))
                barrier()
                el = time.perf_counter() - t0
                if dist is not None:
                    t = torch.tensor([el], dtype=torch.float64, device='cuda')
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    el = float(t.item())
                els.append(el)
        if rank != 0:
            return None
        with open(out, 'rb') as f:
            res = pickle.load(f)
        assert res['obs'].shape == (n_samples, 2 * 2048) and np.isfinite(res['obs'][:1024]).all() and np.isfinite(res['obs'][-1024:]).all()
        el = sorted(els)[(len(els) - 1) // 2]
        return {'metric': 'frames/sec embedded by save_embedded_obs.run end to end (scene pickle -> embeddings pickle)', 'value': round(2 * n_samples / el, 1),
                'unit': 'frames/s', 'samples': n_samples, 'frames_per_sample': 2, 'frame': hw, 'dtype': dtype, 'wall_s': round(el, 2), 'n_gpus': world,
                'runs_frames_per_s': [round(2 * n_samples / e, 1) for e in els], 'scene_MB': round(scene_bytes / 1e6, 1), 'out_MB': round(os.path.getsize(out) / 1e6, 1),
                'note': 'MEDIAN of %d runs of run(flags), wall clock%s: index pass + streamed unpickle into pinned blocks (reader thread) + H2D + ResNet50 on both planes + D2H + '
                        '%s + output pickle; 64x64 frames are bilinearly resized to 256 on the GPU (Resize(256), embeddings.py:80-85)'
                        % (len(els), '' if world == 1 else ' barrier to barrier, max over ranks', 'rows straight into the output pickle' if world == 1 else
                           'per-rank shard files (contiguous row ranges of the one scene) + rank-0 stitch')}
    finally:
        barrier()
        if rank == 0:
            shutil.rmtree(d, ignore_errors=True)


def uber5crop_bench(batch, dtype, n_frames=2048, frame=256, dist=None, parity=False):
    """BASELINE configs[4]: the paper's best PVR - moco_aug_uber_345 (three separately loaded ResNet50 trunks: l3-compressed, l4-compressed,
    conv5; src/embeddings.py:44-57,195-280) on 5 crop windows per frame (corner + centre, torchvision FiveCrop order: the build-defined
    extension of configs[4]): 15 trunk forwards and 31 310 floats per 256x256 uint8 frame.  `value` follows the headline's rule - frames
    resident in HBM when the timed region starts, two batches in flight, results left in HBM; `streamed` is the PCIe-inclusive rate of the same
    work through stream_embed (pinned host frames -> H2D -> forwards -> D2H, overlapped: "embeddings streamed to host").  Rates against the
    MFMA peak use 115.69 GFLOP per frame.

    dist (N > 1, round 6): configs[4] is "1 M frames sharded across 8 GPUs, embeddings streamed to host" - every rank runs both legs on its own
    frames at the same time (barrier on both sides, no collective inside): aggregate = all ranks' frames / the slowest rank's time, per-rank
    spread beside it; the streamed leg is where N uploads + N result streams share the host.
    parity: also compare 4 frames' 31 310 floats with the fp32 CPU oracle (rank 0 only; three trunks x five windows on the host: ~1 min)."""
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0

    def barrier():
        if dist is not None:
            dist.barrier()
    os.environ.setdefault('PVR_SYNTHETIC_WEIGHTS', '1')
    from pvr_habitat_amd import synth
    from pvr_habitat_amd.embeddings import EmbeddingNet, stream_embed, lane_streams
    net = EmbeddingNet('moco_aug_uber_345', pretrained=False, crops=5, max_batch=batch, compute_dtype=dtype)
    assert net.out_size == 5 * 6262
    n_frames = max(2 * batch, n_frames // batch * batch)
    fr = torch.from_numpy(synth.frames(5 + rank, n_frames, frame, frame)).pin_memory()
    dev = fr.cuda()
    outs = [torch.empty((batch, net.out_size), device='cuda') for _ in range(2)]
    streams = lane_streams()

    def resident():
        for s_ in streams:
            s_.wait_stream(torch.cuda.current_stream())
        for i in range(n_frames // batch):
            with torch.cuda.stream(streams[i & 1]):
                net.embedding.forward_into(dev[i * batch:(i + 1) * batch], outs[i & 1], lane=i & 1)
        torch.cuda.synchronize()

    resident()                                                                   # warm-up (allocations, first-use attributes, both lanes)
    # a pass is four forwards of ~60-70 ms: one pass is a noisy sample (the streamed leg read 2.9 - 3.8 k frames/s on one build over the round's boxes);
    # each rate is the MEDIAN of three passes, every pass between barriers
    els = []
    for _ in range(3):
        barrier()
        t0 = time.perf_counter(); resident(); els.append(time.perf_counter() - t0)
    el_own = sorted(els)[1]
    barrier()
    el_res, el_res_min = rank_spread(dist, el_own)
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    out = torch.empty((n_frames, net.out_size), dtype=torch.float32).pin_memory()
    stream_embed(net, fr[:2 * batch], batch=batch, out=out[:2 * batch])
    els = []
    for _ in range(3):
        torch.cuda.synchronize(); barrier(); t0 = time.perf_counter()
        stream_embed(net, fr, batch=batch, out=out)
        torch.cuda.synchronize(); els.append(time.perf_counter() - t0)
    el_own = sorted(els)[1]
    barrier()
    el, el_min = rank_spread(dist, el_own)
    assert np.isfinite(out.numpy()[::97]).all()
    par = None
    if parity and rank == 0:
        # the timed model against the fp32 CPU oracle: every member (l3 / l4 / conv5 of the same synthetic checkpoints) on every crop window
        from oracle import encoder_oracle as eo
        from pvr_habitat_amd.embeddings import _UBER, _load_named_state_dict, FiveCrop
        torch.set_num_threads(min(len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1), 16))
        k = 4
        got = out.numpy()[:k].astype(np.float64)
        cols = []
        for pos in FiveCrop.ORDER:
            for name in _UBER['moco_aug_uber_345']:
                sd_m, variant = _load_named_state_dict(name, False)
                cols.append(eo.embed(sd_m, fr.numpy()[:k], variant, squeeze=False, crop_pos=pos).astype(np.float64))
        ref = np.concatenate(cols, axis=1)
        par = {'rel_l2': _r(np.linalg.norm(got - ref) / np.linalg.norm(ref)), 'max_norm': _r(np.abs(got - ref).max() / np.abs(ref).max()), 'frames': k,
               'note': 'the streamed rows of this leg vs the fp32 CPU oracle (15 trunk forwards per frame), all %d floats per frame' % ref.shape[1]}
    net.close()
    fps, fps_s = world * n_frames / el_res, world * n_frames / el
    gflop = 5 * 23.138
    res = {'metric': 'frames/sec embedded (5-crop moco_aug_uber_345, 256x256)', 'value': round(fps, 1), 'unit': 'frames/s', 'dtype': dtype,
           'frames': n_frames * world, 'floats_per_frame': int(net.out_size), 'trunk_forwards_per_frame': 15, 'trunk_frames_per_s': round(15 * fps, 1),
           'tflops': round(fps * gflop / 1e3, 1), 'frac_of_mfma_peak': round(fps * gflop / 1e3 / PEAK_BF16_TFLOPS / world, 4),
           'streamed': {'value': round(fps_s, 1), 'unit': 'frames/s', 'd2h_GBps': round(fps_s * net.out_size * 4 / 1e9, 3),
                        'frac_of_mfma_peak': round(fps_s * gflop / 1e3 / PEAK_BF16_TFLOPS / world, 4),
                        'note': 'PCIe-inclusive: pinned host frames -> H2D -> 15 trunk forwards per frame -> D2H of the fp32 rows, stream_embed (two lanes)'},
           'note': 'MEDIAN of three passes (resident and streamed alike); frames resident in HBM, two batches in flight, results left in HBM (the headline\'s rule); algorithmic %.2f GFLOP per frame (5 windows x '
                   '23.138); f16 = the compliant plan: the l3 / l4 members keep an fp32 residual stream and run their last stage and head as fp32 convolutions - '
                   'since round 6 on the 16-bit matrix pipe (conv_split16: exact hi / lo f16 pairs, 3 MFMAs per product), 3x the algorithmic matrix work of '
                   'that stage, not counted in tflops' % gflop}
    if par is not None:
        res['parity'] = par
    if world > 1:
        res.update(n_gpus=world, per_rank_s={'resident': {'min': round(el_res_min, 3), 'max': round(el_res, 3)}, 'streamed': {'min': round(el_min, 3), 'max': round(el, 3)}},
                   scaling_note='all ranks at the same time on their own frames, no collective in the timed regions; rates = all ranks\' frames / the slowest rank\'s time; frac_of_mfma_peak per GPU')
    return res


_ORACLE_REF = {}


def parity_stats(model, sd, frames_np, n_frames=8):
    """the TIMED model (same handle, same dtype) against the CPU oracle on a few frames of the bench's own pool: rel-L2, max|d| / max|ref|,
    and the ELEMENT-WISE relative error |out - ref| / |ref| over the elements with |ref| > 1e-2 max|ref| (below that a post-ReLU average is
    indistinguishable from zero and a relative error means nothing): p50 / p99 / max.  The oracle forward is computed once per run."""
    from oracle import encoder_oracle as eo
    key = (id(sd), n_frames)
    fr = frames_np[:n_frames]
    if key not in _ORACLE_REF:
        torch.set_num_threads(min(len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1), 16))
        _ORACLE_REF[key] = eo.embed(sd, fr, 'conv5', squeeze=False).astype(np.float64)
    ref = _ORACLE_REF[key]
    out = model(torch.from_numpy(fr).cuda()).cpu().numpy().astype(np.float64)
    d = np.abs(out - ref)
    big = np.abs(ref) > 1e-2 * np.abs(ref).max()
    rel = d[big] / np.abs(ref[big])
    return {'rel_l2': float(np.linalg.norm(out - ref) / np.linalg.norm(ref)), 'max_norm': float(d.max() / np.abs(ref).max()),
            'elementwise': {'p50': float(np.percentile(rel, 50)), 'p99': float(np.percentile(rel, 99)), 'max': float(rel.max()),
                            'n_elements': int(big.sum()), 'of': int(ref.size), 'frames': int(len(fr)),
                            'note': '|out - ref| / |ref| over the elements with |ref| > 1e-2 * max|ref|, fp32 CPU oracle'}}


def _r(x, nd=6):
    return float('%.*g' % (nd, x))


DUMP_LIMIT_BYTES = 63 * 10 ** 6                           # all .npy files of --dump-outputs together, headers included, stay under 64 MB


def dump_outputs(dirname, arrays, seed=0):
    """--dump-outputs: DIR/<name>.npy of every array, float32 / float64 as computed.  An array larger than its share of DUMP_LIMIT_BYTES
    keeps a fixed, seeded sample of its rows (in row order), so that two runs with the same arguments write the same elements."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(arrays)) - 4096
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if a.nbytes > share:
            keep = share // (a.nbytes // a.shape[0])
            a = a[np.sort(np.random.default_rng(seed).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a))


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start `python -m torch.distributed.run --nnodes=1 --nproc-per-node N bench.py <same
    arguments>` as a CHILD process (this process has not touched a GPU and never does: no HIP call, no exec after one), let rank 0's single
    JSON line and everything else pass through on the inherited stdout / stderr, and return the child's exit code (3 on a time-out)."""
    import socket
    import subprocess
    with socket.socket() as sk:                            # a free rendezvous port on the loopback interface
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC: RCCL across processes needs it on this driver
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    limit = float(os.environ.get('PVR_BENCH_LAUNCH_TIMEOUT', '3000'))
    proc = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return proc.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        import signal
        print('bench.py: the %d-rank run did not finish within %.0f s; stopping it' % (n, limit), file=sys.stderr, flush=True)
        try:
            os.killpg(proc.pid, signal.SIGKILL)            # exactly the process group started above
        except ProcessLookupError:
            pass
        proc.wait()
        return 3


def finish(line, dist, failed=None):
    """rank 0 (the only rank with a line) prints it; every rank leaves the process group; a failed leg exits non-zero once the line is out"""
    if line is not None:
        print(json.dumps(line), flush=True)
    if dist is not None:
        try:
            dist.destroy_process_group()
        except Exception:
            pass
    if failed is not None:
        sys.exit(3)                                             # the headline line is out; the launcher still sees the failed leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=320, help='timed steps of every embedding leg (each leg is timed once); the default makes the '
                                                             'headline\'s timed region ~1 s and cycles the 4096-frame pool 20 times')
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--frame', type=int, default=256)
    ap.add_argument('--dtype', default='f16', choices=['bf16', 'f16', 'f32'],
                    help='storage / MFMA input type of the headline leg.  f16 (default since round 5) is the product default and the type that meets the '
                         'north-star 1e-3 parity bound; the other 16-bit type (bf16: BASELINE configs[1] names it, 3e-3) runs as a second leg of the SAME length')
    ap.add_argument('--chunk', type=int, default=0)
    ap.add_argument('--lanes', type=int, default=2, help='batches in flight per GPU (1 = strictly one forward at a time)')
    ap.add_argument('--pool', type=int, default=4096, help='distinct frames resident in HBM, cycled batch by batch (SURVEY 8d frame pool)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline leg, run everything else the line can carry: the one-lane leg, the other 16-bit leg, the roofline passes, '
                         'parity against the fp32 CPU oracle, the CPU baseline and the PNG / PCIe / e2e / 5-crop / ViT / BC legs (N = 1), the '
                         'data-parallel finetune leg (N > 1); the --no-* options below leave parts of it out.  Without --full a run does only '
                         'what the headline needs')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-bc', action='store_true', help='skip the BC steps/sec legs')
    ap.add_argument('--no-pcie', action='store_true', help='skip the PCIe-inclusive streaming leg')
    ap.add_argument('--no-png', action='store_true', help='skip the PNG-source leg (writes 12 000 small files to a temporary directory)')
    ap.add_argument('--png-traj', type=int, default=48, help='trajectories (x 250 frames) of the PNG-source leg')
    ap.add_argument('--no-e2e', action='store_true', help='skip the save_embedded_obs end-to-end leg (writes a 2.4 GB synthetic scene pickle to a temporary directory)')
    ap.add_argument('--e2e-samples', type=int, default=100000, help='observations of the end-to-end leg\'s synthetic scene')
    ap.add_argument('--no-vit', action='store_true', help='skip the CLIP ViT legs (BASELINE config 3)')
    ap.add_argument('--no-f16', '--no-alt-dtype', dest='no_f16', action='store_true', help='skip the second 16-bit leg (bf16 beside an f16 headline, f16 beside a bf16 one)')
    ap.add_argument('--no-uber', action='store_true', help='skip the configs[4] leg (5-crop moco_aug_uber_345 streamed to the host)')
    ap.add_argument('--no-dp', action='store_true', help='skip the data-parallel finetune leg (N > 1)')
    ap.add_argument('--no-fuse', action='store_true', help='one launch per convolution (A/B against the fused bottleneck tails)')
    ap.add_argument('--per-op', action='store_true', help='print per-launch ms / TFLOP/s of one chunk to stderr (--full)')
    ap.add_argument('--dump-plan', default='', help='(--full) write the launch plan of the timed model (names in launch order) to this JSON file; '
                    'scripts/pmc_summary.py stores it next to the PMC bytes so that a later run can tell whether they still describe its plan')
    ap.add_argument('--dump-outputs', default='', metavar='DIR',
                    help='after the timed headline leg, write what its last step computed (the fp32 embeddings a caller of forward_into receives) '
                         'to DIR/embeddings.npy (rank 0; at most 64 MB, a fixed seeded row sample beyond that).  The frames and weights are '
                         'seeded, so two builds run with the same arguments can be compared output for output')
    args = ap.parse_args()
    if (args.per_op or args.dump_plan) and not args.full:
        ap.error('--per-op and --dump-plan report on the roofline passes, which only --full runs')

    rank = int(os.environ.get('RANK', 0))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args.gpus))                   # `python bench.py --gpus N` as typed: one rank per GPU under torch.distributed.run
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit('WORLD_SIZE=%d but --gpus %d: launch with torch.distributed.run --nproc-per-node %d' % (world, args.gpus, args.gpus))
    # PVR_BENCH_ONE_GPU=1 (test aid for 1-GPU boxes): every rank on cuda:0 with the gloo backend, to exercise the N > 1 path
    one_gpu = os.environ.get('PVR_BENCH_ONE_GPU', '0') == '1'
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if one_gpu:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=torch.device('cuda', local_rank))

    from pvr_habitat_amd import synth, _lib
    from pvr_habitat_amd.embeddings import HipResNet50
    sd = synth.resnet50_state_dict(1, 'conv5')               # MoCo-v2 encoder_q layout == torchvision resnet50
    n_pool = max(args.batch, args.pool // args.batch * args.batch)
    # each rank owns its own shard of the frame stream (different seed = different frames); the pool is generated once and stays in HBM
    pool_np = synth.frames(1 + rank, n_pool, args.frame, args.frame)
    pool = torch.from_numpy(pool_np).cuda()
    batches = [pool[i:i + args.batch] for i in range(0, n_pool, args.batch)]

    def make_model(dtype, lanes_req):
        model = HipResNet50(sd, 'conv5', compute_dtype=dtype, max_batch=args.batch, chunk=args.chunk)
        if args.no_fuse:
            model.set_fusion(False)
        o_ = torch.empty((args.batch, model.out_size), dtype=torch.float32, device='cuda')
        for lane in range(max(1, min(lanes_req, model.lanes))):      # allocates the lane's workspace (off the timed path)
            model.forward_into(batches[0], o_, lane=lane)
        torch.cuda.synchronize()
        return model

    # Both models exist before either leg is timed and nothing is freed in between (scripts/leg_order_ab.py: a model whose workspace
    # is allocated right after another model's 5 GB workspace was freed ran 14 % slower; scripts/sustained_rate.py: with both
    # resident, ten back-to-back 1 s legs give bf16 80.3 k and f16 79.3 k frames/s, flat).
    models = {args.dtype: make_model(args.dtype, args.lanes)}
    alt = {'f16': 'bf16', 'bf16': 'f16'}.get(args.dtype)        # the other 16-bit storage type, timed at the same length beside the headline
    if args.no_f16 or not args.full:
        alt = None
    if alt:
        models[alt] = make_model(alt, args.lanes)

    # the compute streams of every leg, created once: HIP maps streams onto a few hardware queues in creation order, and two lanes whose
    # streams land on the same hardware queue serialise (a leg on freshly created streams measured the one-lane rate)
    from pvr_habitat_amd.embeddings import lane_streams as _pkg_lane_streams
    lane_streams = _pkg_lane_streams()
    while len(lane_streams) < args.lanes:
        lane_streams.append(torch.cuda.Stream())

    spread = []                                               # (slowest, fastest) rank time of every timed leg, in order

    def embed_leg(dtype, steps, warmup, lanes_req):
        """K full forwards, each of its own batch of the pool, `lanes` of them in flight; barrier + synchronize on both sides."""
        model = models[dtype]
        lanes = max(1, min(lanes_req, model.lanes))
        outs = [torch.empty((args.batch, model.out_size), dtype=torch.float32, device='cuda') for _ in range(lanes)]
        streams = lane_streams[:lanes] if lanes > 1 else [torch.cuda.current_stream()]

        def barrier():
            if dist is not None:
                dist.barrier()
            torch.cuda.synchronize()

        def run_steps(k, first=0):
            for i in range(first, first + k):
                with torch.cuda.stream(streams[i % lanes]):
                    model.forward_into(batches[i % len(batches)], outs[i % lanes], lane=i % lanes)

        torch.cuda.synchronize()                                 # default-stream setup work done before the side streams start
        run_steps(max(warmup, lanes))
        barrier()
        t0 = time.perf_counter()
        run_steps(steps)
        barrier()
        el = time.perf_counter() - t0
        el, el_fastest = rank_spread(dist, el)                   # MAX over ranks is the leg's time; the fastest rank's beside it (stragglers)
        spread.append((el, el_fastest))
        if args.full:
            for o_ in outs:
                assert torch.isfinite(o_).all()
            # the last batch each lane embedded, against a fresh forward of the same frames: what was timed produced these embeddings
            last = [(steps - 1 - j) for j in range(lanes)]
            for j, i in enumerate(last):
                chk = torch.empty_like(outs[0])
                model.forward_into(batches[i % len(batches)], chk, lane=0)
                torch.cuda.synchronize()
                assert torch.equal(chk, outs[i % lanes]), 'lane %d result differs from a sequential forward' % (i % lanes)
        return model, el, lanes, outs[(steps - 1) % lanes]

    # every leg is timed once: exactly `steps` forwards between barrier + synchronize
    model, el, lanes, last_out = embed_leg(args.dtype, args.steps, args.warmup, args.lanes)
    head_spread = spread[:1]                                  # the headline leg's (slowest, fastest) rank pair
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {'embeddings': last_out})
    chunk = args.chunk if args.chunk else args.batch
    line = None
    if rank == 0:
        fps = world * args.steps * args.batch / el
        line = {
            'metric': 'frames/sec embedded (ResNet50, 256x256)', 'value': round(fps, 1), 'unit': 'frames/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(el / args.steps * 1e3, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
            'timed_region_s': round(el, 3),
            'config': {'workload': 'configs[1]: ResNet50 (MoCo-v2 layout) frozen, %dx%d uint8 frames resident in HBM, batch %d/GPU, '
                                   'random-init synthetic weights, %s storage / MFMA inputs with fp32 accumulation%s'
                                   % (args.frame, args.frame, args.batch, args.dtype,
                                      ' (the product default, inside the 1e-3 parity bound; configs[1] names bf16%s)'
                                      % (': the `bf16` leg of the same length is in this line' if alt else '') if args.dtype == 'f16' else ''),
                       'global_batch': world * args.batch, 'frame': args.frame, 'chunk': chunk, 'batches_in_flight': lanes,
                       'frame_pool': '%d distinct frames per GPU resident in HBM, cycled batch by batch (every step embeds a different batch)' % n_pool,
                       'parallelism': 'frame shards, no collective (dp%d)' % world},
            'per_rank_ms_per_step': {'max': round(head_spread[0][0] / args.steps * 1e3, 3), 'min': round(head_spread[0][1] / args.steps * 1e3, 3),
                                     'note': 'slowest / fastest rank of the headline leg; value uses the slowest'},
            'tflops_whole_net': round(fps * GFLOP_PER_FRAME / 1e3, 2),
        }
    if not args.full:
        finish(line, dist)
        return
    # the same leg with ONE batch in flight (the headline keeps `--lanes` batches in flight; the roofline object below is a one-lane measurement)
    el_one = embed_leg(args.dtype, args.steps, 1, 1)[1] if lanes > 1 else el
    # the parity mode at the headline configuration, back to back with the headline leg (all ranks run it: weak scaling)
    leg16 = None
    if alt:
        k16 = args.steps                                      # full length: the two 16-bit types are reported side by side
        m16, el16, l16, _ = embed_leg(alt, k16, args.warmup, args.lanes)
        leg16 = (m16, el16, l16, k16)
    out = torch.empty((args.batch, model.out_size), dtype=torch.float32, device='cuda')
    frames = batches[0]

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # roofline of the dominant kernel family (implicit-GEMM convolutions): HIP events between launches on the launch stream
    cap = 128
    op_ms = (C.c_float * cap)(); op_fl = (C.c_double * cap)(); n_ops = C.c_int32()
    conv_ms, conv_fl, other_ms, bound_ms = 0.0, 0.0, 0.0, 0.0
    plan_names = [nm for nm in model.op_names()]
    # which kernel each entry runs as at this chunk size: entries '(in the run)' have no launch of their own (round 6: layer3.1 .. 3.5 are ONE launch),
    # so the identity of the plan the PMC file is tied to carries the kinds, and launches are counted without them
    plan_kinds = model.kernel_names(chunk) if args.dtype != 'f32' and hasattr(model, 'kernel_names') else [''] * len(plan_names)
    plan_id = ['%s [%s]' % (nm, k) if k in ('bneck_frame(run)', '(in the run)') else nm for nm, k in zip(plan_names, plan_kinds)]
    if args.dump_plan and rank == 0:
        json.dump({'plan_launches': plan_id, 'dtype': args.dtype, 'chunk': chunk}, open(args.dump_plan, 'w'))
    algo_bytes = conv_algorithmic_bytes(chunk, plan_names if args.dtype != 'f32' else None)
    grp = {}                                                 # per ResNet stage: [ms, flops, algorithmic bytes] of its conv launches
    reps = 5
    for r_ in range(reps):
        _lib.check(_lib.lib().pvr_encoder_profile(model._handle, C.c_void_p(batches[r_ % len(batches)].data_ptr()), chunk, args.frame, args.frame,
                                                  C.c_void_p(out.data_ptr()), out.stride(0), _lib.stream_ptr(), op_ms, op_fl,
                                                  cap, C.byref(n_ops)))
        for i in range(n_ops.value):
            if i >= 3 and op_fl[i] > 0:
                conv_ms += op_ms[i]; conv_fl += op_fl[i]
                if args.dtype != 'f32' and i - 3 < len(plan_names):
                    g = grp.setdefault(plan_names[i - 3].split('.')[0], [0.0, 0.0, 0.0])
                    ab = conv_algorithmic_bytes(chunk, [plan_names[i - 3]])
                    g[0] += op_ms[i]; g[1] += op_fl[i]; g[2] += ab
                    # this launch's own lower bound: its FLOPs on the matrix pipe or its algorithmic bytes through HBM, whichever is longer
                    bound_ms += max(op_fl[i] / (PEAK_BF16_TFLOPS * 1e12), ab / 8e12) * 1e3
            else:
                other_ms += op_ms[i]
    # every stage against BOTH roofs: layer1 / layer2 (fused tails, 16-bit NHWC activations) sit on the HBM roof,
    # layer3 / layer4 (deep-K implicit GEMMs) on the MFMA roof
    stages = {k: {'ms': round(v[0] / reps, 3), 'TFLOPs': round(v[1] / (v[0] * 1e-3) / 1e12, 1),
                  'frac_mfma': round(v[1] / (v[0] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 3),
                  'algorithmic_GBps': round(v[2] / (v[0] * 1e-3) / 1e9, 1), 'frac_hbm': round(v[2] / (v[0] * 1e-3) / 8e12, 3)}
              for k, v in sorted(grp.items())}
    n_conv = n_ops.value - 4 - sum(1 for k in plan_kinds if k == '(in the run)')
    traffic, traffic_source = None, None
    tf = os.path.join(ROOT, 'profiles', 'pmc_conv_traffic.json')
    if os.path.isfile(tf) and args.dtype != 'f32':           # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command (bf16 kernels)
        tj = json.load(open(tf))
        if tj.get('plan_launches') == plan_id:
            traffic = round(tj['avg_hbm_bytes_per_launch'])
            traffic_source = 'committed rocprofv3 PMC passes of this command (%s), NOT measured in this run: profiles/pmc_conv_traffic.json' % tj.get('captured', 'round 1 build')
        else:
            # the committed counters describe another plan (different fusions / launch list): a stale number is worse than none
            traffic_source = ('profiles/pmc_conv_traffic.json was captured for a different launch plan (%d launches recorded, %d in this run): '
                              'traffic withheld; re-run the --pmc passes (scripts/pmc_summary.py)' % (len(tj.get('plan_launches') or []), len(plan_id)))
    if args.per_op and rank == 0:
        names = ['preprocess', 'stem', 'maxpool'] + [op for op in model.op_names()] + ['pool/flatten']
        for i in range(n_ops.value):
            tfl = op_fl[i] / (op_ms[i] * 1e-3) / 1e12 if op_ms[i] > 0 else 0.0
            print('%-28s %8.3f ms %8.1f TFLOP/s' % (names[i] if i < len(names) else '?', op_ms[i], tfl), file=sys.stderr)
    # The conv family's time in an UNPERTURBED one-lane forward: two events only (start of the first conv launch, end of the last).  The
    # per-launch pass above puts an event between every two launches; each costs a few microseconds of dispatch serialisation, so its
    # sum overstates the family by ~4 % against rocprofv3's kernel durations (profiles/r04_kernel_stats_lanes1.csv).  The span still
    # contains the real launch-to-launch gaps, so it is an upper bound of the sum of kernel durations.
    span_ms, sp = 0.0, C.c_float()
    first_conv, last_conv = 3, n_ops.value - 2
    for r_ in range(reps + 1):
        _lib.check(_lib.lib().pvr_encoder_profile_span(model._handle, C.c_void_p(batches[r_ % len(batches)].data_ptr()), chunk, args.frame, args.frame,
                                                       C.c_void_p(out.data_ptr()), out.stride(0), _lib.stream_ptr(), first_conv, last_conv, C.byref(sp)))
        if r_ > 0:
            span_ms += sp.value
    events_ms = conv_ms                                     # per-launch event sums (reps forwards), kept for the stage / per-op tables
    conv_ms = span_ms
    achieved = conv_fl / (conv_ms * 1e-3) / 1e12
    peak = PEAK_F32_TFLOPS if args.dtype == 'f32' else PEAK_BF16_TFLOPS
    barrier()

    if rank == 0:
        line.update({
            'one_lane': {'value': round(world * args.steps * args.batch / el_one, 1), 'unit': 'frames/s', 'ms_per_step': round(el_one / args.steps * 1e3, 3),
                         'note': 'the same %d-step leg with one batch in flight per GPU (strictly one forward at a time)' % args.steps},
            'roofline': {'bound': 'mfma', 'achieved': round(achieved, 2), 'peak': peak, 'unit': 'TFLOP/s',
                         'frac': round(achieved / peak, 4), 'traffic': traffic, 'traffic_source': traffic_source,
                         'traffic_note': 'avg HBM bytes per conv launch; algorithmic in+out+residual bytes per launch average %.0f' % (algo_bytes / max(n_conv, 1)),
                         'kernel': '%s (all' % ('conv_f32_kernel' if args.dtype == 'f32' else 'implicit-GEMM conv family: conv_igemm_kernel + conv_pp256_kernel + bottleneck_chain_kernel + chain_wave_kernel + conv_expand_kernel + bneck_frame_kernel + conv_wfrag_kernel') + ' %d conv launches of one %d-frame chunk, HIP events on the launch stream, ONE batch in flight: conv_ms_per_chunk is a one-lane measurement and may exceed ms_per_step, which is timed with %d batches in flight)' % (n_conv, chunk, lanes),
                         'avg_launch_ms': round(conv_ms / reps / max(n_conv, 1), 4),
                         # the whole step against the HBM roof: PMC bytes of the conv launches of one batch / wall time of one step
                         # (with two batches in flight the step is shorter than the sum of its launches)
                         'hbm_step': None if traffic is None else {
                             'achieved': round(traffic * n_conv / (el / args.steps) / 1e9, 1), 'peak': 8000.0, 'unit': 'GB/s',
                             'frac': round(traffic * n_conv / (el / args.steps) / 8e12, 4),
                             'note': 'conv-launch HBM bytes per batch (committed PMC passes) / step time of THIS run'},
                         'conv_ms_per_chunk': round(conv_ms / reps, 3), 'other_ms_per_chunk': round(other_ms / reps, 3),
                         'method': 'conv_ms_per_chunk = HIP-event time from the start of the first to the end of the last conv launch of a one-lane forward that '
                                   'carries only those two events (launch-to-launch gaps included); per_launch_events = the older method, the sum of per-launch '
                                   'durations from a forward with an event between every two launches (stages / --per-op use it)',
                         'per_launch_events': {'conv_ms_per_chunk': round(events_ms / reps, 3), 'frac': round(conv_fl / (events_ms * 1e-3) / 1e12 / peak, 4)},
                         # both roofs at once (extra to the contract's single-roof frac): sum over the conv launches of max(FLOPs / MFMA peak,
                         # algorithmic bytes / 8 TB/s) against the sum of their measured durations - layer1 / layer2 launches are bounded by HBM
                         'two_roof': None if bound_ms == 0.0 else {'bound_ms_per_chunk': round(bound_ms / reps, 3), 'frac': round(bound_ms / conv_ms, 4),
                                                                  'note': 'per launch max(flops / %.0f TFLOP/s, algorithmic bytes / 8 TB/s), summed, / measured conv_ms_per_chunk' % PEAK_BF16_TFLOPS},
                         'stages': stages},
        })
        # parity of what was timed: the same model handle / dtype vs the fp32 CPU oracle (north-star tolerance 1e-3 relative fp32)
        ps = parity_stats(model, sd, pool_np)
        line['parity_rel_l2'] = round(ps['rel_l2'], 6)
        line['parity'] = {args.dtype: {'rel_l2': _r(ps['rel_l2']), 'max_norm': _r(ps['max_norm']), 'elementwise': {k: (_r(v) if isinstance(v, float) else v) for k, v in ps['elementwise'].items()}}}
        line['parity_note'] = ('timed embeddings vs the fp32 CPU oracle on 8 frames of the pool, per storage type: rel-L2, max|d| / max|ref| and the element-wise '
                               'relative error distribution.  North-star bound 1e-3: met by f16 (the product default and, since round 5, the headline); bf16 '
                               'storage (8-bit significand) sits at ~3e-3')
    if leg16 is not None and rank == 0:
        m16, el16, l16, k16 = leg16
        ps16 = parity_stats(m16, sd, pool_np)
        line['parity'][alt] = {'rel_l2': _r(ps16['rel_l2']), 'max_norm': _r(ps16['max_norm']), 'elementwise': {k: (_r(v) if isinstance(v, float) else v) for k, v in ps16['elementwise'].items()}}
        line[alt] = {'metric': 'frames/sec embedded (ResNet50, 256x256), %s storage' % alt, 'value': round(world * k16 * args.batch / el16, 1),
                     'unit': 'frames/s', 'dtype': alt, 'steps': k16, 'ms_per_step': round(el16 / k16 * 1e3, 3), 'batches_in_flight': l16,
                     'timed_region_s': round(el16, 3), 'parity_rel_l2': round(ps16['rel_l2'], 6),
                     'note': 'the same leg as the headline (same steps, same frame pool, same kernels) with the other 16-bit storage type'}
    if rank == 0:
        if world == 1 and not args.no_cpu_baseline:
            line['cpu_baseline'] = cpu_baseline(sd, pool_np[:args.batch])
        if world == 1 and not args.no_png:
            line['png_source'] = png_source_bench(sd, args.batch, args.dtype, n_traj=args.png_traj)
    # The host-fed legs run at every N (round 5): at N > 1 all ranks run them concurrently, so that the line says what the HOST side
    # (pinned-memory bandwidth, staging / reader threads, the file system) does to the scaling of the precompute path - the HBM-resident
    # `value` cannot fail to scale.  A failure here must not cost the headline: it is reported inside the line.
    guard = LegGuard(dist, rank, lambda: line)

    def host_leg(key, fn, limit_s=900.0):
        """N = 1: exceptions propagate.  N > 1: a rank whose leg raises tells the others through the rendezvous store and the whole run ends
        promptly with the line so far + the error (LegGuard) - no rank is left blocked in the leg's collectives."""
        guard.enter(key, limit_s)
        try:
            r = fn()
            if rank == 0 and r is not None:
                line[key] = r
        except Exception as e:                                  # noqa: BLE001
            if world == 1:
                raise
            if rank == 0:
                line[key] = {'error': '%s: %s' % (type(e).__name__, e)}
            guard.failed(key, e)
        finally:
            guard.leave()
    if not args.no_pcie:
        host_leg('pcie_inclusive', lambda: pcie_bench(sd, args.batch, pool_np, args.dtype, dist=dist))
        if rank == 0 and 'pinned_source' in line.get('pcie_inclusive', {}):
            # host uint8 -> H2D -> encode -> D2H fp32, the end-to-end rate of the "embeddings streamed to host" path (never `value`)
            line['value_pcie_inclusive'] = line['pcie_inclusive']['pinned_source']['value']
    if not args.no_e2e and not args.no_pcie:
        host_leg('save_embedded_obs_e2e', lambda: save_obs_e2e_bench(args.batch, args.dtype, n_samples=args.e2e_samples, dist=dist))
    if not args.no_uber:
        # configs[4] at every N (round 6): `value` = the COMPLIANT plan (f16: inside the 1e-3 bound on every member, its parity in the leg), the bf16
        # throughput plan beside it - as the headline does
        def uber_leg():
            r = uber5crop_bench(args.batch, 'f16', n_frames=1024 if world == 1 else 512, dist=dist, parity=(world == 1 and not args.no_cpu_baseline))
            b = uber5crop_bench(args.batch, 'bf16', n_frames=1024 if world == 1 else 512, dist=dist, parity=(world == 1 and not args.no_cpu_baseline))
            if r is not None and b is not None:
                r['bf16_throughput_plan'] = {k: v for k, v in b.items() if k in ('value', 'unit', 'dtype', 'frames', 'trunk_frames_per_s', 'tflops', 'frac_of_mfma_peak', 'streamed', 'parity', 'per_rank_s')}
            return r
        host_leg('uber5crop', uber_leg, limit_s=1500.0)
    if not args.no_vit:
        vdt = 'f16' if args.dtype == 'f32' else args.dtype   # the fp32 mode covers the ResNet50 family only
        vs = lane_streams[:2] if len(lane_streams) >= 2 else None
        host_leg('vit', lambda: [vit_bench('clip_b16', args.batch, 20, 2, vdt, vs, dist=dist)] + ([vit_bench('clip_b32', args.batch, 20, 2, vdt, vs)] if world == 1 else []))
    if rank == 0:
        if world == 1 and not args.no_bc:
            line['bc'] = bc_bench(100, args.warmup, not args.no_cpu_baseline)
            line['bc_finetune'] = finetune_bench(60, args.warmup)
    dp_failed = None
    if world > 1 and not args.no_dp:
        # BASELINE config 4.  A failure or a stuck collective here must not cost the headline line: a watchdog prints it and exits.
        import threading
        done = threading.Event()

        def watchdog():
            if not done.wait(240.0):
                if rank == 0:
                    line['bc_finetune_dp'] = {'error': 'data-parallel leg did not finish within 240 s'}
                    print(json.dumps(line), flush=True)
                os._exit(3)          # non-zero on EVERY rank: a stuck collective is a failed run for the launcher, the headline line is already out
        threading.Thread(target=watchdog, daemon=True).start()
        try:
            res = finetune_dp_bench(dist, 20, 3)
            if rank == 0:
                line['bc_finetune_dp'] = res
        except Exception as e:                                  # noqa: BLE001 - reported in the line; the process still exits non-zero below
            dp_failed = '%s: %s' % (type(e).__name__, e)
            if rank == 0:
                line['bc_finetune_dp'] = {'error': dp_failed}
        done.set()
    guard.close()
    finish(line, dist, dp_failed)


if __name__ == '__main__':
    main()
