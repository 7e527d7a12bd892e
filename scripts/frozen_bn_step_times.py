"""Step time of end-to-end BC with frozen BatchNorm (EmbeddingNet(..., train=True, freeze_bn=True, max_batch=chunk) + models.HipJointRMSprop) at the
reference's T = 100 -> profiles/frozen_bn_step_times.txt.  B = 16, two frames per observation, BatchNorm1d on, 64x64 frames; resnet50 in passes of
320 frames, resnet18 in passes of 640.  Per trunk, in one session:

  1. the chunked frozen step at T = 100: ms per step (median and spread over --steps steps after a warm-up step), frames/s, workspace, passes;
  2. the batch-statistics step at the largest T it admits - one pass of the same 320 / 640 frames (the cases of profiles/e2e_bc_step_times.txt);
  3. the expected ratio of frames/s, (F + B) / ((2 - 1 / passes) F + B): the chunked step recomputes the forward of every pass but the last.
     F and B are the batch-statistics trainer's forward and backward at the chunk size, timed with one event pair each;
  4. the per-launch times of a pass in both modes (pvr_trainer_debug_set_timing), summed per group, and layer1's 256-channel bn3 launches - the
     largest shape of the two new kernels - next to their byte floor (tensors streamed x bytes / 6.0 TB/s, the in-order HBM sweep rate).

    python scripts/frozen_bn_step_times.py [--steps 5] [--T 100] [--only resnet50] [--out profiles/frozen_bn_step_times.txt]

--wgrad_split16 measures item 1 alone, with the fp32 and with the split-f16 weight gradients (pvr_trainer_set_wgrad_split16) in the same process, and
APPENDS the lines to --out (default profiles/wgrad_split16_times.txt, next to the per-launch figures of scripts/train_step_times.py --wgrad_split16).
--conv_split16 measures item 1 in four modes - fp32, split-f16 weight gradients, split-f16 convolutions and data gradients
(pvr_trainer_set_conv_split16), both - and APPENDS to --out (default profiles/conv_split16_times.txt).
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
HBM_STREAM = 6.0e12                                            # bytes/s: a 1.2 GB table swept in order


def batch(T):
    n = T * B * F_
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()
    obs = fr[torch.arange(n, device='cuda') % 64].view(T, B, F_, 64, 64, 3).permute(0, 1, 3, 4, 2, 5).reshape(T, B, 64, 64, 3 * F_)
    return obs.contiguous(), torch.zeros((T, B), dtype=torch.bool, device='cuda'), torch.randint(0, 3, (T, B), device='cuda')


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def spread(ms):
    return '%9.2f ms median (min %.2f, max %.2f, %d steps)' % (statistics.median(ms), min(ms), max(ms), len(ms))


def step_times(name, T, chunk, freeze, steps, split16=False, conv16=False):
    """-> (per-step ms list, workspace bytes, passes, loss, norm) of the fused step"""
    n = T * B * F_
    net = E.EmbeddingNet(name, pretrained=False, train=True, freeze_bn=freeze, max_batch=chunk, **({'wgrad_split16': True} if split16 else {}),
                         **({'conv_split16': True} if conv16 else {}))
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    obs, done, act = batch(T)
    res = []

    def one():
        opt.scheduler_step()
        res[:] = opt.step(obs, done, act)
    one()                                                      # warm-up: allocates the workspaces
    torch.cuda.synchronize()
    ms = timed(one, steps)
    out = (ms, net.embedding.workspace_bytes(), len(net.embedding._passes(n)), float(res[0]), float(res[1]))
    model.close()
    del opt, model, net
    torch.cuda.empty_cache()
    return out


def launches(handle):
    L, out, i = _lib.lib(), [], 0
    name, ms, fl = C.create_string_buffer(128), C.c_float(), C.c_double()
    while L.pvr_trainer_launch_time(handle, i, name, 128, C.byref(ms), C.byref(fl)) > 0:
        out.append((name.value.decode(), ms.value))
        i += 1
    return out


def kind(n):
    last = n.split()[-1]
    if last in ('wgrad', 'dgrad', 'pack'):
        return last
    if last == 'bwd':
        return 'pool bwd' if 'pool' in n else 'bn bwd'
    return 'bn' if ('bn' in n or 'downsample.1' in n) else 'conv / other'


def pass_times(name, chunk, freeze, reps=3):
    """one trainer pass of `chunk` frames -> (forward ms, backward ms, per-launch rows of a forward + backward)"""
    sd, variant = E._load_named_state_dict(name, False)
    m = E.HipTrainableResNet(sd, variant, max_batch=chunk, freeze_bn=freeze)
    m.train()
    fr = torch.from_numpy(synth.smooth_frames(11, 64, 64, 64)).cuda()[torch.arange(chunk, device='cuda') % 64].contiguous()
    dout = torch.randn((chunk, m.out_size), device='cuda') / chunk
    g = torch.empty_like(m._flat)
    m._forward_raw(fr)
    m._backward_raw(fr, dout, g)
    torch.cuda.synchronize()
    fwd, bwd = [], []
    for _ in range(reps):
        fwd += timed(lambda: m._forward_raw(fr), 1)
        bwd += timed(lambda: m._backward_raw(fr, dout, g), 1)
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
    m._forward_raw(fr)
    m._backward_raw(fr, dout, g)
    torch.cuda.synchronize()
    rows = launches(m._handle)
    _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 0))
    del m
    torch.cuda.empty_cache()
    return statistics.median(fwd), statistics.median(bwd), rows


def one(name, T, chunk, steps, lines):
    n = T * B * F_
    lines.append('== %s, frozen BatchNorm, T %d x B %d x %d frames = %d frames per step in passes of %d ==' % (name, T, B, F_, n, chunk))
    ms, ws, passes, loss, norm = step_times(name, T, chunk, True, steps)
    med = statistics.median(ms)
    fps_frozen = n / med * 1e3
    lines.append('1. frozen, chunked   %s, %7.1f frames/s, workspace %.1f GB, %d passes (loss %.4f, gradient norm %.3f)'
                 % (spread(ms), fps_frozen, ws / 2 ** 30, passes, loss, norm))
    t_parent = chunk // (B * F_)
    ms, ws, _, loss, norm = step_times(name, t_parent, chunk, False, steps)
    fps_parent = chunk / statistics.median(ms) * 1e3
    lines.append('2. batch statistics  %s, %7.1f frames/s, workspace %.1f GB, one pass of T %d x B %d x %d = %d frames (the largest this mode admits; '
                 'loss %.4f, gradient norm %.3f)' % (spread(ms), fps_parent, ws / 2 ** 30, t_parent, B, F_, chunk, loss, norm))
    f_b, b_b, rows_b = pass_times(name, chunk, False)
    f_f, b_f, rows_f = pass_times(name, chunk, True)
    expected = (f_b + b_b) / ((2 - 1.0 / passes) * f_b + b_b)
    measured = fps_frozen / fps_parent
    lines.append('3. trainer pass of %d frames: batch statistics forward %.2f ms, backward %.2f ms; frozen forward %.2f ms, backward %.2f ms' % (chunk, f_b, b_b, f_f, b_f))
    lines.append('   frames/s frozen / batch statistics: measured %.3f, expected (F + B) / ((2 - 1/passes) F + B) = %.3f with the batch-statistics F and B '
                 '(measured / expected %.3f); with the frozen F and B the same formula against the batch-statistics pass gives %.3f'
                 % (measured, expected, measured / expected, (f_b + b_b) / ((2 - 1.0 / passes) * f_f + b_f)))
    lines.append('4. per-launch times of one pass of %d frames, summed per group (ms; event pairs around every launch):' % chunk)
    lines.append('   %-14s %16s %16s' % ('group', 'batch statistics', 'frozen'))
    groups = {}
    for col, rows in enumerate((rows_b, rows_f)):
        for nme, t in rows:
            groups.setdefault(kind(nme), [0.0, 0.0])[col] += t
    for k, (a, b) in sorted(groups.items(), key=lambda kv: -kv[1][0]):
        lines.append('   %-14s %16.3f %16.3f' % (k, a, b))
    if name == 'resnet50':
        per = chunk * 56 * 56 * 256 * 4
        tb, tf = dict(rows_b), dict(rows_f)
        lines.append('   layer1 bn3 (rows %d x 256 channels, %.2f GB per tensor; floor = tensors streamed x bytes / 6.0 TB/s):' % (chunk * 56 * 56, per / 1e9))
        # forward: z, residual -> y.  backward: z, y, dy -> dz, dres; dres of layer1.0 (the downsample's dy) is written, of layer1.1 / .2 it is
        # written too (the block input's gradient receives the residual branch first) - 5 tensors
        for blk in ('layer1.0', 'layer1.1', 'layer1.2'):
            for suffix, tensors in (('bn3', 3), ('bn3 bwd', 5)):
                k = '%s.%s' % (blk, suffix)
                floor = tensors * per / HBM_STREAM * 1e3
                lines.append('   %-18s batch statistics %7.3f ms, frozen %7.3f ms, floor %6.3f ms (%d tensors): frozen = %.2f x floor'
                             % (k, tb[k], tf[k], floor, tensors, tf[k] / floor))
    lines.append('')


def split16_compare(name, T, chunk, steps, lines):
    n = T * B * F_
    lines.append('== %s, frozen BatchNorm, fused step, T %d x B %d x %d frames = %d frames per step in passes of %d ==' % (name, T, B, F_, n, chunk))
    med = {}
    for split16 in (False, True):
        ms, ws, passes, loss, norm = step_times(name, T, chunk, True, steps, split16)
        med[split16] = statistics.median(ms)
        lines.append('%-24s %s, %7.1f frames/s, workspace %.2f GB, %d passes (loss %.4f, gradient norm %.3f)'
                     % ('split-f16 weight gradients' if split16 else 'fp32 weight gradients', spread(ms), n / med[split16] * 1e3, ws / 2 ** 30, passes, loss, norm))
    lines.append('step time fp32 / split-f16: %.2fx' % (med[False] / med[True]))
    lines.append('')


def conv16_compare(name, T, chunk, steps, lines):
    n = T * B * F_
    lines.append('== %s, frozen BatchNorm, fused step, T %d x B %d x %d frames = %d frames per step in passes of %d ==' % (name, T, B, F_, n, chunk))
    med = {}
    for conv16, split16 in ((False, False), (False, True), (True, False), (True, True)):
        ms, ws, passes, loss, norm = step_times(name, T, chunk, True, steps, split16, conv16)
        med[(conv16, split16)] = statistics.median(ms)
        what = '%s convolutions and data gradients, %s weight gradients' % ('split-f16' if conv16 else 'fp32', 'split-f16' if split16 else 'fp32')
        lines.append('%-72s %s, %7.1f frames/s, workspace %.2f GB, %d passes (loss %.4f, gradient norm %.3f)'
                     % (what, spread(ms), n / med[(conv16, split16)] * 1e3, ws / 2 ** 30, passes, loss, norm))
    lines.append('step time fp32 / split-f16 convolutions: %.2fx with fp32 weight gradients, %.2fx with split-f16 weight gradients; all fp32 / all split-f16 %.2fx'
                 % (med[(False, False)] / med[(True, False)], med[(False, True)] / med[(True, True)], med[(False, False)] / med[(True, True)]))
    lines.append('')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--T', type=int, default=100)
    ap.add_argument('--only', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wgrad_split16', action='store_true', help='the chunked frozen step with fp32 and with split-f16 weight gradients; appends to --out')
    ap.add_argument('--conv_split16', action='store_true', help='the chunked frozen step in the four combinations of the two split modes; appends to --out')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'conv_split16_times.txt' if a.conv_split16 else 'wgrad_split16_times.txt' if a.wgrad_split16
                             else 'frozen_bn_step_times.txt')
    if a.wgrad_split16 or a.conv_split16:
        lines = ['fused end-to-end BC step with frozen BatchNorm (scripts/frozen_bn_step_times.py --%s), %s; one process, a warm-up step, then '
                 '--steps timed steps per mode' % ('conv_split16' if a.conv_split16 else 'wgrad_split16', torch.cuda.get_device_name(0)), '']
        for name, chunk in (('resnet50', 320), ('resnet18', 640)):
            if a.only in (None, name):
                (conv16_compare if a.conv_split16 else split16_compare)(name, a.T, chunk, a.steps, lines)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')
        print('\n'.join(lines))
        return
    lines = ['fused end-to-end BC step with frozen BatchNorm (scripts/frozen_bn_step_times.py), %s; eager launches, BatchNorm1d on, 64x64 frames'
             % torch.cuda.get_device_name(0),
             'one session, one process: both BatchNorm modes of the same build, measured when the frozen mode was added; a warm-up step, then --steps timed steps', '']
    for name, chunk in (('resnet50', 320), ('resnet18', 640)):
        if a.only in (None, name):
            one(name, a.T, chunk, a.steps, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
