"""Step time of end-to-end BC (models.PolicyNetWithEncoder + models.HipJointRMSprop: trainer forward, pvr_policy_backward_dobs, pvr_trainer_backward,
pvr_joint_apply_rmsprop) -> profiles/e2e_bc_step_times.txt: ms per step, frames/s and the share of the policy call, for resnet18 and resnet50 at the
largest unroll_length T <= 100 (resnet50: <= 20) whose T x 16 x 2 frames the trainer admits (no tensor of its workspace above 2 GiB: 668 frames for
resnet18, 334 for resnet50) and the free device memory holds (B = 16, two frames per observation, BatchNorm1d on).

The policy call is bracketed with events by wrapping the ctypes entry; everything else of a step is the encoder's trainer and the joint update.

    python scripts/e2e_bc_step_times.py [--steps 3] [--out profiles/e2e_bc_step_times.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pvr_habitat_amd import synth  # noqa: E402
from pvr_habitat_amd import embeddings as E  # noqa: E402
from pvr_habitat_amd import models as M  # noqa: E402
from pvr_habitat_amd.main_bc_finetune import largest_fitting_frames  # noqa: E402

B, F_ = 16, 2


def one(name, T, steps, lines):
    n = T * B * F_
    need = E.trainer_workspace_bytes(name, n)
    net = E.EmbeddingNet(name, pretrained=False, train=True, max_batch=n)
    model = M.PolicyNetWithEncoder(net, 3, True, num_frames=F_, max_unroll=T, max_batch=B)
    model.train()
    opt = M.HipJointRMSprop(model, lr=1e-4, max_epochs=1000)
    fr = synth.smooth_frames(11, 64, 64, 64)
    obs = torch.from_numpy(fr).cuda()[torch.arange(n, device='cuda') % 64].view(T, B, F_, 64, 64, 3).permute(0, 1, 3, 4, 2, 5).reshape(T, B, 64, 64, 3 * F_)
    done = torch.zeros((T, B), dtype=torch.bool, device='cuda')
    act = torch.randint(0, 3, (T, B), device='cuda')
    L = M._plib()
    inner, pairs = L.pvr_policy_backward_dobs, []

    def timed(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s = inner(*a)
        e1.record()
        pairs.append((e0, e1))
        return s
    opt.scheduler_step()
    loss, norm = opt.step(obs, done, act)                          # warm-up: allocates the workspaces
    torch.cuda.synchronize()
    L.pvr_policy_backward_dobs = timed
    try:
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        for _ in range(steps):
            opt.scheduler_step()
            loss, norm = opt.step(obs, done, act)
        s1.record()
        torch.cuda.synchronize()
    finally:
        L.pvr_policy_backward_dobs = inner
    ms = s0.elapsed_time(s1) / steps
    pol = sum(a.elapsed_time(b) for a, b in pairs) / steps
    lines.append('%-9s T %3d x B %d x %d frames = %4d frames (workspace %.1f GB): %9.2f ms per step, %7.1f frames/s, policy call %7.2f ms = %4.1f %% '
                 '(loss %.4f, gradient norm %.3f)' % (name, T, B, F_, n, need / 2 ** 30, ms, n / ms * 1e3, pol, 100.0 * pol / ms, float(loss), float(norm)))
    model.close()
    del opt, model, net
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'e2e_bc_step_times.txt'))
    a = ap.parse_args()
    lines = ['fused end-to-end BC step (scripts/e2e_bc_step_times.py), %s; eager launches, BatchNorm1d on, 64x64 frames' % torch.cuda.get_device_name(0), '']
    free = int(torch.cuda.mem_get_info()[0] * 0.9)                  # (the policy workspace and the batch live next to the trainer's)
    for name, t_max in (('resnet18', 100), ('resnet50', 20)):
        one(name, largest_fitting_frames(name, t_max * B * F_, free) // (B * F_), a.steps, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
