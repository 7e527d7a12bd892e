"""End-to-end BC of `PolicyNetWithConv` on raw uint8 frames: same `run(flags)` contract, flags, data files and
update rule as reference main_bc_finetune.py:25-242 (model :70, data :102-128, loop :167-208).

Data parallel (BASELINE config 4 / SURVEY 8e; the reference `main` is single-GPU): under an initialised
torch.distributed group every rank draws the SAME `sample_with_minimum_distance` list (same `random.seed(run_id)`),
takes its contiguous slice of the B start indices (the LSTM keeps T whole), runs forward/backward on it, and the
flat 18.1 M-float gradient is averaged in four buckets (RCCL over xGMI with backend "nccl") that leave while backward is still
running (HipRMSprop.step_data_parallel / pvr_policy_set_data_parallel) before the clipped RMSprop update, which is then
identical on every rank.  Launch:
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m pvr_habitat_amd.main_bc_finetune ...
(`__main__` reads RANK / LOCAL_RANK / WORLD_SIZE, picks the GPU and creates the process group before the first GPU call).
`--train_embedding` with a trainable `--embedding_name` selects end-to-end BC instead (`run_end_to_end`: EmbeddingNet(train=True) in front of
PolicyNet, one GPU; `--freeze_embedding_bn [--embedding_chunk N]` trains on the running BatchNorm statistics in passes of N frames, at any T x B).  Interrupted runs resume, completed runs return early (main_bc_finetune.py:47-56,84-89,135-143).  Habitat evaluation needs the
simulator: pass `make_env` as in main_bc_2.run."""
import os
import pickle
import random

import numpy as np
import torch

from .arguments import make_parser
from .models import PolicyNetWithConv, HipRMSprop
from .utils_bc import is_essential_save, sample_with_minimum_distance, shard_bounds
from .test_model import test
from .dist_utils import rank_world, init_distributed, finalize_distributed


def load_raw(flags, from_env):
    """main_bc_finetune.py:102-128: per-scene `<env>.pickle` with lists of per-trajectory arrays."""
    obs = action = reward = done = None
    for env_id in from_env.split(','):
        data = pickle.load(open(os.path.join(flags.data_path, env_id + '.pickle'), 'rb'))
        n = flags.batch_size * flags.unroll_length if flags.debug else len(data['obs'])
        parts = [np.concatenate(data[k][:n]) for k in ('obs', 'action', 'reward', 'done')]
        if obs is None:
            obs, action, reward, done = parts
        else:
            obs, action = np.concatenate((obs, parts[0])), np.concatenate((action, parts[1]))
            reward, done = np.concatenate((reward, parts[2])), np.concatenate((done, parts[3]))
    assert len(obs) == len(action) == len(reward) == len(done), 'data length does not match'
    assert len(reward) > 0, 'no data found'
    return obs, action, reward, done


def largest_fitting_frames(embedding_name, frames_wanted, free_bytes, wgrad_split16=False, conv_split16=False, train_from=None, prefix_once=False,
                           extra_per_frame=0):
    """the largest frame count <= frames_wanted whose training workspace (with fp32 or split-f16 weight gradients / convolutions, training everything
    or from train_from's stage up, in the prefix_once mode or not) fits free_bytes (0: not even one frame).  extra_per_frame: bytes per frame that live
    next to the workspace and grow with it (--embedding_prefix_cache: the staging tensor of a pass)"""
    conv16 = {'conv_split16': True} if conv_split16 else {}
    if train_from is not None:
        conv16['train_from'] = train_from
    if prefix_once:
        conv16['prefix_once'] = True
    from .embeddings import trainer_workspace_bytes
    lo, hi = 0, int(frames_wanted)                              # invariant: lo fits (or is 0), hi + 1 does not
    while lo < hi:
        mid = (lo + hi + 1) // 2
        need = trainer_workspace_bytes(embedding_name, mid, wgrad_split16, **conv16)     # (None: more frames than the trainer's launches can address)
        if need is not None and need + mid * extra_per_frame <= free_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


def check_train_from_flag(flags):
    """--embedding_train_from is a mode of --train_embedding: a ValueError without it (argparse has checked the choices)"""
    stage = getattr(flags, 'embedding_train_from', None)
    if stage is not None and not getattr(flags, 'train_embedding', False):
        raise ValueError('--embedding_train_from %s needs --train_embedding: it chooses the stage a trainable encoder trains from (a frozen encoder '
                         'trains nothing)' % stage)
    return stage


def check_prefix_once_flag(flags):
    """--embedding_prefix_once keeps the frozen prefix's output across the passes of a step: a ValueError without --embedding_train_from"""
    on = bool(getattr(flags, 'embedding_prefix_once', False))
    if on and getattr(flags, 'embedding_train_from', None) is None:
        raise ValueError('--embedding_prefix_once needs --embedding_train_from: with everything training there is no frozen prefix whose output could be '
                         'kept across the passes of a step')
    return on


def check_prefix_cache_flag(flags):
    """--embedding_prefix_cache computes the frozen prefix's output once per dataset frame: a ValueError without --embedding_train_from"""
    on = bool(getattr(flags, 'embedding_prefix_cache', False))
    if on and getattr(flags, 'embedding_train_from', None) is None:
        raise ValueError('--embedding_prefix_cache needs --embedding_train_from: with everything training there is no frozen prefix whose output could be '
                         'computed once per dataset frame')
    return on


def check_random_crop_flag(flags):
    """--embedding_random_crop is a mode of --train_embedding, and not of --embedding_prefix_cache: a ValueError otherwise"""
    on = bool(getattr(flags, 'embedding_random_crop', False))
    if on and not getattr(flags, 'train_embedding', False):
        raise ValueError('--embedding_random_crop needs --train_embedding: it crops a random window per frame in the training steps of a trainable '
                         'encoder (a frozen encoder embeds the centre crop)')
    if on and getattr(flags, 'embedding_prefix_cache', False):
        raise ValueError('--embedding_random_crop with --embedding_prefix_cache: the cache holds the frozen prefix\'s output for ONE window per frame (the '
                         'deterministic centre crop), and a random crop moves the window in every step; --embedding_prefix_once, which keeps the '
                         'prefix\'s output for the frames and windows of one step, is the compatible mode')
    return on


def check_color_jitter_flag(flags):
    """--embedding_color_jitter B C S is a mode of --train_embedding, and not of --embedding_prefix_cache: a ValueError otherwise, and for a negative or
    non-finite strength.  -> the three strengths, or None when the mode is off (no flag, or 0 0 0)"""
    given = getattr(flags, 'embedding_color_jitter', None)
    if given is None:
        return None
    from .embeddings import color_strengths
    try:
        strengths = color_strengths(tuple(given))
    except ValueError as e:
        raise ValueError('--embedding_color_jitter: %s' % e)
    if strengths is not None and not getattr(flags, 'train_embedding', False):
        raise ValueError('--embedding_color_jitter needs --train_embedding: it jitters brightness, contrast and saturation per frame in the training '
                         'steps of a trainable encoder (a frozen encoder embeds the un-jittered centre crop)')
    if strengths is not None and getattr(flags, 'embedding_prefix_cache', False):
        raise ValueError('--embedding_color_jitter with --embedding_prefix_cache: the cache holds the frozen prefix\'s output for ONE image per frame (the '
                         'un-jittered centre crop), and the jitter changes the image in every step; --embedding_prefix_once, which keeps the prefix\'s '
                         'output for the frames and images of one step, is the compatible mode')
    return strengths


def check_random_resized_crop_flag(flags):
    """--embedding_random_resized_crop LO HI is a mode of --train_embedding, and not of --embedding_random_crop or --embedding_prefix_cache: a ValueError
    otherwise, and for a scale that is not finite or not 0 < LO <= HI <= 1.  -> the (lo, hi) scale range, or None when the mode is off (no flag)"""
    given = getattr(flags, 'embedding_random_resized_crop', None)
    if given is None:
        return None
    from .embeddings import crop_scale
    try:
        scale = crop_scale(tuple(given))
    except ValueError as e:
        raise ValueError('--embedding_random_resized_crop: %s' % e)
    if not getattr(flags, 'train_embedding', False):
        raise ValueError('--embedding_random_resized_crop needs --train_embedding: it resizes a random rectangle of every frame to the crop in the '
                         'training steps of a trainable encoder (a frozen encoder embeds the centre crop)')
    if getattr(flags, 'embedding_random_crop', False):
        raise ValueError('--embedding_random_resized_crop with --embedding_random_crop: both choose the frame\'s window - the one moves a 224 x 224 window in '
                         'the frame after Resize(256), the other resizes a random rectangle of the original frame to 224 x 224; give one of the two flags')
    if getattr(flags, 'embedding_prefix_cache', False):
        raise ValueError('--embedding_random_resized_crop with --embedding_prefix_cache: the cache holds the frozen prefix\'s output for ONE window per '
                         'frame (the deterministic centre crop), and the rectangle changes in every step; --embedding_prefix_once, which keeps the '
                         'prefix\'s output for the frames and rectangles of one step, is the compatible mode')
    return scale


def check_gaussian_blur_flags(flags):
    """--embedding_gaussian_blur P LO HI and --embedding_random_grayscale P are modes of --train_embedding, and not of --embedding_prefix_cache: a
    ValueError otherwise, and for a probability outside [0, 1] or a sigma range that is not finite or not 0 < LO <= HI.  -> ((p, lo, hi) or None, p or
    None): None where a mode is off (no flag, or a probability of 0)"""
    from .embeddings import blur_spec, gray_prob
    out = []
    for flag, given, conv in (('--embedding_gaussian_blur', getattr(flags, 'embedding_gaussian_blur', None), lambda v: blur_spec(tuple(v))),
                              ('--embedding_random_grayscale', getattr(flags, 'embedding_random_grayscale', None), gray_prob)):
        if given is None:
            out.append(None)
            continue
        try:
            out.append(conv(given))
        except ValueError as e:
            raise ValueError('%s: %s' % (flag, e))
        if out[-1] is None:                                     # (a probability of 0: off, nothing to refuse)
            continue
        if not getattr(flags, 'train_embedding', False):
            raise ValueError('%s needs --train_embedding: it changes the image of a frame in the training steps of a trainable encoder (a frozen '
                             'encoder embeds the plain centre crop)' % flag)
        if getattr(flags, 'embedding_prefix_cache', False):
            raise ValueError('%s with --embedding_prefix_cache: the cache holds the frozen prefix\'s output for ONE image per frame (the plain centre '
                             'crop), and the mode changes the image in every step; --embedding_prefix_once, which keeps the prefix\'s output for the '
                             'frames and images of one step, is the compatible mode' % flag)
    return tuple(out)


def prefix_cache_bytes(flags, n_dataset_frames):
    """--embedding_prefix_cache: (bytes of the boundary tensors of all n_dataset_frames = samples x frames dataset frames, bytes per frame of a pass's
    staging tensor), both next to the workspace; (0, 0) without the flag"""
    if not getattr(flags, 'embedding_prefix_cache', False):
        return 0, 0
    from .embeddings import trainer_prefix_cache_bytes, trainer_boundary_bytes
    return (trainer_prefix_cache_bytes(flags.embedding_name, flags.embedding_train_from, n_dataset_frames),
            trainer_boundary_bytes(flags.embedding_name, flags.embedding_train_from))


def prefix_cache_does_not_fit(flags, n_dataset_frames, cache, staging, workspace, free):
    """the RuntimeError of a prefix cache that does not fit next to the workspace: both sizes, the free memory and the alternatives"""
    return RuntimeError("--embedding_prefix_cache: the prefix cache of '%s' from %s for %d dataset frames takes %.2f GB, next to it live a pass's "
                        "staging tensor of %.2f GB and the training workspace of %.2f GB; %.2f GB of device memory are free.  Train from a higher "
                        "stage (its boundary tensor is smaller), or use --embedding_prefix_once, which keeps the boundary tensors of one step only"
                        % (flags.embedding_name, flags.embedding_train_from, n_dataset_frames, cache / 2 ** 30, staging / 2 ** 30,
                           workspace / 2 ** 30, free / 2 ** 30))


def boundary_cache_bytes(flags, n_frames):
    """--embedding_prefix_once: bytes of the boundary tensors of a step's n_frames frames, which live next to the workspace (0 without the flag, and
    with --embedding_prefix_cache, which replaces the step-sized cache)"""
    if not getattr(flags, 'embedding_prefix_once', False) or getattr(flags, 'embedding_prefix_cache', False):
        return 0
    from .embeddings import trainer_boundary_bytes
    return int(n_frames) * trainer_boundary_bytes(flags.embedding_name, flags.embedding_train_from)


def workspace_modes(flags):
    """the keywords of trainer_workspace_bytes / largest_fitting_frames behind the weight-gradient mode, from the flags (only what is on)"""
    kw = {'conv_split16': True} if getattr(flags, 'embedding_conv_split16', False) else {}
    if getattr(flags, 'embedding_train_from', None) is not None:  # (a frozen prefix keeps no activations: the workspace shrinks with the stage)
        kw['train_from'] = flags.embedding_train_from
    if check_prefix_once_flag(flags) or check_prefix_cache_flag(flags):             # (with conv_split16 the prefix keeps no pre-BN tensor; the step's boundary cache is counted by the callers)
        kw['prefix_once'] = True
    return kw


def check_workspace_fits(flags, n_frames_per_obs, n_samples=0):
    """The trainer keeps every activation of a step: its workspace grows with unroll_length x batch_size x frames (about 0.03 GB per frame for
    resnet18, 0.14 GB for resnet50: the reference's default T=100, B=32 does not fit an MI355X), and the trainer refuses a frame count at which one of
    its tensors would pass 2 GiB (668 frames for resnet18, 334 for resnet50).  Compared with that limit and the free device memory BEFORE anything
    is allocated, so that the error names a size that fits instead of an allocation failing inside the first step.  --embedding_prefix_cache: the
    boundary tensors of all n_samples x frames dataset frames and the staging tensor of a pass are counted next to the workspace."""
    from .embeddings import trainer_workspace_bytes
    want = flags.unroll_length * flags.batch_size * n_frames_per_obs
    if getattr(flags, 'freeze_embedding_bn', False):
        return check_chunk_fits(flags, want, int(n_samples) * n_frames_per_obs)
    split16 = bool(getattr(flags, 'embedding_wgrad_split16', False))       # (the mode's scale slots and scratch are part of the workspace)
    conv16 = workspace_modes(flags)
    need = trainer_workspace_bytes(flags.embedding_name, want, split16, **conv16)
    free = int(torch.cuda.mem_get_info()[0])
    cache = boundary_cache_bytes(flags, want)     # (--embedding_prefix_once: the step's boundary tensors live next to the workspace)
    pc_cache, pc_frame = prefix_cache_bytes(flags, int(n_samples) * n_frames_per_obs)
    if pc_cache and need is not None and need + pc_cache + want * pc_frame > free:
        raise prefix_cache_does_not_fit(flags, int(n_samples) * n_frames_per_obs, pc_cache, want * pc_frame, need, free)
    cache += pc_cache + want * pc_frame           # (one pass: the staging tensor holds the step's frames)
    if need is not None:
        need += cache
    if need is None or need > free:
        fit = largest_fitting_frames(flags.embedding_name, want, max(free - cache, 0), split16, **conv16)
        why = 'is more than the trainer\'s launches can address (one tensor of its workspace would pass 2 GiB)' if need is None \
            else 'takes %.2f GB%s, %.2f GB of device memory are free' % (need / 2 ** 30, ' (%.2f GB of them the boundary cache of '
                                                                        '--embedding_prefix_once)' % (cache / 2 ** 30) if cache else '', free / 2 ** 30)
        raise RuntimeError("--train_embedding: the training workspace of '%s' for unroll_length %d x batch_size %d x %d frames = %d frames %s; "
                           "the largest unroll_length x batch_size x frames that fits is %d (unroll_length <= %d at this batch_size)"
                           % (flags.embedding_name, flags.unroll_length, flags.batch_size, n_frames_per_obs, want, why, fit,
                              fit // (flags.batch_size * n_frames_per_obs)))
    return need


def check_chunk_fits(flags, want, n_dataset_frames=0):
    """--freeze_embedding_bn: frames are independent and a step of `want` frames runs as passes of --embedding_chunk frames, so it is the CHUNK's
    workspace that has to fit.  Without --embedding_chunk the chunk is the largest frame count <= want that the trainer admits and whose workspace
    fits nine tenths of the free device memory (the policy's workspace, the batch, the embeddings and one pass's gradient live next to it).  A given
    chunk is compared with the free memory and the trainer's limit as it is, and the error names the largest chunk that fits.  The resolved chunk
    is written back to flags.embedding_chunk (a checkpoint's flags carry it); returns the chunk's workspace bytes.  --embedding_prefix_once: the
    boundary tensors of ALL `want` frames of a step live next to the chunk's workspace; the default chunk is the largest one that fits the nine tenths
    together with that cache, `need` includes it and the messages name both sizes.  --embedding_prefix_cache: in its place the boundary tensors of all
    n_dataset_frames dataset frames and the staging tensor of one pass (chunk frames) live next to the chunk's workspace; a cache that does not fit is
    a RuntimeError that names the sizes and the alternatives."""
    from .embeddings import trainer_workspace_bytes
    free = int(torch.cuda.mem_get_info()[0])
    chunk = getattr(flags, 'embedding_chunk', None)
    split16 = bool(getattr(flags, 'embedding_wgrad_split16', False))
    conv16 = workspace_modes(flags)
    cache = boundary_cache_bytes(flags, want)
    with_cache = ' next to the %.2f GB boundary cache of --embedding_prefix_once for %d frames' % (cache / 2 ** 30, want) if cache else ''
    pc_cache, pc_frame = prefix_cache_bytes(flags, n_dataset_frames)
    if pc_cache:
        one = trainer_workspace_bytes(flags.embedding_name, 1 if chunk is None else max(min(int(chunk), want), 1), split16, **conv16)
        frames_of_one = 1 if chunk is None else max(min(int(chunk), want), 1)
        if one is not None and pc_cache + frames_of_one * pc_frame + one > (free // 10 * 9 if chunk is None else free):
            raise prefix_cache_does_not_fit(flags, n_dataset_frames, pc_cache, frames_of_one * pc_frame, one, free)
        cache = pc_cache
        with_cache = ' next to the %.2f GB prefix cache of --embedding_prefix_cache for %d dataset frames' % (cache / 2 ** 30, n_dataset_frames)
    fit_kw = dict(conv16, extra_per_frame=pc_frame) if pc_cache else conv16       # (the staging tensor grows with the chunk)
    if chunk is None:
        chunk = largest_fitting_frames(flags.embedding_name, want, max(free // 10 * 9 - cache, 0), split16, **fit_kw)
        if chunk < 1:
            raise RuntimeError("--train_embedding --freeze_embedding_bn: the training workspace of '%s' for a chunk of one frame takes %.2f GB%s, %.2f GB "
                               "of device memory are free" % (flags.embedding_name, trainer_workspace_bytes(flags.embedding_name, 1, split16, **conv16) / 2 ** 30,
                                                              with_cache, free / 2 ** 30))
    if chunk < 1:
        raise ValueError('--embedding_chunk %d: a pass takes at least one frame' % chunk)
    chunk = min(int(chunk), want)
    need = trainer_workspace_bytes(flags.embedding_name, chunk, split16, **conv16)
    if need is not None:
        need += cache + chunk * pc_frame
    if need is None or need > free:
        fit = largest_fitting_frames(flags.embedding_name, chunk, max(free - cache, 0), split16, **fit_kw)
        why = 'is more than the trainer\'s launches can address (one tensor of its workspace would pass 2 GiB)' if need is None \
            else 'takes %.2f GB%s, %.2f GB of device memory are free' % ((need - cache) / 2 ** 30, with_cache, free / 2 ** 30)
        raise RuntimeError("--train_embedding --freeze_embedding_bn: the training workspace of '%s' for --embedding_chunk %d frames %s; the largest "
                           "--embedding_chunk that fits is %d" % (flags.embedding_name, chunk, why, fit))
    flags.embedding_chunk = chunk
    return need


def run_end_to_end(flags, make_env=None):
    """`--train_embedding`: BASELINE configs[3], the reference's main_bc_finetune with EmbeddingNet(embedding_name, train=True) in front of PolicyNet.
    Same loader, sampler, device gather, stats pickle, resume and early return as `run`; the model is models.PolicyNetWithEncoder and the update is
    models.HipJointRMSprop (four library calls per iteration) or, with --autograd_step, the reference's own lines over both parameter sets."""
    from torch import nn
    from torch.nn import functional as F
    from . import embeddings as E
    from .models import PolicyNetWithEncoder, HipJointRMSprop
    E.require_trainable(flags.embedding_name)                   # NotImplementedError names what is trainable
    train_from = check_train_from_flag(flags)
    if train_from is not None:                                  # the run's first line names the stage
        print('=== Training the embedding from %s up: conv1 / bn1 and the stages below are frozen ===' % train_from)
    prefix_once = check_prefix_once_flag(flags)
    if prefix_once:
        print('  ', 'prefix once: the frozen prefix runs once per frame and step (--embedding_prefix_once)')
    prefix_cache = check_prefix_cache_flag(flags)
    if prefix_cache:
        print('  ', 'prefix cache: the frozen prefix runs once per dataset frame, before training (--embedding_prefix_cache)')
    random_crop = check_random_crop_flag(flags)
    if random_crop:
        print('  ', 'random crop: every frame of a step is cropped at its own random window, seed %d (--embedding_random_crop)' % flags.run_id)
    color_jitter = check_color_jitter_flag(flags)
    if color_jitter is not None:
        print('  ', 'colour jitter: every frame of a step gets its own brightness, contrast and saturation factor, strengths %g %g %g, in a random '
              'order, seed %d (--embedding_color_jitter)' % (color_jitter + (flags.run_id,)))
    rrc_scale = check_random_resized_crop_flag(flags)
    if rrc_scale is not None:
        print('  ', 'random resized crop: every frame of a step is replaced by a random rectangle of itself, %g .. %g of its area and 3/4 .. 4/3 in '
              'aspect ratio, resized to the crop, seed %d (--embedding_random_resized_crop)' % (rrc_scale + (flags.run_id,)))
    blur, gray = check_gaussian_blur_flags(flags)
    if blur is not None:
        print('  ', 'gaussian blur: a frame of a step is blurred with probability %g, 23 x 23 taps, sigma %g .. %g, seed %d '
              '(--embedding_gaussian_blur)' % (blur + (flags.run_id,)))
    if gray is not None:
        print('  ', 'random grayscale: a frame of a step is replaced by its gray values with probability %g, seed %d (--embedding_random_grayscale)'
              % (gray, flags.run_id))
    world = max(rank_world()[1], int(os.environ.get('WORLD_SIZE', '1')))
    if world > 1:
        raise NotImplementedError('--train_embedding with a world size of %d: data-parallel encoder training is not built (the trainable encoder and its '
                                  'BatchNorm statistics are single-GPU); run one process' % world)
    fused = not getattr(flags, 'autograd_step', False)
    if fused and (getattr(flags, 'optimizer', 'rmsprop') == 'adam' or flags.momentum != 0):
        raise NotImplementedError('--train_embedding: the fused joint update is clip + RMSprop with momentum 0 (pvr_joint_apply_rmsprop); '
                                  '--optimizer adam and --momentum != 0 are not built for it (--autograd_step runs torch.optim.RMSprop with momentum)')
    if getattr(flags, 'optimizer', 'rmsprop') == 'adam':
        raise NotImplementedError('--train_embedding --autograd_step runs the reference lines with torch.optim.RMSprop; --optimizer adam is not built here')
    torch.manual_seed(flags.run_id)
    np.random.seed(flags.run_id)
    random.seed(flags.run_id)
    from_env, to_env = flags.env, flags.to_env
    os.makedirs(flags.save_path, exist_ok=True)
    save_path = os.path.join(flags.save_path, from_env + '_em' + flags.embedding_name + '_finetuned_s' + str(flags.run_id) + '_' + to_env)
    resume = False
    if os.path.isfile(save_path + '.pickle'):
        stats = pickle.load(open(save_path + '.pickle', 'rb'))
        if stats[to_env]['frames'][-1] >= flags.max_frames:
            print('   WARNING! This run was already completed. Stopping now.')
            return stats
        resume = os.path.isfile(save_path + '.tar')
    if flags.disable_cuda or not torch.cuda.is_available():
        raise NotImplementedError('--train_embedding needs the GPU: training the embedding on the host backend (disable_cuda) is not built')
    flags.device = torch.device('cuda')
    print('=== Loading trajectories ===')
    obs, action, reward, done = load_raw(flags, from_env)
    n_samples = len(reward)
    print('  ', 'total number of samples', n_samples)
    assert obs.dtype == np.uint8 and obs.ndim == 4 and obs.shape[3] % 3 == 0, 'raw (n, H, W, 3F) uint8 frames expected, got %s %s' % (obs.dtype, obs.shape)
    n_f = obs.shape[3] // 3
    env = None
    n_actions = int(getattr(flags, 'num_actions', 3))
    if make_env is not None:
        flags.env = to_env
        env = make_env(flags, None)
        n_actions = env.gym_env.action_space.n
    assert int(np.min(action)) >= 0 and int(np.max(action)) < n_actions, \
        'actions in the data (%d..%d) do not fit num_actions=%d' % (int(np.min(action)), int(np.max(action)), n_actions)
    T, B = flags.unroll_length, flags.batch_size
    check_workspace_fits(flags, n_f, n_samples)
    split16 = {'wgrad_split16': True} if getattr(flags, 'embedding_wgrad_split16', False) else {}
    if split16:
        print('  ', 'weight gradients: exact-split products on the f16 matrix pipe')
    if getattr(flags, 'embedding_conv_split16', False):
        split16 = dict(split16, conv_split16=True)
        print('  ', 'forward convolutions and data gradients: exact-split products on the f16 matrix pipe')
    if train_from is not None:
        split16 = dict(split16, train_from=train_from)
    if prefix_once:                                             # (the bits are the same with and without it: a resume may change the flag)
        split16 = dict(split16, prefix_once=True)
    if prefix_cache:                                            # (the workspace mode; the bits are the same: a resume may change this flag too)
        split16 = dict(split16, prefix_cache=True)
    if random_crop:                                             # (the parameters do not depend on the mode: a resume may switch it on or off)
        split16 = dict(split16, random_crop=True, crop_seed=flags.run_id)
    if color_jitter is not None:                                # (likewise)
        split16 = dict(split16, color_jitter=color_jitter, color_seed=flags.run_id)
    if rrc_scale is not None:                                   # (likewise)
        split16 = dict(split16, random_resized_crop=rrc_scale, crop_seed=flags.run_id)
    if blur is not None:                                        # (likewise)
        split16 = dict(split16, gaussian_blur=blur, blur_seed=flags.run_id)
    if gray is not None:                                        # (likewise)
        split16 = dict(split16, random_grayscale=gray, blur_seed=flags.run_id)
    if getattr(flags, 'freeze_embedding_bn', False):            # the encoder is sized by the chunk; a step of T x B x frames runs as passes of it
        if not flags.pretrained_embedding:
            print('   WARNING! --freeze_embedding_bn with --disable_pretrained_embedding: a randomly initialised trunk with running statistics 0 / 1 is not normalised.')
        print('  ', 'frozen BatchNorm:', T * B * n_f, 'frames per step in passes of', flags.embedding_chunk)
        net = E.EmbeddingNet(flags.embedding_name, pretrained=flags.pretrained_embedding, train=True, freeze_bn=True, max_batch=flags.embedding_chunk, **split16)
    else:
        net = E.EmbeddingNet(flags.embedding_name, pretrained=flags.pretrained_embedding, train=True, max_batch=T * B * n_f, **split16)
    model = PolicyNetWithEncoder(net, n_actions, flags.batch_norm, num_frames=n_f, max_unroll=T, max_batch=B)
    max_epochs = flags.max_frames // (T * B) + 1
    if fused:
        optimizer = HipJointRMSprop(model, lr=flags.learning_rate, eps=flags.epsilon, alpha=flags.alpha, max_grad_norm=flags.max_grad_norm,
                                    max_epochs=max_epochs)
    else:                                                       # main_bc_2.py:80-90 over both parameter sets
        optimizer = torch.optim.RMSprop(model.parameters(), lr=flags.learning_rate, momentum=flags.momentum, eps=flags.epsilon, alpha=flags.alpha)
        scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda epoch: 1 - epoch / max_epochs)
    stat_keys = ['episode_return', 'episode_success']
    init_frames = 0
    if resume:
        print('=== Resuming previous run ===')
        checkpoint = torch.load(save_path + '.tar', weights_only=False, map_location='cpu')
        saved_from = checkpoint.get('flags', {}).get('embedding_train_from', None)
        if saved_from != train_from:              # (the optimizer state and the schedule belong to the parameters that run trained)
            raise ValueError('--embedding_train_from %s: the checkpoint %s was trained with --embedding_train_from %s; resume with the same stage'
                             % (train_from, save_path + '.tar', saved_from))
        model.load_state_dict(checkpoint['actor_model_state_dict'])
        optimizer.load_state_dict(checkpoint['actor_model_optimizer_state_dict'])
        if fused:
            optimizer.last_epoch = checkpoint['scheduler_state_dict']['last_epoch']
        else:
            scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
        init_frames = stats[to_env]['frames'][-1]
    else:
        stats = {to_env: {**{k: [np.nan] for k in stat_keys}, 'frames': [0], 'training_loss': [np.nan], 'gradient_norm': [np.nan]}}
    print('=== Training policy and embedding ===')
    model.train()
    from .bc_data import DeviceDataset
    dataset = DeviceDataset(obs, action, done, flags.device)
    if prefix_cache:                                            # after a resume's load_state_dict: the cache holds what the loaded prefix computes
        pc = model.build_prefix_cache(dataset.obs)
        print('  ', 'prefix cache: %d frames, %.2f GB, filled in %.2f s (%.0f frames/s)'
              % (pc.n_frames, pc.nbytes / 2 ** 30, pc.fill_seconds, pc.n_frames / max(pc.fill_seconds, 1e-9)))
    for frames in range(init_frames, flags.max_frames, B * T):
        epoch = frames // (B * T)
        model.embedding.crop_call = epoch                       # (--embedding_random_crop, --embedding_color_jitter, --embedding_random_resized_crop, --embedding_gaussian_blur, --embedding_random_grayscale: the iteration names the draw, so a resumed run draws what an uninterrupted one would)
        starting_i = sample_with_minimum_distance(n=n_samples, k=B, d=T)
        if prefix_cache:                                        # (T, B) sample indices: a step reads its frames' boundary tensors, no uint8 frame
            o = dataset.rows(starting_i, T)
            a, d = dataset.action[o], dataset.done[o].bool()
        else:
            o, a, d = dataset.gather(starting_i, T)             # (T, B, H, W, 3F) uint8
        if fused:
            optimizer.scheduler_step()
            loss, gradient_norm = optimizer.step_cached(o, d, a) if prefix_cache else optimizer.step(o, d, a)
        else:                                                   # main_bc_2.py:206-227, as written there
            output, _ = model(dict(obs_rows=o, done=d) if prefix_cache else dict(obs=o, done=d), model.initial_state(batch_size=B))
            loss = F.nll_loss(F.log_softmax(torch.flatten(output['policy_logits'], 0, 1), dim=-1), target=torch.flatten(a, 0, 1).long())
            scheduler.step()
            optimizer.zero_grad()
            loss.backward()
            gradient_norm = 0.
            for p in model.parameters():
                if p.grad is not None and p.requires_grad:
                    gradient_norm += p.grad.detach().data.norm(2).item() ** 2
            gradient_norm = gradient_norm ** 0.5
            nn.utils.clip_grad_norm_(model.parameters(), flags.max_grad_norm)
            optimizer.step()
        if (epoch + 1) % flags.eval_frequency == 0:
            ev = {k: np.nan for k in stat_keys}
            if env is not None and ((flags.essential_save_only and is_essential_save(epoch, max_epochs, flags.eval_frequency))
                                    or not flags.essential_save_only):
                model.eval()                                    # the frozen 'f32' plan of the current encoder parameters + the eval policy
                ep = test(model, env, stat_keys, flags.n_episodes_test)
                model.train()
                ev = {k: float(np.mean(ep[k])) for k in stat_keys}
            for k in stat_keys:
                stats[to_env][k].append(ev[k])
            stats[to_env]['frames'].append(frames)
            stats[to_env]['training_loss'].append(float(loss))              # (synchronises)
            stats[to_env]['gradient_norm'].append(float(gradient_norm))
            model.check_status()
            print('  ', 'frames', frames, 'training loss', float(loss), 'gradient norm', float(gradient_norm))
            if not flags.disable_save:
                pickle.dump(stats, open(save_path + '.pickle', 'wb'), protocol=pickle.HIGHEST_PROTOCOL)
                # (host copies: the encoder's int64 BatchNorm counters are views of its fp32 buffer block, which torch.save refuses as they are)
                torch.save({'actor_model_state_dict': {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                            'actor_model_optimizer_state_dict': optimizer.state_dict(),
                            'scheduler_state_dict': {'last_epoch': optimizer.last_epoch} if fused else scheduler.state_dict(),
                            'flags': {k: v for k, v in vars(flags).items() if k != 'device'}}, save_path + '.tar')
    torch.cuda.synchronize()
    model.check_status()
    model.close()
    if env is not None:
        env.close()
    return stats


def run(flags, make_env=None):
    check_train_from_flag(flags)
    check_prefix_once_flag(flags)
    check_prefix_cache_flag(flags)
    check_random_crop_flag(flags)
    check_color_jitter_flag(flags)
    check_random_resized_crop_flag(flags)
    check_gaussian_blur_flags(flags)
    if getattr(flags, 'train_embedding', False):
        return run_end_to_end(flags, make_env)
    rank, world = rank_world()
    torch.manual_seed(flags.run_id)
    np.random.seed(flags.run_id)
    random.seed(flags.run_id)                                   # identical sampler stream on every rank
    from_env, to_env = flags.env, flags.to_env
    os.makedirs(flags.save_path, exist_ok=True)
    save_path = os.path.join(flags.save_path, from_env + '_emrandom_finetuned_s' + str(flags.run_id) + '_' + to_env)
    # a finished run returns early, an interrupted one resumes (main_bc_finetune.py:47-56); every rank reads the same files
    resume = False
    if os.path.isfile(save_path + '.pickle'):
        stats = pickle.load(open(save_path + '.pickle', 'rb'))
        if stats[to_env]['frames'][-1] >= flags.max_frames:
            print('   WARNING! This run was already completed. Stopping now.')
            return stats
        resume = os.path.isfile(save_path + '.tar')
    flags.device = torch.device('cuda') if torch.cuda.is_available() and not flags.disable_cuda else torch.device('cpu')
    print('=== Loading trajectories ===')
    obs, action, reward, done = load_raw(flags, from_env)
    n_samples = len(reward)
    print('  ', 'total number of samples', n_samples)
    env = None
    if make_env is not None:
        flags.env = to_env
        env = make_env(flags, None)
        obs_shape, n_actions = env.gym_env.observation_space.shape, env.gym_env.action_space.n
    else:
        obs_shape, n_actions = obs.shape[1:], int(getattr(flags, 'num_actions', 3))           # never derived from the data
    # torch's nll_loss raises for a target outside [0, A); the fused loss kernel would only turn it into a NaN loss: check once here
    assert int(np.min(action)) >= 0 and int(np.max(action)) < n_actions, \
        'actions in the data (%d..%d) do not fit num_actions=%d' % (int(np.min(action)), int(np.max(action)), n_actions)
    assert flags.batch_size % world == 0, 'batch_size must divide evenly over the ranks'
    b_lo, b_hi = shard_bounds(flags.batch_size, rank, world)
    actor_model = PolicyNetWithConv(obs_shape, n_actions, flags.batch_norm, max_unroll=flags.unroll_length,
                                    max_batch=b_hi - b_lo).to(device=flags.device)
    max_epochs = flags.max_frames // (flags.unroll_length * flags.batch_size) + 1
    optimizer = HipRMSprop(actor_model, lr=flags.learning_rate, momentum=flags.momentum, eps=flags.epsilon, alpha=flags.alpha,
                           max_grad_norm=flags.max_grad_norm, max_epochs=max_epochs)
    test_model = PolicyNetWithConv(obs_shape, n_actions, flags.batch_norm, max_unroll=1, max_batch=1).to(device=flags.device)
    test_model.eval()
    stat_keys = ['episode_return', 'episode_success']
    init_frames = 0
    if resume:                                                  # (:84-89,135-143) weights, optimizer state and schedule position
        print('=== Resuming previous run ===')
        checkpoint = torch.load(save_path + '.tar', weights_only=False, map_location='cpu')
        actor_model.load_state_dict(checkpoint['actor_model_state_dict'])
        optimizer.load_state_dict(checkpoint['actor_model_optimizer_state_dict'])
        optimizer.last_epoch = checkpoint['scheduler_state_dict']['last_epoch']
        init_frames = stats[to_env]['frames'][-1]                # (the sampler stream restarts from the seed, as in the reference)
    else:
        stats = {to_env: {**{k: [np.nan] for k in stat_keys}, 'frames': [0], 'training_loss': [np.nan], 'gradient_norm': [np.nan]}}
    print('=== Training policy ===')
    actor_model.train()
    from .bc_data import DeviceDataset
    dataset = DeviceDataset(obs, action, done, flags.device)    # raw uint8 frames resident in HBM (24.6 KB per sample)
    for frames in range(init_frames, flags.max_frames, flags.batch_size * flags.unroll_length):
        epoch = frames // (flags.batch_size * flags.unroll_length)
        starting_i = sample_with_minimum_distance(n=n_samples, k=flags.batch_size, d=flags.unroll_length)
        o, a, d = dataset.gather(starting_i[b_lo:b_hi], flags.unroll_length)     # (T, B/world, 64, 64, 6) uint8, this rank's sequences
        optimizer.scheduler_step()
        loss, gradient_norm = optimizer.step_data_parallel(o, d, a)
        if (epoch + 1) % flags.eval_frequency == 0:
            ev = {k: np.nan for k in stat_keys}
            if env is not None and ((flags.essential_save_only and is_essential_save(epoch, max_epochs, flags.eval_frequency))
                                    or not flags.essential_save_only):
                test_model.load_state_dict(actor_model.state_dict())
                ep = test(test_model, env, stat_keys, flags.n_episodes_test)
                ev = {k: float(np.mean(ep[k])) for k in stat_keys}
            for k in stat_keys:
                stats[to_env][k].append(ev[k])
            stats[to_env]['frames'].append(frames)
            stats[to_env]['training_loss'].append(float(loss))              # (synchronises)
            stats[to_env]['gradient_norm'].append(float(gradient_norm))
            actor_model.check_status()
            if rank == 0:
                print('  ', 'frames', frames, 'training loss', float(loss), 'gradient norm', float(gradient_norm))
                if not flags.disable_save:
                    pickle.dump(stats, open(save_path + '.pickle', 'wb'), protocol=pickle.HIGHEST_PROTOCOL)
                    torch.save({'actor_model_state_dict': actor_model.state_dict(),
                                'actor_model_optimizer_state_dict': optimizer.state_dict(),
                                'scheduler_state_dict': {'last_epoch': optimizer.last_epoch},
                                'flags': {k: v for k, v in vars(flags).items() if k != 'device'}}, save_path + '.tar')
    if flags.device.type == 'cuda':
        torch.cuda.synchronize()
    actor_model.check_status()
    actor_model.close()                                         # library handles are freed here, not at garbage-collection time
    test_model.close()
    if env is not None:
        env.close()
    return stats


def main(argv=None):
    flags = make_parser().parse_args(argv)
    init_distributed()                                          # device + process group first, before any GPU call
    try:
        return run(flags)
    finally:
        finalize_distributed()


if __name__ == '__main__':
    main()
