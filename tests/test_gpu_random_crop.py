"""The random_crop mode on the GPU (pvr_trainer_forward_windows; HipTrainableResNet(..., random_crop=True, crop_seed=...); HipJointRMSprop;
--embedding_random_crop): resnet18 with the synthetic weights of the other trainer tests.

The oracle is equality of bits with the centre-crop path on host-shifted frames.  A 256 x 256 frame is not resized and its centre window is
[16:240, 16:240], so frame F at window (t, l) is, bit for bit, the frame G at the centre window with G[16:240, 16:240] = F[t:t+224, l:l+224] and the
rest of G arbitrary (random bytes here).  The windows of a step are predicted with E.crop_windows(crop_seed, call, n, 32, 32)."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

import policy_dobs_refs as R
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SEED = 9
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(n):
    """(weights, n 256 x 256 frames, d(loss)/d(embeddings)): once per n"""
    if n not in _cache:
        dout = torch.randn((n, E.OUT_SIZE['r18']), generator=torch.Generator().manual_seed(17)) / n
        _cache[n] = (synth.resnet50_state_dict(3, 'r18'), synth.smooth_frames(11, n, 256, 256), dout)
    return _cache[n]


def _shift(frames, windows, seed=23):
    """G with G[i, 16:240, 16:240] = frames[i, t:t+224, l:l+224] and random bytes around it"""
    g = np.random.default_rng(seed).integers(0, 256, frames.shape, dtype=np.uint8)
    for i, (t, l) in enumerate(np.asarray(windows).tolist()):
        g[i, 16:240, 16:240] = frames[i, t:t + 224, l:l + 224]
    return g


def _model(sd, max_batch, **modes):
    m = E.HipTrainableResNet(sd, 'r18', max_batch=max_batch, **modes)
    m.train()
    for p in m.trained_parameters():
        p.requires_grad = True
    return m


def _step(m, frames, dout):
    """one autograd forward + backward -> (embeddings, {parameter: gradient or None}, {BatchNorm buffer: value}) on the host"""
    out = m(torch.from_numpy(frames).cuda())
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()}
    return out.detach().cpu(), grads, {k: v.detach().cpu().clone() for k, v in m.named_buffers()}


def _same(a, b):
    """every embedding, gradient and buffer of two steps in every bit"""
    if not torch.equal(a[0], b[0]):
        return 'embeddings'
    for what in (1, 2):
        assert sorted(a[what]) == sorted(b[what])
        for k in a[what]:
            x, y = a[what][k], b[what][k]
            if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
                return k
    return None


def _launches(m):
    L = _lib.lib()
    names, buf = [], C.create_string_buffer(128)
    while L.pvr_trainer_launch_time(m._handle, len(names), buf, 128, None, None):
        names.append(buf.value.decode())
    return names


# ------------------------------------------------------------------------------------------------------------------
# batch statistics: 4 frames, one pass
# ------------------------------------------------------------------------------------------------------------------
def test_batch_statistics_step_is_the_centre_crop_step_on_shifted_frames():
    sd, frames, dout = _inputs(4)
    win = E.crop_windows(SEED, 0, 4, 32, 32)
    assert not (win == 16).all() and len({tuple(w) for w in win.tolist()}) > 1          # (16, 16) everywhere would make the comparison vacuous
    m = _model(sd, 4, random_crop=True, crop_seed=SEED)
    assert m.random_crop and m.crop_seed == SEED and m.crop_call == 0 and m.crop_range(256, 256) == (32, 32) and m.crop_range(96, 72) == (117, 32)
    on = _step(m, frames, dout)
    assert m.crop_call == 1 and m._windows is None             # the node took the windows and released them after its backward
    shifted = _step(_model(sd, 4), _shift(frames, win), dout)
    centre = _step(_model(sd, 4), frames, dout)
    assert all(g is not None for g in on[1].values()) and bool(torch.isfinite(on[0]).all())
    assert 'bn1.running_mean' in on[2] and 'layer4.1.bn2.num_batches_tracked' in on[2] and int(on[2]['bn1.num_batches_tracked']) == 1
    assert _same(on, shifted) is None, _same(on, shifted)
    assert not torch.equal(on[0], centre[0]) and not torch.equal(on[1]['conv1.weight'], centre[1]['conv1.weight'])
    assert not torch.equal(on[2]['bn1.running_mean'], centre[2]['bn1.running_mean'])
    # the next forward draws call 1 (batch statistics: the embeddings do not depend on the running statistics the first step moved)
    out2 = m(torch.from_numpy(frames).cuda()).detach().cpu()
    ref_out2 = _model(sd, 4)(torch.from_numpy(_shift(frames, E.crop_windows(SEED, 1, 4, 32, 32))).cuda()).detach().cpu()
    assert m.crop_call == 2 and torch.equal(out2, ref_out2) and not torch.equal(out2, on[0])


# ------------------------------------------------------------------------------------------------------------------
# frozen BatchNorm, chunked: 5 frames in passes of 2, 2, 1; the backward recomputes two passes
# ------------------------------------------------------------------------------------------------------------------
CHUNKED = {'fp32': {}, 'both_split16': {'conv_split16': True, 'wgrad_split16': True}, 'layer3': {'train_from': 'layer3'},
           'layer3_prefix_once': {'train_from': 'layer3', 'prefix_once': True}}


def _chunked(name, random_crop):
    key = ('chunked', name, random_crop)
    if key not in _cache:
        sd, frames, dout = _inputs(5)
        win = E.crop_windows(SEED, 0, 5, 32, 32)
        m = _model(sd, 2, freeze_bn=True, **dict(CHUNKED[name], **({'random_crop': True, 'crop_seed': SEED} if random_crop else {})))
        assert len(m._passes(5)) == 3
        _cache[key] = _step(m, frames if random_crop else _shift(frames, win), dout)
        assert m.crop_call == (1 if random_crop else 0)
    return _cache[key]


@pytest.mark.parametrize('name', ['fp32', 'both_split16', 'layer3_prefix_once'])
def test_chunked_frozen_bn_step_is_the_centre_crop_step_on_shifted_frames(name):
    sd, frames, dout = _inputs(5)
    win = E.crop_windows(SEED, 0, 5, 32, 32)
    assert not (win == 16).all() and not np.array_equal(win[:2], win[2:4])            # the passes crop at different windows
    on, shifted = _chunked(name, True), _chunked(name, False)
    assert _same(on, shifted) is None, _same(on, shifted)
    trained = [k for k, g in on[1].items() if g is not None]
    assert ('conv1.weight' in trained) == ('train_from' not in CHUNKED[name]) and 'layer3.0.conv1.weight' in trained
    assert all(float(on[1][k].abs().sum()) > 0 for k in trained)
    sd_centre = _step(_model(sd, 2, freeze_bn=True, **CHUNKED[name]), frames, dout)
    assert not torch.equal(on[0], sd_centre[0])                # and not the centre crop of the frames themselves


def test_prefix_once_keeps_the_bits_of_the_mode_without_it():
    """with prefix_once the recompute passes start at the boundary tensor, without it they run the stem again at the same windows: the same bits"""
    a, b = _chunked('layer3_prefix_once', True), _chunked('layer3', True)
    assert _same(a, b) is None, _same(a, b)


# ------------------------------------------------------------------------------------------------------------------
# the joint step
# ------------------------------------------------------------------------------------------------------------------
def test_two_joint_steps_are_the_centre_crop_steps_on_shifted_observations():
    T, B, F_ = 2, 2, 2
    n = T * B * F_
    obs, done, act = R.chain_inputs(13, T, B, F_, hw=256)
    frames = obs.reshape(T * B, 256, 256, F_, 3).transpose(0, 3, 1, 2, 4).reshape(n, 256, 256, 3)        # split_frames' (observation, frame) order
    to_obs = lambda fr: np.ascontiguousarray(fr.reshape(T, B, F_, 256, 256, 3).transpose(0, 1, 3, 4, 2, 5).reshape(T, B, 256, 256, 3 * F_))
    assert np.array_equal(to_obs(frames), obs)
    d, a = done.cuda(), act.cuda()
    runs = []
    for random_crop in (True, False):
        enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], 1)
        enc = _model(enc_sd, n, **({'random_crop': True, 'crop_seed': SEED} if random_crop else {}))
        enc.crop_call = 5                                      # a caller's own call number, as the driver sets it
        m = M.PolicyNetWithEncoder(enc, R.A, True, num_frames=F_, max_unroll=T, max_batch=B)
        m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
        m.train()
        opt = M.HipJointRMSprop(m, lr=1e-3)
        assert torch.equal(m.split_frames(torch.from_numpy(obs).cuda()).cpu(), torch.from_numpy(frames))
        per_step = []
        for k in range(2):
            win = E.crop_windows(SEED, 5 + k, n, 32, 32)
            assert not (win == 16).all() and not np.array_equal(win[0::2], win[1::2])  # the two frames of an observation: independent windows
            o = torch.from_numpy(obs if random_crop else to_obs(_shift(frames, win))).cuda()
            loss, norm = opt.step(o, d, a)
            torch.cuda.synchronize()
            per_step.append((float(loss), float(norm), enc._flat.clone(), enc._bufs.clone(), m.policy._flat.clone()))
            assert np.isfinite(per_step[-1][0]) and np.isfinite(per_step[-1][1])
        assert enc.crop_call == (7 if random_crop else 5) and enc._windows is None
        runs.append(per_step)
        m.close()
    for k, (on, off) in enumerate(zip(*runs)):
        assert on[:2] == off[:2], (k, on[:2], off[:2])
        assert all(torch.equal(x, y) for x, y in zip(on[2:], off[2:])), k
    assert not torch.equal(runs[0][0][2], runs[0][1][2])       # and the steps moved the encoder


# ------------------------------------------------------------------------------------------------------------------
# the entry point without windows; the launch names; eval mode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [256, 64], ids=['no_resize', 'x4_upscale'])
def test_forward_windows_without_windows_is_forward_and_with_them_one_launch_replaces_two(hw):
    L = _lib.lib()
    sd, frames, dout = _inputs(4)
    fr = torch.from_numpy(frames if hw == 256 else synth.smooth_frames(11, 4, hw, hw)).cuda()
    results = {}
    for how in ('forward', 'null_windows', 'windows'):
        m = _model(sd, 4)
        _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
        out = torch.full((4, m.out_size), float('nan'), device='cuda')
        win = torch.from_numpy(np.tile(np.array([[16, 16]], np.int32), (4, 1))).cuda()       # the centre window, as windows
        if how == 'forward':
            _lib.check(L.pvr_trainer_forward(m._handle, vp(m._flat), vp(m._bufs), vp(fr), 4, hw, hw, vp(out), out.stride(0), _lib.stream_ptr()))
        else:
            _lib.check(L.pvr_trainer_forward_windows(m._handle, vp(m._flat), vp(m._bufs), vp(fr), 4, hw, hw, vp(win) if how == 'windows' else None, None, 0,
                                                     vp(out), out.stride(0), _lib.stream_ptr()))
        names = _launches(m)
        g = torch.empty_like(m._flat)
        dd = dout.cuda()
        _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()))
        torch.cuda.synchronize()
        results[how] = (names, out.cpu(), g.cpu(), m._bufs.cpu())
    a, b, c = results['forward'], results['null_windows'], results['windows']
    assert a[0][:3] == ['preprocess', 'normalize', 'conv1 pack'] and b[0] == a[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert c[0] == ['preprocess windows'] + a[0][2:] and 'preprocess' not in c[0] and 'normalize' not in c[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))        # the centre window through the one launch: the two launches' bits
    assert bool(torch.isfinite(a[1]).all()) and float(a[2].abs().sum()) > 0


def test_eval_mode_is_the_eval_mode_of_the_encoder_without_the_mode():
    sd, frames, _ = _inputs(4)
    fr = torch.from_numpy(frames).cuda()
    outs = []
    for modes in ({'random_crop': True, 'crop_seed': SEED}, {}):
        m = _model(sd, 4, **modes)
        m.eval()
        outs.append(m(fr).cpu())
        assert m.crop_call == 0
        m.close()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_the_cache_entry_points_refuse_the_mode():
    sd, frames, _ = _inputs(4)
    m = _model(sd, 2, freeze_bn=True, train_from='layer3', prefix_once=True, random_crop=True)
    with pytest.raises(ValueError, match='random_crop with build_prefix_cache.*ONE window per frame.*prefix_once'):
        m.build_prefix_cache(torch.from_numpy(frames).cuda())
    with pytest.raises(ValueError, match='random_crop with forward_cached.*ONE window per frame.*prefix_once'):
        m.forward_cached(None, None)
    with pytest.raises(ValueError, match='random_crop with prefix_cache'):
        E.HipTrainableResNet(sd, 'r18', max_batch=2, train_from='layer3', prefix_cache=True, random_crop=True)


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
T_, B_ = 3, 2


def _scene(tmp_path, n=40):
    fr = synth.smooth_frames(7, 2 * n, 64, 64).reshape(n, 2, 64, 64, 3).transpose(0, 2, 3, 1, 4).reshape(n, 64, 64, 6)
    rng = np.random.default_rng(0)
    raw = dict(obs=[np.ascontiguousarray(fr)], action=[rng.integers(0, 3, n)], reward=[np.zeros(n, np.float32)], done=[np.eye(1, n, n - 1, dtype=bool)[0]],
               true_state=[np.zeros((n, 12), np.float32)])
    pickle.dump(raw, open(tmp_path / 'scene.pickle', 'wb'))


def _args(tmp_path, save, max_frames, *extra):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / save), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--embedding_name', 'resnet18', '--disable_pretrained_embedding', '--unroll_length', str(T_),
                                     '--batch_size', str(B_), '--eval_frequency', '1', '--max_frames', str(max_frames)] + list(extra))


def _final(tmp_path, save):
    ck = torch.load(tmp_path / save / 'scene_emresnet18_finetuned_s1_scene.tar', weights_only=False)
    return ck['actor_model_state_dict'], ck['actor_model_optimizer_state_dict']['square_avg']


def _by_hand(tmp_path, schedule, checkpoints):
    """the driver's iterations as one uninterrupted process: schedule = [(frames, max_frames of the run the iteration belongs to)]; the sampler is
    re-seeded where a run starts, as the driver does; -> {index in schedule: state_dict} for the indices in `checkpoints`"""
    from pvr_habitat_amd import main_bc_finetune as Fz
    from pvr_habitat_amd.bc_data import DeviceDataset
    from pvr_habitat_amd.utils_bc import sample_with_minimum_distance
    flags = _args(tmp_path, 'hand', 0, '--embedding_random_crop')
    torch.manual_seed(flags.run_id)
    obs, action, reward, done = Fz.load_raw(flags, 'scene')
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=T_ * B_ * 2, random_crop=True, crop_seed=flags.run_id)
    model = M.PolicyNetWithEncoder(net, 3, False, num_frames=2, max_unroll=T_, max_batch=B_)
    opt = M.HipJointRMSprop(model, lr=flags.learning_rate, eps=flags.epsilon, alpha=flags.alpha, max_grad_norm=flags.max_grad_norm)
    model.train()
    ds = DeviceDataset(obs, action, done, torch.device('cuda'))
    out, run_of = {}, None
    for i, (frames, max_frames) in enumerate(schedule):
        if max_frames != run_of:
            random.seed(flags.run_id)
            run_of, opt.max_epochs = max_frames, max_frames // (T_ * B_) + 1
        model.embedding.crop_call = frames // (T_ * B_)
        o, a, d = ds.gather(sample_with_minimum_distance(n=len(reward), k=B_, d=T_), T_)
        opt.scheduler_step()
        opt.step(o, d, a)
        if i in checkpoints:
            torch.cuda.synchronize()
            out[i] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.close()
    return out


def test_a_resumed_driver_run_draws_what_an_uninterrupted_process_would(tmp_path, capsys):
    """Four iterations (T = 3, B = 2: 12 64 x 64 frames per step) with --embedding_random_crop, and the same run interrupted after two iterations and
    resumed; the final parameters are compared bit for bit.

    The driver keeps the reference's resume (tests/test_gpu_e2e_bc.py pins it): a resumed run starts at the LAST SAVED frame count, so it repeats that
    iteration, and it restarts the sampler from the seed.  The resumed run therefore makes the updates of frames 0, 6 | 6, 12, 18 on the batches
    d0, d1 | d0, d1, d2, and no uninterrupted DRIVER run makes that sequence, with or without the mode.  The uninterrupted side is therefore one
    process that makes exactly these updates by hand on one model, without a checkpoint in between, setting crop_call = frames // (B T) as the driver
    does: equal bits say that the checkpoint carries everything and that the resumed run's windows are a function of the iteration alone.  The four
    iterations of the uninterrupted driver run are held to the same process (frames 0, 6, 12, 18 on d0 .. d3)."""
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 'whole', 24, '--embedding_random_crop'))['scene']
    printed = capsys.readouterr().out
    assert 'random crop' in printed and '--embedding_random_crop' in printed
    assert stats['frames'] == [0, 0, 6, 12, 18] and all(np.isfinite(stats['training_loss'][1:]))
    whole, _ = _final(tmp_path, 'whole')
    Fz.run(_args(tmp_path, 'parts', 12, '--embedding_random_crop'))
    half, _ = _final(tmp_path, 'parts')
    again = Fz.run(_args(tmp_path, 'parts', 24, '--embedding_random_crop'))['scene']
    assert again['frames'] == [0, 0, 6, 6, 12, 18]
    parts, _ = _final(tmp_path, 'parts')
    hand = _by_hand(tmp_path, [(0, 12), (6, 12), (6, 24), (12, 24), (18, 24)], {1, 4})
    hand_whole = _by_hand(tmp_path, [(0, 24), (6, 24), (12, 24), (18, 24)], {3})[3]
    for name, got, want in (('two iterations', half, hand[1]), ('resumed', parts, hand[4]), ('uninterrupted', whole, hand_whole)):
        assert sorted(got) == sorted(want)
        bad = [k for k in got if not torch.equal(got[k].cpu(), want[k])]
        assert not bad, (name, bad[:5])
    assert not torch.equal(parts['embedding.conv1.weight'], half['embedding.conv1.weight'])
    # the parameters do not depend on the flag: a resume may switch it off (and the windows stop) or on
    capsys.readouterr()
    off = Fz.run(_args(tmp_path, 'parts', 30))['scene']
    assert off['frames'][-1] == 24 and np.isfinite(off['training_loss'][-1])
    assert 'random crop' not in capsys.readouterr().out
