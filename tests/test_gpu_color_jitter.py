"""The color_jitter mode on the GPU (pvr_trainer_forward_augmented; HipTrainableResNet(..., color_jitter=(b, c, s), color_seed=...); HipJointRMSprop;
--embedding_color_jitter): resnet18 with the synthetic weights of the other trainer tests, four frames per step.

The oracle is equality of bits with the path without the mode on PRE-JITTERED frames.  A 256 x 256 frame is not resized, so frame F jittered at window
(t, l) is, bit for bit, the frame G at the same window with G[t:t+224, l:l+224] = jitter(F[t:t+224, l:l+224]) - the jitter reads nothing outside the
window - made on the CPU with the reference of tests/color_jitter_refs.py.  The window is the centre one, (16, 16), or with random_crop the draw of
E.crop_windows; the parameters of a step are predicted with E.color_params(color_seed, call, n, strengths)."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

import color_jitter_refs as CR
import policy_dobs_refs as R
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SEED, CSEED = 9, 21
STRENGTHS = (0.4, 0.6, 0.8)
N = 4
# max_batch and the modes next to color_jitter: one pass with batch statistics; 4 frames in passes of 2, the backward's recompute pass runs the stem
# again on the same rows; the recompute pass starts at the boundary tensor, both split modes; windows and jitter together
CONFIGS = {'batch_statistics': (4, {}),
           'chunked_frozen_bn': (2, {'freeze_bn': True}),
           'layer3_prefix_once_split16': (2, {'freeze_bn': True, 'train_from': 'layer3', 'prefix_once': True, 'conv_split16': True, 'wgrad_split16': True}),
           'with_random_crop': (4, {'random_crop': True, 'crop_seed': SEED})}
ON = {'color_jitter': STRENGTHS, 'color_seed': CSEED}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs():
    """(weights, 4 256 x 256 frames, d(loss)/d(embeddings)): once"""
    if 'inputs' not in _cache:
        dout = torch.randn((N, E.OUT_SIZE['r18']), generator=torch.Generator().manual_seed(17)) / N
        _cache['inputs'] = (synth.resnet50_state_dict(3, 'r18'), synth.smooth_frames(11, N, 256, 256), dout)
    return _cache['inputs']


def _prejitter(frames, call, random_crop):
    """the frames with each one's window replaced by its jittered window, as the step number `call` of an encoder with these modes jitters it"""
    n = len(frames)
    windows = E.crop_windows(SEED, call, n, 32, 32) if random_crop else np.tile(np.array([[16, 16]], np.int32), (n, 1))
    params = CR.unpack_params(E.color_params(CSEED, call, n, STRENGTHS))
    out = frames.copy()
    for i, (t, l) in enumerate(windows.tolist()):
        out[i, t:t + 224, l:l + 224] = CR.jitter(frames[i, t:t + 224, l:l + 224], *params[i])
    assert not any(np.array_equal(out[i], frames[i]) for i in range(n))                 # every frame is jittered, or the comparison would be vacuous
    assert len({p[3] for p in params}) > 1 or n < 3
    return out


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
# a jittered step is the step without the mode on pre-jittered frames
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CONFIGS))
def test_autograd_step_is_the_step_on_prejittered_frames(name):
    sd, frames, dout = _inputs()
    max_batch, modes = CONFIGS[name]
    m = _model(sd, max_batch, **dict(modes, **ON))
    assert m.color_jitter == tuple(float(np.float32(s)) for s in STRENGTHS) and m.color_seed == CSEED and m.crop_call == 0
    assert len(m._passes(N)) == N // max_batch
    on = _step(m, frames, dout)
    assert m.crop_call == 1 and m._color is None and m._windows is None      # the node took the parameters and released them after its backward
    ref_m = _model(sd, max_batch, **modes)
    ref = _step(ref_m, _prejitter(frames, 0, 'random_crop' in modes), dout)
    plain = _step(_model(sd, max_batch, **modes), frames, dout)
    assert bool(torch.isfinite(on[0]).all())
    assert _same(on, ref) is None, _same(on, ref)
    trained = [k for k, g in on[1].items() if g is not None]
    assert ('conv1.weight' in trained) == ('train_from' not in modes) and 'layer3.0.conv1.weight' in trained
    assert all(float(on[1][k].abs().sum()) > 0 for k in trained)
    assert not torch.equal(on[0], plain[0]) and not torch.equal(on[1]['layer3.0.conv1.weight'], plain[1]['layer3.0.conv1.weight'])
    if not modes.get('freeze_bn'):                              # the next forward draws call 1 (batch statistics: the embeddings ignore the moved running ones)
        out2 = m(torch.from_numpy(frames).cuda()).detach().cpu()
        want2 = ref_m(torch.from_numpy(_prejitter(frames, 1, 'random_crop' in modes)).cuda()).detach().cpu()
        assert m.crop_call == 2 and torch.equal(out2, want2) and not torch.equal(out2, on[0])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_joint_step_is_the_step_on_prejittered_observations(name):
    """T = 1, B = 2, two frames per observation: loss, gradient norm and the updated parameters of encoder and policy after one HipJointRMSprop step"""
    T, B, F_ = 1, 2, 2
    max_batch, modes = CONFIGS[name]
    obs, done, act = R.chain_inputs(13, T, B, F_, hw=256)
    frames = obs.reshape(T * B, 256, 256, F_, 3).transpose(0, 3, 1, 2, 4).reshape(N, 256, 256, 3)        # split_frames' (observation, frame) order
    to_obs = lambda fr: np.ascontiguousarray(fr.reshape(T, B, F_, 256, 256, 3).transpose(0, 1, 3, 4, 2, 5).reshape(T, B, 256, 256, 3 * F_))
    assert np.array_equal(to_obs(frames), obs)
    d, a = done.cuda(), act.cuda()
    runs = []
    for on in (True, False):
        enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], 1)
        enc = _model(enc_sd, max_batch, **dict(modes, **(ON if on else {})))
        enc.crop_call = 5                                      # a caller's own call number, as the driver sets it
        m = M.PolicyNetWithEncoder(enc, R.A, True, num_frames=F_, max_unroll=T, max_batch=B)
        m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
        m.train()
        opt = M.HipJointRMSprop(m, lr=1e-3)
        o = torch.from_numpy(obs if on else to_obs(_prejitter(frames, 5, 'random_crop' in modes))).cuda()
        before = enc._flat.clone()
        loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        runs.append((float(loss), float(norm), enc._flat.clone(), enc._bufs.clone(), m.policy._flat.clone()))
        assert np.isfinite(runs[-1][0]) and np.isfinite(runs[-1][1]) and not torch.equal(before, runs[-1][2])
        assert enc.crop_call == (6 if on or 'random_crop' in modes else 5) and enc._windows is None and enc._color is None
        m.close()
    on, off = runs
    assert on[:2] == off[:2], (on[:2], off[:2])
    assert all(torch.equal(x, y) for x, y in zip(on[2:], off[2:]))


# ------------------------------------------------------------------------------------------------------------------
# off means off; on, two launches stand where the image was made
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('random_crop', [False, True], ids=['centre', 'random_crop'])
def test_off_moves_nothing_and_on_replaces_the_image_launches_alone(random_crop):
    sd, frames, dout = _inputs()
    fr = torch.from_numpy(frames).cuda()
    crop = {'random_crop': True, 'crop_seed': SEED} if random_crop else {}
    got = {}
    for how, kw in (('without', {}), ('none', {'color_jitter': None}), ('zeros', {'color_jitter': (0, 0, 0), 'color_seed': 5}), ('on', ON)):
        m = _model(sd, 4, **dict(crop, **kw))
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        step = _step(m, frames, dout)
        got[how] = (_launches(m), step, m.workspace_bytes(), m._color_jitter)
        m.close()
    base = got['without']
    image = ['preprocess windows'] if random_crop else ['preprocess', 'normalize']
    assert base[0][:len(image) + 1] == image + ['conv1 pack'] and base[3] is None
    for how in ('none', 'zeros'):
        assert got[how][0] == base[0] and got[how][2] == base[2] and got[how][3] is None, how
        assert _same(got[how][1], base[1]) is None, how
    on = got['on']
    assert on[0] == ['colour stats', 'preprocess colour'] + base[0][len(image):] and on[2] == base[2]
    assert not set(image) & set(on[0]) and not torch.equal(on[1][0], base[1][0])


def test_the_entry_point_without_colour_parameters_is_forward_windows():
    """color_dev == NULL: the same launches, names and bits as pvr_trainer_forward_windows; and identity parameters give those bits through the two launches"""
    L = _lib.lib()
    sd, frames, dout = _inputs()
    fr = torch.from_numpy(frames).cuda()
    win = torch.from_numpy(E.crop_windows(SEED, 0, N, 32, 32)).cuda()
    ones = torch.from_numpy(CR.pack_params([(1.0, 1.0, 1.0, k) for k in range(N)])).cuda()
    sums = torch.zeros((N,), dtype=torch.int32, device='cuda')
    results = {}
    for how in ('windows', 'null_color', 'identity'):
        m = _model(sd, 4)
        _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
        out = torch.full((N, m.out_size), float('nan'), device='cuda')
        if how == 'windows':
            _lib.check(L.pvr_trainer_forward_windows(m._handle, vp(m._flat), vp(m._bufs), vp(fr), N, 256, 256, vp(win), None, 0, vp(out), out.stride(0),
                                                     _lib.stream_ptr()))
        else:
            _lib.check(L.pvr_trainer_forward_augmented(m._handle, vp(m._flat), vp(m._bufs), vp(fr), N, 256, 256, vp(win), vp(ones) if how == 'identity' else None,
                                                       vp(sums) if how == 'identity' else None, None, 0, vp(out), out.stride(0), _lib.stream_ptr()))
        names = _launches(m)
        g = torch.empty_like(m._flat)
        dd = dout.cuda()
        _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()))
        torch.cuda.synchronize()
        results[how] = (names, out.cpu(), g.cpu(), m._bufs.cpu())
        m.close()
    a, b, c = results['windows'], results['null_color'], results['identity']
    assert a[0][0] == 'preprocess windows' and b[0] == a[0] and c[0] == ['colour stats', 'preprocess colour'] + a[0][1:]
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
    assert bool(torch.isfinite(a[1]).all()) and float(a[2].abs().sum()) > 0


def test_eval_mode_is_the_eval_mode_of_the_encoder_without_the_mode():
    sd, frames, _ = _inputs()
    fr = torch.from_numpy(frames).cuda()
    outs = []
    for modes in (ON, {}):
        m = _model(sd, 4, **modes)
        m.eval()
        outs.append(m(fr).cpu())
        assert m.crop_call == 0 and m._color is None
        m.close()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_the_cache_entry_points_refuse_the_mode():
    sd, frames, _ = _inputs()
    m = _model(sd, 2, freeze_bn=True, train_from='layer3', prefix_once=True, **ON)
    with pytest.raises(ValueError, match='color_jitter with build_prefix_cache.*ONE image per frame.*prefix_once'):
        m.build_prefix_cache(torch.from_numpy(frames).cuda())
    with pytest.raises(ValueError, match='color_jitter with forward_cached.*ONE image per frame.*prefix_once'):
        m.forward_cached(None, None)
    with pytest.raises(ValueError, match='color_jitter with prefix_cache'):
        E.HipTrainableResNet(sd, 'r18', max_batch=2, train_from='layer3', prefix_cache=True, **ON)
    m.close()


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
T_, B_ = 3, 2
FLAG = ('--embedding_color_jitter', '0.4', '0.3', '0.5')


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
    return ck['actor_model_state_dict']


def _by_hand(tmp_path, schedule, checkpoints):
    """the driver's iterations as one uninterrupted process: schedule = [(frames, max_frames of the run the iteration belongs to)]; the sampler is
    re-seeded where a run starts, as the driver does; -> ({index in schedule: state_dict} for the indices in `checkpoints`, the losses)"""
    from pvr_habitat_amd import main_bc_finetune as Fz
    from pvr_habitat_amd.bc_data import DeviceDataset
    from pvr_habitat_amd.utils_bc import sample_with_minimum_distance
    flags = _args(tmp_path, 'hand', 0, *FLAG)
    torch.manual_seed(flags.run_id)
    obs, action, reward, done = Fz.load_raw(flags, 'scene')
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=T_ * B_ * 2, color_jitter=flags.embedding_color_jitter, color_seed=flags.run_id)
    model = M.PolicyNetWithEncoder(net, 3, False, num_frames=2, max_unroll=T_, max_batch=B_)
    opt = M.HipJointRMSprop(model, lr=flags.learning_rate, eps=flags.epsilon, alpha=flags.alpha, max_grad_norm=flags.max_grad_norm)
    model.train()
    ds = DeviceDataset(obs, action, done, torch.device('cuda'))
    out, losses, run_of = {}, [], None
    for i, (frames, max_frames) in enumerate(schedule):
        if max_frames != run_of:
            random.seed(flags.run_id)
            run_of, opt.max_epochs = max_frames, max_frames // (T_ * B_) + 1
        model.embedding.crop_call = frames // (T_ * B_)
        o, a, d = ds.gather(sample_with_minimum_distance(n=len(reward), k=B_, d=T_), T_)
        opt.scheduler_step()
        losses.append(float(opt.step(o, d, a)[0]))
        if i in checkpoints:
            torch.cuda.synchronize()
            out[i] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.close()
    return out, losses


def test_a_resumed_driver_run_draws_what_an_uninterrupted_process_would(tmp_path, capsys):
    """Four iterations (T = 3, B = 2: 12 64 x 64 frames per step) with --embedding_color_jitter, and the same run interrupted after two iterations and
    resumed: stats and saved parameters.

    The driver keeps the reference's resume (tests/test_gpu_e2e_bc.py pins it, tests/test_gpu_random_crop.py explains it): a resumed run starts at the
    LAST SAVED frame count, so it repeats that iteration, and it restarts the sampler from the seed.  The resumed run therefore makes the updates of
    frames 0, 6 | 6, 12, 18 on the batches d0, d1 | d0, d1, d2, which no uninterrupted DRIVER run makes, with or without the mode.  The uninterrupted
    side is therefore one process that makes exactly these updates by hand on one model, without a checkpoint in between, setting crop_call =
    frames // (B T) as the driver does: equal bits say that the checkpoint carries everything and that the resumed run's colour parameters are a
    function of the iteration alone.  The four iterations of the uninterrupted driver run are held to the same process (frames 0, 6, 12, 18)."""
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 'whole', 24, *FLAG))['scene']
    printed = capsys.readouterr().out
    assert 'colour jitter' in printed and '--embedding_color_jitter' in printed and 'strengths 0.4 0.3 0.5' in printed
    assert stats['frames'] == [0, 0, 6, 12, 18] and all(np.isfinite(stats['training_loss'][1:]))
    whole = _final(tmp_path, 'whole')
    Fz.run(_args(tmp_path, 'parts', 12, *FLAG))
    half = _final(tmp_path, 'parts')
    again = Fz.run(_args(tmp_path, 'parts', 24, *FLAG))['scene']
    assert again['frames'] == [0, 0, 6, 6, 12, 18]
    parts = _final(tmp_path, 'parts')
    hand, hand_losses = _by_hand(tmp_path, [(0, 12), (6, 12), (6, 24), (12, 24), (18, 24)], {1, 4})
    hand_whole, whole_losses = _by_hand(tmp_path, [(0, 24), (6, 24), (12, 24), (18, 24)], {3})
    for name, got, want in (('two iterations', half, hand[1]), ('resumed', parts, hand[4]), ('uninterrupted', whole, hand_whole[3])):
        assert sorted(got) == sorted(want)
        bad = [k for k in got if not torch.equal(got[k].cpu(), want[k])]
        assert not bad, (name, bad[:5])
    # the stats: the driver's training losses are the by-hand process's, iteration by iteration
    assert [float(x) for x in stats['training_loss'][1:]] == whole_losses
    assert [float(x) for x in again['training_loss'][1:]] == hand_losses
    assert not torch.equal(parts['embedding.conv1.weight'], half['embedding.conv1.weight'])
    # the mode moved the run: the same four iterations without the flag end elsewhere
    capsys.readouterr()
    Fz.run(_args(tmp_path, 'plain', 24))
    assert 'colour jitter' not in capsys.readouterr().out
    plain = _final(tmp_path, 'plain')
    assert sorted(plain) == sorted(whole) and not torch.equal(plain['embedding.conv1.weight'].cpu(), whole['embedding.conv1.weight'].cpu())
    # the parameters do not depend on the flag: a resume may switch it off (and the jitter stops) or on
    off = Fz.run(_args(tmp_path, 'parts', 30))['scene']
    assert off['frames'][-1] == 24 and np.isfinite(off['training_loss'][-1])
    assert 'colour jitter' not in capsys.readouterr().out
