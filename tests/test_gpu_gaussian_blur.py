"""The gaussian_blur and random_grayscale modes on the GPU (pvr_trainer_forward_staged; HipTrainableResNet(..., gaussian_blur=(p, lo, hi),
random_grayscale=p, blur_seed=...); HipJointRMSprop; --embedding_gaussian_blur, --embedding_random_grayscale): resnet18 with the synthetic weights of
the other trainer tests, four frames per step.

The oracle is equality of bits with the path WITHOUT any augmentation on PRE-AUGMENTED frames.  A 256 x 256 frame is not resized and its centre window
is (16, 16), so a step with the modes on equals, bit for bit, the plain step on frames whose centre window holds the augmented 224 x 224 uint8 image.
That image is made by the ops themselves - pvr_op_preprocess_staged and pvr_op_blur_normalize on the parameters the host predicts for the step
(E.crop_windows / E.crop_rects, E.color_params, E.blur_params), read back through refs.recover_u8 - and tests/test_gpu_gaussian_blur_kernels.py holds
those ops to the references.  What this file adds is the trainer: the launches, the parameters of every pass and recompute pass, conv1's weight
gradient on the augmented image, the joint step and the driver."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

import gaussian_blur_refs as BR
import policy_dobs_refs as R
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SEED, CSEED, BSEED = 9, 21, 21
STRENGTHS, SCALE = (0.4, 0.6, 0.8), (0.2, 1.0)
BLUR, GRAY = (0.5, 0.1, 2.0), 0.5
N = 4
ON = {'gaussian_blur': BLUR, 'random_grayscale': GRAY, 'blur_seed': BSEED}
# max_batch, the structural modes (kept by the reference model) and the other augmentations (made on the host side of the reference)
CONFIGS = {'batch_statistics': (4, {}, {}),
           'chunked_frozen_bn': (2, {'freeze_bn': True}, {}),
           'layer3_prefix_once_split16': (2, {'freeze_bn': True, 'train_from': 'layer3', 'prefix_once': True, 'conv_split16': True, 'wgrad_split16': True}, {}),
           'with_random_crop': (4, {}, {'random_crop': True, 'crop_seed': SEED}),
           'with_rrc_and_colour_chunked': (2, {'freeze_bn': True}, {'random_resized_crop': SCALE, 'crop_seed': SEED, 'color_jitter': STRENGTHS,
                                                                   'color_seed': CSEED})}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs():
    """(weights, 4 256 x 256 frames, d(loss)/d(embeddings)): once"""
    if 'inputs' not in _cache:
        dout = torch.randn((N, E.OUT_SIZE['r18']), generator=torch.Generator().manual_seed(17)) / N
        _cache['inputs'] = (synth.resnet50_state_dict(3, 'r18'), synth.smooth_frames(11, N, 256, 256), dout)
    return _cache['inputs']


def _augmented(frames, call, aug, blur=BLUR, gray=GRAY, hw=256, crop=224):
    """the frames a plain encoder must be given to see what step number `call` of an encoder with the modes `aug` + gaussian_blur + random_grayscale sees:
    zeros with the augmented image in the centre window"""
    L = _lib.lib()
    n = len(frames)
    h, w = frames.shape[1:3]
    rh, rw = E.resized_size(h, w, 256)
    params = E.blur_params(BSEED, call, n, blur, gray)
    assert 0 < (params['sigma'] > 0).sum() < n or n < 3         # blurred and unblurred frames in one step
    if 'random_resized_crop' in aug:
        src, rects = E.crop_rects(SEED, call, n, h, w, SCALE), True
    else:
        src = E.crop_windows(SEED, call, n, rh - crop, rw - crop) if aug.get('random_crop') else \
            np.tile(np.array([[int(round((rh - crop) / 2.0)), int(round((rw - crop) / 2.0))]], np.int32), (n, 1))
        rects = False
    dev, src_d = torch.from_numpy(frames).cuda(), torch.from_numpy(np.ascontiguousarray(src, np.int32)).cuda()
    col = torch.from_numpy(E.color_params(CSEED, call, n, STRENGTHS).view(np.int32).reshape(n, 4)).cuda() if 'color_jitter' in aug else None
    sums = torch.zeros((n,), dtype=torch.int32, device='cuda')
    staged = torch.empty((n, crop, crop, 4), dtype=torch.uint8, device='cuda')
    par = torch.from_numpy(params.view(np.int32).reshape(n, 2)).cuda()
    out = torch.empty((n, crop, crop, 4), device='cuda')
    mean, std = (C.c_float * 3)(*E.IMAGENET_MEAN), (C.c_float * 3)(*E.IMAGENET_STD)
    _lib.check(L.pvr_op_preprocess_staged(vp(dev), n, h, w, 256, crop, None if rects else vp(src_d), vp(src_d) if rects else None, vp(col),
                                          None if col is None else vp(sums), vp(staged), _lib.stream_ptr()))
    _lib.check(L.pvr_op_blur_normalize(vp(staged), n, crop, mean, std, vp(par), vp(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    image = BR.recover_u8(out.cpu().numpy())
    plain = staged.cpu().numpy()[..., :3]
    changed = [not np.array_equal(image[i], plain[i]) for i in range(n)]
    touched = [bool(p['sigma'] > 0 or p['gray']) for p in params]
    assert all(c <= t for c, t in zip(changed, touched)) and any(changed), (changed, params)             # (a weak blur may leave a smooth frame as it is)
    assert all(c for c, p in zip(changed, params) if p['gray']), (changed, params)
    big = np.zeros((n, hw, hw, 3), np.uint8)
    t = (hw - crop) // 2
    big[:, t:t + crop, t:t + crop] = image
    return big


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
# an augmented step is the plain step on pre-augmented frames
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CONFIGS))
def test_autograd_step_is_the_plain_step_on_preaugmented_frames(name):
    sd, frames, dout = _inputs()
    max_batch, structure, aug = CONFIGS[name]
    m = _model(sd, max_batch, **dict(structure, **aug, **ON))
    assert m.gaussian_blur == (0.5, float(np.float32(0.1)), 2.0) and m.random_grayscale == 0.5 and m.blur_seed == BSEED and m.crop_call == 0
    assert len(m._passes(N)) == N // max_batch
    on = _step(m, frames, dout)
    assert m.crop_call == 1 and m._blur is None and m._color is None and m._windows is None      # the node took the parameters and released them
    ref_m = _model(sd, max_batch, **structure)
    ref = _step(ref_m, _augmented(frames, 0, aug), dout)
    assert bool(torch.isfinite(on[0]).all())
    assert _same(on, ref) is None, _same(on, ref)
    trained = [k for k, g in on[1].items() if g is not None]
    assert ('conv1.weight' in trained) == ('train_from' not in structure) and 'layer3.0.conv1.weight' in trained
    assert all(float(on[1][k].abs().sum()) > 0 for k in trained)
    without = _step(_model(sd, max_batch, **dict(structure, **aug)), frames, dout)       # the two modes moved the step
    assert not torch.equal(on[0], without[0]) and not torch.equal(on[1]['layer3.0.conv1.weight'], without[1]['layer3.0.conv1.weight'])
    if not structure.get('freeze_bn'):                          # the next forward draws call 1 (batch statistics: the embeddings ignore the moved running ones)
        out2 = m(torch.from_numpy(frames).cuda()).detach().cpu()
        want2 = ref_m(torch.from_numpy(_augmented(frames, 1, aug)).cuda()).detach().cpu()
        assert m.crop_call == 2 and torch.equal(out2, want2) and not torch.equal(out2, on[0])


@pytest.mark.parametrize('name', ['chunked_frozen_bn', 'with_rrc_and_colour_chunked'])
def test_joint_step_is_the_plain_step_on_preaugmented_observations(name):
    """T = 1, B = 2, two frames per observation: loss, gradient norm and the updated parameters of encoder and policy after one HipJointRMSprop step"""
    T, B, F_ = 1, 2, 2
    max_batch, structure, aug = CONFIGS[name]
    obs, done, act = R.chain_inputs(13, T, B, F_, hw=256)
    frames = obs.reshape(T * B, 256, 256, F_, 3).transpose(0, 3, 1, 2, 4).reshape(N, 256, 256, 3)        # split_frames' (observation, frame) order
    to_obs = lambda fr: np.ascontiguousarray(fr.reshape(T, B, F_, 256, 256, 3).transpose(0, 1, 3, 4, 2, 5).reshape(T, B, 256, 256, 3 * F_))
    assert np.array_equal(to_obs(frames), obs)
    d, a = done.cuda(), act.cuda()
    runs = []
    for on in (True, False):
        enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], 1)
        enc = _model(enc_sd, max_batch, **dict(structure, **(dict(aug, **ON) if on else {})))
        enc.crop_call = 5                                      # a caller's own call number, as the driver sets it
        m = M.PolicyNetWithEncoder(enc, R.A, True, num_frames=F_, max_unroll=T, max_batch=B)
        m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
        m.train()
        opt = M.HipJointRMSprop(m, lr=1e-3)
        o = torch.from_numpy(obs if on else to_obs(_augmented(frames, 5, aug))).cuda()
        before = enc._flat.clone()
        loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        runs.append((float(loss), float(norm), enc._flat.clone(), enc._bufs.clone(), m.policy._flat.clone()))
        assert np.isfinite(runs[-1][0]) and np.isfinite(runs[-1][1]) and not torch.equal(before, runs[-1][2])
        assert enc.crop_call == (6 if on else 5) and enc._windows is None and enc._color is None and enc._blur is None
        m.close()
    on, off = runs
    assert on[:2] == off[:2], (on[:2], off[:2])
    assert all(torch.equal(x, y) for x, y in zip(on[2:], off[2:]))


# ------------------------------------------------------------------------------------------------------------------
# off means off; on, the launch list changes before conv1 alone
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('other', ['centre', 'random_crop', 'colour', 'rrc_colour'])
def test_off_moves_nothing_and_on_replaces_the_image_launches_alone(other):
    sd, frames, dout = _inputs()
    aug = {'centre': {}, 'random_crop': {'random_crop': True, 'crop_seed': SEED}, 'colour': {'color_jitter': STRENGTHS, 'color_seed': CSEED},
           'rrc_colour': {'random_resized_crop': SCALE, 'crop_seed': SEED, 'color_jitter': STRENGTHS, 'color_seed': CSEED}}[other]
    image = {'centre': ['preprocess', 'normalize'], 'random_crop': ['preprocess windows'], 'colour': ['colour stats', 'preprocess colour'],
             'rrc_colour': ['colour stats', 'preprocess colour']}[other]
    got = {}
    for how, kw in (('without', {}), ('none', {'gaussian_blur': None, 'random_grayscale': None}),
                    ('zeros', {'gaussian_blur': (0, 0.1, 2.0), 'random_grayscale': 0.0, 'blur_seed': 5}), ('on', ON)):
        m = _model(sd, 4, **dict(aug, **kw))
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        step = _step(m, frames, dout)
        got[how] = (_launches(m), step, m.workspace_bytes(), (m.gaussian_blur, m.random_grayscale), m._staged)
        m.close()
    base = got['without']
    assert base[0][:len(image) + 1] == image + ['conv1 pack'] and base[3] == (None, None) and base[4] is None
    for how in ('none', 'zeros'):
        assert got[how][0] == base[0] and got[how][2] == base[2] and got[how][3] == (None, None) and got[how][4] is None, how
        assert _same(got[how][1], base[1]) is None, how
    on = got['on']
    staged = (['colour stats'] if 'color_jitter' in aug else []) + ['stage image', 'blur normalize']
    assert on[0] == staged + base[0][len(image):] and on[2] == base[2]
    assert on[0].index('conv1 pack') == len(staged) and not torch.equal(on[1][0], base[1][0])
    assert on[4] is not None and tuple(on[4].shape) == (4, 224, 224, 4) and on[4].dtype == torch.uint8


def test_the_entry_point_without_blur_parameters_is_the_one_it_extends():
    """blur_dev == NULL: the launches, names and bits of pvr_trainer_forward_augmented (windows) and pvr_trainer_forward_rects; and rows of (0, 0) give those
    bits through the staged launches"""
    L = _lib.lib()
    sd, frames, dout = _inputs()
    fr = torch.from_numpy(frames).cuda()
    win = torch.from_numpy(E.crop_windows(SEED, 0, N, 32, 32)).cuda()
    rects = torch.from_numpy(E.crop_rects(SEED, 0, N, 256, 256, SCALE)).cuda()
    col = torch.from_numpy(E.color_params(CSEED, 0, N, STRENGTHS).view(np.int32).reshape(N, 4)).cuda()
    sums = torch.zeros((N,), dtype=torch.int32, device='cuda')
    zeros = torch.zeros((N, 2), dtype=torch.int32, device='cuda')
    staged = torch.empty((N, 224, 224, 4), dtype=torch.uint8, device='cuda')
    results = {}
    for how in ('augmented', 'staged_null_w', 'staged_zero_w', 'rects', 'staged_null_r', 'staged_zero_r'):
        m = _model(sd, 4)
        _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
        out = torch.full((N, m.out_size), float('nan'), device='cuda')
        head = (m._handle, vp(m._flat), vp(m._bufs), vp(fr), N, 256, 256)
        tail = (None, 0, vp(out), out.stride(0), _lib.stream_ptr())
        if how == 'augmented':
            _lib.check(L.pvr_trainer_forward_augmented(*head, vp(win), vp(col), vp(sums), *tail))
        elif how == 'rects':
            _lib.check(L.pvr_trainer_forward_rects(*head, vp(rects), vp(col), vp(sums), *tail))
        else:
            w, r = (vp(win), None) if how.endswith('_w') else (None, vp(rects))
            _lib.check(L.pvr_trainer_forward_staged(*head, w, r, vp(col), vp(sums), vp(zeros) if 'zero' in how else None,
                                                    vp(staged) if 'zero' in how else None, *tail))
        names = _launches(m)
        g = torch.empty_like(m._flat)
        dd = dout.cuda()
        _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()))
        torch.cuda.synchronize()
        results[how] = (names, out.cpu(), g.cpu(), m._bufs.cpu())
        m.close()
    for base, null, zero in (('augmented', 'staged_null_w', 'staged_zero_w'), ('rects', 'staged_null_r', 'staged_zero_r')):
        a, b, c = results[base], results[null], results[zero]
        assert a[0][:2] == ['colour stats', 'preprocess colour'] and b[0] == a[0] and c[0] == ['colour stats', 'stage image', 'blur normalize'] + a[0][2:]
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
        assert bool(torch.isfinite(a[1]).all()) and float(a[2].abs().sum()) > 0


def test_eval_mode_is_the_eval_mode_of_the_encoder_without_the_modes():
    sd, frames, _ = _inputs()
    fr = torch.from_numpy(frames).cuda()
    outs = []
    for modes in (ON, {}):
        m = _model(sd, 4, **modes)
        m.eval()
        outs.append(m(fr).cpu())
        assert m.crop_call == 0 and m._blur is None and m._staged is None
        m.close()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_the_cache_entry_points_refuse_the_modes():
    sd, frames, _ = _inputs()
    for kw, name in (({'gaussian_blur': BLUR}, 'gaussian_blur'), ({'random_grayscale': GRAY}, 'random_grayscale')):
        m = _model(sd, 2, freeze_bn=True, train_from='layer3', prefix_once=True, **kw)
        with pytest.raises(ValueError, match='%s with build_prefix_cache.*ONE image per frame.*prefix_once' % name):
            m.build_prefix_cache(torch.from_numpy(frames).cuda())
        with pytest.raises(ValueError, match='%s with forward_cached.*ONE image per frame.*prefix_once' % name):
            m.forward_cached(None, None)
        with pytest.raises(ValueError, match='%s with prefix_cache' % name):
            E.HipTrainableResNet(sd, 'r18', max_batch=2, train_from='layer3', prefix_cache=True, **kw)
        m.close()


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
T_, B_ = 3, 2
FLAG = ('--embedding_gaussian_blur', '0.5', '0.1', '2.0', '--embedding_random_grayscale', '0.2')


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
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=T_ * B_ * 2, gaussian_blur=flags.embedding_gaussian_blur,
                         random_grayscale=flags.embedding_random_grayscale, blur_seed=flags.run_id)
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
    """Four iterations (T = 3, B = 2: 12 64 x 64 frames per step) with both flags, and the same run interrupted after two iterations and resumed: stats
    and saved parameters.  As tests/test_gpu_color_jitter.py explains, a resumed driver run repeats its last saved iteration and restarts the sampler, so
    it is held to ONE process that makes the same updates by hand on one model, setting crop_call = frames // (B T) as the driver does: equal bits say
    that the checkpoint carries everything and that the blur parameters are a function of the iteration alone."""
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 'whole', 24, *FLAG))['scene']
    printed = capsys.readouterr().out
    assert 'gaussian blur' in printed and '--embedding_gaussian_blur' in printed and 'sigma 0.1 .. 2' in printed
    assert 'random grayscale' in printed and '--embedding_random_grayscale' in printed
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
    assert [float(x) for x in stats['training_loss'][1:]] == whole_losses
    assert [float(x) for x in again['training_loss'][1:]] == hand_losses
    # the modes moved the run: the same four iterations without the flags end elsewhere
    capsys.readouterr()
    Fz.run(_args(tmp_path, 'plain', 24))
    assert 'gaussian blur' not in capsys.readouterr().out
    plain = _final(tmp_path, 'plain')
    assert sorted(plain) == sorted(whole) and not torch.equal(plain['embedding.conv1.weight'].cpu(), whole['embedding.conv1.weight'].cpu())
