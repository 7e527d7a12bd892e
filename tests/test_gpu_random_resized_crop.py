"""The random_resized_crop mode on the GPU (pvr_trainer_forward_rects; HipTrainableResNet(..., random_resized_crop=(lo, hi), crop_seed=...);
HipJointRMSprop; --embedding_random_resized_crop): resnet18 with the synthetic weights of the other trainer tests, 4 - 5 frames of 64 x 64.

The oracle is equality of bits with the plain step on prepared frames.  A 256 x 256 frame is not resized and its centre window is [16:240, 16:240],
so frame F at rectangle r is, bit for bit, the frame G at the centre window with G[16:240, 16:240] = the oracle form's resized crop of F at r
(tests/random_resized_crop_refs.py: F.interpolate on the cropped array, .round(), uint8) and the rest of G arbitrary (random bytes here).  The
rectangles of a step are predicted with E.crop_rects(crop_seed, call, n, 64, 64, scale)."""
import ctypes as C
import pickle
import random

import numpy as np
import pytest
import torch

import color_jitter_refs as CR
import random_resized_crop_refs as RR
from pvr_habitat_amd import _lib, synth
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import models as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason='needs an MI355X')]

SEED, CSEED = 9, 21
SCALE = (0.2, 1.0)
STRENGTHS = (0.4, 0.4, 0.4)
HW = 64
ON = {'random_resized_crop': SCALE, 'crop_seed': SEED}
COLOR = {'color_jitter': STRENGTHS, 'color_seed': CSEED}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _inputs(n):
    """(weights, n 64 x 64 frames, d(loss)/d(embeddings)): once per n"""
    if n not in _cache:
        dout = torch.randn((n, E.OUT_SIZE['r18']), generator=torch.Generator().manual_seed(17)) / n
        _cache[n] = (synth.resnet50_state_dict(3, 'r18'), synth.smooth_frames(11, n, HW, HW), dout)
    return _cache[n]


def _rects(call, n):
    r = E.crop_rects(SEED, call, n, HW, HW, SCALE)
    assert len({tuple(x) for x in r.tolist()}) == n and not (r[:, 2:] == HW).all(axis=1).any()      # n different rectangles, none the whole frame
    return r


def _prepared(frames, rects, seed=23):
    """G, 256 x 256, with G[i, 16:240, 16:240] = the oracle form's resized crop of frames[i] at rects[i] and random bytes around it"""
    g = np.random.default_rng(seed).integers(0, 256, (len(frames), 256, 256, 3), dtype=np.uint8)
    g[:, 16:240, 16:240] = RR.resized_crops(frames, rects, 224)
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
def test_batch_statistics_step_is_the_plain_step_on_prepared_frames():
    sd, frames, dout = _inputs(4)
    rects = _rects(0, 4)
    m = _model(sd, 4, **ON)
    assert m.random_resized_crop == (float(np.float32(0.2)), 1.0) and not m.random_crop and m.crop_seed == SEED and m.crop_call == 0
    on = _step(m, frames, dout)
    assert m.crop_call == 1 and m._windows is None             # the node took the rectangles and released them after its backward
    prepared = _step(_model(sd, 4), _prepared(frames, rects), dout)
    plain = _step(_model(sd, 4), frames, dout)
    assert all(g is not None for g in on[1].values()) and bool(torch.isfinite(on[0]).all())
    assert 'bn1.running_mean' in on[2] and 'layer4.1.bn2.num_batches_tracked' in on[2] and int(on[2]['bn1.num_batches_tracked']) == 1
    assert _same(on, prepared) is None, _same(on, prepared)
    assert not torch.equal(on[0], plain[0]) and not torch.equal(on[1]['conv1.weight'], plain[1]['conv1.weight'])
    assert not torch.equal(on[2]['bn1.running_mean'], plain[2]['bn1.running_mean'])
    # the comparison tells the mutants of the reference from the kernel: frames prepared with either give other embeddings
    for mutant in ('frame_clamp', 'swapped'):
        g = _prepared(frames, rects)
        g[:, 16:240, 16:240] = RR.resized_crops(frames, rects, 224, form=RR.kernel_resized_crop, mutant=mutant)
        assert not torch.equal(_model(sd, 4)(torch.from_numpy(g).cuda()).detach().cpu(), on[0]), mutant
    # the next forward draws call 1 (batch statistics: the embeddings do not depend on the running statistics the first step moved)
    out2 = m(torch.from_numpy(frames).cuda()).detach().cpu()
    ref_out2 = _model(sd, 4)(torch.from_numpy(_prepared(frames, _rects(1, 4))).cuda()).detach().cpu()
    assert m.crop_call == 2 and torch.equal(out2, ref_out2) and not torch.equal(out2, on[0])


# ------------------------------------------------------------------------------------------------------------------
# frozen BatchNorm, chunked: 5 frames in passes of 2, 2, 1; the backward recomputes two passes
# ------------------------------------------------------------------------------------------------------------------
CHUNKED = {'fp32': {}, 'conv_split16': {'conv_split16': True}, 'wgrad_split16': {'wgrad_split16': True}, 'layer3': {'train_from': 'layer3'},
           'layer3_prefix_once': {'train_from': 'layer3', 'prefix_once': True}}


def _chunked(name, how):
    """how: 'on' (the mode on the frames), 'prepared' (the plain step on the prepared frames), 'on_color' / 'prepared_color' (both with color_jitter)"""
    key = ('chunked', name, how)
    if key not in _cache:
        sd, frames, dout = _inputs(5)
        modes = dict(CHUNKED[name], **(COLOR if how.endswith('color') else {}))
        on = how.startswith('on')
        m = _model(sd, 2, freeze_bn=True, **dict(modes, **(ON if on else {})))
        assert len(m._passes(5)) == 3
        _cache[key] = _step(m, frames if on else _prepared(frames, _rects(0, 5)), dout)
        assert m.crop_call == (1 if on or how.endswith('color') else 0)
    return _cache[key]


@pytest.mark.parametrize('name', ['fp32', 'conv_split16', 'wgrad_split16', 'layer3_prefix_once'])
def test_chunked_frozen_bn_step_is_the_plain_step_on_prepared_frames(name):
    sd, frames, dout = _inputs(5)
    rects = _rects(0, 5)
    assert not np.array_equal(rects[:2], rects[2:4])           # the passes get different rectangles
    on, prepared = _chunked(name, 'on'), _chunked(name, 'prepared')
    assert _same(on, prepared) is None, _same(on, prepared)
    trained = [k for k, g in on[1].items() if g is not None]
    assert ('conv1.weight' in trained) == ('train_from' not in CHUNKED[name]) and 'layer3.0.conv1.weight' in trained
    assert all(float(on[1][k].abs().sum()) > 0 for k in trained)
    plain = _step(_model(sd, 2, freeze_bn=True, **CHUNKED[name]), frames, dout)
    assert not torch.equal(on[0], plain[0])                    # and not Resize(256) + centre crop of the frames themselves


def test_prefix_once_keeps_the_bits_of_the_mode_without_it():
    """with prefix_once the recompute passes start at the boundary tensor, without it they run the stem again at the same rectangles: the same bits"""
    a, b = _chunked('layer3_prefix_once', 'on'), _chunked('layer3', 'on')
    assert _same(a, b) is None, _same(a, b)


# ------------------------------------------------------------------------------------------------------------------
# with color_jitter: the colour step on the prepared frames at the centre window
# ------------------------------------------------------------------------------------------------------------------
def test_batch_statistics_step_with_colour_is_the_colour_step_on_prepared_frames():
    sd, frames, dout = _inputs(4)
    m = _model(sd, 4, **dict(ON, **COLOR))
    on = _step(m, frames, dout)
    assert m.crop_call == 1 and m._windows is None and m._color is None
    ref = _step(_model(sd, 4, **COLOR), _prepared(frames, _rects(0, 4)), dout)
    assert _same(on, ref) is None, _same(on, ref)
    without_colour = _step(_model(sd, 4, **ON), frames, dout)
    assert not torch.equal(on[0], without_colour[0]) and bool(torch.isfinite(on[0]).all())
    # the colour parameters are the ones color_jitter alone draws: the rectangles come from a stream of their own
    params = CR.unpack_params(E.color_params(CSEED, 0, 4, STRENGTHS))
    assert any(abs(p[1] - 1.0) > 0.01 for p in params)          # contrast is not the identity


@pytest.mark.parametrize('name', ['fp32', 'layer3_prefix_once'])
def test_chunked_step_with_colour_is_the_colour_step_on_prepared_frames(name):
    on, ref = _chunked(name, 'on_color'), _chunked(name, 'prepared_color')
    assert _same(on, ref) is None, _same(on, ref)
    assert not torch.equal(on[0], _chunked(name, 'on')[0])


# ------------------------------------------------------------------------------------------------------------------
# the joint step
# ------------------------------------------------------------------------------------------------------------------
def test_a_joint_step_is_the_plain_step_on_prepared_observations():
    T, B, F_ = 1, 2, 2
    n = T * B * F_
    import policy_dobs_refs as R
    obs, done, act = R.chain_inputs(13, T, B, F_, hw=HW)
    frames = obs.reshape(T * B, HW, HW, F_, 3).transpose(0, 3, 1, 2, 4).reshape(n, HW, HW, 3)            # split_frames' (observation, frame) order
    to_obs = lambda fr: np.ascontiguousarray(fr.reshape(T, B, F_, 256, 256, 3).transpose(0, 1, 3, 4, 2, 5).reshape(T, B, 256, 256, 3 * F_))
    d, a = done.cuda(), act.cuda()
    runs = []
    for on in (True, False):
        enc_sd, pol_sd = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * E.OUT_SIZE['r18'], 1)
        enc = _model(enc_sd, n, **(ON if on else {}))
        enc.crop_call = 5                                      # a caller's own call number, as the driver sets it
        m = M.PolicyNetWithEncoder(enc, R.A, True, num_frames=F_, max_unroll=T, max_batch=B)
        m.policy.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pol_sd.items()})
        m.train()
        opt = M.HipJointRMSprop(m, lr=1e-3)
        rects = _rects(5, n)
        o = torch.from_numpy(obs if on else to_obs(_prepared(frames, rects))).cuda()
        before = enc._flat.clone()
        loss, norm = opt.step(o, d, a)
        torch.cuda.synchronize()
        runs.append((float(loss), float(norm), enc._flat.clone(), enc._bufs.clone(), m.policy._flat.clone()))
        assert np.isfinite(runs[-1][0]) and np.isfinite(runs[-1][1]) and not torch.equal(before, runs[-1][2])
        assert enc.crop_call == (6 if on else 5) and enc._windows is None
        m.close()
    on, off = runs
    assert on[:2] == off[:2], (on[:2], off[:2])
    assert all(torch.equal(x, y) for x, y in zip(on[2:], off[2:]))


# ------------------------------------------------------------------------------------------------------------------
# the launch names; the entry point without rectangles; off means off; eval mode
# ------------------------------------------------------------------------------------------------------------------
def test_off_moves_nothing_and_on_replaces_the_image_launches_alone():
    sd, frames, dout = _inputs(4)
    got = {}
    for how, kw in (('without', {}), ('none', {'random_resized_crop': None, 'crop_seed': 5}), ('on', ON), ('colour', COLOR), ('on_colour', dict(ON, **COLOR))):
        m = _model(sd, 4, **kw)
        _lib.check(_lib.lib().pvr_trainer_debug_set_timing(m._handle, 1))
        step = _step(m, frames, dout)
        got[how] = (_launches(m), step, m.workspace_bytes(), m.random_resized_crop)
        m.close()
    base = got['without']
    assert base[0][:3] == ['preprocess', 'normalize', 'conv1 pack'] and base[3] is None
    assert got['none'][0] == base[0] and got['none'][2] == base[2] and got['none'][3] is None and _same(got['none'][1], base[1]) is None
    on = got['on']
    assert on[0] == ['preprocess rects'] + base[0][2:] and on[2] == base[2] and not torch.equal(on[1][0], base[1][0])
    assert not {'preprocess', 'normalize', 'preprocess windows'} & set(on[0])
    colour, both = got['colour'], got['on_colour']
    assert colour[0] == ['colour stats', 'preprocess colour'] + base[0][2:] and both[0] == colour[0] and both[2] == base[2]
    assert not torch.equal(both[1][0], colour[1][0]) and not torch.equal(both[1][0], on[1][0])


def test_the_entry_point_without_rectangles_is_forward_augmented():
    """rects_dev == NULL: the same launches, names and bits as pvr_trainer_forward_augmented with null windows (pvr_trainer_forward); and the whole frame
    as every frame's rectangle gives the bits of one 'preprocess rects' launch wherever it is called from"""
    L = _lib.lib()
    sd, frames, dout = _inputs(4)
    fr = torch.from_numpy(frames).cuda()
    whole = torch.from_numpy(np.tile(np.array([[0, 0, HW, HW]], np.int32), (4, 1))).cuda()
    results = {}
    for how in ('augmented', 'null_rects', 'rects'):
        m = _model(sd, 4)
        _lib.check(L.pvr_trainer_debug_set_timing(m._handle, 1))
        out = torch.full((4, m.out_size), float('nan'), device='cuda')
        if how == 'augmented':
            _lib.check(L.pvr_trainer_forward_augmented(m._handle, vp(m._flat), vp(m._bufs), vp(fr), 4, HW, HW, None, None, None, None, 0, vp(out), out.stride(0),
                                                       _lib.stream_ptr()))
        else:
            _lib.check(L.pvr_trainer_forward_rects(m._handle, vp(m._flat), vp(m._bufs), vp(fr), 4, HW, HW, vp(whole) if how == 'rects' else None, None, None,
                                                   None, 0, vp(out), out.stride(0), _lib.stream_ptr()))
        names = _launches(m)
        g = torch.empty_like(m._flat)
        dd = dout.cuda()
        _lib.check(L.pvr_trainer_backward(m._handle, vp(m._flat), vp(dd), dd.stride(0), vp(g), _lib.stream_ptr()))
        torch.cuda.synchronize()
        results[how] = (names, out.cpu(), g.cpu(), m._bufs.cpu())
        m.close()
    a, b, c = results['augmented'], results['null_rects'], results['rects']
    assert a[0][:3] == ['preprocess', 'normalize', 'conv1 pack'] and b[0] == a[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert c[0] == ['preprocess rects'] + a[0][2:] and bool(torch.isfinite(c[1]).all()) and float(c[2].abs().sum()) > 0
    # the whole 64 x 64 frame resized to 224 is not Resize(256) + centre crop
    assert not torch.equal(a[1], c[1])
    want = _model(sd, 4)(torch.from_numpy(_prepared(frames, whole.cpu().numpy())).cuda()).detach().cpu()
    assert torch.equal(c[1], want)


def test_a_frame_smaller_than_the_crop_is_legal():
    """no Resize runs on this path: 40 x 56 frames, which pvr_trainer_forward_windows would resize first"""
    sd, _, dout = _inputs(4)
    frames = synth.smooth_frames(5, 4, 40, 56)
    rects = E.crop_rects(SEED, 0, 4, 40, 56, SCALE)
    on = _step(_model(sd, 4, **ON), frames, dout)
    assert _same(on, _step(_model(sd, 4), _prepared(frames, rects), dout)) is None


def test_eval_mode_is_the_eval_mode_of_the_encoder_without_the_mode():
    sd, frames, _ = _inputs(4)
    fr = torch.from_numpy(frames).cuda()
    outs = []
    for modes in (ON, {}):
        m = _model(sd, 4, **modes)
        m.eval()
        outs.append(m(fr).cpu())
        assert m.crop_call == 0
        m.close()
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())


def test_the_cache_entry_points_refuse_the_mode():
    sd, frames, _ = _inputs(4)
    m = _model(sd, 2, freeze_bn=True, train_from='layer3', prefix_once=True, **ON)
    with pytest.raises(ValueError, match='random_resized_crop with build_prefix_cache.*ONE window per frame.*prefix_once'):
        m.build_prefix_cache(torch.from_numpy(frames).cuda())
    with pytest.raises(ValueError, match='random_resized_crop with forward_cached.*ONE window per frame.*prefix_once'):
        m.forward_cached(None, None)
    with pytest.raises(ValueError, match='random_resized_crop with prefix_cache'):
        E.HipTrainableResNet(sd, 'r18', max_batch=2, train_from='layer3', prefix_cache=True, **ON)
    with pytest.raises(ValueError, match='random_resized_crop with random_crop'):
        E.HipTrainableResNet(sd, 'r18', max_batch=2, random_crop=True, **ON)


# ------------------------------------------------------------------------------------------------------------------
# the driver
# ------------------------------------------------------------------------------------------------------------------
T_, B_ = 3, 2
FLAG = ('--embedding_random_resized_crop', '0.2', '1')


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
    flags = _args(tmp_path, 'hand', 0, *FLAG)
    torch.manual_seed(flags.run_id)
    obs, action, reward, done = Fz.load_raw(flags, 'scene')
    net = E.EmbeddingNet('resnet18', pretrained=False, train=True, max_batch=T_ * B_ * 2, random_resized_crop=(0.2, 1.0), crop_seed=flags.run_id)
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
    """Four iterations (T = 3, B = 2: 12 64 x 64 frames per step) with --embedding_random_resized_crop 0.2 1, and the same run interrupted after two
    iterations and resumed; the final parameters are compared bit for bit.

    As in tests/test_gpu_random_crop.py: the driver keeps the reference's resume, so a resumed run starts at the LAST SAVED frame count, repeats that
    iteration and restarts the sampler from the seed.  The uninterrupted side is therefore one process that makes exactly the resumed run's updates by
    hand on one model, without a checkpoint in between, setting crop_call = frames // (B T) as the driver does: equal bits say that the checkpoint
    carries everything and that the resumed run's rectangles are a function of the iteration alone.  The four iterations of the uninterrupted driver
    run are held to the same process."""
    from pvr_habitat_amd import main_bc_finetune as Fz
    _scene(tmp_path)
    stats = Fz.run(_args(tmp_path, 'whole', 24, *FLAG))['scene']
    printed = capsys.readouterr().out
    assert 'random resized crop' in printed and '--embedding_random_resized_crop' in printed
    assert stats['frames'] == [0, 0, 6, 12, 18] and all(np.isfinite(stats['training_loss'][1:]))
    whole, _ = _final(tmp_path, 'whole')
    Fz.run(_args(tmp_path, 'parts', 12, *FLAG))
    half, _ = _final(tmp_path, 'parts')
    again = Fz.run(_args(tmp_path, 'parts', 24, *FLAG))['scene']
    assert again['frames'] == [0, 0, 6, 6, 12, 18]
    parts, _ = _final(tmp_path, 'parts')
    hand = _by_hand(tmp_path, [(0, 12), (6, 12), (6, 24), (12, 24), (18, 24)], {1, 4})
    hand_whole = _by_hand(tmp_path, [(0, 24), (6, 24), (12, 24), (18, 24)], {3})[3]
    for name, got, want in (('two iterations', half, hand[1]), ('resumed', parts, hand[4]), ('uninterrupted', whole, hand_whole)):
        assert sorted(got) == sorted(want)
        bad = [k for k in got if not torch.equal(got[k].cpu(), want[k])]
        assert not bad, (name, bad[:5])
    assert not torch.equal(parts['embedding.conv1.weight'], half['embedding.conv1.weight'])
    # the parameters do not depend on the flag: a resume may switch it off (and the rectangles stop) or on
    capsys.readouterr()
    off = Fz.run(_args(tmp_path, 'parts', 30))['scene']
    assert off['frames'][-1] == 24 and np.isfinite(off['training_loss'][-1])
    assert 'random resized crop' not in capsys.readouterr().out
