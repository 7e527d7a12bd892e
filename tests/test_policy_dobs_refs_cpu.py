"""The references of tests/policy_dobs_refs.py on the CPU: the dtype-generic policy equals oracle/policy_oracle.forward in fp32; the acceptance rule
for gradients passes for torch's own fp32 d(loss)/d(obs) and for the by-hand fp32 computation, and fails for every classic mistake; the workspace
size the driver's memory guard reads; and what `main_bc_finetune --train_embedding` refuses, before it needs a GPU."""
import pytest
import torch

import policy_dobs_refs as R
from oracle import policy_oracle as po
from pvr_habitat_amd import _lib
from pvr_habitat_amd import embeddings as E
from pvr_habitat_amd import synth

SMALL = [c for c in R.CASES if c[0] * c[1] < 64]
_cache = {}


def case(T, B, O, bn):
    key = (T, B, O, bn)
    if key not in _cache:
        sd = R.policy_params(7, O, bn)
        obs, done, act = R.inputs(11 + O, T, B, O)
        _cache[key] = dict(sd=sd, obs=obs, done=done, act=act, f64=R.dobs_autograd(sd, obs, done, act, bn, torch.float64),
                           f32=R.dobs_autograd(sd, obs, done, act, bn, torch.float32))
    return _cache[key]


@pytest.mark.parametrize('T,B,O,bn', SMALL)
def test_generic_forward_equals_the_oracle_in_fp32(T, B, O, bn):
    c = case(T, B, O, bn)
    p = po.to_params(c['sd'])
    ref, _ = po.forward(p, c['obs'], c['done'], (torch.zeros(2, B, 1024), torch.zeros(2, B, 1024)), bool(bn), training=True)
    got = c['f32'][2]
    assert got.dtype == torch.float32 and R.rel_l2(got, ref['policy_logits'].detach()) <= 1e-6
    assert R.dobs_autograd(c['sd'], c['obs'], c['done'], c['act'], bn, torch.float64)[2].dtype == torch.float64


@pytest.mark.parametrize('T,B,O,bn', SMALL)
def test_rule_passes_for_fp32_and_the_by_hand_gradient(T, B, O, bn):
    c = case(T, B, O, bn)
    ok, d, d32 = R.accept(c['f32'][0], c['f32'][0], c['f64'][0])
    assert ok and d32 < 1e-4, (d, d32)
    hand64 = R.dobs_by_hand(c['sd'], c['obs'], c['done'], c['act'], bn, torch.float64)
    assert R.rel_l2(hand64, c['f64'][0]) < 1e-12                 # the by-hand formula IS the gradient
    ok, d, d32 = R.accept(R.dobs_by_hand(c['sd'], c['obs'], c['done'], c['act'], bn, torch.float32), c['f32'][0], c['f64'][0])
    print('\n[dobs by hand fp32 %s] rel-L2 to float64 %.3e, torch fp32 %.3e' % ((T, B, O, bn), d, d32))
    assert ok, (d, d32)


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_rule_fails_for_every_mutant(mutant):
    for T, B, O, bn in SMALL:
        if (mutant.startswith('bn_') and not bn) or (mutant == 'w_not_transposed' and O != 1024):
            continue
        c = case(T, B, O, bn)
        ok, d, d32 = R.accept(R.dobs_by_hand(c['sd'], c['obs'], c['done'], c['act'], bn, torch.float32, mutant=mutant), c['f32'][0], c['f64'][0])
        print('\n[dobs mutant %s %s] rel-L2 to float64 %.3e, torch fp32 %.3e' % (mutant, (T, B, O, bn), d, d32))
        assert not ok, (mutant, (T, B, O, bn), d, d32)


def test_chain_rule_passes_in_fp32_and_fails_for_frame_major_frames():
    """the chain's reference (the reference's split / stack / concatenate lines) against the mistake of viewing frame-major embeddings as observations"""
    T, B, F_ = 2, 1, 2
    enc, pol = synth.resnet50_state_dict(3, 'r18'), R.policy_params(5, F_ * 512, 1)
    obs, done, act = R.chain_inputs(13, T, B, F_)
    _, e64, p64 = R.chain_grads(enc, pol, obs, done, act, 'r18', 1, torch.float64)
    _, e32, p32 = R.chain_grads(enc, pol, obs, done, act, 'r18', 1, torch.float32)
    _, em, pm = R.chain_grads(enc, pol, obs, done, act, 'r18', 1, torch.float32, order='frame_major_view')
    for name, g64, g32, gm in (('encoder', e64, e32, em), ('policy', p64, p32, pm)):
        ok, d, d32 = R.accept(R.cat(gm), R.cat(g32), R.cat(g64))
        print('\n[chain %s] frame-major mutant rel-L2 to float64 %.3e, torch fp32 %.3e' % (name, d, d32))
        assert R.accept(R.cat(g32), R.cat(g32), R.cat(g64))[0] and not ok, (name, d, d32)


@pytest.mark.parametrize('name,gb_per_frame', [('resnet18', 0.03), ('resnet50', 0.14)])
def test_trainer_workspace_bytes(name, gb_per_frame):
    b4, b6, b8 = (E.trainer_workspace_bytes(name, n) for n in (4, 6, 8))
    assert 0 < b4 < b6 < b8
    per = (b8 - b4) / 4.0
    const = b4 - 4 * per
    assert abs(b6 - (const + 6 * per)) <= 0.01 * b6                 # linear in max_batch, apart from a constant (weights-sized scratch)
    assert 0 <= const < b4
    assert gb_per_frame / 2 <= per / 1e9 <= gb_per_frame * 2, per / 1e9


def test_trainer_refuses_a_batch_whose_tensors_pass_2_gib_and_names_the_largest():
    # resnet50: the zero-filled grid of layer2.0's stride-2 data gradients, 56 x 56 x 512 floats = 6.4 MB per frame; resnet18: conv1's output, 3.2 MB
    for name, frames in (('resnet50', 334), ('resnet18', 668)):
        assert E.trainer_workspace_bytes(name, frames) > 0
        assert E.trainer_workspace_bytes(name, frames + 1) is None
        assert 'largest max_batch is %d frames' % frames in _lib.last_error()
    from pvr_habitat_amd.main_bc_finetune import largest_fitting_frames
    assert largest_fitting_frames('resnet50', 6400, 1 << 40) == 334


def _flags(tmp_path, *extra):
    from pvr_habitat_amd.arguments import make_parser
    return make_parser().parse_args(['--data_path', str(tmp_path), '--save_path', str(tmp_path / 'out'), '--env', 'scene', '--to_env', 'scene',
                                     '--train_embedding', '--disable_pretrained_embedding', '--unroll_length', '3', '--batch_size', '2'] + list(extra))


def test_driver_refuses_an_untrainable_name(tmp_path):
    from pvr_habitat_amd import main_bc_finetune as Fz
    with pytest.raises(NotImplementedError, match="training the embedding 'resnet50_l3' is not built"):
        Fz.run(_flags(tmp_path, '--embedding_name', 'resnet50_l3'))


def test_driver_refuses_a_world_size_above_one(tmp_path, monkeypatch):
    from pvr_habitat_amd import main_bc_finetune as Fz
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(NotImplementedError, match='data-parallel encoder training is not built'):
        Fz.run(_flags(tmp_path, '--embedding_name', 'resnet18'))


def test_driver_refuses_adam_and_momentum_on_the_fused_path(tmp_path):
    from pvr_habitat_amd import main_bc_finetune as Fz
    with pytest.raises(NotImplementedError, match='--optimizer adam and --momentum != 0 are not built'):
        Fz.run(_flags(tmp_path, '--embedding_name', 'resnet18', '--optimizer', 'adam'))
    with pytest.raises(NotImplementedError, match='--optimizer adam and --momentum != 0 are not built'):
        Fz.run(_flags(tmp_path, '--embedding_name', 'resnet18', '--momentum', '0.9'))
