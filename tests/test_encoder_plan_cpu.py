"""The encoder's launch plan, pinned on the CPU: pvr_encoder_create plans from the desc and the switches alone (csrc/encoder_plan.hip), so a handle that was
never finalized answers pvr_encoder_launch_name / pvr_encoder_launch_kernel for every batch size.  tests/golden/encoder_plans.json holds what FINALIZED
handles answered on the GPU at the commit named in its "recorded_at", before the planner moved to create: per configuration the launch names and, for
n = 1 .. 256, the kernel names, run-length encoded as [n_from, n_to, list]; "lists" holds each distinct list once, as indices into "names", and "runs" each
distinct run table once.  The fixture is a recording: it is never regenerated from the code under test."""
import ctypes as C
import json
import os
import re

import pytest

from pvr_habitat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pvr_habitat_amd', 'csrc')
ARCH = {'RESNET50': 0, 'RESNET50_L4': 1, 'RESNET50_L3': 2, 'CLIP_RN50': 9, 'RESNET18': 10, 'RESNET34': 11}
DTYPE = {'bf16': _lib.PVR_BF16, 'f16': _lib.PVR_F16, 'f32': _lib.PVR_F32}
DTYPES = {a: ('f16', 'bf16') if a == 'CLIP_RN50' else ('f16', 'bf16', 'f32') for a in ARCH}      # what pvr_encoder_create accepts
SWITCHED = (('RESNET50', 'f16'), ('RESNET50', 'bf16'), ('RESNET50_L3', 'f16'), ('RESNET50_L4', 'f16'))

with open(os.path.join(ROOT, 'tests', 'golden', 'encoder_plans.json')) as _f:
    GOLD = json.load(_f)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _planner_settings():
    """(variable, value) for every PlanSwitches member encoder_plan.hip reads: one non-default value each, and the extra values the fixture was asked for"""
    decl = _src('encoder_internal.h')
    decl = decl[decl.index('struct PlanSwitches'):decl.index('void read_switches')]
    members = {m: (env, int(d)) for m, d, env in re.findall(r'int (\w+) = (-?\d+);\s*// (PVR_\w+)', decl)}
    read = set(re.findall(r'\bsw\.(\w+)', re.sub(r'//[^\n]*', '', _src('encoder_plan.hip'))))
    assert read and read <= set(members), read - set(members)
    out = [(members[m][0], 0 if members[m][1] != 0 else 1) for m in sorted(read)]
    extra = {'conv_algo': 1, 'conv_wfrag': 2, 'frame_min_n': 1, 'smallk_div': 2}
    return out + [(members[m][0], v) for m, v in sorted(extra.items()) if m in read]


def _expected():
    """keys of the configurations the fixture must hold: defaults of every architecture x dtype x fusion x low latency, one planner switch at a time"""
    keys = []
    for a in ARCH:
        for dt in DTYPES[a]:
            keys += ['%s/%s/default/fusion=%d/ll=%d' % (a, dt, fu, ll) for fu in (1, 0) for ll in (0, 1)]
    for a, dt in SWITCHED:
        for env, v in _planner_settings():
            keys += ['%s/%s/%s=%d/fusion=created/ll=%d' % (a, dt, env, v, ll) for ll in (0, 1)]
    return keys


def _names(fn, h, *front):
    out, buf, i = [], C.create_string_buffer(256), 3
    while fn(h, *front, i, buf, 256) > 0:
        out.append(buf.value.decode())
        i += 1
    return out


def _plan_of_unfinalized_handle(cfg, monkeypatch):
    """(op_names, {n: kernel_names}) of a handle that is created, switched and destroyed - never finalized, no weights, no device"""
    L = _lib.lib()
    with monkeypatch.context() as m:                          # the switches are read once, in pvr_encoder_create
        for k, v in cfg['env'].items():
            m.setenv(k, str(v))
        h = C.c_void_p()
        d = _lib.EncoderDesc(arch=ARCH[cfg['arch']], dtype=DTYPE[cfg['dtype']], max_batch=GOLD['max_batch'], chunk=0, resize=256, crop=224)
        _lib.check(L.pvr_encoder_create(C.byref(d), C.byref(h)))
    try:
        if cfg['fusion'] is not None:
            _lib.check(L.pvr_encoder_debug_set_fusion(h, cfg['fusion']))
        _lib.check(L.pvr_encoder_set_low_latency(h, cfg['low_latency']))
        ops = [x for x in _names(L.pvr_encoder_launch_name, h) if x != 'pool/flatten']
        return ops, {n: _names(L.pvr_encoder_launch_kernel, h, n) for n in range(1, GOLD['max_batch'] + 1)}
    finally:
        L.pvr_encoder_destroy(h)


def _gold_list(i):
    return [GOLD['names'][j] for j in GOLD['lists'][i]]


def test_fixture_covers_every_architecture_dtype_and_planner_switch():
    missing = [k for k in _expected() if k not in GOLD['configs']]
    assert not missing, missing
    assert GOLD['max_batch'] == 256 and len(GOLD['recorded_at']) >= 7
    for k, c in GOLD['configs'].items():
        runs = GOLD['runs'][c['kernels']]
        assert runs[0][0] == 1 and runs[-1][1] == 256 and all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:])), k     # every batch size, once


@pytest.mark.parametrize('key', sorted(GOLD['configs']))
def test_unfinalized_handle_reports_the_recorded_plan(key, monkeypatch):
    cfg = GOLD['configs'][key]
    ops, kernels = _plan_of_unfinalized_handle(cfg, monkeypatch)
    assert ops == _gold_list(cfg['op_names'])
    for n0, n1, li in GOLD['runs'][cfg['kernels']]:
        want = _gold_list(li)
        for n in range(n0, n1 + 1):
            assert kernels[n] == want, (key, n)
