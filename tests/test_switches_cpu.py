"""CPU checks of the encoder's switch contract: every A/B switch of the encoder path is read from the environment in ONE place
(encoder.hip: read_switches, into PlanSwitches) - no kernel file reads it on its own, at first use or per launch."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pvr_habitat_amd', 'csrc')
# getenv outside the encoder's switch table: roctx ranges, host-backend threads, the policy handle's switches, an experiment kernel's stamps
ALLOWED = {'api.hip', 'host_encoder.hip', 'host_math.h', 'policy.hip', 'conv_w4.hip'}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, head):
    """text of the brace block that follows the first occurrence of `head`"""
    i = src.index('{', src.index(head))
    depth = 0
    for j in range(i, len(src)):
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
    raise AssertionError('unbalanced braces after ' + head)


def test_encoder_path_reads_the_environment_only_in_read_switches():
    hits = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')):
            n = sum('getenv' in line for line in _src(name).splitlines())
            if n:
                hits[name] = n
    assert set(hits) - ALLOWED == {'encoder.hip'}, hits
    assert hits['encoder.hip'] == 1, hits
    assert 'getenv' in _body(_src('encoder.hip'), 'void read_switches(PlanSwitches &sw)')


def test_plan_switches_is_the_one_list():
    """each member of PlanSwitches names its variable and default in its declaration, and read_switches reads exactly those"""
    decl = _body(_src('encoder_internal.h'), 'struct PlanSwitches')
    members = {m: (env, int(d)) for m, d, env in re.findall(r'int (\w+) = (-?\d+);\s*// (PVR_\w+)', decl)}
    reads = {m: (env, int(d)) for m, env, d in re.findall(r'sw\.(\w+) = get\("(PVR_\w+)", (-?\d+)\)', _body(_src('encoder.hip'), 'void read_switches'))}
    assert len(members) == len(re.findall(r'^\s*int ', decl, re.M)) and members == reads, (set(members.items()) ^ set(reads.items()))


def test_the_planner_is_host_code_and_nothing_in_csrc_matches_names():
    """encoder_plan.hip decides the plan from the desc and the switches: it calls no HIP runtime function and no launcher, so pvr_encoder_create can run it
    on a machine without a GPU; no file of csrc/ recognises blocks by state-dict names (the builders record roles and blocks: OpRole, Block)"""
    plan = re.sub(r'/\*.*?\*/', '', re.sub(r'//[^\n]*', '', _src('encoder_plan.hip')), flags=re.S)
    assert 'plan_encoder' in plan and len(plan) > 10000
    assert not re.findall(r'\bhip[A-Z]\w*\(', plan)
    assert not re.findall(r'\blaunch_(?!kind_name)\w+\(', plan)
    assert not [name for name in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, name)) and 'ends_with(' in _src(name)]


def test_every_plan_switch_is_read_by_the_code_it_switches():
    """a PlanSwitches member that only read_switches and pvr_encoder_debug_set_switch touch switches nothing: every member is read (not merely assigned)
    somewhere else in csrc/"""
    decl = _body(_src('encoder_internal.h'), 'struct PlanSwitches')
    members = re.findall(r'^\s*int (\w+) = ', decl, re.M)
    assert len(members) > 20
    text = ''
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')):
            src = _src(name)
            if name == 'encoder.hip':
                for head in ('void read_switches(PlanSwitches &sw)', 'pvr_status pvr_encoder_debug_set_switch('):
                    src = src.replace(_body(src, head), '{}')
            text += re.sub(r'/\*.*?\*/', '', re.sub(r'//[^\n]*', '', src), flags=re.S)
    dead = [m for m in members if not re.search(r'\bsw\.%s\b(?!\s*=[^=])' % m, text)]
    assert not dead, dead
