"""The bconv planner honours a forced tiling, and the sweep's shapes reach
every instance of bconv_kernel<E, CV, NSUB, MPW, NPF, MODE> (no device needed:
planning is host code).

Each case is planned under every HCU_BCONV_FORCE="CK,NSUB,MPW[,NPF]" with
HCU_CONV2_LOG=1 and the planner's log lines are read back.  A plan counts
only if its logged CK / NSUB / MPW / NPF are the forced ones and the call
succeeded.  (A convolution that has no candidate under the force is planned as
if the variable were unset, and a forced NPF below the halo elements per
thread is replaced by the planner's depth: neither counts.)  The reached sets
asserted here are what tests/test_gpu_bconv_tilings.py then holds to the fp64
reference instance by instance."""
import ctypes

import pytest

from hcunet_amd import _lib
from tests import bconv_tilings as bt


@pytest.fixture
def planner_env(monkeypatch):
    monkeypatch.setenv('HCU_CONV2_LOG', '1')
    monkeypatch.setenv('HCU_BCONV_TUNE', '0')
    return monkeypatch


def _sweep_ops(bf16, env, capfd):
    """{(case index, role): {instance: set of ksplit}} over the force sweep."""
    L = _lib.lib()
    reached = {}
    for i, case in enumerate(bt.OP_CASES[bf16]):
        d = bt.op_desc(case, bf16)
        for fs, want in bt.forces(bf16):
            env.setenv('HCU_BCONV_FORCE', fs)
            capfd.readouterr()
            n = L.hcu_conv_scratch_bytes(ctypes.byref(d))
            plans = bt.parse_plans(capfd.readouterr().err)
            if n == 0:
                continue
            for p in plans:
                assert p['es'] == (2 if bf16 else 4)
                if bt.honoured(p, want):
                    reached.setdefault((i, bt.op_role(p, case)), {}).setdefault(p['inst'], set()).add(p['ks'])
    return reached


def _sweep_chain(C, dims, bf16, env, capfd):
    """{role: {instance: set of ksplit}} of one chain case."""
    reached = {r: {} for r in bt.CHAIN_ROLES}
    for fs, want in bt.forces(bf16):
        env.setenv('HCU_BCONV_FORCE', fs)
        capfd.readouterr()
        rc = bt.chain_plan_rc(C, dims, bf16)
        plans = bt.parse_plans(capfd.readouterr().err)
        if rc != 0:
            continue
        # (a role that did not plan bconv at all logs no line: roles unknown)
        if len(plans) != len(bt.CHAIN_ROLES):
            continue
        for role, p in zip(bt.CHAIN_ROLES, plans):
            if bt.honoured(p, want):
                reached[role].setdefault(p['inst'], set()).add(p['ks'])
    return reached


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_per_op_cases_reach_every_instance(bf16, planner_env, capfd):
    reached = _sweep_ops(bf16, planner_env, capfd)
    counts = [(len(reached.get((i, 'fwd'), {})), len(reached.get((i, 'dgrad'), {})))
              for i in range(len(bt.OP_CASES[bf16]))]
    print('honoured instances per case (fwd, dgrad):', counts)
    union, role = {}, {'fwd': set(), 'dgrad': set()}
    for (i, r), insts in reached.items():
        role[r] |= set(insts)
        for inst, ks in insts.items():
            union.setdefault(inst, set()).update(ks)
    ks1 = {i for i, ks in union.items() if 1 in ks}
    ksn = {i for i, ks in union.items() if max(ks) > 1}
    want = bt.ALL - bt.EXCLUDED[(bf16, '')]
    assert set(union) == want, sorted(want - set(union))
    assert ks1 == want, sorted(want - ks1)                     # every instance without a K split
    assert ksn == bt.ALL - bt.CHAIN_12x11x4_REFUSED, sorted(bt.ALL - ksn)   # and most with one
    assert role['fwd'] == want
    assert role['dgrad'] == bt.ALL - bt.CHAIN_12x11x4_REFUSED, sorted(bt.ALL - role['dgrad'])
    assert counts == bt.OP_REACHED[bf16]


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_chain_cases_reach_every_instance(bf16, planner_env, capfd):
    per_role = {r: set() for r in bt.CHAIN_ROLES}
    split_seen = {r: set() for r in bt.CHAIN_ROLES}
    for C, dims in bt.CHAIN_CASES[bf16]:
        reached = _sweep_chain(C, dims, bf16, planner_env, capfd)
        for r in bt.CHAIN_ROLES:
            got = set(reached[r])
            assert got == bt.chain_expected(dims), (C, dims, r, sorted(bt.ALL - got))
            for inst, ks in reached[r].items():
                assert all(k > 1 for k in ks) if bt.chain_ksplit(C) else ks == {1}, (C, dims, r, inst, ks)
                split_seen[r].add((inst, bt.chain_ksplit(C)))
            per_role[r] |= got
    # every convolution role of the chains (mode 0 and the ',bnb' input
    # gradient) reaches every instance, with a K split and without
    for r in bt.CHAIN_ROLES:
        mode = ',bnb' if r == bt.BNB_ROLE else ''
        want = bt.ALL - bt.EXCLUDED[(bf16, mode)]
        assert per_role[r] == want, (r, sorted(want - per_role[r]))
        assert split_seen[r] == {(i, s) for i in want for s in (False, True)}, r


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_ncx_network_plans_every_first_layer_instance(bf16, planner_env, capfd):
    """The small U-Net of the ',ncx' sweep plans under each of its 27 forces,
    its first convolution as the forced instance in the form the NCXYZ staging
    needs (one channel group, prefetched halo, no K split)."""
    from hcat.unet import Unet_Constructor
    from hcunet_amd.unet import spec_struct
    L = _lib.lib()
    spec = _lib.UnetSpec.from_buffer_copy(spec_struct(Unet_Constructor(**bt.NCX_KW)))
    spec.compute_dtype = _lib.HCU_BF16 if bf16 else _lib.HCU_F32
    B, _, X, Y, Z = bt.NCX_SHAPE
    reached = set()
    for fs, want in bt.ncx_forces(bf16):
        planner_env.setenv('HCU_BCONV_FORCE', fs)
        capfd.readouterr()
        h = ctypes.c_void_p()
        rc = L.hcu_unet_plan_create_ex(ctypes.byref(spec), B, X, Y, Z, 0, ctypes.byref(h))
        plans = bt.parse_plans(capfd.readouterr().err)
        assert rc == 0, (fs, _lib.last_error())
        L.hcu_unet_plan_destroy(h)
        first = plans[0]   # down conv1 of level 0 is planned first
        assert (first['IX'], first['IY'], first['IZ'], first['ICs']) == (X, Y, Z, bt.vec(bf16)), first
        assert bt.honoured(first, want) and first['ks'] == 1 and first['nph'] == 1 and first['NPF'] > 0, (fs, first)
        reached.add(first['inst'])
    assert reached == bt.NCX_INSTANCES - bt.EXCLUDED[(bf16, ',ncx')]


def test_exclusions_are_named_and_refused(planner_env, capfd):
    """An instance may be missing from the sweeps only if EXCLUDED names it and
    the planner refuses it for every case: at most 3 per (element type, mode)."""
    for (bf16, mode), insts in bt.EXCLUDED.items():
        assert len(insts) <= 3 and insts <= bt.ALL, (bf16, mode)
        for inst in insts:
            fs = '%d,%d,%d,%d' % ((inst[0] * bt.vec(bf16),) + tuple(inst[1:]))
            planner_env.setenv('HCU_BCONV_FORCE', fs)
            capfd.readouterr()
            for case in bt.OP_CASES[bf16]:
                d = bt.op_desc(case, bf16)
                _lib.lib().hcu_conv_scratch_bytes(ctypes.byref(d))
            for C, dims in bt.CHAIN_CASES[bf16]:
                bt.chain_plan_rc(C, dims, bf16)
            plans = bt.parse_plans(capfd.readouterr().err)
            assert not [p for p in plans if p['inst'] == inst], (bf16, mode, inst)
