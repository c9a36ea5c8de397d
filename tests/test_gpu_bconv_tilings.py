"""Numerical parity of every bconv tiling instance, not only the planned one.

plan_bconv picks one of the 108 (CV, NSUB, MPW, NPF) instances of
bconv_kernel<E, CV, NSUB, MPW, NPF, MODE> per convolution, so the rest of the
suite runs about a dozen of them.  Here each case runs under every
HCU_BCONV_FORCE="CK,NSUB,MPW,NPF" (read per plan) and is compared with the
fp64 reference of the same operation, once per case:

  * per-op (MODE 0): hcu_conv_fwd_cl / hcu_conv_dgrad_cl as in
    tests/test_gpu_ops.py, with that file's operands and tolerances;
  * chains (MODE 0 and ',bnb', with and without the K-split reduce): two
    Conv3d + BatchNorm3d + ReLU through hcunet_amd.chain.Chain in training
    mode: output, dx and every parameter gradient;
  * ',ncx' (MODE 2): a small U-Net whose first convolution stages the NCXYZ
    volume, bitwise against the layout-pass run (HCU_NCX=0) of the same force,
    which runs the MODE 0 instance held to fp64 above.

A comparison counts for an instance only if hcu_timing_report shows the exact
kernel label the force implies; tests/test_bconv_tilings.py establishes which
instances each case reaches, and the labels seen here must be those.  A HIP
error ends the session: nothing more is started on the device after it."""
import contextlib
import copy
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from hcunet_amd import _lib
from hcunet_amd.chain import Chain, FlatParams
from tests import bconv_tilings as bt
from tests.helpers import out_dims, rup4, scratch_for, stream, to_cl
from tests.test_gpu_bf16 import SLACK
from tests.test_gpu_chain import _Holder, _check
from tests.test_gpu_ops import _bf, _conv_ref, _rup8, _to_cl_bf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ['f32', 'bf16']
_RESULTS = {}


@pytest.fixture
def sweep(monkeypatch, request):
    """Launch labels on (off again in a finalizer); returns the monkeypatch
    that sets the force."""
    L = _lib.lib()
    _lib.check(L.hcu_timing_enable(1024))
    request.addfinalizer(L.hcu_timing_disable)
    monkeypatch.delenv('HCU_BCONV_FORCE', raising=False)
    return monkeypatch


@contextlib.contextmanager
def _device_guard(what):
    """A HIP error (an HCU_ERR_HIP return or a failed synchronize) ends the
    pytest session at once instead of failing one test after another on a
    device in an unknown state."""
    try:
        yield
    except RuntimeError as e:
        pytest.exit('device error under %s: %s' % (what, e), returncode=3)


def _labels(bf16, want, rep):
    """(launches of the forced instance in mode 0, with ',bnb', of the K-split
    reduce) in one timing report."""
    n = lambda k: rep.get(k, {}).get('count', 0)   # noqa: E731
    return n(bt.label(bf16, want)), n(bt.label(bf16, want, ',bnb')), n(bt.reduce_label(bf16))


# ---------------------------------------------------------------------------
# per-op, MODE 0
@functools.lru_cache(maxsize=None)
def _op_reference(bf16, idx):
    """Operands and fp64 results of a per-op case, as tests/test_gpu_ops.py
    builds them (bf16: operands rounded to bf16 before the fp64 reference)."""
    B, Cin, Cout, X, Y, Z, k, s, tr = bt.OP_CASES[bf16][idx]
    rnd = _bf if bf16 else (lambda t: t)
    if not tr:
        if bf16:
            g = torch.Generator().manual_seed(5)
            x = torch.randn(B, Cin, X, Y, Z, generator=g, dtype=torch.float64)
            w = torch.randn(Cout, Cin, *k, generator=g, dtype=torch.float64) * (1.0 / (Cin * 9) ** 0.5)
            b = torch.randn(Cout, generator=g, dtype=torch.float64)
        else:
            x, w, b = _conv_ref(B, Cin, Cout, X, Y, Z, k, (1, 1, 1), 1)
        gseed = 7
    else:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(B, Cin, X, Y, Z, generator=g, dtype=torch.float64)
        w = torch.randn(Cin, Cout, *k, generator=g, dtype=torch.float64) * (1.0 / Cin ** 0.5 if bf16 else 0.2)
        b = torch.randn(Cout, generator=g, dtype=torch.float64)
        gseed = 3
    x = rnd(x)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, rnd(w), b))
    y = F.conv_transpose3d(xr, wr, br, stride=s) if tr else F.conv3d(xr, wr, br)
    gy = rnd(torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed), dtype=torch.float64))
    y.backward(gy)
    cl = _to_cl_bf if bf16 else to_cl
    ref = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous().cuda()   # noqa: E731  (fp64, channels-last)
    return dict(xcl=cl(x), gcl=cl(gy), wd=w.float().cuda().contiguous(), bd=b.float().cuda(),
                y=ref(y), dx=ref(xr.grad), ymax=y.abs().max().item(), dxmax=xr.grad.abs().max().item())


def _op_tol(bf16, scale):
    return 1e-2 * scale if bf16 else 2e-6 * scale + 1e-6


def _op_result(bf16, idx, env):
    """Sweeps one per-op case: {'bad': mismatches, 'fwd' / 'dgrad': {instance:
    the K-split reduce ran}} for the launches confirmed by their label."""
    key = ('op', bf16, idx)
    if key in _RESULTS:
        return _RESULTS[key]
    case = bt.OP_CASES[bf16][idx]
    B, Cin, Cout, X, Y, Z = case[:6]
    r = _op_reference(bf16, idx)
    L = _lib.lib()
    rup = _rup8 if bf16 else rup4
    dt = torch.bfloat16 if bf16 else torch.float32
    res = {'bad': [], 'fwd': {}, 'dgrad': {}}
    env.delenv('HCU_BCONV_FORCE', raising=False)   # the planner's own tiling first
    for fs, want in [(None, None)] + bt.forces(bf16, npfs=bt.NPFS):
        if fs is not None:
            env.setenv('HCU_BCONV_FORCE', fs)
        d = bt.op_desc(case, bf16)
        od = out_dims(d)
        assert (B,) + od == tuple(r['y'].shape[:4])
        with _device_guard('HCU_BCONV_FORCE=%s, %r' % (fs, case)):
            sc = scratch_for(d)
            ycl = torch.full((B, *od, rup(Cout)), float('nan'), device='cuda', dtype=dt)
            _lib.check(L.hcu_conv_fwd_cl(ctypes.byref(d), _lib.ptr(r['xcl']), _lib.ptr(r['wd']), _lib.ptr(r['bd']),
                                         _lib.ptr(ycl), _lib.ptr(sc), sc.numel(), stream()))
            torch.cuda.synchronize()
            rep_f = _lib.timing_report()
            dx = torch.full((B, X, Y, Z, rup(Cin)), float('nan'), device='cuda', dtype=dt)
            _lib.check(L.hcu_conv_dgrad_cl(ctypes.byref(d), _lib.ptr(r['gcl']), _lib.ptr(r['wd']), _lib.ptr(dx),
                                           _lib.ptr(sc), sc.numel(), stream()))
            torch.cuda.synchronize()
            rep_d = _lib.timing_report()
            checks = []
            for role, got, C, refv, scale, rep in (('fwd', ycl, Cout, r['y'], r['ymax'], rep_f),
                                                   ('dgrad', dx, Cin, r['dx'], r['dxmax'], rep_d)):
                err = (got[..., :C].double() - refv).abs().max().item()
                pad_ok = bool(torch.all(got[..., C:] == 0)) if got.shape[-1] != C else True
                checks.append((role, err, _op_tol(bf16, scale), pad_ok, rep))
        for role, err, tol, pad_ok, rep in checks:
            if not err <= tol or not pad_ok:
                res['bad'].append((fs, role, 'err %.3g tol %.3g' % (err, tol), 'padding zero: %s' % pad_ok))
            if want is not None:
                n0, nb, nr = _labels(bf16, want, rep)
                assert nb == 0 and n0 <= 1, (fs, role, sorted(rep))
                if n0:
                    res[role][want] = nr > 0
    _RESULTS[key] = res
    return res


@pytest.mark.parametrize('idx', range(4))
@pytest.mark.parametrize('bf16', [False, True], ids=IDS)
def test_per_op_every_forced_tiling(bf16, idx, sweep):
    """Forward and input gradient of one per-op case under every forced tiling
    (and the planner's own) against fp64, NaN-prefilled outputs, padding
    channels zero; the instances confirmed by their launch label are exactly
    as many as the planner test records for the case."""
    res = _op_result(bf16, idx, sweep)
    assert not res['bad'], (len(res['bad']), res['bad'][:12])
    assert (len(res['fwd']), len(res['dgrad'])) == bt.OP_REACHED[bf16][idx]


@pytest.mark.parametrize('bf16', [False, True], ids=IDS)
def test_per_op_sweep_covers_every_instance(bf16, sweep):
    """Over the per-op cases every instance launched in MODE 0, each also
    without the K-split reduce, and the reduce ran behind most of them."""
    seen = {}
    for idx in range(len(bt.OP_CASES[bf16])):
        res = _op_result(bf16, idx, sweep)
        for role in ('fwd', 'dgrad'):
            for inst, reduced in res[role].items():
                seen.setdefault(inst, set()).add(reduced)
    want = bt.ALL - bt.EXCLUDED[(bf16, '')]
    assert set(seen) == want, sorted(want - set(seen))
    assert {i for i, s in seen.items() if False in s} == want
    assert {i for i, s in seen.items() if True in s} == bt.ALL - bt.CHAIN_12x11x4_REFUSED


# ---------------------------------------------------------------------------
# chains: MODE 0 and ',bnb', with and without the K split
CANCELLED = ('m.0.bias', 'm.2.bias')   # conv biases ahead of a train-mode BatchNorm: exact gradient 0


def _rl2(a, b, denom=None):
    a, b = a.double(), b.double()
    return ((a - b).norm() / max((b if denom is None else denom.double()).norm().item(), 1e-30)).item()


def _chain_forward(mods, x):
    """relu(bn(conv(.))) twice; returns the output and the two pre-BatchNorm
    tensors."""
    c0 = mods[0](x)
    c1 = mods[2](torch.relu(mods[1](c0)))
    return torch.relu(mods[3](c1)), c0, c1


@functools.lru_cache(maxsize=None)
def _chain_reference(bf16, idx):
    C, dims = bt.CHAIN_CASES[bf16][idx]
    torch.manual_seed(20 + idx)
    mods = [nn.Conv3d(C, C, bt.CHAIN_K), nn.BatchNorm3d(C), nn.Conv3d(C, C, bt.CHAIN_K), nn.BatchNorm3d(C)]
    with torch.no_grad():
        for bn in (mods[1], mods[3]):
            bn.weight.copy_(1.0 + 0.2 * torch.randn(C))
            bn.bias.copy_(0.2 * torch.randn(C))
    x = torch.randn((1, C) + tuple(dims), generator=torch.Generator().manual_seed(1))
    names = [k for k, _ in _Holder(*mods).named_parameters()]

    def run(ms, xin, gdt):
        y, c0, c1 = _chain_forward(ms, xin)
        c0.retain_grad()
        c1.retain_grad()
        g = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
        (y.to(gdt) * g.to(gdt)).sum().backward()
        t = {'out': y.detach(), 'dx': xin.grad}
        t.update({k: p.grad for k, p in _Holder(*ms).named_parameters()})
        return t, g, (c0.grad, c1.grad)

    ref, g, dz = run([copy.deepcopy(m).double() for m in mods], x.double().requires_grad_(True), torch.float64)
    out = dict(mods=mods, x=x, g=g, names=names, ref={k: v.cuda() for k, v in ref.items()})
    if bf16:
        # the same modules under torch's own bf16 policy: the yardstick of
        # tests/test_gpu_bf16.py.  The BatchNorm-cancelled conv biases (exact
        # gradient 0: a relative distance means nothing) are measured against
        # the sum they cancel from, sum |dz| per channel.
        with torch.autocast('cpu', dtype=torch.bfloat16):
            auto, _, _ = run([copy.deepcopy(m).float() for m in mods], x.clone().requires_grad_(True),
                             torch.float32)
        out['denom'] = {k: z.abs().sum(dim=(0, 2, 3, 4)).cuda() for k, z in zip(CANCELLED, dz)}
        out['auto'] = {k: _rl2(auto[k].cuda(), out['ref'][k], out['denom'].get(k)) for k in ref}
    return out


def _chain_verdict(bf16, r, got):
    """(failures, worst distance / bar, worst distance / torch autocast's
    distance over the tensors with a non-zero exact value) of one run."""
    if not bf16:
        errs = {k: ((got[k].double() - v).abs().max().item(), v.abs().max().item()) for k, v in r['ref'].items()}
        worst = max(e / (1e-4 if k in CANCELLED else 1e-4 * max(m, 1e-3)) for k, (e, m) in errs.items())
        try:
            _check(errs, rel=1e-4, cancelled=CANCELLED)
        except AssertionError as e:
            return [str(e)[:400]], worst, 0.0
        return [], worst, 0.0
    bad, worst, worst_auto = [], 0.0, 0.0
    for k, v in r['ref'].items():
        ours = _rl2(got[k], v, r['denom'].get(k))
        bar = SLACK * r['auto'][k] + (1e-3 if k == 'out' else 1e-2)
        worst = max(worst, ours / bar)
        if k not in CANCELLED:
            worst_auto = max(worst_auto, ours / r['auto'][k])
        if not ours <= bar or (k == 'out' and not ours <= 0.3):
            bad.append((k, 'ours %.3g torch autocast %.3g bar %.3g' % (ours, r['auto'][k], bar)))
    return bad, worst, worst_auto


def _chain_result(bf16, idx, env):
    key = ('chain', bf16, idx)
    if key in _RESULTS:
        return _RESULTS[key]
    C, dims = bt.CHAIN_CASES[bf16][idx]
    r = _chain_reference(bf16, idx)
    holder = _Holder(*[copy.deepcopy(m).float() for m in r['mods']]).cuda()
    flat = FlatParams(holder)
    m = holder.m
    gdev = r['g'].float().cuda()
    res = {'bad': [], 'default_bad': None, 'plain': {}, 'bnb': {}, 'worst': 0.0, 'worst_auto': 0.0}
    env.delenv('HCU_BCONV_FORCE', raising=False)   # the planner's own tiling first
    for fs, want in [(None, None)] + bt.forces(bf16, npfs=bt.NPFS):
        if fs is not None:
            env.setenv('HCU_BCONV_FORCE', fs)
        for p in holder.parameters():
            p.grad = None
        with _device_guard('HCU_BCONV_FORCE=%s, chain C%d %r' % (fs, C, dims)):
            # (a new Chain: its plans are kept per input shape, not per force)
            ch = Chain(flat, C, [('conv', m[0], m[1], False), ('conv', m[2], m[3], False)])
            xg = r['x'].cuda().requires_grad_(True)
            out = ch(xg, True, bf16)
            (out * gdev).sum().backward()
            torch.cuda.synchronize()
            rep = _lib.timing_report()
            got = {'out': out.detach(), 'dx': xg.grad}
            got.update({k: p.grad for k, p in holder.named_parameters()})
            bad, worst, worst_auto = _chain_verdict(bf16, r, got)
        res['worst'] = max(res['worst'], worst)
        res['worst_auto'] = max(res['worst_auto'], worst_auto)
        if want is None:
            res['default_bad'] = bad
            continue
        if bad:
            res['bad'].append((fs, bad))
        n0, nb, nr = _labels(bf16, want, rep)
        # c0 forward, c1 forward and c0's input gradient in mode 0, c1's input
        # gradient with the BatchNorm backward of c0's BatchNorm
        if n0 == 3:
            res['plain'][want] = nr > 0
        if nb == 1:
            res['bnb'][want] = nr > 0
    _RESULTS[key] = res
    return res


@pytest.mark.parametrize('idx', range(4))
@pytest.mark.parametrize('bf16', [False, True], ids=IDS)
def test_chain_every_forced_tiling(bf16, idx, sweep):
    """Conv3d + BatchNorm3d + ReLU twice, training mode, under every forced
    tiling: output, dx and the gradients of both weights, biases, gammas and
    betas against fp64.  fp32: tests/test_gpu_chain.py's bar for such a chain
    (1e-4 of each tensor's largest element, 1e-4 absolute for the cancelled
    conv biases).  bf16: tests/test_gpu_bf16.py's criterion per tensor: the
    relative L2 distance to fp64 within SLACK = 1.5 of the distance of the
    same modules under torch.autocast('cpu', bfloat16), plus 1e-3 (output) or
    1e-2 (gradients).  The planner's own tiling has to pass the same bar first:
    failing there would be the bar's fault, not a tiling's.

    Measured on MI355X, worst over the four cases, all 108 tilings and the
    planner's own, and all tensors: bf16 distance / torch autocast's distance
    1.162 (SLACK allows 1.5; C96 8x8x2; 0.994 / 1.076 / 0.982 in the other
    cases), bf16 distance / bar 0.670; fp32 error / bar 0.200."""
    res = _chain_result(bf16, idx, sweep)
    C, dims = bt.CHAIN_CASES[bf16][idx]
    print('chain C%d %r %s: worst distance / bar %.3f, / torch autocast %.3f'
          % (C, dims, bt.TAG[bf16], res['worst'], res['worst_auto']))
    assert not res['default_bad'], ('the planned tiling misses the bar', res['default_bad'])
    assert not res['bad'], (len(res['bad']), res['bad'][:8])
    want = bt.chain_expected(dims)
    assert set(res['plain']) == want, sorted(want ^ set(res['plain']))
    assert set(res['bnb']) == want, sorted(want ^ set(res['bnb']))
    assert set(res['bnb'].values()) == {bt.chain_ksplit(C)}


@pytest.mark.parametrize('bf16', [False, True], ids=IDS)
def test_chain_sweep_covers_bnb_and_reduce(bf16, sweep):
    """Over the chain cases every instance launched with the fused
    BatchNorm-backward epilogue (',bnb') and in mode 0, each with the K-split
    reduce behind it and without."""
    for mode, key in ((',bnb', 'bnb'), ('', 'plain')):
        seen = {}
        for idx in range(len(bt.CHAIN_CASES[bf16])):
            for inst, reduced in _chain_result(bf16, idx, sweep)[key].items():
                seen.setdefault(inst, set()).add(reduced)
        want = bt.ALL - bt.EXCLUDED[(bf16, mode)]
        assert set(seen) == want, (mode, sorted(want - set(seen)))
        assert all(s == {False, True} for s in seen.values()), mode


# ---------------------------------------------------------------------------
# ',ncx' (MODE 2): HCU_NCX is read once per process, so each arm is a child
NCX_CHILD = r'''
import hashlib, json, os, sys, torch
sys.path.insert(0, %(root)r)
from hcat.loss import cross_entropy
from hcat.unet import Unet_Constructor
from hcunet_amd import _lib
from oracle import inputs
from tests import bconv_tilings as bt
bf16 = os.environ['HCU_TEST_BF16'] == '1'
ncx = os.environ['HCU_NCX'] == '1'
x = torch.from_numpy(inputs.make_x(bt.NCX_SHAPE)).cuda()
if bf16:
    x = x.bfloat16()
L = _lib.lib()
_lib.check(L.hcu_timing_enable(4096))
res = {}
for fs, want in bt.ncx_forces(bf16):
    os.environ['HCU_BCONV_FORCE'] = fs
    torch.manual_seed(0)
    m = Unet_Constructor(**bt.NCX_KW).cuda().train()
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
        out = m(x)
    ms = (x.shape[0], 1) + tuple(out.shape[2:])
    loss = cross_entropy(out, torch.from_numpy(inputs.make_mask(ms)).cuda(),
                         torch.from_numpy(inputs.make_pwl(ms)).cuda(), method='pixel')
    loss.backward()
    torch.cuda.synchronize()
    rep = _lib.timing_report()
    kernels = sorted(k for k in rep if k.startswith('bconv_kernel'))
    assert (bt.label(bf16, want, ',ncx') in rep) == ncx, (fs, kernels)
    assert ncx or (bt.label(bf16, want) in rep and not [k for k in kernels if 'ncx' in k]), (fs, kernels)
    ts = [out.detach()] + [p.grad for p in m.parameters()]
    assert all(bool(torch.isfinite(t).all()) for t in ts), fs
    res[fs] = [hashlib.sha256(t.float().cpu().contiguous().numpy().tobytes()).hexdigest() for t in ts]
L.hcu_timing_disable()
json.dump(res, open(%(out)r, 'w'))
'''


@pytest.mark.parametrize('bf16', ['0', '1'], ids=IDS)
def test_ncx_every_forced_first_layer(tmp_path, bf16):
    """The first convolution staging the NCXYZ volume itself (HCU_NCX=1) under
    each of the 27 (CV 1, NSUB, MPW, NPF > 0) instances it has, against the
    channels-last layout pass (HCU_NCX=0) of the same force: the output and
    every gradient of one training step of a fresh small U-Net bitwise equal
    (fp32 plan; bf16 plan with a bf16 volume).  Each child confirms its
    first-layer kernel by the launch label; the second child only starts when
    the first ended clean."""
    got = []
    for ncx in ('0', '1'):
        out = str(tmp_path / ('ncx%s.json' % ncx))
        env = dict(os.environ, HCU_NCX=ncx, HCU_TEST_BF16=bf16, HCU_BCONV_TUNE='0')
        env.pop('HCU_BCONV_FORCE', None)
        r = subprocess.run([sys.executable, '-c', NCX_CHILD % dict(root=ROOT, out=out)], env=env,
                           capture_output=True, text=True, timeout=240)
        if r.returncode != 0 and 'AssertionError' not in r.stderr:   # a device error or a crash, not a finding
            pytest.exit('the HCU_NCX=%s child died (%d): %s' % (ncx, r.returncode, r.stderr[-2000:]), returncode=3)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(out) as f:
            got.append(json.load(f))
    lay, stg = got
    forces = [fs for fs, _ in bt.ncx_forces(bf16 == '1')]
    assert sorted(lay) == sorted(stg) == sorted(forces) and len(forces) == 27
    bad = [(fs, k) for fs in forces for k, (a, b) in enumerate(zip(lay[fs], stg[fs])) if a != b]
    assert not bad, bad[:8]
