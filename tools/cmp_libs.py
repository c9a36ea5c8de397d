"""Bitwise comparison of two library builds on the same training steps (the
child process of tests/test_gpu_modes.py, 3 steps of a 5-level net):
  python tools/cmp_libs.py LIB_A LIB_B [--bf16] [--wide]
or, with --ops, on the per-op C-ABI: forward, input gradient and weight / bias
gradient of every case of tests/test_gpu_ops.py (y, dx, dw, db and the return
codes), the check that two builds write the same weight images:
  python tools/cmp_libs.py LIB_A LIB_B --ops [--env-a K=V,K=V --env-b K=V,K=V]"""
import argparse
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tests import test_gpu_modes as tm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('a')
ap.add_argument('b')
ap.add_argument('--bf16', action='store_true')
ap.add_argument('--wide', action='store_true', help='feature_sizes [32..512] (config-3 widths)')
ap.add_argument('--ops', action='store_true', help='the per-op entry points on the cases of tests/test_gpu_ops.py')
ap.add_argument('--env-a', default='', help='K=V[,K=V] for run a only (A/B of an environment switch)')
ap.add_argument('--env-b', default='', help='K=V[,K=V] for run b only')
args = ap.parse_args()

# One process per library: every case list of tests/test_gpu_ops.py through
# hcu_conv_{fwd,dgrad,wgrad}_cl on NaN-filled outputs; saves per case the
# return codes and (y, dx, dw, db).
OPS_CHILD = r'''
import ctypes, sys, torch
sys.path.insert(0, %(root)r)
from hcunet_amd import _lib
from tests import test_gpu_ops as T
from tests.helpers import desc, rup4, scratch_for, stream, to_cl
L = _lib.lib()
res = []
for cases, transposed, bf in ((T.CONV_CASES, 0, 0), (T.CONVT_CASES, 1, 0), (T.BF_CONV_CASES, 0, 1),
                              (T.BF_CONVT_CASES, 1, 1)):
    for case in cases:
        B, Cin, Cout, X, Y, Z, k = case[:7]
        groups = 1
        if transposed:
            d = desc(B, Cin, Cout, X, Y, Z, k, stride=case[7], transposed=1)
        elif len(case) > 7:
            groups = case[8]
            d = desc(B, Cin, Cout, X, Y, Z, k, dil=case[7], groups=groups)
        else:
            d = desc(B, Cin, Cout, X, Y, Z, k)
        if bf:
            d.dtype = _lib.HCU_BF16
        od = (ctypes.c_int * 3)()
        rc = [L.hcu_conv_out_dims(ctypes.byref(d), od)]
        if rc[0]:
            res.append((rc, []))
            continue
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, Cin, X, Y, Z, generator=g)
        gy = torch.randn(B, Cout, *od, generator=g)
        w = torch.randn(*((Cin, Cout) if transposed else (Cout, Cin // groups)), *k, generator=g) * 0.2
        b = torch.randn(Cout, generator=g)
        cl, rup, dt = (T._to_cl_bf, T._rup8, torch.bfloat16) if bf else (to_cl, rup4, torch.float32)
        xcl, gcl, wd, bd = cl(x), cl(gy), w.cuda().contiguous(), b.cuda()
        sc = scratch_for(d)
        y = torch.full((B, *od, rup(Cout)), float('nan'), device='cuda', dtype=dt)
        dx = torch.full((B, X, Y, Z, rup(Cin)), float('nan'), device='cuda', dtype=dt)
        dw, db = torch.full_like(wd, float('nan')), torch.full_like(bd, float('nan'))
        rc.append(L.hcu_conv_fwd_cl(ctypes.byref(d), _lib.ptr(xcl), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y),
                                    _lib.ptr(sc), sc.numel(), stream()))
        rc.append(L.hcu_conv_dgrad_cl(ctypes.byref(d), _lib.ptr(gcl), _lib.ptr(wd), _lib.ptr(dx), _lib.ptr(sc),
                                      sc.numel(), stream()))
        rc.append(L.hcu_conv_wgrad_cl(ctypes.byref(d), _lib.ptr(xcl), _lib.ptr(gcl), _lib.ptr(dw), _lib.ptr(db),
                                      _lib.ptr(sc), sc.numel(), stream()))
        torch.cuda.synchronize()
        res.append((rc, [t.cpu() for t in (y, dx, dw, db)]))
torch.save(res, %(out)r)
'''


def _kv(spec):
    return dict(kv.split('=', 1) for kv in spec.split(',') if kv)


def _run_ops(tmp_path, tag, env_extra):
    out = str(tmp_path / ('%s.pt' % tag))
    env = dict(os.environ, **env_extra)
    env['HCU_BCONV_TUNE'] = '0'   # measured tile choices may differ between processes (as tm._run)
    r = subprocess.run([sys.executable, '-c', OPS_CHILD % dict(root=ROOT, out=out)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out, weights_only=True)


def _bits(t):
    return t.contiguous().view(torch.uint8)


tmp = pathlib.Path(tempfile.mkdtemp())
if args.ops:
    ra = _run_ops(tmp, 'a', dict(HCU_LIB_PATH=args.a, **_kv(args.env_a)))
    rb = _run_ops(tmp, 'b', dict(HCU_LIB_PATH=args.b, **_kv(args.env_b)))
    diff = [(i, 'rc', ca, cb) for i, ((ca, _), (cb, _)) in enumerate(zip(ra, rb)) if ca != cb]
    diff += [(i, 'y dx dw db'.split()[k], (x.double() - y.double()).abs().max().item())
             for i, ((_, ta), (_, tb)) in enumerate(zip(ra, rb))
             for k, (x, y) in enumerate(zip(ta, tb)) if not torch.equal(_bits(x), _bits(y))]
    ran = sum(1 for rc, _ in ra if not any(rc))
    print(('bitwise equal' if not diff and len(ra) == len(rb) else 'DIFFERENT: %d, first %s' % (len(diff), diff[:5])) +
          ' (%d cases, %d without an error code)' % (len(ra), ran))
    sys.exit(0)
kw = tm.KW.replace('[8, 16, 32, 64, 128]', '[32, 64, 128, 256, 512]') if args.wide else tm.KW
env = {'HCU_TEST_BF16': '1' if args.bf16 else '0'}
ra = tm._run(tmp, 'a', dict(env, HCU_LIB_PATH=args.a, **_kv(args.env_a)), kw=kw)
rb = tm._run(tmp, 'b', dict(env, HCU_LIB_PATH=args.b, **_kv(args.env_b)), kw=kw)
diff = [(it, k, (x.double() - y.double()).abs().max().item())
        for it in range(3) for k, (x, y) in enumerate(zip(ra[it], rb[it])) if not torch.equal(x, y)]
print('bitwise equal' if not diff else 'DIFFERENT: %d tensors, first %s' % (len(diff), diff[:5]))
