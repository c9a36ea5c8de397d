"""CPU: the planner's workspace sizes are pinned, and the weight-gradient slab
arena of every plan holds the largest slab a job will ask it for.

The plans (tests/plan_sizes.py) are built once, in a child process with
HCU_BCONV_TUNE=0 and HCU_PLAN_LOG=1; the library's `arena <floats> largest
slab <floats>` line of each plan is read back from its stderr."""
import os
import re
import subprocess
import sys

import pytest

from hcunet_amd import _lib
from tests import plan_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (saved_bytes, scratch_bytes) read from a build of commit 30fcce9, the parent
# of the change that made one job record size the arena and request the slab.
PINNED = {
    'unet-2-4-f32': (94208, 33879040),
    'unet-8..128-f32': (297802496, 1795676928),
    'unet-32..512-bf16': (1144267776, 7009038592),
    'unet-groups-up8-f32': (9167872, 63247872),
    'unet-8..128-f32-forward-only': (128905472, 26883840),
    'chain-conv-bn-64-f32': (877568, 9386240),
    'chain-conv-bn-64-bf16': (440320, 5534720),
    'chain-convt-pad-f32': (276224, 5691136),
    'chain-convt-pad-bf16': (147968, 5090304),
    'chain-pw-50-10-part10-bf16': (10240, 7921664),
    'chain-pw-80-10-64x64x24-bf16': (18887680, 98863104),
    'chain-pw-96-32-32x32x8-bf16': (2109440, 14035200),
}
# Conv3d(96, 32, 1) at 64 x 64 x 48: the pointwise weight gradient runs 768
# blocks of one 97 x 32 slab each.  At 30fcce9 the chain's arena was the 1 M
# float floor (scratch 232,545,280 bytes) and that slab ran past it; the arena
# is now the slab, and the scratch grew by exactly the arena's growth.
BIG = 'chain-pw-96-32-64x64x48-bf16'
BIG_SLAB = 768 * 97 * 32
BIG_SIZES = (50345984, 232545280 + 4 * (BIG_SLAB - (1 << 20)))


@pytest.fixture(scope='module')
def planned():
    """{plan name: dict(sizes=(saved, scratch), arena=floats, slab=floats)}"""
    env = dict(os.environ, HCU_BCONV_TUNE='0', HCU_PLAN_LOG='1')
    env.pop('HCU_CONV2_LOG', None)
    r = subprocess.run([sys.executable, '-m', 'tests.plan_sizes'], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r'plan (\S+)$', line)
        if m:
            cur = out.setdefault(m.group(1), {})
        m = re.match(r'arena (\d+) largest slab (\d+)$', line)
        if m:
            assert 'arena' not in cur, line   # one line per plan
            cur['arena'], cur['slab'] = int(m.group(1)), int(m.group(2))
        m = re.match(r'sizes (\d+) (\d+)$', line)
        if m:
            cur['sizes'] = (int(m.group(1)), int(m.group(2)))
    assert set(out) == set(plan_sizes.PLANS)
    return out


def test_workspace_sizes_are_pinned(planned):
    got = {k: v['sizes'] for k, v in planned.items()}
    print(got)
    assert got == dict(PINNED, **{BIG: BIG_SIZES})


def test_arena_holds_every_job(planned):
    print({k: (v['arena'], v['slab']) for k, v in planned.items()})
    for name, v in planned.items():
        assert v['arena'] >= v['slab'], (name, v)
        # a training plan runs weight gradients; a forward-only one has no arena
        assert (v['slab'] > 0) == ('forward-only' not in name), (name, v)
    assert BIG_SLAB == 2383872 == _lib.lib().hcu_pw_conv_work_floats(64 * 64 * 48, 1, 96, 32)
    assert planned[BIG]['slab'] == BIG_SLAB
