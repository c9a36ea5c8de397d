"""CPU: the kernel family the planning ladders (csrc/families.cpp) choose for
every convolution and weight gradient of three fp32 U-Net plans, by default
and with each family's off-switch set.

The plans are tests/plan_sizes.py's, built in one child process per switch
(the library reads the switches once) with HCU_BCONV_TUNE=0 and
HCU_PLAN_LOG=1; the `conv <layer> <role> <family> ...` and `wgrad <layer>
<family> ...` lines are read back from stderr.

The expected families were printed from the planner's flags by a build of
commit 309bb54, the parent of the change that gave every plan one family tag:
  * unet-2-4-f32 is the plan that runs conv2 by default (the 2-channel
    ConvTranspose3d forward with its four phases folded, the strided 4-channel
    input gradient) and the generic wgrad kernel (u0.up); without conv2 its
    ConvTranspose3d forward runs one gconv launch per phase;
  * unet-groups-up8-f32: the (8, 8, 2) ConvTranspose3d input gradients fall to
    gconv without the fp32 bconv."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# plan -> family -> 'layer/role ...' with no switch set
DEFAULT = {
    'unet-2-4-f32': {
        'conv8': 'd0.c1/fwd d0.c1/dgrad d1.c1/fwd d1.c1/dgrad d0.c2/fwd d0.c2/dgrad d1.c2/fwd d1.c2/dgrad '
                 'u0.c1/fwd u0.c1/dgrad u0.c2/fwd u0.c2/dgrad',
        'conv2': 'u0.up/up.fwd u0.up/up.dgrad',
        'wgrad8': 'd0.c1/wgrad d1.c1/wgrad d0.c2/wgrad u0.c1/wgrad u0.c2/wgrad',
        'wgrad2': 'd1.c2/wgrad',
        'wgrad': 'u0.up/wgrad',
    },
    'unet-8..128-f32': {
        'conv8': 'd0.c1/fwd d0.c1/dgrad d1.c1/dgrad d0.c2/fwd d0.c2/dgrad u3.c1/fwd u3.c1/dgrad u3.c2/fwd u3.c2/dgrad',
        'bconv-f32': 'd1.c1/fwd d2.c1/fwd d2.c1/dgrad d3.c1/fwd d3.c1/dgrad d4.c1/fwd d4.c1/dgrad '
                     'd1.c2/fwd d1.c2/dgrad d2.c2/fwd d2.c2/dgrad d3.c2/fwd d3.c2/dgrad d4.c2/fwd d4.c2/dgrad '
                     'u0.c1/fwd u0.c1/dgrad u1.c1/fwd u1.c1/dgrad u2.c1/fwd u2.c1/dgrad '
                     'u0.c2/fwd u0.c2/dgrad u1.c2/fwd u1.c2/dgrad u2.c2/fwd u2.c2/dgrad '
                     'u0.up/up.fwd u0.up/up.dgrad u1.up/up.fwd u1.up/up.dgrad '
                     'u2.up/up.fwd u2.up/up.dgrad u3.up/up.fwd u3.up/up.dgrad',
        'wgrad8': 'd0.c1/wgrad d0.c2/wgrad d1.c2/wgrad u3.c1/wgrad u2.c2/wgrad u3.c2/wgrad',
        'wgrad2': 'd1.c1/wgrad d2.c1/wgrad u2.c1/wgrad',
        'wgrad3': 'd3.c1/wgrad d4.c1/wgrad d2.c2/wgrad d3.c2/wgrad d4.c2/wgrad u0.c1/wgrad u1.c1/wgrad '
                  'u0.c2/wgrad u1.c2/wgrad u0.up/wgrad u1.up/wgrad u2.up/wgrad u3.up/wgrad',
    },
    'unet-groups-up8-f32': {
        'bconv-f32': 'd0.c1/fwd d1.c1/fwd d1.c1/dgrad d2.c1/fwd d2.c1/dgrad d0.c2/fwd d0.c2/dgrad '
                     'd1.c2/fwd d1.c2/dgrad d2.c2/fwd d2.c2/dgrad u0.c1/fwd u0.c1/dgrad u1.c1/fwd u1.c1/dgrad '
                     'u0.c2/fwd u0.c2/dgrad u1.c2/fwd u1.c2/dgrad '
                     'u0.up/up.fwd u0.up/up.dgrad u1.up/up.fwd u1.up/up.dgrad',
        'conv8': 'd0.c1/dgrad',
        'wgrad2': 'd0.c1/wgrad d1.c1/wgrad u1.c1/wgrad',
        'wgrad3': 'd2.c1/wgrad d1.c2/wgrad d2.c2/wgrad u0.c1/wgrad u0.c2/wgrad u0.up/wgrad u1.up/wgrad',
        'wgrad8': 'd0.c2/wgrad u1.c2/wgrad',
    },
}
# switch -> (the family it takes out, the family its GEMMs ran instead, the
# GEMMs that did otherwise: (plan, 'layer/role') -> family, None = not planned)
SWITCHES = {
    'HCU_NO_CONV8=1': ('conv8', 'conv2', {}),
    'HCU_NO_CONV2=1': ('conv2', 'gconv', {
        ('unet-2-4-f32', 'u0.up/up.fwd'): None, ('unet-2-4-f32', 'u0.up/ph0'): 'gconv',
        ('unet-2-4-f32', 'u0.up/ph1'): 'gconv', ('unet-2-4-f32', 'u0.up/ph2'): 'gconv',
        ('unet-2-4-f32', 'u0.up/ph3'): 'gconv'}),
    'HCU_NO_BCONV_F32=1': ('bconv-f32', 'conv2', {
        ('unet-groups-up8-f32', 'u0.up/up.dgrad'): 'gconv', ('unet-groups-up8-f32', 'u1.up/up.dgrad'): 'gconv'}),
    'HCU_NO_WGRAD8=1': ('wgrad8', 'wgrad2', {}),
    'HCU_NO_WGRAD2=1': ('wgrad2', 'wgrad', {}),
    # (the ConvTranspose3d phase form only runs on wgrad3: without it, the per-tap form on the generic kernel)
    'HCU_WGRAD3=0': ('wgrad3', 'wgrad2', {
        ('unet-8..128-f32', 'u0.up/wgrad'): 'wgrad', ('unet-8..128-f32', 'u1.up/wgrad'): 'wgrad',
        ('unet-8..128-f32', 'u2.up/wgrad'): 'wgrad', ('unet-8..128-f32', 'u3.up/wgrad'): 'wgrad',
        ('unet-groups-up8-f32', 'u0.up/wgrad'): 'wgrad', ('unet-groups-up8-f32', 'u1.up/wgrad'): 'wgrad'}),
}
CASES = [''] + list(SWITCHES)

CHILD = ('import sys\n'
         'from tests import plan_sizes\n'
         'for n in %r:\n'
         '    sys.stderr.write("plan %%s\\n" %% n)\n'
         '    sys.stderr.flush()\n'
         '    plan_sizes.PLANS[n]()\n' % (tuple(DEFAULT),))


def expected(case):
    """{(plan, 'layer/role'): family} under the switch `case` ('' = none)."""
    out = {(plan, gemm): fam for plan, fams in DEFAULT.items() for fam, gemms in fams.items()
           for gemm in gemms.split()}
    if case:
        off, instead, other = SWITCHES[case]
        out = {k: instead if fam == off else fam for k, fam in out.items()}
        out.update(other)
        out = {k: fam for k, fam in out.items() if fam is not None}
    return out


@pytest.fixture(scope='module')
def planned():
    """{case: {(plan, 'layer/role'): family}}, the children run side by side."""
    env = {k: v for k, v in os.environ.items() if k not in [c.split('=')[0] for c in SWITCHES]}
    env.update(HCU_BCONV_TUNE='0', HCU_PLAN_LOG='1')
    env.pop('HCU_CONV2_LOG', None)
    procs = {}
    for case in CASES:
        e = dict(env, **dict([case.split('=')] if case else []))
        procs[case] = subprocess.Popen([sys.executable, '-c', CHILD], cwd=ROOT, env=e, stdout=subprocess.DEVNULL,
                                       stderr=subprocess.PIPE, text=True)
    out = {}
    for case, p in procs.items():
        err = p.communicate(timeout=600)[1]
        assert p.returncode == 0, (case, err[-3000:])
        got, plan = {}, None
        for line in err.splitlines():
            m = re.match(r'plan (\S+)$', line)
            if m:
                plan = m.group(1)
            m = re.match(r'conv (\S+) +(\S+) +(\S+) +grid \d+ x \d+ x \d+ lds \d+ rows \d+ partial \d+ wimage \d+$', line)
            if m:
                assert (plan, m.group(1) + '/' + m.group(2)) not in got, line
                got[plan, m.group(1) + '/' + m.group(2)] = m.group(3)
            m = re.match(r'wgrad (\S+) +(\S+) +KB ', line)
            if m:
                assert (plan, m.group(1) + '/wgrad') not in got, line
                got[plan, m.group(1) + '/wgrad'] = m.group(2)
        out[case] = got
    return out


@pytest.mark.parametrize('case', CASES)
def test_family_of_every_gemm(planned, case):
    got, want = planned[case], expected(case)
    print({k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
    assert got == want


def test_every_family_is_covered():
    """The table itself: each of the eight fp32 families is the expectation of some GEMM."""
    seen = {fam for case in CASES for fam in expected(case).values()}
    assert seen == {'gconv', 'conv2', 'conv8', 'bconv-f32', 'wgrad', 'wgrad2', 'wgrad8', 'wgrad3'}
