"""Shared by test_bconv_tilings.py (planner, CPU) and test_gpu_bconv_tilings.py
(numerical parity): the convolution cases, the HCU_BCONV_FORCE sweep and the
parser of the planner's HCU_CONV2_LOG lines.

An instance of bconv_kernel<E, CV, NSUB, MPW, NPF, MODE> is named here by
(CV, NSUB, MPW, NPF); a force string carries CK = CV * (4 fp32 | 8 bf16
channels per 16 bytes)."""
import ctypes
import itertools
import re

from hcunet_amd import _lib
from hcunet_amd.chain import CONV, ChainSpec

CVS = (1, 2, 4)
NSUBS = (1, 2, 4)
MPWS = (1, 2, 4)
NPFS = (0, 4, 8, 12)
ALL = frozenset(itertools.product(CVS, NSUBS, MPWS, NPFS))          # 108 instances
TAG = {False: 'f32', True: 'bf16'}


def vec(bf16):
    """Channels per 16-byte vector: CK = CV * vec."""
    return 8 if bf16 else 4


def forces(bf16, cvs=CVS, npfs=(None,) + NPFS):
    """Every (force string, (CV, NSUB, MPW, NPF or None)) of the sweep: the
    3-value form leaves the prefetch depth to the planner."""
    out = []
    for cv, ns, mp in itertools.product(cvs, NSUBS, MPWS):
        for pf in npfs:
            s = '%d,%d,%d' % (cv * vec(bf16), ns, mp)
            out.append((s if pf is None else '%s,%d' % (s, pf), (cv, ns, mp, pf)))
    return out


# Per-op cases (B, Cin, Cout, X, Y, Z, k, stride, transposed): ragged x / y
# tiles, two z tiles (Z = 20), 8 padded output columns (Cout 56 in a 64-wide
# block), four stride phases folded into N (the ConvTranspose3d), single- and
# multi-chunk K.
OP_CASES = {
    False: [
        (1, 16, 64, 13, 12, 9, (3, 3, 2), (1, 1, 1), 0),
        (2, 32, 56, 11, 10, 20, (3, 3, 1), (1, 1, 1), 0),
        (1, 64, 64, 12, 11, 4, (3, 3, 1), (1, 1, 1), 0),
        (1, 32, 16, 6, 5, 5, (2, 2, 2), (2, 2, 1), 1),
    ],
    True: [
        (1, 32, 64, 13, 12, 9, (3, 3, 2), (1, 1, 1), 0),
        (2, 64, 56, 11, 10, 20, (3, 3, 1), (1, 1, 1), 0),
        (1, 64, 64, 12, 11, 4, (3, 3, 1), (1, 1, 1), 0),
        (1, 64, 32, 6, 5, 5, (2, 2, 2), (2, 2, 1), 1),
    ],
}

# Chain cases: two Conv3d (C -> C, k (3, 3, 1), valid) + BatchNorm3d + ReLU on
# 1 x C x X x Y x Z.  C = 64 plans every role with a K split; C = 80 (fp32) /
# 96 (bf16) without one (256 % (OCs / VEC) != 0 disables it); the 8 x 8 x 2
# input is for the instances whose 12 x 11 x 4 halo needs more than 4 elements
# per thread.
CHAIN_K = (3, 3, 1)
CHAIN_CASES = {
    False: [(64, (12, 11, 4)), (80, (12, 11, 4)), (64, (8, 8, 2)), (80, (8, 8, 2))],
    True: [(64, (12, 11, 4)), (96, (12, 11, 4)), (64, (8, 8, 2)), (96, (8, 8, 2))],
}
CHAIN_ROLES = ('c0.fwd', 'c0.dgrad', 'c1.fwd', 'c1.dgrad')   # planning order
BNB_ROLE = 'c1.dgrad'   # the input gradient with the fused BatchNorm backward of c0's BatchNorm

# ---- the record (test_bconv_tilings.py asserts it against the planner, the GPU
# sweep against the kernels that launched) ------------------------------------
# Instances the planner refuses for every case of an (element type, mode) and
# that the sweeps therefore leave out: none.  (At most 3 per key, each named
# here and shown refused by test_bconv_tilings.py.)
EXCLUDED = {(bf16, mode): frozenset() for bf16 in (False, True) for mode in ('', ',bnb', ',ncx')}
# A 12 x 11 x 4 chain tile of MPW 4 with CV 4 stages more than 4 halo elements
# per thread: the planner keeps its own depth (8) there.  The 8 x 8 x 2 input
# reaches these three.
CHAIN_12x11x4_REFUSED = frozenset((4, ns, 4, 4) for ns in NSUBS)
# Honoured forced instances per per-op case, (forward, input gradient)
OP_REACHED = {
    False: [(89, 34), (99, 48), (105, 105), (108, 56)],
    True: [(89, 65), (99, 36), (105, 105), (108, 81)],
}


def chain_expected(dims):
    """Instances every role of a chain case reaches."""
    return ALL - CHAIN_12x11x4_REFUSED if tuple(dims) == (12, 11, 4) else ALL


def chain_ksplit(C):
    """Whether the chain's convolutions take a K split (see CHAIN_CASES)."""
    return C == 64


# ---- MODE 2 (',ncx'): the first layer reading the NCXYZ volume.  One channel
# group (CV 1) and a prefetched halo (NPF > 0) only; NSUB 4 needs 64 output
# columns, and feature sizes double per level.
NCX_KW = dict(image_dimensions=3, in_channels=4, out_channels=1, feature_sizes=[64, 128],
              kernel={'conv1': (3, 3, 2), 'conv2': (3, 3, 1)}, upsample_kernel=(2, 2, 2),
              max_pool_kernel=(2, 2, 1), upsample_stride=(2, 2, 1))
NCX_SHAPE = (1, 4, 28, 28, 4)
NCX_INSTANCES = frozenset(itertools.product((1,), NSUBS, MPWS, (4, 8, 12)))   # 27


def ncx_forces(bf16):
    return forces(bf16, cvs=(1,), npfs=(4, 8, 12))


def op_desc(case, bf16):
    B, Cin, Cout, X, Y, Z, k, s, tr = case
    d = _lib.ConvDesc()
    d.B, d.Cin, d.Cout, d.X, d.Y, d.Z = B, Cin, Cout, X, Y, Z
    d.k = _lib.c_int3(*k)
    d.stride = _lib.c_int3(*s)
    d.dil = _lib.c_int3(1, 1, 1)
    d.groups = 1
    d.transposed = tr
    d.dtype = _lib.HCU_BF16 if bf16 else _lib.HCU_F32
    return d


def chain_spec(C, bf16):
    """The ChainSpec hcunet_amd.chain.Chain builds for [Conv3d(C, C, CHAIN_K),
    BatchNorm3d, ReLU] x 2 with the parameters in module order (planning reads
    no parameter, so no device is needed)."""
    s = ChainSpec()
    s.n_ops = 2
    s.in_channels = C
    off = 0
    nw = C * C * CHAIN_K[0] * CHAIN_K[1] * CHAIN_K[2]
    for i in range(2):
        o = s.ops[i]
        o.kind = CONV
        o.out_channels = C
        o.k = _lib.c_int3(*CHAIN_K)
        o.stride = _lib.c_int3(1, 1, 1)
        o.dil = _lib.c_int3(1, 1, 1)
        o.pad = _lib.c_int3(0, 0, 0)
        o.groups = 1
        o.bn_relu = 1
        o.cat_fold = 0
        o.w_off, o.b_off, o.gamma_off, o.beta_off = off, off + nw, off + nw + C, off + nw + 2 * C
        off += nw + 3 * C
    s.bn_eps = 1e-5
    s.bn_momentum = 0.1
    s.compute_dtype = _lib.HCU_BF16 if bf16 else _lib.HCU_F32
    return s


def chain_plan_rc(C, dims, bf16):
    """hcu_chain_plan_create's return code for the chain case (the plan is
    destroyed again)."""
    L = _lib.lib()
    spec = chain_spec(C, bf16)
    h = ctypes.c_void_p()
    rc = L.hcu_chain_plan_create(ctypes.addressof(spec), 1, dims[0], dims[1], dims[2], ctypes.byref(h))
    if rc == 0 and h:
        L.hcu_unet_plan_destroy(h)
    return rc


PLAN_RE = re.compile(
    r'bconv plan \(es (\d+)\): B(\d+) I(\d+)x(\d+)x(\d+) ICs(\d+) O(\d+)x(\d+)x(\d+) S(\d+)x(\d+)x(\d+) '
    r'OCs(\d+) Cout(\d+) K(\d+)x(\d+)x(\d+) s(\d)(\d)(\d) nph(\d+) \| CK(\d+) NSUB(\d+) MPW(\d+) '
    r'T(\d+)x(\d+)x(\d+) ks(\d+) cps(\d+) NPF(\d+) gridx(\d+) lds(\d+) halo (\d+),(\d+),(\d+)/(\d+)')
_FIELDS = ('es B IX IY IZ ICs OX OY OZ SX SY SZ OCs Cout KX KY KZ sx sy sz nph CK NSUB MPW TX TY TZ ks cps NPF '
           'gridx lds hsx hsy hsz hvp').split()


def parse_plans(err):
    """The planner's log lines as dicts of ints, in planning order, each with
    'inst' = (CV, NSUB, MPW, NPF)."""
    out = []
    for m in PLAN_RE.finditer(err):
        p = dict(zip(_FIELDS, (int(v) for v in m.groups())))
        p['inst'] = (p['CK'] // (16 // p['es']), p['NSUB'], p['MPW'], p['NPF'])
        out.append(p)
    return out


def honoured(plan, want):
    """Whether a logged plan is the forced tiling (NPF None: any depth)."""
    got = plan['inst']
    return got[:3] == want[:3] and (want[3] is None or got[3] == want[3])


def op_role(plan, case):
    """'fwd' or 'dgrad' of a per-op plan line: a forward reads the op's input
    extent (a ConvTranspose3d forward folds its stride phases into N), an
    input gradient computes it."""
    X, Y, Z = case[3:6]
    if case[8]:
        return 'fwd' if plan['nph'] > 1 else 'dgrad'
    if (plan['IX'], plan['IY'], plan['IZ']) == (X, Y, Z):
        return 'fwd'
    assert (plan['OX'], plan['OY'], plan['OZ']) == (X, Y, Z), plan
    return 'dgrad'


def label(bf16, inst, mode=''):
    """The kernel's name in hcu_timing_report, mode '' / ',bnb' / ',ncx'."""
    return 'bconv_kernel<%s,%d,%d,%d,%d%s>' % ((TAG[bf16],) + tuple(inst) + (mode,))


def reduce_label(bf16):
    return 'bconv_reduce_kernel<%s>' % TAG[bf16]
