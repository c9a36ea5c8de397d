"""The plans whose workspace sizes and slab arena tests/test_plan_sizes.py
checks (host only: planning needs no device).

Run as a module it plans every one of them and writes to stderr, around the
library's own HCU_PLAN_LOG lines,

    plan <name>
    sizes <saved_bytes> <scratch_bytes>

The planner's tiling choices (and with them the statistics rows and K-split
partials that size the scratch) depend on HCU_BCONV_TUNE, which the library
reads once per process: test_plan_sizes.py runs this module in a child process
with HCU_BCONV_TUNE=0 (the cost model's first choice: no table, no timing)."""
import ctypes
import sys

from hcunet_amd import _lib
from hcunet_amd.chain import CONV, CONVT, ChainSpec
from tests import bconv_tilings as bt

KW = dict(image_dimensions=3, in_channels=4, out_channels=1,
          kernel={'conv1': (3, 3, 2), 'conv2': (3, 3, 1)}, upsample_kernel=(2, 2, 2),
          max_pool_kernel=(2, 2, 1), upsample_stride=(2, 2, 1))
# the grouped (8, 8, 2)-upsample network and geometry of tests/test_gpu_modes.py
KW_GROUPS = dict(KW, feature_sizes=[16, 32, 64], upsample_kernel=(8, 8, 2), dilation=1, groups=2)
SHAPE_GROUPS = (1, 64, 60, 6)


def unet_sizes(kw, B, X, Y, Z, bf16=False, flags=0):
    from hcat.unet import Unet_Constructor
    from hcunet_amd.unet import _Plan, spec_struct
    spec = spec_struct(Unet_Constructor(**kw))
    spec.compute_dtype = _lib.HCU_BF16 if bf16 else _lib.HCU_F32
    p = _Plan(spec, B, X, Y, Z, flags)
    return p.saved_bytes, p.scratch_bytes


def chain_sizes(spec, B, X, Y, Z):
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.hcu_chain_plan_create(ctypes.addressof(spec), B, X, Y, Z, ctypes.byref(h)), 'chain')
    sv, sc = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.hcu_chain_plan_query(h, None, None, ctypes.byref(sv), ctypes.byref(sc)))
    L.hcu_unet_plan_destroy(h)
    return int(sv.value), int(sc.value)


def one_op_spec(kind, cin, cout, k, stride=(1, 1, 1), pad=(0, 0, 0), bf16=False, cl=False, in_part=0):
    """A chain of one Conv3d / ConvTranspose3d with bias, as hcunet_amd.chain.Chain.spec lays it out."""
    s = ChainSpec()
    s.n_ops = 1
    s.in_channels = cin
    o = s.ops[0]
    o.kind = kind
    o.out_channels = cout
    o.k = _lib.c_int3(*k)
    o.stride = _lib.c_int3(*stride)
    o.dil = _lib.c_int3(1, 1, 1)
    o.pad = _lib.c_int3(*pad)
    o.groups = 1
    o.w_off = 0
    o.b_off = cin * cout * k[0] * k[1] * k[2]
    o.gamma_off = o.beta_off = -1
    s.bn_eps = 1e-5
    s.bn_momentum = 0.1
    s.compute_dtype = _lib.HCU_BF16 if bf16 else _lib.HCU_F32
    s.in_cl = s.out_cl = int(cl)
    s.in_part_channels = in_part
    return s


def pointwise(cin, cout, dims, in_part=0):
    """A bf16 chain of one Conv3d(cin, cout, 1), the layer that takes pwconv.hip's
    kernels: NCXYZ boundaries, or (in_part) test_pointwise_conv_chain_bf16's
    channels-last cat of channel parts."""
    return lambda: chain_sizes(one_op_spec(CONV, cin, cout, (1, 1, 1), bf16=True, cl=in_part > 0,
                                           in_part=in_part), 1, *dims)


def convt_padded(bf16):
    """RDCNet.transposed_conv, test_convt_chain's first geometry: kernel 4, stride 2, padding 1."""
    return lambda: chain_sizes(one_op_spec(CONVT, 10, 5, (4, 4, 4), (2, 2, 2), (1, 1, 1), bf16=bf16), 1, 12, 12, 5)


PLANS = {
    'unet-2-4-f32': lambda: unet_sizes(dict(KW, feature_sizes=[2, 4]), 2, 18, 18, 3),
    'unet-8..128-f32': lambda: unet_sizes(dict(KW, feature_sizes=[8, 16, 32, 64, 128]), 2, 256, 256, 16),
    'unet-32..512-bf16': lambda: unet_sizes(dict(KW, feature_sizes=[32, 64, 128, 256, 512]), 4, 256, 256, 16,
                                            bf16=True),
    'unet-groups-up8-f32': lambda: unet_sizes(KW_GROUPS, *SHAPE_GROUPS),
    'unet-8..128-f32-forward-only': lambda: unet_sizes(dict(KW, feature_sizes=[8, 16, 32, 64, 128]), 2, 256, 256, 16,
                                                       flags=_lib.HCU_PLAN_FORWARD_ONLY),
    'chain-conv-bn-64-f32': lambda: chain_sizes(bt.chain_spec(64, False), 1, 12, 11, 4),
    'chain-conv-bn-64-bf16': lambda: chain_sizes(bt.chain_spec(64, True), 1, 12, 11, 4),
    'chain-convt-pad-f32': convt_padded(False),
    'chain-convt-pad-bf16': convt_padded(True),
    'chain-pw-50-10-part10-bf16': pointwise(50, 10, (24, 20, 6), in_part=10),
    'chain-pw-80-10-64x64x24-bf16': pointwise(80, 10, (64, 64, 24)),
    'chain-pw-96-32-32x32x8-bf16': pointwise(96, 32, (32, 32, 8)),
    'chain-pw-96-32-64x64x48-bf16': pointwise(96, 32, (64, 64, 48)),
}


def main():
    for name, plan in PLANS.items():
        sys.stderr.write('plan %s\n' % name)
        sys.stderr.flush()
        saved, scratch = plan()
        sys.stderr.write('sizes %d %d\n' % (saved, scratch))
        sys.stderr.flush()


if __name__ == '__main__':
    main()
