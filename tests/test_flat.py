"""The flat parameter / gradient store on host tensors (no device, no native
library): layout, what ready() detects, adoption of storage that is already
flat, the two grad_target rules and the one contiguity test.

These pin the behaviour the engine of Unet_Constructor and the layer chains'
store had as two implementations; only the adapter lines below differed when
the same tests ran against those."""
import pytest
import torch
import torch.nn as nn

from hcat.unet import Unet_Constructor
from hcunet_amd import dist as hdist
from hcunet_amd.flat import FlatParams, flat_run


def host_ready(store):
    return store.ready(require_gpu=False)


def chain_grad_target(store):
    return store.grad_target(overwrite=False)


# ---------------------------------------------------------------------------
KW = dict(image_dimensions=3, in_channels=4, out_channels=1, feature_sizes=[2, 4],
          kernel={'conv1': (3, 3, 2), 'conv2': (3, 3, 1)}, upsample_kernel=(2, 2, 2),
          max_pool_kernel=(2, 2, 1), upsample_stride=(2, 2, 1))
N_STATS = 2 * (2 + 2 + 4 + 4 + 2 + 2)   # running mean + var of the six BatchNorm3d


class _Holder(nn.Module):
    def __init__(self, *mods):
        super().__init__()
        self.m = nn.ModuleList(mods)


class _UnetCase:
    """Unet_Constructor through its engine."""

    def __init__(self):
        torch.manual_seed(0)
        self.root = Unet_Constructor(**KW)

    def ready(self):
        eng = self.root.engine()
        params = eng.params_ready(require_gpu=False)
        return eng.flat, params


class _HolderCase:
    """Three modules in a holder through the chains' store."""

    def __init__(self):
        torch.manual_seed(1)
        self.root = _Holder(nn.Conv3d(3, 4, 3), nn.BatchNorm3d(4), nn.ConvTranspose3d(4, 2, 2, stride=2))
        self.store = FlatParams(self.root)

    def ready(self):
        host_ready(self.store)
        params = self.store.params
        assert [self.store.offset(p) for p in params] == _cumulative(params)
        return self.store.flat, params


CASES = {'unet': _UnetCase, 'holder': _HolderCase}


def _cumulative(params):
    out, off = [], 0
    for p in params:
        out.append(off)
        off += p.numel()
    return out


def _assert_layout(root, flat, params):
    """Every parameter of root is the view at base + 4 * offset, in parameters() order."""
    live = list(root.parameters())
    assert len(live) == len(params) and all(p is q for p, q in zip(live, params))
    assert flat.dtype == torch.float32 and flat.numel() == sum(p.numel() for p in live)
    for p, off in zip(live, _cumulative(live)):
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        assert p.is_contiguous()


def _state(root):
    return {k: v.detach().clone() for k, v in root.state_dict().items()}


def _assert_state(root, want):
    got = root.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


# -- layout -------------------------------------------------------------------
@pytest.mark.parametrize('case', list(CASES))
def test_layout_and_second_ready_is_a_noop(case):
    c = CASES[case]()
    want = _state(c.root)
    flat, params = c.ready()
    _assert_layout(c.root, flat, params)
    _assert_state(c.root, want)
    flat2, params2 = c.ready()
    assert flat2 is flat and params2 is params
    _assert_state(c.root, want)


# -- detection ----------------------------------------------------------------
def _replace_parameter(root):
    mod = [m for m in root.modules() if isinstance(m, nn.BatchNorm3d)][0]
    mod.weight = nn.Parameter(mod.weight.detach().clone() * 2)


def _clone_data(root):
    p = list(root.parameters())[2]
    p.data = p.data.clone()


def _double_float(root):
    root.double().float()


@pytest.mark.parametrize('change', [_replace_parameter, _clone_data, _double_float])
@pytest.mark.parametrize('case', list(CASES))
def test_ready_detects_and_relays(case, change):
    c = CASES[case]()
    flat, params = c.ready()
    change(c.root)
    want = _state(c.root)
    flat2, params2 = c.ready()
    # `flat` is still alive here, so the new buffer cannot reuse its address
    assert flat2 is not flat and flat2.data_ptr() != flat.data_ptr()
    _assert_layout(c.root, flat2, params2)
    _assert_state(c.root, want)
    flat3, params3 = c.ready()
    assert flat3 is flat2 and params3 is params2


# -- adoption -----------------------------------------------------------------
def test_block_store_adopts_the_flattened_networks_storage():
    c = _UnetCase()
    flat, params = c.ready()
    want = _state(c.root)
    block = c.root.down_steps[0]
    store = FlatParams(block)
    host_ready(store)
    assert store.flat.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    assert store.flat.data_ptr() == flat.data_ptr()
    assert store.params is not params and all(p is q for p, q in zip(store.params, block.parameters()))
    for p in block.parameters():
        assert store.offset(p) == p.storage_offset()
        assert p.data_ptr() == store.flat.data_ptr() + 4 * store.offset(p)
    assert store.offset(None) == -1
    _assert_state(c.root, want)
    # no copy was made: a write through the network's buffer shows in the block
    off = store.offset(block.conv2.bias)
    with torch.no_grad():
        flat[off] = 123.5
    assert block.conv2.bias.detach().reshape(-1)[0].item() == 123.5
    # ... and the network's own store is undisturbed
    flat2, params2 = c.ready()
    assert flat2 is flat and params2 is params
    _assert_layout(c.root, flat, params)


def test_new_engine_adopts_a_storage_that_is_already_the_packed_layout():
    """Not inherited from the two earlier stores: Unet_Constructor._apply drops
    the engine even when it moved nothing (.float() on an fp32 network); the next
    engine finds the exact packed layout and keeps it instead of copying it."""
    c = _UnetCase()
    flat, params = c.ready()
    want = _state(c.root)
    c.root.float()
    assert c.root._engine is None
    flat2, params2 = c.ready()
    assert flat2 is not flat and flat2.data_ptr() == flat.data_ptr() and flat2.numel() == flat.numel()
    _assert_layout(c.root, flat2, params2)
    _assert_state(c.root, want)


# -- grad_target, the U-Net's rule (one backward per step: overwrite) -----------
def _fill(G):
    with torch.no_grad():
        G.copy_(torch.arange(1, G.numel() + 1, dtype=torch.float32) / 8)
    return G.clone()


def test_overwrite_fresh_then_attached():
    c = _UnetCase()
    flat, params = c.ready()
    eng = c.root.engine()
    n = flat.numel()
    G, accumulate, finish = eng.grad_target()
    assert accumulate == 0 and G is eng.grad_flat and G.numel() == n
    assert eng.comm_flat.numel() == n + N_STATS and eng.comm_flat.data_ptr() == G.data_ptr()
    assert all(p.grad is None for p in params)
    g = _fill(G)
    finish()
    for p, off in zip(params, _cumulative(params)):
        assert p.grad.data_ptr() == eng.comm_flat.data_ptr() + 4 * off and p.grad.shape == p.shape
        assert torch.equal(p.grad.reshape(-1), g[off:off + p.numel()])
    G2, accumulate2, finish2 = eng.grad_target()
    assert G2 is G and accumulate2 == 1
    finish2()
    assert torch.equal(G, g)   # nothing zeroed, nothing added by the host
    # gradients cleared: fresh again, the same buffer, still no zero fill
    for p in params:
        p.grad = None
    G3, accumulate3, _ = eng.grad_target()
    assert G3 is G and accumulate3 == 0 and torch.equal(G, g)


def test_overwrite_foreign_grad_takes_a_temporary():
    c = _UnetCase()
    flat, params = c.ready()
    eng = c.root.engine()
    odd = params[3]
    odd.grad = torch.ones_like(odd)
    G, accumulate, finish = eng.grad_target()
    assert accumulate == 0 and G.numel() == flat.numel()
    assert G is not eng.grad_flat and G.data_ptr() != eng.grad_flat.data_ptr()
    g = _fill(G)
    finish()
    for p, off in zip(params, _cumulative(params)):
        want = g[off:off + p.numel()].view_as(p)
        assert torch.equal(p.grad, want + 1 if p is odd else want)
        # a clone, not a view of the temporary or of the engine's buffer
        assert not (G.data_ptr() <= p.grad.data_ptr() < G.data_ptr() + 4 * G.numel())
        gf = eng.grad_flat
        assert not (gf.data_ptr() <= p.grad.data_ptr() < gf.data_ptr() + 4 * gf.numel())


def test_overwrite_frozen_parameter_stays_on_the_temporary_path():
    c = _UnetCase()
    flat, params = c.ready()
    eng = c.root.engine()
    frozen = c.root.out_conv.weight
    frozen.requires_grad_(False)
    G, accumulate, finish = eng.grad_target()
    assert accumulate == 0 and G is eng.grad_flat
    g = _fill(G)
    finish()
    assert frozen.grad is None
    assert all(p.grad is not None for p in params if p is not frozen)
    # the frozen parameter's missing .grad is examined too: not "all attached"
    G2, accumulate2, finish2 = eng.grad_target()
    assert accumulate2 == 0 and G2.data_ptr() != eng.grad_flat.data_ptr()
    with torch.no_grad():
        G2.fill_(1.0)
    finish2()
    assert frozen.grad is None
    for p, off in zip(params, _cumulative(params)):
        if p is not frozen:
            assert torch.equal(p.grad.reshape(-1), g[off:off + p.numel()] + 1)


# -- grad_target, the chains' rule (many backwards per step: zero once, add) ----
def test_accumulate_fresh_attached_foreign():
    c = _HolderCase()
    flat, params = c.ready()
    store = c.store
    G, accumulate, finish = chain_grad_target(store)
    assert accumulate == 1 and G.numel() == flat.numel() and G.data_ptr() == store.grad.data_ptr()
    with torch.no_grad():
        G.fill_(5.0)     # dirtied without attaching anything
    G2, accumulate2, finish2 = chain_grad_target(store)
    assert G2.data_ptr() == G.data_ptr() and accumulate2 == 1
    assert torch.count_nonzero(G2) == 0
    finish2()
    for p, off in zip(params, _cumulative(params)):
        assert p.grad.data_ptr() == G.data_ptr() + 4 * off and p.grad.shape == p.shape
    with torch.no_grad():
        G.fill_(3.0)
    G3, accumulate3, finish3 = chain_grad_target(store)
    assert G3.data_ptr() == G.data_ptr() and accumulate3 == 1
    finish3()
    assert bool((G == 3.0).all())          # attached: accumulate in place, not re-zeroed
    odd = params[1]
    odd.grad = torch.ones_like(odd)
    G4, accumulate4, finish4 = chain_grad_target(store)
    assert G4.data_ptr() != G.data_ptr() and accumulate4 == 1 and G4.numel() == flat.numel()
    assert torch.count_nonzero(G4) == 0
    with torch.no_grad():
        G4.fill_(2.0)
    finish4()
    for p, off in zip(params, _cumulative(params)):
        if p is odd:
            assert bool((p.grad == 3.0).all())
        else:   # still the view of the store's buffer, added to in place
            assert p.grad.data_ptr() == G.data_ptr() + 4 * off and bool((p.grad == 5.0).all())


def test_accumulate_skips_frozen_parameters():
    c = _HolderCase()
    flat, params = c.ready()
    store = c.store
    frozen = params[0]
    frozen.requires_grad_(False)
    G, accumulate, finish = chain_grad_target(store)
    assert accumulate == 1 and G.data_ptr() == store.grad.data_ptr()
    finish()
    assert frozen.grad is None
    assert all(p.grad is not None for p in params[1:])
    with torch.no_grad():
        G.fill_(4.0)
    G2, accumulate2, finish2 = chain_grad_target(store)
    assert G2.data_ptr() == G.data_ptr() and accumulate2 == 1   # not the temporary path
    finish2()
    assert frozen.grad is None and bool((G == 4.0).all())


# -- the contiguity test ----------------------------------------------------------
def _views(base):
    return [base[0:6].view(2, 3), base[6:10], base[10:24].view(2, 7)]


def _bad_runs():
    base = torch.arange(24, dtype=torch.float32)
    a, b, c = _views(base)
    gap = [a, c]
    order = [b, a, c]
    f64 = _views(torch.arange(24, dtype=torch.float64))
    strided = [torch.arange(6, dtype=torch.float32).view(3, 2).t()]
    return {'gap': gap, 'order': order, 'dtype': f64, 'noncontiguous': strided}


def test_flat_run_accepts_consecutive_views():
    base = torch.arange(30, dtype=torch.float32)[3:27]
    run = flat_run(_views(base))
    assert run is not None
    assert run[0].data_ptr() == base.data_ptr() and run[1] == 24


@pytest.mark.parametrize('kind', ['gap', 'order', 'dtype', 'noncontiguous'])
def test_flat_run_rejects(kind):
    assert flat_run(_bad_runs()[kind]) is None


def _with_grads(grads):
    params = [nn.Parameter(torch.zeros(g.shape, dtype=g.dtype)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g
    return params


def test_flat_grads_and_adam_fast_path_decision():
    base = torch.arange(30, dtype=torch.float32)[3:27]
    F = hdist._flat_grads(_with_grads(_views(base)))
    assert F.dim() == 1 and F.numel() == 24 and F.data_ptr() == base.data_ptr()
    assert torch.equal(F, base)
    for kind, grads in _bad_runs().items():
        assert hdist._flat_grads(_with_grads(grads)) is None, kind
    # optim.Adam updates a group in one launch when its parameters and their
    # gradients are both such runs: what a store leaves behind is
    c = _HolderCase()
    flat, params = c.ready()
    _, _, finish = chain_grad_target(c.store)
    finish()
    assert flat_run(params) is not None and flat_run([p.grad for p in params]) is not None
    params[1].grad = torch.ones_like(params[1])
    assert flat_run(params) is not None and flat_run([p.grad for p in params]) is None
