"""Results must not depend on unwritten bytes.

The executor never clears its device memory (saved, scratch, outputs, dx, the
chains' weight images, the r_unet helper buffers, the loss scalars are all
uninitialised), so a step is correct only when every kernel writes each word
a later kernel reads: channel padding slots, halo and phase columns,
statistic and split-K partial rows, weight-gradient slabs.  In a fresh
process such memory reads 0 (or finite leftovers of the same shapes), so no
parity test sees a violation.

Here every buffer handed out by hcunet_amd._lib.empty (and the gradient
buffer where the backward overwrites it) is filled with a byte first
(_lib.POISON), and each case runs three times from the same seed and inputs:
0x00 (what a fresh process sees), 0xFF (NaN in fp32, bf16 and fp16) and 0x3F
(about 0.75 in fp32 and bf16: ReLU-on-load, max, pooling and x > 0 ? a : b
selections swallow a NaN, a finite value shows).  Every returned tensor must
be finite and bitwise equal across the three runs -- no tolerance; the
tilings are deterministic in test processes (conftest.py) and the unpoisoned
step is bitwise repeatable (test_gpu_unet.test_deterministic_bitwise), so a
difference is a read of memory the step did not write.  No CPU oracle runs
here."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import hcat.dataloader as hdl
import hcat.loss as hl
import hcat.transforms as ht
from hcat.r_unet import RDCNet, RecursiveUnet
from hcat.unet import Unet_Constructor
from hcunet_amd import _lib
from hcunet_amd import segment as seg
from hcunet_amd.chain import Chain, FlatParams, cl_channels
from hcunet_amd.optim import Adam
from oracle import inputs
from tests import test_gpu_chain as tch
from tests import test_gpu_input_path as tip
from tests import test_gpu_loss_methods as tlm
from tests import test_gpu_modes as tmodes
from tests import test_gpu_runet as tru
from tests.helpers import REF_KW
from tests.test_gpu_unet import CONFIGS, _mask_pwl, _weighted_backward
from tests.test_loss_oracle import CASE_FN, CASES, case_inputs
from tests.test_segment_oracle import SEG_KW, gold, golden_state, golden_volume

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0x3F)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """t on the host through an integer view: equality on bits (NaN == NaN, -0 != 0)."""
    t = t.detach().cpu().contiguous()
    return t if not t.is_floating_point() else t.view(_INT[t.element_size()])


def same_bits(a, b):
    """[(name, differing words, of)] of two {name: tensor} results."""
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        x, y = bits(a[k]), bits(b[k])
        if x.shape != y.shape or not torch.equal(x, y):
            bad.append((k, int((x != y).sum()) if x.shape == y.shape else -1, x.numel()))
    return bad


def not_finite(res):
    return [k for k, v in res.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]


def poisoned(monkeypatch, fn):
    """fn() -> {name: tensor}, run once per fill in a fresh state (fn builds its
    model from the same seed and the same inputs each time): every tensor
    finite, and bitwise equal whatever the uninitialised buffers held."""
    runs = []
    for b in FILLS:
        monkeypatch.setattr(_lib, 'POISON', b)
        res = fn()
        torch.cuda.synchronize()
        runs.append({k: v.detach().cpu() for k, v in res.items()})
    monkeypatch.setattr(_lib, 'POISON', None)
    assert not not_finite(runs[0]), ('fill 0x00 not finite', not_finite(runs[0])[:8])
    for b, r in zip(FILLS[1:], runs[1:]):
        bad = same_bits(runs[0], r)
        assert not bad, ('fill 0x%02X differs from 0x00 in (name, words, of)' % b, bad[:8])
    return runs[0]


@functools.lru_cache(maxsize=None)
def _x(shape):
    return torch.from_numpy(inputs.make_x(shape))


@functools.lru_cache(maxsize=None)
def _targets(out_shape):
    mask, pwl = _mask_pwl(out_shape)
    return torch.from_numpy(mask), torch.from_numpy(pwl)


def _state(m, res, tag):
    for k, p in m.named_parameters():
        res[tag + k] = p.detach().clone()
    for k, b in m.named_buffers():
        res[tag + k] = b.detach().clone()


# ---------------------------------------------------------------------------
# U-Net
def _unet_steps(kw, shape, bf16=False, x_dtype=torch.float32):
    """Two full training steps on one model (train forward, pixel loss,
    backward with the input gradient, Adam.step: the second step reuses the
    plan, the graph and the gradient buffer), then an eval forward."""
    torch.manual_seed(0)
    m = Unet_Constructor(**kw).cuda().train()
    opt = Adam(m.parameters(), lr=1e-3)
    x0 = _x(shape).cuda().to(x_dtype)
    res = {}
    for step in range(2):
        opt.zero_grad()
        x = x0.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
            out = m(x)
        mask, pwl = _targets(tuple(out.shape))
        loss = hl.cross_entropy(out, mask.cuda(), pwl.cuda(), method='pixel')
        loss.backward()
        res['out%d' % step], res['loss%d' % step], res['dx%d' % step] = out, loss, x.grad
        for k, p in m.named_parameters():
            res['grad%d.%s' % (step, k)] = p.grad.detach().clone()
        opt.step()
    _state(m, res, 'after.')
    m.eval()
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
        res['eval'] = m(x0)
    return res


# smallest first; `odd` (3, 6, 12 and 2 channels) has padding slots in every
# layer, g2_up8 the groups and the 8x8x2 upsample phases
@pytest.mark.parametrize('name', ['odd', 'l3', 'g2_up8', 'dil', 'l4', 'l5_min'])
def test_unet_fp32(monkeypatch, name):
    kw, shape = CONFIGS[name]
    poisoned(monkeypatch, lambda: _unet_steps(kw, shape))


BF16_CASES = {
    'f16-32-64_x32': (dict(REF_KW, feature_sizes=[16, 32, 64]), (2, 4, 44, 44, 5), torch.float32),
    'f16-32-64_x16': (dict(REF_KW, feature_sizes=[16, 32, 64]), (2, 4, 44, 44, 5), torch.float16),
    'f16-32-64_xbf16': (dict(REF_KW, feature_sizes=[16, 32, 64]), (2, 4, 44, 44, 5), torch.bfloat16),
    'f4-8-16': (dict(REF_KW, feature_sizes=[4, 8, 16]), (2, 4, 44, 44, 5), torch.float32),   # 4 channels in 8 slots
    'odd': CONFIGS['odd'] + (torch.float32,),
    # config 3's widths: the deep layers have split-K partial rows and bwgrad slabs
    'config3_widths': (dict(REF_KW, feature_sizes=[32, 64, 128, 256, 512]), (1, 4, 188, 188, 6), torch.float32),
}


@pytest.mark.parametrize('name', list(BF16_CASES))
def test_unet_bf16(monkeypatch, name):
    kw, shape, x_dtype = BF16_CASES[name]
    poisoned(monkeypatch, lambda: _unet_steps(kw, shape, bf16=True, x_dtype=x_dtype))


def _seg_net(g, train):
    torch.manual_seed(0)
    m = Unet_Constructor(**SEG_KW)
    m.load_state_dict(golden_state(g))
    m = m.cuda()
    return m.train() if train else m.eval()


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
def test_forward_only_plan(monkeypatch, train):
    """The no-grad plan (HCU_PLAN_FORWARD_ONLY: activations in two ping-pong
    buffers), as tests/test_gpu_segment.py reaches it."""
    g = gold()
    x = torch.from_numpy(np.nan_to_num(golden_volume(g).numpy()[:, :, :96, :96, :],
                                       nan=0.0, posinf=1.0, neginf=1.0)).cuda()

    def fn():
        m = _seg_net(g, train)
        with torch.no_grad():
            res = {'out': m(x)}
        _state(m, res, 'after.')
        return res
    poisoned(monkeypatch, fn)


def test_gradient_accumulation(monkeypatch):
    """Two backwards without zero_grad: the second adds in place."""
    kw, shape = CONFIGS['l2']

    def fn():
        torch.manual_seed(0)
        m = Unet_Constructor(**kw).cuda().train()
        x = _x(shape).cuda().requires_grad_(True)
        res = {}
        for step in range(2):
            out = m(x)
            _weighted_backward(out, 11)
            res['out%d' % step] = out
            res['dx%d' % step] = x.grad.detach().clone()
            for k, p in m.named_parameters():
                res['grad%d.%s' % (step, k)] = p.grad.detach().clone()
        return res
    poisoned(monkeypatch, fn)


def test_partially_frozen_network(monkeypatch):
    """out_conv frozen (test_gpu_unet.test_partially_frozen_network): the
    second backward goes through a temporary buffer.  Only what the API
    exposes is compared: the frozen slots of the buffers belong to nobody."""
    kw, shape = CONFIGS['l2']

    def fn():
        torch.manual_seed(0)
        m = Unet_Constructor(**kw).cuda().train()
        for p in m.out_conv.parameters():
            p.requires_grad_(False)
        x = _x(shape).cuda()
        res = {}
        for step in range(2):
            out = m(x)
            _weighted_backward(out, 11)
            res['out%d' % step] = out
            for k, p in m.named_parameters():
                assert (p.grad is None) == k.startswith('out_conv.')
                if p.grad is not None:
                    res['grad%d.%s' % (step, k)] = p.grad.detach().clone()
        return res
    poisoned(monkeypatch, fn)


def test_unet_blocks_on_their_own(monkeypatch):
    """A Down and an Up block called alone (the chains behind them), shapes of
    test_gpu_runet.test_unet_blocks_callable_on_their_own."""
    g = np.load(os.path.join(tru.GOLD, 'unet_blocks.npz'))
    kw = dict(REF_KW, feature_sizes=[4, 8, 16])
    xd0, xu0 = _x(tuple(int(v) for v in g['xd_shape'])), _x(tuple(int(v) for v in g['xu_shape']))
    skip = tuple(int(v) for v in g['skip'])

    def fn():
        torch.manual_seed(5)
        net = Unet_Constructor(**kw).cuda().train()
        d, u = net.down_steps[0], net.up_steps[0]
        res = {}
        xd = xd0.cuda().requires_grad_(True)
        od = d(xd)
        (od * _x(tuple(od.shape)).cuda()).sum().backward()
        xu = xu0.cuda().requires_grad_(True)
        ou = u(xu, torch.zeros(skip, device='cuda'))
        (ou * _x(tuple(ou.shape)).cuda()).sum().backward()
        res.update(down=od, down_dx=xd.grad, up=ou, up_dx=xu.grad)
        for tag, blk in (('down.', d), ('up.', u)):
            for k, p in blk.named_parameters():
                res[tag + 'grad.' + k] = p.grad.detach().clone()
            for k, b in blk.named_buffers():
                res[tag + k] = b.detach().clone()
        return res
    poisoned(monkeypatch, fn)


# ---------------------------------------------------------------------------
# Execution modes: 3 steps in a child process (tests/test_gpu_modes._run), with
# HCU_POISON set for the child and without
_KW_BF16 = tmodes.KW.replace('[8, 16, 32, 64, 128]', '[16, 32, 64, 128]')
_plain = {}


def _child(tmp_path, tag, env, bf16, poison):
    env = dict(env, HCU_TEST_BF16=bf16, HCU_POISON=poison)
    return tmodes._run(tmp_path, tag, env, kw=tmodes.KW if bf16 == '0' else _KW_BF16)


def _same_dump(a, b):
    assert len(a) == len(b) == 3
    bad = []
    for it in range(3):
        assert len(a[it]) == len(b[it])
        for k, (x, y) in enumerate(zip(a[it], b[it])):
            if not torch.isfinite(x).all() or not torch.equal(bits(x), bits(y)):
                bad.append((it, k))
    assert not bad, bad[:8]


def _ids(sw):
    return ','.join('%s=%s' % kv for kv in sw.items()) or 'default'


@pytest.mark.parametrize('bf16,sw', [('0', s) for s in (
    {}, {'HCU_SIDE': '0'}, {'HCU_GRAPHS': '1'}, {'HCU_NO_BNFUSE': '1'}, {'HCU_WGF_DEFER': '0'},
    {'HCU_WGRAD3': '0'})] + [('1', s) for s in ({}, {'HCU_BW_CUS': '128'})],
    ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_execution_modes(tmp_path, bf16, sw):
    plain = _child(tmp_path, 'plain', sw, bf16, '')
    if not sw:
        _plain[bf16] = plain
    _same_dump(plain, _child(tmp_path, 'ff', sw, bf16, 'ff'))


def test_execution_default_finite_fill(tmp_path):
    plain = _plain.get('0') or _child(tmp_path, 'plain', {}, '0', '')
    _same_dump(plain, _child(tmp_path, '3f', {}, '0', '3f'))


# ---------------------------------------------------------------------------
# Chains, RDCNet, RecursiveUnet
def _rows(test):
    return [m for m in test.pytestmark if m.name == 'parametrize'][0].args[1]


def _chain_steps(make_mods, spec_of, x, bf16, need_dx=True):
    """A chain over fresh modules: an eval forward (the plan's weight-image
    buffer, new and poisoned, gets the forward images: image_level 1), a train
    step (the input-gradient images: level 2), a parameter edit and a second
    train step on the same plan (everything re-laid from level 0)."""
    torch.manual_seed(0)
    holder = tch._Holder(*make_mods()).cuda()
    flat = FlatParams(holder)
    ch = Chain(flat, x.shape[1], spec_of(holder.m))
    res = {}
    with torch.no_grad():
        res['eval'] = ch(x.cuda(), False, bf16)
    for step in range(2):
        holder.zero_grad(set_to_none=True)
        xg = x.cuda().requires_grad_(need_dx)
        out = ch(xg, True, bf16)
        (out * _x(tuple(out.shape)).cuda()).sum().backward()
        res['out%d' % step] = out
        if need_dx:
            res['dx%d' % step] = xg.grad
        for k, p in holder.named_parameters():
            res['grad%d.%s' % (step, k)] = p.grad.detach().clone()
        with torch.no_grad():
            for p in holder.parameters():
                p.mul_(0.75)
    assert len(ch.plans) == 1
    for k, b in holder.named_buffers():
        res['buf.' + k] = b.detach().clone()
    return res


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('k,s,p,d,cin,cout,shape', _rows(tch.test_conv_chain))
def test_conv_chain(monkeypatch, k, s, p, d, cin, cout, shape, bf16):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    poisoned(monkeypatch, lambda: _chain_steps(
        lambda: [nn.Conv3d(cin, cout, k, stride=s, padding=p, dilation=d)],
        lambda m: [('conv', m[0], None, False)], x, bf16, need_dx=(s == 1)))


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('k,s,p,cin,cout,shape', _rows(tch.test_convt_chain))
def test_convt_chain(monkeypatch, k, s, p, cin, cout, shape, bf16):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(2))
    poisoned(monkeypatch, lambda: _chain_steps(
        lambda: [nn.ConvTranspose3d(cin, cout, k, stride=s, padding=p)],
        lambda m: [('convt', m[0])], x, bf16))


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_down_pool_chain(monkeypatch, bf16):
    """test_gpu_chain.test_down_pool_chain's module list."""
    x = torch.randn((1, 9, 16, 16, 4), generator=torch.Generator().manual_seed(4))
    poisoned(monkeypatch, lambda: _chain_steps(
        lambda: [nn.Conv3d(9, 16, 3, padding=1), nn.BatchNorm3d(16), nn.Conv3d(16, 16, 3, padding=1),
                 nn.BatchNorm3d(16)],
        lambda m: [('conv', m[0], m[1], False), ('conv', m[2], m[3], False), ('pool', (2, 2, 1))], x, bf16))


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
def test_channels_last_boundaries_and_parts(monkeypatch, bf16):
    """in_cl / out_cl / in_part, 10 channels in 12 (fp32) or 16 (bf16) slots
    (test_gpu_chain.test_channels_last_boundaries_and_parts): the output and
    the gradients of both inputs are compared with their padding slots."""
    C = 10
    shape = (1, C, 40, 36, 12)
    gen = torch.Generator().manual_seed(3)
    a, b, g = (torch.randn(shape, generator=gen) for _ in range(3))
    dt = torch.bfloat16 if bf16 else torch.float32
    cs = cl_channels(C, bf16)

    def fn():
        torch.manual_seed(3)
        holder = tch._Holder(nn.Conv3d(2 * C, C, 1), nn.Conv3d(C, C, 5, dilation=4, padding=8)).cuda()
        flat = FlatParams(holder)
        m1, m2 = holder.m
        k1 = Chain(flat, 2 * C, [('conv', m1, None, False)], in_cl=True, out_cl=True, in_part=C)
        k2 = Chain(flat, C, [('conv', m2, None, False)], in_cl=True, out_cl=True)
        xa = tch._to_cl(a.cuda(), cs, dt).requires_grad_(True)
        xb = tch._to_cl(b.cuda(), cs, dt).requires_grad_(True)
        y = k2(k1(torch.cat((xa, xb), -1), True, bf16), True, bf16)
        (y.float() * tch._to_cl(g.cuda(), cs, torch.float32)).sum().backward()
        res = dict(y=y, da=xa.grad, db=xb.grad)
        for k, p in holder.named_parameters():
            res['grad.' + k] = p.grad.detach().clone()
        return res
    r = poisoned(monkeypatch, fn)
    for k in ('y', 'da', 'db'):
        assert r[k].shape[-1] == cs and not r[k][..., C:].any(), k


def _net_results(net, out, loss):
    res = {'out': out, 'loss': torch.as_tensor(loss)}
    for k, p in net.named_parameters():
        res['grad.' + k] = p.grad.detach().clone()
    for k, b in net.named_buffers():
        res['buf.' + k] = b.detach().clone()
    return res


def test_rdcnet_train_step(monkeypatch):
    g = np.load(os.path.join(tru.GOLD, 'runet_rdc.npz'))
    x = inputs.make_x(tuple(g['x_shape']))

    def fn():
        torch.manual_seed(int(g['seed']))
        net = RDCNet(4, 5).cuda().train()
        return _net_results(net, *tru._train_step(net, g, x))
    poisoned(monkeypatch, fn)


def test_recursive_unet_train_step(monkeypatch):
    g = np.load(os.path.join(tru.GOLD, 'runet_rec.npz'))
    x = inputs.make_x(tuple(g['x_shape']))

    def fn():
        torch.manual_seed(int(g['seed']))
        net = RecursiveUnet(image_dimensions=3).cuda().train()
        return _net_results(net, *tru._train_step(net, g, x))
    poisoned(monkeypatch, fn)


def test_rdcnet_bf16_autocast(monkeypatch):
    """The bf16 recurrence: cat-free 1x1x1 convolutions, the residual add, the
    gradient sums, the padded ConvTranspose3d phase columns."""
    shape = (1, 4, 64, 64, 24)
    mshape = (1, 1) + shape[2:]
    x = _x(shape).cuda()
    mask = torch.from_numpy(inputs.make_mask(mshape)).cuda()
    pwl = torch.from_numpy(inputs.make_pwl(mshape)).cuda()
    vec = (_x((1, 3) + shape[2:]) * 0.5).cuda()

    def fn():
        torch.manual_seed(0)
        net = RDCNet(4, 5).cuda().train()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = net(x)
            loss = hl.cross_entropy(out[:, 0:1], mask, pwl, method='pixel') + hl.MSELoss(out[:, 2:], vec)
        loss.backward()
        return _net_results(net, out, loss.detach())
    poisoned(monkeypatch, fn)


# ---------------------------------------------------------------------------
# Loss, segment, ingest
@pytest.mark.parametrize('name', [n for n in CASES if CASE_FN[n][1] != 'random'])
def test_loss(monkeypatch, name):
    pred, mask, pwl = case_inputs(name)

    def fn():
        pd = pred.cuda().requires_grad_(True)
        v = tlm.run(hl, name, pd, mask.cuda(), None if pwl is None else pwl.cuda(), gscale=2.5)
        return {'loss': v, 'grad': pd.grad}
    poisoned(monkeypatch, fn)


def test_tiled_probability_map(monkeypatch):
    """The tiled driver on test_gpu_segment's whole 160x160x16 volume (12 tiles
    of 383x383x25, one NaN and two Inf voxels cleaned by the gather): the
    driver, like the reference, refuses a volume narrower than its 128-voxel
    evaluation window, so there is no smaller crop to run."""
    g = gold()
    x = golden_volume(g)
    xf = torch.nan_to_num(x, nan=0.0, posinf=1.0, neginf=1.0).cuda()   # the plain padding call does not clean

    def fn():
        m = _seg_net(g, False)
        return {'prob': seg.predict_segmentation_mask(m, x, 'cuda', use_probability_map=True,
                                                      total_memory=float(g['cuda_mem'])),
                'padded': seg.pad_image_with_reflections(xf, pad_size=(4, 6, 2))}
    poisoned(monkeypatch, fn)


def test_ingest(monkeypatch, tmp_path):
    """Stack and the transform chain of tests/test_gpu_input_path.py (img_odd)."""
    G = tip.GOLD
    for suffix, key in [('.tif', 'stack.image_raw'), ('.mask.tif', 'stack.mask_raw'), ('.pwl.tif', 'stack.pwl_raw')]:
        with open(os.path.join(tmp_path, 'vol' + suffix), 'wb') as f:
            np.save(f, G[key])

    def fn():
        data = hdl.Stack(str(tmp_path), image_transforms=[ht.normalize([0.5] * 4, [0.5] * 4)],
                         joint_transforms=[ht.to_float(), ht.reshape()], reader=np.load)
        image, mask, pwl = data[0]
        img = G['img_odd.raw']
        for t in [ht.to_float(), ht.reshape(), ht.normalize(list(G['img_odd.mean']), list(G['img_odd.std'])),
                  ht.to_tensor()]:
            img = t(img)
        return dict(image=image, mask=mask, pwl=pwl, img_odd=img)
    r = poisoned(monkeypatch, fn)
    np.testing.assert_array_equal(tip.bits(r['img_odd']), G['img_odd.out'])
