"""hcat.r_unet (RDCNet, RecursiveUnet) and the callable U-Net Down / Up
blocks on the MI355X vs fixtures produced by the REFERENCE itself
(tests/golden/make_runet_golden.py runs /root/reference/hcat/r_unet.py and
hcat/unet.py on the CPU in fp32 and fp64).

Bars: outputs and losses within max(8x the reference's own fp32-vs-fp64
deviation, a small absolute floor); every gradient tensor (RDCNet, blocks:
in full; RecursiveUnet: as a digest of sum, L2 norm, max|.| and 64 hashed
elements) within max(8x the reference's fp32 noise on that tensor, 1e-5 of
its largest element), against the fp64 run; BatchNorm running statistics
after the training forward (ten updates per BatchNorm in RecursiveUnet)."""
import os

import numpy as np
import pytest
import torch

import hcat.loss as hl
from hcat.r_unet import RDCNet, RecursiveUnet
from hcat.unet import Unet_Constructor
from oracle import inputs
from tests.helpers import REF_KW

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _summary(t):
    t = t.detach().double().reshape(-1).cpu()
    idx = (inputs.splitmix64(99, 64) % np.uint64(t.numel())).astype(np.int64)
    return np.concatenate([[t.sum().item(), t.norm().item(), t.abs().max().item()],
                           t[torch.from_numpy(idx)].numpy()])


def _close(name, got, f32, f64, k=8.0, floor_rel=1e-5, floor_abs=0.0, report=None):
    got, f32, f64 = (np.asarray(v, dtype=np.float64) for v in (got, f32, f64))
    noise = np.abs(f32 - f64).max()
    bar = max(k * noise, floor_rel * np.abs(f64).max(), floor_abs)
    err = np.abs(got - f64).max()
    msg = '%s: max err %.3g, bar %.3g (ref fp32 noise %.3g, max %.3g)' % (name, err, bar, noise,
                                                                        np.abs(f64).max())
    if report is not None:
        report.append((err <= bar, msg))
        return
    assert err <= bar, msg


def _report(rows):
    for ok, msg in rows:
        print(('ok   ' if ok else 'FAIL ') + msg)
    assert all(ok for ok, _ in rows), [m for ok, m in rows if not ok]


def _train_step(net, g, x):
    dev = torch.device('cuda', 0)
    out = net(torch.from_numpy(x).to(dev))
    oshape = tuple(g['out_shape'])
    assert tuple(out.shape) == oshape
    mshape = (oshape[0], 1) + oshape[2:]
    mask = torch.from_numpy(inputs.make_mask(mshape)).to(dev)
    pwl = torch.from_numpy(inputs.make_pwl(mshape)).to(dev)
    vec = torch.from_numpy(g['vec']).to(dev)
    loss = hl.cross_entropy(out[:, 0:1], mask, pwl, method='pixel') + hl.MSELoss(out[:, 2:], vec)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), float(loss.item())


def test_rdcnet_train_step_matches_reference():
    g = np.load(os.path.join(GOLD, 'runet_rdc.npz'))
    torch.manual_seed(int(g['seed']))
    net = RDCNet(4, 5)
    for k, v in net.state_dict().items():     # torch's default init in the reference's order
        np.testing.assert_array_equal(v.numpy(), g['init.' + k], err_msg=k)
    net = net.cuda().train()
    x = inputs.make_x(tuple(g['x_shape']))
    out, loss = _train_step(net, g, x)
    _close('out', out.numpy(), g['f32.out'], g['f64.out'], floor_abs=1e-5)
    _close('loss', loss, g['f32.loss'], g['f64.loss'], floor_abs=1e-6)
    rows = []
    for k, p in net.named_parameters():
        _close('grad ' + k, p.grad.cpu().numpy(), g['f32.grad.' + k], g['f64.grad.' + k], report=rows)
    _report(rows)


def test_recursive_unet_train_step_matches_reference():
    g = np.load(os.path.join(GOLD, 'runet_rec.npz'))
    x = inputs.make_x(tuple(g['x_shape']))
    # eval-mode BatchNorm (running statistics): the gradients do not pass ten
    # steps of batch statistics and are held to the strict bar
    torch.manual_seed(int(g['seed']))
    net = RecursiveUnet(image_dimensions=3)
    for k, v in net.state_dict().items():
        np.testing.assert_allclose(_summary(v), g['init.' + k], rtol=0, atol=1e-6, err_msg=k)
    net = net.cuda().eval()
    out_e, loss_e = _train_step(net, g, x)
    _close('eval out', out_e.numpy(), g['e32.out'], g['e64.out'], floor_abs=1e-5)
    _close('eval loss', loss_e, g['e32.loss'], g['e64.loss'], floor_abs=1e-6)
    rows = []
    for k, p in net.named_parameters():
        _close('eval grad ' + k, _summary(p.grad), g['e32.grad.' + k], g['e64.grad.' + k],
               floor_rel=1e-5, report=rows)
    _report(rows)
    # train mode
    torch.manual_seed(int(g['seed']))
    net = RecursiveUnet(image_dimensions=3).cuda().train()
    out, loss = _train_step(net, g, x)
    _close('out', out.numpy(), g['f32.out'], g['f64.out'], floor_abs=1e-4)
    _close('loss', loss, g['f32.loss'], g['f64.loss'], floor_abs=1e-5)
    # Train-mode gradients pass ten recurrent steps of BatchNorm batch
    # statistics over 64 voxels at the bottom level (16x16x4 input, B = 1) and
    # are ill-conditioned: the reference's own fp32 run moves by up to ~20 % of
    # a tensor's digest when its input is perturbed by 1e-6 relative noise
    # (fixture sens.grad.*, make_runet_golden.py), the size of a reordered fp32
    # reduction's rounding.  Bar per tensor: digest relative L2 (sum, norm,
    # max, 64 samples) against the fp64 run <= max(2e-2, 1.5 x that envelope);
    # the eval-mode gradients above carry the strict check.
    rows = []
    for k, p in net.named_parameters():
        d, d64 = _summary(p.grad), g['f64.grad.' + k]
        rel = np.linalg.norm(d - d64) / max(np.linalg.norm(d64), 1e-12)
        bar = max(2e-2, 1.5 * float(g['sens.grad.' + k]))
        ok = rel <= bar or np.abs(d - d64).max() <= 1e-4   # BN-cancelled biases: exact 0
        rows.append((ok, 'train grad %s: digest rel L2 %.3g (bar %.3g)' % (k, rel, bar)))
    _report(rows)
    # ten BatchNorm updates per module in one forward (r_unet.py:139-160)
    for k, b in net.named_buffers():
        got = b.detach().cpu().double().numpy()
        if k.endswith('num_batches_tracked'):
            assert int(got) == int(g['f32.buf.' + k]), k
        else:
            _close('buf ' + k, got, g['f32.buf.' + k], g['f64.buf.' + k], floor_rel=1e-5, floor_abs=1e-6)


def test_unet_blocks_callable_on_their_own():
    g = np.load(os.path.join(GOLD, 'unet_blocks.npz'))
    kw = dict(REF_KW, feature_sizes=[4, 8, 16])
    torch.manual_seed(5)
    net = Unet_Constructor(**kw)
    for k, v in net.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), g['init.' + k], err_msg=k)
    net = net.cuda().train()
    dev = torch.device('cuda', 0)
    d, u = net.down_steps[0], net.up_steps[0]
    xd = torch.from_numpy(inputs.make_x(tuple(g['xd_shape']))).to(dev).requires_grad_(True)
    od = d(xd)
    gd = torch.from_numpy(inputs.make_x(tuple(od.shape))).to(dev)
    (od * gd).sum().backward()
    _close('down out', od.detach().cpu().numpy(), g['f32.down.out'], g['f64.down.out'], floor_abs=1e-5)
    _close('down dx', xd.grad.cpu().numpy(), g['f32.down.dx'], g['f64.down.dx'])
    for k, p in d.named_parameters():
        _close('down grad ' + k, p.grad.cpu().numpy(), g['f32.down.grad.' + k], g['f64.down.grad.' + k],
               floor_abs=1e-4 if k.endswith('bias') and 'conv' in k else 0.0)
    for k, b in d.named_buffers():
        if not k.endswith('num_batches_tracked'):
            _close('down buf ' + k, b.cpu().numpy(), g['f32.down.buf.' + k], g['f64.down.buf.' + k],
                   floor_abs=1e-6)
    xu = torch.from_numpy(inputs.make_x(tuple(g['xu_shape']))).to(dev).requires_grad_(True)
    ou = u(xu, torch.zeros(tuple(g['skip']), device=dev))
    gu = torch.from_numpy(inputs.make_x(tuple(ou.shape))).to(dev)
    (ou * gu).sum().backward()
    _close('up out', ou.detach().cpu().numpy(), g['f32.up.out'], g['f64.up.out'], floor_abs=1e-5)
    _close('up dx', xu.grad.cpu().numpy(), g['f32.up.dx'], g['f64.up.dx'])
    for k, p in u.named_parameters():
        _close('up grad ' + k, p.grad.cpu().numpy(), g['f32.up.grad.' + k], g['f64.up.grad.' + k],
               floor_abs=1e-4 if k.endswith('bias') else 0.0)
    # the upsampled tensor larger than the skip: torch.cat raises (hcat/unet.py:312)
    with pytest.raises(RuntimeError):
        u(xu.detach(), torch.zeros(2, 8, 10, 16, 6, device=dev))


def _rl2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


@pytest.mark.parametrize('tile', [(64, 64, 24), (512, 512, 24)])
def test_rdcnet_bf16_autocast_relative(tile):
    """BASELINE config 5 runs RDCNet under bf16 autocast; the reference has no
    bf16 path, so this build's distance to the fp32 oracle must be within 1.5x
    of torch's own CPU bf16 autocast of the oracle (output and median
    gradient relative L2), as tests/test_gpu_bf16.py does for the U-Net --
    on a small tile and on config 5's own 512x512x24 tile (where the dilated
    convolutions take their sub-lattice tilings; ~40 s of host time)."""
    from oracle import loss_oracle as lo, runet_oracle as ro
    torch.set_num_threads(16)
    torch.manual_seed(0)
    net = RDCNet(4, 5)
    shape = (1, 4) + tile
    x = torch.from_numpy(inputs.make_x(shape))
    oshape = (1, 5) + shape[2:]
    mshape = (1, 1) + shape[2:]
    mask = torch.from_numpy(inputs.make_mask(mshape))
    pwl = torch.from_numpy(inputs.make_pwl(mshape))
    vec = torch.from_numpy(inputs.make_x((1, 3) + shape[2:]) * 0.5)

    def oracle(autocast):
        s = ro.state_of(net, torch.float32)
        with torch.autocast('cpu', dtype=torch.bfloat16, enabled=autocast):
            out = ro.rdcnet_forward(s, x)
        out = out.float()
        loss = lo.cross_entropy(out[:, 0:1], mask, pwl, method='pixel') + lo.MSELoss(out[:, 2:], vec)
        loss.backward()
        return out.detach(), loss.item(), {k: s[k].grad for k, _ in net.named_parameters()}
    ref_out, ref_loss, ref_g = oracle(False)
    a_out, a_loss, a_g = oracle(True)
    m = net.cuda().train()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m(x.cuda())
        loss = hl.cross_entropy(out[:, 0:1], mask.cuda(), pwl.cuda(), method='pixel') + \
            hl.MSELoss(out[:, 2:], vec.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert out.shape == oshape
    ours = dict(out=_rl2(out.detach().cpu(), ref_out),
                g=float(np.median([_rl2(p.grad.cpu(), ref_g[k]) for k, p in m.named_parameters()])))
    auto = dict(out=_rl2(a_out, ref_out), g=float(np.median([_rl2(a_g[k], ref_g[k]) for k in ref_g])))
    print('RDCNet bf16 vs fp32 oracle: ours out %.3g grad median %.3g | torch autocast out %.3g grad %.3g'
          % (ours['out'], ours['g'], auto['out'], auto['g']))
    assert ours['out'] <= 1.5 * auto['out'] + 1e-3
    assert ours['g'] <= 1.5 * auto['g'] + 1e-2
    assert abs(loss.item() - ref_loss) <= 1e-2 * abs(ref_loss)


def test_rdcnet_full_tile_512x512x24_matches_oracle():
    """BASELINE config 5's tile: RDCNet(4, 5) fp32 train step (forward, pixel
    BCE + MSE, backward) on one 512x512x24 tile, where the dilated 5^3
    convolutions run their sub-lattice (space-to-batch) tilings that the small
    fixture never picks.  Checked against the oracle restatement
    (oracle/runet_oracle.py, pinned to the reference by runet_rdc.npz) run on
    the host in fp32 (an fp64 oracle step takes ~15 min of host time here:
    torch's CPU fp64 dilated convolution has no fast path; the fixture test
    carries the fp64-anchored bar).  Bars, for two fp32 computations in
    different summation orders: output within 2e-4 of its largest element,
    loss within 1e-5 relative, every gradient within 1e-3 relative L2 and 1e-3
    of its largest element (measured: see the printed report)."""
    from oracle import loss_oracle as lo
    from oracle import runet_oracle as ro
    torch.set_num_threads(16)
    torch.manual_seed(7)
    net = RDCNet(4, 5)
    st = ro.state_of(net, torch.float32)
    shape = (1, 4, 512, 512, 24)
    x = inputs.make_x(shape)
    oshape = (1, 5) + shape[2:]
    mshape = (1, 1) + shape[2:]
    mask, pwl = inputs.make_mask(mshape), inputs.make_pwl(mshape)
    vec = (inputs.make_x((1, 3) + shape[2:], seed=4) * 0.5).astype(np.float32)
    g = {'out_shape': oshape, 'vec': vec}
    net = net.cuda().train()
    out, loss = _train_step_with(net, g, x, mask, pwl)
    o = ro.rdcnet_forward(st, torch.from_numpy(x))
    ls = lo.cross_entropy(o[:, 0:1], torch.from_numpy(mask).float(), torch.from_numpy(pwl),
                          method='pixel') + lo.MSELoss(o[:, 2:], torch.from_numpy(vec))
    ls.backward()
    o = o.detach()
    rows = []
    err = (out - o).abs().max().item()
    bar = 2e-4 * o.abs().max().item() + 1e-6
    rows.append((err <= bar, 'out: max err %.3g, bar %.3g' % (err, bar)))
    lerr = abs(loss - ls.item()) / abs(ls.item())
    rows.append((lerr <= 1e-5, 'loss: rel err %.3g (%.6f vs %.6f)' % (lerr, loss, ls.item())))
    for k, p in net.named_parameters():
        a, b = p.grad.cpu().double(), st[k].grad.double()
        rel = ((a - b).norm() / max(b.norm().item(), 1e-30)).item()
        mx = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
        rows.append((rel <= 1e-3 and mx <= 1e-3, 'grad %s: rel L2 %.3g, max %.3g of max' % (k, rel, mx)))
    _report(rows)


def _train_step_with(net, g, x, mask, pwl):
    dev = torch.device('cuda', 0)
    out = net(torch.from_numpy(x).to(dev))
    assert tuple(out.shape) == tuple(g['out_shape'])
    vec = torch.from_numpy(g['vec']).to(dev)
    loss = hl.cross_entropy(out[:, 0:1], torch.from_numpy(mask).to(dev), torch.from_numpy(pwl).to(dev),
                            method='pixel') + hl.MSELoss(out[:, 2:], vec)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), float(loss.item())


def test_rdcnet_bf16_residual_error_does_not_compound_512x512x24():
    """BASELINE config 5's tile (512x512x24) under bf16 autocast: the
    recurrence's residual state y stays fp32 (r_unet.py:223-225 under
    autocast: fp32 zeros + bf16 block output -> fp32), so its distance to the
    fp32 run (this build's fp32 path, pinned to the oracle at this tile by
    test_rdcnet_full_tile_512x512x24_matches_oracle) after each of the 10
    steps stays at the level of one bf16 block evaluation instead of adding a
    bf16 rounding of the state every step: relative L2 of y_t <= 2e-2 for
    every t, and y_10's error within 3x of y_1's."""
    torch.manual_seed(0)
    net = RDCNet(4, 5).cuda().train()
    x = torch.from_numpy(inputs.make_x((1, 4, 512, 512, 24))).cuda()
    traces = {}
    for bf16 in (False, True):
        net._y_trace = []
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=bf16):
            net(x)
        traces[bf16] = net._y_trace
    net._y_trace = None
    assert all(t.dtype == torch.float32 for t in traces[True])
    # (channels-last states padded to the vector width: fp32 12, bf16 16 channels; 10 are real)
    errs = [((b[..., :10] - a[..., :10]).norm() / a[..., :10].norm().clamp_min(1e-30)).item()
            for a, b in zip(traces[False], traces[True])]
    print('RDCNet bf16 vs fp32, residual state y_t relative L2 per step:', ' '.join('%.2e' % e for e in errs))
    assert max(errs) <= 2e-2, errs
    assert errs[-1] <= 3.0 * errs[0] + 1e-3, errs


def _step_outputs(net, x):
    net.zero_grad(set_to_none=True)
    out = net(x)
    (out.float() ** 2).mean().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), [p.grad.detach().cpu().clone() for p in net.parameters()]


def _fresh_like(net):
    m = RDCNet(4, 5)
    m.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return m.cuda().train()


def _assert_same(a, b):
    assert torch.equal(a[0], b[0])
    for ga, gb in zip(a[1], b[1]):
        assert torch.equal(ga, gb)


def test_chain_weight_images_follow_parameter_updates():
    """The layer chains keep their packed weight images across calls (a
    recurrence re-lays them once per parameter change, not once per call):
    after every way the parameters change -- in-place torch ops, this
    package's Adam, .data writes with invalidate_weight_images(), an eval
    forward before the training step -- the step equals a fresh module's with
    the same state, bitwise."""
    from hcunet_amd import chain as ch
    from hcunet_amd.optim import Adam
    g = np.load(os.path.join(GOLD, 'runet_rdc.npz'))
    torch.manual_seed(3)
    net = RDCNet(4, 5).cuda().train()
    x = torch.from_numpy(inputs.make_x(tuple(g['x_shape']))).cuda()
    _step_outputs(net, x)
    with torch.no_grad():                       # in-place torch op: version counters move
        for p in net.parameters():
            p.mul_(0.9)
    _assert_same(_step_outputs(net, x), _step_outputs(_fresh_like(net), x))
    opt = Adam(net.parameters(), lr=1e-2)       # raw-pointer writes: the optimizer's epoch
    _step_outputs(net, x)
    opt.step()
    _assert_same(_step_outputs(net, x), _step_outputs(_fresh_like(net), x))
    for p in net.parameters():                  # .data bypasses the version counter
        p.data.mul_(1.1)
    ch.invalidate_weight_images()
    _assert_same(_step_outputs(net, x), _step_outputs(_fresh_like(net), x))
    with torch.no_grad():                       # eval forward lays out the forward images only
        for p in net.parameters():
            p.mul_(0.95)
    net.eval()
    with torch.no_grad():
        net(x)
    net.train()
    _assert_same(_step_outputs(net, x), _step_outputs(_fresh_like(net), x))
    # a second forward with other weights before the first one's backward:
    # the backward would read the new weight images -- it raises instead
    net.zero_grad(set_to_none=True)
    out1 = net(x)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)
    net(x)
    with pytest.raises(RuntimeError, match='modified'):
        (out1.float() ** 2).mean().backward()


@pytest.mark.parametrize('dtype,widths', [
    (dt, w) for dt in (torch.bfloat16, torch.float32) for w in ((16, 16), (16, 16, 16, 16, 16))] + [
    (torch.float32, (8, 24, 4, 4)), (torch.bfloat16, (8, 24, 8, 16))])
def test_channel_cat_matches_torch_cat(dtype, widths, monkeypatch):
    """hcu_cl_cat (RDCNet's recurrence cats, hcat/r_unet.py:223,362): forward
    bitwise equal to torch.cat(dim=-1), and each part's gradient bitwise
    equal to torch.cat's backward (contiguous tensors here; rows of 16-byte
    multiples, narrow parts included), into NaN-prefilled outputs."""
    from hcunet_amd import _lib
    from hcunet_amd.r_unet import cl_cat
    monkeypatch.setattr(_lib, 'POISON', 0xFF)
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    assert all(w % vec == 0 for w in widths)
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(7)
    parts = [torch.randn(1, 37, 29, 11, w, generator=g).to(dtype).to(dev).requires_grad_() for w in widths]
    ref = [p.detach().clone().requires_grad_() for p in parts]
    out = cl_cat(parts)
    want = torch.cat(ref, dim=-1)
    assert out.dtype == want.dtype and out.shape == want.shape
    assert torch.equal(out, want)
    dout = torch.randn(want.shape, generator=g).to(dtype).to(dev)
    out.backward(dout)
    want.backward(dout)
    for p, r in zip(parts, ref):
        assert p.grad.is_contiguous() and torch.equal(p.grad, r.grad)


@pytest.mark.parametrize('use', ['both', 'cast', 'fp32'])
def test_residual_add_matches_torch(use, monkeypatch):
    """hcu_resid_fwd/bwd (RDCNet's residual under autocast, hcat/r_unet.py
    :223-225): m (bf16) + y (fp32) and its bf16 cast bitwise equal to torch's
    promoting add and .to(), and so are the gradients of m and y with either
    or both outputs used; every output NaN-prefilled."""
    from hcunet_amd import _lib
    from hcunet_amd.r_unet import resid_add
    monkeypatch.setattr(_lib, 'POISON', 0xFF)
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(11)
    m = torch.randn(1, 33, 21, 13, 16, generator=g).to(torch.bfloat16).to(dev).requires_grad_()
    y = torch.randn(1, 33, 21, 13, 16, generator=g).to(dev).requires_grad_()
    m2, y2 = m.detach().clone().requires_grad_(), y.detach().clone().requires_grad_()
    s, sc = resid_add(m, y)
    t = m2 + y2
    tc = t.to(torch.bfloat16)
    assert s.dtype == torch.float32 and sc.dtype == torch.bfloat16
    assert torch.equal(s, t) and torch.equal(sc, tc)
    d32 = torch.randn(t.shape, generator=g).to(dev)
    dc = torch.randn(t.shape, generator=g).to(torch.bfloat16).to(dev)
    if use == 'both':
        ((s * d32).sum() + (sc.float() * dc.float()).sum()).backward()
        ((t * d32).sum() + (tc.float() * dc.float()).sum()).backward()
    elif use == 'cast':
        sc.backward(dc)
        tc.backward(dc)
    else:
        s.backward(d32)
        t.backward(d32)
    assert torch.equal(m.grad, m2.grad) and torch.equal(y.grad, y2.grad)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_fan_gradient_sum(dtype, monkeypatch):
    """hcu_sum_parts behind fan(): the k consumers' gradients summed in fp32
    in consumer order and rounded once (bitwise equal to that sum in torch),
    unused consumers skipped; the sum goes into a NaN-prefilled output."""
    from hcunet_amd import _lib
    from hcunet_amd.r_unet import fan
    monkeypatch.setattr(_lib, 'POISON', 0xFF)
    dev = torch.device('cuda', 0)
    g = torch.Generator(device='cpu').manual_seed(5)
    t = torch.randn(1, 17, 19, 13, 16, generator=g).to(dtype).to(dev).requires_grad_()
    ws = [torch.randn(t.shape, generator=g).to(dtype).to(dev) for _ in range(6)]
    outs = fan(t, 7)
    assert len(outs) == 7 and all(torch.equal(o, t) for o in outs)
    loss = sum((o.float() * w.float()).sum() for o, w in zip(outs, ws))   # outs[6] unused
    loss.backward()
    acc = ws[0].float()
    for w in ws[1:]:
        acc = acc + w.float()
    assert t.grad.dtype == dtype and torch.equal(t.grad, acc.to(dtype))


_RDC_CHILD = r'''
import sys, torch
sys.path.insert(0, %(root)r)
import hcat.loss as hl
from hcat.r_unet import RDCNet
from oracle import inputs
torch.manual_seed(0)
net = RDCNet(4, 5).cuda().train()
shape = %(shape)r
x = torch.from_numpy(inputs.make_x(shape)).cuda()
mshape = (1, 1) + shape[2:]
mask = torch.from_numpy(inputs.make_mask(mshape)).cuda()
pwl = torch.from_numpy(inputs.make_pwl(mshape)).cuda()
vec = torch.from_numpy(inputs.make_x((1, 3) + shape[2:]) * 0.5).cuda()
with torch.autocast('cuda', dtype=torch.bfloat16):
    out = net(x)
    loss = hl.cross_entropy(out[:, 0:1], mask, pwl, method='pixel') + hl.MSELoss(out[:, 2:], vec)
loss.backward()
torch.cuda.synchronize()
torch.save({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, %(out)r)
'''


def _rdc_child(tmp_path, tag, env_extra, shape):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / ('%s.pt' % tag))
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, '-c', _RDC_CHILD % dict(root=root, out=out, shape=shape)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out, weights_only=True)


@pytest.mark.parametrize('shape', [(1, 4, 64, 64, 24), (1, 4, 40, 56, 20)])
def test_rdcnet_bf16_weight_gradient_all_taps_matches_split(tmp_path, shape):
    """The bf16 weight gradient of RDCNet's 5x5x5 convolutions with all 125
    taps in one block (each voxel tile staged once, HCU_BW_ALLTAPS default)
    against the form that splits the taps over 4 blocks (HCU_BW_ALLTAPS=0):
    the same products summed over other slab partitions, so every gradient
    tensor agrees to fp32 reassociation of the bf16 products (relative L2
    <= 1e-4; the dilated branches' tensors are the ones that differ)."""
    a = _rdc_child(tmp_path, 'all', {'HCU_BW_ALLTAPS': '1'}, shape)
    b = _rdc_child(tmp_path, 'split', {'HCU_BW_ALLTAPS': '0'}, shape)
    bad = []
    for k in a:
        r = _rl2(a[k], b[k])
        if not r <= 1e-4:
            bad.append((k, r))
    assert not bad, bad


def test_rdcnet_bf16_cat_free_mixing_matches_cat_and_chain(monkeypatch):
    """The bf16 RDCNet recurrence's two channel cats + 1x1x1 convolutions as
    one native op each (r_unet.pw_conv: hcu_pw_conv_forward / _backward on
    the separate parts) against cl_cat + the layer chain (HCU_PW_CAT=0, the
    chain's own pointwise kernels): the same kernels and summation order, so
    the output, the loss and every gradient must be bitwise equal."""
    torch.manual_seed(3)
    net = RDCNet(4, 5).cuda().train()
    shape = (1, 4, 64, 48, 24)
    x = torch.from_numpy(inputs.make_x(shape)).cuda()
    mshape = (1, 1) + shape[2:]
    mask = torch.from_numpy(inputs.make_mask(mshape)).cuda()
    pwl = torch.from_numpy(inputs.make_pwl(mshape)).cuda()
    res = {}
    for arm in ('0', '1'):
        monkeypatch.setenv('HCU_PW_CAT', arm)
        net.zero_grad(set_to_none=True)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = net(x)
            loss = hl.cross_entropy(out[:, 0:1], mask, pwl, method='pixel')
        loss.backward()
        torch.cuda.synchronize()
        res[arm] = (out.detach().cpu(), loss.item(), [p.grad.detach().cpu().clone() for p in net.parameters()])
    (o0, l0, g0), (o1, l1, g1) = res['0'], res['1']
    assert torch.equal(o0, o1) and l0 == l1
    for (k, _), a, b in zip(net.named_parameters(), g0, g1):
        assert torch.equal(a, b), k


@pytest.mark.parametrize('nparts,part_c,cout,nvox', [(5, 10, 10, 786), (2, 10, 10, 333), (1, 16, 16, 17),
                                                      (3, 8, 5, 1), (2, 10, 10, 0)])
def test_pw_conv_c_abi_matches_torch(nparts, part_c, cout, nvox):
    """hcu_pw_conv_forward / _backward (include/hcunet.h) on their own: the
    cat of `nparts` channels-last bf16 parts of part_c channels (16-byte
    padded slots) through a 1x1x1 Conv3d, against fp64 torch on the same
    bf16-representable operands -- ragged voxel counts (not a multiple of the
    kernels' 16-voxel groups), a single voxel and an empty input; input
    gradients in the parts' layout with their padding slots 0; dW / db
    accumulated onto existing values (accumulate = 1)."""
    import ctypes
    from hcunet_amd import _lib
    from hcunet_amd.chain import cl_channels
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(nparts * 100 + nvox)
    pcs, ocs = cl_channels(part_c, True), cl_channels(cout, True)
    cin = nparts * part_c
    w = torch.randn(cout, cin, generator=g).bfloat16().float()
    b = torch.randn(cout, generator=g)
    xs = [torch.randn(nvox, part_c, generator=g).bfloat16().float() for _ in range(nparts)]
    dy = torch.randn(nvox, cout, generator=g).bfloat16().float()
    x = torch.cat(xs, 1).double() if nvox else torch.zeros(0, cin, dtype=torch.float64)
    y = x @ w.double().t() + b.double()
    dx = dy.double() @ w.double()
    dw = dy.double().t() @ x
    db = dy.double().sum(0)
    pad = lambda t, c: torch.nn.functional.pad(t, (0, c - t.shape[1])).to(torch.bfloat16).to(dev).contiguous()  # noqa: E731
    parts = [pad(t, pcs) for t in xs]
    nan = float('nan')   # every output and workspace prefilled: each word must be written
    out = torch.full((nvox, ocs), nan, dtype=torch.bfloat16, device=dev)
    L = _lib.lib()
    ptrs = (ctypes.c_void_p * nparts)(*[p.data_ptr() for p in parts])
    wd, bd = w.to(dev), b.to(dev)
    st = _lib.stream_handle(dev)
    _lib.check(L.hcu_pw_conv_forward(ptrs, nparts, part_c, pcs, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out),
                                     nvox, cout, ocs, st), 'pw forward')
    dparts = [torch.full_like(p, nan) for p in parts]
    dptrs = (ctypes.c_void_p * nparts)(*[d.data_ptr() for d in dparts])
    gw, gb = torch.ones(cout, cin, device=dev), torch.ones(cout, device=dev)   # accumulated onto
    nw = int(L.hcu_pw_conv_work_floats(nvox, nparts, pcs, cout))
    work = torch.full((max(nw, 1),), nan, device=dev)
    _lib.check(L.hcu_pw_conv_backward(ptrs, nparts, part_c, pcs, _lib.ptr(wd), _lib.ptr(pad(dy, ocs)), cout, ocs,
                                      dptrs, _lib.ptr(gw), _lib.ptr(gb), nvox, _lib.ptr(work), nw, 1, st),
               'pw backward')
    torch.cuda.synchronize()
    assert not out[:, cout:].any()
    got_dx = torch.cat([d[:, :part_c] for d in dparts], 1).float().cpu() if nvox else torch.zeros(0, cin)
    for d in dparts:
        assert not d[:, part_c:].any()
    scale = lambda t: max(t.abs().max().item() if t.numel() else 0.0, 1e-6)  # noqa: E731
    assert (out[:, :cout].float().cpu().double() - y).abs().max().item() <= 1e-2 * scale(y) if nvox else True
    assert (got_dx.double() - dx).abs().max().item() <= 1e-2 * scale(dx) if nvox else True
    assert (gw.cpu().double() - 1 - dw).abs().max().item() <= 2e-3 * scale(dw) + 1e-6
    assert (gb.cpu().double() - 1 - db).abs().max().item() <= 2e-3 * scale(db) + 1e-6
