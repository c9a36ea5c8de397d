"""Whole-network parity: hcat.unet.Unet_Constructor on the MI355X vs the CPU
oracle (oracle/unet_oracle.py, itself pinned to the reference by
tests/golden/).  Covers train-mode forward, loss, every parameter gradient,
running statistics, the Adam step and eval-mode forward.

Gradient parity is judged against a DECISION-PINNED fp64 oracle: the GPU's own
ReLU masks and max-pool argmaxes are read from its saved workspace
(hcu_unet_plan_bn_layers) and the fp64 oracle is made to route its backward
through exactly those decisions (unet_oracle.pin_decisions).  A ReLU input or
pool top-2 gap within fp32 rounding of zero makes the routing itself a coin
toss for any fp32 implementation (the fp32 reference included), and the
5-level nets have millions of such inputs; pinning removes that ambiguity, so
every gradient tensor is held to a strict bar (relative L2 <= max(1e-4, 8x the
fp32 noise of the same pinned step on the CPU), max error <= 8x that noise),
with no relaxed floor and no self-referenced check."""
import ctypes

import numpy as np
import pytest
import torch

from hcat.loss import cross_entropy
from hcat.unet import Unet_Constructor
from hcunet_amd import _lib
from hcunet_amd.optim import Adam
from oracle import inputs, unet_oracle as uo
from tests.helpers import REF_KW

pytestmark = pytest.mark.gpu

CONFIGS = {
    'l2': (dict(REF_KW, feature_sizes=[2, 4]), (2, 4, 18, 18, 3)),
    'l3': (dict(REF_KW, feature_sizes=[4, 8, 16]), (2, 4, 44, 44, 5)),
    'l4': (dict(REF_KW, feature_sizes=[4, 8, 16, 32]), (1, 4, 92, 92, 6)),
    'l5_min': (dict(REF_KW, feature_sizes=[8, 16, 32, 64, 128]), (2, 4, 188, 188, 6)),
    'g2_up8': (dict(REF_KW, feature_sizes=[4, 8, 16], groups=2, upsample_kernel=(8, 8, 2)),
               (1, 4, 64, 60, 6)),
    'dil': (dict(REF_KW, feature_sizes=[4, 8, 16], dilation={'conv1': (2, 2, 1), 'conv2': 1}),
            (1, 4, 68, 66, 6)),
    'odd': (dict(image_dimensions=3, in_channels=3, out_channels=2, feature_sizes=[6, 12],
                 kernel={'conv1': (3, 3, 3), 'conv2': (3, 3, 1)}, upsample_kernel=(2, 2, 2),
                 max_pool_kernel=(2, 2, 2), upsample_stride=(2, 2, 2)), (2, 3, 22, 20, 13)),
}

RL2_MAX = 1e-4          # per-tensor relative L2 vs the pinned fp64 oracle
CANCELLED_ABS = 1e-4    # biases whose exact gradient is 0 (feed a train-mode BatchNorm)


def _bn_cancelled(name):
    return name.endswith('conv1.bias') or name.endswith('conv2.bias') or name.endswith('up_conv.bias')


def _build(kw, shape, seed=0):
    torch.manual_seed(seed)
    m = Unet_Constructor(**kw)
    spec = uo.normalize_spec(**kw)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = inputs.make_x(shape)
    return m, spec, state, x


def _mask_pwl(out_shape, pad=(3, 2, 1)):
    B, C, X, Y, Z = out_shape
    ms = (B, C, X + pad[0], Y + pad[1], Z + pad[2])
    return inputs.make_mask(ms), inputs.make_pwl(ms)


def _oshape(spec, state, x):
    net = uo.OracleUnet(spec, state)
    with torch.no_grad():
        return tuple(net.forward(torch.from_numpy(x), training=False).shape)


def gpu_pins(model, out, spec):
    """ReLU masks / pool argmaxes of the GPU forward that produced `out`."""
    x, saved = out.grad_fn.saved_tensors
    plan = model.engine().plan(tuple(x.shape))
    n = plan.n_bn
    infos = (_lib.BNLayerInfo * n)()
    assert _lib.lib().hcu_unet_plan_bn_layers(plan.handle, infos, n) == n
    ys, coefs = {}, {}
    for i, name in enumerate(uo.bn_names(spec)):
        r = infos[i]
        assert r.elem_bytes == 4
        nel = r.B * r.X * r.Y * r.Z * r.Cs
        y = saved[r.y_offset:r.y_offset + nel * 4].view(torch.float32)
        y = y.reshape(r.B, r.X, r.Y, r.Z, r.Cs)[..., :r.C].permute(0, 4, 1, 2, 3).cpu()
        c = saved[r.coef_offset:r.coef_offset + 6 * r.Cs * 4].view(torch.float32)
        c = c.reshape(6, r.Cs)[:, :r.C].cpu()
        ys[name] = y
        coefs[name] = (c[0], c[1])
    return uo.pin_decisions(spec, ys, coefs)


def run_step(m, spec, state, x, mask, pwl):
    """One GPU train step (forward, pixel loss, backward, Adam) plus the pinned
    fp32 / fp64 oracle steps on the same decisions."""
    m = m.cuda().train()
    opt = Adam(m.parameters(), lr=1e-3)
    opt.zero_grad()
    out = m(torch.from_numpy(x).cuda())
    pins = gpu_pins(m, out, spec)
    loss = cross_entropy(out, torch.from_numpy(mask).cuda(), torch.from_numpy(pwl).cuda(),
                         method='pixel')
    loss.backward()
    torch.cuda.synchronize()
    ref32 = uo.train_step(spec, state, x, mask, pwl, dtype=torch.float32)
    p32 = uo.train_step(spec, state, x, mask, pwl, dtype=torch.float32, pins=pins)
    p64 = uo.train_step(spec, state, x, mask, pwl, dtype=torch.float64, pins=pins)
    return m, opt, out, loss, ref32, p32, p64


def check_grads(m, spec, p32, p64, rl2_max=RL2_MAX):
    names = uo.param_names(spec)
    params = dict(m.named_parameters())
    worst = []
    for n in names:
        g = params[n].grad.detach().cpu().double()
        g64 = p64['grads'][n].double()
        g32 = p32['grads'][n].double()
        err = (g - g64).abs().max().item()
        if _bn_cancelled(n):
            worst.append((err / CANCELLED_ABS, n, 'abs', err))
            continue
        noise = (g32 - g64).abs().max().item()
        tol = max(8 * noise, 1e-5 * g64.abs().max().item(), 1e-9)
        nrm = max(g64.norm().item(), 1e-30)
        rl2 = (g - g64).norm().item() / nrm
        rl2_tol = max(rl2_max, 8 * (g32 - g64).norm().item() / nrm)
        worst.append((max(err / tol, rl2 / rl2_tol), n,
                      'max %.3g tol %.3g rl2 %.3g tol %.3g' % (err, tol, rl2, rl2_tol), err))
    worst.sort(key=lambda t: -t[0])
    assert worst[0][0] <= 1.0, worst[:5]
    return worst


def check_adam(m, spec, p64, p32, frac=2e-3, lr=1e-3):
    params = dict(m.named_parameters())
    for n in uo.param_names(spec):
        if _bn_cancelled(n):
            continue
        a = params[n].detach().cpu().double()
        b = p64['state_after'][n].double()
        # one Adam step moves each weight by ~lr (p - lr*g/(|g|+eps) at step 1)
        assert (a - b).abs().max().item() <= 2.0 * lr + 1e-6, n
        diff = (a - b).abs() > 1e-5
        # where |g| is within the fp32 reference's own gradient error, the sign
        # of that step is not determined by fp32 arithmetic (the reference's
        # fp32 step differs from fp64 there too): only determined entries count
        g64 = p64['grads'][n].double()
        # per-element noise: the fp32 reference's own error at that entry,
        # floored at its mean over the tensor
        e32 = (p32['grads'][n].double() - g64).abs()
        determined = g64.abs() > 8.0 * torch.maximum(e32, e32.mean())
        # the check must not pass vacuously: at most 10 % of a tensor excluded
        if g64.numel() >= 32:
            assert determined.double().mean().item() >= 0.90, (n, determined.double().mean().item())
        diff &= determined
        bad = diff.double().mean().item()
        assert bad <= frac, (n, bad)


def check_running_stats(m, spec, ref32, nbt=1):
    sd = m.state_dict()
    for bn in uo.bn_names(spec):
        for s in ('running_mean', 'running_var'):
            a = sd[bn + '.' + s].cpu().double()
            b = ref32['state_after'][bn + '.' + s].double()
            assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item()), (bn, s)
        assert int(sd[bn + '.num_batches_tracked']) == nbt


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_step_parity(name):
    kw, shape = CONFIGS[name]
    m, spec, state, x = _build(kw, shape)
    mask, pwl = _mask_pwl(_oshape(spec, state, x))
    m, opt, out, loss, ref32, p32, p64 = run_step(m, spec, state, x, mask, pwl)
    # forward output: within 1e-4 of the fp32 reference (north-star bar)
    assert out.shape == ref32['out'].shape
    err_out = (out.detach().cpu().double() - ref32['out'].double()).abs().max().item()
    assert err_out <= 1e-4, err_out
    assert abs(loss.item() - p64['loss'].item()) <= 1e-5 * max(1.0, abs(p64['loss'].item()))
    check_grads(m, spec, p32, p64)
    check_running_stats(m, spec, ref32)
    opt.step()
    torch.cuda.synchronize()
    check_adam(m, spec, p64, p32)
    # eval-mode forward with the updated weights and running stats
    m.eval()
    with torch.no_grad():
        oe = m(torch.from_numpy(x).cuda()).cpu()
    net = uo.OracleUnet(spec, {k: v.cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        re = net.forward(torch.from_numpy(x), training=False)
    assert (oe.double() - re.double()).abs().max().item() <= 1e-4


def test_pins_explain_the_routing():
    """The l5_min step has ReLU inputs within fp32 reach of 0 (the reason for
    pinning): show that the unpinned fp64 step differs from the pinned one, and
    that the GPU follows the pinned one."""
    kw, shape = CONFIGS['l5_min']
    m, spec, state, x = _build(kw, shape)
    assert uo.tie_margin(spec, state, x) < 1e-5
    mask, pwl = _mask_pwl(_oshape(spec, state, x))
    m, opt, out, loss, ref32, p32, p64 = run_step(m, spec, state, x, mask, pwl)
    check_grads(m, spec, p32, p64)


def test_bn_cancellation_large_bias_shifted_input():
    """Conv biases of +-40 and an input shifted by +6: every conv output has
    |mean| >> std, where E[y^2] - E[y]^2 from fp32 partial sums loses most of
    its digits.  The pivot-shifted statistics keep the forward within 1e-4 and
    the gradients within the strict bar."""
    kw, shape = CONFIGS['l3']
    m, spec, state, x = _build(kw, shape)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('.bias') and 'batch' not in n:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * 40.0)
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = x + np.float32(6.0)
    mask, pwl = _mask_pwl(_oshape(spec, state, x))
    m, opt, out, loss, ref32, p32, p64 = run_step(m, spec, state, x, mask, pwl)
    # forward output against the fp64 oracle: here the reference's own fp32
    # arithmetic is ~9e-5 from fp64 (|out| ~ 4), so the bar is the larger of
    # 1e-4 and twice that fp32 noise
    out64 = uo.OracleUnet(spec, state, dtype=torch.float64).forward(
        torch.as_tensor(x).double(), training=True).detach()
    noise = (ref32['out'].double() - out64).abs().max().item()
    err_out = (out.detach().cpu().double() - out64).abs().max().item()
    assert err_out <= max(1e-4, 2.0 * noise), (err_out, noise)
    check_grads(m, spec, p32, p64)
    check_running_stats(m, spec, ref32)


def test_full_config2_train_step():
    """Config 2 at full size: [2,4,256,256,16] -> [2,1,68,68,11].  Forward within
    1e-4 of the fp32 reference; loss, every gradient (vs the pinned fp64 step),
    running statistics and the Adam step."""
    kw = dict(REF_KW, feature_sizes=[8, 16, 32, 64, 128])
    m, spec, state, x = _build(kw, (2, 4, 256, 256, 16))
    mask, pwl = inputs.make_mask((2, 1, 256, 256, 16)), inputs.make_pwl((2, 1, 256, 256, 16))
    torch.set_num_threads(16)
    m, opt, out, loss, ref32, p32, p64 = run_step(m, spec, state, x, mask, pwl)
    assert out.shape == (2, 1, 68, 68, 11)
    assert (out.detach().cpu().double() - ref32['out'].double()).abs().max().item() <= 1e-4
    assert abs(loss.item() - p64['loss'].item()) <= 1e-5 * abs(p64['loss'].item())
    check_grads(m, spec, p32, p64)
    check_running_stats(m, spec, ref32)
    opt.step()
    torch.cuda.synchronize()
    check_adam(m, spec, p64, p32)


def test_deterministic_bitwise():
    kw, shape = CONFIGS['l3']
    m, spec, state, x = _build(kw, shape)
    m = m.cuda()
    xs = torch.from_numpy(x).cuda()
    res = []
    for _ in range(2):
        m.load_state_dict({k: v.cuda() for k, v in state.items()})
        for p in m.parameters():
            p.grad = None
        out = m(xs)
        out.sum().backward()
        torch.cuda.synchronize()
        res.append((out.detach().clone(), [p.grad.clone() for p in m.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


def test_grad_accumulation_and_input_grad():
    kw, shape = CONFIGS['l2']
    m, spec, state, x = _build(kw, shape)
    m = m.cuda()
    xs = torch.from_numpy(x).cuda().requires_grad_(True)
    out = m(xs)
    out.sum().backward()
    g1 = [p.grad.clone() for p in m.parameters()]
    dx = xs.grad.detach().cpu().double()
    m.load_state_dict({k: v.cuda() for k, v in state.items()})
    out = m(xs)
    out.sum().backward()
    for p, a in zip(m.parameters(), g1):
        assert torch.allclose(p.grad, 2 * a, rtol=1e-5, atol=1e-7)
    net = uo.OracleUnet(spec, state, dtype=torch.float64)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    net.forward(xr).sum().backward()
    assert (dx - xr.grad).abs().max().item() <= 1e-5 * xr.grad.abs().max().item() + 1e-7


def _weighted_backward(out, seed):
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed)).to(out.device)
    (out * w).sum().backward()


def _clear(m):
    for p in m.parameters():
        p.grad = None


def test_block_alone_on_a_flattened_network_accumulates():
    """A Down block of a flattened network called alone: its store adopts the
    network's parameter buffer (hcunet_amd.flat) and its backward adds into the
    gradients the network's backward attached.  whole + block + whole without
    clearing equals the sum of the three contributions, each computed from a
    cleared state; the parameters are never copied or changed."""
    kw, shape = CONFIGS['l2']
    m, spec, state, x = _build(kw, shape)
    m = m.cuda()
    xs = torch.from_numpy(x).cuda()
    block = m.down_steps[0]
    steps = [lambda: _weighted_backward(m(xs), 11), lambda: _weighted_backward(block(xs), 12),
             lambda: _weighted_backward(m(xs), 11)]
    m(xs)   # flattens
    values = [p.detach().clone() for p in m.parameters()]
    ptrs = [p.data_ptr() for p in m.parameters()]

    def unchanged():
        torch.cuda.synchronize()
        return all(p.data_ptr() == q and torch.equal(p.detach(), v)
                   for p, q, v in zip(m.parameters(), ptrs, values))
    in_block = {id(p) for p in block.parameters()}
    parts = []
    for i, step in enumerate(steps):
        _clear(m)
        step()
        # the block alone reaches its own parameters only
        assert all((p.grad is not None) == (i != 1 or id(p) in in_block) for p in m.parameters())
        parts.append([torch.zeros_like(p, dtype=torch.float64) if p.grad is None else p.grad.double()
                      for p in m.parameters()])
        assert unchanged()
    _clear(m)
    for step in steps:
        step()
        assert unchanged()
    eng_flat = m.engine().flat
    assert block._hcu_flat.flat.untyped_storage().data_ptr() == eng_flat.untyped_storage().data_ptr()
    for p, a, b, c in zip(m.parameters(), *parts):
        assert torch.allclose(p.grad, (a + b + c).float(), rtol=1e-5, atol=1e-7)


def test_partially_frozen_network():
    """out_conv frozen: its parameters keep .grad None, every other gradient is
    bitwise the unfrozen run's; a second backward (the frozen .grad is still
    None, so the gradients go through a temporary buffer) doubles them."""
    kw, shape = CONFIGS['l2']
    m, spec, state, x = _build(kw, shape)
    m = m.cuda()
    xs = torch.from_numpy(x).cuda()
    _weighted_backward(m(xs), 11)
    ref = [p.grad.clone() for p in m.parameters()]
    _clear(m)
    frozen = list(m.out_conv.parameters())
    for p in frozen:
        p.requires_grad_(False)
    _weighted_backward(m(xs), 11)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in frozen)
    for p, g in zip(m.parameters(), ref):
        if not any(p is f for f in frozen):
            assert torch.equal(p.grad, g)
    _weighted_backward(m(xs), 11)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in frozen)
    for p, g in zip(m.parameters(), ref):
        if not any(p is f for f in frozen):
            assert torch.allclose(p.grad, 2 * g, rtol=1e-5, atol=1e-7)
