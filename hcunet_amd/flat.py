"""The one flat parameter / gradient store of the package.

FlatParams(root) makes every parameter of the module tree `root` a view of
ONE fp32 buffer (`flat`) and hands the backward ONE gradient buffer of the
same layout (`grad`) whose per-parameter views it attaches as .grad, so the
native executor takes two base pointers plus offsets, and the optimizer step
and the data-parallel reduction are single launches over contiguous memory.
Unet_Constructor's engine, the layer chains (hcunet_amd.chain), the 1x1x1
convolutions of r_unet.py, optim.Adam and dist.allreduce_gradients all go
through this module.

ready() -- what it detects, what it does not
    The steady-state check follows the (module, name) slots recorded at
    layout time: each slot must still hold the same Parameter object and that
    Parameter must still be the view at base + 4 * offset.  A replaced
    nn.Parameter, `p.data = ...`, and .to() / .cuda() / .double().float()
    (new storage) are therefore detected, and the next ready() walks the
    module tree again.  A submodule swapped into `root` after the layout is
    NOT detected (the slots still point into the old submodule): rebuild the
    model, as the reference's own load() does.  The chains share the limit
    through the modules their cached `ops` name.

    On a miss, parameters that already are consecutive contiguous fp32 views
    of one storage (flat_run) are adopted where they are: `flat` becomes that
    whole storage and the offsets are the storage offsets, nothing is copied.
    This is the case of a Down / Up block of a flattened Unet_Constructor
    called alone (or a sub-block of a flattened r_unet.py model): the block's
    store ALIASES the network's parameter buffer.  Each store still owns its
    own gradient buffer; the block's backward then finds the network's views
    attached as .grad, which are foreign to it, and adds through a temporary
    (below), so the sums stay in the network's buffer.  Anything else is laid
    out in a fresh buffer in parameters() order.  `packed` stores (the U-Net's,
    whose executor derives the offsets itself) adopt only a storage that is
    exactly the packed layout.

grad_target(overwrite) -- the two rules
    Returns (buffer, accumulate, finish): the backward writes into `buffer`,
    adding when `accumulate`, then calls finish().
      * views of `grad` already attached: (grad, 1, no-op) -- in place;
      * foreign .grads (anything else that is not None): a temporary buffer,
        and finish() clones into / adds to each .grad as torch does;
      * nothing attached: `grad` itself, and finish() attaches the cached
        views to the parameters that require grad.
    overwrite=True is the U-Net's rule: its one backward per step writes every
    gradient exactly once, so a fresh buffer (or a temporary) is overwritten,
    accumulate == 0, and nothing is zero-filled.  It examines every parameter,
    so a partially frozen network (a .grad that stays None) takes the
    temporary path from its second backward on.  overwrite=False is the
    chains' rule: a step runs many chain backwards, several per parameter, so
    the fresh buffer (or the temporary) is zero-filled once and every backward
    adds, accumulate == 1.  It examines the trainable parameters only.

stats_tail
    Extra floats behind the gradients: `grad` is the head of `comm`, so a
    data-parallel step reduces gradients and BatchNorm running statistics in
    one collective (hcunet_amd.dist).  The U-Net's engine sets it; chains
    leave 0.
"""
import torch

from . import _lib


def flat_run(tensors):
    """(1-D tensor over the run, total numel) when `tensors` are consecutive
    contiguous fp32 views of one storage, else None."""
    if not tensors:
        return None
    t0 = tensors[0]
    base, off = t0.data_ptr(), 0
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() != base + 4 * off:
            return None
        off += t.numel()
    store = t0.untyped_storage()
    if base + 4 * off > store.data_ptr() + store.nbytes():
        return None   # pointer-adjacent, but past the end of the first tensor's storage
    return torch.empty(0, dtype=torch.float32, device=t0.device).set_(
        store, t0.storage_offset(), (off,), (1,)), off


class FlatParams:
    def __init__(self, root, what='module parameters', packed=False):
        self.root = root
        self.what = what
        self.packed = packed
        self.stats_tail = 0
        self.flat = None
        self.params = None
        self.grad = None     # the head of comm
        self.comm = None
        self._offs = None    # offset in floats of each parameter, in self.params order
        self._index = {}     # id(parameter) -> offset
        self._slots = None   # (module, name) of each parameter, in self.params order
        # (parameter, view of grad, offset) rows, made once per grad (attaching
        # a cached view costs the host ~0.4 us, slicing a new one ~5 us)
        self._rows = None

    def _holds(self, params):
        return len(params) == len(self.params) and all(
            p is q and p.data_ptr() == self.flat.data_ptr() + 4 * o
            for p, q, o in zip(params, self.params, self._offs))

    def ready(self, require_gpu=True):
        flat = self.flat
        if flat is not None and self._slots is not None:
            # fast path, no recursive module walk per call (host time)
            base = flat.data_ptr()
            for (mod, name), q, o in zip(self._slots, self.params, self._offs):
                if mod._parameters.get(name) is not q or q.data_ptr() != base + 4 * o:
                    break
            else:
                return self
        params = list(self.root.parameters())
        if flat is None or not self._holds(params):
            self._layout(params, require_gpu)
        slots = [(mod, name) for _, mod in self.root.named_modules()
                 for name, prm in mod._parameters.items() if prm is not None]
        # unusual registration order (a shared Parameter): keep the full check
        self._slots = slots if len(slots) == len(params) and all(
            mod._parameters[n] is q for (mod, n), q in zip(slots, params)) else None
        return self

    def _layout(self, params, require_gpu):
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32:
                raise RuntimeError('hcunet_amd: parameters must be float32')
            if p.device != dev:
                raise RuntimeError('hcunet_amd: parameters on several devices')
        if require_gpu:
            _lib.require_device(params[0], self.what)
        n = sum(p.numel() for p in params)
        offs = None
        if flat_run(params) is not None:
            store = params[0].untyped_storage()
            if not self.packed or (params[0].storage_offset() == 0 and store.nbytes() == 4 * n):
                flat = torch.empty(0, dtype=torch.float32, device=dev).set_(
                    store, 0, (store.nbytes() // 4,), (1,))
                offs = [p.storage_offset() for p in params]
        if offs is None:
            flat = torch.empty(n, dtype=torch.float32, device=dev)
            offs, off = [], 0
            with torch.no_grad():
                for p in params:
                    k = p.numel()
                    flat[off:off + k].copy_(p.data.reshape(-1))
                    p.data = flat[off:off + k].view_as(p)
                    offs.append(off)
                    off += k
        self.flat, self.params, self._offs = flat, params, offs
        self._index = {id(p): o for p, o in zip(params, offs)}
        self.grad = self.comm = self._rows = None

    def offset(self, p):
        """Offset of parameter p in floats from the flat base; -1 for None."""
        return self._index[id(p)] if p is not None else -1

    def grad_target(self, overwrite):
        flat = self.flat
        n = flat.numel()
        G = self.grad
        if G is None or G.numel() != n or G.device != flat.device:
            self.comm = torch.zeros(n + self.stats_tail, dtype=torch.float32, device=flat.device)
            G = self.grad = self.comm[:n]
            self._rows = None
        rows = self._rows
        if rows is None:
            rows = self._rows = [(p, G[o:o + p.numel()].view_as(p), o)
                                 for p, o in zip(self.params, self._offs)]
        if not overwrite:
            rows = [r for r in rows if r[0].requires_grad]
        grads = [r[0].grad for r in rows]
        if all(g is None for g in grads):
            if not overwrite:
                G.zero_()
            elif _lib.POISON is not None:
                _lib.poison(G)   # accumulate == 0: the backward writes every trainable slot

            def finish():
                for p, v, _ in rows:
                    if p.requires_grad:
                        p.grad = v
            return G, 0 if overwrite else 1, finish
        base = G.data_ptr()
        if all(g is r[1] for g, r in zip(grads, rows)) or all(
                g is not None and g.data_ptr() == base + 4 * o and g.shape == p.shape
                for g, (p, _, o) in zip(grads, rows)):
            return G, 1, _nothing
        tmp = _lib.empty_like(flat) if overwrite else torch.zeros_like(flat)

        def finish_foreign():
            for p, _, o in rows:
                if not p.requires_grad:
                    continue
                g = tmp[o:o + p.numel()].view_as(p)
                if p.grad is None:
                    p.grad = g.clone()
                else:
                    p.grad.add_(g)
        return tmp, 0 if overwrite else 1, finish_foreign


def _nothing():
    return None
