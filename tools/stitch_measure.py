"""Timings of the tiled stitch quoted in DESIGN.md §3 (whole-stack instance
labels): python tools/stitch_measure.py [result.json], from the repository
root on an MI355X.
  A: hcu_vec_label_paste against the unfused route it replaces (hcu_vec_label,
     then a torch remap, mask and sliced assignment), one 512 x 512 x 24 window
     with 100 peaks and an fp16 field, alternating in one process;
  B: a 1024 x 1024 x 24 stack through RDCNet with the default tile and halo,
     ms per window of forward, votes + smooth, peak read-back and label-paste.
Convolution tilings come from the table and the cost model (HCU_BCONV_TUNE=1)
unless the environment says otherwise."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
os.environ.setdefault('HCU_BCONV_TUNE', '1')
from hcunet_amd import _lib, instances, segment   # noqa: E402
from hcunet_amd.r_unet import RDCNet   # noqa: E402

dev = torch.device('cuda', 0)
res = {}


def ms_events(fn, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


# ---- A: one 512 x 512 x 24 window, 100 peaks, fp16 field, inside a 1024 x 1024 x 24 int32 volume
X, Y, Z = 512, 512, 24
rng = np.random.default_rng(1)
cen = np.array([(26 + 51 * i, 26 + 51 * j, 6 + 12 * ((i + j) % 2)) for i in range(10) for j in range(10)])
gx, gy = np.arange(X), np.arange(Y)
ix, iy = np.clip((gx - 26 + 25) // 51, 0, 9), np.clip((gy - 26 + 25) // 51, 0, 9)
k = ix[:, None] * 10 + iy[None, :]                       # nearest centre in x, y
grid = np.indices((X, Y, Z)).astype(np.float32)
to = np.moveaxis(cen[k], -1, 0)[:, :, :, None].astype(np.float32) - grid
v = (to[::-1] + rng.normal(0, 0.6, size=(3, X, Y, Z)).astype(np.float32)).astype(np.float16)
vec = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
mask = torch.from_numpy(rng.random((X, Y, Z)) > 0.1).to(dev)
t, code, stride = instances._planes(vec, dev, 'measure')
peaks = cen.astype(np.int64)
window = dict(core_lo=(256, 256, 0), core_hi=(768, 768, 24), lo=(256, 256, 0), hi=(768, 768, 24))
ids_host = np.arange(1, 101, dtype=np.int32)
ids_host[::7] = 0                                       # some peaks another window's
shape = (1024, 1024, 24)
fused_vol = torch.zeros(shape, dtype=torch.int32, device=dev)
unfused_vol = torch.zeros(shape, dtype=torch.int32, device=dev)
table = torch.from_numpy(np.concatenate([peaks.astype(np.int32).reshape(-1), ids_host])).to(dev)
remap = torch.from_numpy(np.concatenate([[0], ids_host]).astype(np.int32)).to(dev)
m8 = mask.view(torch.uint8)
inf = float('inf')
bounds = (ctypes.c_float * 6)(-inf, inf, -inf, inf, -inf, inf)   # open: what the unfused route computes


def fused():
    _lib.check(_lib.lib().hcu_vec_label_paste(_lib.ptr(t), code, stride, X, Y, Z, _lib.ptr(table),
                                              _lib.ptr(table[300:]), 100, _lib.ptr(m8), _lib.HCU_U8, bounds,
                                              _lib.ptr(fused_vol), *shape, 256, 256, 0, _lib.stream_handle(dev)))


def unfused():
    label = instances.vec_label(t, code, stride, peaks, mask, 1)        # float64 tile, 0 background / masked
    g = remap[label.long()]                                              # the remap
    keep = g != 0                                                        # the mask
    unfused_vol[256:768, 256:768, :][keep] = g[keep]                     # the sliced masked assignment


def unfused_where():   # the cheapest torch form of the same: one where into the slice
    label = instances.vec_label(t, code, stride, peaks, mask, 1)
    g = remap[label.long()]
    view = unfused_vol[256:768, 256:768, :]
    view.copy_(torch.where(g != 0, g, view))


for f in (fused, unfused, unfused_where):
    for _ in range(3):
        f()
torch.cuda.synchronize()
assert torch.equal(fused_vol, unfused_vol) and int((fused_vol != 0).sum()) > 1000000
tf, tu, tw = [], [], []
for _ in range(15):                                      # interleaved, one process
    tf += ms_events(fused, 1)
    tu += ms_events(unfused, 1)
    tw += ms_events(unfused_where, 1)
for name, xs in (('fused', tf), ('unfused', tu), ('unfused_where', tw)):
    res['A_' + name] = dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))
_lib.lib().hcu_timing_enable(1)
for _ in range(5):
    fused()
    instances.vec_label(t, code, stride, peaks, mask, 1)
torch.cuda.synchronize()
rep = _lib.timing_report()
_lib.lib().hcu_timing_disable()
res['A_kernels'] = {k2: v2['ms'] / v2['count'] for k2, v2 in rep.items()}
res['A_painted_fraction'] = float((fused_vol[256:768, 256:768] != 0).float().mean())
print(json.dumps(res, indent=1), flush=True)

# ---- B: a 1024 x 1024 x 24 stack through RDCNet with the default tile and halo
torch.manual_seed(3)
net = RDCNet(4, 5)
with torch.no_grad():
    net.transposed_conv.weight.mul_(25.0)
net = net.to(dev).eval()
image = torch.from_numpy(np.random.default_rng(2).normal(0, 1, size=(1, 4, 1024, 1024, 24)).astype(np.float32)).to(dev)
wins = instances.windows((1024, 1024, 24), (384, 384, None), (64, 64, 0))


def staged(timed):
    labels = torch.zeros((1024, 1024, 24), dtype=torch.int32, device=dev)
    count, rows = 0, []
    with torch.no_grad():
        for w in wins:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            box = tuple(slice(a, b) for a, b in zip(w['lo'], w['hi']))
            out = net(image[(slice(None), slice(None)) + box].contiguous())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tt, cc, ss = instances._planes(out[0, 2:5], dev, 'measure')
            h = instances._Votes(tt, cc, ss).smooth(5)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            pk = instances.select_peaks(*instances.peak_candidates(h), tuple(tt.shape[1:]), 100)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            got = instances.paste_peaks(tt, cc, ss, out[0, 0] > 0.5, pk, w, labels, count + 1)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            count += len(got)
            rows.append((tuple(tt.shape[1:]), len(pk), len(got), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3,
                         (t4 - t3) * 1e3))
    return rows, labels


staged(False)                                            # warm-up: every window shape once
rows1, lab1 = staged(True)
rows2, lab2 = staged(True)
res['B_windows'] = [dict(shape=r[0], peaks=r[1], owned=r[2], forward=min(r[3], q[3]), votes_smooth=min(r[4], q[4]),
                         peaks_readback=min(r[5], q[5]), label_paste=min(r[6], q[6])) for r, q in zip(rows1, rows2)]
for key in ('forward', 'votes_smooth', 'peaks_readback', 'label_paste'):
    res['B_mean_' + key] = float(np.mean([r[key] for r in res['B_windows']]))
torch.cuda.synchronize()
t0 = time.perf_counter()
lab3, centres = segment.predict_instance_mask(net, image)
torch.cuda.synchronize()
res['B_predict_instance_mask_ms'] = (time.perf_counter() - t0) * 1e3
res['B_ids'] = int(len(centres))
res['B_same_labels_as_one_by_one'] = bool(torch.equal(lab3[0, 0], lab2))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps({k2: v2 for k2, v2 in res.items() if k2.startswith('B_') and k2 != 'B_windows'}, indent=1))
for r in res['B_windows']:
    print(r)
