"""CPU: random_rotate of the lazy input chain (hcunet_amd/transforms.py)
against the reference's own outputs (tests/golden/rotate.npz,
tests/golden/make_rotate_golden.py).  Each fixture chain runs under its numpy
seed; the recorded state, restated on the host by `PendingVolume.to_ndarray()`
and rounded as the reference's to_tensor rounds, must equal the reference's
bits, and the np.random.random() drawn right after the chain must equal the
reference's.  Also the numpy restatement against scipy.ndimage.rotate itself
(exact: no tolerance), the committed sine / cosine table, the job record's new
fields and the launcher's host-side validation of them, which runs before
anything is enqueued and needs no device."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import hcat.transforms as ht
from hcunet_amd import _lib
from hcunet_amd import transforms as tr
from tests import rotate_chains as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'rotate.npz'))
BASE = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'augment.npz'))


def host_bits(v):
    """The reference's to_tensor (:133-136) on the host restatement: fp16 bits of [1,C,X,Y,Z]."""
    a = v.to_ndarray() if isinstance(v, tr.PendingVolume) else v
    h = torch.as_tensor(a, dtype=torch.half)
    return h.permute(3, 0, 1, 2)[None].contiguous().view(torch.int16).numpy().view(np.uint16)


def run_chain(name):
    """The pending volumes of fixture chain `name` under its seed."""
    np.random.seed(int(GOLD[name + '.seed']))
    chain = rc.chain(ht, name)
    return rc.apply(chain, *rc.raws(BASE, chain['raw']))


def test_drop_in_names_are_exported():
    from hcat.transforms import random_affine, random_rotate  # noqa: F401
    assert ht.random_rotate().angle is None and ht.random_rotate(90).angle == 90


@pytest.mark.parametrize('name', rc.DEVICE + rc.HOST)
def test_chain_matches_reference_bits_and_draws(name):
    vols = run_chain(name)
    np.random.randint(0, 1e8, 1)   # to_tensor's joint seed (:78), drawn by the reference before its next draw
    nxt = np.random.random()
    for key, v in zip(('image', 'mask', 'pwl'), vols):
        np.testing.assert_array_equal(host_bits(v), GOLD[name + '.' + key], err_msg=key)
    assert nxt == float(GOLD[name + '.next'])


def test_random_affine_fails_as_the_reference():
    assert str(GOLD['affine.error']) == 'TypeError'   # `raise NotImplemented(...)`: the constant is not callable
    with pytest.raises(TypeError):
        run_chain('affine')


def test_device_chains_stay_lazy_and_host_chains_leave():
    for name in rc.DEVICE:
        for v in run_chain(name):
            assert isinstance(v, tr.PendingVolume) and v.rot is not None and tr._is_job(v), name
    image, mask, pwl = run_chain('val')
    R = image.rot
    assert (R.c, R.s) == (0.0, 1.0) and (R.nx, R.ny, R.after) == (37, 33, 0) and len(image.steps) == 1
    assert (R.px, R.py, R.ox, R.oy) == (0, 0, 37, 33) and image.shape == (37, 33, 9, 4)
    image, mask, pwl = run_chain('drawn')    # the crop after the rotation moved a window inside the rotated view
    R = image.rot
    assert (R.nx, R.ny, R.ox, R.oy) == (70, 45, 37, 33) and image.sel[1] is None and image.sel[2] is None
    assert (mask.rot.c, mask.rot.s, mask.rot.px, mask.rot.py) == (R.c, R.s, R.px, R.py) == \
        (pwl.rot.c, pwl.rot.s, pwl.rot.px, pwl.rot.py)
    assert image.sel[0][1] == 9 and image.shape == (37, 33, 9, 4)
    image, mask, pwl = run_chain('recipe')   # keep lists from before the rotation index the pre-rotation view
    assert isinstance(image.sel[2], np.ndarray) and len(image.sel[2]) == image.rot.nx == 47
    assert isinstance(image.sel[1], np.ndarray) and len(image.sel[1]) == image.rot.ny == 29
    kinds = [s.kind for s in image.steps if s.kind != tr.DROP]   # (drop_channel records a step only when it drops)
    assert image.rot.after == 0 and kinds == [tr.INTENSITY, tr.CLEAN, tr.NORMALIZE]
    image = run_chain('fill_order')[0]
    assert image.rot.after == 1 and [s.kind for s in image.steps] == [tr.NORMALIZE, tr.INTENSITY]
    for name in rc.HOST:
        v = run_chain(name)[0]
        assert v.rot is None and v.raw.dtype == np.float64, name


def test_nul_crop_after_a_rotation_takes_the_host_path():
    image, mask, pwl = (BASE['base.image'].copy(), BASE['base.mask'][..., None].copy(),
                        BASE['base.pwl'][..., None].copy())
    np.random.seed(3)
    vols = ht.random_rotate(30)(ht.reshape()(ht.to_float()([image, mask, pwl])))
    assert all(v.rot is not None for v in vols)
    want = [v.to_ndarray() for v in vols]
    out = ht.nul_crop(1)(vols)
    lr = want[1].sum(axis=(1, 2, 3)) > 1
    ud = want[1][lr].sum(axis=(0, 2, 3)) > 1
    for v, w in zip(out, want):
        assert v.rot is None and v.raw.dtype == np.float64
        np.testing.assert_array_equal(v.to_ndarray(), w[lr][:, ud])


def test_rng_use_and_input_types():
    raw = BASE['base.image'][:3, :9, :11].copy()
    with pytest.raises(TypeError):              # :243-244
        ht.random_rotate(30)('not an image')
    for angle in (None, 0):                     # `if not self.angle`: 0 draws too
        np.random.seed(8)
        v = ht.random_rotate(angle)(ht.reshape()(ht.to_float()(raw.copy())))
        nxt = np.random.random()
        np.random.seed(8)
        np.random.randint(0, 1e8, 1), np.random.randint(0, 1e8, 1)   # to_float's and reshape's joint seeds
        seed = np.random.randint(0, 1e8, 1)
        np.random.seed(seed)
        theta = np.random.randint(0, 360, 1)[0]
        assert nxt == np.random.random()
        assert (v.rot.c, v.rot.s) == tr.cos_sin(theta)
    np.random.seed(8)                           # a given angle draws the joint seed only and does not re-seed
    v = ht.random_rotate(30)(ht.reshape()(ht.to_float()(raw.copy())))
    nxt = np.random.random()
    np.random.seed(8)
    for _ in range(3):
        np.random.randint(0, 1e8, 1)
    assert nxt == np.random.random()


# ---------------------------------------------------------------------------
# the restatement against scipy itself
ANGLES = sorted(set(range(0, 360, 7)) | {1, 30, 45, 60, 90, 135, 180, 270, 359})


@pytest.mark.parametrize('shape', [(7, 5), (33, 17), (40, 40), (64, 48), (128, 96)])
def test_restatement_equals_scipy_exactly(shape):
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(shape[0])
    a = rng.integers(1, 65536, size=shape + (2, 1)).astype(np.float64) / 2 ** 16   # no zeros: outside is told apart
    differing = 0
    for angle in ANGLES:
        want = ndimage.rotate(a, axes=(0, 1), angle=angle, reshape=False, order=0, mode='constant', prefilter=False)
        got = tr.rotate_nearest(a, *tr.cos_sin(angle))
        differing += int((got != want).sum())
    assert differing == 0


def test_committed_table_equals_scipy_special():
    special = pytest.importorskip('scipy.special')
    for a in range(360):
        assert tr.cos_sin(a) == (float(special.cosdg(a)), float(special.sindg(a))), a
        assert tr.cos_sin(np.int64(a)) == tr.cos_sin(float(a)) == tr.cos_sin(a)
    assert tr.cos_sin(12.5) == (float(special.cosdg(12.5)), float(special.sindg(12.5)))   # not in the table
    assert tr.cos_sin(360) == (float(special.cosdg(360)), float(special.sindg(360)))


def test_a_non_integer_angle_without_scipy_names_scipy(monkeypatch):
    monkeypatch.setitem(sys.modules, 'scipy', None)   # `from scipy import special` raises ImportError
    assert tr.cos_sin(45) == tr.cos_sin(45.0)          # the table needs no scipy
    with pytest.raises(ImportError, match='scipy'):
        tr.cos_sin(12.5)


def test_package_does_not_import_scipy_ndimage():
    code = ('import sys, numpy as np; import hcat.transforms as ht; '
            'v = ht.random_rotate(45)(ht.reshape()(ht.to_float()(np.ones((2, 5, 6, 1), np.uint8)))); '
            'v.to_ndarray(); assert not any(m.startswith("scipy") for m in sys.modules), sorted(sys.modules)')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=ROOT, capture_output=True)


# ---------------------------------------------------------------------------
# ABI and host validation
NEW_FIELDS = ['rot', 'rot_m', 'rot_off', 'rot_nx', 'rot_ny', 'rot_px', 'rot_py', 'fill_after']


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs a C compiler')
def test_new_job_fields_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hcunet.h"', 'int main(void) {',
             'hcu_ingest_job j;', 'printf("size %zu %zu\\n", sizeof(hcu_ingest_job), (size_t)0);']
    for f in ['steps'] + NEW_FIELDS:
        lines.append('printf("%s %%zu %%zu\\n", offsetof(hcu_ingest_job, %s), sizeof(j.%s));' % (f, f, f))
    lines += ['return 0;', '}']
    src = tmp_path / 'abi.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'abi'
    subprocess.run(['gcc', '-std=c11', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n'):
        parts = ln.split()
        if len(parts) == 3:
            got[parts[0]] = (int(parts[1]), int(parts[2]))
    assert got['size'][0] == ctypes.sizeof(_lib.IngestJob)
    for f in NEW_FIELDS:
        assert got[f] == (getattr(_lib.IngestJob, f).offset, getattr(_lib.IngestJob, f).size), f
    # appended: every new field lies behind the last old one
    assert min(got[f][0] for f in NEW_FIELDS) >= got['steps'][0] + got['steps'][1]


def _job(**kw):
    """A valid rotated job on a [Z=8,Y=20,X=30,C=4] uint16 source: the
    pre-rotation view is the 12x10 window at (18, 10), rotated by 30 degrees,
    the output the 10x8 window at (1, 2) of the rotated view (the pointers are
    never dereferenced: validation fails before anything is enqueued)."""
    j = _lib.IngestJob()
    j.src, j.dst = 0x1000, 0x2000
    j.src_dtype, j.Z, j.Y, j.X, j.C = _lib.HCU_U16, 8, 20, 30, 4
    j.ox, j.oy, j.oz = 10, 8, 4
    j.x0, j.y0, j.z0 = 18, 10, 4
    j.n_chan = 4
    for c in range(4):
        j.chan[c] = c
    j.scale = 2.0 ** -16
    j.n_steps = 2
    j.steps[0].kind = j.steps[1].kind = _lib.AUG_CLEAN
    c, s = tr.cos_sin(30)
    m, off = tr.rotation_terms(c, s, 12, 10)
    j.rot, j.fill_after = 1, 1
    j.rot_m[:] = list(m.reshape(-1))
    j.rot_off[:] = list(off)
    j.rot_nx, j.rot_ny, j.rot_px, j.rot_py = 12, 10, 1, 2
    return _set(j, kw)


def _set(j, kw):
    for k, v in kw.items():
        if isinstance(v, tuple):     # (index, value) of an array field
            getattr(j, k)[v[0]] = v[1]
        else:
            setattr(j, k, v)
    return j


def _unrotated(**kw):
    """The same source with the plain 10x8 window at (18, 10) and every new field 0."""
    j = _job()
    j.rot = j.fill_after = j.rot_nx = j.rot_ny = j.rot_px = j.rot_py = 0
    j.rot_m[:] = [0.0] * 4
    j.rot_off[:] = [0.0] * 2
    return _set(j, kw)


def _submit(job):
    return _lib.lib().hcu_ingest_jobs(ctypes.addressof(job), 0x3000, 1, None)


def _passes_validation(job):
    """True when `job` gets through aug_validate.  Nothing may be launched on
    fake pointers, so the job is made wide -- 2^30 one-byte voxels along x,
    2^25 tiles -- and submitted 66 times in one table: the launcher validates
    every job and then refuses the table for its more than 2^31 tiles
    (HCU_ERR_UNSUPPORTED, 'too many tiles') before anything is enqueued."""
    job.src_dtype, job.Z, job.Y, job.X, job.C = _lib.HCU_U8, 1, 1, 2 ** 30, 1
    job.ox, job.oy, job.oz, job.x0, job.y0, job.z0, job.n_chan = 2 ** 30, 1, 1, 0, 0, 0, 1
    if job.rot:
        job.rot_nx, job.rot_ny, job.rot_px, job.rot_py = 2 ** 30, 1, 0, 0
    table = (_lib.IngestJob * 66)(*[job] * 66)
    rc_ = _lib.lib().hcu_ingest_jobs(ctypes.addressof(table), 0x3000, 66, None)
    if rc_ == _lib.HCU_ERR_UNSUPPORTED and 'too many tiles' in _lib.last_error():
        return True
    assert 'job 0' in _lib.last_error()
    return False


def test_host_validation_of_the_rotation_fields():
    L, INV, SHP = _lib.last_error, _lib.HCU_ERR_INVALID, _lib.HCU_ERR_SHAPE
    assert _submit(_job(rot=2)) == INV and 'rot must be 0 or 1' in L()
    assert _submit(_job(rot=-1)) == INV
    for i in range(4):
        assert _submit(_job(rot_m=(i, float('nan')))) == INV and 'matrix' in L()
        assert _submit(_job(rot_m=(i, float('inf')))) == INV
        assert _submit(_job(rot_m=(i, -1.0000001))) == INV
    for i in range(2):
        assert _submit(_job(rot_off=(i, float('nan')))) == INV and 'offset' in L()
        assert _submit(_job(rot_off=(i, float('-inf')))) == INV
    assert _submit(_job(rot_nx=0)) == SHP and 'pre-rotation' in L()
    assert _submit(_job(rot_ny=-3)) == SHP
    assert _submit(_job(rot_px=-1)) == SHP and 'rotated view' in L()
    assert _submit(_job(rot_px=3)) == SHP       # 3 + 10 > 12
    assert _submit(_job(rot_py=-1)) == SHP
    assert _submit(_job(rot_py=3)) == SHP       # 3 + 8 > 10
    assert _submit(_job(ox=12)) == SHP          # 1 + 12 > 12
    # the raw window is bounded by the pre-rotation extents, not by the output's
    assert _submit(_job(x0=19)) == SHP and 'x window' in L()    # 19 + 12 > 30 although 19 + 10 <= 30
    assert _submit(_job(y0=11)) == SHP and 'y window' in L()    # 11 + 10 > 20 although 11 + 8 <= 20
    xmap = np.arange(18, 30, dtype=np.int32)    # rot_nx = 12 entries; the last one is beyond the output's 10
    xmap[11] = 30
    assert _submit(_job(xmap_dev=0x4000, xmap_host=xmap.ctypes.data)) == SHP and 'x window or map' in L()
    ymap = np.arange(10, 20, dtype=np.int32)    # rot_ny = 10 entries
    ymap[9] = -1
    assert _submit(_job(ymap_dev=0x4000, ymap_host=ymap.ctypes.data)) == SHP and 'y window or map' in L()
    assert _submit(_job(fill_after=-1)) == INV and 'fill_after' in L()
    assert _submit(_job(fill_after=3)) == INV   # n_steps = 2
    # without rot every new field must be 0
    for kw in (dict(rot_m=(0, 1.0)), dict(rot_m=(3, float('nan'))), dict(rot_off=(1, .5)), dict(rot_nx=12),
               dict(rot_ny=10), dict(rot_px=1), dict(rot_py=1), dict(fill_after=1)):
        assert _submit(_unrotated(**kw)) == INV and 'without rot' in L(), kw
    # a step kind is not how a rotation is recorded: kind 7 stays invalid
    bad = _job()
    bad.steps[1].kind = 7
    assert _submit(bad) == INV and 'unknown step kind' in L()


def test_valid_jobs_pass_validation_up_to_the_launch():
    # a zeroed record with valid old fields means "no rotation" ...
    j = _lib.IngestJob()
    j.src, j.dst, j.scale = 0x1000, 0x2000, 1.0
    assert all(getattr(j, f) == 0 for f in NEW_FIELDS if isinstance(getattr(j, f), int))
    assert not any(j.rot_m) and not any(j.rot_off)
    assert _passes_validation(j)
    # ... a valid rotated job passes too, fill_after = 0 and = n_steps included ...
    for fill in (0, 1, 2):
        assert _passes_validation(_job(fill_after=fill))
    assert _passes_validation(_unrotated())
    # ... and the same wide job is refused for a rotation field, not for its size
    assert not _passes_validation(_job(rot=2))
    j = _lib.IngestJob()
    j.src, j.dst, j.scale, j.rot_px = 0x1000, 0x2000, 1.0, 1
    assert not _passes_validation(j)
