"""CPU: the crop and augmentation transforms of the lazy input chain
(hcunet_amd/transforms.py) against the reference's own outputs
(tests/golden/augment.npz, tests/golden/make_augment_golden.py).  Each fixture
chain runs under the fixture's numpy seed; the recorded state, turned into fp16
by the host restatement `PendingVolume.to_ndarray()` and the oracle's
to_tensor, must equal the reference's bits, and the np.random.random() drawn
right after the chain must equal the reference's, which pins the number and the
order of the draws.  Also the job struct's ABI and the launcher's host-side
validation, which runs before anything is enqueued and needs no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hcat.transforms as ht
from hcunet_amd import _lib
from hcunet_amd import transforms as tr
from oracle import input_oracle as io
from tests import augment_chains as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'augment.npz'))
CHAINS = ['crop', 'recipe', 'order', 'order_f64', 'remove', 'nul_rate0', 'quirk_x_whole', 'quirk_short_z']


def host_bits(v):
    a = v.to_ndarray() if isinstance(v, tr.PendingVolume) else v
    return io.to_tensor(a).view(np.uint16)


def run_chain(name):
    """The pending volumes of fixture chain `name` under its seed."""
    chain = ac.chains(ht)[name]
    np.random.seed(int(GOLD[name + '.seed']))
    return ac.apply(chain, *ac.raws(GOLD, chain['raw']))


def test_drop_in_names_are_exported():
    from hcat.transforms import (clean_image, drop_channel, normalize, nul_crop, random_crop,  # noqa: F401
                                 random_gamma, random_intensity, remove_channel, reshape, spekle, to_float,
                                 to_tensor)


@pytest.mark.parametrize('name', CHAINS)
def test_chain_matches_reference_bits_and_draws(name):
    vols = run_chain(name)
    np.random.randint(0, 1e8, 1)   # to_tensor's joint seed (:78), drawn by the reference before its next draw
    nxt = np.random.random()
    for key, v in zip(('image', 'mask', 'pwl'), vols):
        np.testing.assert_array_equal(host_bits(v), GOLD[name + '.' + key], err_msg=key)
    assert nxt == float(GOLD[name + '.next'])


def test_chains_stay_lazy_on_integer_stacks():
    # nothing of the recipe falls back to the host: one window / keep list per axis and a 4-step program
    image, mask, pwl = run_chain('recipe')
    assert all(isinstance(v, tr.PendingVolume) and v.raw.dtype != np.float64 for v in (image, mask, pwl))
    assert image.shape == (47, 29, 9, 4) and mask.shape == (47, 29, 9, 1)
    assert [s.kind for s in image.steps] == [tr.INTENSITY, tr.DROP, tr.CLEAN, tr.NORMALIZE]
    assert isinstance(image.sel[2], np.ndarray) and np.any(np.diff(image.sel[2]) > 1)   # non-contiguous x keep list
    assert 66 not in image.sel[2] and 41 not in image.sel[1]                            # the isolated voxel's rows
    image = run_chain('order')[0]
    assert [s.kind for s in image.steps] == [tr.NORMALIZE, tr.INTENSITY, tr.CLEAN]


def test_crop_error_types_match_reference():
    assert str(GOLD['quirk_too_small.error']) == 'IndexError'
    with pytest.raises(IndexError):
        run_chain('quirk_too_small')
    with pytest.raises(ValueError):     # :350-351
        ht.random_crop([4, 4, 4])('not an image')
    with pytest.raises(ValueError):     # :472-473
        ht.nul_crop(1)(np.zeros((4, 4, 4, 1)))
    with pytest.raises(TypeError):      # :312-313
        ht.random_intensity()('not an image')
    raw = np.zeros((3, 4, 5, 2), dtype=np.uint16)
    with pytest.raises(TypeError):      # spekle / random_gamma want a float image (:171-172, :191-192)
        ht.spekle(.1)(raw)
    with pytest.raises(TypeError):
        ht.random_gamma()(raw)
    with pytest.raises(ValueError):     # :173-174
        ht.spekle(1.5)(ht.to_float()(raw))
    with pytest.raises(NotImplementedError):
        ht.normalize([.5] * 2, [.5] * 2)(ht.normalize([.5] * 2, [.5] * 2)(ht.to_float()(raw)))


def test_random_gamma_records_only_non_negative_programs():
    rng = np.random.default_rng(1)
    raw = rng.integers(0, 65536, (3, 4, 5, 2)).astype(np.uint16)
    v = ht.reshape()(ht.to_float()(raw.copy()))   # (joint transforms: one seed draw each)
    np.random.seed(3)
    v = ht.random_gamma((.7, 1.3))(v)
    np.random.seed(3)
    g = np.random.uniform(.7, 1.3, 1)
    assert [s.kind for s in v.steps] == [tr.GAMMA] and v.steps[0].a[0] == g[0]
    np.testing.assert_array_equal(v.to_ndarray(), (raw.astype(np.float64) / 2 ** 16).swapaxes(2, 0) ** g)
    # after normalize the values may be negative: the host path, which raises as adjust_gamma does
    n = ht.normalize([.5] * 2, [.5] * 2)(ht.to_float()(raw.copy()))
    with pytest.raises(ValueError):
        ht.random_gamma((.7, 1.3))(n)


def test_spekle_draws_one_key_on_the_device_path_and_numpy_normals_on_the_host():
    raw = np.full((3, 4, 5, 2), 32768, dtype=np.uint16)
    v = ht.to_float()(raw.copy())
    np.random.seed(9)
    v = ht.spekle(.05)(v)
    nxt = np.random.random()
    np.random.seed(9)
    key = int(np.random.randint(0, 2 ** 31 - 1))
    assert nxt == np.random.random()
    assert [s.kind for s in v.steps] == [tr.SPEKLE] and v.steps[0].key == key
    # a float64 image: the reference's own stream
    f = raw.astype(np.float64) / 2 ** 16
    np.random.seed(9)
    got = ht.spekle(.05)(f.copy()).to_ndarray()
    np.random.seed(9)
    want = f + np.float32(np.random.normal(0, .05, f.shape))
    np.testing.assert_array_equal(got, np.clip(want, 0, 1))


def test_a_ninth_step_moves_the_chain_to_the_host_in_order():
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 65536, (3, 4, 5, 2)).astype(np.uint16)
    v = ht.to_float()(raw.copy())
    want = raw.astype(np.float64) / 2 ** 16
    np.random.seed(4)
    for _ in range(10):
        v = ht.random_intensity((-15, 15))(v)
    np.random.seed(4)
    for _ in range(10):
        val = np.random.randint(-15, 15, 2) / 100
        for c in range(2):
            if np.random.random() > 0:
                want[..., c] -= val[c]
        want[want < 0] = 0
    assert len(v.steps) == 0 and v.raw.dtype == np.float64   # steps 1-8 recorded, then everything on the host
    np.testing.assert_array_equal(v.to_ndarray(), want)


def test_nul_crop_keep_lists_are_cached_per_stack_while_uncropped():
    from hcunet_amd.dataloader import _Raw
    src = _Raw(GOLD['base.mask'])
    lists = []
    for _ in range(2):
        vols = [tr.PendingVolume(GOLD['base.image'].copy()), src.pending(expand=True),
                tr.PendingVolume(GOLD['base.pwl'][..., None].copy())]
        vols = ht.reshape()(ht.to_float()(vols))
        np.random.seed(0)
        vols = ht.nul_crop(1)(vols)
        assert vols[0].shape == (47, 29, 12, 4) and vols[2].shape == (47, 29, 12, 1)
        lists.append(src.keep_lists[(True, True)])
    assert len(src.keep_lists) == 1 and lists[0][0] is lists[1][0]


# ---------------------------------------------------------------------------
# ABI and host validation
FIELDS = {
    'hcu_aug_step': (_lib.AugStep, ['kind', 'key', 'a', 'b']),
    'hcu_ingest_job': (_lib.IngestJob, ['src', 'dst', 'xmap_dev', 'ymap_dev', 'xmap_host', 'ymap_host', 'src_dtype',
                                        'Z', 'Y', 'X', 'C', 'ox', 'oy', 'oz', 'x0', 'y0', 'z0', 'n_chan', 'chan',
                                        'n_steps', 'scale', 'steps']),
}


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs a C compiler')
def test_job_structs_match_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hcunet.h"', 'int main(void) {']
    for name, (_, fields) in FIELDS.items():
        lines.append('printf("%s size %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines.append('printf("const max_c %d\\n", HCU_INGEST_MAX_C);')
    lines.append('printf("const max_steps %d\\n", HCU_AUG_MAX_STEPS);')
    lines.append('printf("const kinds %d\\n", HCU_AUG_NORMALIZE + 10 * (HCU_AUG_INTENSITY + 10 * (HCU_AUG_DROP + 10 * '
                 '(HCU_AUG_CLEAN + 10 * (HCU_AUG_GAMMA + 10 * HCU_AUG_SPEKLE)))));')
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
            got[(parts[0], parts[1])] = int(parts[2])
    for name, (cls, fields) in FIELDS.items():
        assert got[(name, 'size')] == ctypes.sizeof(cls), name
        for f in fields:
            assert got[(name, f)] == getattr(cls, f).offset, (name, f)
    assert got[('const', 'max_c')] == _lib.INGEST_MAX_C and got[('const', 'max_steps')] == _lib.AUG_MAX_STEPS
    assert got[('const', 'kinds')] == (_lib.AUG_NORMALIZE + 10 * (_lib.AUG_INTENSITY + 10 * (_lib.AUG_DROP + 10 * (
        _lib.AUG_CLEAN + 10 * (_lib.AUG_GAMMA + 10 * _lib.AUG_SPEKLE)))))


def _job(**kw):
    """A valid job on a [Z=8,Y=20,X=30,C=4] uint16 source (the pointers are
    never dereferenced: validation fails before anything is enqueued)."""
    j = _lib.IngestJob()
    j.src, j.dst = 0x1000, 0x2000
    j.src_dtype, j.Z, j.Y, j.X, j.C = _lib.HCU_U16, 8, 20, 30, 4
    j.ox, j.oy, j.oz = 10, 10, 4
    j.x0, j.y0, j.z0 = 20, 10, 4
    j.n_chan = 4
    for c in range(4):
        j.chan[c] = c
    j.scale = 2.0 ** -16
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _submit(job):
    return _lib.lib().hcu_ingest_jobs(ctypes.addressof(job), 0x3000, 1, None)


def test_host_validation_rejects_bad_jobs_before_any_launch():
    assert _submit(_job(x0=21)) == _lib.HCU_ERR_SHAPE           # x window past the source
    assert 'x window' in _lib.last_error()
    assert _submit(_job(y0=11)) == _lib.HCU_ERR_SHAPE
    assert _submit(_job(z0=5)) == _lib.HCU_ERR_SHAPE
    assert _submit(_job(z0=-1)) == _lib.HCU_ERR_SHAPE
    xmap = np.arange(20, 30, dtype=np.int32)
    xmap[7] = 30                                                # a map entry equal to X
    assert _submit(_job(xmap_dev=0x4000, xmap_host=xmap.ctypes.data)) == _lib.HCU_ERR_SHAPE
    ymap = np.arange(10, dtype=np.int32)
    ymap[0] = -1
    assert _submit(_job(ymap_dev=0x4000, ymap_host=ymap.ctypes.data)) == _lib.HCU_ERR_SHAPE
    assert _submit(_job(xmap_dev=0x4000)) == _lib.HCU_ERR_INVALID   # a device map without its host copy
    assert _submit(_job(oz=0)) == _lib.HCU_ERR_SHAPE            # empty extent
    assert _submit(_job(C=17)) == _lib.HCU_ERR_UNSUPPORTED      # 17 channels
    assert '16 channels' in _lib.last_error()
    assert _submit(_job(n_chan=17)) == _lib.HCU_ERR_UNSUPPORTED
    assert _submit(_job(n_steps=9)) == _lib.HCU_ERR_UNSUPPORTED     # 9 steps
    assert '8 steps' in _lib.last_error()
    assert _submit(_job(src_dtype=_lib.HCU_F64)) == _lib.HCU_ERR_INVALID
    assert _submit(_job(src=None)) == _lib.HCU_ERR_INVALID
    bad_chan = _job()
    bad_chan.chan[2] = 4
    assert _submit(bad_chan) == _lib.HCU_ERR_INVALID
    bad_step = _job(n_steps=1)
    bad_step.steps[0].kind = 7
    assert _submit(bad_step) == _lib.HCU_ERR_INVALID
    assert _submit(_job(Z=4096, Y=4096, X=64, z0=0)) == _lib.HCU_ERR_UNSUPPORTED   # 2^31 source bytes
    assert _lib.lib().hcu_ingest_jobs(None, 0x3000, 1, None) == _lib.HCU_ERR_INVALID
    assert _lib.lib().hcu_ingest_jobs(ctypes.addressof(_job()), 0x3000, 0, None) == _lib.HCU_ERR_SHAPE
