"""The fixture chains of tests/golden/rotate.npz, shared by the generator
(tests/golden/make_rotate_golden.py, which builds them from the REFERENCE's
classes) and the tests (which build them from hcat.transforms): random_rotate
(hcat/transforms.py:230-254) in the reference's validation chain
(tests/transforms_test.py:41-53), in the training recipe, and its corner cases.
All run on the 12x45x70 base stack of tests/golden/augment.npz, whose view
after reshape is 70x45x12.

`chain(T, name)` builds one chain from any namespace with the transform
classes, in the format of tests/augment_chains.py (raw, stack, joint, image);
the constructors run only then, because `affine`'s raises.
"""
try:
    from tests.augment_chains import apply, raws  # noqa: F401
except ImportError:   # the generator runs with tests/ itself on sys.path
    from augment_chains import apply, raws  # noqa: F401

DEVICE = ['val', 'drawn', 'recipe', 'fill_order', 'ties']
HOST = ['host_before_reshape', 'host_before_to_float', 'host_twice']
SEEDS = {'val': 41, 'drawn': 42, 'recipe': 43, 'fill_order': 44, 'ties': 45, 'host_before_reshape': 46,
         'host_before_to_float': 47, 'host_twice': 48, 'affine': 49}


def chain(T, name):
    g = T.__getitem__ if isinstance(T, dict) else (lambda n: getattr(T, n))
    to_float, reshape, normalize = g('to_float'), g('reshape'), g('normalize')
    random_crop, nul_crop, random_intensity = g('random_crop'), g('nul_crop'), g('random_intensity')
    drop_channel, clean_image, random_rotate = g('drop_channel'), g('clean_image'), g('random_rotate')
    build = {
        # the reference's validation chain on a non-square window; the cut corners become (0 - .5) / .5 = -1
        'val': lambda: dict(raw='base', stack=True,
                            joint=[to_float(), reshape(), random_crop([37, 33, 9]), random_rotate(90)],
                            image=[normalize()]),
        # a drawn angle (re-seed, then randint), and a crop AFTER the rotation: a window inside the rotated view
        'drawn': lambda: dict(raw='base', stack=True,
                              joint=[to_float(), reshape(), random_rotate(), random_crop([37, 33, 9])],
                              image=[normalize()]),
        # the training recipe with the rotation: keep lists before it, image, mask and pwl rotated together
        'recipe': lambda: dict(raw='base', stack=True,
                               joint=[to_float(), reshape(), nul_crop(1), random_crop([37, 33, 9]), random_rotate()],
                               image=[random_intensity((-15, 15)), drop_channel(.8), clean_image(),
                                      normalize([.5] * 4, [.5] * 4)]),
        # normalize BEFORE the rotation: outside voxels are 0 when random_intensity sees them, not (0 - m) / s
        'fill_order': lambda: dict(raw='base', stack=False, joint=[],
                                   image=[to_float(), reshape(), normalize([.4, .5, .6, .3], [.5] * 4),
                                          random_rotate(30), random_intensity((-15, 15))]),
        # 45 degrees on a square window: source coordinates at exact .5 along the diagonal
        'ties': lambda: dict(raw='base', stack=False, joint=[],
                             image=[to_float(), reshape(), random_crop([40, 40, 12]), random_rotate(45)]),
        # host cases
        'host_before_reshape': lambda: dict(raw='base', stack=False, joint=[],
                                            image=[to_float(), random_rotate(30), reshape(), normalize()]),
        'host_before_to_float': lambda: dict(raw='base', stack=False, joint=[],
                                             image=[random_rotate(30), to_float(), reshape(), normalize()]),
        'host_twice': lambda: dict(raw='base', stack=False, joint=[],
                                   image=[to_float(), reshape(), random_rotate(30), random_rotate(45), normalize()]),
        # the constructor raises
        'affine': lambda: dict(raw='base', stack=False, joint=[], image=[g('random_affine')()]),
    }
    return build[name]()
