"""The fixture chains of tests/golden/augment.npz, shared by the generator
(tests/golden/make_augment_golden.py, which builds them from the REFERENCE's
classes) and the tests (which build them from hcat.transforms): the reference's
training recipe (tests/transforms_test.py:22-39) and its corner cases.

`chains(T)` takes any namespace with the transform classes.  A chain is
  raw     which raw inputs it runs on (keys of the fixture file)
  stack   True: Stack.__getitem__'s pattern (hcat/dataloader.py:79-90) on
          [image, mask, pwl]; False: the image alone
  joint   transforms applied to the list, then
  image   transforms applied to the image; to_tensor follows on everything.
"""
import numpy as np


def chains(T):
    g = T.__getitem__ if isinstance(T, dict) else (lambda n: getattr(T, n))
    to_float, reshape, normalize = g('to_float'), g('reshape'), g('normalize')
    random_crop, nul_crop, random_intensity = g('random_crop'), g('nul_crop'), g('random_intensity')
    drop_channel, clean_image, remove_channel = g('drop_channel'), g('clean_image'), g('remove_channel')
    return {
        # a real window in all three axes
        'crop': dict(raw='base', stack=True, joint=[to_float(), reshape(), random_crop([37, 33, 9])],
                     image=[normalize()]),
        # the training recipe: non-contiguous keep lists, (47,29,12) after nul_crop, then the
        # crop's quirks (x widened to the whole axis :361-362, y shrunk :370-373) -> (47,29,9)
        'recipe': dict(raw='base', stack=True,
                       joint=[to_float(), reshape(), nul_crop(1), random_crop([37, 33, 9])],
                       image=[random_intensity((-15, 15)), drop_channel(.8), clean_image(),
                              normalize([.5] * 4, [.5] * 4)]),
        # step order: normalize BEFORE random_intensity
        'order': dict(raw='base', stack=False, joint=[],
                      image=[to_float(), reshape(), random_crop([37, 33, 9]), normalize([.4, .5, .6, .3], [.5] * 4),
                             random_intensity((-15, 15)), clean_image()]),
        # a float64 image with NaN and +-Inf: the host path
        'order_f64': dict(raw='f64', stack=False, joint=[],
                          image=[to_float(), reshape(), random_intensity((-15, 15)), clean_image(),
                                 normalize([.5] * 4, [.5] * 4)]),
        'remove': dict(raw='q30', stack=False, joint=[],
                       image=[to_float(), reshape(), remove_channel((0, 2, 3)), normalize([.5] * 3, [.25] * 3)]),
        # nul_crop's rate = 0 branch: one draw, nothing dropped
        'nul_rate0': dict(raw='base', stack=True,
                          joint=[to_float(), reshape(), nul_crop(0), random_crop([37, 33, 9])], image=[]),
        'quirk_x_whole': dict(raw='q47', stack=False, joint=[],
                              image=[to_float(), reshape(), random_crop([37, 33, 9])]),      # (47,29,12) -> (47,29,9)
        'quirk_short_z': dict(raw='q30', stack=False, joint=[],
                              image=[to_float(), reshape(), random_crop([20, 20, 30])]),     # (30,25,12) -> (20,20,12)
        'quirk_too_small': dict(raw='q30', stack=False, joint=[],
                                image=[to_float(), reshape(), random_crop([50, 50, 5])]),    # IndexError
    }


def raws(G, key):
    """[image, mask, pwl] (mask / pwl None for an image-only input) of raw input `key`."""
    if key == 'base':
        return [G['base.image'], G['base.mask'], G['base.pwl']]
    if key == 'q47':   # corners of the base image: [12,29,47,4] and [12,25,30,4]
        return [np.ascontiguousarray(G['base.image'][:, :29, :47]), None, None]
    if key == 'q30':
        return [np.ascontiguousarray(G['base.image'][:, :25, :30]), None, None]
    return [G[key + '.image'], None, None]


def apply(chain, image, mask, pwl):
    """The chain up to (not including) to_tensor: [image, mask, pwl] or [image]."""
    image = image.copy()
    if chain['stack']:
        mask = np.expand_dims(mask.copy(), axis=mask.ndim)   # hcat/dataloader.py:80-81
        pwl = np.expand_dims(pwl.copy(), axis=pwl.ndim)
        for jt in chain['joint']:
            image, mask, pwl = jt([image, mask, pwl])
    for it in chain['image']:
        image = it(image)
    return [image, mask, pwl] if chain['stack'] else [image]
