#!/usr/bin/env python3
"""Write cosdg_sindg.txt: scipy.special.cosdg / sindg of the integer angles
0..359 as float64 hex, one `angle cos sin` line each.  random_rotate
(transforms.py) reads the table, so the package needs no scipy for the angles
the reference draws; numpy's cos(deg2rad(a)) is not a substitute (it differs
from cosdg in the last bit for most of these angles, which moves source
coordinates across .5 ties).

Usage:  python hcunet_amd/make_cosdg_sindg.py
"""
import os

from scipy import special

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    with open(os.path.join(HERE, 'cosdg_sindg.txt'), 'w') as f:
        f.write('# angle cosdg sindg (scipy.special, float64 hex); written by make_cosdg_sindg.py\n')
        for a in range(360):
            f.write('%d %s %s\n' % (a, float(special.cosdg(a)).hex(), float(special.sindg(a)).hex()))


if __name__ == '__main__':
    main()
