#!/usr/bin/env python
"""Generate g24_render.npz by running the GENUINE reference's rotation (lib/visualization/utils.py) on CPU.

usage: make_golden_render.py <path of the reference checkout>      (needs matplotlib, which that module imports)

The reference is imported, never copied; only data is written: a (3, 3, 17) float64 random cloud, its rotate_np(., 25, 135, 0) -- the
rotation add_figures_reconstruction_tb applies before it draws -- and COLORS_PLT, the eight component colours."""
import os
import sys

import numpy as np

if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
import matplotlib                                   # noqa: E402
matplotlib.use('Agg')
from lib.visualization import utils as vis          # noqa: E402  (the reference)

rng = np.random.RandomState(2407)
cloud = rng.normal(0, 1, (3, 3, 17))
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'g24_render.npz')
np.savez(out, cloud=cloud, rotated=vis.rotate_np(cloud, 25, 135, 0), angles=np.array([25.0, 135.0, 0.0]),
         colors_plt=np.array(vis.COLORS_PLT, np.float64))
print('wrote', out, os.path.getsize(out), 'bytes')
