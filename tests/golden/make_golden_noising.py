"""Records tests/golden/noising.npz from the reference's own utils/so3.py and utils/torus.py, unmodified:

    cd <an empty scratch directory> && python <repo>/tests/golden/make_golden_noising.py <reference checkout> <repo>/tests/golden/noising.npz

The two modules build their tables on first import (minutes of NumPy, about 430 MB of .npy caches in the working directory, hence the scratch
directory).  What is kept, under 150 KB:
  so3_rows [3] and so3_cdf / so3_score_norms [3, 2000]   _cdf_vals and _score_norms at rows 0, 500, 999
  so3_vec_eps [32], so3_vec [32, 3], so3_vec_score [32, 3]   so3.score_vec at 32 fixed (eps, vec) pairs inside the support of their row
  torus_x, torus_sigma, torus_score [256]                 torus.score at 256 fixed (x, sigma) pairs, the NaN corner (x index 5000 at sigma index 0) included
"""
import os
import sys

import numpy as np

SO3_ROWS = (0, 500, 999)


def fixed_points():
    rng = np.random.RandomState(20240611)
    eps = 10 ** rng.uniform(np.log10(0.01), np.log10(2), 32)
    eps[:2] = (0.01, 2.0)
    vec = eps[:, None] * rng.randn(32, 3)
    norm = np.linalg.norm(vec, axis=1)
    vec *= np.where(norm > 3.0, 3.0 / norm, 1.0)[:, None]
    sigma = 10 ** rng.uniform(np.log10(3e-3), np.log10(2), 256) * np.pi
    x = sigma * rng.randn(256) * rng.choice([0.1, 1.0, 3.0], 256)
    # the corners: the NaN corner (|x| = pi at the smallest sigma), x = 0, the first grid point, beyond the wrap, sigmas outside the table
    x[:8] = (-np.pi, np.pi, 0.0, 1e-5 * np.pi, 1e-7, 7.0, -7.0, 3.0)
    sigma[:8] = (3e-3 * np.pi, 3e-3 * np.pi, 1.0, 2 * np.pi, 1e-3, 9.0, 0.5, 3e-3 * np.pi)
    return eps, vec, x, sigma


def main(reference, out):
    sys.path.insert(0, os.path.abspath(reference))
    from utils import so3, torus
    eps, vec, x, sigma = fixed_points()
    rows = np.array(SO3_ROWS)
    with np.errstate(all='ignore'):
        vec_score = np.stack([so3.score_vec(eps=e, vec=v) for e, v in zip(eps, vec)])
        t_score = torus.score(x, sigma)
    assert np.isnan(t_score[:2]).all(), 'the NaN corner is expected to be NaN'
    np.savez_compressed(out, so3_rows=rows, so3_cdf=so3._cdf_vals[rows], so3_score_norms=so3._score_norms[rows], so3_vec_eps=eps, so3_vec=vec,
                        so3_vec_score=vec_score, torus_x=x, torus_sigma=sigma, torus_score=t_score)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
