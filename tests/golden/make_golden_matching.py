"""Writes tests/golden/conformer_matching.npz: the twelve yardstick cases of the conformer matching (tests/matching_ref.golden_case, seeds 100..111) with the
result of the optimiser the reference calls, scipy's differential_evolution with its defaults (utils/parsing.py:50-51: popsize 20, maxiter 20), on the fp64
restatement of the objective.  A couple of minutes on a CPU:  python tests/golden/make_golden_matching.py"""
import os
import sys

import numpy as np
from scipy.optimize import differential_evolution

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, '..'), os.path.join(HERE, '..', '..')]
import matching_ref as mr      # noqa: E402


def main():
    out = {}
    for seed in mr.GOLDEN_SEEDS:
        c = mr.golden_case(seed)
        f = lambda x: mr.objective(c['pos0'], c['target'], c['rot_bonds'], c['mask_rotate'], x)
        n_rot = len(c['rot_bonds'])
        res = differential_evolution(f, [(-np.pi, np.pi)] * n_rot, **mr.SCIPY_OPTIONS)
        rigid = f(np.zeros(n_rot))
        print(f'seed {seed}: n_lig {len(c["pos0"])}, n_rot {n_rot}, rigid {rigid:.4f}, scipy {res.fun:.4f} after {res.nit} generations, {res.nfev} evaluations')
        for k in ('pos0', 'target', 'rot_bonds', 'mask_rotate'):
            out[f'{k}_{seed}'] = c[k]
        out[f'rigid_{seed}'], out[f'x_{seed}'], out[f'fun_{seed}'] = np.float64(rigid), res.x.astype(np.float64), np.float64(res.fun)
    np.savez_compressed(os.path.join(HERE, 'conformer_matching.npz'), **out)


if __name__ == '__main__':
    main()
