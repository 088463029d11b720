"""Conformer matching, the parts a CPU can check (include/ddk.h: ddk_conformer_rmsd, ddk_conformer_match): the declared symbols and the host workspace query,
the fp64 restatement of the objective against the rule of utils/torsion.py on a hand case, the yardstick fixture (scipy's differential_evolution, the
optimiser the reference calls) against the restated search, and the integer index draws."""
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import matching_ref as mr
import philox_ref as pr
from disco_diffdock_amd import _lib, runtime

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
NAMES = ('ddk_conformer_match_workspace', 'ddk_conformer_rmsd', 'ddk_conformer_match')


def test_declarations_match_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    L = _lib.lib()
    for name, n_args in zip(NAMES, (4, 13, 15)):
        assert name in _lib.SYMBOLS
        m = re.search(r'(?:int|int64_t) %s\((.*?)\);' % name, hdr, re.S)
        assert m, name
        args = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
        assert len(getattr(L, name).argtypes) == len(args.split(',')) == n_args
    assert L.ddk_conformer_match_workspace.restype is _lib.C.c_int64
    assert L.ddk_conformer_rmsd.restype is _lib.C.c_int and L.ddk_conformer_match.restype is _lib.C.c_int
    # the options struct is the header's, member for member
    body = re.search(r'typedef struct ddk_match_options \{(.*?)\} ddk_match_options;', hdr, re.S).group(1)
    names = [n.strip() for line in body.split(';') if line.strip() for n in line.strip().split(None, 1)[1].split(',')]
    assert names == [f[0] for f in _lib.ddk_match_options._fields_]
    assert runtime.RNG_MATCH_PURPOSES == dict(match_population=mr.PURPOSE_POPULATION, match_generation=mr.PURPOSE_GENERATION)
    assert not set(runtime.RNG_MATCH_PURPOSES.values()) & (set(runtime.RNG_PURPOSES.values()) | set(runtime.RNG_FORWARD_PURPOSES.values()))
    assert '#define DDK_RNG_LAYOUT 1' in hdr      # purposes 0-8 keep their streams: the layout number stays


def test_workspace_query_refuses_each_broken_limit():
    ws = _lib.lib().ddk_conformer_match_workspace
    assert ws(30, 7, 15, 1) > 0 and ws(3, 0, 1, 1) > 0 and ws(256, 128, 64, 16) > 0
    for bad in ((2, 7, 15, 1), (257, 7, 15, 1), (30, -1, 15, 1), (30, 129, 15, 1), (30, 7, 0, 1), (30, 7, 65, 1), (30, 7, 15, 0), (30, 7, 15, 17),
                (200, 129, 64, 1)):
        assert ws(*bad) == -1, bad
    # two populations of n_islands * NP vectors and their costs fit
    NP = mr.members(20, 8)
    assert ws(30, 8, 20, 4) >= 2 * 4 * NP * (8 + 1) * 4
    assert ws(30, 8, 20, 4) > ws(30, 8, 20, 1)


def test_objective_is_the_torsion_rule_on_a_hand_case():
    """one rotor, a quarter turn, coordinates that are small multiples of 0.5: atoms 2 and 3 turn about atom 1 around the axis pos[0] - pos[1] = -x.
    The issue asks for an exact check; this one departs from it by one ulp: scipy's fp64 matrix of a quarter turn has 2^-52 where the exact matrix has 0, so
    the comparison allows 2^-52 (times lever arms of at most 1) and is exact after rounding to 12 digits.  No tighter bar exists for this restatement."""
    pos0 = np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 1.0, 0], [2.5, 0, 0.5], [-0.5, 1.0, 0]], np.float64)      # (atom 4 stays: off the axis, so the turn is no rigid motion)
    rot_bonds, mask = np.array([[0, 1]]), np.array([[False, True, True, True, False]])
    got = mr.apply_torsions(pos0, rot_bonds, mask, [np.pi / 2])
    # a quarter turn around -x: (y, z) -> (z, -y)
    want = np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 0, -1.0], [2.5, 0.5, 0], [-0.5, 1.0, 0]], np.float64)
    # exact but for the one ulp of 1 by which the fp64 matrix of a quarter turn (1 - 2 sin^2(pi / 4)) misses 0, times coordinates of at most 1 from the pivot
    assert np.abs(got - want).max() <= 2.0 ** -52 and np.array_equal(np.round(got, 12), want)
    assert np.array_equal(mr.apply_torsions(pos0, rot_bonds, mask, [0.0]), pos0)
    # against itself the RMSD is 0; against the turned copy it is what is left after the best rigid fit, the same from both sides
    assert mr.objective(pos0, want, rot_bonds, mask, [np.pi / 2]) <= 1e-15
    a, b = mr.objective(pos0, want, rot_bonds, mask, [0.0]), mr.objective(want, pos0, rot_bonds, mask, [0.0])
    assert a > 0.1 and abs(a - b) <= 1e-15
    with pytest.raises(AssertionError):
        mr.apply_torsions(pos0, np.array([[1, 0]]), mask, [1.0])      # u inside the mask: the reference's assert
    # the batched restatement the GPU tests take their bar from is the same rule
    batch = mr.apply_torsions_batch(pos0, rot_bonds, mask, np.array([[np.pi / 2], [0.0]]))
    assert np.abs(batch[0] - want).max() <= 1e-6 and np.array_equal(batch[1], pos0)


def test_objective_is_invariant_under_a_rigid_motion_of_the_target():
    c = mr.golden_case(103)
    rng = np.random.default_rng(0)
    tor = rng.uniform(-np.pi, np.pi, size=len(c['rot_bonds']))
    target = np.asarray(c['target'], np.float64)
    moved = target @ Rotation.random(random_state=5).as_matrix().T + np.array([30.0, -20.0, 10.0])
    args = (c['rot_bonds'], c['mask_rotate'], tor)
    assert abs(mr.objective(c['pos0'], target, *args) - mr.objective(c['pos0'], moved, *args)) <= 1e-12
    mask = np.arange(len(target)) % 3 != 0
    assert abs(mr.objective(c['pos0'], target, *args, atom_mask=mask) - mr.objective(c['pos0'], moved, *args, atom_mask=mask)) <= 1e-12


def test_fixture_is_the_generator_and_scipy_improves_on_the_rigid_fit(golden):
    cases = mr.golden_cases(golden)
    assert len(cases) == 12
    for seed, g in zip(mr.GOLDEN_SEEDS, cases):
        assert float(g['fun']) <= float(g['rigid'])
        assert 0.2 < float(g['fun']) < 0.3 and 1.3 < float(g['rigid']) < 2.2      # the noise floor of 0.15 per coordinate; an unmatched conformer
        f = lambda x: mr.objective(g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate'], x)
        assert abs(f(g['x']) - float(g['fun'])) <= 1e-9 and abs(f(np.zeros(len(g['x']))) - float(g['rigid'])) <= 1e-9
    c = mr.golden_case(100)
    assert all(np.array_equal(c[k], cases[0][k]) for k in ('pos0', 'target', 'rot_bonds', 'mask_rotate'))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_restated_search_reaches_scipy_on_the_fixture(golden, seed):
    """the search of include/ddk.h (synchronous, wrapped, seeded, compass polish) with the reference's popsize 20 / maxiter 20: within 0.01 A of scipy's
    minimum on at least 11 of the 12 cases, never above the rigid fit"""
    miss = []
    for s, g in zip(mr.GOLDEN_SEEDS, mr.golden_cases(golden)):
        f = lambda x: mr.objective(g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate'], x)
        r = mr.search(f, len(g['x']), popsize=20, maxiter=20, polish_iters=128, seed=seed, stream=pr.fnv1a64(f'case{s}'))
        got = f(r['torsions'])
        print(f'seed {seed} case {s}: search {got:.4f}, scipy {float(g["fun"]):.4f}, rigid {float(g["rigid"]):.4f}, {r["generations"]} generations')
        assert got <= float(g['rigid']) + 1e-6
        if got > float(g['fun']) + 0.01:
            miss.append((s, got, float(g['fun'])))
    assert len(miss) <= 1, miss


@pytest.mark.parametrize('NP', [5, 6, 8192])
def test_index_draws(NP):
    n, n_rot = 1 << 16, 7
    i = np.arange(n) % NP
    w = pr.block(3, 4, np.arange(n), mr.PURPOSE_GENERATION, 1, 0)
    r1, r2, forced = mr.index_draws(w, i, NP, n_rot)
    assert ((r1 >= 0) & (r1 < NP) & (r2 >= 0) & (r2 < NP) & (forced >= 0) & (forced < n_rot)).all()
    assert (r1 != i).all() and (r2 != i).all() and (r1 != r2).all()
    # flat within 5 sigma: r1 over the NP - 1 others, r2 over the NP - 2 left (as offsets from i, which has no excluded slot), forced over the components
    for offsets, k in (((r1 - i) % NP - 1, NP - 1), (forced, n_rot)):
        cnt = np.bincount(offsets, minlength=k)
        p = 1.0 / k
        assert np.abs(cnt - n * p).max() <= 5 * np.sqrt(n * p * (1 - p)) + 1, (k, cnt.min(), cnt.max())
    if NP <= 6:      # r2 given (i, r1): uniform over what is left
        rank = np.array([sorted(set(range(NP)) - {a, b}).index(c) for a, b, c in zip(i[:4096], r1[:4096], r2[:4096])])
        cnt = np.bincount(rank, minlength=NP - 2)
        p = 1.0 / (NP - 2)
        assert np.abs(cnt - 4096 * p).max() <= 5 * np.sqrt(4096 * p * (1 - p))
    # the extremes of the 24-bit uniform stay in range
    ends = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4], np.uint64)
    for ii in (0, NP - 1):
        a, b, c = mr.index_draws(ends, np.array([ii, ii]), NP, n_rot)
        assert ((a >= 0) & (a < NP) & (b >= 0) & (b < NP) & (a != ii) & (b != ii) & (a != b) & (c < n_rot)).all()


def test_population_and_wrap():
    p0, p1 = mr.initial_population(7, 9, 0, 40, 6), mr.initial_population(7, 9, 1, 40, 6)
    assert not p0[0].any() and p1[0].any() and (np.abs(p0) <= np.float32(np.pi)).all()
    assert np.array_equal(mr.initial_population(7, 9, 1, 40, 6), p1) and not np.array_equal(mr.initial_population(8, 9, 1, 40, 6), p1)
    t = np.float32([0, 3.2, -3.2, 9.5, -9.5, np.pi, -np.pi, 6.5])
    w = mr.wrap(t)
    assert ((w >= -np.float32(np.pi)) & (w < np.float32(np.pi))).all()
    assert np.abs(np.exp(1j * w.astype(np.float64)) - np.exp(1j * t.astype(np.float64))).max() <= 2e-6
