"""CPU checks of the forward-diffusion restatement tests/noising_ref.py, the yardstick of tests/test_gpu_noising.py, against values recorded from the
reference's own utils/so3.py and utils/torus.py (tests/golden/noising.npz, written by tests/golden/make_golden_noising.py) and against the shipped
so3_exp_score_norms.npy; plus the Python-side contracts of the feature (index helpers, purposes, declared symbols)."""
import os
import re

import numpy as np
import pytest

import noising_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'noising.npz')
SHIPPED = os.path.join(ROOT, 'disco_diffdock_amd', 'data', 'so3_exp_score_norms.npy')
NEW_CALLS = ('ddk_so3_rows', 'ddk_torus_score', 'ddk_rng_perturbation', 'ddk_score_matching_loss')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def rows():
    return {i: nr.so3_row(i) for i in (0, 1, 130, 500, 868, 999)}


def test_so3_rows_equal_the_reference(golden, rows):
    """rows 0, 500, 999: the CDF bit for bit or within 1e-15; the scores wherever pdf >= 1e-6 max(pdf), a contiguous set with >= 99.999 % of sum |pdf|"""
    for k, i in enumerate(golden['so3_rows']):
        r = rows[int(i)]
        d_cdf = float(np.abs(r['cdf'] - golden['so3_cdf'][k]).max())
        live, contiguous, share = nr.live_set(r['pdf'])
        ref = golden['so3_score_norms'][k][live]
        d_score = float((np.abs(r['score'][live] - ref) / np.abs(ref)).max())
        print(f'row {i}: cdf max abs diff {d_cdf:.3e}, score max rel diff {d_score:.3e} on {int(live.sum())} entries holding {share:.9f} of the mass')
        assert d_cdf <= 1e-15
        assert contiguous and share >= 0.99999
        assert np.isfinite(ref).all() and d_score <= 1e-12


def test_ascending_exp_score_norm_is_the_shipped_table_bit_for_bit(rows):
    shipped = np.load(SHIPPED)
    assert shipped.shape == (nr.N_EPS,) and np.isfinite(shipped).all()
    for i, r in rows.items():
        assert r['exp_score_norm'] == shipped[i], (i, r['exp_score_norm'], shipped[i])
        # the rule of ddk_so3_rows (finite scores above the rounding noise of their expansion only) moves it by at most 1e-9
        assert abs(r['exp_score_norm_finite'] - shipped[i]) <= 1e-9 * shipped[i], i
        assert abs(r['exp_score_norm_guarded'] - shipped[i]) <= 1e-9 * shipped[i], i


def test_score_vec_points(golden):
    for eps, vec, want in zip(golden['so3_vec_eps'], golden['so3_vec'], golden['so3_vec_score']):
        got = nr.so3_score_vec(eps, vec)
        assert np.isfinite(want).all()
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (eps, vec, got, want)


def test_torus_score_points(golden):
    x, sigma, want = golden['torus_x'], golden['torus_sigma'], golden['torus_score']
    got = nr.torus_score(x, nr.torus_sigma_index(sigma))
    nan = np.isnan(want)
    assert nan[:2].all() and np.array_equal(np.isnan(got), nan)      # the NaN corner, and NaN exactly where the table has it
    assert np.abs(got[~nan] - want[~nan]).max() <= 1e-12 + 1e-12 * np.abs(want[~nan]).max()
    assert got[x == 0].size and (got[x == 0] == 0).all()


def test_interp_is_numpy_interp_on_a_monotone_row(rows):
    r = rows[500]
    live, _, _ = nr.live_set(r['pdf'], 1e-9)
    j = np.flatnonzero(live)
    cdf, om = r['cdf'][j[0]:j[-1] + 1], nr.omegas[j[0]:j[-1] + 1]
    assert (np.diff(cdf) > 0).all()
    for u in np.concatenate([np.linspace(0, cdf[-1] * 1.01, 97), cdf[::37]]):
        assert abs(nr.interp(u, cdf, om) - np.interp(u, cdf, om)) <= 4e-16 * np.pi


def test_index_helpers():
    from disco_diffdock_amd import training
    eps = np.concatenate([10 ** np.linspace(-2.5, 0.5, 301), nr.eps_array[::50]])
    assert np.array_equal(training.so3_eps_index(eps), nr.so3_eps_index(eps))
    assert int(training.so3_eps_index(0.01)) == 0 and int(training.so3_eps_index(2.0)) == nr.N_EPS - 1 and int(training.so3_eps_index(50.0)) == nr.N_EPS - 1
    # the reference's quirk: the index is scaled by N_EPS, so eps_array[i] does not map to i in the upper rows
    assert int(training.so3_eps_index(nr.eps_array[500])) == 501
    sigma = np.concatenate([10 ** np.linspace(-3, 1, 401), nr.torus_sigma[::250]])
    assert np.array_equal(training.torus_sigma_index(sigma), nr.torus_sigma_index(sigma))
    assert int(training.torus_sigma_index(1e-4)) == 0 and int(training.torus_sigma_index(100.0)) == nr.T_SIGMA_N


def test_forward_purposes_do_not_collide():
    from disco_diffdock_amd import runtime
    fwd, old = runtime.RNG_FORWARD_PURPOSES, runtime.RNG_PURPOSES
    assert fwd == nr.FORWARD_PURPOSE
    assert not set(fwd.values()) & set(old.values()) and not set(fwd) & set(old)
    assert len(set(fwd.values())) == len(fwd) and all(0 <= v < 16 for v in fwd.values())
    assert runtime.RNG_LAYOUT == 1


def test_header_declares_the_calls_and_lib_lists_them():
    from disco_diffdock_amd import _lib, build
    with open(os.path.join(ROOT, 'include', 'ddk.h')) as f:
        header = f.read()
    for name in NEW_CALLS:
        assert re.search(r'^int ' + name + r'\(ddk_ctx\* ctx,', header, re.M), name
        assert name in _lib.SYMBOLS
    assert 'typedef struct ddk_perturbation' in header
    members = re.search(r'typedef struct ddk_perturbation \{(.*?)\} ddk_perturbation;', header, re.S).group(1)
    members = re.sub(r'/\*.*?\*/', '', members, flags=re.S)
    assert re.findall(r'\*(\w+)', members) == [k for k, _ in _lib.ddk_perturbation._fields_]
    assert 'k_so3.hip' in build.SOURCES and 'k_noising.hip' in build.SOURCES


def test_loss_restatement_on_a_hand_case():
    """B = 1, n_rot = 2, numbers small enough to do by hand"""
    out = nr.score_matching_loss([[1, 0, 0]], [[0, 2, 0]], [[1, 1]], [[0, 0, 0]], [[0, 0, 0]], [[0, 3]], 2.0, 0.5, 4.0)
    assert np.allclose(out[0, :2], [4 / 3, 16 / 3]) and np.allclose(out[0, 2], (1 / 4 + 4 / 4) / 2.0001)
    assert np.allclose(out[0, 3:5], 0) and np.allclose(out[0, 5], (9 / 4) / 2.0001)
