"""ddk_rng_noise / ddk_rng_initial / ddk_rng_uniform (csrc/k_rng.hip, csrc/k_philox.h) on the device against the numpy restatement tests/philox_ref.py
(tests/test_rng_host.py checks the restatement itself on the CPU, and runs the statistics below on it with the same seeds and counts).

What is bit-exact: the Philox words, hence the uniforms and the torsion angles (exact integer -> fp32 conversions and one multiplication), and every value
under a different cut of the same work into calls.  What is held to a derived bound: the normals, which go through the device library's logf, sqrtf,
sinpif and cospif.  With u = 2^-23 (one ulp of x is at most u |x|) and the library's error limits (OpenCL full profile, which the device library is
written to: log 3 ulp, sqrt 3 ulp, sinpi / cospi 4 ulp; products correctly rounded, 1/2 ulp):
    -2 log(u1)      relative 3 u           (the factor 2 is exact)
    r = sqrt(.)     relative 3 u / 2 + 3 u = 4.5 u
    c = cospi(2 u2) relative 4 u           (2 u2 is exact; at the exact zeros 2 u2 = 1/2, 3/2 four ulp of 0 is 0)
    z = r c         relative 4.5 u + 4 u + u / 2 = 9 u
so |z - z64| <= NORMAL_ULPS u |z64| with NORMAL_ULPS = 9.5, the half ulp on top covering the second-order terms and the fp64 restatement's own 1e-15.
No absolute term is needed: the smallest nonzero |z| is sqrt(2^-23) * pi 2^-23 = 1.3e-10, far from the subnormals.  A translation tr_sigma * z is one
more product: 10 u.  A rotation matrix entry is a sum of products of two components of the normalised quaternion: a component q_i / |q| carries 9 u (q_i)
+ 10.25 u (1 / sqrt of |q|^2, itself 2 * 9 u + 2.5 u) + 1.5 u (square root, division, product) = 21 u, a product of two 42.5 u of its size, and the
sizes of an entry's products sum to at most 1 (2 |xy| + 2 |zw| <= |q|^2 = 1), plus 1.5 u for the sums: ROTATION_ULPS = 45, absolute.  Orthogonality: the
matrix of a quaternion of squared norm s is s times a rotation; the computed s is 1 within 5.5 u (the roundings of the normalisation alone), so R^T R is
(1 +- 11 u) I, and the entries' own roundings (2 u each: four products, three sums) move R^T R by at most 2 sqrt(3) 2 u = 7 u: ORTHO_ULPS = 18, taken
as 24 for the second-order terms.

The largest observed errors are written as JSON when DDK_RNG_ERROR_PROFILE names a file (how profiles/rng_error.json is made); the bounds above were fixed
before any device run and are not derived from that file."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import philox_ref as pr

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NORMAL_ULPS, TRANSLATION_ULPS, ROTATION_ULPS, ORTHO_ULPS = 9.5, 10.5, 45.0, 24.0
FIGURES = {}


@pytest.fixture(scope='module')
def ctx():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


@pytest.fixture(scope='module', autouse=True)
def profile_file():
    """DDK_RNG_ERROR_PROFILE=<path>: the figures of this run as JSON"""
    yield
    path = os.environ.get('DDK_RNG_ERROR_PROFILE')
    if path and FIGURES:
        about = ('Largest observed errors of the device draws (csrc/k_rng.hip) against the fp64 restatement tests/philox_ref.py on an MI355X, in units of 2^-23 '
                 '(relative to |z| for normals and translations, absolute for rotation entries and R^T R - I), next to the derived bounds of '
                 'tests/test_gpu_rng.py, and the statistics of its one seed.  Written by that module under DDK_RNG_ERROR_PROFILE.')
        with open(path, 'w') as f:
            json.dump(dict(about=about, figures=FIGURES), f, indent=1, sort_keys=True)
            f.write('\n')


def _record(name, value, bound):
    prev = FIGURES.get(name, dict(observed=0.0))
    FIGURES[name] = dict(observed=max(prev['observed'], float('%.4g' % value)), bound=bound)


def _normal_err_ulps(got, want):
    """max |got - want| / (u |want|); entries where want == 0 must be 0 exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    assert (got[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((np.abs(got - want)[~zero] / (U * np.abs(want[~zero]))).max())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(t, ref32):
    return np.array_equal(_bits(t), np.ascontiguousarray(ref32, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('n_rot', [0, 1, 3, 4, 5, 9])
def test_torsions_bit_exact(ctx, n_rot, B):
    seed, stream, sample0 = 11, pr.fnv1a64('bits'), 6
    tor, rot, tr = ctx.rng_initial(seed, stream, sample0, B, n_rot, tr_sigma=19.0)
    want_tor, want_rot, want_tr = pr.initial(seed, stream, sample0, B, n_rot, 19.0)
    assert tuple(tor.shape) == (B, n_rot) and tuple(rot.shape) == (B, 3, 3) and tuple(tr.shape) == (B, 3)
    assert _same_bits(tor, want_tor)
    if n_rot:
        t = tor.cpu().numpy()
        assert (t >= -np.float32(np.pi)).all() and (t < np.float32(np.pi)).all()
    e_rot = float(np.abs(rot.cpu().numpy() - want_rot).max() / U)
    e_tr = _normal_err_ulps(tr.cpu().numpy(), want_tr)
    _record('rotation_entry', e_rot, ROTATION_ULPS)
    _record('translation', e_tr, TRANSLATION_ULPS)
    assert e_rot <= ROTATION_ULPS and e_tr <= TRANSLATION_ULPS
    # without the optional outputs the rotation is the same bits, and the optional ones are not produced
    t2, r2, x2 = ctx.rng_initial(seed, stream, sample0, B, n_rot, torsions=False, translations=False)
    assert t2 is None and x2 is None and torch.equal(r2, rot)


@pytest.mark.parametrize('decoding_idx', [0, 1, 7])
def test_uniforms_bit_exact(ctx, decoding_idx):
    seed, stream = 11, pr.fnv1a64('bits')
    for B, sample0 in ((1, 0), (3, 6), (300, 2)):      # 300: more than one workgroup
        u = ctx.rng_uniform(seed, stream, sample0, B, decoding_idx)
        assert _same_bits(u, pr.uniform(seed, stream, sample0, B, decoding_idx))
        assert float(u.min()) >= 0 and float(u.max()) < 1
    assert not torch.equal(ctx.rng_uniform(seed, stream, 0, 8, decoding_idx), ctx.rng_uniform(seed, stream, 0, 8, decoding_idx + 1))


def test_64_bit_seed_and_stream(ctx):
    """seeds 0 and 2^32, stream ids 1 and 2^32 + 1: truncating either to 32 bits would make two of the four equal"""
    outs = {}
    for seed in (0, 1 << 32):
        for stream in (1, (1 << 32) + 1):
            tor, rot, tr = ctx.rng_initial(seed, stream, 0, 3, 5)
            u = ctx.rng_uniform(seed, stream, 0, 3, 2)
            z = ctx.rng_noise(seed, stream, 0, 3, 2, 7)
            want_tor, want_rot, _ = pr.initial(seed, stream, 0, 3, 5)
            assert _same_bits(tor, want_tor) and _same_bits(u, pr.uniform(seed, stream, 0, 3, 2))
            assert np.abs(rot.cpu().numpy() - want_rot).max() <= ROTATION_ULPS * U
            assert _normal_err_ulps(z.cpu().numpy(), pr.noise(seed, stream, 0, 3, 0, 2, 7)) <= NORMAL_ULPS
            outs[(seed, stream)] = (tor.cpu(), u.cpu(), z.cpu(), rot.cpu())
    keys = list(outs)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            for a, b in zip(outs[keys[i]], outs[keys[j]]):
                assert not torch.equal(a, b), (keys[i], keys[j])


@pytest.mark.parametrize('n_cols', [6, 7, 9, 13])
@pytest.mark.parametrize('all_active', [False, True])
def test_noise_layout(ctx, n_cols, all_active):
    """B = 3, steps = 4, step0 = 2, sample0 = 5, noise_coeff rows [a, 0, a, a]: the zero step and the padded columns are exactly 0, every other value is the
    restatement's within NORMAL_ULPS (module docstring)"""
    seed, stream = 5, pr.fnv1a64('layout')
    n_active = n_cols if all_active else 6
    B, steps, step0, sample0 = 3, 4, 2, 5
    a = np.array([0.3, 0.0, 1.7], np.float32)
    nc = np.stack([a, np.zeros(3, np.float32), a, a])
    z = ctx.rng_noise(seed, stream, sample0, B, steps, n_cols, n_active, step0=step0, noise_coeff=nc).cpu().numpy()
    want = pr.noise(seed, stream, sample0, B, step0, steps, n_cols, n_active, nc)
    assert z.shape == (steps, B, n_cols)
    assert (z[1] == 0).all() and (z[:, :, n_active:] == 0).all()
    live = z[[0, 2, 3]][:, :, :n_active]
    assert (live != 0).all() and np.isfinite(z).all() and np.abs(z).max() <= 5.769
    err = _normal_err_ulps(z, want)
    _record('normal', err, NORMAL_ULPS)
    print(f'noise n_cols {n_cols} active {n_active}: {err:.3f} ulp (bound {NORMAL_ULPS})')
    assert err <= NORMAL_ULPS
    # noise_coeff = NULL: every step is active, and the active rows are the same bits
    z_all = ctx.rng_noise(seed, stream, sample0, B, steps, n_cols, n_active, step0=step0).cpu().numpy()
    assert np.array_equal(z_all[[0, 2, 3]], z[[0, 2, 3]]) and (z_all[1, :, :n_active] != 0).all()


def test_cut_invariance(ctx):
    """B = 40, steps = 20 in one call == five calls of B = 8 at sample0 = 0, 8, ... == two calls split at step0 = 10, bit for bit"""
    seed, stream, n_cols = 3, pr.fnv1a64('cuts'), 13
    whole = ctx.rng_noise(seed, stream, 0, 40, 20, n_cols)
    by_sample = torch.cat([ctx.rng_noise(seed, stream, s0, 8, 20, n_cols) for s0 in range(0, 40, 8)], dim=1)
    by_step = torch.cat([ctx.rng_noise(seed, stream, 0, 40, 10, n_cols, step0=k0) for k0 in (0, 10)], dim=0)
    assert torch.equal(whole, by_sample) and torch.equal(whole, by_step)
    tor, rot, tr = ctx.rng_initial(seed, stream, 0, 40, 9, tr_sigma=5.0)
    parts = [ctx.rng_initial(seed, stream, s0, 8, 9, tr_sigma=5.0) for s0 in range(0, 40, 8)]
    for k, full in enumerate((tor, rot, tr)):
        assert torch.equal(full, torch.cat([p[k] for p in parts]))
    assert torch.equal(ctx.rng_uniform(seed, stream, 0, 40, 3), torch.cat([ctx.rng_uniform(seed, stream, s0, 8, 3) for s0 in range(0, 40, 8)]))


def test_rotations(ctx):
    seed, stream, B = 21, pr.fnv1a64('rotations'), 257
    _, rot, _ = ctx.rng_initial(seed, stream, 4, B, 0)
    _, rot5, _ = ctx.rng_initial(seed, stream, 4, B, 0, purpose_rot=5)
    R = rot.cpu().numpy().astype(np.float64)
    ortho = float(np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() / U)
    _record('rotation_orthogonality', ortho, ORTHO_ULPS)
    assert ortho <= ORTHO_ULPS and np.linalg.det(R).min() > 0
    assert np.abs(R - pr.initial(seed, stream, 4, B, 0)[1]).max() <= ROTATION_ULPS * U
    R5 = rot5.cpu().numpy().astype(np.float64)
    assert np.abs(R5 - pr.initial(seed, stream, 4, B, 0, purpose_rot=5)[1]).max() <= ROTATION_ULPS * U
    assert np.abs(R5 - R).reshape(B, -1).max(axis=1).min() > 1e-3      # purpose 5 is another draw for every sample


def test_statistics(ctx):
    """one seed, N = 2^20 normals through rng_noise: |mean| < 5 / sqrt N, |var - 1| < 5 sqrt(2 / N), Kolmogorov-Smirnov distance < 1.95 / sqrt N (the 5-sigma
    widths and the 0.1 % critical value); 2^16 rotations: every entry of the mean matrix below 5 sqrt(1 / 3) / sqrt N"""
    z = ctx.rng_noise(pr.STAT_SEED, pr.STAT_STREAM, 0, **pr.STAT_NORMALS).cpu().numpy()
    n = z.size
    assert n == 1 << 20 and np.isfinite(z).all() and np.abs(z).max() <= 5.769
    mean, var, ks = pr.normal_statistics(z)
    b_mean, b_var, b_ks = pr.normal_statistics_bounds(n)
    print(f'device: |mean| {mean:.3e} < {b_mean:.3e}, |var - 1| {var:.3e} < {b_var:.3e}, KS {ks:.3e} < {b_ks:.3e}')
    FIGURES['statistics'] = dict(n=n, mean=float('%.4g' % mean), mean_bound=float(b_mean), var_minus_1=float('%.4g' % var), var_bound=float(b_var),
                                 ks=float('%.4g' % ks), ks_bound=float(b_ks))
    assert mean < b_mean and var < b_var and ks < b_ks
    _, rot, _ = ctx.rng_initial(pr.STAT_SEED, pr.STAT_STREAM, 0, pr.STAT_ROTATIONS, 0)
    m = np.abs(rot.cpu().numpy().astype(np.float64).mean(axis=0))
    bound = pr.rotation_mean_bound(pr.STAT_ROTATIONS)
    FIGURES['statistics'].update(rotations=pr.STAT_ROTATIONS, rotation_mean_max=float('%.4g' % m.max()), rotation_mean_bound=float(bound))
    assert (m < bound).all()


def test_refusals(ctx):
    """every broken limit is DDK_ERR_INVALID (-1) with a message, checked before anything is enqueued: the output buffer keeps its contents"""
    L, h = ctx.L, ctx.h
    dev = torch.device('cuda', ctx.device)
    out = torch.full((4096,), 7.0, device=dev)
    p, s = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nc = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    I32 = (1 << 31) - 1

    def noise(sample0=0, B=2, step0=0, steps=2, n_cols=8, n_active=8, ptr=p):
        return L.ddk_rng_noise(h, 1, 2, sample0, B, step0, steps, n_cols, n_active, nc, ptr, s)

    def initial(sample0=0, B=2, n_rot=3, purpose=2, rot=p):
        return L.ddk_rng_initial(h, 1, 2, sample0, B, n_rot, 1.0, purpose, None, rot, None, s)

    def uniform(sample0=0, B=2, idx=0, ptr=p):
        return L.ddk_rng_uniform(h, 1, 2, sample0, B, idx, ptr, s)

    bad = [lambda: noise(B=0), lambda: noise(sample0=-1), lambda: noise(sample0=I32 - 1, B=2), lambda: noise(step0=-1), lambda: noise(steps=0),
           lambda: noise(step0=(1 << 20) - 1, steps=2), lambda: noise(n_cols=0), lambda: noise(n_cols=1025), lambda: noise(n_active=-1),
           lambda: noise(n_active=9), lambda: noise(ptr=None),
           lambda: initial(B=0), lambda: initial(sample0=-1), lambda: initial(sample0=I32, B=1), lambda: initial(n_rot=-1), lambda: initial(n_rot=1025),
           lambda: initial(purpose=3), lambda: initial(rot=None),
           lambda: uniform(B=0), lambda: uniform(sample0=-1), lambda: uniform(sample0=I32 - 2, B=3), lambda: uniform(idx=-1), lambda: uniform(idx=1 << 20),
           lambda: uniform(ptr=None)]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert L.ddk_last_error(h).decode().startswith('ddk_rng_'), k
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the limits themselves are accepted: the last sample index, the last step, the last decoding index, the widest row
    assert noise(sample0=I32 - 2, B=2) == 0 and noise(step0=(1 << 20) - 2, steps=2) == 0 and noise(n_cols=1024, n_active=0, B=1, steps=1) == 0
    assert initial(sample0=I32 - 1, B=1) == 0 and uniform(sample0=I32 - 3, B=3, idx=(1 << 20) - 1) == 0
    torch.cuda.synchronize()
    # the Python wrappers turn the status into an exception that carries the library's text
    with pytest.raises(RuntimeError, match=r'n_cols.*rc=-1'):
        ctx.rng_noise(1, 2, 0, 2, 2, 1025)
    with pytest.raises(ValueError, match='int32'):
        ctx.rng_uniform(1, 2, 1 << 31, 2, 0)
    with pytest.raises(ValueError, match='64-bit'):
        ctx.rng_uniform(1 << 64, 2, 0, 2, 0)
