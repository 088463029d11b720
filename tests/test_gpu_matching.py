"""Conformer matching on the device (csrc/k_match.hip) through the C ABI and the Python shims, against the fp64 restatement of tests/matching_ref.py and
the yardstick of tests/golden/conformer_matching.npz (scipy's differential_evolution, the optimiser the reference calls).

The bar of every comparison with fp64 is tests/adversarial_geometry.py's: bar(err32, scale) = max(4 err32, 8 * 2^-24 scale), err32 the error of the rotor chain
restated in fp32 (with the reference's axis_angle_to_matrix) against fp64 on the same torsions.  The RMSD after the optimal fit is 1-Lipschitz in the RMS
displacement of the points, so the position bar of the rotor chain bounds it too."""
import ctypes as C

import numpy as np
import pytest
import torch

import adversarial_geometry as ag
import matching_ref as mr
import philox_ref as pr

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL = -77.0
YARD = dict(popsize=20, maxiter=20, polish_iters=128, n_islands=1, seed=0)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


@pytest.fixture(scope='module')
def cases(golden):
    return mr.golden_cases(golden)


def _case_stream(k):
    return pr.fnv1a64(f'case{mr.GOLDEN_SEEDS[k]}')


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(a, dt, dev):
    return None if a is None else T(np.ascontiguousarray(a, dt)).to(dev)


_ligands = {}


def _ligand(ctx, n):
    """-> (pos0 [n, 3] float32, rot_bonds [R, 2], mask_rotate [R, n]): synthetic.make_ligand for 16, 30 and 80 atoms (4, 5 and 29 rotors); for 256 a chain whose
    masks come from the device builder, cut to the 128 rotors the call takes (every rotor's row is valid on its own)"""
    if n not in _ligands:
        from disco_diffdock_amd import synthetic
        if n == 256:
            pos = ag._chain_positions(n, np.random.default_rng(356), planar=False).astype(np.float32)
            bi = np.zeros((2, 2 * (n - 1)), np.int64)
            bi[:, 0::2], bi[:, 1::2] = (np.arange(n - 1), np.arange(1, n)), (np.arange(1, n), np.arange(n - 1))
            em, mk = (t.cpu().numpy().astype(bool) for t in ctx.transformation_mask(n, bi))
            rb, mk = bi.T[em].reshape(-1, 2)[64:192], mk[64:192]
        else:
            lig = synthetic.make_ligand(np.random.default_rng({16: 11, 30: 30, 80: 80}[n]), n)
            pos, rb, mk = np.asarray(lig['lig_pos'], np.float32), mr.rotors(lig), np.asarray(lig['mask_rotate'], bool)
        assert len(pos) == n and len(rb) == {16: 4, 30: 5, 80: 29, 256: 128}[n]
        _ligands[n] = (pos, rb, mk)
    return _ligands[n]


def _target(pos0, rb, mk, seed, offset=0.0, noise=0.15):
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    t = mr.apply_torsions(pos0, rb, mk, rng.uniform(-np.pi, np.pi, size=len(rb))) @ Rotation.random(random_state=seed).as_matrix().T
    t = t - t.mean(0) + 5.0 * rng.normal(size=3) + noise * rng.normal(size=t.shape)
    return (t + np.array([offset, -offset, offset])).astype(np.float32)


def _torsion_rows(R, M=512, seed=0):
    """uniform rows with the special values placed: all-zero rows, exact zeros among non-zeros, +-fp32(pi), 1e-7"""
    rng = np.random.default_rng(seed)
    tor = rng.uniform(-np.pi, np.pi, size=(M, R)).astype(np.float32)
    tor[:4] = 0
    for m in range(4, 36):
        tor[m, rng.choice(R, size=max(1, R // 2), replace=False)] = 0
    for m in range(36, 68):
        tor[m, rng.choice(R, size=max(1, R // 3), replace=False)] = np.float32(np.pi) * rng.choice([-1.0, 1.0])
    for m in range(68, 100):
        tor[m, rng.choice(R, size=max(1, R // 2), replace=False)] = np.float32(1e-7)
    tor[100] = np.float32(np.pi)
    tor[101] = np.float32(1e-7)
    if R > 64:
        tor[102] = 0
        tor[102, 63:66] = 1.0      # the rotors on both sides of the wave width alone
    return tor


def _raw_match(ctx, dev, pos0, target, rb, mk, mask=None, ws_fill=0xA5, **opt):
    """ddk_conformer_match through the C ABI with every output pre-filled with a sentinel and a garbage workspace -> host (torsions, pos, rmsd [2], count [2])"""
    from disco_diffdock_amd import _lib
    n, R = len(pos0), len(rb)
    o = dict(popsize=15, maxiter=15, tol=0.01, polish_iters=128, n_islands=1, seed=0, stream_id=0)
    o.update(opt)
    d = [_up(pos0, np.float32, dev), _up(target, np.float32, dev), _up(mask, np.uint8, dev), _up(rb, np.int32, dev) if R else None,
         _up(mk, np.uint8, dev) if R else None]
    tor = torch.full((max(R, 1),), SENTINEL, dtype=torch.float32, device=dev)
    pos = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    rmsd = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev)
    count = torch.full((2,), int(SENTINEL), dtype=torch.int32, device=dev)
    nbytes = ctx.L.ddk_conformer_match_workspace(n, R, o['popsize'], o['n_islands'])
    ws = torch.full((max(nbytes, 16),), ws_fill, dtype=torch.uint8, device=dev)
    co = _lib.ddk_match_options(**o)
    rc = ctx.L.ddk_conformer_match(ctx.h, n, *[_ptr(t) for t in d], R, C.byref(co), _ptr(tor), _ptr(pos), _ptr(rmsd), _ptr(count), _ptr(ws), _stream())
    torch.cuda.synchronize()
    return rc, tor.cpu().numpy()[:R] if R else tor.cpu().numpy(), pos.cpu().numpy(), rmsd.cpu().numpy(), count.cpu().numpy()


# ---- 1. the objective -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0.0, 150.0])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('n', [16, 30, 80, 256])
def test_objective_against_fp64(ctx, dev, n, masked, offset):
    pos0, rb, mk = _ligand(ctx, n)
    target = _target(pos0, rb, mk, seed=n, offset=offset)
    mask = (np.arange(n) % 4 != 1) if masked else None
    tor = _torsion_rows(len(rb))
    got = ctx.conformer_rmsd(pos0, target, rb, mk, tor, atom_mask=mask).cpu().numpy().astype(np.float64)
    p64, p32 = mr.apply_torsions_batch(pos0, rb, mk, tor), mr.apply_torsions_batch(pos0, rb, mk, tor, np.float32)
    want = mr.fit_rmsd_batch(p64, target, mask)
    err32 = np.abs(p32.astype(np.float64) - p64).max(axis=(1, 2))
    bars = np.maximum(ag.K * err32, ag.FLOOR * float(np.abs(pos0).max()))
    err = np.abs(got - want)
    worst = int(np.argmax(err / bars))
    print(f'objective n = {n} R = {len(rb)} masked = {masked} offset = {offset:g}: max |rmsd - fp64| {err.max():.2e}, worst {err[worst]:.2e} against its bar '
          f'{bars[worst]:.2e} (fp32 chain {err32[worst]:.2e}; largest fp32 chain error {err32.max():.2e})')
    assert np.isfinite(got).all() and (err <= bars).all()


# ---- 2. the yardstick -------------------------------------------------------------------------------------------------------------------------------------
def test_yardstick_cases_reach_scipy(ctx, dev, cases):
    miss, rows = [], []
    for k, g in enumerate(cases):
        pos0, target, rb, mk = g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate']
        out = ctx.match_conformer(pos0, target, rb, mk, stream=_case_stream(k), **YARD)
        nop = ctx.match_conformer(pos0, target, rb, mk, stream=_case_stream(k), **dict(YARD, polish_iters=0))
        tor = out['torsions'].cpu().numpy()
        host = mr.objective(pos0, target, rb, mk, tor)
        rigid, matched = float(out['rmsd_rigid']), float(out['rmsd'])
        p64, p32 = mr.apply_torsions_batch(pos0, rb, mk, tor[None]), mr.apply_torsions_batch(pos0, rb, mk, tor[None], np.float32)
        err32 = float(np.abs(p32 - p64).max())
        host_nop = mr.objective(pos0, target, rb, mk, nop['torsions'].cpu().numpy())
        rows.append((mr.GOLDEN_SEEDS[k], float(g['fun']), host, host_nop, rigid, int(out['generations'])))
        print(f'case {mr.GOLDEN_SEEDS[k]}: scipy {float(g["fun"]):.4f}, device {host:.4f} (fp64 of its torsions; its own {matched:.4f}), without polish {host_nop:.4f}, '
              f'rigid {rigid:.4f}, {int(out["generations"])} generations')
        assert int(out['status']) == 0 and int(nop['status']) == 0
        assert matched <= rigid and float(nop['rmsd']) <= float(nop['rmsd_rigid'])      # the monotone guarantee, with and without polish
        assert abs(matched - host) <= ag.bar(err32, np.abs(pos0).max())
        assert abs(rigid - float(g['rigid'])) <= ag.bar(0.0, np.abs(pos0).max())
        want_pos = mr.matched_pose(pos0, target, rb, mk, tor)
        assert ag.max_err(out['pos'].cpu().numpy(), want_pos) <= ag.bar(err32, np.abs(target).max())
        if host > float(g['fun']) + 0.01:
            miss.append(rows[-1])
    assert len(miss) <= 1, miss


# ---- 3. exact recovery --------------------------------------------------------------------------------------------------------------------------------------
def test_exact_recovery_with_four_islands(ctx, dev):
    miss = []
    for k, seed in enumerate(mr.GOLDEN_SEEDS):
        c = mr.golden_case(seed, noise=0.0)
        out = ctx.match_conformer(c['pos0'], c['target'], c['rot_bonds'], c['mask_rotate'], stream=_case_stream(k), **dict(YARD, n_islands=4, maxiter=100))
        r = float(out['rmsd'])
        print(f'exact recovery case {seed}: matched {r:.5f} (rigid {float(out["rmsd_rigid"]):.4f}) after {int(out["generations"])} generations')
        if not r < 0.01:
            miss.append((seed, r))
    assert len(miss) <= 1, miss


# ---- 4. determinism and stream independence -------------------------------------------------------------------------------------------------------------------
def _bits(out):
    return [out[k].cpu().numpy().tobytes() for k in ('torsions', 'pos', 'rmsd', 'rmsd_rigid', 'generations')]


def test_determinism(ctx, dev, cases):
    g = cases[3]
    args = (g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate'])
    a = ctx.match_conformer(*args, stream=5, **YARD)
    b = ctx.match_conformer(*args, stream=5, **YARD)
    # an unrelated seeded sampling call in between (the set-up of tests/test_gpu_seeded_sampling.py: 3 steps, 8 samples, random weights), same seed and more
    # draws from the same generator's older purposes
    from functools import partial
    from oracle import score_model_ref as smr
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    from disco_diffdock_amd.model_utils import get_model
    import test_gpu_seeded_sampling as tss
    model = get_model(tss.ARGS, dev, partial(t_to_sigma, args=tss.ARGS), no_parallel=True)
    model.score_model.load_state_dict(smr.random_state_dict(smr.ScoreModelConfig(latent_vocab=64), seed=7), strict=True)
    poses, _ = tss._run(model, synthetic.make_complex(31, n_res=40, n_lig=22), dev, seed=0)
    assert torch.isfinite(poses).all()
    ctx.rng_noise(0, 5, 0, 8, 3, 12)
    c = ctx.match_conformer(*args, stream=5, **YARD)
    assert _bits(a) == _bits(b) == _bits(c)
    other = ctx.match_conformer(*args, stream=5, **dict(YARD, seed=1, maxiter=0, polish_iters=0))
    same = ctx.match_conformer(*args, stream=5, **dict(YARD, maxiter=0, polish_iters=0))
    again = ctx.match_conformer(*args, stream=5, **dict(YARD, maxiter=0, polish_iters=0))
    # maxiter = 0 without polish returns the best member of the generation-0 population: another seed draws another one
    assert _bits(same) == _bits(again) and _bits(other)[0] != _bits(same)[0]
    R, NP = len(g['rot_bonds']), mr.members(20, len(g['rot_bonds']))
    pop = mr.initial_population(0, 5, 0, NP, R)
    assert any(np.array_equal(same['torsions'].cpu().numpy(), row) for row in pop)      # bit for bit a member of the restated population


def test_islands_and_generations_never_hurt(ctx, dev, cases):
    for k in (0, 4, 10):
        g = cases[k]
        args = (g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate'])
        one = ctx.match_conformer(*args, stream=_case_stream(k), **dict(YARD, polish_iters=0))
        four = ctx.match_conformer(*args, stream=_case_stream(k), **dict(YARD, polish_iters=0, n_islands=4))
        assert float(four['rmsd']) <= float(one['rmsd'])      # island 0 draws the same numbers
        short = ctx.match_conformer(*args, stream=_case_stream(k), **dict(YARD, polish_iters=0, tol=0.0, maxiter=5))
        long = ctx.match_conformer(*args, stream=_case_stream(k), **dict(YARD, polish_iters=0, tol=0.0, maxiter=20))
        assert float(long['rmsd']) <= float(short['rmsd'])      # the first five generations are the same computation
        assert int(short['generations']) == 5 and int(long['generations']) == 20
        print(f'case {mr.GOLDEN_SEEDS[k]}: 1 island {float(one["rmsd"]):.4f}, 4 islands {float(four["rmsd"]):.4f}; 5 generations {float(short["rmsd"]):.4f}, '
              f'20 generations {float(long["rmsd"]):.4f}')


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------------------------------
def test_no_rotor_is_the_rigid_fit(ctx, dev, cases):
    g = cases[0]
    rc, tor, pos, rmsd, count = _raw_match(ctx, dev, g['pos0'], g['target'], np.zeros((0, 2), np.int32), np.zeros((0, len(g['pos0'])), bool))
    assert rc == 0 and list(count) == [0, 0] and rmsd[0] == rmsd[1]
    want, moved = mr.fit_rmsd(np.asarray(g['pos0'], np.float64), np.asarray(g['target'], np.float64))
    assert abs(rmsd[0] - want) <= ag.FLOOR * np.abs(g['pos0']).max() and abs(rmsd[0] - float(g['rigid'])) <= ag.FLOOR * np.abs(g['pos0']).max()
    assert ag.max_err(pos, moved) <= ag.FLOOR * np.abs(g['target']).max()
    assert (tor == SENTINEL).all()      # nothing to write


def test_polish_alone_improves_and_identity_target(ctx, dev, cases):
    g = cases[1]
    out = ctx.match_conformer(g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate'], stream=1, **dict(YARD, maxiter=0))
    assert int(out['generations']) == 0 and float(out['rmsd']) < float(out['rmsd_rigid'])
    same = ctx.match_conformer(g['pos0'], g['pos0'], g['rot_bonds'], g['mask_rotate'], stream=1, **YARD)
    assert float(same['rmsd']) < 1e-3 and float(same['rmsd_rigid']) < 1e-3
    assert mr.objective(g['pos0'], g['pos0'], g['rot_bonds'], g['mask_rotate'], same['torsions'].cpu().numpy()) < 1e-3      # the torsions reproduce it
    assert ag.max_err(same['pos'].cpu().numpy(), g['pos0']) < 3e-3


def test_status_2_and_3_write_nothing(ctx, dev, cases):
    g = cases[2]
    pos0, target, rb, mk = g['pos0'], g['target'], g['rot_bonds'].copy(), g['mask_rotate'].copy()
    n, R = len(pos0), len(rb)
    u, v = rb[1]

    def causes():
        for bad in (-1, n):
            b = rb.copy(); b[1, 0] = bad
            yield f'u = {bad}', dict(rb=b), 2
            b = rb.copy(); b[R - 1, 1] = bad
            yield f'v = {bad}', dict(rb=b), 2
        b = rb.copy(); b[1, 0] = b[1, 1]
        yield 'u == v', dict(rb=b), 2
        m = mk.copy(); m[1, u] = True
        yield 'mask[u] set', dict(mk=m), 2
        m = mk.copy(); m[1, v] = False
        yield 'mask[v] clear', dict(mk=m), 2
        keep = np.zeros(n, bool); keep[:2] = True
        yield 'two kept atoms', dict(mask=keep), 2
        for value in (np.nan, np.inf):
            p = pos0.copy(); p[n - 1, 2] = value
            yield f'pos0 {value}', dict(pos0=p), 3
            t = target.copy(); t[0, 0] = -value
            yield f'target {-value}', dict(target=t), 3

    for name, change, status in causes():
        a = dict(pos0=pos0, target=target, rb=rb, mk=mk, mask=None)
        a.update(change)
        rc, tor, pos, rmsd, count = _raw_match(ctx, dev, a['pos0'], a['target'], a['rb'], a['mk'], mask=a['mask'], **YARD)
        assert rc == 0 and list(count) == [0, status], (name, count)
        assert (tor == SENTINEL).all() and (pos == SENTINEL).all() and (rmsd == SENTINEL).all(), name
        # the objective alone refuses the same input
        r, st = ctx.conformer_rmsd(a['pos0'], a['target'], a['rb'], a['mk'], np.zeros((3, R), np.float32), atom_mask=a['mask'], return_status=True)
        assert int(st) == status, name


def test_broken_limits_are_refused(ctx, dev, cases):
    g = cases[2]
    pos0, target, rb, mk = g['pos0'], g['target'], g['rot_bonds'], g['mask_rotate']
    for bad in (dict(popsize=0), dict(popsize=65), dict(maxiter=-1), dict(maxiter=1001), dict(polish_iters=-1), dict(polish_iters=1025), dict(n_islands=0),
                dict(n_islands=17), dict(tol=-1.0), dict(tol=float('nan'))):
        rc, tor, pos, rmsd, count = _raw_match(ctx, dev, pos0, target, rb, mk, **bad)
        assert rc == -1 and ctx.L.ddk_last_error(ctx.h).decode().startswith('ddk_conformer_match'), bad
        assert (pos == SENTINEL).all() and (count == int(SENTINEL)).all(), bad      # nothing was enqueued
    # (NP = max(5, popsize * n_rot) <= 8192 follows from popsize <= 64 and n_rot <= 128: it has no case of its own)
    # n_lig outside [3, 256] for the search itself (the arrays are long enough for what is declared; nothing is enqueued)
    long = np.zeros((257, 3), np.float32)
    for n_bad in (2, 257):
        rc, tor, pos, rmsd, count = _raw_match(ctx, dev, long[:n_bad], long[:n_bad], np.zeros((0, 2), np.int32), np.zeros((0, n_bad), bool))
        assert rc == -1 and ctx.L.ddk_last_error(ctx.h).decode().startswith('ddk_conformer_match: n_lig'), n_bad
        assert (pos == SENTINEL).all() and (count == int(SENTINEL)).all(), n_bad
    with pytest.raises(RuntimeError, match='ddk_conformer_match: n_rot'):
        ctx.match_conformer(pos0, target, np.tile(rb[:1], (129, 1)), np.tile(mk[:1], (129, 1)))
    with pytest.raises(RuntimeError, match='ddk_conformer_rmsd: n_lig'):
        ctx.conformer_rmsd(long, long, np.zeros((0, 2)), np.zeros((0, 257)), np.zeros((1, 0), np.float32))
    with pytest.raises(RuntimeError, match='ddk_conformer_rmsd: M must be'):      # M = 65537; 65536 is taken
        ctx.conformer_rmsd(pos0, target, rb, mk, np.zeros((65537, len(rb)), np.float32))
    assert tuple(ctx.conformer_rmsd(pos0, target, rb, mk, np.zeros((65536, len(rb)), np.float32)).shape) == (65536,)
    with pytest.raises(RuntimeError, match='ddk_conformer_rmsd: n_lig'):
        ctx.conformer_rmsd(pos0[:2], target[:2], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((1, 0), np.float32))
    with pytest.raises(RuntimeError, match='ddk_conformer_rmsd: n_rot'):
        ctx.conformer_rmsd(pos0, target, np.tile(rb[:1], (129, 1)), np.tile(mk[:1], (129, 1)), np.zeros((1, 129), np.float32))
    from disco_diffdock_amd import _lib
    co = _lib.ddk_match_options(15, 15, 0.01, 128, 1, 0, 0)
    out = torch.zeros(64, device=dev)
    assert ctx.L.ddk_conformer_match(ctx.h, len(pos0), None, _ptr(out), None, None, None, 0, C.byref(co), None, _ptr(out), _ptr(out), _ptr(out), _ptr(out), _stream()) == -1
    assert 'null argument' in ctx.L.ddk_last_error(ctx.h).decode()
    assert ctx.L.ddk_conformer_rmsd(ctx.h, len(pos0), _ptr(out), _ptr(out), None, None, None, 0, 0, None, _ptr(out), _ptr(out), _stream()) == -1
    assert 'M must be' in ctx.L.ddk_last_error(ctx.h).decode()


# ---- 6. the shim ----------------------------------------------------------------------------------------------------------------------------------------------
def test_graphs_match_conformer_and_validation_loss(ctx, dev):
    from oracle import score_model_ref as smr
    from disco_diffdock_amd import graphs, synthetic, training
    from disco_diffdock_amd.runtime import Context, stream_id
    c = synthetic.make_complex(7, n_res=60)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    rb, mk = mr.rotors(c), np.asarray(c['mask_rotate'], bool)
    assert len(rb) > 0
    rng = np.random.default_rng(3)
    conformer = mr.apply_torsions(c['lig_pos'], rb, mk, rng.uniform(-np.pi, np.pi, size=len(rb))).astype(np.float32) + np.float32(3.0)
    out = graphs.match_conformer(c, conformer, ctx=ctx, popsize=20, maxiter=20)
    assert out is c and set(c) - set(before) == {'orig_pos', 'orig_rdkit_pos', 'rmsd_matching'}
    for k, v in before.items():
        if k != 'lig_pos':
            assert (np.array_equal(c[k], v) if isinstance(v, np.ndarray) else c[k] == v), k
    assert np.array_equal(c['orig_pos'], before['lig_pos']) and np.array_equal(c['orig_rdkit_pos'], conformer)
    assert c['lig_pos'].shape == before['lig_pos'].shape and c['lig_pos'].dtype == np.float32
    direct = ctx.match_conformer(conformer, before['lig_pos'], rb, mk, popsize=20, maxiter=20, stream=stream_id(c['name']))
    assert np.array_equal(direct['pos'].cpu().numpy(), c['lig_pos']) and float(direct['rmsd']) == c['rmsd_matching']
    rigid = mr.fit_rmsd(conformer.astype(np.float64), before['lig_pos'].astype(np.float64))[0]
    assert c['rmsd_matching'] <= rigid + 1e-5 and abs(mr.fit_rmsd(c['lig_pos'].astype(np.float64), c['orig_pos'].astype(np.float64))[0] - c['rmsd_matching']) < 1e-4
    print(f'shim: rmsd_matching {c["rmsd_matching"]:.4f} (rigid {rigid:.4f}), {len(rb)} rotors')
    model = Context(device=0, deterministic=1)
    model.load_state_dict(smr.random_state_dict(smr.ScoreModelConfig(latent_vocab=64), seed=23))
    a = training.validation_loss(model, [c], t_values=[0.5], samples_per_complex=2, seed=3)
    assert a['n'] == 2 and np.isfinite(a['loss'])
