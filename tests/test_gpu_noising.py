"""ddk_so3_rows, ddk_torus_score, ddk_rng_perturbation and ddk_score_matching_loss (csrc/k_so3.hip, csrc/k_noising.hip) and disco_diffdock_amd.training on
the device, against the fp64 NumPy restatement tests/noising_ref.py (tests/test_noising_host.py checks the restatement itself against values recorded from
the reference and against the shipped so3_exp_score_norms.npy).

The bars.  An IGSO(3) row is a sum of 2000 terms of alternating sign; where the density vanishes the sum cancels and the reference's own tables are noise.
The yardstick is therefore the restatement's disagreement with ITSELF when the same terms are added in the opposite order, d (per row and quantity,
computed here and printed): device and host sin / cos / exp differ by an ulp per term, which perturbs the sums about as much as the order does, hence 100 d,
with floors 1e-13 (CDF, absolute), 1e-12 (scores, relative, on the entries with pdf >= 1e-6 max(pdf) only) and 1e-10 (exp_score_norm, relative, against the
shipped table).  A torus score is ONE fp64 evaluation rounded to fp32: 1e-6 relative + 1e-12 absolute (the reference has ~1e-17 noise at the zero crossing
|x| = pi).  The perturbation's updates and scores: 1e-5 of each vector's norm (one fp32 rounding, 6e-8; the normals' 9.5 ulp = 1.1e-6; table noise at the
farthest reachable bracket <= 1.3e-7).  The loss terms: fp64 inside, one rounding: 1e-6 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

import noising_ref as nr
import philox_ref as pr

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
NORMAL_ULPS = 9.5      # tests/test_gpu_rng.py: a normal of the device against the fp64 restatement, relative, in units of 2^-23
ROWS = (0, 1, 130, 500, 868, 999)
POSE_BAR, PARITY_BAR = 1e-3, 1e-4      # tests/test_gpu_trajectory.py's pose bar; the project's parity bar for scores


@pytest.fixture(scope='module')
def ctx():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


@pytest.fixture(scope='module')
def ref_rows():
    """the restatement's rows, ascending and descending, computed once and left unchanged"""
    return {i: (nr.so3_row(i), nr.so3_row(i, descending=True)) for i in ROWS}


def _rel(a, b):
    return np.abs(a - b) / np.abs(b)


def _esn_d(asc, desc):
    return abs(asc['exp_score_norm_finite'] - desc['exp_score_norm_finite']) / asc['exp_score_norm_finite']


def test_so3_rows_six_rows(ctx, ref_rows, tables):
    cdf, score, esn = (t.cpu().numpy() for t in ctx.so3_rows(ROWS))
    assert cdf.shape == score.shape == (len(ROWS), 2000) and esn.shape == (len(ROWS),)
    for k, i in enumerate(ROWS):
        asc, desc = ref_rows[i]
        live, contiguous, share = nr.live_set(asc['pdf'])
        assert contiguous and share >= 0.99999, (i, contiguous, share)
        d_cdf = float(np.abs(asc['cdf'] - desc['cdf']).max())
        d_score = float(_rel(desc['score'][live], asc['score'][live]).max())
        d_esn = _esn_d(asc, desc)
        e_cdf = float(np.abs(cdf[k] - asc['cdf']).max())
        e_score = float(_rel(score[k][live], asc['score'][live]).max())
        e_esn = abs(esn[k] - tables[0][i]) / tables[0][i]
        print(f'row {i}: d cdf {d_cdf:.2e} score {d_score:.2e} esn {d_esn:.2e} | device cdf {e_cdf:.2e} score {e_score:.2e} esn {e_esn:.2e} '
              f'({int(live.sum())} live entries, share {share:.9f})')
        assert e_cdf <= max(100 * d_cdf, 1e-13), i
        assert e_score <= max(100 * d_score, 1e-12), i
        assert e_esn <= max(100 * d_esn, 1e-10), i


def test_so3_rows_whole_table_duplicates_and_null_outputs(ctx, tables):
    _, _, esn = ctx.so3_rows(np.arange(1000), cdf=False, score=False)
    esn = esn.cpu().numpy()
    err = np.abs(esn - tables[0]) / tables[0]
    print(f'all 1000 rows: exp_score_norm max rel diff to the shipped table {err.max():.2e} at row {int(err.argmax())}')
    for i in np.flatnonzero(~(err <= 1e-10)):      # the bar is max(100 d, 1e-10): d is only worked out for the rows beyond the floor
        d = _esn_d(nr.so3_row(int(i)), nr.so3_row(int(i), descending=True))
        print(f'row {i}: {err[i]:.2e}, d = {d:.2e}')
        assert err[i] <= 100 * d, i
    # duplicates and any order: every copy is the same bits as the row of the whole-table call; any subset of the outputs
    idx = [999, 3, 3, 500, 0, 3]
    cdf, score, e2 = ctx.so3_rows(idx)
    assert np.array_equal(e2.cpu().numpy(), esn[idx])
    assert torch.equal(cdf[1], cdf[2]) and torch.equal(cdf[1], cdf[5]) and torch.equal(score[1], score[2])
    c_only, none_s, none_e = ctx.so3_rows(idx, score=False, exp_score_norm=False)
    assert none_s is None and none_e is None and torch.equal(c_only, cdf)
    _, s_only, _ = ctx.so3_rows(idx, cdf=False, exp_score_norm=False)
    assert torch.equal(s_only.view(torch.int64), score.view(torch.int64))      # bits: the dead tail holds NaN
    c = cdf.cpu().numpy()
    assert np.isfinite(c).all() and (np.abs(c[:, -1] - 1) < 1e-2).all()


def test_so3_rows_refusals(ctx):
    L, h = ctx.L, ctx.h
    out = torch.full((2 * 2000,), 7.0, dtype=torch.float64, device=torch.device('cuda', ctx.device))
    p, s = C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = (C.c_int32 * 2)(0, 999)
    big = (C.c_int32 * 4097)()
    bad = [lambda: L.ddk_so3_rows(h, 0, ok, p, None, None, s), lambda: L.ddk_so3_rows(h, 4097, big, None, None, p, s),
           lambda: L.ddk_so3_rows(h, 2, None, p, None, None, s), lambda: L.ddk_so3_rows(h, 2, ok, None, None, None, s),
           lambda: L.ddk_so3_rows(h, 2, (C.c_int32 * 2)(0, 1000), p, None, None, s), lambda: L.ddk_so3_rows(h, 2, (C.c_int32 * 2)(-1, 5), p, None, None, s)]
    for k, call in enumerate(bad):
        assert call() == -1, k
        assert L.ddk_last_error(h).decode().startswith('ddk_so3_rows'), k
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match=r'eps_idx.*rc=-1'):
        ctx.so3_rows([1000])


@pytest.mark.parametrize('sigma_idx', [0, 2500, 5000])
def test_torus_score_draws(ctx, sigma_idx):
    rng = np.random.default_rng(sigma_idx)
    sigma = nr.torus_sigma[sigma_idx]
    x = (rng.uniform(-8, 8, 4096) * sigma).astype(np.float32)
    x[:4] = (0.0, -0.0, np.float32(np.pi), -np.float32(np.pi))
    got = ctx.torus_score(torch.from_numpy(x).cuda(), sigma_idx).cpu().numpy().astype(np.float64)
    want = nr.torus_score(x, sigma_idx)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(got - want)[~nan]
    print(f'sigma index {sigma_idx}: {int(nan.sum())} NaN of {x.size}, max err / (1e-6 |ref| + 1e-12) = {float((err / (1e-6 * np.abs(want[~nan]) + 1e-12)).max()):.3f}')
    assert (err <= 1e-6 * np.abs(want[~nan]) + 1e-12).all()
    assert (got[:2] == 0).all()
    if sigma_idx == 0:
        assert nan.any()      # |x| beyond ~38 sigma underflows p: the reference's NaN


def test_torus_score_golden_points(ctx, golden):
    g = golden('noising')
    x, sigma, want = g['torus_x'], g['torus_sigma'], g['torus_score']
    idx = nr.torus_sigma_index(sigma)
    x32 = x.astype(np.float32)
    got = np.concatenate([ctx.torus_score(torch.from_numpy(x32[k:k + 1]).cuda(), int(idx[k])).cpu().numpy() for k in range(len(x))]).astype(np.float64)
    same_cell = nr.torus_score(x32, idx) == nr.torus_score(x, idx)      # the fp32 rounding of x may move a point to the next grid cell: not the kernel's doing
    nan = np.isnan(want)
    assert nan[:2].all() and np.array_equal(np.isnan(got), nan)
    keep = same_cell & ~nan
    assert keep.sum() >= 200
    assert (np.abs(got - want)[keep] <= 1e-6 * np.abs(want[keep]) + 1e-12).all()
    # shapes pass through, an empty tensor is fine, a sigma index outside the table is refused
    assert tuple(ctx.torus_score(torch.zeros(3, 5, device='cuda'), 7).shape) == (3, 5) and ctx.torus_score(torch.zeros(0, device='cuda'), 7).numel() == 0
    with pytest.raises(RuntimeError, match=r'sigma_idx.*rc=-1'):
        ctx.torus_score(torch.zeros(4, device='cuda'), 5001)


def _sigmas(t):
    from disco_diffdock_amd.diffusion_utils import t_to_sigma
    from disco_diffdock_amd.runtime import DEFAULTS
    from types import SimpleNamespace
    return tuple(float(v) for v in t_to_sigma(t, t, t, SimpleNamespace(**DEFAULTS)))


def _vec_err(got, want):
    """max over the rows of |got - want| / |want| (2-norms); an all-zero row must be all zero"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    n = np.linalg.norm(want, axis=-1)
    assert (got[n == 0] == 0).all()
    return float((np.linalg.norm(got - want, axis=-1)[n > 0] / n[n > 0]).max()) if (n > 0).any() else 0.0


def test_perturbation_raw_draws(ctx):
    """tr_sigma = tor_sigma = 1 makes the translation and torsion updates the raw normals of purposes 6 and 8; a cdf row that is linear in the angle makes
    |rot_update| / pi the raw uniform of purpose 7 and rot_update / |rot_update| its normalised axis"""
    seed, stream, sample0, B, n_rot, draw = 17, pr.fnv1a64('raw'), 6, 5, 9, 3
    lin = torch.arange(1, 2001, dtype=torch.float64, device='cuda') / 2000
    p = ctx.rng_perturbation(seed, stream, sample0, B, n_rot, 1.0, 1.0, 2500, lin, None, draw=draw, scores=False)
    assert p.tr_score is None and p.rot_score is None and p.tor_score is None
    z_tr, a, u, z_tor = nr.perturbation_words(seed, stream, sample0, B, draw, n_rot)
    for got, want in ((p.tr_update, z_tr), (p.tor_update, z_tor)):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == want.shape and (np.abs(got - want) <= NORMAL_ULPS * U * np.abs(want)).all()
    rot = p.rot_update.cpu().numpy().astype(np.float64)
    om = np.linalg.norm(rot, axis=1)
    assert (u >= 1 / 2000).all() and (np.abs(om / np.pi - u) <= 4 * U * u).all()
    axis = a / np.linalg.norm(a, axis=1, keepdims=True)
    assert np.abs(rot / om[:, None] - axis).max() <= (2 * NORMAL_ULPS + 4) * U


@pytest.mark.parametrize('t', [0.02, 0.5, 0.98])
@pytest.mark.parametrize('n_rot', [0, 3, 9])
def test_perturbation_vs_restatement(ctx, n_rot, t):
    seed, stream, sample0, B, draw = 29, pr.fnv1a64('forward'), 11, 5, 2
    tr_sigma, rot_sigma, tor_sigma = _sigmas(t)
    eps_idx, tor_idx = int(nr.so3_eps_index(rot_sigma)), int(nr.torus_sigma_index(tor_sigma))
    cdf, score, _ = ctx.so3_rows([eps_idx], exp_score_norm=False)
    p = ctx.rng_perturbation(seed, stream, sample0, B, n_rot, tr_sigma, tor_sigma, tor_idx, cdf[0], score[0], draw=draw)
    row = nr.so3_row(eps_idx)
    want = nr.perturbation(*nr.perturbation_words(seed, stream, sample0, B, draw, n_rot), tr_sigma, tor_sigma, tor_idx, row['cdf'], row['score'])
    errs = {}
    for k in ('tr_update', 'rot_update', 'tor_update', 'tr_score', 'rot_score'):
        got = getattr(p, k).cpu().numpy()
        assert got.shape == want[k].shape, k
        errs[k] = _vec_err(got, want[k])
    # tor_score is the torus arithmetic on the device's own fp32 tor_update (the quantisation to the grid is a step function of it)
    tor_upd = p.tor_update.cpu().numpy()
    errs['tor_score'] = _vec_err(p.tor_score.cpu().numpy(), nr.torus_score(tor_upd, tor_idx)) if n_rot else 0.0
    print(f't {t} n_rot {n_rot}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert all(np.isfinite(getattr(p, k).cpu().numpy()).all() for k in want)
    assert max(errs.values()) <= 1e-5, errs
    om = np.linalg.norm(p.rot_update.cpu().numpy().astype(np.float64), axis=1)
    assert (om > 0).all() and (om <= np.pi * (1 + 1e-6)).all()


def test_perturbation_cuts_draws_and_older_purposes(ctx):
    seed, stream, n_rot = 5, pr.fnv1a64('cuts'), 9
    tr_sigma, rot_sigma, tor_sigma = _sigmas(0.5)
    cdf, score, _ = ctx.so3_rows([int(nr.so3_eps_index(rot_sigma))], exp_score_norm=False)
    args = (tr_sigma, tor_sigma, int(nr.torus_sigma_index(tor_sigma)), cdf[0], score[0])
    noise0, init0 = ctx.rng_noise(seed, stream, 0, 40, 3, 6 + n_rot), ctx.rng_initial(seed, stream, 0, 40, n_rot, tr_sigma=5.0)
    whole = ctx.rng_perturbation(seed, stream, 0, 40, n_rot, *args)
    parts = [ctx.rng_perturbation(seed, stream, s0, 8, n_rot, *args) for s0 in range(0, 40, 8)]
    again = ctx.rng_perturbation(seed, stream, 0, 40, n_rot, *args)
    other = ctx.rng_perturbation(seed, stream, 0, 40, n_rot, *args, draw=1)
    for k in range(6):
        assert torch.equal(whole[k], torch.cat([q[k] for q in parts])) and torch.equal(whole[k], again[k])
    for k in range(3):      # another draw: other numbers for every sample
        assert float((whole[k] - other[k]).abs().reshape(40, -1).max(dim=1).values.min()) > 0
    # the purposes 0-5 keep their bits: the same calls after the forward draws, and the restatement's torsions
    assert torch.equal(ctx.rng_noise(seed, stream, 0, 40, 3, 6 + n_rot), noise0)
    for a, b in zip(ctx.rng_initial(seed, stream, 0, 40, n_rot, tr_sigma=5.0), init0):
        assert torch.equal(a, b)
    assert np.array_equal(init0[0].cpu().numpy().view(np.int32), pr.initial(seed, stream, 0, 40, n_rot, 5.0)[0].view(np.int32))
    # the forward draws are none of the older ones
    assert not torch.equal(whole.tr_update[:, :3] / tr_sigma, noise0[0, :, :3])


def test_perturbation_refusals(ctx):
    from disco_diffdock_amd import _lib
    L, h = ctx.L, ctx.h
    dev = torch.device('cuda', ctx.device)
    out = torch.full((4096,), 7.0, device=dev)
    row = torch.ones(2000, dtype=torch.float64, device=dev)
    p, r, s = out.data_ptr(), C.c_void_p(row.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    full = dict(tr_update=p, rot_update=p + 64, tor_update=p + 128, tr_score=p + 1024, rot_score=p + 2048, tor_score=p + 3072)
    I32 = (1 << 31) - 1

    def call(sample0=0, B=2, draw=0, n_rot=3, tr_sigma=1.0, tor_sigma=1.0, idx=10, cdf=r, score=r, out=full):
        o = None if out is None else C.byref(_lib.ddk_perturbation(**out))
        return L.ddk_rng_perturbation(h, 1, 2, sample0, B, draw, n_rot, tr_sigma, tor_sigma, idx, cdf, score, o, s)

    without = lambda k: {a: (None if a == k else b) for a, b in full.items()}
    bad = [lambda: call(B=0), lambda: call(sample0=-1), lambda: call(sample0=I32 - 1, B=2), lambda: call(draw=-1), lambda: call(draw=1 << 20),
           lambda: call(n_rot=-1), lambda: call(n_rot=1025), lambda: call(tr_sigma=0.0), lambda: call(tor_sigma=-1.0), lambda: call(tr_sigma=float('nan')),
           lambda: call(idx=-1), lambda: call(idx=5001), lambda: call(cdf=None), lambda: call(score=None), lambda: call(out=None),
           lambda: call(out=without('tr_update')), lambda: call(out=without('rot_update')), lambda: call(out=without('tor_update'))]
    for k, c in enumerate(bad):
        assert c() == -1, k
        assert L.ddk_last_error(h).decode().startswith('ddk_rng_perturbation'), k
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # accepted: the limits themselves, score members left out (then no score row is needed), no torsion arrays with n_rot = 0
    assert call(sample0=I32 - 2, B=2, draw=(1 << 20) - 1) == 0 and call(out=without('rot_score'), score=None) == 0
    assert call(n_rot=0, out=dict(full, tor_update=None, tor_score=None)) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('B', [1, 7])
@pytest.mark.parametrize('n_rot', [0, 5])
def test_score_matching_loss(ctx, n_rot, B):
    rng = np.random.default_rng(100 * B + n_rot)
    f = lambda *shape: rng.normal(0, 2.0, size=shape).astype(np.float32)
    tr_p, rot_p, tor_p, tr_s, rot_s, tor_s = f(B, 3), f(B, 3), f(B, n_rot), f(B, 3), f(B, 3), f(B, n_rot)
    scal = (np.float32(1.3797), np.float32(0.7311), np.float32(2.417))
    d = lambda a: torch.from_numpy(a).cuda()
    got = ctx.score_matching_loss(d(tr_p), d(rot_p), d(tor_p) if n_rot else None, d(tr_s), d(rot_s), d(tor_s) if n_rot else None, *scal)
    again = ctx.score_matching_loss(d(tr_p), d(rot_p), d(tor_p) if n_rot else None, d(tr_s), d(rot_s), d(tor_s) if n_rot else None, *scal)
    want = nr.score_matching_loss(tr_p, rot_p, tor_p if n_rot else None, tr_s, rot_s, tor_s, *scal)
    assert tuple(got.shape) == (B, 6) and torch.equal(got, again)
    g = got.cpu().numpy().astype(np.float64)
    if n_rot == 0:
        assert (g[:, [2, 5]] == 0).all()
    assert (np.abs(g - want) <= 1e-6 * np.abs(want)).all(), (g, want)
    if n_rot:      # tor_pred = NULL: the torsion terms are 0, the others the same bits
        no_tor = ctx.score_matching_loss(d(tr_p), d(rot_p), None, d(tr_s), d(rot_s), d(tor_s), *scal)
        assert bool((no_tor[:, [2, 5]] == 0).all()) and torch.equal(no_tor[:, [0, 1, 3, 4]], got[:, [0, 1, 3, 4]])
    L, h, s = ctx.L, ctx.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = C.c_void_p(got.data_ptr())
    for k, rc in enumerate((L.ddk_score_matching_loss(h, 0, 0, p, p, None, p, p, None, 1.0, 1.0, 1.0, p, s),
                            L.ddk_score_matching_loss(h, 1, 1025, p, p, p, p, p, p, 1.0, 1.0, 1.0, p, s),
                            L.ddk_score_matching_loss(h, 1, 0, None, p, None, p, p, None, 1.0, 1.0, 1.0, p, s),
                            L.ddk_score_matching_loss(h, 1, 0, p, p, None, p, p, None, 1.0, 0.0, 1.0, p, s),
                            L.ddk_score_matching_loss(h, 1, 2, p, p, p, p, p, None, 1.0, 1.0, 1.0, p, s))):
        assert rc == -1, k
        assert L.ddk_last_error(h).decode().startswith('ddk_score_matching_loss'), k


def test_end_to_end_validation_loss(ctx, tables):
    """60 residues, B = 4, t = 0.5, random weights, a deterministic context: the noisy poses against the fp64 oracle pose update fed the device's updates (the trajectory tests' pose
    bar), loss_function on the device's predictions against the same loss on oracle.score_model_ref's predictions (the parity bar), and validation_loss twice"""
    from oracle import score_model_ref as smr, sampler_ref as spr
    from helpers import batch_of, rel_err
    import adversarial_geometry as ag
    from disco_diffdock_amd import synthetic, training
    from disco_diffdock_amd.runtime import Context, Complex
    cfg = smr.ScoreModelConfig(latent_vocab=64)
    P = smr.random_state_dict(cfg, seed=23)
    c = synthetic.make_complex(7, n_res=60)
    B, t, seed = 4, 0.5, 3
    model = Context(device=0, deterministic=1)      # (the default scatter's float atomics move a score by ~1e-7 from run to run: tests/test_gpu_seeded_sampling.py)
    model.load_state_dict(P)
    cx = Complex(model, c, B)
    assert cx.R > 0
    pos, tg = training.noise_complex(model, c, t, B, seed, cx=cx)
    assert tuple(pos.shape) == (B, cx.n_lig, 3) and tuple(tg.tor_score.shape) == (B, cx.R)
    assert (tg.tr_sigma, tg.rot_sigma, tg.tor_sigma) == _sigmas(t)
    pos0 = np.broadcast_to(np.asarray(c['lig_pos'], np.float32), (B, cx.n_lig, 3))
    want = ag.update_ref(c, pos0, tg.tr_update.cpu().numpy(), tg.rot_update.cpu().numpy(), tg.tor_update.cpu().numpy())
    e_pos = rel_err(pos.cpu().numpy().reshape(-1, 3), want.reshape(-1, 3))
    tr, rot, tor = cx.score_forward(pos, t, t, t)
    bt = batch_of(c, B, pos.cpu())
    spr.set_time(bt, t, t, t, B)
    tr_r, rot_r, tor_r = smr.score_model_forward(P, cfg, bt, tables[0], tables[1])
    dev_loss = training.loss_function(tr, rot, tor, tg, model, apply_mean=False)
    ref_loss = training.loss_function(tr_r.cuda(), rot_r.cuda(), tor_r.cuda(), tg, model, apply_mean=False)
    e_loss = max(rel_err(a.cpu(), b.cpu()) for a, b in zip(dev_loss, ref_loss))
    print(f'end to end: poses {e_pos:.2e} (bar {POSE_BAR}), losses {e_loss:.2e} (bar {PARITY_BAR}); per-sample loss {dev_loss[0].cpu().numpy()}')
    assert e_pos < POSE_BAR and e_loss < PARITY_BAR
    # the restatement on the same predictions, and the batch means of apply_mean=True (the torsion term over all torsions of the batch)
    so3_norm, torus_norm2 = tables[0][int(nr.so3_eps_index(tg.rot_sigma))], tables[1][int(nr.torus_sigma_index(tg.tor_sigma))]
    host = nr.score_matching_loss(tr.cpu().numpy(), rot.cpu().numpy(), tor.cpu().numpy(), tg.tr_score.cpu().numpy(), tg.rot_score.cpu().numpy(),
                                  tg.tor_score.cpu().numpy(), tg.tr_sigma, so3_norm, torus_norm2)
    got = torch.stack(dev_loss[1:], dim=1).cpu().numpy().astype(np.float64)
    assert (np.abs(got - host) <= 1e-6 * np.abs(host)).all()
    mean = training.loss_function(tr, rot, tor, tg, model)
    assert tuple(mean[3].shape) == (1,) and mean[1].dim() == 0
    tor_all = ((tor.cpu().numpy().astype(np.float64) - tg.tor_score.cpu().numpy().reshape(-1)) ** 2 / np.float64(np.float32(torus_norm2))).mean()
    assert abs(float(mean[3]) - tor_all) <= 1e-5 * tor_all and abs(float(mean[1]) - host[:, 0].mean()) <= 1e-5 * host[:, 0].mean()
    assert abs(float(mean[0]) - (host[:, 0].mean() + host[:, 1].mean() + tor_all)) <= 1e-5 * float(mean[0])
    a = training.validation_loss(model, [c], t_values=[t], samples_per_complex=B, seed=seed)
    b = training.validation_loss(model, [c], t_values=[t], samples_per_complex=B, seed=seed)
    assert a == b and a['n'] == B and set(a['per_t']) == {t}
    assert abs(a['loss'] - float(dev_loss[0].double().mean())) <= 1e-6 * abs(a['loss'])      # draw 0 of the same seed: the batch above
    assert training.validation_loss(model, [c], t_values=[t], samples_per_complex=B, seed=seed + 1) != a
