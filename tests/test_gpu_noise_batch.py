"""GPU tests of the ragged training batch: ddk_rng_perturbation_batch, ddk_modify_conformer_batch, ddk_score_matching_loss_batch and its backward
(csrc/k_noising.hip, csrc/k_se3.hip) and disco_diffdock_amd.training.noise_batch / loss_function / train_epoch, on the standing batch of
tests/noise_batch_ref.py: four different complexes with 4, 7, 0 and 1 rotatable bonds at the times 0.05, 0.3, 0.6 and 0.95.

The bars are those of the same quantities elsewhere in the suite: the perturbation's updates and scores 1e-5 of each vector's norm
(tests/test_gpu_noising.py::test_perturbation_vs_restatement), the poses 2e-4 of the largest coordinate against the fp64 oracle update
(tests/test_gpu_round3.py's se3_update parity), the loss rows 1e-6 relative (test_score_matching_loss: fp64 inside, one rounding), their fp32 batch means
1e-5 (test_end_to_end_validation_loss), a gradient element 1e-6 relative (fp64 inside, one rounding).  Everything that is promised bit for bit is compared
bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import noise_batch_ref as nb
import noising_ref as nr
import philox_ref as pr

pytestmark = pytest.mark.gpu

SEED, DRAW = 29, 2
SAMPLES = (0, 3, 1, 2)
POSE_BAR = 2e-4


def _bits(t):
    return t.detach().contiguous().float().view(torch.int32)


@pytest.fixture(scope='module')
def ctx():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


@pytest.fixture(scope='module')
def standing(ctx):
    """the standing batch, its per-graph tables and ONE noise_batch of it, computed once and left unchanged"""
    from disco_diffdock_amd import training
    cs = nb.standing_batch()
    rotors = nb.rotor_counts(cs)
    assert rotors == [4, 7, 0, 1] and [len(c['lig_pos']) for c in cs] == [16, 19, 16, 20]
    sig = np.asarray([training._sigmas(ctx, t) for t in nb.TIMES], np.float32)
    eps_idx = [int(nr.so3_eps_index(training._sigmas(ctx, t)[1])) for t in nb.TIMES]
    tor_idx = [int(nr.torus_sigma_index(training._sigmas(ctx, t)[2])) for t in nb.TIMES]
    data, tg = training.noise_batch(ctx, cs, nb.TIMES, SEED, draw=DRAW, samples=SAMPLES)
    return dict(cs=cs, rotors=rotors, tor_ptr=nb.prefix(rotors), node_ptr=nb.prefix([len(c['lig_pos']) for c in cs]), sig=sig, eps_idx=eps_idx, tor_idx=tor_idx,
                streams=[pr.fnv1a64(c['name']) for c in cs], data=data, tg=tg)


def _vec_err(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    if want.size == 0:
        return 0.0
    n = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / n) if n > 0 else float(np.abs(got).max())


# ---- 1. draws and targets ----------------------------------------------------------------------------------------------------------------------------------
def test_perturbation_batch_against_the_restatement_and_the_single_call(ctx, standing):
    s = standing
    G, tp = 4, s['tor_ptr']
    cdf, score = ctx.so3_table()
    assert tuple(cdf.shape) == tuple(score.shape) == (1000, 2000) and ctx.so3_table()[0] is cdf      # kept on the context
    p = ctx.rng_perturbation_batch(SEED, s['streams'], SAMPLES, tp, s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], s['eps_idx'], cdf, score, draw=DRAW)
    assert tuple(p.tr_update.shape) == (G, 3) and tuple(p.tor_update.shape) == tuple(p.tor_score.shape) == (int(tp[-1]),)
    want = nb.perturbation_batch(SEED, s['streams'], SAMPLES, DRAW, s['rotors'], s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], s['eps_idx'])
    host = {k: getattr(p, k).cpu().numpy() for k in want}
    assert all(np.isfinite(v).all() for v in host.values())
    for g in range(G):
        a, b = tp[g], tp[g + 1]
        errs = {k: _vec_err(host[k][g], want[k][g]) for k in ('tr_update', 'rot_update', 'tr_score', 'rot_score')}
        errs['tor_update'] = _vec_err(host['tor_update'][a:b], want['tor_update'][a:b])
        # tor_score is the torus arithmetic on the device's own fp32 tor_update (the quantisation to the grid is a step function of it)
        errs['tor_score'] = _vec_err(host['tor_score'][a:b], nr.torus_score(host['tor_update'][a:b], s['tor_idx'][g]))
        print(f'graph {g} (R = {s["rotors"][g]}, t = {nb.TIMES[g]}): ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        assert max(errs.values()) <= 1e-5, (g, errs)
        # bit for bit the single call with B = 1 and the graph's own scalars and rows
        one = ctx.rng_perturbation(SEED, s['streams'][g], SAMPLES[g], 1, s['rotors'][g], float(s['sig'][g, 0]), float(s['sig'][g, 2]), s['tor_idx'][g],
                                   cdf[s['eps_idx'][g]], score[s['eps_idx'][g]], draw=DRAW)
        for k in ('tr_update', 'rot_update', 'tr_score', 'rot_score'):
            assert torch.equal(_bits(getattr(p, k)[g]), _bits(getattr(one, k)[0])), (g, k)
        for k in ('tor_update', 'tor_score'):
            assert torch.equal(_bits(getattr(p, k)[a:b]), _bits(getattr(one, k).reshape(-1))), (g, k)
    # the caller's rows in any order, and the targets noise_batch hands on
    rows_c, rows_s, _ = ctx.so3_rows(s['eps_idx'][::-1], exp_score_norm=False)
    q = ctx.rng_perturbation_batch(SEED, s['streams'], SAMPLES, tp, s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], [3, 2, 1, 0], rows_c, rows_s, draw=DRAW)
    for k in want:
        assert torch.equal(_bits(getattr(q, k)), _bits(getattr(p, k))), k
        assert torch.equal(_bits(getattr(s['tg'], k)), _bits(getattr(p, k))), k
    no_scores = ctx.rng_perturbation_batch(SEED, s['streams'], SAMPLES, tp, s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], s['eps_idx'], cdf, None, draw=DRAW,
                                           scores=False)
    assert no_scores.tr_score is None and torch.equal(_bits(no_scores.tor_update), _bits(p.tor_update))


# ---- 2. poses --------------------------------------------------------------------------------------------------------------------------------------------------
def test_poses_against_noise_complex_and_the_fp64_update(ctx, standing):
    from disco_diffdock_amd import training
    from oracle import sampler_ref as spr
    s, tg = standing, standing['tg']
    pos = s['data']['ligand'].pos
    assert pos.is_cuda and tuple(pos.shape) == (int(s['node_ptr'][-1]), 3)
    assert torch.equal(s['data'].complex_t['tr'].cpu(), torch.tensor(nb.TIMES)) and s['data'].num_graphs == 4
    assert torch.equal(tg.tor_ptr.cpu(), torch.from_numpy(s['tor_ptr'])) and tg.rotors == tuple(s['rotors'])
    ref = nb.modify_conformer_batch(s['cs'], tg.tr_update.cpu().numpy(), tg.rot_update.cpu().numpy(), tg.tor_update.cpu().numpy(), s['tor_ptr'])
    for g, c in enumerate(s['cs']):
        mine = pos[s['node_ptr'][g]:s['node_ptr'][g + 1]]
        alone, one = training.noise_complex(ctx, c, nb.TIMES[g], 1, SEED, draw=DRAW, sample_offset=SAMPLES[g])
        assert torch.equal(_bits(mine), _bits(alone[0])), g
        for k in ('tr_score', 'rot_score', 'tr_update', 'rot_update'):
            assert torch.equal(_bits(getattr(tg, k)[g]), _bits(getattr(one, k)[0])), (g, k)
        assert torch.equal(_bits(tg.tor_score[s['tor_ptr'][g]:s['tor_ptr'][g + 1]]), _bits(one.tor_score.reshape(-1))), g
        err = float(np.abs(mine.cpu().numpy() - ref[g]).max() / np.abs(ref[g]).max())
        print(f'graph {g}: pose against the fp64 update {err:.2e} (bar {POSE_BAR})')
        assert err < POSE_BAR, (g, err)
    # the ligand without rotatable bonds gets the rigid move: (pos - centroid) R^T + tr + centroid
    g = s['rotors'].index(0)
    p0 = np.asarray(s['cs'][g]['lig_pos'], np.float64)
    Rm = spr.axis_angle_to_matrix(tg.rot_update[g:g + 1].cpu().double())[0].numpy()
    want = (p0 - p0.mean(0)) @ Rm.T + tg.tr_update[g].cpu().double().numpy() + p0.mean(0)
    got = pos[s['node_ptr'][g]:s['node_ptr'][g + 1]].cpu().numpy()
    assert np.abs(got - want).max() < POSE_BAR * np.abs(want).max()


# ---- 3. composition independence ---------------------------------------------------------------------------------------------------------------------------------
def _graph_bits(data, tg, g, node_ptr, tor_ptr):
    a, b = node_ptr[g], node_ptr[g + 1]
    out = [_bits(data['ligand'].pos[a:b])] + [_bits(getattr(tg, k)[g]) for k in ('tr_score', 'rot_score', 'tr_update', 'rot_update', 'tr_sigma', 'so3_score_norm')]
    return out + [_bits(getattr(tg, k)[tor_ptr[g]:tor_ptr[g + 1]]) for k in ('tor_score', 'tor_update')]


def test_a_graph_does_not_depend_on_the_rest_of_the_batch(ctx, standing):
    from disco_diffdock_amd import training
    s = standing
    cs, G = s['cs'], 4
    want = [_graph_bits(s['data'], s['tg'], g, s['node_ptr'], s['tor_ptr']) for g in range(G)]
    rev = training.noise_batch(ctx, cs[::-1], nb.TIMES[::-1], SEED, draw=DRAW, samples=SAMPLES[::-1])
    node_rev, tor_rev = nb.prefix([len(c['lig_pos']) for c in cs[::-1]]), nb.prefix(s['rotors'][::-1])
    for g in range(G):
        alone = training.noise_batch(ctx, [cs[g]], [nb.TIMES[g]], SEED, draw=DRAW, samples=[SAMPLES[g]])
        forms = {'alone': _graph_bits(*alone, 0, nb.prefix([len(cs[g]['lig_pos'])]), nb.prefix([s['rotors'][g]])),
                 'reversed': _graph_bits(*rev, G - 1 - g, node_rev, tor_rev)}
        for name, got in forms.items():
            assert all(torch.equal(a, b) for a, b in zip(got, want[g])), (g, name)
    # twice in one batch with samples (SAMPLES[g], SAMPLES[g] + 1): the first copy is the graph of the standing batch, the second differs from it
    for g in (0, 2):
        n, r = len(cs[g]['lig_pos']), s['rotors'][g]
        twice = training.noise_batch(ctx, [cs[g], cs[1], cs[g]], [nb.TIMES[g], nb.TIMES[1], nb.TIMES[g]], SEED, draw=DRAW,
                                     samples=[SAMPLES[g], SAMPLES[1], SAMPLES[g] + 1])
        node, tor = nb.prefix([n, len(cs[1]['lig_pos']), n]), nb.prefix([r, s['rotors'][1], r])
        first, second = _graph_bits(*twice, 0, node, tor), _graph_bits(*twice, 2, node, tor)
        assert all(torch.equal(a, b) for a, b in zip(first, want[g])), g
        assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1]) and torch.equal(first[5], second[5])
    other_draw = training.noise_batch(ctx, cs, nb.TIMES, SEED, draw=DRAW + 1, samples=SAMPLES)
    assert not torch.equal(_bits(other_draw[0]['ligand'].pos), _bits(s['data']['ligand'].pos))


# ---- 4. loss -----------------------------------------------------------------------------------------------------------------------------------------------------
def _predictions(tg, seed=5, grad=False):
    gen = torch.Generator().manual_seed(seed)
    G, T = tg.tr_score.shape[0], sum(tg.rotors)
    out = [(torch.randn(*shape, generator=gen) * 2).cuda().requires_grad_(grad) for shape in ((G, 3), (G, 3), (T,))]
    return out


def _host_targets(tg):
    n = lambda v: None if v is None else v.detach().cpu().numpy()
    return dict(tr_score=n(tg.tr_score), rot_score=n(tg.rot_score), tor_score=n(tg.tor_score), tr_sigma=n(tg.tr_sigma), so3_norm=n(tg.so3_score_norm),
                torus_norm2=n(tg.torus_score_norm2), tor_ptr=n(tg.tor_ptr))


def test_loss_rows_and_means(ctx, standing, tables):
    from disco_diffdock_amd import training
    tg = standing['tg']
    h = _host_targets(tg)
    # the per-graph norms noise_batch looked up: the tables at each graph's own sigma index
    assert np.array_equal(h['so3_norm'], tables[0][standing['eps_idx']].astype(np.float32))
    assert np.array_equal(h['torus_norm2'], tables[1][standing['tor_idx']].astype(np.float32))
    assert np.array_equal(h['tr_sigma'], standing['sig'][:, 0])
    tr, rot, tor = _predictions(tg)
    args = (tr.cpu().numpy(), rot.cpu().numpy(), tor.cpu().numpy(), h['tr_score'], h['rot_score'], h['tor_score'], h['tr_sigma'], h['so3_norm'], h['torus_norm2'],
            h['tor_ptr'])
    rows = ctx.score_matching_loss_batch(tr, rot, tor, tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_sigma, tg.so3_score_norm, tg.torus_score_norm2, tg.tor_ptr,
                                         sum(tg.rotors))
    want = nb.loss_batch(*args)
    got = rows.cpu().numpy().astype(np.float64)
    print('rows: max rel err', float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max()))
    assert got.shape == (4, 6) and (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), (got, want)
    assert (got[standing['rotors'].index(0), [2, 5]] == 0).all()
    # row g is bit for bit the single call with B = 1, n_rot = R_g and g's scalars
    for g in range(4):
        a, b = h['tor_ptr'][g], h['tor_ptr'][g + 1]
        one = ctx.score_matching_loss(tr[g:g + 1], rot[g:g + 1], tor[a:b] if b > a else None, tg.tr_score[g:g + 1], tg.rot_score[g:g + 1],
                                      tg.tor_score[a:b] if b > a else None, float(h['tr_sigma'][g]), float(h['so3_norm'][g]), float(h['torus_norm2'][g]))
        assert torch.equal(_bits(one[0]), _bits(rows[g])), g
    # both apply_mean forms against the transcription of the reference
    for apply_mean, bar in ((False, 2e-6), (True, 1e-5)):      # [G]: a row (1e-6) and one fp32 sum of three; means: fp32 sums over the graphs on top
        out = training.loss_function(tr, rot, tor, tg, ctx, apply_mean=apply_mean, tr_weight=0.5, rot_weight=2, tor_weight=3)
        ref = nb.reference_loss_function(*args, apply_mean=apply_mean, tr_weight=0.5, rot_weight=2, tor_weight=3)
        assert [tuple(v.shape) for v in out] == [tuple(v.shape) for v in ref]
        for k, (a, w) in enumerate(zip(out, ref)):
            assert (np.abs(a.cpu().numpy() - w.numpy()) <= bar * np.abs(w.numpy())).all(), (apply_mean, k, a, w)


def test_loss_equals_the_rectangular_path_on_a_rectangular_batch(ctx, standing):
    """three samples of ONE complex at ONE time: the ragged path and loss_function(Targets) give the same bits in every per-sample column"""
    from disco_diffdock_amd import training
    c, t, B = standing['cs'][1], 0.5, 3
    _, tg_b = training.noise_batch(ctx, [c] * B, [t] * B, SEED, draw=DRAW, samples=range(B))
    _, tg_s = training.noise_complex(ctx, c, t, B, SEED, draw=DRAW)
    assert torch.equal(_bits(tg_b.tor_score), _bits(tg_s.tor_score.reshape(-1))) and torch.equal(_bits(tg_b.rot_score), _bits(tg_s.rot_score))
    tr, rot, tor = _predictions(tg_b)
    ragged = training.loss_function(tr, rot, tor, tg_b, ctx, apply_mean=False)
    rect = training.loss_function(tr, rot, tor, tg_s, ctx, apply_mean=False)
    for k, (a, b) in enumerate(zip(ragged, rect)):
        assert tuple(a.shape) == (B,) and torch.equal(_bits(a), _bits(b)), k


def test_loss_backward_against_fp64_autograd(ctx, standing):
    from disco_diffdock_amd import training
    tg = standing['tg']
    h = _host_targets(tg)
    w = torch.randn(4, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    ref_p = [p.detach().cpu().double().requires_grad_() for p in _predictions(tg)]
    cols = nb.loss_batch_torch(*ref_p, *[torch.from_numpy(h[k].astype(np.float64)) for k in ('tr_score', 'rot_score', 'tor_score')], h['tr_sigma'], h['so3_norm'],
                               h['torus_norm2'], h['tor_ptr'])
    (cols * w).sum().backward()
    dev_p = _predictions(tg, grad=True)
    out = training.loss_function(*dev_p, tg, ctx, apply_mean=False)
    (torch.stack(out[1:4], dim=1).double() * w.cuda()).sum().backward()
    for name, a, b in zip(('tr', 'rot', 'tor'), dev_p, ref_p):
        got, want = a.grad.cpu().numpy().astype(np.float64), b.grad.numpy()
        # w reaches the kernel rounded to fp32 (6e-8), the kernel rounds once more: 1e-6 of each element with room to spare
        print(f'grad {name}: max rel err {float((np.abs(got - want) / np.abs(want)).max()):.2e}')
        assert got.shape == want.shape and (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), name
    # only what asks for a gradient gets one; the batch mean is differentiable too and runs the same kernel
    only = _predictions(tg)
    only[0].requires_grad_()
    training.loss_function(*only, tg, ctx)[0].sum().backward()
    assert only[0].grad is not None and only[1].grad is None and only[2].grad is None
    again = _predictions(tg, grad=True)
    out2 = training.loss_function(*again, tg, ctx, apply_mean=False)
    (torch.stack(out2[1:4], dim=1).double() * w.cuda()).sum().backward()
    assert all(torch.equal(_bits(a.grad), _bits(b.grad)) for a, b in zip(again, dev_p))


def test_loss_without_torsions(ctx, standing):
    """T = 0 and no_torsion: zeros of the reference's shapes, with and without apply_mean, and gradients for the two predictions that remain"""
    from disco_diffdock_amd import training
    from disco_diffdock_amd.runtime import Context
    rigid = standing['cs'][standing['rotors'].index(0)]
    no_torsion = Context(device=0, no_torsion=1)
    cases = {'T = 0': (ctx, training.noise_batch(ctx, [rigid, rigid], [0.3, 0.6], SEED, samples=[0, 1])),
             'no_torsion': (no_torsion, training.noise_batch(no_torsion, standing['cs'], nb.TIMES, SEED, draw=DRAW, samples=SAMPLES))}
    for name, (model, (data, tg)) in cases.items():
        G = tg.tr_score.shape[0]
        assert sum(tg.rotors) == 0 and tg.tor_update.numel() == 0, name
        assert (tg.tor_score is None) == (name == 'no_torsion')
        tr, rot, _ = _predictions(tg, grad=True)
        tor = torch.zeros(0, device='cuda') if name == 'T = 0' else None
        per = training.loss_function(tr, rot, tor, tg, model, apply_mean=False)
        mean = training.loss_function(tr, rot, tor, tg, model)
        assert tuple(per[3].shape) == tuple(per[6].shape) == (G,) and not bool(per[3].any()) and not bool(per[6].any()), name
        assert tuple(mean[3].shape) == tuple(mean[6].shape) == (1,) and float(mean[3]) == 0 and float(mean[6]) == 0, name
        assert torch.equal(per[0], per[1] + per[2])
        mean[0].sum().backward()
        assert bool(torch.isfinite(tr.grad).all()) and bool((rot.grad != 0).any())
    # the rigid move of the no_torsion batch is the standing batch's rigid part: same translations and rotations, no torsion step
    assert torch.equal(_bits(cases['no_torsion'][1][1].tr_update), _bits(standing['tg'].tr_update))
    g = standing['rotors'].index(0)
    a, b = standing['node_ptr'][g], standing['node_ptr'][g + 1]
    assert torch.equal(_bits(cases['no_torsion'][1][0]['ligand'].pos[a:b]), _bits(standing['data']['ligand'].pos[a:b]))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def _big_ligand(c, n_lig=None, n_rot=None):
    c = dict(c)
    if n_lig is not None:
        c.update(lig_pos=np.zeros((n_lig, 3), np.float32) + np.arange(n_lig, dtype=np.float32)[:, None], edge_mask=np.zeros(0, bool),
                 mask_rotate=np.zeros((0, n_lig), bool), bond_index=np.zeros((2, 0), np.int64))
    if n_rot is not None:
        n = len(c['lig_pos'])
        c.update(edge_mask=np.ones(n_rot, bool), mask_rotate=np.zeros((n_rot, n), bool), bond_index=np.stack([np.zeros(n_rot, np.int64), np.ones(n_rot, np.int64)]))
    return c


def test_refusals_enqueue_nothing(ctx, standing):
    from disco_diffdock_amd import _lib, training
    s = standing
    cs = s['cs']
    nameless = {k: v for k, v in cs[0].items() if k != 'name'}
    for bad, match in ((lambda: training.noise_batch(ctx, cs, (0.1, 0.2, 1.5, 0.3), SEED), r'every t must be in \[0, 1\]'),
                       (lambda: training.noise_batch(ctx, cs, (0.1, 0.2, float('nan'), 0.3), SEED), r'every t must be'),
                       (lambda: training.noise_batch(ctx, cs, (0.1, 0.2), SEED), r't must hold one time per complex'),
                       (lambda: training.noise_batch(ctx, [cs[0], nameless], (0.1, 0.2), SEED), r'with a name'),
                       (lambda: training.noise_batch(ctx, [cs[0], _big_ligand(cs[1], n_lig=257)], (0.1, 0.2), SEED), r'n_lig of complex 1 .* \[1, 256\], got 257'),
                       (lambda: training.noise_batch(ctx, [_big_ligand(cs[1], n_rot=1025)], (0.1,), SEED), r'R_g of complex 0 .* \[0, 1024\], got 1025'),
                       (lambda: training.noise_batch(ctx, cs, nb.TIMES, SEED, samples=(0, 1, -1, 2)), r'samples')):
        with pytest.raises(ValueError, match=match):
            bad()
    dev = torch.device('cuda', ctx.device)
    tg, N, T = s['tg'], int(s['node_ptr'][-1]), int(s['tor_ptr'][-1])
    pos0 = torch.from_numpy(np.concatenate([np.asarray(c['lig_pos'], np.float32) for c in cs])).to(dev)
    bonds = np.concatenate([nb.rot_bonds(c) for c in cs]).astype(np.int32)
    masks = np.concatenate([np.asarray(c['mask_rotate'], np.uint8).reshape(-1) for c in cs])
    mask_ptr = nb.prefix([r * len(c['lig_pos']) for r, c in zip(s['rotors'], cs)])
    good = ctx.modify_conformer_batch(pos0, s['node_ptr'], bonds, masks, mask_ptr, s['tor_ptr'], tg.tr_update, tg.rot_update, tg.tor_update)
    assert torch.equal(_bits(good), _bits(s['data']['ligand'].pos))
    # prefix tables given on the host: nodes that are not grouped by graph, a tor_ptr that decreases
    with pytest.raises(ValueError, match=r'node_ptr .* grouped by graph'):
        ctx.modify_conformer_batch(pos0, [0, 35, 16, 51, N], bonds, masks, mask_ptr, s['tor_ptr'], tg.tr_update, tg.rot_update, tg.tor_update)
    with pytest.raises(ValueError, match=r'tor_ptr must be a non-decreasing prefix'):
        ctx.modify_conformer_batch(pos0, s['node_ptr'], bonds, masks, mask_ptr, [0, 11, 4, 11, T], tg.tr_update, tg.rot_update, tg.tor_update)
    with pytest.raises(ValueError, match=r'tor_ptr must be a non-decreasing prefix'):
        ctx.score_matching_loss_batch(tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_sigma, tg.so3_score_norm,
                                      tg.torus_score_norm2, [0, 11, 4, 11, T], T)
    with pytest.raises(ValueError, match=r'tor_ptr must be a non-decreasing prefix'):
        ctx.rng_perturbation_batch(SEED, s['streams'], SAMPLES, [0, 11, 4, 11, T], s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], s['eps_idx'], *ctx.so3_table())
    # the C entry points: a NULL required output or argument, a broken limit: -1, a text that names it, nothing written
    L, h, st = ctx.L, ctx.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    guard = torch.full((4096,), 7.0, device=dev)
    iguard = torch.full((64,), 7, dtype=torch.int32, device=dev)
    p, ip = C.c_void_p(guard.data_ptr()), C.c_void_p(iguard.data_ptr())
    d = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)
    node, tor_p, mask_p = d(s['node_ptr'], torch.int32), d(s['tor_ptr'], torch.int32), d(mask_ptr, torch.int32)
    bonds_d, masks_d = d(bonds, torch.int32), d(masks, torch.uint8)
    q = lambda t: C.c_void_p(t.data_ptr())

    def conformer(G=4, N=N, T=T, pos=q(pos0), out=p, status=ip, tor=q(tg.tor_update), tor_ptr=q(tor_p)):
        return L.ddk_modify_conformer_batch(h, G, N, pos, q(node), T, q(bonds_d), q(masks_d), q(mask_p), masks_d.numel(), tor_ptr, q(tg.tr_update),
                                            q(tg.rot_update), tor, out, status, st)

    def loss(G=4, T=T, out=p, tor_ptr=q(tor_p), sigma=q(tg.tr_sigma)):
        return L.ddk_score_matching_loss_batch(h, G, tor_ptr, T, q(tg.tr_score), q(tg.rot_score), q(tg.tor_score), q(tg.tr_score), q(tg.rot_score), q(tg.tor_score),
                                               sigma, q(tg.so3_score_norm), q(tg.torus_score_norm2), out, st)

    def loss_bwd(grad=p, G=4):
        return L.ddk_score_matching_loss_batch_backward(h, G, q(tor_p), T, grad, q(tg.tr_score), q(tg.rot_score), q(tg.tor_score), q(tg.tr_score), q(tg.rot_score),
                                                        q(tg.tor_score), q(tg.tr_sigma), q(tg.so3_score_norm), q(tg.torus_score_norm2), p, p, p, st)

    cdf, score = ctx.so3_table()
    streams_d, samples_d = d(np.asarray(s['streams'], np.uint64).view(np.int64), torch.int64), d(SAMPLES, torch.int32)
    eps_d, tidx_d, sig_d = d(s['eps_idx'], torch.int32), d(s['tor_idx'], torch.int32), d(s['sig'], torch.float32).t().contiguous()
    full = dict(tr_update=guard.data_ptr(), rot_update=guard.data_ptr() + 256, tor_update=guard.data_ptr() + 512, tr_score=guard.data_ptr() + 1024,
                rot_score=guard.data_ptr() + 2048, tor_score=guard.data_ptr() + 3072)

    def perturb(G=4, T=T, draw=0, n_rows=1000, out=full, cdf_rows=q(cdf), tor_ptr=q(tor_p)):
        o = None if out is None else C.byref(_lib.ddk_perturbation(**out))
        return L.ddk_rng_perturbation_batch(h, SEED, G, q(streams_d), q(samples_d), tor_ptr, T, draw, q(sig_d[0]), q(sig_d[2]), q(tidx_d), q(eps_d), n_rows,
                                            cdf_rows, q(score), o, st)

    bad = [(lambda: conformer(out=None), 'ddk_modify_conformer_batch', 'pos_out'), (lambda: conformer(status=None), 'ddk_modify_conformer_batch', 'status_out'),
           (lambda: conformer(pos=None), 'ddk_modify_conformer_batch', 'pos'), (lambda: conformer(G=0), 'ddk_modify_conformer_batch', 'G must'),
           (lambda: conformer(N=4 * 256 + 1), 'ddk_modify_conformer_batch', 'N must'), (lambda: conformer(T=4 * 1024 + 1), 'ddk_modify_conformer_batch', 'T must'),
           (lambda: conformer(tor_ptr=None), 'ddk_modify_conformer_batch', 'tor_ptr'),
           (lambda: loss(out=None), 'ddk_score_matching_loss_batch', 'out'), (lambda: loss(G=0), 'ddk_score_matching_loss_batch', 'G must'),
           (lambda: loss(tor_ptr=None), 'ddk_score_matching_loss_batch', 'tor_ptr'), (lambda: loss(sigma=None), 'ddk_score_matching_loss_batch', 'tr_sigma'),
           (lambda: loss(T=-1), 'ddk_score_matching_loss_batch', 'T must'),
           (lambda: loss_bwd(grad=None), 'ddk_score_matching_loss_batch_backward', 'grad'), (lambda: loss_bwd(G=65537), 'ddk_score_matching_loss_batch_backward', 'G must'),
           (lambda: perturb(out=None), 'ddk_rng_perturbation_batch', 'null output'),
           (lambda: perturb(out=dict(full, tr_update=None)), 'ddk_rng_perturbation_batch', 'null output'),
           (lambda: perturb(out=dict(full, tor_update=None)), 'ddk_rng_perturbation_batch', 'tor_update'),
           (lambda: perturb(cdf_rows=None), 'ddk_rng_perturbation_batch', 'IGSO'), (lambda: perturb(tor_ptr=None), 'ddk_rng_perturbation_batch', 'tor_ptr'),
           (lambda: perturb(draw=1 << 20), 'ddk_rng_perturbation_batch', 'draw'), (lambda: perturb(n_rows=0), 'ddk_rng_perturbation_batch', 'n_rows'),
           (lambda: perturb(G=0), 'ddk_rng_perturbation_batch', 'G must')]
    for k, (call, who, word) in enumerate(bad):
        assert call() == -1, k
        text = L.ddk_last_error(h).decode()
        assert text.startswith(who + ':') and word in text, (k, text)
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all()) and bool((iguard == 7).all())


def test_broken_tables_on_the_device_give_a_status_not_a_fault(ctx, standing):
    """what only the device can see, a table entry inside a device array, is found there before it is used as an address: the graph gets its status and is
    left unwritten, the other graphs get their poses.  Every index below stays inside the arrays that are passed: the test provokes nothing."""
    s, tg = standing, standing['tg']
    cs = s['cs']
    dev = torch.device('cuda', ctx.device)
    N, T = int(s['node_ptr'][-1]), int(s['tor_ptr'][-1])
    pos0 = np.concatenate([np.asarray(c['lig_pos'], np.float32) for c in cs])
    bonds = np.concatenate([nb.rot_bonds(c) for c in cs]).astype(np.int32)
    masks = np.concatenate([np.asarray(c['mask_rotate'], np.uint8).reshape(-1) for c in cs])
    mask_ptr = nb.prefix([r * len(c['lig_pos']) for r, c in zip(s['rotors'], cs)])
    d = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)

    def run(pos=pos0, node_ptr=s['node_ptr'], bonds=bonds, tor_ptr=s['tor_ptr']):
        out, status = ctx.modify_conformer_batch(d(pos, torch.float32), d(node_ptr, torch.int32), d(bonds, torch.int32), d(masks, torch.uint8),
                                                 d(mask_ptr, torch.int32), d(tor_ptr, torch.int32), tg.tr_update, tg.rot_update, tg.tor_update, T=T,
                                                 return_status=True)
        return out, status.cpu().tolist()

    good, status = run()
    assert status == [0, 0, 0, 0] and torch.equal(_bits(good), _bits(s['data']['ligand'].pos))
    node = s['node_ptr']
    same = lambda out, graphs: all(torch.equal(_bits(out[node[g]:node[g + 1]]), _bits(good[node[g]:node[g + 1]])) for g in graphs)
    b = bonds.copy(); b[5, 0] = len(cs[1]['lig_pos'])      # graph 1: a bond index one past its last atom
    out, status = run(bonds=b)
    assert status == [0, 2, 0, 0] and same(out, (0, 2, 3))
    b = bonds.copy(); b[0, 1] = -1
    assert run(bonds=b)[1] == [2, 0, 0, 0]
    b = bonds.copy(); b[T - 1, 1] = b[T - 1, 0]            # u == v
    assert run(bonds=b)[1] == [0, 0, 0, 2]
    p = pos0.copy(); p[node[2] + 3, 1] = np.inf            # the rigid ligand: a coordinate that is not finite
    out, status = run(pos=p)
    assert status == [0, 0, 3, 0] and same(out, (0, 1, 3))
    # nodes not grouped by graph, in a device table: graph 0's 35 atoms do not fit its mask block, graph 1 has a negative count; graphs 2 and 3 are ranges
    # of the array with matching blocks, which is all the kernel can know
    out, status = run(node_ptr=[0, 35, 16, 51, N])
    assert status == [4, 4, 0, 0] and same(out, (3,))
    # a tor_ptr that decreases, in a device table: only graph 3's entries still agree with its mask block
    out, status = run(tor_ptr=[0, 11, 4, 11, T])
    assert status == [4, 4, 4, 0] and same(out, (3,))
    # the other two kernels mark such a graph with NaN and touch nothing else
    rows = ctx.score_matching_loss_batch(tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_score, tg.rot_score, tg.tor_score, tg.tr_sigma, tg.so3_score_norm,
                                         tg.torus_score_norm2, d([0, 11, 4, 11, T], torch.int32), T).cpu().numpy()
    assert np.isnan(rows[1]).all() and np.isfinite(rows[[0, 2, 3]]).all()      # (0, 11), (4, 11) and (11, 12) are ranges of [0, T]; (11, 4) is not
    cdf, score = ctx.so3_table()
    pert = ctx.rng_perturbation_batch(SEED, s['streams'], SAMPLES, d([0, 11, 4, 11, T], torch.int32), s['sig'][:, 0], s['sig'][:, 2], s['tor_idx'], s['eps_idx'],
                                      cdf, score, draw=DRAW, T=T)
    assert bool(torch.isnan(pert.tr_update[1]).all()) and bool(torch.isnan(pert.rot_update[1]).all())
    assert all(torch.equal(_bits(pert.tr_update[g]), _bits(tg.tr_update[g])) for g in (0, 2, 3))


# ---- 6. a real training step -------------------------------------------------------------------------------------------------------------------------------------
def _model(dev, P, **kw):
    from disco_diffdock_amd.train_model import TrainableScoreModel
    from test_gpu_train_model import MODEL
    model = TrainableScoreModel(**dict(MODEL, **kw))
    model.load_state_dict({k: v for k, v in P.items() if k in model.state_dict()}, strict=True)
    return model.to(dev)


@pytest.fixture(scope='module')
def weights():
    from oracle import score_model_ref as smr
    return smr.random_state_dict(smr.ScoreModelConfig(), seed=6)


def test_training_step_on_the_ragged_batch_reaches_every_parameter(ctx, standing, weights):
    from disco_diffdock_amd import training
    dev = torch.device('cuda', ctx.device)
    torch.manual_seed(4321)
    model = _model(dev, weights, batch_norm=True, dropout=0.1).train()
    data, tg = training.noise_batch(model, standing['cs'], nb.TIMES, SEED, draw=DRAW, samples=SAMPLES)
    assert torch.equal(_bits(data['ligand'].pos), _bits(standing['data']['ligand'].pos))      # the model's context is the shared one
    tr, rot, tor = model(data, seed=77)
    assert tuple(tr.shape) == tuple(rot.shape) == (4, 3) and tuple(tor.shape) == (sum(standing['rotors']),)
    loss = training.loss_function(tr, rot, tor, tg, model)[0]
    assert tuple(loss.shape) == (1,) and bool(torch.isfinite(loss).all())
    loss.backward()
    for k, p in model.named_parameters():
        if p.numel():
            assert p.grad is not None, k
            assert bool(torch.isfinite(p.grad).all()), k
            assert bool((p.grad != 0).any()), k


def test_train_epoch_is_a_pure_function_of_state_and_seed(ctx, standing, weights):
    from disco_diffdock_amd import synthetic, training
    dev = torch.device('cuda', ctx.device)
    complexes = standing['cs'] + [synthetic.make_complex(seed, n_res=n_res, n_lig=12) for seed, n_res in ((71, 28), (67, 24), (3, 23))]
    complexes.append(nb.with_rotors(synthetic.make_complex(9, n_res=26, n_lig=12), 2))
    assert len(complexes) == 8 and len({c['name'] for c in complexes}) == 8

    def run(seed):
        model = _model(dev, weights, batch_norm=True, dropout=0.1)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        ema = training.ExponentialMovingAverage(model.parameters(), 0.999)
        summary = training.train_epoch(model, complexes, opt, 4, seed, 0, ema=ema)
        return summary, {k: v.detach().clone() for k, v in model.state_dict().items()}, [v.clone() for v in ema.shadow_params], ema.num_updates

    (sum_a, state_a, ema_a, n_a), (sum_b, state_b, ema_b, _), (sum_c, state_c, _, _) = run(11), run(11), run(12)
    assert set(sum_a) == set(training.TRAIN_METERS) and all(np.isfinite(v) for v in sum_a.values()) and n_a == 2
    assert sum_a == sum_b
    assert all(torch.equal(_bits(state_a[k].float()), _bits(state_b[k].float())) for k in state_a)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ema_a, ema_b))
    assert sum_c != sum_a and any(not torch.equal(state_a[k], state_c[k]) for k in state_a)
    fresh = _model(dev, weights, batch_norm=True, dropout=0.1)
    moved = [k for k, v in fresh.state_dict().items() if v.numel() and not torch.equal(v, state_a[k])]
    assert len(moved) >= len([1 for _, p in fresh.named_parameters() if p.numel()])      # the steps moved every parameter
    # a last batch of one graph is skipped, as in the reference: five complexes in batches of four run one step
    model = _model(dev, weights, batch_norm=True, dropout=0.1)
    ema = training.ExponentialMovingAverage(model.parameters(), 0.999)
    training.train_epoch(model, complexes[:5], torch.optim.Adam(model.parameters(), lr=1e-3), 4, 11, 0, ema=ema)
    assert ema.num_updates == 1


# ---- 7. it learns --------------------------------------------------------------------------------------------------------------------------------------------------
def test_thirty_adam_steps_on_one_noised_batch_lower_the_loss(ctx, standing, weights):
    """30 Adam steps (lr 1e-3, dropout 0) on ONE fixed noised batch, the standing one: the loss of the last step is below the loss of the first, and the
    run is deterministic"""
    from disco_diffdock_amd import training
    from test_gpu_round3 import _record_drift
    dev = torch.device('cuda', ctx.device)

    def run():
        model = _model(dev, weights, batch_norm=True, dropout=0.0).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        data, tg = training.noise_batch(model, standing['cs'], nb.TIMES, SEED, draw=DRAW, samples=SAMPLES)
        losses = []
        for _ in range(30):
            opt.zero_grad()
            loss = training.loss_function(*model(data, seed=1), tg, model)[0]
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        return torch.cat(losses).cpu()

    a, b = run(), run()
    print('loss curve:', [round(float(v), 4) for v in a])
    _record_drift('noise_batch.learns.first_loss', float(a[0]), last_loss=float(a[-1]), steps=30)
    assert torch.equal(_bits(a), _bits(b))
    assert bool(torch.isfinite(a).all()) and float(a[-1]) < float(a[0]), a
