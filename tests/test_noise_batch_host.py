"""Host tests of the ragged training batch (disco_diffdock_amd.training: BatchTargets, loss_function's dispatch, draw_times, epoch_permutation,
ExponentialMovingAverage) and of its restatement tests/noise_batch_ref.py.  No GPU: the context is a stand-in whose two loss methods are the restatement.

The semantics under test (tests/noise_batch_ref.py states them in full): per graph the torsion term is divided by R_g + 1e-4; with apply_mean the
torsion term is the mean over ALL torsions of the batch, [1], and 0 when the batch has none."""
import os
import re

import numpy as np
import pytest
import torch

import noise_batch_ref as nb
import noising_ref as nr
import philox_ref as pr

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
NEW_CALLS = ('ddk_rng_perturbation_batch', 'ddk_rng_forward_times', 'ddk_modify_conformer_batch', 'ddk_score_matching_loss_batch',
             'ddk_score_matching_loss_batch_backward')


def _ragged(seed, rotors):
    """random predictions, targets and per-graph scalars of a batch with the given rotor counts"""
    rng = np.random.default_rng(seed)
    G, T = len(rotors), int(sum(rotors))
    f = lambda *s: rng.normal(0, 2.0, size=s).astype(np.float32)
    scal = [rng.uniform(0.3, 3.0, G).astype(np.float32) for _ in range(3)]
    return dict(tr_pred=f(G, 3), rot_pred=f(G, 3), tor_pred=f(T), tr_score=f(G, 3), rot_score=f(G, 3), tor_score=f(T), tr_sigma=scal[0], so3_norm=scal[1],
                torus_norm2=scal[2], tor_ptr=nb.prefix(rotors))


def _rows(d, tor=True):
    return nb.loss_batch(d['tr_pred'], d['rot_pred'], d['tor_pred'] if tor else None, d['tr_score'], d['rot_score'], d['tor_score'] if tor else None,
                         d['tr_sigma'], d['so3_norm'], d['torus_norm2'], d['tor_ptr'])


def _reference(d, **kw):
    return nb.reference_loss_function(d['tr_pred'], d['rot_pred'], d['tor_pred'], d['tr_score'], d['rot_score'], d['tor_score'], d['tr_sigma'], d['so3_norm'],
                                      d['torus_norm2'], d['tor_ptr'], **kw)


@pytest.mark.parametrize('rotors', [(4, 7, 0, 1), (0, 0, 0), (3,), (0, 5, 0, 0, 2)])
def test_ragged_loss_restatement_against_the_reference_transcription(rotors):
    """the per-graph rows (noising_ref's per-sample loss on each graph's own slice and scalars) against the transcription of utils/training.py:14-61, both
    apply_mean forms, no_torsion, and batches with T = 0"""
    d = _ragged(sum(rotors) + len(rotors), rotors)
    G, T = len(rotors), sum(rotors)
    rows = _rows(d)
    per = _reference(d, apply_mean=False)
    assert all(tuple(v.shape) == (G,) for v in per)
    for k in range(6):
        assert np.allclose(rows[:, k], per[k + 1].numpy(), rtol=1e-12, atol=0), k
    assert np.allclose(per[0].numpy(), rows[:, 0] + rows[:, 1] + rows[:, 2], rtol=1e-12)
    for g, r in enumerate(rotors):      # R_g + 1e-4, and 0 for a graph without torsions
        a, b = d['tor_ptr'][g], d['tor_ptr'][g + 1]
        want = ((d['tor_pred'][a:b].astype(np.float64) - d['tor_score'][a:b]) ** 2 / np.float64(d['torus_norm2'][g])).sum() / (r + 1e-4)
        assert np.isclose(rows[g, 2], want, rtol=1e-12) and (r > 0 or rows[g, 2] == 0)
    mean = _reference(d, apply_mean=True)
    assert mean[1].dim() == 0 and mean[2].dim() == 0 and tuple(mean[3].shape) == (1,) and tuple(mean[0].shape) == (1,)
    got = nb.batch_mean_from_rows(rows, d['tor_ptr'])
    for k in range(6):
        assert np.allclose(got[k], mean[k + 1].numpy(), rtol=1e-12, atol=0), k
    if T:      # the mean over ALL torsions, which is not the mean of the per-graph values
        edge = (d['tor_pred'].astype(np.float64) - d['tor_score']) ** 2 / np.repeat(d['torus_norm2'], rotors).astype(np.float64)
        assert np.isclose(float(mean[3]), edge.mean(), rtol=1e-12)
    else:
        assert float(mean[3]) == 0 and float(mean[6]) == 0
    # no_torsion: zeros of the reference's shapes, the other terms untouched
    nt_per, nt_mean = _reference(d, apply_mean=False, no_torsion=True), _reference(d, apply_mean=True, no_torsion=True)
    assert tuple(nt_per[3].shape) == (G,) and not nt_per[3].any() and tuple(nt_mean[3].shape) == (1,) and not nt_mean[3].any()
    assert torch.equal(nt_per[1], per[1]) and torch.equal(nt_mean[2], mean[2])
    assert np.allclose(_rows(d, tor=False)[:, [0, 1, 3, 4]], rows[:, [0, 1, 3, 4]], rtol=0, atol=0) and not _rows(d, tor=False)[:, [2, 5]].any()


def test_differentiable_restatement_matches_the_rows():
    d = _ragged(5, (4, 7, 0, 1))
    t = lambda k: torch.as_tensor(d[k].astype(np.float64))
    cols = nb.loss_batch_torch(t('tr_pred'), t('rot_pred'), t('tor_pred'), t('tr_score'), t('rot_score'), t('tor_score'), d['tr_sigma'], d['so3_norm'],
                               d['torus_norm2'], d['tor_ptr'])
    assert np.allclose(cols.numpy(), _rows(d)[:, :3], rtol=1e-12)


class _StandInContext:
    """a context whose loss methods are the restatement on host tensors, and that records which one ran"""

    def __init__(self):
        self.calls = []
        self.cfg = None
        so3 = np.linspace(0.5, 2.0, 1000)
        self.score_norm_tables = (so3, np.linspace(0.2, 3.0, 5001))

    def score_matching_loss(self, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2):
        self.calls.append(('single', float(tr_sigma), float(so3_norm), float(torus_norm2)))
        n = lambda v: None if v is None else v.detach().numpy()
        return torch.from_numpy(nr.score_matching_loss(n(tr_pred), n(rot_pred), n(tor_pred), n(tr_score), n(rot_score), n(tor_score) if tor_score is not None
                                                       else np.zeros((tr_score.shape[0], 0)), tr_sigma, so3_norm, torus_norm2)).float()

    def score_matching_loss_batch(self, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_norm, torus_norm2, tor_ptr, T):
        self.calls.append(('batch', int(T)))
        n = lambda v: None if v is None else v.detach().numpy()
        return torch.from_numpy(nb.loss_batch(n(tr_pred), n(rot_pred), n(tor_pred), n(tr_score), n(rot_score), n(tor_score), n(tr_sigma), n(so3_norm),
                                              n(torus_norm2), n(tor_ptr))).float()


def _batch_targets(d, no_torsion=False):
    from disco_diffdock_amd import training
    t = lambda k: torch.from_numpy(d[k])
    G = len(d['tr_sigma'])
    return training.BatchTargets(t('tr_score'), t('rot_score'), None if no_torsion else t('tor_score'), t('tr_sigma'), torch.ones(G), torch.ones(G),
                                 torch.full((G,), 0.5), t('tor_ptr'), None, None, None, t('so3_norm'), t('torus_norm2'),
                                 tuple(int(v) for v in np.diff(d['tor_ptr'])))


@pytest.mark.parametrize('rotors', [(4, 7, 0, 1), (0, 0)])
def test_loss_function_dispatch_and_reductions(rotors):
    """Targets -> the per-sample call with three host scalars, as before; BatchTargets -> the ragged call, the per-graph norms taken from the targets, and
    the reference's 7-tuple in both apply_mean forms"""
    from disco_diffdock_amd import training
    d = _ragged(11, rotors)
    G, T = len(rotors), sum(rotors)
    ctx = _StandInContext()
    tg = _batch_targets(d)
    p = [torch.from_numpy(d[k]) for k in ('tr_pred', 'rot_pred', 'tor_pred')]
    per = training.loss_function(*p, tg, ctx, apply_mean=False)
    assert ctx.calls == [('batch', T)] and all(tuple(v.shape) == (G,) for v in per)
    want = _reference(d, apply_mean=False)
    for a, w in zip(per, want):
        assert np.allclose(a.numpy(), w.numpy(), rtol=2e-6, atol=0)
    mean = training.loss_function(*p, tg, ctx, tr_weight=0.5, rot_weight=2, tor_weight=3)
    want = _reference(d, apply_mean=True, tr_weight=0.5, rot_weight=2, tor_weight=3)
    assert [tuple(v.shape) for v in mean] == [tuple(v.shape) for v in want] == [(1,), (), (), (1,), (), (), (1,)]
    for a, w in zip(mean, want):
        assert np.allclose(a.numpy(), w.numpy(), rtol=5e-6, atol=0)
    if T == 0:
        assert float(mean[3]) == 0 and float(mean[6]) == 0
    nt = training.loss_function(p[0], p[1], None, _batch_targets(d, no_torsion=True), ctx, apply_mean=False)
    assert tuple(nt[3].shape) == (G,) and not nt[3].any() and not nt[6].any()
    assert tuple(training.loss_function(p[0], p[1], None, _batch_targets(d, no_torsion=True), ctx)[3].shape) == (1,)
    # the old path: one complex, B samples, host sigmas, norms looked up in the context's tables
    ctx.calls.clear()
    B, n_rot = 3, 2
    e = _ragged(12, (n_rot,) * B)
    old = training.Targets(torch.from_numpy(e['tr_score']), torch.from_numpy(e['rot_score']), torch.from_numpy(e['tor_score']).reshape(B, n_rot), 1.5, 0.4, 0.9,
                           0.5, None, None, None)
    out = training.loss_function(torch.from_numpy(e['tr_pred']), torch.from_numpy(e['rot_pred']), torch.from_numpy(e['tor_pred']), old, ctx, apply_mean=False)
    so3_norm = float(np.float32(ctx.score_norm_tables[0][int(training.so3_eps_index(0.4))]))
    torus_norm2 = float(np.float32(ctx.score_norm_tables[1][int(training.torus_sigma_index(0.9))]))
    assert ctx.calls == [('single', 1.5, so3_norm, torus_norm2)] and tuple(out[0].shape) == (B,)


def test_exponential_moving_average():
    from disco_diffdock_amd.training import ExponentialMovingAverage
    gen = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(4, 3, generator=gen, dtype=torch.float64)), torch.nn.Parameter(torch.randn(5, generator=gen, dtype=torch.float64)),
              torch.nn.Parameter(torch.randn(2, generator=gen, dtype=torch.float64), requires_grad=False)]
    with pytest.raises(ValueError):
        ExponentialMovingAverage(params, 1.5)
    for use_num_updates in (True, False):
        ema = ExponentialMovingAverage(params, 0.9, use_num_updates=use_num_updates)
        assert len(ema.shadow_params) == 2      # the frozen parameter is not tracked
        shadow, k = [p.detach().numpy().copy() for p in params[:2]], (0 if use_num_updates else None)
        cur = [p.detach().clone() for p in params]
        for step in range(12):
            with torch.no_grad():
                for p in params[:2]:
                    p.add_(torch.randn(p.shape, generator=gen, dtype=torch.float64))
            ema.update(params)
            shadow, k = nb.ema_update(shadow, [p.detach().numpy() for p in params[:2]], 0.9, k)
            for s, w in zip(ema.shadow_params, shadow):
                assert np.allclose(s.numpy(), w, rtol=1e-13, atol=0), step
        assert ema.num_updates == k      # the decay ramps as (1 + k) / (10 + k) until it reaches 0.9 at k = 80: never within these 12 updates
        # store / copy_to / restore
        live = [p.detach().clone() for p in params]
        ema.store(params)
        ema.copy_to(params)
        assert all(torch.equal(p.detach(), s) for p, s in zip(params[:2], ema.shadow_params)) and torch.equal(params[2].detach(), live[2])
        ema.restore(params)
        assert all(torch.equal(p.detach(), w) for p, w in zip(params, live))
        # state_dict round trip
        other = ExponentialMovingAverage(params, 0.5)
        other.load_state_dict(ema.state_dict())
        assert other.decay == 0.9 and other.num_updates == k and all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
        with torch.no_grad():
            for p, c in zip(params, cur):
                p.copy_(c)


def test_epoch_permutation_is_a_pure_function():
    from disco_diffdock_amd.training import epoch_permutation
    for n in (0, 1, 2, 8, 1000):
        a = epoch_permutation(n, 5, 3)
        assert sorted(a) == list(range(n)) and a == epoch_permutation(n, 5, 3)
    assert epoch_permutation(8, 1, 0) == [7, 5, 3, 1, 4, 2, 0, 6]      # recorded: the order may never change under a seed
    orders = {tuple(epoch_permutation(50, s, e)) for s in range(4) for e in range(4)}
    assert len(orders) == 16


def test_draw_times_word_layout():
    """purpose 11, step = draw, block 0, word 0, sample 0, t = the uniform: against the Philox restatement, bit for bit"""
    from disco_diffdock_amd import runtime, training
    assert runtime.RNG_TIME_PURPOSE == 11
    taken = set(runtime.RNG_PURPOSES.values()) | set(runtime.RNG_FORWARD_PURPOSES.values()) | set(runtime.RNG_MATCH_PURPOSES.values())
    assert runtime.RNG_TIME_PURPOSE not in taken and runtime.RNG_LAYOUT == 1
    names = ['a', 'synthetic_70', 'complex with spaces', '']
    for seed, draw in ((0, 0), (7, 3), ((1 << 64) - 1, (1 << 20) - 1)):
        t = training.draw_times(names, seed, draw)
        assert t.dtype == np.float32 and t.shape == (len(names),)
        want = np.array([pr.uniform32(pr.block(seed, pr.fnv1a64(n), np.array([0]), runtime.RNG_TIME_PURPOSE, draw, 0)[:, 0])[0] for n in names], np.float32)
        assert np.array_equal(t.view(np.int32), want.view(np.int32))
        assert (t >= 0).all() and (t < 1).all()
        assert np.array_equal(training.draw_times(names[::-1], seed, draw), t[::-1])      # a complex's time does not depend on its neighbours
    assert not np.array_equal(training.draw_times(names, 7, 3), training.draw_times(names, 7, 4))
    assert training.draw_times([], 1, 0).shape == (0,)
    for kw in (dict(alpha=2), dict(beta=0.5)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            training.draw_times(names, 1, 0, **kw)
    with pytest.raises(RuntimeError, match=r'ddk_rng_forward_times: draw'):
        training.draw_times(names, 1, 1 << 20)


def test_header_declares_the_calls_and_lib_lists_them():
    from disco_diffdock_amd import _lib
    with open(os.path.join(ROOT, 'include', 'ddk.h')) as f:
        header = f.read()
    for name in NEW_CALLS:
        assert re.search(r'^int ' + name + r'\(ddk_ctx\* ctx,', header, re.M), name
        assert name in _lib.SYMBOLS
    assert re.search(r'^ \*\s+11 forward time', header, re.M) and '#define DDK_RNG_LAYOUT 1' in header


def test_standing_batch_covers_the_rotor_counts():
    cs = nb.standing_batch()
    rotors, atoms = nb.rotor_counts(cs), [len(c['lig_pos']) for c in cs]
    assert rotors[0] in (2, 3, 4) and rotors[1] >= 5 and rotors[2:] == [0, 1], rotors
    assert len(set(atoms)) >= 2 and all(20 <= len(c['rec_pos']) <= 40 for c in cs), atoms
    assert all(np.asarray(c['mask_rotate']).size == r * n for c, r, n in zip(cs, rotors, atoms))
    assert len({c['name'] for c in cs}) == 4
