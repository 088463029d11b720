"""CPU tests of tests/adversarial_latent.py: every generator has the properties it claims (positions sit in the thread and trip of gumbel_fwd_kernel's
loops that the case names, tied sets tie exactly in fp32, the saturated logit absorbs the noise that is actually drawn), the margins that keep the device
comparisons honest hold for EVERY case with no row left out, and the numpy references agree with the restatements the suite already trusts
(tests/test_gpu_round2.py's inverse_cdf, oracle.ar_ref's predictor)."""
import numpy as np
import pytest
import torch

import adversarial_latent as al
import latent_embedding_ref as lref
from oracle import ar_ref
from oracle import score_model_ref as smr

F32 = np.float32


# ---- Gumbel --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_trips_reaches_the_second_trip_where_it_claims():
    c = al.gumbel_case('two_trips')
    assert [nl + nr for nl, nr in c['graphs']] == [1800, 1025, 1, 0, 1024, 9] and c['graphs'] == al.TWO_TRIPS
    cl = c['claims']
    g, p = cl['alone_in_second_quad']
    n = sum(c['graphs'][g])
    assert p == n - 1 and al.thread_trip(p) == (0, 1) and al.thread_trip(p - 1) == (al.GUM_T - 1, 0)      # the last position alone in thread 0's second quad
    n = sum(c['graphs'][cl['every_thread_once']])
    assert n == al.GUM_T * al.QUAD and al.thread_trip(n - 1) == (al.GUM_T - 1, 0)      # every thread exactly one full quad, no second trip
    assert sum(c['graphs'][cl['empty']]) == 0 and 0 < cl['empty'] < len(c['graphs']) - 1      # the empty graph between two others
    assert all(c['graphs'][g][0] == 0 for g in cl['no_ligand'])
    assert al.thread_trip(1799) == (193, 1) and al.thread_trip(300)[1] == 0      # the 1800-node graph: 450 quads, 194 threads take a second trip
    for g, (nl, nr) in enumerate(c['graphs']):
        assert c['logits'][g].shape == c['grads'][g].shape == (nl + nr, al.D_MAX) and c['logits'][g].dtype == F32
    for D in (1, 3):      # a case at D columns holds the first D columns of the case at 4
        cd = al.gumbel_case('two_trips', D)
        assert all(np.array_equal(a, b[:, :D]) for a, b in zip(cd['logits'] + cd['grads'], c['logits'] + c['grads'])) and cd['streams'] == c['streams']


@pytest.mark.parametrize('name', ['two_trips', 'sharp'])
def test_unique_maximum_cases_have_a_margin_fp32_cannot_flip(name):
    """for every (graph, d) the two largest of logit + gum in fp64 are more than 1e-4 apart (the condition tests/test_gpu_gumbel.py asserts), and the fp64
    softmax's argmax is that node at both temperatures"""
    c = al.gumbel_case(name)
    assert c['claims']['unique_maximum']
    for g, (nl, nr) in enumerate(c['graphs']):
        if nl + nr == 0:
            continue
        for d in range(al.D_MAX):
            k, gap = al.gumbel_margin(c, g, d)
            assert gap > al.MARGIN_GUMBEL, (name, g, d, gap)
            for T in (1.0, 0.01):
                assert lref.gumbel_forward(c['logits'][g][:, d], al.gumbel_uniforms(c, g, d), T)[2] == k


def test_sharp_is_two_trips_first_graph():
    s, t = al.gumbel_case('sharp'), al.gumbel_case('two_trips')
    assert s['T'] == 0.01 and s['graphs'] == t['graphs'][:1] and s['streams'] == t['streams'][:1] and np.array_equal(s['logits'][0], t['logits'][0])
    g = np.abs(s['grads'][0].astype(np.float64))
    assert g.min() < 1e-18 and g.max() > 1e18 and ((g > 1e-3) & (g < 1e3)).any() and np.isfinite(s['grads'][0]).all()      # all three scales are present


def test_saturated_ties_tie_exactly_in_fp32():
    c = al.gumbel_case('saturated_ties')
    cl = c['claims']
    assert c['T'] == 1.0 and c['graphs'] == ((700, 500), (700, 500))
    assert cl['where'] == {1029: (1, 1), 1000: (250, 0), 699: (174, 0), 700: (175, 0)}      # thread 1's second quad; thread 250; the two sides of the boundary
    assert cl['boundary'] == (c['graphs'][0][0] - 1, c['graphs'][0][0])
    assert cl['hard'] == (min(cl['tied'][0]), min(cl['tied'][1])) == (699, 1000)
    assert al.thread_trip(cl['hard'][1])[0] > al.thread_trip(1029)[0]      # second graph: the lowest tied position sits in a higher thread than the other one
    for g in range(2):
        tied = np.zeros(1200, bool)
        tied[list(cl['tied'][g])] = True
        for d in range(al.D_MAX):
            lg = c['logits'][g][:, d]
            assert (lg[tied] == al.BIG).all() and np.abs(lg[~tied]).max() < 10
            gum = lref.gumbel_noise(al.gumbel_uniforms(c, g, d), dtype=F32)      # the noise actually drawn, in fp32
            assert np.isfinite(gum).all() and np.abs(gum).max() > 1
            z = lg + gum
            assert z.dtype == F32 and (z[tied] == al.BIG).all() and np.abs(z[~tied]).max() < 100      # 1e30f + gum == 1e30f: z ties exactly
            # the same in fp64, where the kernel forms z (ulp(1e30) = 1.4e14 there): the tied z are the one fp32 number 1e30f, their pair's lo is 0
            z64 = lg.astype(np.float64) + lref.gumbel_noise(al.gumbel_uniforms(c, g, d))
            assert (z64[tied] == float(al.BIG)).all() and (z64[tied].astype(F32).astype(np.float64) == z64[tied]).all()
            # and the ~100 wide band around 0 is far under expf's reach of 1e30: every other exponential is exactly 0, y = 1 / k
            assert float(z[~tied].max()) - float(al.BIG) < -1e29


def test_flat_makes_every_exponential_one():
    c = al.gumbel_case('flat')
    assert c['T'] == 1e30 and c['graphs'] == ((5, 1100),) and al.thread_trip(1104) == (20, 1)      # 277 quads: threads 0 .. 20 take a second trip
    for d in range(al.D_MAX):
        z = ((c['logits'][0][:, d] + lref.gumbel_noise(al.gumbel_uniforms(c, 0, d), dtype=F32)) / F32(1e30)).astype(F32)
        arg = z.astype(np.float64) - float(z.max())
        assert np.abs(arg).max() < 1e-28 and (np.exp(arg.astype(F32)) == 1).all()
        z64 = (c['logits'][0][:, d].astype(np.float64) + lref.gumbel_noise(al.gumbel_uniforms(c, 0, d))) / 1e30      # as the kernel forms it, in fp64
        assert (np.exp(z64 - z64.max()).astype(F32) == 1).all()
    assert c['claims']['y'] == F32(1) / F32(1105) and c['claims']['hard'] == 0
    g = np.abs(c['grads'][0])
    assert np.isfinite(g).all() and 1e20 < np.median(g) < 1e25


# ---- the AR pick ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ar_sizes_give_one_two_and_three_logits_per_thread():
    assert [nl + nr for nl, nr in al.AR_SIZES] == [37, 319, 540] and [al.ar_chunk(nl + nr) for nl, nr in al.AR_SIZES] == [1, 2, 3]
    assert (319 + 1) // 2 == 160      # at n = 319 the threads from 160 on own nothing


@pytest.mark.parametrize('n_lig,n_rec', al.AR_SIZES)
def test_ar_cases_state_what_the_pick_rule_gives(n_lig, n_rec):
    """every constructed row's expectation is what ar_pick_ref computes, and the rows are built the way their names say"""
    n, per = n_lig + n_rec, al.ar_chunk(n_lig + n_rec)
    cases = al.ar_decode_cases(n_lig, n_rec)
    rows = {r['name']: r for r in cases['argmax']}
    assert len(rows) == len(cases['argmax']) == 11
    for r in cases['argmax']:
        assert r['logits'].shape == (n,) and r['logits'].dtype == F32 and r['u'] is None
        for T in al.AR_ARGMAX_T:
            assert al.ar_pick_ref(r['logits'], T)[0] == r['expect'], (r['name'], T)
    assert [rows[k]['expect'] for k in ('max_first', 'max_last_ligand', 'max_first_residue', 'max_last')] == [0, n_lig - 1, n_lig, n - 1]
    tie = np.flatnonzero(rows['tie3']['logits'] == rows['tie3']['logits'].max())
    assert len(tie) == 3 and tie[0] == n_lig - 1 and tie[1] == n_lig and len({int(i) // per for i in tie}) >= 2 and rows['tie3']['expect'] == tie[0]
    assert rows['all_neg_inf']['expect'] == 0
    lg = rows['nan_after_inf']['logits']
    assert np.flatnonzero(np.isinf(lg))[0] < np.flatnonzero(np.isnan(lg))[0] == rows['nan_after_inf']['expect']
    assert list(np.flatnonzero(np.isnan(rows['two_nans']['logits']))) == [rows['two_nans']['expect'], n - 2]
    lg = rows['overflow']['logits']
    with np.errstate(over='ignore'):
        assert all(np.isinf(lg[lg > 1e36] * F32(T)).all() for T in al.AR_ARGMAX_T) and int(np.argmax(lg)) != rows['overflow']['expect'] == np.flatnonzero(lg > 1e36)[0]
    lg = rows['negative_zero']['logits']
    zeros = np.flatnonzero(lg == 0)
    assert len(zeros) == 2 and np.signbit(lg[zeros[0]]) and not np.signbit(lg[zeros[1]]) and (np.delete(lg, zeros) < 0).all() and rows['negative_zero']['expect'] == zeros[0]
    assert (rows['negative']['logits'] < 0).all() and np.isfinite(rows['negative']['logits']).all()
    # ---- sampling ----
    srows = {r['name']: r for r in cases['sample']}
    assert len(srows) == len(cases['sample'])
    for r in cases['sample']:
        assert r['u'].dtype == F32 and 0 <= r['u'] < 1
        assert al.ar_pick_ref(r['logits'], al.AR_SAMPLE_T, r['u'])[0] == r['expect'], r['name']
    top = F32(1) - F32(2.0 ** -24)
    assert srows['zeros_u0']['expect'] == 0 and srows['zeros_u_half']['expect'] == n // 2 and srows['zeros_u_top']['expect'] == n - 1 and srows['zeros_u_top']['u'] == top
    for k in (1, n_lig, n - 1):
        u = srows[f'zeros_u_{k}_over_n']['u']
        assert float(u) <= k / n < float(np.nextafter(u, F32(1))) and srows[f'zeros_u_{k}_over_n']['expect'] in (k - 1, k)
    r = srows['leading_zero_mass']
    lead = r['logits'][:r['expect']]
    assert r['u'] == 0 and r['expect'] > n_lig + per and (np.isnan(lead) | np.isneginf(lead)).all() and np.isnan(lead).any() and np.isneginf(lead).any()
    assert np.isfinite(r['logits'][r['expect']])
    for k in ('one_inf_u1e-6', 'one_inf_u_half', 'one_inf_u_top'):
        assert srows[k]['u'] >= F32(1e-6) and list(np.flatnonzero(np.isinf(srows[k]['logits']))) == [srows[k]['expect']]
    for k, which in (('two_overflows_first', 0), ('two_overflows_second', 1)):
        lg = srows[k]['logits']
        over = np.flatnonzero(lg * F32(al.AR_SAMPLE_T) > F32(88.73))
        assert len(over) == 2 and over[which] == srows[k]['expect']
        assert n == 37 or over[0] // per // 64 != over[1] // per // 64      # (the two sit in different waves of the scan wherever the graph has more than one)
        with np.errstate(over='ignore'):
            assert np.isinf(np.exp(lg[over] * F32(al.AR_SAMPLE_T))).all()      # both fp32 exponentials overflow
    assert srows['all_neg_inf']['expect'] == n - 1


def test_no_random_sampling_row_is_closer_than_the_margin():
    """THE condition that keeps the sampling comparison honest.  The device's expf and the fp64 exp of the same fp32 argument differ by a few fp32 ulps, which
    moves every partial sum by under 3e-7 of the total; the kernel's blocked fp64 scan against the sequential cumsum moves it by about n * 2^-53.  A target
    at least 1e-5 of the total away from every partial sum - more than 30 times both - is picked the same way by both.  Every random row of every size has
    to meet it: none is left out, the generator's seeds are chosen so."""
    picks = set()
    for n_lig, n_rec in al.AR_SIZES:
        rows = [r for r in al.ar_decode_cases(n_lig, n_rec)['sample'] if r['name'].startswith('random')]
        assert len(rows) == al.AR_RANDOM_ROWS == 40
        for r in rows:
            idx, margin = al.ar_pick_ref(r['logits'], al.AR_SAMPLE_T, r['u'])
            assert margin >= al.AR_MARGIN, (n_lig, n_rec, r['name'], margin)
            assert np.isfinite(r['logits']).all()
            picks.add((n_lig, idx < n_lig))
        assert len({r['expect'] for r in rows}) > 10      # the draws spread over the nodes
    assert len(picks) >= 4      # both sides of the boundary are picked


def test_ar_pick_ref_agrees_with_the_inverse_cdf_of_the_round2_test():
    """tests/test_gpu_round2.py's inverse_cdf (the pick rule restated in torch on logits * T) on the random rows"""
    for n_lig, n_rec in al.AR_SIZES:
        rows = [r for r in al.ar_decode_cases(n_lig, n_rec)['sample'] if r['name'].startswith('random')]
        lat = torch.from_numpy(np.stack([r['logits'] for r in rows])) * al.AR_SAMPLE_T
        u = torch.from_numpy(np.array([r['u'] for r in rows], F32))
        p = torch.nan_to_num(torch.exp(lat.float())).double()
        cum = torch.cumsum(p, 1)
        target = u.double()[:, None] * cum[:, -1:]
        got = (cum > target).int().argmax(1)
        assert got.tolist() == [r['expect'] for r in rows]


# ---- the AR predictors ---------------------------------------------------------------------------------------------------------------------------------------------
CFG = smr.ScoreModelConfig(latent_dim=2, latent_vocab=1, latent_droprate=0.1)


@pytest.mark.parametrize('H,ns,no_bn,stats', al.AR_LOGITS_CASES + ((128, 16, False, None),))
def test_ar_mlp_ref_equals_the_oracle_predictor(H, ns, no_bn, stats):
    P, claims = al.ar_state_dict(CFG, H, ns, no_bn, stats)
    assert claims == dict(H=H, ns=ns, no_bn=no_bn)
    for name in al.PREDICTORS:
        assert tuple(P[f'{name}.0.weight'].shape) == (H, 2 * ns) and tuple(P[f'{name}.4.weight'].shape) == (H, H) and tuple(P[f'{name}.8.weight'].shape) == (1, H)
        for i in (1, 5):
            assert (f'{name}.{i}.running_var' in P) == (not no_bn) and (f'{name}.{i}.weight' in P) == (not no_bn)
            if stats == 'hard':
                var, w = P[f'{name}.{i}.running_var'], P[f'{name}.{i}.weight']
                assert set(var.tolist()) == {float(F32(1e-6)), float(F32(1e-5)), 1.0}
                assert int((w < 0).sum()) == H // 4 and int((w == 0).sum()) == 1 and float(P[f'{name}.{i}.running_mean'].abs().max()) > 3
    x = torch.randn(70, 84, dtype=torch.float64, generator=torch.Generator().manual_seed(H + ns))
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    if no_bn:      # the oracle's predictor always normalises: give it the identity statistics (eps included) to stand for "no BatchNorm"
        for name in al.PREDICTORS:
            for i in (1, 5):
                P64.update({f'{name}.{i}.running_mean': torch.zeros(H, dtype=torch.float64), f'{name}.{i}.running_var': torch.full((H,), 1 - 1e-5, dtype=torch.float64),
                            f'{name}.{i}.weight': torch.ones(H, dtype=torch.float64), f'{name}.{i}.bias': torch.zeros(H, dtype=torch.float64)})
    for name in al.PREDICTORS:
        want = ar_ref._predictor(torch.cat([x[:, :ns], x[:, -ns:]], 1), P64, name)[:, 0].numpy()
        got = al.ar_mlp_ref(x.numpy(), P, name, ns)
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        got32 = al.ar_mlp_ref(x.numpy(), P, name, ns, np.float32)
        assert got32.dtype == F32 and 0 < np.abs(got32 - want).max() < 1e-3 * np.abs(want).max()      # the fp32 form is another evaluation of the same function
    lg = al.ar_logits_ref(x[:22].numpy(), x[22:66].numpy(), P, ns, 2)
    sl, sr = al.ar_mlp_ref(x[:22].numpy(), P, al.PREDICTORS[0], ns), al.ar_mlp_ref(x[22:66].numpy(), P, al.PREDICTORS[1], ns)
    assert lg.shape == (2, 33) and np.array_equal(lg[1], np.concatenate([sl[11:22], sr[22:44]]))      # graph b's atoms, then graph b's residues
