"""CPU tests of tests/adversarial_edges.py: every generator has the property its docstring claims, the host restatement of edge_features_body meets every
bar the GPU module (tests/test_gpu_edge_features_adversarial.py) applies, and the bars bite - every named mutant of the restatement breaks one on a class
that is named here."""
import numpy as np
import pytest

import adversarial_edges as ae

F32 = np.float32


def _dist(cs, ref, g):
    """fp64 lengths of the edges of reference group g"""
    n_lig, n_rec, nl = cs.pos.shape[1], len(cs.c['rec_pos']), cs.B * cs.pos.shape[1]
    lp, rp = cs.pos.reshape(-1, 3).astype(np.float64), np.asarray(cs.c['rec_pos'], np.float64)
    at = lambda node: np.where((node < nl)[:, None], lp[np.minimum(node, nl - 1)], rp[(np.maximum(node, nl) - nl) % n_rec])
    return np.linalg.norm(at(ref[g]['dst']) - at(ref[g]['src']), axis=1)


def _has(ref, g, src, dst):
    return bool(((ref[g]['src'] == src) & (ref[g]['dst'] == dst)).any())


# ---- the generators ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ae.CLASSES)
def test_sizes_and_one_edge_set_for_both_references(name):
    cs = ae.case(name)
    r64, r32 = ae.references(cs)          # (asserts inside that the fp64 neighbour tests give the fp32 edge lists)
    assert cs.pos.dtype == F32 and 2 <= cs.B <= 3 and 12 <= cs.pos.shape[1] <= 70 and 40 <= len(cs.c['rec_pos']) <= 64
    assert all(len(a['src']) == len(b['src']) for a, b in zip(r64, r32))
    assert np.array_equal(np.sort(r64[1]['src'] * 10 ** 6 + r64[1]['dst']), np.sort(r64[3]['dst'] * 10 ** 6 + r64[3]['src']))      # group 3 is group 1 flipped


def test_coincident_pairs_are_in_the_graph():
    cs = ae.case('coincident')
    ref = ae.reference(cs)
    n, nl = cs.pos.shape[1], cs.B * cs.pos.shape[1]
    n_rec = len(cs.c['rec_pos'])
    d0, d1 = _dist(cs, ref, 0), _dist(cs, ref, 1)
    for b in range(cs.B):
        for i, j in cs.props['zero_ll']:
            for s, t in ((i, j), (j, i)):
                m = (ref[0]['src'] == b * n + s) & (ref[0]['dst'] == b * n + t)
                assert m.sum() == 1 and d0[m][0] == 0.0
                assert np.array_equal(ref[0]['sh'][m][0], [1.0, 0.0, 0.0, 0.0])          # F.normalize's eps: the zero vector stays zero
        i, j = cs.props['ulp_ll']
        m = (ref[0]['src'] == b * n + i) & (ref[0]['dst'] == b * n + j)
        assert m.sum() == 1 and d0[m][0] == np.spacing(np.abs(cs.pos[b, j, 0])) > 1e-8          # one ulp of the coordinate, nowhere near subnormal
        i, j = cs.props['zero_lr']
        m = (ref[1]['src'] == b * n + i) & (ref[1]['dst'] == nl + b * n_rec + j)
        assert m.sum() == 1 and d1[m][0] == 0.0
        i, j = cs.props['ulp_lr']
        m = (ref[1]['src'] == b * n + i) & (ref[1]['dst'] == nl + b * n_rec + j)
        assert m.sum() == 1 and 0 < d1[m][0] == np.spacing(np.abs(cs.c['rec_pos'][j, 0]))
    assert min(d0[d0 > 0].min(), d1[d1 > 0].min()) > 1e-8          # nothing below an ulp of a coordinate


def test_binade_sweep_brackets_every_centre_an_edge_can_reach():
    cs = ae.case('binades')
    ref = ae.reference(cs)
    P = ae.params()
    cut = ae.cross_cutoff(cs.t)
    for g, tab, lo, hi in ((0, 'lig', 0.0, np.inf), (2, 'rec', 3.8, np.inf), (1, 'cross', 0.0, cut)):
        off = P[f'{tab}_distance_expansion.offset'].numpy().astype(np.float64)
        step, d = off[1] - off[0], _dist(cs, ref, g)
        for c in off:
            if c - step / 2 >= lo:
                assert ((d > c - step / 2) & (d <= c)).any() or c > hi, (tab, c, 'below')
            if c + step / 2 > lo and c < hi:
                assert ((d >= c) & (d < c + step / 2)).any() or c + step / 2 > hi, (tab, c, 'above')
        coeff = -0.5 / step ** 2
        under = np.exp(coeff * (d[:, None] - off[None]) ** 2).astype(F32).max(1) == 0
        assert under.any() or g == 1, tab          # beyond the last centre: all 32 Gaussians are exactly 0 in fp32 (lig: the long bonds; rec: 60 and 100 A)
        assert (d > off[-1]).any() or g == 1
    d0, d1 = _dist(cs, ref, 0), _dist(cs, ref, 1)
    radius_copies = d0[cs.B * cs.c['bond_index'].shape[1]:]
    assert radius_copies.max() < 5.0 and radius_copies.max() > 5.0 * (1 - 2e-5)          # a pair just inside the ligand radius
    assert d1.max() < cut and d1.max() > cut * (1 - 2e-5)                                  # ... and one just inside the cross cutoff
    nl, n_rec = cs.B * cs.pos.shape[1], len(cs.c['rec_pos'])
    for j in cs.props['far_residues']:
        assert _has(ref, 2, nl + j, nl) and _has(ref, 2, nl, nl + j)


@pytest.mark.parametrize('name', ['far_shift', 'far_mirror'])
def test_far_classes(name):
    cs = ae.case(name)
    if name == 'far_shift':
        assert np.abs(cs.pos.mean((0, 1)) - [150, -80, 60]).max() < 25 and np.abs(cs.c['rec_pos'].mean(0) - [150, -80, 60]).max() < 1
    else:
        assert (cs.pos.min((0, 1)) < 0).all() and (cs.pos.max((0, 1)) > 0).all()          # the ligand straddles every coordinate plane
        ref = ae.reference(cs)
        v = cs.pos.reshape(-1, 3)[ref[0]['dst']] * cs.pos.reshape(-1, 3)[ref[0]['src']]
        assert (v < 0).any(0).all()          # edges whose endpoints have coordinates of opposite sign, in x, y and z
    assert len(ae.reference(cs)[1]['src']) > 0


def test_bonded_pairs_appear_twice_and_long_bonds_once():
    cs = ae.case('bonded')
    ref = ae.reference(cs)
    n, M = cs.pos.shape[1], cs.c['bond_index'].shape[1]
    d0 = _dist(cs, ref, 0)
    key = ref[0]['src'] * 10 ** 6 + ref[0]['dst']
    count = lambda b, i, j: int((key == (b * n + i) * 10 ** 6 + b * n + j).sum())
    long_ = set(map(tuple, cs.props['long_bonds'])) | {(j, i) for i, j in cs.props['long_bonds']}
    assert len(long_) == 4
    for b in range(cs.B):
        for i, j in zip(*cs.c['bond_index']):
            length = np.linalg.norm(cs.pos[b, i].astype(np.float64) - cs.pos[b, j])
            if (int(i), int(j)) in long_:
                assert length > 8.9 and count(b, i, j) == 1          # longer than the radius: the bond copy only
            else:
                assert length < 1.6 and count(b, i, j) == 2          # inside the radius: bond copy and radius copy
    assert (d0[:cs.B * M] > 5.0).sum() == cs.B * 4
    assert (cs.c['bond_attr'].sum(0) > 0).all() and set(np.unique(cs.c['bond_attr'])) == {0.0, 1.0}          # one-hots in all four columns


def test_cap_binds():
    cs = ae.case('cap')
    ref = ae.reference(cs)
    n, M = cs.props['n'], cs.c['bond_index'].shape[1]
    p = cs.pos[0].astype(np.float64)
    within = (np.linalg.norm(p[:, None] - p[None], axis=-1) < 5.0).sum(1) - 1
    received = np.bincount(ref[0]['dst'][cs.B * M:], minlength=cs.B * n)[:n]          # radius_graph caps the neighbours of a CENTRE, and the centre is edge_index[1]
    assert within.max() > 40 and received.max() <= 33 and (received < within).sum() > 10          # more neighbours in range than the cap keeps, for many atoms


def test_empty_and_single_edge_samples():
    cs = ae.case('single_edge')
    ref = ae.reference(cs)
    n, nl, n_rec = cs.pos.shape[1], cs.B * cs.pos.shape[1], len(cs.c['rec_pos'])
    sample = ref[1]['src'] // n
    assert (sample == 0).sum() == 0 and (sample == 1).sum() == 1 and (sample == 2).sum() > 100
    m = sample == 1
    assert ref[1]['src'][m][0] == n + cs.props['atom'] and ref[1]['dst'][m][0] == nl + n_rec + cs.props['residue']
    d = _dist(cs, ref, 1)[m][0]
    cut = ae.cross_cutoff(cs.t)
    assert cut * (1 - 2e-4) < d < cut
    assert np.linalg.norm(cs.c['rec_pos'][None].astype(np.float64) - cs.pos[0][:, None], axis=-1).min() > 150          # sample 0 is 200 A away


@pytest.mark.parametrize('u', [0, 1])
def test_latent_class(u):
    cs = ae.case(f'latents_u{u}')
    assert cs.disco and cs.unconditional == float(u) and cs.B == 3
    assert sorted(np.flatnonzero(np.abs(cs.rec_latent).sum(1))) == cs.props['rec_latent_nodes']
    assert sorted(np.flatnonzero(np.abs(cs.lig_latent).sum(1))) == cs.props['lig_latent_nodes']
    n_rec = len(cs.c['rec_pos'])
    per_sample = [np.abs(cs.rec_latent[b * n_rec:(b + 1) * n_rec]).sum() > 0 for b in range(3)]
    assert per_sample == [True, True, False]          # sample 0 (the shared copy's rows) and sample 1 carry receptor latents, sample 2 ligand ones only
    assert ((cs.rec_latent != 0) & (cs.rec_latent != 1)).any() and ((cs.lig_latent != 0) & (cs.lig_latent != 1)).any()          # not only one-hots


def test_in_degree_counts_every_group():
    cs = ae.case('bonded')
    ref = ae.reference(cs)
    deg = ae.in_degree(cs, ref)
    assert deg.sum() == sum(len(g['src']) for g in ref) and len(deg) == ae.n_nodes(cs) and deg.min() > 0


# ---- the restatement against the bar ----------------------------------------------------------------------------------------------------------
def _figures(name, mutant=None):
    cs = ae.case(name)
    with np.errstate(all='ignore'):
        return ae.compare(cs, ae.host_edges(cs, mutant))


@pytest.mark.parametrize('name', ae.CLASSES)
def test_restatement_is_within_the_bar(name):
    fig = _figures(name)
    assert len(fig) == 8 and not ae.broken(fig), {k: v for k, v in fig.items() if k in ae.broken(fig)}
    assert all(np.isfinite(e) and b > 0 for e, b, _ in fig.values())


def test_multiset_check_leaves_no_edge_out():
    cs = ae.case('bonded')
    got = [dict(g) for g in ae.host_edges(cs)]
    for drop in (0, 2):
        bad = [dict(g) for g in got]
        bad[drop] = {k: v[1:] for k, v in got[drop].items()}          # one edge missing
        with pytest.raises(AssertionError, match='multisets'):
            ae.compare(cs, bad)
    bad = [dict(g) for g in got]
    bad[1] = dict(got[1], dst=np.r_[got[1]['dst'][0] + 1, got[1]['dst'][1:]])          # one edge to the wrong residue
    with pytest.raises(AssertionError, match='multisets'):
        ae.compare(cs, bad)
    nan = [dict(g) for g in got]
    nan[3] = dict(got[3], emb=got[3]['emb'].copy())
    nan[3]['emb'][5, 7] = np.nan
    assert ('rec->lig', 'emb') in ae.broken(ae.compare(cs, nan))          # a NaN never passes


# the class that kills every mutant, and the figure it breaks
KILLED_BY = {
    'sh_negated_group3': ('single_edge', ('rec->lig', 'sh')),
    'sqrt3_omitted': ('coincident', ('lig-lig', 'sh')),
    'bond_row_on_radius_copy': ('bonded', ('lig-lig', 'emb')),
    'cross_table_for_lig': ('binades', ('lig-lig', 'emb')),
    'offsets_shifted': ('binades', ('rec-rec', 'emb')),
    'mirror_from_next_slot': ('far_shift', ('rec->lig', 'emb')),
    'latent_columns_swapped': ('latents_u1', ('rec-rec', 'emb')),
    'unconditional_always': ('latents_u0', ('lig->rec', 'emb')),
}


@pytest.mark.parametrize('mutant', ae.MUTANTS)
def test_every_mutant_breaks_a_bar(mutant):
    name, figure = KILLED_BY[mutant]
    fig = _figures(name, mutant)
    assert figure in ae.broken(fig), (mutant, name, fig[figure])
    assert ae.ratio(*fig[figure][:2]) > 100 * ae.K          # not a near miss: orders of magnitude over the bar
    assert not ae.broken(_figures(name))


def test_mutants_that_need_their_class_pass_elsewhere():
    """the latent and unconditional mutants change nothing without latents (and 'unconditional always' nothing at unconditional = 1): only the DisCo classes see them"""
    assert not ae.broken(_figures('bonded', 'latent_columns_swapped')) and not ae.broken(_figures('latents_u1', 'unconditional_always'))
    assert set(KILLED_BY) == set(ae.MUTANTS)


# ---- the confidence case ------------------------------------------------------------------------------------------------------------------------
def test_confidence_case_and_its_numbering():
    import torch
    cc = ae.conf_case()
    c, B, Bm = cc['c'], cc['pos'].shape[0], cc['max_batch']
    n_lig, n_atom, n_rec = len(c['lig_pos']), len(c['atom_pos']), len(c['rec_pos'])
    assert B == 2 and Bm == B + 1 and n_rec == 40 and 120 <= n_atom <= 200 and 18 <= n_lig <= 24
    r64, r32 = ae.conf_reference(), ae.conf_reference(torch.float32)
    assert all(len(r64[g]['src']) > 0 and r64[g]['sh'].shape[1] == 4 for g in ae.CONF_GROUPS)
    for b in range(B):          # ligand-atom and ligand-residue edges in BOTH poses
        assert ((r64['la']['src'] // n_lig) == b).any() and ((r64['lr']['src'] // n_lig) == b).any()
    for g, f in ae.CONF_FLIPPED.items():          # a flipped group is its forward group with the two ends exchanged, same rows
        assert np.array_equal(r64[g]['src'], r64[f]['dst']) and np.array_equal(r64[g]['emb'], r64[f]['emb'])
    # the mapping: device ids of sample b of every type come back as the oracle's type-local index; the virtual sample is refused
    args = (B, Bm, n_lig, n_atom, n_rec)
    assert ae.conf_device_to_oracle([Bm * n_lig + 1 * n_atom + 7], 'a', *args)[0] == n_atom + 7
    assert ae.conf_device_to_oracle([Bm * n_lig + (Bm + 1) * n_atom + n_rec + 3], 'r', *args)[0] == n_rec + 3
    assert ae.conf_device_to_oracle([n_lig + 2], 'l', *args)[0] == n_lig + 2
    with pytest.raises(AssertionError):
        ae.conf_device_to_oracle([Bm * n_lig + Bm * n_atom], 'a', *args)          # an atom of the virtual ligand-free sample
    # the comparison accepts the oracle's own fp32 rows moved to device numbering, and refuses a missing edge
    base = dict(l=0, a=Bm * n_lig, r=Bm * n_lig + (Bm + 1) * n_atom)
    dev_rows = {g: (r32[g]['src'] + base[g[0]], r32[g]['dst'] + base[g[1]], r32[g]['emb'].astype(F32), r32[g]['sh'].astype(F32)) for g in ae.CONF_GROUPS}
    fig = ae.conf_compare(dev_rows, Bm)
    assert len(fig) == 18 and not ae.broken(fig)
    dev_rows['aa'] = tuple(v[1:] for v in dev_rows['aa'])
    with pytest.raises(AssertionError, match='multisets'):
        ae.conf_compare(dev_rows, Bm)
