"""CPU tests of the specification of the device table builders (tests/graph_build_ref.py; csrc/k_build.hip): the numpy restatements against the host
generators of synthetic.py, which are how the project got these tables so far, against oracle/cluster_lite.py, and against networkx where it imports;
the margins that make the GPU comparison exact; and the plumbing of graphs.complete_complex and of the ctypes declarations."""
import os
import re

import numpy as np
import pytest
import torch

import graph_build_ref as gb
from disco_diffdock_amd import graphs, synthetic, _lib
from oracle import cluster_lite

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n_res, seed', ((65, 65), (300, 301), (1025, 1025)))
def test_knn_restatement_equals_make_receptor(n_res, seed):
    """make_receptor measures the float64 points it later rounds to float32 and sorts with an unstable argsort: the seeds are ones whose receptor has no
    two distances within 1e-6 relative of each other in a selected row (asserted), so that both say the same about the same points"""
    rec = synthetic.make_receptor(np.random.default_rng(seed), n_res, esm_dim=4)
    assert gb.knn_margins(rec['rec_pos'], 15.0, 24, interior=True) == (True, True)
    got, status = gb.knn_graph_ref(rec['rec_pos'], 15.0, 24)
    assert status == 0 and np.array_equal(got, rec['rec_edge_index'])


ATOM_CAP = 64          # a max_num_neighbors that never binds on the synthetic receptor atoms (asserted where it is used)


def _complex_with_atoms(seed=2, n_res=40, atom_max_neighbors=ATOM_CAP):
    c = synthetic.make_complex(seed, n_res=n_res, esm_dim=4)
    return synthetic.add_receptor_atoms(c, np.random.default_rng(seed + 100), atom_max_neighbors=atom_max_neighbors)


def test_radius_restatement_equals_add_receptor_atoms_and_cluster_lite():
    """add_receptor_atoms drops the centre BEFORE it cuts to max_num_neighbors, torch_cluster (oracle/cluster_lite.py, the rule of ddk_radius_graph)
    after: the two are the same graph where the cap does not bind, and where it binds they differ exactly at the centres whose own index comes after
    their first max_num_neighbors + 1 in-radius points, which keep one neighbour more (the next one in index order)."""
    c = _complex_with_atoms()
    assert gb.radius_margins(c['atom_pos'], 5.0)
    got, status = gb.radius_graph_ref(c['atom_pos'], 5.0, ATOM_CAP)
    assert status == 0 and np.bincount(got[1]).max() < ATOM_CAP
    assert np.array_equal(got, c['atom_edge_index'])
    assert np.array_equal(got, cluster_lite.radius_graph(torch.from_numpy(c['atom_pos']), 5.0, max_num_neighbors=ATOM_CAP).numpy())
    c8 = _complex_with_atoms(atom_max_neighbors=8)
    assert np.array_equal(c8['atom_pos'], c['atom_pos'])
    got8, _ = gb.radius_graph_ref(c8['atom_pos'], 5.0, 8)
    assert np.array_equal(got8, cluster_lite.radius_graph(torch.from_numpy(c8['atom_pos']), 5.0, max_num_neighbors=8).numpy())
    extra = 0
    for i in range(len(c8['atom_pos'])):
        mine, theirs, every = got8[0][got8[1] == i], c8['atom_edge_index'][0][c8['atom_edge_index'][1] == i], got[0][got[1] == i]
        late = len(every) >= 9 and i > np.sort(np.append(every, i))[8]          # self is not among the first nine in-radius points
        assert mine[:len(theirs)].tolist() == theirs.tolist() and len(mine) - len(theirs) == int(late)
        extra += int(late)
    assert extra > 0


@pytest.mark.parametrize('name', ('coincident', 'lattice_r5', 'lattice_r5_wide', 'atoms_300', 'one_point'))
def test_radius_restatement_equals_cluster_lite(name):
    pos, r, k = gb.radius_cases()[name]
    got, status = gb.radius_graph_ref(pos, r, k)
    assert status == 0 and np.array_equal(got, cluster_lite.radius_graph(torch.from_numpy(pos).double(), r, max_num_neighbors=k).numpy())
    if name == 'coincident':          # atoms 0..4 keep 4 neighbours, atoms 5..11 keep 5
        assert np.bincount(got[1], minlength=12).tolist() == [4] * 5 + [5] * 7


def test_boundary_and_tie_cases_are_what_they_claim():
    lat, cutoff, _ = gb.knn_cases()['lattice_k24']
    d2 = gb.d2_rows(lat, 0, len(lat))
    assert (d2 == 225.0).any() and len(lat) == 125
    ei, _ = gb.knn_graph_ref(lat, cutoff, 24)
    pairs = set(map(tuple, ei.T.tolist()))
    assert all((i, j) not in pairs for i, j in zip(*np.nonzero(d2 == 225.0)))          # exactly at the cutoff: not a neighbour
    ei6, _ = gb.knn_graph_ref(lat, cutoff, 6)
    assert np.bincount(ei6[0]).max() == 6 and ei6.shape[1] == 125 * 6
    centre = 62          # (6, 6, 6): its six nearest are tied at distance 3 and come in index order
    assert ei6[1][ei6[0] == centre].tolist() == sorted(ei6[1][ei6[0] == centre].tolist()) and (d2[centre][ei6[1][ei6[0] == centre]] == 9.0).all()
    unit = gb.radius_cases()['lattice_r5'][0]
    assert (gb.d2_rows(unit, 0, len(unit)) == 25.0).any()
    ball, cutoff, k = gb.knn_cases()['dense_ball']
    assert (gb.d2_rows(ball, 0, 64) < 225.0).all() and len(ball) == 1500
    eb, _ = gb.knn_graph_ref(ball, cutoff, k)
    assert eb.shape[1] == 1500 * 24
    iso, cutoff, k = gb.knn_cases()['isolated']
    ei, _ = gb.knn_graph_ref(iso, cutoff, k)
    assert (ei[0] == 7).sum() == 1
    assert gb.knn_graph_ref(gb.two_points(), 15.0, 24)[0].tolist() == [[0, 1], [1, 0]]
    pos, r, k = gb.radius_cases()['cap_1024']
    counts = np.bincount(gb.radius_graph_ref(pos, r, k)[0][1])
    assert counts[:1025].tolist() == [1024] * 1025 and counts[1025:].tolist() == [1025] * 75


@pytest.mark.parametrize('name', tuple(gb.ligand_cases()))
def test_mask_restatement_equals_synthetic(name):
    n, bi = gb.ligand_cases()[name]
    edge_mask, mask_rotate, status = gb.transformation_mask_ref(n, bi)
    want_e, want_r = synthetic.transformation_mask(n, [tuple(p) for p in bi[:, 0::2].T.tolist()])
    assert status == 0 and np.array_equal(edge_mask, want_e) and np.array_equal(mask_rotate, want_r)
    assert int(edge_mask.sum()) == len(mask_rotate)
    if name.startswith('bridge'):          # the tie: both sides have six atoms, the side with atom 0 is l
        assert mask_rotate.tolist() == [[1] * 6 + [0] * 6] and edge_mask[-2:].tolist() == ([1, 0] if name == 'bridge_flipped' else [0, 1])


@pytest.mark.parametrize('name', ('path4', 'ring6', 'star', 'bridge', 'bridge_flipped', 'make_ligand_0', 'make_ligand_5'))
def test_mask_restatement_equals_networkx(name):
    nx = pytest.importorskip('networkx')
    n, bi = gb.ligand_cases()[name]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(bi[:, 0::2].T.tolist())
    to_rotate = []          # utils/torsion.py:15-45 on an undirected graph whose edge k is column 2k
    for u, v in bi[:, 0::2].T.tolist():
        G2 = G.copy()
        G2.remove_edge(u, v)
        if not nx.is_connected(G2):
            l = list(sorted(nx.connected_components(G2), key=len)[0])
            if len(l) > 1:
                to_rotate += ([[], l] if u in l else [l, []])
                continue
        to_rotate += [[], []]
    edge_mask, mask_rotate, _ = gb.transformation_mask_ref(n, bi)
    assert edge_mask.tolist() == [int(len(l) > 0) for l in to_rotate]
    rows = [l for l in to_rotate if l]
    assert all(sorted(np.nonzero(r)[0].tolist()) == sorted(l) for r, l in zip(mask_rotate, rows))


def test_broken_ligands_have_the_stated_status():
    for name, (n, bi, status) in gb.broken_ligands().items():
        edge_mask, mask_rotate, got = gb.transformation_mask_ref(n, bi)
        assert got == status, name
        assert not edge_mask.any() and len(mask_rotate) == 0


def test_non_finite_coordinates_are_status_2():
    lat = gb.lattice(3)
    for bad in (gb.with_nan(lat), gb.with_inf(lat)):
        assert gb.knn_graph_ref(bad)[1] == 2 and gb.radius_graph_ref(bad)[1] == 2


def test_random_gpu_inputs_keep_their_margins():
    """every random point set the GPU tests compare exactly: no pair within 1e-6 relative of its cutoff, no near-tie at a selected row's boundary"""
    ball, cutoff, k = gb.knn_cases()['dense_ball']
    assert gb.knn_margins(ball, cutoff, k) == (True, True)
    assert gb.knn_margins(gb.random_residues(3000, 1), 15.0, 24) == (True, True)
    assert gb.radius_margins(gb.protein_atoms(8000, 3), 5.0)
    for name in ('cap_1024', 'atoms_300'):
        pos, r, _ = gb.radius_cases()[name]
        assert gb.radius_margins(pos, r)
    for c in (synthetic.make_complex(2, n_res=300, esm_dim=4), _complex_with_atoms()):
        assert gb.knn_margins(c['rec_pos'], 15.0, 24) == (True, True)          # the two complexes of the end-to-end test
    assert gb.radius_margins(_complex_with_atoms()['atom_pos'], 5.0)


class _FakeContext:
    """stands in for runtime.Context: the three builders answer from the restatements and count their calls"""

    def __init__(self):
        self.calls = []

    def receptor_knn_graph(self, pos, cutoff, max_neighbor):
        self.calls.append('knn')
        return torch.from_numpy(gb.knn_graph_ref(pos, cutoff, max_neighbor)[0]).int()

    def radius_graph(self, pos, r, max_num_neighbors):
        self.calls.append('radius')
        return torch.from_numpy(gb.radius_graph_ref(pos, r, max_num_neighbors)[0]).int()

    def transformation_mask(self, n_lig, bond_index):
        self.calls.append('mask')
        e, r, _ = gb.transformation_mask_ref(n_lig, bond_index)
        return torch.from_numpy(e), torch.from_numpy(r)


def test_complete_complex_fills_what_is_missing_and_nothing_else():
    full = _complex_with_atoms()
    tables = ('rec_edge_index', 'edge_mask', 'mask_rotate', 'atom_edge_index')
    ctx = _FakeContext()
    c = {k: v for k, v in full.items() if k not in tables}
    out = graphs.complete_complex(c, ctx=ctx, atom_max_neighbors=ATOM_CAP)
    assert out is c and ctx.calls == ['knn', 'mask', 'radius']
    for k in tables:
        assert np.array_equal(out[k], full[k]) and out[k].dtype == full[k].dtype, k
    # present keys are handed back as they are, the same objects, and their builders are not called
    ctx = _FakeContext()
    marked = dict(full)
    marked['rec_edge_index'] = full['rec_edge_index'][:, :5].copy()
    del marked['atom_edge_index']
    before = {k: (id(v), v.copy() if isinstance(v, np.ndarray) else v) for k, v in marked.items()}
    out = graphs.complete_complex(marked, ctx=ctx)
    assert ctx.calls == ['radius']
    assert all(id(out[k]) == i and (not isinstance(v, np.ndarray) or np.array_equal(out[k], v)) for k, (i, v) in before.items())
    # no atom level: no atom graph
    ctx = _FakeContext()
    c = {k: v for k, v in synthetic.make_complex(3, n_res=30, esm_dim=4).items() if k not in tables}
    assert 'atom_edge_index' not in graphs.complete_complex(c, ctx=ctx) and ctx.calls == ['knn', 'mask']
    # one of the pair missing: both are written
    ctx = _FakeContext()
    c = {k: v for k, v in full.items() if k != 'mask_rotate'}
    assert np.array_equal(graphs.complete_complex(c, ctx=ctx)['mask_rotate'], full['mask_rotate']) and ctx.calls == ['mask']


def test_graph_cache_takes_a_completed_complex(tmp_path):
    from disco_diffdock_amd import graph_cache
    full = _complex_with_atoms()
    c = graphs.complete_complex({k: v for k, v in full.items() if k not in ('rec_edge_index', 'edge_mask', 'mask_rotate', 'atom_edge_index')},
                                ctx=_FakeContext(), atom_max_neighbors=ATOM_CAP)
    path = str(tmp_path / 'c.ddkg')
    assert graph_cache.save_complexes(path, [c]) == 1
    back = graph_cache.load_complexes(path)[0]
    for k in ('rec_edge_index', 'edge_mask', 'mask_rotate', 'atom_edge_index'):
        assert np.array_equal(back[k], full[k])


def test_declarations_match_the_header():
    hdr = open(os.path.join(ROOT, 'include', 'ddk.h')).read()
    L = _lib.lib()
    for name in ('ddk_receptor_knn_graph', 'ddk_radius_graph', 'ddk_ligand_transformation_mask'):
        assert name in _lib.SYMBOLS and name + '_workspace' in _lib.SYMBOLS
        m = re.search(r'int %s\((.*?)\);' % name, hdr, re.S)
        assert m, name
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(',')) == 10
        assert getattr(L, name + '_workspace').restype is _lib.C.c_int64
    # the host queries refuse what the calls refuse
    assert L.ddk_receptor_knn_graph_workspace(1, 24) < 0 and L.ddk_receptor_knn_graph_workspace(65537, 24) < 0 and L.ddk_receptor_knn_graph_workspace(2, 129) < 0
    assert L.ddk_radius_graph_workspace(0, 8) < 0 and L.ddk_radius_graph_workspace(8, 1025) < 0 and L.ddk_radius_graph_workspace(65536, 1024) > 0
    assert L.ddk_ligand_transformation_mask_workspace(257, 2) < 0 and L.ddk_ligand_transformation_mask_workspace(6, 3) < 0
    assert L.ddk_ligand_transformation_mask_workspace(6, 2050) < 0 and L.ddk_ligand_transformation_mask_workspace(1, 0) > 0
    assert L.ddk_receptor_knn_graph_workspace(3000, 24) >= 3000 * 24 * 4
