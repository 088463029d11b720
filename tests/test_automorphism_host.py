"""tests/automorphism_ref.py, the specification the device enumeration (csrc/k_autos.hip) is tested against, checked on the CPU: its row counts, that
each table is a group, that networkx finds the same set, and that the level-by-level form of the search never holds more partial maps than the K
automorphisms on these graphs, so that the GPU tests' capacity of 2 K leaves the four pruning rules a factor of two."""
import numpy as np
import pytest

import automorphism_ref as ar

NAMES = tuple(ar.GRAPHS)


def test_the_graphs_are_the_listed_ones():
    assert NAMES == ('one_atom', 'toluene', 'hexagon', 'star', 'no_bonds', 'cubane', 'c6_c3_c3', 'cf3_x4', 'cf3_x5', 'path256')
    for name in NAMES:
        colour, bonds, K = ar.GRAPHS[name]()
        assert len(colour) == ar.ATOMS[name] and bonds.shape[0] == 2 and (bonds.size == 0 or (0 <= bonds.min() and bonds.max() < len(colour)))
    assert {n: ar.GRAPHS[n]()[2] for n in ('cf3_x4', 'cf3_x5')} == {'cf3_x4': 6 ** 4, 'cf3_x5': 6 ** 5}
    deg = np.bincount(ar.GRAPHS['cubane']()[1].reshape(-1), minlength=8)
    assert (deg == 3).all()                                                      # 3-regular: no degree splits anything
    assert (np.bincount(ar.GRAPHS['c6_c3_c3']()[1].reshape(-1)) == 2).all()      # every atom has degree 2


@pytest.mark.parametrize('name', NAMES)
def test_row_count_identity_and_validity(name):
    colour, bonds, K, table = ar.graph_and_table(name)
    n = len(colour)
    assert table.shape == (K, n) and table.dtype == np.int32
    assert np.array_equal(table[0], np.arange(n))
    assert len({r.tobytes() for r in table}) == K
    adj = np.zeros((n, n), bool)
    adj[bonds[0], bonds[1]] = adj[bonds[1], bonds[0]] = True
    for row in table[:: max(K // 50, 1)]:
        assert np.array_equal(np.sort(row), np.arange(n)) and np.array_equal(colour[row], colour)
        assert np.array_equal(adj[np.ix_(row, row)], adj)


@pytest.mark.parametrize('name', NAMES)
def test_the_table_is_a_group(name):
    """closed under composition and inverse (for the large tables: every row composed with 40 of them)"""
    _, _, K, table = ar.graph_and_table(name)
    have = {r.tobytes() for r in table}
    partners = table if K <= 200 else table[np.random.default_rng(0).choice(K, 40, replace=False)]
    for g in partners:
        assert all(r.tobytes() in have for r in table[:, g])          # row o g
        assert all(r.tobytes() in have for r in g[table])             # g o row
    inv = np.argsort(table, axis=1).astype(np.int32)
    assert all(r.tobytes() in have for r in inv)


@pytest.mark.parametrize('name', NAMES)
def test_peak_frontier_is_K(name):
    colour, bonds, K, _ = ar.graph_and_table(name)
    assert ar.peak_frontier(colour, bonds) == (K, K)


@pytest.mark.parametrize('name', NAMES)
def test_networkx_finds_the_same_set(name):
    nx = pytest.importorskip('networkx')
    from networkx.algorithms.isomorphism import GraphMatcher
    colour, bonds, K, table = ar.graph_and_table(name)
    G = nx.Graph()
    G.add_nodes_from((a, dict(colour=int(c))) for a, c in enumerate(colour))
    G.add_edges_from(bonds.T.tolist())
    gm = GraphMatcher(G, G, node_match=lambda a, b: a['colour'] == b['colour'])
    rows = np.array([[mp[a] for a in range(len(colour))] for mp in gm.isomorphisms_iter()], np.int32)
    assert ar.same_set(rows, table)


def test_mask_cases():
    """masked-out atoms are not part of the graph whatever their colour; kept, an odd atom breaks the symmetry"""
    colour, bonds = ar.hexagon_with_hydrogens()
    t = ar.automorphisms_ref(colour, bonds, colour != 0)
    assert t.shape == (12, 12) and (t[:, 6:] == np.arange(6, 12)).all()
    assert ar.same_set(t[:, :6], ar.graph_and_table('hexagon')[3])
    colour2, _ = ar.hexagon_with_hydrogens(odd=True)
    heavy_ring = np.arange(12) < 6
    assert ar.same_set(ar.automorphisms_ref(colour2, bonds, heavy_ring), t)
    t2 = ar.automorphisms_ref(colour2, bonds, colour2 != 0)
    assert t2.shape == (2, 12)
    # here the frontier is NOT bounded by K: the ring is matched before the odd atom is reached (the GPU test sizes its capacity by this peak)
    assert ar.peak_frontier(colour2, bonds, colour2 != 0) == (8, 2)
    assert len(ar.automorphisms_ref(colour, bonds)) == 12          # with the hydrogens in the graph: the ring group acting on both


def test_input_form_and_relabelling():
    colour, bonds, K, table = ar.graph_and_table('c6_c3_c3')
    both = np.concatenate([bonds, bonds[::-1]], axis=1)
    dup = np.concatenate([bonds, bonds[:, :5], bonds[::-1][:, 3:9]], axis=1)
    assert ar.same_set(ar.automorphisms_ref(colour, both), table) and ar.same_set(ar.automorphisms_ref(colour, dup), table)
    relabel = np.random.default_rng(1).permutation(len(colour))
    c2, b2, _ = ar.relabelled(colour, bonds, None, relabel)
    assert ar.same_set(ar.automorphisms_ref(c2, b2), ar.conjugate(table, relabel))
    with pytest.raises(ValueError):
        ar.automorphisms_ref(colour, np.array([[0], [12]]))
