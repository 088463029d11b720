"""The ligand automorphism enumeration on the device (csrc/k_autos.hip) through the C ABI, ddk_ligand_automorphisms, against the plain backtracking search
of tests/automorphism_ref.py (tests/test_automorphism_host.py checks that one on the CPU, against networkx too).  Tables are compared as SETS of rows
(sorted on the host), row 0 exactly with the identity; every output is pre-filled with a sentinel, perms_out has a guard region behind its cap rows and the
workspace starts as garbage.  cap = 2 K for the named graphs, on which the search never holds more than K partial maps (checked on the CPU); where the
peak is above K (a kept odd atom, a relabelled graph) cap = 2 * the reference's peak_frontier.

The graphs sit on the search's paths (runtime.AUTOS_*): cap * n_lig <= 16384 is one workgroup's walk alone (one_atom ... cubane, path256 with its 256 levels
and atom 255 in a uint8 row); c6_c3_c3, cf3_x4 and cf3_x5 have levels of more than 1024 (row, candidate) items, which take the launch pairs and the scan
across workgroups (cf3_x5: up to 7776 rows x 4 candidates = 122 workgroup chunks); the project ligands run at the default cap, where every level small
enough stays in the walk and the pairs find nothing to do."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import automorphism_ref as ar

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL, GUARD_ROWS = -77, 64


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ctx(dev):
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(a, dt, dev):
    return None if a is None else T(np.ascontiguousarray(a, dt)).to(dev)


def _raw(ctx, dev, colour, bonds, mask=None, cap=1, n_lig=None, null_colour=False):
    """ddk_ligand_automorphisms through the C ABI -> (perms_out with its guard rows [cap + GUARD_ROWS, n_lig], count_out [2]) on the host"""
    n = len(colour) if n_lig is None else n_lig
    E = 0 if bonds is None else np.asarray(bonds).shape[1]
    d_c, d_b, d_m = _up(colour, np.int32, dev), (_up(bonds, np.int32, dev) if E else None), _up(mask, np.uint8, dev)
    out = torch.full((max(cap, 0) + GUARD_ROWS, n), SENTINEL, dtype=torch.int32, device=dev)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    nbytes = ctx.L.ddk_ligand_automorphisms_workspace(n, cap)
    ws = torch.full((max(nbytes, 16),), 0xA5, dtype=torch.uint8, device=dev)
    ctx._check(ctx.L.ddk_ligand_automorphisms(ctx.h, n, None if null_colour else _ptr(d_c), _ptr(d_b), E, _ptr(d_m), _ptr(out), cap, _ptr(count), _ptr(ws),
                                              _stream()), 'ddk_ligand_automorphisms')
    return out.cpu().numpy(), count.cpu().numpy()


def _check_complete(out, count, want, cap):
    n = want.shape[1]
    K = len(want)
    assert count.tolist() == [K, 0], count
    assert np.array_equal(out[0], np.arange(n))
    assert ar.same_set(out[:K], want)
    assert (out[K:] == SENTINEL).all()          # the unused rows and the guard region


def _check_identity_only(out, count, status):
    assert count.tolist() == [1, status], count
    assert np.array_equal(out[0], np.arange(out.shape[1])) and (out[1:] == SENTINEL).all()


@pytest.mark.parametrize('name', tuple(ar.GRAPHS))
def test_named_graphs(dev, ctx, name):
    colour, bonds, K, want = ar.graph_and_table(name)
    assert len(colour) == ar.ATOMS[name] and len(want) == K
    cap = 2 * K
    out, count = _raw(ctx, dev, colour, None if name == 'no_bonds' else bonds, cap=cap)
    _check_complete(out, count, want, cap)


def test_paths_of_the_search_are_covered():
    from disco_diffdock_amd import runtime as rt
    size = {n: 2 * ar.GRAPHS[n]()[2] * ar.ATOMS[n] for n in ar.GRAPHS}
    assert all(size[n] <= rt.AUTOS_WALK_ONLY_ITEMS for n in ('one_atom', 'toluene', 'hexagon', 'star', 'no_bonds', 'cubane', 'path256'))
    assert all(size[n] > rt.AUTOS_WALK_ONLY_ITEMS for n in ('c6_c3_c3', 'cf3_x4', 'cf3_x5'))
    # their last levels: K rows x the parent's degree (2 in a ring, 4 at a CF3 carbon) is past the walk and more than one chunk
    assert rt.AUTOS_WALK_ITEMS < 864 * 2 < 1296 * 4 and 864 * 2 > 2 * rt.AUTOS_CHUNK


def test_mask(dev, ctx):
    colour, bonds = ar.hexagon_with_hydrogens()
    heavy = colour != 0
    want = ar.automorphisms_ref(colour, bonds, heavy)
    assert len(want) == 12
    out, count = _raw(ctx, dev, colour, bonds, heavy, cap=24)
    _check_complete(out, count, want, 24)
    assert (out[:12, 6:] == np.arange(6, 12)).all()          # the hydrogen columns are the identity
    colour2, _ = ar.hexagon_with_hydrogens(odd=True)
    ring = np.arange(12) < 6                                  # the odd atom masked out with the hydrogens: it breaks nothing
    out, count = _raw(ctx, dev, colour2, bonds, ring, cap=24)
    _check_complete(out, count, want, 24)
    kept_odd = colour2 != 0
    want2 = ar.automorphisms_ref(colour2, bonds, kept_odd)
    peak, K = ar.peak_frontier(colour2, bonds, kept_odd)
    assert K == len(want2) == 2
    out, count = _raw(ctx, dev, colour2, bonds, kept_odd, cap=2 * peak)
    _check_complete(out, count, want2, 2 * peak)


@pytest.mark.parametrize('name', ('toluene', 'c6_c3_c3', 'cf3_x4'))
def test_input_form(dev, ctx, name):
    colour, bonds, K, want = ar.graph_and_table(name)
    rng = np.random.default_rng(len(colour))
    both = np.concatenate([bonds, bonds[::-1]], axis=1)
    dup = np.concatenate([bonds, bonds[:, ::2], bonds[::-1][:, 1::3]], axis=1)[:, rng.permutation(bonds.shape[1] + len(bonds[0, ::2]) + len(bonds[0, 1::3]))]
    tables = [_raw(ctx, dev, colour, b, cap=2 * K) for b in (bonds, both, dup)]
    for out, count in tables:
        _check_complete(out, count, want, 2 * K)
    # the matching order reads the graph, not the columns: the same rows in the same order
    assert all(t[0].tobytes() == tables[0][0].tobytes() for t in tables)
    relabel = rng.permutation(len(colour))
    c2, b2, _ = ar.relabelled(colour, bonds, None, relabel)
    cap = 2 * ar.peak_frontier(c2, b2)[0]
    out, count = _raw(ctx, dev, c2, b2, cap=cap)
    _check_complete(out, count, ar.conjugate(want, relabel), cap)


def test_project_ligands(dev, ctx):
    """twenty ligands of synthetic.py, heavy-atom mask, through Complex.automorphisms() at its default cap"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Complex
    sizes = set()
    for seed in range(20):
        c = synthetic.make_complex(seed, n_res=30)
        cx = Complex(ctx, c, max_batch=1)
        perms, count = cx.automorphisms()
        assert perms.is_cuda and count.is_cuda and perms.shape == (65536, cx.n_lig) and cx.automorphisms()[0] is perms
        want = ar.automorphisms_ref(c['lig_x'][:, 0], c['bond_index'], c['lig_x'][:, 0] != 0)
        rows, status = count.cpu().tolist()
        assert status == 0 and rows == len(want)
        got = perms[:rows].cpu().numpy()
        assert np.array_equal(got[0], np.arange(cx.n_lig)) and ar.same_set(got, want)
        sizes.add(rows)
        cx.close()
    print('project ligands: table sizes', sorted(sizes))


@pytest.mark.parametrize('name', ('hexagon', 'c6_c3_c3', 'cf3_x4'))
def test_overflow_is_a_result(dev, ctx, name):
    colour, bonds, K, _ = ar.graph_and_table(name)
    out, count = _raw(ctx, dev, colour, bonds, cap=K - 1)
    _check_identity_only(out, count, 1)


def test_bad_bond_index_and_refusals(dev, ctx):
    colour, bonds, K, want = ar.graph_and_table('hexagon')
    for bad in (len(colour), -1):
        for where in ((0, 2), (1, 4)):
            b = bonds.copy()
            b[where] = bad
            out, count = _raw(ctx, dev, colour, b, cap=2 * K)
            _check_identity_only(out, count, 2)
    with pytest.raises(RuntimeError, match=r'n_lig must be in \[1, 256\]'):
        _raw(ctx, dev, np.zeros(257, np.int32), None, cap=4)
    with pytest.raises(RuntimeError, match=r'cap must be in \[1, 1048576\]'):
        _raw(ctx, dev, colour, bonds, cap=0)
    with pytest.raises(RuntimeError, match='null argument'):
        _raw(ctx, dev, colour, bonds, cap=4, null_colour=True)
    assert ctx.L.ddk_ligand_automorphisms_workspace(257, 4) < 0 and ctx.L.ddk_ligand_automorphisms_workspace(6, 0) < 0
    out, count = _raw(ctx, dev, colour, bonds, cap=2 * K)          # the context is usable afterwards
    _check_complete(out, count, want, 2 * K)


def test_two_calls_are_byte_identical(dev, ctx):
    colour, bonds, K, _ = ar.graph_and_table('cf3_x5')
    a, b = _raw(ctx, dev, colour, bonds, cap=2 * K), _raw(ctx, dev, colour, bonds, cap=2 * K)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].tolist() == [K, 0]


def _cf3_complex(ctx):
    """a complex whose ligand is the CF3 x 4 chain (22 atoms, K = 1296), with a conformer and the rest of a synthetic complex around it"""
    from disco_diffdock_amd import synthetic
    from disco_diffdock_amd.runtime import Complex
    colour, bonds, K, table = ar.graph_and_table('cf3_x4')
    n, pairs = len(colour), bonds.T.tolist()
    c = synthetic.make_complex(3, n_res=30, n_lig=22)
    edge_mask, mask_rotate = synthetic.transformation_mask(n, [tuple(p) for p in pairs])
    ei = np.zeros((2, 2 * len(pairs)), np.int64)
    ei[:, 0::2], ei[:, 1::2] = bonds, bonds[::-1]
    ea = np.zeros((2 * len(pairs), 4), np.float32)
    ea[:, 0] = 1.0
    x = np.zeros((n, c['lig_x'].shape[1]), np.int64)
    x[:, 0] = colour
    c.update(lig_x=x, bond_index=ei, bond_attr=ea, edge_mask=edge_mask, mask_rotate=mask_rotate, name='cf3_x4')
    c['lig_pos'] = c['lig_pos'][:n]
    return c, Complex(ctx, c, max_batch=8), table


def test_consumers(dev, ctx):
    """pose_metrics and pairwise_rmsd with the device table equal the same calls with the reference table bit for bit (a minimum does not depend on the row
    order); cluster_poses(perms='auto') equals cluster_poses(perms=<reference table>) integer for integer; with the capacity below K 'auto' warns and
    equals perms=None; perms=None is what it was before anything 'auto' ran"""
    from disco_diffdock_amd import sampling
    from disco_diffdock_amd.data import HeteroData
    c, cx, table = _cf3_complex(ctx)
    n, B = cx.n_lig, 8
    rng = np.random.default_rng(0)
    # poses that differ by turned CF3 groups and a little noise: the table decides which are the same mode
    pos = np.stack([c['lig_pos'][table[rng.integers(len(table))]] + rng.normal(0, 0.3 * (b % 3), size=(1, 3)) + rng.normal(0, 0.05, size=(n, 3))
                    for b in range(B)]).astype(np.float32)
    d_pos, ref = T(pos).to(dev), T(c['lig_pos']).to(dev)
    x = T(c['lig_x'])
    data_list = []
    for p in d_pos:
        g = HeteroData()
        g['ligand'].pos, g['ligand'].x = p, x
        g['ligand', 'lig_bond', 'ligand'].edge_index = T(c['bond_index'])
        g.name = 'cf3_x4'
        data_list.append(g)
    score = T(rng.normal(size=B).astype(np.float32)).to(dev)
    plain_metrics = cx.pose_metrics(d_pos, ref)
    plain_clusters = sampling.cluster_poses(data_list, confidence=score, ctx=ctx)

    perms, count = cx.automorphisms()
    assert count.cpu().tolist() == [len(table), 0]
    dev_table = perms[:len(table)]
    assert torch.equal(cx.pose_metrics(d_pos, ref, perms=dev_table), cx.pose_metrics(d_pos, ref, perms=table))
    assert torch.equal(cx.pose_metrics(d_pos, ref, perms='auto'), cx.pose_metrics(d_pos, ref, perms=table))
    assert torch.equal(ctx.pairwise_rmsd(d_pos, perms=dev_table), ctx.pairwise_rmsd(d_pos, perms=table))
    assert not torch.equal(ctx.pairwise_rmsd(d_pos, perms=dev_table), ctx.pairwise_rmsd(d_pos))          # the premise: the table matters for these poses
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        auto = sampling.cluster_poses(data_list, confidence=score, perms='auto', ctx=ctx)
    want = sampling.cluster_poses(data_list, confidence=score, perms=table, ctx=ctx)
    assert all(torch.equal(a, b) for a, b in zip(auto, want))
    with pytest.warns(UserWarning, match=r"ligand 'cf3_x4'.*status 1"):
        small = sampling.cluster_poses(data_list, confidence=score, perms='auto', auto_cap=len(table) - 1, ctx=ctx)
    assert all(torch.equal(a, b) for a, b in zip(small, plain_clusters))
    with pytest.warns(UserWarning, match=r"ligand 'cf3_x4'.*status 1"):
        assert torch.equal(cx.pose_metrics(d_pos, ref, perms='auto', auto_cap=100), plain_metrics)
    assert torch.equal(cx.pose_metrics(d_pos, ref), plain_metrics)
    assert all(torch.equal(a, b) for a, b in zip(sampling.cluster_poses(data_list, confidence=score, ctx=ctx), plain_clusters))
    cx.close()
