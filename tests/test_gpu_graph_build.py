"""The three table builders of csrc/k_build.hip through the raw C ABI (ddk_receptor_knn_graph, ddk_radius_graph, ddk_ligand_transformation_mask) against
the numpy restatements of tests/graph_build_ref.py, exactly: counts, order and every entry (tests/test_graph_build_host.py checks the restatements and
the margins of the random inputs on the CPU).  Every output is pre-filled with a sentinel and has guard columns / rows behind its cap, and the workspace
starts as garbage.  Rows far above a wave's 64 lanes and above 1024 items: dense_ball (24 of 1499), cap_1024 (quota 1025) and path256."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import graph_build_ref as gb

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SENTINEL, GUARD = -77, 64


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


def _edges(ctx, dev, which, pos, r, k, cap=None, n=None, null=None):
    """call 1 ('knn') or 2 ('radius') -> (edge_index_out with its guard [2 * cap + GUARD] int32, count_out [2], cap) on the host"""
    pos = np.ascontiguousarray(pos, np.float32)
    n = len(pos) if n is None else n
    if cap is None:
        cap = n * k if which == 'knn' else n * (k + 1)
    d_pos = T(pos).to(dev)
    out = torch.full((2 * max(cap, 0) + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    query, call = ((ctx.L.ddk_receptor_knn_graph_workspace, ctx.L.ddk_receptor_knn_graph) if which == 'knn' else
                   (ctx.L.ddk_radius_graph_workspace, ctx.L.ddk_radius_graph))
    ws = torch.full((max(query(n, k), 16),), 0xA5, dtype=torch.uint8, device=dev)
    p = dict(pos=_ptr(d_pos), out=_ptr(out), count=_ptr(count), ws=_ptr(ws))
    if null:
        p[null] = None
    ctx._check(call(ctx.h, n, p['pos'], float(r), k, p['out'], cap, p['count'], p['ws'], _stream()), 'ddk_' + which)
    return out.cpu().numpy(), count.cpu().numpy(), cap


def _check_edges(out, count, cap, want, status=0):
    E = want.shape[1]
    assert count.tolist() == [E, status], count
    assert np.array_equal(out[:E], want[0]) and np.array_equal(out[cap:cap + E], want[1])
    assert (out[E:cap] == SENTINEL).all() and (out[cap + E:] == SENTINEL).all()          # the unused columns and the guard


def _mask(ctx, dev, n_lig, bi, cap_rot=None, M=None, null=None):
    """call 3 -> (edge_mask_out [M + GUARD], mask_rotate_out [cap_rot + GUARD, n_lig], count_out [2]) on the host"""
    bi = np.ascontiguousarray(bi, np.int32).reshape(2, -1)
    M = bi.shape[1] if M is None else M
    cap_rot = max(M // 2, 1) if cap_rot is None else cap_rot
    d_b = T(bi).to(dev) if bi.size else None
    em = torch.full((M + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    mr = torch.full((max(cap_rot, 0) + GUARD, n_lig), 0xEE, dtype=torch.uint8, device=dev)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.full((max(ctx.L.ddk_ligand_transformation_mask_workspace(n_lig, M), 16),), 0xA5, dtype=torch.uint8, device=dev)
    p = dict(em=_ptr(em), mr=_ptr(mr), count=_ptr(count), ws=_ptr(ws))
    if null:
        p[null] = None
    ctx._check(ctx.L.ddk_ligand_transformation_mask(ctx.h, n_lig, _ptr(d_b), M, p['em'], p['mr'], cap_rot, p['count'], p['ws'], _stream()),
               'ddk_ligand_transformation_mask')
    return em.cpu().numpy(), mr.cpu().numpy(), count.cpu().numpy()


def _check_mask(em, mr, count, M, want_e, want_r, status=0, R=None):
    R = len(want_r) if R is None else R
    assert count.tolist() == [R, status], count
    assert np.array_equal(em[:M], want_e) and (em[M:] == 0xEE).all()
    assert np.array_equal(mr[:len(want_r)], want_r) and (mr[len(want_r):] == 0xEE).all()          # rows past R and the guard are not touched


@pytest.fixture(scope='module')
def knn_refs():
    return {name: gb.knn_graph_ref(*case)[0] for name, case in gb.knn_cases().items()}


@pytest.fixture(scope='module')
def radius_refs():
    return {name: gb.radius_graph_ref(*case)[0] for name, case in gb.radius_cases().items()}


@pytest.mark.parametrize('name', tuple(gb.knn_cases()))
def test_knn_cases(dev, ctx, knn_refs, name):
    pos, cutoff, k = gb.knn_cases()[name]
    out, count, cap = _edges(ctx, dev, 'knn', pos, cutoff, k)
    _check_edges(out, count, cap, knn_refs[name])


@pytest.mark.parametrize('name', tuple(gb.radius_cases()))
def test_radius_cases(dev, ctx, radius_refs, name):
    pos, r, k = gb.radius_cases()[name]
    out, count, cap = _edges(ctx, dev, 'radius', pos, r, k)
    _check_edges(out, count, cap, radius_refs[name])


@pytest.mark.parametrize('name', tuple(gb.ligand_cases()))
def test_ligand_cases(dev, ctx, name):
    n, bi = gb.ligand_cases()[name]
    want_e, want_r, status = gb.transformation_mask_ref(n, bi)
    assert status == 0
    _check_mask(*_mask(ctx, dev, n, bi), bi.shape[1], want_e, want_r)


def test_knn_3000_residues(dev, ctx):
    pos = gb.random_residues(3000, 1)
    out, count, cap = _edges(ctx, dev, 'knn', pos, 15.0, 24)
    _check_edges(out, count, cap, gb.knn_graph_ref(pos, 15.0, 24)[0])


def test_radius_8000_atoms(dev, ctx):
    pos = gb.protein_atoms(8000, 3)
    out, count, cap = _edges(ctx, dev, 'radius', pos, 5.0, 8)
    want = gb.radius_graph_ref(pos, 5.0, 8)[0]
    assert np.bincount(want[1]).max() == 9          # the quirk is there at this density
    _check_edges(out, count, cap, want)


def test_two_runs_are_bit_identical(dev, ctx):
    pos, cutoff, k = gb.knn_cases()['dense_ball']
    a, b = _edges(ctx, dev, 'knn', pos, cutoff, k), _edges(ctx, dev, 'knn', pos, cutoff, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    pos, r, k = gb.radius_cases()['atoms_300']
    a, b = _edges(ctx, dev, 'radius', pos, r, k), _edges(ctx, dev, 'radius', pos, r, k)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    n, bi = gb.ligand_cases()['make_ligand_3']
    a, b = _mask(ctx, dev, n, bi), _mask(ctx, dev, n, bi)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_status_codes(dev, ctx, radius_refs):
    lat = gb.lattice(3)
    for bad in (gb.with_nan(lat), gb.with_inf(lat), gb.with_nan(lat, len(lat) - 1)):          # status 2: E = 0 and nothing is written
        for which, k in (('knn', 24), ('radius', 8)):
            out, count, cap = _edges(ctx, dev, which, bad, 15.0 if which == 'knn' else 5.0, k)
            assert count.tolist() == [0, 2] and (out == SENTINEL).all()
    # radius status 1: the E the graph needs is reported, nothing past cap columns is written
    pos, r, k = gb.radius_cases()['atoms_300']
    want = radius_refs['atoms_300']
    E = want.shape[1]
    for cap in (E - 1, 7, 1):
        out, count, _ = _edges(ctx, dev, 'radius', pos, r, k, cap=cap)
        assert count.tolist() == [E, 1]
        assert (out[2 * cap:] == SENTINEL).all()
        assert np.array_equal(out[:cap], want[0][:cap]) and np.array_equal(out[cap:2 * cap], want[1][:cap])
    out, count, cap = _edges(ctx, dev, 'radius', pos, r, k, cap=E)          # exactly enough
    _check_edges(out, count, cap, want)
    # mask status 1: R reported, edge_mask all 0, mask_rotate not touched
    n, bi = gb.ligand_cases()['make_ligand_1']
    want_e, want_r, _ = gb.transformation_mask_ref(n, bi)
    R = len(want_r)
    assert R >= 2
    em, mr, count = _mask(ctx, dev, n, bi, cap_rot=R - 1)
    _check_mask(em, mr, count, bi.shape[1], np.zeros_like(want_e), want_r[:0], status=1, R=R)
    _check_mask(*_mask(ctx, dev, n, bi, cap_rot=R), bi.shape[1], want_e, want_r)
    # mask statuses 2 and 3
    for name, (n, bi, status) in gb.broken_ligands().items():
        em, mr, count = _mask(ctx, dev, n, bi)
        _check_mask(em, mr, count, bi.shape[1], np.zeros(bi.shape[1], np.uint8), np.zeros((0, n), np.uint8), status=status)


def test_refusals(dev, ctx):
    lat = gb.lattice(3)
    big = np.zeros((65537, 3), np.float32)
    with pytest.raises(RuntimeError, match=r'n must be in \[2, 65536\]'):
        _edges(ctx, dev, 'knn', lat[:1], 15.0, 24)
    with pytest.raises(RuntimeError, match=r'n must be in \[2, 65536\]'):
        _edges(ctx, dev, 'knn', big, 15.0, 24, cap=65537 * 24)
    with pytest.raises(RuntimeError, match=r'max_neighbor must be in \[1, 128\]'):
        _edges(ctx, dev, 'knn', lat, 15.0, 129)
    with pytest.raises(RuntimeError, match=r'cap must be at least n \* max_neighbor = 648'):
        _edges(ctx, dev, 'knn', lat, 15.0, 24, cap=27 * 24 - 1)
    with pytest.raises(RuntimeError, match=r'n must be in \[1, 65536\]'):
        _edges(ctx, dev, 'radius', big, 5.0, 8, cap=16)
    with pytest.raises(RuntimeError, match=r'n must be in \[1, 65536\]'):
        _edges(ctx, dev, 'radius', lat, 5.0, 8, n=0, cap=16)
    with pytest.raises(RuntimeError, match=r'max_num_neighbors must be in \[1, 1024\]'):
        _edges(ctx, dev, 'radius', lat, 5.0, 1025, cap=16)
    with pytest.raises(RuntimeError, match=r'cap must be >= 1'):
        _edges(ctx, dev, 'radius', lat, 5.0, 8, cap=0)
    for which in ('knn', 'radius'):
        for null in ('pos', 'out', 'count', 'ws'):
            with pytest.raises(RuntimeError, match='null argument'):
                _edges(ctx, dev, which, lat, 5.0, 8, null=null)
    n, bi = gb.ligand_cases()['path4']
    with pytest.raises(RuntimeError, match=r'n_lig must be in \[1, 256\]'):
        _mask(ctx, dev, 257, bi)
    with pytest.raises(RuntimeError, match=r'M must be even'):
        _mask(ctx, dev, n, bi, M=5)
    with pytest.raises(RuntimeError, match=r'M must be even'):
        _mask(ctx, dev, n, bi, M=2050)
    with pytest.raises(RuntimeError, match=r'cap_rot must be >= 1'):
        _mask(ctx, dev, n, bi, cap_rot=0)
    for null in ('em', 'mr', 'count', 'ws'):
        with pytest.raises(RuntimeError, match='null argument'):
            _mask(ctx, dev, n, bi, null=null)
    out, count, cap = _edges(ctx, dev, 'knn', lat, 15.0, 24)          # the context is usable afterwards
    _check_edges(out, count, cap, gb.knn_graph_ref(lat, 15.0, 24)[0])


def test_context_methods(dev, ctx):
    """the Python layer: trimmed device tensors, ValueError on bad input, a warning and no torsion for a ligand that is not connected"""
    pos, cutoff, k = gb.knn_cases()['isolated']
    ei = ctx.receptor_knn_graph(pos, cutoff, k)
    assert ei.is_cuda and ei.dtype == torch.int32 and np.array_equal(ei.cpu().numpy(), gb.knn_graph_ref(pos, cutoff, k)[0])
    pos, r, k = gb.radius_cases()['coincident']
    ei = ctx.radius_graph(T(pos).to(dev), r, k)
    assert ei.is_cuda and np.array_equal(ei.cpu().numpy(), gb.radius_graph_ref(pos, r, k)[0])
    n, bi = gb.ligand_cases()['bridge']
    em, mr = ctx.transformation_mask(n, bi)
    want_e, want_r, _ = gb.transformation_mask_ref(n, bi)
    assert em.is_cuda and em.dtype == torch.uint8 and np.array_equal(em.cpu().numpy(), want_e) and np.array_equal(mr.cpu().numpy(), want_r)
    em, mr = ctx.transformation_mask(1, np.zeros((2, 0), np.int64))
    assert em.shape == (0,) and mr.shape == (0, 1)
    with pytest.raises(ValueError, match='not finite'):
        ctx.receptor_knn_graph(gb.with_nan(gb.lattice(3)))
    with pytest.raises(ValueError, match='not finite'):
        ctx.radius_graph(gb.with_inf(gb.lattice(3)))
    broken = gb.broken_ligands()
    with pytest.raises(ValueError, match='repeated'):
        ctx.transformation_mask(*broken['repeated'][:2])
    with pytest.warns(UserWarning, match='status 3'):
        em, mr = ctx.transformation_mask(*broken['counter_ion'][:2])
    assert not em.any() and mr.shape == (0, 7)
    with pytest.raises(RuntimeError, match=r'n must be in \[2, 65536\]'):
        ctx.receptor_knn_graph(np.zeros((1, 3), np.float32))


TABLES = ('rec_edge_index', 'edge_mask', 'mask_rotate', 'atom_edge_index')
ATOM_CAP = 64          # a max_num_neighbors that never binds on the synthetic receptor atoms: there add_receptor_atoms and radius_graph are the same graph


def test_end_to_end_score_model(dev):
    """a config-2 sized synthetic complex with its three tables deleted -> graphs.complete_complex -> the deleted arrays, and one score_forward with the
    bits of the complex built from the host tables"""
    from disco_diffdock_amd import graphs, synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    full = synthetic.make_complex(2, n_res=300)
    ctx = Context(device=0, deterministic=1)          # the mode in which a forward's bits are defined run to run
    ctx.load_state_dict(synthetic.random_score_model_state_dict(seed=1))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        built = graphs.complete_complex({k: v for k, v in full.items() if k not in TABLES}, ctx=ctx)
    for k in TABLES[:3]:
        assert np.array_equal(built[k], full[k]) and built[k].dtype == full[k].dtype, k
    assert 'atom_edge_index' not in built
    B = 2
    pos = T(np.stack([full['lig_pos'], full['lig_pos'] + 1.0]).astype(np.float32)).to(dev)
    outs = []
    for c in (full, built):
        cx = Complex(ctx, c, B)
        outs.append([o.clone() for o in cx.score_forward(pos, 0.5, 0.5, 0.5)])
        cx.close()
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    ctx.close()


def test_end_to_end_confidence_model(dev):
    """the same with the receptor atoms: all four tables, and one confidence_forward of the all-atom model.  With the default max_num_neighbors = 8 the
    atom graph is torch_cluster's (oracle/cluster_lite.py), which keeps nine neighbours where add_receptor_atoms keeps eight
    (tests/test_graph_build_host.py); where the cap does not bind the generator's array comes back exactly."""
    from disco_diffdock_amd import graphs, synthetic
    from disco_diffdock_amd.runtime import Context, Complex
    from oracle import cluster_lite
    full = synthetic.add_receptor_atoms(synthetic.make_complex(2, n_res=40), np.random.default_rng(102), atom_max_neighbors=ATOM_CAP)
    ctx = Context(device=0, all_atoms=1, num_confidence_outputs=2)
    ctx.load_state_dict(synthetic.random_confidence_state_dict(seed=3))
    bare = {k: v for k, v in full.items() if k not in TABLES}
    built = graphs.complete_complex(dict(bare), ctx=ctx, atom_max_neighbors=ATOM_CAP)
    for k in TABLES:
        assert np.array_equal(built[k], full[k]) and built[k].dtype == full[k].dtype, k
    built8 = graphs.complete_complex(dict(bare), ctx=ctx)
    host8 = dict(full, atom_edge_index=cluster_lite.radius_graph(T(full['atom_pos']), 5.0, max_num_neighbors=8).numpy())
    assert np.array_equal(built8['atom_edge_index'], host8['atom_edge_index'])
    pos = T(np.stack([full['lig_pos'], full['lig_pos'] + 1.0]).astype(np.float32)).to(dev)

    def forward(c):
        cx = Complex(ctx, c, 2)
        cx.set_atoms(c['atom_x'], c['atom_pos'], c['atom_edge_index'], c['atom_rec_index'])
        out = cx.confidence_forward(pos).clone()
        cx.close()
        return out

    for host, device in ((full, built), (host8, built8)):
        # what the forward reads of the two complexes is the same bytes
        assert all(np.asarray(host[k], np.int32).tobytes() == np.asarray(device[k], np.int32).tobytes() for k in ('rec_edge_index', 'atom_edge_index'))
        assert all(np.asarray(host[k], np.uint8).tobytes() == np.asarray(device[k], np.uint8).tobytes() for k in ('edge_mask', 'mask_rotate'))
        # the all-atom model has no deterministic mode (its ligand-atom edges take their slots from an atomic cursor and its conv scatters with float
        # atomics), so "the bits of the host complex" are defined up to its own run-to-run spread: three forwards of the host complex measure it.  Where
        # they agree the device-built complex must give those bits; else it must stay within 8 x that spread, and never beyond 1e-5 relative (a dozen fp32
        # roundings of reordered sums; the suite holds this model to 1e-4 against the oracle).
        h = [forward(host) for _ in range(3)]
        d = forward(device)
        assert torch.isfinite(d).all()
        spread = max(float((a - b).abs().max()) for a in h for b in h)
        err = float((d - h[0]).abs().max())
        print(f'confidence forward: host run-to-run spread {spread:.3e}, device-built vs host {err:.3e}')
        if spread == 0.0:
            assert torch.equal(d, h[0])
        assert err <= min(8.0 * spread, 1e-5 * max(1.0, float(h[0].abs().max())))
    ctx.close()
