"""ddk_randomize_position_batch (csrc/k_se3.hip; ar_training.randomize_position_batch): random start poses for G DIFFERENT ligands in one launch.  The
contract: graph g's pose is BIT FOR BIT what ddk_rng_initial + ddk_randomize_position (sampling.randomize_position(seed=...)) give that ligand alone at the
same (seed, stream, sample), whatever else is in the batch and wherever the graph stands in it.  Three complexes of tests/noise_batch_ref.py's standing batch:
19 atoms / 7 rotors, 16 atoms / no rotor, 20 atoms / 1 rotor.  A bad table is tested through its documented status only: the kernel checks every entry
before it becomes an address."""
import numpy as np
import pytest
import torch

import noise_batch_ref as nb

pytestmark = pytest.mark.gpu
SEED, SIGMA = 41, 19.0


@pytest.fixture(scope='module')
def ctx():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return _shape_context(0)


@pytest.fixture(scope='module')
def complexes():
    cs = nb.standing_batch()[1:]
    assert nb.rotor_counts(cs) == [7, 0, 1] and [len(c['lig_pos']) for c in cs] == [19, 16, 20]
    return cs


def _bits(t):
    return t.detach().contiguous().float().cpu().view(torch.int32)


_alone = {}


def _pose_alone(c, sample, no_torsion=False):
    """sampling.randomize_position on the complex by itself: one ddk_rng_initial and one ddk_randomize_position launch; computed once per (complex, sample)"""
    key = (c['name'], sample, no_torsion)
    if key not in _alone:
        from disco_diffdock_amd.data import from_arrays
        from disco_diffdock_amd.sampling import randomize_position
        dl = [from_arrays(c)]
        randomize_position(dl, no_torsion, False, SIGMA, unbatched=True, device=torch.device('cuda:0'), seed=SEED, sample_offset=sample)
        _alone[key] = _bits(dl[0]['ligand'].pos)
    return _alone[key]


def _split(pos, cs):
    return torch.split(pos, [len(c['lig_pos']) for c in cs])


@pytest.mark.parametrize('order,samples', [((0, 1, 2), (0, 5, 2)), ((2, 0, 1), (2, 0, 5)), ((1, 0, 0, 2), (5, 0, 3, 2))])
def test_every_graph_gets_the_bits_of_its_ligand_alone(ctx, complexes, order, samples):
    """two batch orders, and one batch in which a complex appears twice at different samples"""
    from disco_diffdock_amd import ar_training
    cs = [complexes[i] for i in order]
    pos = ar_training.randomize_position_batch(ctx, cs, SEED, samples, SIGMA)
    assert pos.is_cuda and tuple(pos.shape) == (sum(len(c['lig_pos']) for c in cs), 3) and bool(torch.isfinite(pos).all())
    for g, (c, s, mine) in enumerate(zip(cs, samples, _split(pos, cs))):
        assert torch.equal(_bits(mine), _pose_alone(c, s)), (g, c['name'], s)
    if len(order) == 4:      # the same complex at two samples: two different poses
        assert not torch.equal(_bits(_split(pos, cs)[1]), _bits(_split(pos, cs)[2]))


def test_no_torsion_draws_no_torsions(ctx, complexes):
    from disco_diffdock_amd import ar_training
    samples = (1, 2, 3)
    pos = ar_training.randomize_position_batch(ctx, complexes, SEED, samples, SIGMA, no_torsion=True)
    full = ar_training.randomize_position_batch(ctx, complexes, SEED, samples, SIGMA)
    for g, (c, s, mine, other) in enumerate(zip(complexes, samples, _split(pos, complexes), _split(full, complexes))):
        assert torch.equal(_bits(mine), _pose_alone(c, s, no_torsion=True)), g
        assert torch.equal(_bits(mine), _bits(other)) == (nb.rotor_counts([c])[0] == 0), g      # only the ligand without rotors is unchanged
        # rigid: every pairwise distance of the true pose is kept
        p0, p1 = torch.as_tensor(np.asarray(c['lig_pos'], np.float32)), mine.cpu()
        assert float((torch.cdist(p0, p0) - torch.cdist(p1, p1)).abs().max()) < 1e-4


def test_a_bad_bond_gives_its_status_and_the_others_are_written(ctx, complexes):
    """graph 0's second rotor bond names atom n_0 (one past its ligand): status 2, its rows of pos_out keep the sentinel; graphs 1 and 2 are as in the clean
    batch.  Then a tor_ptr entry past T: status 4."""
    from disco_diffdock_amd import ar_training
    from disco_diffdock_amd.runtime import CONFORMER_BATCH_STATUS
    samples = np.asarray((0, 5, 2), np.int32)
    streams, pos, node_ptr, tor_ptr, mask_ptr, bonds, masks = ar_training._ligand_tables(complexes, False, 'test')
    clean, status = ctx.randomize_position_batch(SEED, pos, node_ptr, bonds, masks, mask_ptr, tor_ptr, torch.from_numpy(streams), samples, SIGMA, return_status=True)
    assert status.tolist() == [0, 0, 0]
    for g, (c, s, mine) in enumerate(zip(complexes, samples.tolist(), _split(clean, complexes))):
        assert torch.equal(_bits(mine), _pose_alone(c, s)), g
    bad = bonds.copy()
    bad[1, 0] = len(complexes[0]['lig_pos'])
    out, status = ctx.randomize_position_batch(SEED, pos, node_ptr, bad, masks, mask_ptr, tor_ptr, torch.from_numpy(streams), samples, SIGMA, return_status=True)
    assert status.tolist() == [2, 0, 0] and CONFORMER_BATCH_STATUS[2].startswith('a bond index')
    for g in (1, 2):
        assert torch.equal(_bits(_split(out, complexes)[g]), _bits(_split(clean, complexes)[g])), g
    # a sentinel shows that graph 0 is not written: the same call through the C entry with a filled pos_out
    import ctypes as C
    from disco_diffdock_amd.runtime import _ptr, _stream
    dev = torch.device('cuda:0')
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    d_pos, d_node, d_bad, d_masks, d_mp, d_tp = d(pos, torch.float32), d(node_ptr, torch.int32), d(bad, torch.int32), d(masks, torch.uint8), d(mask_ptr, torch.int32), d(tor_ptr, torch.int32)
    d_st, d_sa = d(streams, torch.int64), d(samples, torch.int32)
    filled = torch.full_like(d_pos, -7.0)
    st = torch.full((3,), -7, dtype=torch.int32, device=dev)
    rc = ctx.L.ddk_randomize_position_batch(ctx.h, C.c_uint64(SEED), 3, d_pos.shape[0], _ptr(d_pos), _ptr(d_node), int(tor_ptr[-1]), _ptr(d_bad), _ptr(d_masks),
                                            _ptr(d_mp), d_masks.numel(), _ptr(d_tp), _ptr(d_st), _ptr(d_sa), SIGMA, _ptr(filled), _ptr(st), _stream())
    assert rc == 0 and st.tolist() == [2, 0, 0]
    parts = _split(filled, complexes)
    assert bool((parts[0] == -7.0).all()) and torch.equal(_bits(parts[1]), _bits(_split(clean, complexes)[1]))
    tp_bad = tor_ptr.copy()
    tp_bad[3] = tor_ptr[3] + 1      # graph 2's rotors would end past T
    d_tpb = d(tp_bad, torch.int32)
    filled.fill_(-7.0)
    rc = ctx.L.ddk_randomize_position_batch(ctx.h, C.c_uint64(SEED), 3, d_pos.shape[0], _ptr(d_pos), _ptr(d_node), int(tor_ptr[-1]), _ptr(d(bonds, torch.int32)),
                                            _ptr(d_masks), _ptr(d_mp), d_masks.numel(), _ptr(d_tpb), _ptr(d_st), _ptr(d_sa), SIGMA, _ptr(filled), _ptr(st), _stream())
    assert rc == 0 and st.tolist() == [0, 0, 4]
    parts = _split(filled, complexes)
    assert bool((parts[2] == -7.0).all()) and torch.equal(_bits(parts[0]), _bits(_split(clean, complexes)[0]))


def test_host_checks_raise_before_anything_is_uploaded(ctx, complexes):
    from disco_diffdock_amd import ar_training
    broken = dict(complexes[0])
    bi = np.array(broken['bond_index'], copy=True)
    em = np.asarray(broken['edge_mask']).astype(bool)
    bi[0, np.flatnonzero(em)[0]] = 99
    broken['bond_index'] = bi
    with pytest.raises(ValueError, match='rotatable bond'):
        ar_training.randomize_position_batch(ctx, [broken], SEED, [0], SIGMA)
    with pytest.raises(ValueError, match='samples'):
        ar_training.randomize_position_batch(ctx, complexes, SEED, [0, -1, 2], SIGMA)
    with pytest.raises(ValueError, match='name'):
        ar_training.randomize_position_batch(ctx, [{k: v for k, v in complexes[0].items() if k != 'name'}], SEED, [0], SIGMA)
