"""From coordinates, bonds and features to a complete complex dict: the static graph tables of SURVEY.md Appendix B.1 that the reference's data pipeline
builds on the host (get_calpha_graph, radius_graph, get_transformation_mask) come from the device builders of csrc/k_build.hip instead, and the
matched conformer of get_lig_graph_with_matching from the device search of csrc/k_match.hip."""
import numpy as np


def _host(t, dtype):
    return t.cpu().numpy().astype(dtype)


def complete_complex(c, ctx=None, cutoff=15.0, max_neighbor=24, atom_radius=5.0, atom_max_neighbors=8):
    """Fills whichever of ``rec_edge_index`` (from ``rec_pos``), ``edge_mask`` + ``mask_rotate`` (from ``bond_index`` and the atom count of ``lig_x``) and,
    when ``atom_pos`` is present, ``atom_edge_index`` are missing from the complex dict ``c`` (the keys of ``synthetic.make_complex`` /
    ``synthetic.add_receptor_atoms``), in place, and returns it.  A key that is present is never recomputed (``edge_mask`` and ``mask_rotate`` are a
    pair: both are written when either is missing).  The new arrays are numpy, in the dtypes of the generators (int64 indices, bool masks), which
    ``runtime.Complex``, ``Complex.set_atoms`` and ``graph_cache.save_complexes`` take.  ctx: a ``runtime.Context`` (None: the weightless context of
    device 0)."""
    if ctx is None:
        from .tensor_layers import _shape_context
        ctx = _shape_context(0)
    if 'rec_edge_index' not in c:
        c['rec_edge_index'] = _host(ctx.receptor_knn_graph(np.asarray(c['rec_pos'], np.float32), cutoff, max_neighbor), np.int64)
    if 'edge_mask' not in c or 'mask_rotate' not in c:
        edge_mask, mask_rotate = ctx.transformation_mask(len(c['lig_x']), np.asarray(c['bond_index']))
        c['edge_mask'], c['mask_rotate'] = _host(edge_mask, bool), _host(mask_rotate, bool)
    if 'atom_pos' in c and 'atom_edge_index' not in c:
        c['atom_edge_index'] = _host(ctx.radius_graph(np.asarray(c['atom_pos'], np.float32), atom_radius, atom_max_neighbors), np.int64)
    return c


def match_conformer(c, conformer_pos, ctx=None, heavy_only=None, **options):
    """get_lig_graph_with_matching (datasets_utils/process_mols.py:280-311) for a complex dict: ``c['lig_pos']`` is the true pose, ``conformer_pos``
    [n_lig, 3] a generated conformer of the same ligand (same atom order).  Fits the conformer's torsions to the true pose on the device
    (``Context.match_conformer``; the rotors are ``c['bond_index'][:, c['edge_mask']]`` and ``c['mask_rotate']``) and writes, in place: ``c['orig_pos']`` =
    the true pose (keep_original), ``c['orig_rdkit_pos']`` = the conformer as given, ``c['lig_pos']`` = the matched conformer in the true pose's frame,
    ``c['rmsd_matching']`` (float); returns ``c``.  ``heavy_only``: a mask [n_lig] of the atoms that enter the fit and the RMSD (the reference matches after
    RemoveHs; None: all atoms).  ``options``: popsize, maxiter, polish_iters, n_islands, seed, tol and stream of ``Context.match_conformer``; with
    ``stream=None`` (the default here) the stream id is ``runtime.stream_id(c['name'])``, as in sampling.  One read-back (the result)."""
    from .runtime import MATCH_STATUS, stream_id
    if ctx is None:
        from .tensor_layers import _shape_context
        ctx = _shape_context(0)
    if options.get('stream') is None:
        if c.get('name') is None:
            raise ValueError("ddk: match_conformer needs a complex with a name (its stream id is runtime.stream_id(name)) or an explicit stream")
        options['stream'] = stream_id(c['name'])
    true_pos = np.asarray(c['lig_pos'], np.float32)
    conformer_pos = np.asarray(conformer_pos, np.float32).reshape(-1, 3)
    if conformer_pos.shape != true_pos.shape:
        raise ValueError(f'ddk: the conformer has shape {conformer_pos.shape}, the true pose {true_pos.shape}')
    rot_bonds = np.asarray(c['bond_index']).T[np.asarray(c['edge_mask'], bool)].reshape(-1, 2)
    out = ctx.match_conformer(conformer_pos, true_pos, rot_bonds, np.asarray(c['mask_rotate']), atom_mask=heavy_only, **options)
    status = int(out['status'])
    if status != 0:
        raise RuntimeError(f"ddk: conformer matching of {c.get('name')!r} refused its input (status {status}: {MATCH_STATUS[status]})")
    c['orig_pos'], c['orig_rdkit_pos'] = true_pos, conformer_pos
    c['lig_pos'] = _host(out['pos'], np.float32)
    c['rmsd_matching'] = float(out['rmsd'])
    return c
