"""From coordinates, bonds and features to a complete complex dict: the static graph tables of SURVEY.md Appendix B.1 that the reference's data pipeline
builds on the host (get_calpha_graph, radius_graph, get_transformation_mask) come from the device builders of csrc/k_build.hip instead."""
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
