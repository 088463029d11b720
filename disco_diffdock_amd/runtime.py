"""Thin Python owner of a ddk context (include/ddk.h): config mapping, checkpoint upload, operator calls.
PyTorch is used only for device memory and streams; all compute happens in libddk.so."""
import collections
import ctypes as C
import math
import os
import warnings
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data')

DEFAULTS = dict(ns=24, nv=6, num_conv_layers=5, sigma_embed_dim=32, distance_embed_dim=32, cross_distance_embed_dim=32,
                lig_max_radius=5.0, rec_max_radius=30.0, cross_max_distance=80.0, center_max_distance=30.0,
                dynamic_max_cross=1, embedding_scale=1000.0, scale_by_sigma=1, no_torsion=0, batch_norm=1,
                latent_dim=0, latent_vocab=0, latent_droprate=0.0, lm_embedding_dim=1280,
                tr_sigma_min=0.1, tr_sigma_max=19.0, rot_sigma_min=0.03, rot_sigma_max=1.55,
                tor_sigma_min=0.03, tor_sigma_max=3.14, device=0, all_atoms=0, num_confidence_outputs=1, confidence_no_batchnorm=0,
                conv_kernel=0, deterministic=0, confidence_mode=0)

# the all-atom confidence model's edge groups in the order of its group tables (enum ConfGroup, csrc/conf.hip), and the words of
# ddk_confidence_status (include/ddk.h): CONF_STATUS_INTS int32, word CONF_OVERFLOW_WORD != 0 after a ligand-atom edge capacity overflow
CONF_GROUPS = ('ll', 'lr', 'la', 'aa', 'al', 'ar', 'rr', 'rl', 'ra')
CONF_STATUS_INTS, CONF_OVERFLOW_WORD = 20, 19


# what ``Complex.sample(..., record=...)`` returns: the device arrays of ddk_trajectory (include/ddk.h), None where a member was not recorded.
#   pos [steps + 1, B, n_lig, 3] (row k: before step k; row steps: final), scores / perturb [steps, B, 6 + n_rot], edge_counts [steps, 4] int32
TRAJECTORY_FIELDS = ('pos', 'scores', 'perturb', 'edge_counts')
Trajectory = collections.namedtuple('Trajectory', TRAJECTORY_FIELDS)

# what ``Context.cluster_poses`` returns, all device tensors (ddk_pose_pairwise_rmsd + ddk_pose_cluster, include/ddk.h): rmsd [B, B] float32; int32 cluster [B]
# (ordinal per pose, 0 = the cluster of the top-scored pose), leaders [B] (pose index per cluster, -1 after the first n_clusters entries), n_clusters [1]
PoseClusters = collections.namedtuple('PoseClusters', ('rmsd', 'cluster', 'leaders', 'n_clusters'))
# the limits of the two calls (csrc/model.h) and the tile shape of pose_pairs_kernel (tests place their shapes on its edges)
PAIRS_MAX_B, CLUSTER_MAX_B, PAIRS_TJ, PAIRS_ROWS_PER_PASS = 4096, 1024, 8, 16
# ddk_ligand_automorphisms (csrc/k_autos.hip): the largest table, the words of its status, and the sizes at which the search changes its path (csrc/model.h):
# cap * n_lig <= AUTOS_WALK_ONLY_ITEMS is one workgroup's walk alone; beyond it a level of more than AUTOS_WALK_ITEMS (row, candidate) items takes a pair
# of launches over workgroups of AUTOS_CHUNK items
AUTOS_MAX_CAP, AUTOS_WALK_ITEMS, AUTOS_WALK_ONLY_ITEMS, AUTOS_CHUNK = 1 << 20, 1024, 16384, 256
AUTOS_STATUS = ('complete', 'overflow: a level of the search held more partial maps than cap', 'a bond index outside the ligand')
# the three table builders of csrc/k_build.hip (ddk_receptor_knn_graph, ddk_radius_graph, ddk_ligand_transformation_mask): their limits (csrc/model.h)
BUILD_MAX_POINTS, KNN_MAX_NEIGHBOR, RADIUS_MAX_NEIGHBORS, LIG_MASK_MAX_EDGES = 65536, 128, 1024, 2048
MASK_STATUS = ('complete', 'more rotatable bonds than rows', 'a bond column that is out of range, unpaired, a self bond or repeated',
               'the ligand graph is not connected')


# the ddk_rng_* calls (csrc/k_rng.hip; DDK_RNG_LAYOUT of include/ddk.h): the purposes of the counter's top four bits and the limits (csrc/k_philox.h)
RNG_LAYOUT = 1
RNG_PURPOSES = dict(noise=0, initial_torsion=1, initial_rotation=2, initial_translation=3, ar_pick=4, ar_rotation=5)
RNG_MAX_STEPS, RNG_MAX_COLS = 1 << 20, 1024
# the purposes of the forward process (ddk_rng_perturbation, csrc/k_noising.hip), in the same counter field; their step field holds the draw index
RNG_FORWARD_PURPOSES = dict(forward_translation=6, forward_rotation=7, forward_torsion=8)
# the diffusion time of a complex for one noising (ddk_rng_forward_times): step = the draw index, block 0, word 0
RNG_TIME_PURPOSE = 11
# the latent of the DisCo score model: the keep flag of a complex (ddk_rng_latent_keep) and the Gumbel noise (DDK_GUMBEL_LAYOUT: step = the draw index, block = d)
RNG_LATENT_KEEP_PURPOSE, RNG_GUMBEL_PURPOSE = 12, 13
GUMBEL_LAYOUT, GUMBEL_TAG = 1, 0x47554D42
# the decoding index of an AR training item (ddk_rng_decoding_index): step = the draw index, block 0, word 0
RNG_DECODING_INDEX_PURPOSE = 14
# the ragged batch forms (ddk_rng_perturbation_batch, ddk_modify_conformer_batch, ddk_score_matching_loss_batch): limits (csrc/model.h) and status words
NOISE_BATCH_MAX_GRAPHS, NOISE_BATCH_MAX_LIG, NOISE_BATCH_MAX_ROT = 65536, 256, 1024
CONFORMER_BATCH_STATUS = ('done', None, 'a bond index outside the graph, or u == v', 'a coordinate that is not finite', 'a node_ptr / tor_ptr / mask_ptr entry out of range')
# conformer matching (ddk_conformer_match, csrc/k_match.hip): the purposes of its population and generation draws, its limits (csrc/model.h), the words of its status
RNG_MATCH_PURPOSES = dict(match_population=9, match_generation=10)
MATCH_MAX_ROT, MATCH_MAX_POPSIZE, MATCH_MAX_ITER, MATCH_MAX_POLISH, MATCH_MAX_ISLANDS, MATCH_MAX_MEMBERS, MATCH_MAX_VECTORS = 128, 64, 1000, 1024, 16, 8192, 65536
MATCH_STATUS = ('done', None, 'a rotor table that is out of range or breaks the mask rule, or fewer than 3 kept atoms', 'a coordinate that is not finite')
# the grids of utils/so3.py and utils/torus.py that ddk_so3_rows and ddk_torus_score evaluate (csrc/k_so3.hip, csrc/k_noising.hip)
SO3_N_EPS, SO3_X_N, SO3_MAX_ROWS, TORUS_SIGMA_N = 1000, 2000, 4096, 5000
# what ``Context.rng_perturbation`` returns: the device arrays of ddk_perturbation (include/ddk.h); tor_* are [B, n_rot]
Perturbation = collections.namedtuple('Perturbation', ('tr_update', 'rot_update', 'tor_update', 'tr_score', 'rot_score', 'tor_score'))
# the columns of ``Context.score_matching_loss`` (ddk_score_matching_loss)
LOSS_COLUMNS = ('tr_loss', 'rot_loss', 'tor_loss', 'tr_base_loss', 'rot_base_loss', 'tor_base_loss')


def stream_id(name):
    """The 64-bit id of a complex in the generator's counter (``stream_id`` of the ddk_rng_* calls): FNV-1a over the UTF-8 bytes of its name, so that every
    process, rank and run gives the same complex the same stream without agreeing on an enumeration.  stream_id('a') == 0xaf63dc4c8601ec8c."""
    h = 0xcbf29ce484222325
    for byte in str(name).encode('utf-8'):
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _u64(v, what):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError(f'ddk: {what} must be an unsigned 64-bit integer, got {v}')
    return v


def usable_automorphisms(perms, count, name=None):
    """(perms, count) of ``Context.ligand_automorphisms`` -> the rows a consumer may read, perms[:count[0]].  The consumers take the row count as a
    host integer, so this is ONE read-back of ``count`` (8 bytes; the same kind ``PoseClusters.n_clusters`` asks of its reader).  With status 1 or 2 that
    is the identity alone, the uncorrected fallback of evaluate.py:313, and a warning names the ligand and the status."""
    rows, status = (int(v) for v in count.tolist())
    if status != 0:
        warnings.warn(f'ddk: no automorphism table for ligand {name!r} (status {status}: {AUTOS_STATUS[status]}); its RMSDs are not symmetry-corrected')
    return perms[:rows]


def config_from_args(args, device=0):
    """model_parameters.yml Namespace -> ddk_config fields, the mapping of get_model
    (reference utils/model_utils.py:39-68) plus the constructor defaults it leaves alone."""
    g = lambda k, d: getattr(args, k, d)
    d = dict(DEFAULTS)
    d.update(ns=args.ns, nv=args.nv, num_conv_layers=args.num_conv_layers, sigma_embed_dim=args.sigma_embed_dim,
             distance_embed_dim=args.distance_embed_dim, cross_distance_embed_dim=args.cross_distance_embed_dim,
             lig_max_radius=float(args.max_radius), cross_max_distance=float(args.cross_max_distance),
             dynamic_max_cross=int(bool(args.dynamic_max_cross)), embedding_scale=float(args.embedding_scale),
             scale_by_sigma=int(bool(args.scale_by_sigma)), no_torsion=int(bool(args.no_torsion)),
             batch_norm=int(not args.no_batch_norm), latent_dim=int(g('latent_dim', 0)),
             latent_vocab=int(g('latent_vocab', 0)), latent_droprate=float(g('latent_droprate', 0.0)),
             lm_embedding_dim=1280 if g('esm_embeddings_path', None) is not None else 0,
             tr_sigma_min=args.tr_sigma_min, tr_sigma_max=args.tr_sigma_max, rot_sigma_min=args.rot_sigma_min,
             rot_sigma_max=args.rot_sigma_max, tor_sigma_min=args.tor_sigma_min, tor_sigma_max=args.tor_sigma_max,
             device=device)
    if g('sh_lmax', 2) != 1 or g('use_second_order_repr', False):
        raise RuntimeError('ddk implements the sh_lmax=1, first-order (FasterTensorProduct) score model only')
    return d


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_side_streams = {}


def h2d_async(t, device):
    """Host tensor -> device WITHOUT waiting for the work already queued on the current stream: the copy runs from pinned memory on
    a side stream and the current stream waits for it (a plain ``t.to(device)`` of pageable memory blocks the host until the copy
    has run, i.e. until the sampling loop of the previous complex has drained).  Device tensors pass through."""
    device = torch.device(device)
    if t.is_cuda:
        return t if t.device == device else t.to(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    side = _side_streams.get(idx)
    if side is None:
        side = _side_streams[idx] = torch.cuda.Stream(device=idx)
    pinned = t.contiguous().pin_memory()
    cur = torch.cuda.current_stream(idx)
    with torch.cuda.stream(side):
        d = pinned.to(device, non_blocking=True)
    cur.wait_stream(side)
    d.record_stream(cur)
    return d


def tp_layer_shape(layer, ns=24, nv=6):
    """The FasterTensorProduct of conv layer ``layer`` (get_irrep_seq and FasterTensorProduct.__init__, tensor_layers.py:12-27, 56-63; the table of
    csrc/k_tp_shape.h): input multiplicities A, P, Q, C of 0e, 1o, 1e, 0o, output multiplicities O, the weight blocks' rows R (0 where the block has no
    columns) and offsets B in the weight row of W floats, the widths din and dout of a node row.  Layers 3 and later share a shape."""
    seq = [(ns, 0, 0, 0), (ns, nv, 0, 0), (ns, nv, nv, 0), (ns, nv, nv, ns)]
    (A, P, Q, C), O = seq[min(layer, 3)], seq[min(layer + 1, 3)]
    R = [r if o else 0 for r, o in zip((A + P, A + P + Q, P + Q + C, Q + C), O)]
    B = [sum(r * o for r, o in zip(R[:k], O)) for k in range(5)]
    return dict(A=A, P=P, Q=Q, C=C, O=O, R=R, B=B, W=B[4], din=A + 3 * P + 3 * Q + C, dout=O[0] + 3 * O[1] + 3 * O[2] + O[3])


def tp_layer_shape_aa(layer, ns=24, nv=6):
    """Conv layer ``layer`` of the all-atom (confidence) model (all_atom_score_model.py:26, 112-133): e3nn's ``FullyConnectedTensorProduct(in, '1x0e + 1x1o +
    1x2e', out)`` on the irreps of ``tp_layer_shape``; the table of csrc/k_tp_shape.h and csrc/k_rtp.hip.  The keys of ``tp_layer_shape`` (R: a block's
    fan-in, B: None, the blocks are not adjacent in the weight row) and ``paths``: e3nn's instructions in its order, each a dict of ``ir_in``, ``ir_sh``,
    ``ir_out`` (names), ``offset`` and ``mul_in``, ``mul_out`` of its [mul_in, mul_out] matrix in the flat weight row, ``xoff`` / ``ooff`` (where the input and
    the output irrep start in a node row), ``block`` k and ``row0`` (its first row in weight block k, the order the kernels walk), ``kind`` (the product of one
    input with the sh row [Y0 | Y1 | Y2]: 'ss' i Y0, 'sv' i Y1, 'vs' i Y0, 'vd' i . Y1, 'vx' i x Y1, 'v2' M(Y2) i with M = [[-y2/sqrt3 - y4, y1, y0],
    [y1, 2 y2/sqrt3, y3], [y0, y3, -y2/sqrt3 + y4]]) and ``scale`` = sqrt(dim_out / R_k) times the amplitude of the Frobenius-normalised w3j in that form
    (1, 1/sqrt3, 1/sqrt3, 1/sqrt3, 1/sqrt6, 1/sqrt10).  Instructions without floats (an absent irrep) are left out."""
    s = tp_layer_shape(layer, ns, nv)
    A, P, Q, C, O = s['A'], s['P'], s['Q'], s['C'], s['O']
    R = [r if o else 0 for r, o in zip((A + P, A + P + Q + P, P + Q + C + Q, Q + C), O)]
    xoff = {'0e': 0, '1o': A, '1e': A + 3 * P, '0o': A + 3 * P + 3 * Q}
    ooff = {'0e': 0, '1o': O[0], '1e': O[0] + 3 * O[1], '0o': O[0] + 3 * O[1] + 3 * O[2]}
    mul_in, blk = {'0e': A, '1o': P, '1e': Q, '0o': C}, {'0e': 0, '1o': 1, '1e': 2, '0o': 3}
    amp = {'ss': 1.0, 'sv': 3 ** -0.5, 'vs': 3 ** -0.5, 'vd': 3 ** -0.5, 'vx': 6 ** -0.5, 'v2': 10 ** -0.5}
    # (input, sh, output, kind, first row in the output's block), in e3nn's order: input irrep, then sh irrep, then output irrep
    order = [('0e', '0e', '0e', 'ss', 0), ('0e', '1o', '1o', 'sv', 0), ('1o', '0e', '1o', 'vs', A), ('1o', '1o', '0e', 'vd', A), ('1o', '1o', '1e', 'vx', 0),
             ('1o', '2e', '1o', 'v2', A + P + Q), ('1e', '0e', '1e', 'vs', P), ('1e', '1o', '1o', 'vx', A + P), ('1e', '1o', '0o', 'vd', 0),
             ('1e', '2e', '1e', 'v2', P + Q + C), ('0o', '0e', '0o', 'ss', Q), ('0o', '1o', '1e', 'sv', P + Q)]
    paths, off = [], 0
    for ir_in, ir_sh, ir_out, kind, row0 in order:
        k = blk[ir_out]
        mi, mo = mul_in[ir_in], O[k]
        if mi * mo == 0:
            continue
        dim_out = 3 if k in (1, 2) else 1
        paths.append(dict(ir_in=ir_in, ir_sh=ir_sh, ir_out=ir_out, kind=kind, offset=off, mul_in=mi, mul_out=mo, xoff=xoff[ir_in], ooff=ooff[ir_out],
                          block=k, row0=row0, scale=math.sqrt(dim_out / R[k]) * amp[kind]))
        off += mi * mo
    return dict(s, R=R, B=None, W=off, paths=paths, sh_dim=9)


TP_NV4 = 8      # DDK_TP_NV4 of include/ddk.h: the `layer` argument TP_NV4 + l of the tensor-product ops is layer l of the ns = 24 / nv = 4 family


TP_AA = 16      # DDK_TP_AA: TP_AA + l is conv layer l of the all-atom (confidence) family, sh_lmax = 2 (the radial tensor product and the radial conv only)


def tp_id_shape(layer, ns=24, nv=6):
    """``tp_layer_shape`` of a `layer` argument of the tensor-product ops: TP_NV4 + l (l in 0..4) is layer l of the ns = 24 / nv = 4 family whatever the
    context's nv, TP_AA + l is ``tp_layer_shape_aa(l)``; anything else is conv layer ``layer`` of a model with (``ns``, ``nv``)"""
    if TP_NV4 <= layer < TP_NV4 + 5:
        return tp_layer_shape(layer - TP_NV4, 24, 4)
    if TP_AA <= layer < TP_AA + 5:
        return tp_layer_shape_aa(layer - TP_AA)
    return tp_layer_shape(layer, ns, nv)


def tp_sh_dim(layer):
    """floats of an sh row of the tensor-product ops for this `layer` argument: 9 = [Y0 | Y1 | Y2] for the all-atom family, else 4"""
    return 9 if TP_AA <= layer < TP_AA + 5 else 4


HEAD_CENTER, HEAD_TORSION = 0, 1      # DDK_HEAD_CENTER, DDK_HEAD_TORSION of include/ddk.h


def head_tp_shape(head, ns=24, nv=6):
    """e3nn's FullyConnectedTensorProduct of a score head (tensor_layers.py:137; the table of csrc/k_hconv.hip): ``final_conv`` (``HEAD_CENTER``:
    in (x) '1x0e + 1x1o' -> '2x1o + 2x1e') or ``tor_bond_conv`` (``HEAD_TORSION``: in (x) '1x1o + 1x2e + 1x2o + 1x3o' -> 'ns x 0o + ns x 0e'), ``in`` the
    output irreps of conv layer 3.  W: floats of a weight row, K: the radial MLP's width, din / dout: the widths of a node row and an output row, ``blocks``:
    the weight blocks in e3nn's instruction order as (name, i_in1, i_in2, i_out, offset, (mul_in1, mul_in2, mul_out)), the indices into the three irreps
    lists, ``out_off``: where output irrep i_out starts in the output row."""
    if head == HEAD_CENTER:
        paths = [('A', 0, 1, 0, ns), ('B', 1, 0, 0, nv), ('C', 1, 1, 1, nv), ('D', 2, 0, 1, nv), ('E', 2, 1, 0, nv), ('F', 3, 1, 1, ns)]
        mulo, K, dout, out_off = 2, 2 * ns, 12, (0, 6)
    elif head == HEAD_TORSION:
        paths = [('P', 1, 0, 1, nv), ('Q', 2, 0, 0, nv)]
        mulo, K, dout, out_off = ns, 3 * ns, 2 * ns, (0, ns)
    else:
        raise RuntimeError(f'ddk: head must be HEAD_CENTER (0) or HEAD_TORSION (1); got {head!r}')
    blocks, off = [], 0
    for name, i1, i2, io, mul1 in paths:
        blocks.append((name, i1, i2, io, off, (mul1, 1, mulo)))
        off += mul1 * mulo
    return dict(W=off, K=K, din=2 * ns + 6 * nv, dout=dout, blocks=blocks, out_off=out_off)


class ConvGraph:
    """The graph of the radial conv, made and checked by ``Context.conv_graph``: ``src`` / ``dst`` int32 [E]; ``src_order`` / ``dst_order`` int32 [E], the
    edge ids sorted by node, ascending within a node; ``src_ptr`` [n_out + 1] / ``dst_ptr`` [n_in + 1] int64, node n owns order[ptr[n] : ptr[n + 1]];
    ``src_count`` [n_out] / ``dst_count`` [n_in] int64, the edges per node.  The kernels trust these tables."""
    __slots__ = ('src', 'dst', 'src_order', 'dst_order', 'src_ptr', 'dst_ptr', 'src_count', 'dst_count', 'n_in', 'n_out', 'E')

    def __init__(self, src, dst, src_order, dst_order, src_ptr, dst_ptr, src_count, dst_count, n_in, n_out):
        self.src, self.dst, self.src_order, self.dst_order = src, dst, src_order, dst_order
        self.src_ptr, self.dst_ptr, self.src_count, self.dst_count = src_ptr, dst_ptr, src_count, dst_count
        self.n_in, self.n_out, self.E = n_in, n_out, src.shape[0]


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError('ddk: device tensors only (no CPU path exists); got a tensor on ' + str(t.device))
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _ragged_tables(who, table_l, table_r, *ptrs):
    """(G, D) of an op over a graph's ligand nodes followed by its receptor nodes, after the checks the host can make: two tables [N_lig, D], [N_rec, D] with D in
    1..4 on one device; ``ptrs`` = (lig_ptr, rec_ptr), contiguous int64 [G + 1] there, 1..65536 graphs.  An op on one graph passes none (G is None)."""
    dev = table_l.device
    if table_l.dim() != 2 or table_r.dim() != 2 or table_l.shape[1] != table_r.shape[1] or not 1 <= table_l.shape[1] <= 4 or table_r.device != dev:
        raise RuntimeError(f'ddk: {who} takes two tables [N_lig, D] and [N_rec, D] with D in 1..4 on one device; got {tuple(table_l.shape)} and {tuple(table_r.shape)}')
    if not ptrs:
        return None, table_l.shape[1]
    for name, t in zip(('lig_ptr', 'rec_ptr'), ptrs):
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.device != dev or t.shape != ptrs[0].shape:
            raise RuntimeError(f'ddk: {who} takes {name} as a contiguous int64 vector [G + 1] on the device of the tables')
    G = ptrs[0].shape[0] - 1
    if not 1 <= G <= 65536:
        raise RuntimeError(f'ddk: {who} takes 1..65536 graphs; got {G}')
    return G, table_l.shape[1]


def _temperature(who, temperature):
    if not 0 < float(temperature) < float('inf'):
        raise RuntimeError(f'ddk: {who} takes a positive finite temperature; got {temperature}')
    return float(temperature)


def _need_int31(who, **values):
    for k, v in values.items():
        if not 0 <= int(v) < 1 << 31:
            raise RuntimeError(f'ddk: {who}: {k} = {v} must be a non-negative int32')


def _need(need, who, four=False):
    """``need`` of a ``*_backward`` as a tuple of bools; a call that asks for no gradient (``four``: or not for four flags) is refused"""
    need = tuple(bool(n) for n in need)
    if four and (len(need) != 4 or not any(need)):
        raise RuntimeError(f'ddk: {who} needs at least one of its four gradients to compute')
    if not any(need):
        raise RuntimeError(f'ddk: {who} needs at least one gradient to compute')
    return need


def _outputs(need, shapes, device):
    """(outs, live) of a ``*_backward``: a new fp32 tensor of its shape where ``need`` is set and None elsewhere; ``live``: one of them has an element
    (empty tensors have no address: without one the entry would see no output at all, and the caller returns ``outs`` as they are)"""
    outs = [torch.empty(shape, dtype=torch.float32, device=device) if n else None for n, shape in zip(need, shapes)]
    return outs, any(o is not None and o.numel() for o in outs)


def _workspace(nbytes, what, device):
    """``nbytes`` of a workspace query as a tensor from torch's allocator, which orders its reuse after the launches on the current stream when the
    caller lets go of it; a negative answer is refused as 'ddk: ``what``'"""
    if nbytes < 0:
        raise RuntimeError('ddk: ' + what)
    return torch.empty(max(int(nbytes), 16) // 4, dtype=torch.float32, device=device)


class Context:
    """One ddk_ctx (one device).  device=-1 gives a host-only context (weight packing only, for CPU tests)."""

    def __init__(self, device=0, **cfg):
        self.L = _lib.lib()
        d = dict(DEFAULTS)
        if os.environ.get('DDK_CONV_KERNEL'):     # 1: the fp32-MFMA conv kernel (the fallback), 3: the three-limb / six-product form, for every context of this process
            d['conv_kernel'] = int(os.environ['DDK_CONV_KERNEL'])
        if os.environ.get('DDK_DETERMINISTIC'):   # select the deterministic scatter for every context of this process
            d['deterministic'] = int(os.environ['DDK_DETERMINISTIC'])
        d.update(cfg)
        if d.get('all_atoms'):
            d['deterministic'] = int(cfg.get('deterministic', 0))      # the env switch applies to score-model contexts only
        d['device'] = device
        self.cfg = SimpleNamespace(**d)
        c = _lib.ddk_config(**d)
        self.h = C.c_void_p()
        rc = self.L.ddk_create(C.byref(c), C.byref(self.h))
        if rc != 0:
            msg = self.L.ddk_last_error(self.h).decode() if self.h else 'ddk_create failed'
            raise RuntimeError(f'ddk_create: {msg}')
        self.device = device
        self._tables_set = False
        self._match_ws = {}      # match_conformer's workspace per stream

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f'{what}: {self.L.ddk_last_error(self.h).decode()} (rc={rc})')

    def close(self):
        if getattr(self, 'h', None):
            self.L.ddk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- checkpoint --------------------------------------------------------------------------
    def load_state_dict(self, state_dict, prefix='', finalize=True):
        """state_dict with the reference's key names (score_model.state_dict(), evaluate.py:169-171)."""
        for k, v in state_dict.items():
            if not torch.is_tensor(v) or not v.is_floating_point():
                continue
            a = np.ascontiguousarray(v.detach().cpu().float().numpy())
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(self.L.ddk_load_weights(self.h, (prefix + k).encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                        f'ddk_load_weights({k})')
        if finalize:
            self.finalize()

    def finalize(self):
        if not self._tables_set:
            self.set_tables(np.load(os.path.join(_DATA, 'so3_exp_score_norms.npy')),
                            np.load(os.path.join(_DATA, 'torus_score_norm_seed0.npy')))
        self._check(self.L.ddk_finalize_weights(self.h), 'ddk_finalize_weights')

    def set_tables(self, so3, torus):
        so3 = np.ascontiguousarray(so3, dtype=np.float64)
        torus = np.ascontiguousarray(torus, dtype=np.float64)
        self._check(self.L.ddk_set_score_norm_tables(self.h, so3.ctypes.data_as(C.c_void_p), len(so3),
                                                     torus.ctypes.data_as(C.c_void_p), len(torus)), 'ddk_set_score_norm_tables')
        self._tables_set = True
        self.score_norm_tables = (so3, torus)      # host copies: training.loss_function looks its two norms up here

    def export(self, what, dtype=np.float32):
        n = self.L.ddk_debug_export(self.h, what.encode(), None, 0)
        if n < 0:
            raise RuntimeError(f'ddk_debug_export({what}): {self.L.ddk_last_error(self.h).decode()}')
        buf = np.zeros(n, dtype=dtype)
        self.L.ddk_debug_export(self.h, what.encode(), buf.ctypes.data_as(C.c_void_p), n)
        return buf

    # ---- measurement -------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.L.ddk_profile_enable(self.h, int(on)), 'ddk_profile_enable')

    def profile_read(self):
        """per conv layer: kernel ms, launches, edges evaluated, edges without the receptive-field pruning, reference edges"""
        n = 5 * self.cfg.num_conv_layers
        buf = (C.c_double * n)()
        self._check(self.L.ddk_profile_read(self.h, buf, n), 'ddk_profile_read')
        a = np.array(list(buf)).reshape(-1, 5)
        return [dict(ms=float(r[0]), launches=int(r[1]), edges=int(r[2]), edges_unpruned=int(r[3]), edges_reference=int(r[4])) for r in a]

    def profile_read_forwards(self, max_forwards=32768):
        """per forward since profile_enable(True), in launch order: array [n, 4] = conv kernel ms, edges evaluated, edges without the
        receptive-field pruning, cross edges of the forward's graph"""
        buf = (C.c_double * (4 * max_forwards))()
        n = self.L.ddk_profile_read_forwards(self.h, buf, max_forwards)
        if n < 0:
            raise RuntimeError(f'ddk_profile_read_forwards: {self.L.ddk_last_error(self.h).decode()}')
        if n >= max_forwards:
            raise RuntimeError(f'ddk_profile_read_forwards: {n} forwards recorded, the profile buffer holds {max_forwards}: later launches were not timed')
        return np.array(buf[:4 * min(n, max_forwards)]).reshape(-1, 4)

    def set_pruning(self, on=True):
        """backward receptive-field pruning of the receptor-receptor messages (default on; exact)"""
        self._check(self.L.ddk_set_receptive_field_pruning(self.h, int(bool(on))), 'ddk_set_receptive_field_pruning')

    def pool_stats(self):
        """device-chunk pool of the complexes (include/ddk_debug.h): hipMalloc calls, reuses, hipFree calls, bytes / chunks parked, bytes owned now / at peak"""
        buf = (C.c_int64 * 8)()
        self._check(self.L.ddk_debug_pool_stats(self.h, buf), 'ddk_debug_pool_stats')
        keys = ('hipMalloc_calls', 'reuses', 'hipFree_calls', 'bytes_parked', 'chunks_parked', 'bytes_owned', 'bytes_owned_peak', 'device_bytes_held')
        return dict(zip(keys, [int(v) for v in buf[:8]]))

    def debug_set_alloc_limit(self, nbytes=0):
        """test hook (include/ddk_debug.h): cap on the device memory this context may hold (0 = none); a request beyond it fails like a real out-of-memory"""
        self._check(self.L.ddk_debug_set_alloc_limit(self.h, int(nbytes)), 'ddk_debug_set_alloc_limit')

    def debug_set_layer0_dedup(self, on=True):
        """test hook (include/ddk_debug.h): layer-0 de-duplication of the rec-rec messages on / off"""
        self._check(self.L.ddk_debug_set_layer0_dedup(self.h, int(bool(on))), 'ddk_debug_set_layer0_dedup')

    # ---- operators ---------------------------------------------------------------------------
    def tp_forward(self, layer, x_dst, sh, w, dout):
        x_dst, sh, w = x_dst.contiguous().float(), sh.contiguous().float(), w.contiguous().float()
        E = x_dst.shape[0]
        out = torch.empty((E, dout), dtype=torch.float32, device=x_dst.device)
        self._check(self.L.ddk_tp_forward(self.h, layer, _ptr(x_dst), _ptr(sh), _ptr(w), E, _ptr(out), _stream()), 'ddk_tp_forward')
        return out

    def tp_backward(self, layer, x_dst, sh, w, grad_out, need=(True, True, True)):
        """The vector-Jacobian product of ``tp_forward`` (ddk_tp_backward): (grad_x | None, grad_sh | None, grad_w | None) for the three flags of
        ``need``.  ``w`` may be None when grad_w alone is asked for (it does not depend on w, and w is not read then)."""
        need_x, need_sh, need_w = (bool(n) for n in need)
        if not (need_x or need_sh or need_w):
            raise RuntimeError('ddk: tp_backward needs at least one gradient to compute')
        if w is None and (need_x or need_sh):
            raise RuntimeError('ddk: tp_backward needs w for grad_x and grad_sh')
        x_dst, sh, grad_out = (_need_cuda(t).contiguous().float() for t in (x_dst, sh, grad_out))
        E = x_dst.shape[0]
        if need_x or need_sh:
            w = _need_cuda(w).contiguous().float()
            if w.dim() != 2 or w.shape[0] != E:
                raise RuntimeError('ddk: tp_backward takes w [E, W]; got ' + str(tuple(w.shape)))
            W = w.shape[1]
        else:
            w, W = None, self.tp_weight_numel(layer)
        if sh.shape != (E, 4) or grad_out.dim() != 2 or grad_out.shape[0] != E:
            raise RuntimeError('ddk: tp_backward takes sh [E, 4] and grad_out [E, Dout]')
        new = lambda cols: torch.empty((E, cols), dtype=torch.float32, device=x_dst.device)
        gx, gsh, gw = new(x_dst.shape[1]) if need_x else None, new(4) if need_sh else None, new(W) if need_w else None
        if E == 0:      # (an empty tensor has no address: the entry would see no output at all)
            return gx, gsh, gw
        self._check(self.L.ddk_tp_backward(self.h, layer, _ptr(x_dst), _ptr(sh), _ptr(w), _ptr(grad_out), E, _ptr(gx), _ptr(gsh), _ptr(gw), _stream()),
                    'ddk_tp_backward')
        return gx, gsh, gw

    def _rtp_operands(self, layer, x_dst, sh, h, group_offsets, w2, b2, E=None):
        """checked operands of the radial tensor product: (x, sh, h, offsets as a ctypes int64 array, G, w2, b2, E, W).  E: the rows of x_dst, unless
        given (the radial conv, whose x is a node table)"""
        x_dst, sh, h = (_need_cuda(t).contiguous().float() for t in (x_dst, sh, h))
        offs = [int(o) for o in group_offsets]
        G, E, W = len(offs) - 1, x_dst.shape[0] if E is None else E, self.tp_weight_numel(layer)
        if not 1 <= G <= 4:
            raise RuntimeError(f'ddk: the radial tensor product takes 1..4 edge groups; got {G}')
        if sh.shape != (E, tp_sh_dim(layer)) or h.shape != (E, 72):
            raise RuntimeError(f'ddk: the radial tensor product takes sh [E, {tp_sh_dim(layer)}] and h [E, 72]' + (' (the all-atom family: [Y0 | Y1 | Y2])' if tp_sh_dim(layer) == 9 else ''))
        if w2 is not None:
            w2 = _need_cuda(w2).contiguous().float()
            if w2.shape != (G, W, 72):
                raise RuntimeError(f'ddk: the radial tensor product takes w2 [G, W, 72] = {(G, W, 72)}; got {tuple(w2.shape)}')
        if b2 is not None:
            b2 = _need_cuda(b2).contiguous().float()
            if b2.shape != (G, W):
                raise RuntimeError(f'ddk: the radial tensor product takes b2 [G, W] = {(G, W)}; got {tuple(b2.shape)}')
        return x_dst, sh, h, (C.c_int64 * (G + 1))(*offs), G, w2, b2, E, W

    def rtp_forward(self, layer, x_dst, sh, h, group_offsets, w2, b2, dout):
        """The radial tensor product (ddk_rtp_forward): out [E, dout] = FasterTensorProduct(x_dst, sh, w2[g] h + b2[g]) with the per-edge weights never
        stored.  ``group_offsets``: G + 1 host integers, edge e belongs to group g iff offsets[g] <= e < offsets[g + 1]."""
        x_dst, sh, h, offs, G, w2, b2, E, W = self._rtp_operands(layer, x_dst, sh, h, group_offsets, w2, b2)
        if w2 is None or b2 is None:
            raise RuntimeError('ddk: rtp_forward needs w2 and b2')
        out = torch.empty((E, dout), dtype=torch.float32, device=x_dst.device)
        self._check(self.L.ddk_rtp_forward(self.h, layer, _ptr(x_dst), _ptr(sh), _ptr(h), offs, G, _ptr(w2), _ptr(b2), E, _ptr(out), _stream()), 'ddk_rtp_forward')
        return out

    def rtp_backward(self, layer, x_dst, sh, h, group_offsets, w2, b2, grad_out, need=(True, True, True, True, True)):
        """The vector-Jacobian product of ``rtp_forward`` (ddk_rtp_backward): (grad_x, grad_sh, grad_h, grad_w2, grad_b2), None where ``need`` is false.
        ``w2`` and ``b2`` may be None when only grad_w2 / grad_b2 are asked for; ``b2`` is read for grad_x / grad_sh alone.  The workspace of the
        parameter gradients comes from torch's allocator and is released on return."""
        need = _need(need, 'rtp_backward')
        if w2 is None and any(need[:3]):
            raise RuntimeError('ddk: rtp_backward needs w2 for grad_x, grad_sh and grad_h')
        if b2 is None and any(need[:2]):
            raise RuntimeError('ddk: rtp_backward needs b2 for grad_x and grad_sh')
        x_dst, sh, h, offs, G, w2, b2, E, W = self._rtp_operands(layer, x_dst, sh, h, group_offsets, w2, b2)
        grad_out = _need_cuda(grad_out).contiguous().float()
        if grad_out.dim() != 2 or grad_out.shape[0] != E:
            raise RuntimeError('ddk: rtp_backward takes grad_out [E, Dout]')
        outs, live = _outputs(need, ((E, x_dst.shape[1]), (E, tp_sh_dim(layer)), (E, 72), (G, W, 72), (G, W)), x_dst.device)
        if not live:
            return tuple(outs)
        ws = None
        if need[3] or need[4]:
            ws = _workspace(self.L.ddk_rtp_backward_workspace(layer, E, G), f'rtp_backward: no workspace for layer {layer}, E = {E}, {G} groups', x_dst.device)
        self._check(self.L.ddk_rtp_backward(self.h, layer, _ptr(x_dst), _ptr(sh), _ptr(h), offs, G, _ptr(w2), _ptr(b2), _ptr(grad_out), E,
                                            *[_ptr(o) for o in outs], _ptr(ws), _stream()), 'ddk_rtp_backward')
        return tuple(outs)      # (ws goes back to torch's allocator, which orders its reuse after this launch on the current stream)

    # ---- the radial conv: node features to aggregated node features ---------------------------------
    @staticmethod
    def conv_graph(edge_src, edge_dst, n_in, n_out):
        """The checked graph of ``rconv_forward`` / ``rconv_backward`` (a ``ConvGraph``), built once per graph with torch ops on the device of the
        indices (CPU tensors work too): messages go from node ``edge_dst[e]`` of the ``n_in`` input nodes to node ``edge_src[e]`` of the ``n_out``
        output nodes (edge_index rows 0 / 1 of the reference).  One read-back, of the extremes of the indices; an index outside its range or
        E >= 2^31 raises."""
        src, dst = torch.as_tensor(edge_src).reshape(-1), torch.as_tensor(edge_dst).reshape(-1)
        n_in, n_out, E = int(n_in), int(n_out), src.shape[0]
        if dst.shape[0] != E or dst.device != src.device or src.is_floating_point() or dst.is_floating_point():
            raise RuntimeError('ddk: conv_graph takes two integer index vectors of one length on one device')
        if E >= 1 << 31 or not (0 <= n_in < 1 << 31 and 0 <= n_out < 1 << 31):
            raise RuntimeError(f'ddk: conv_graph: E = {E}, n_in = {n_in}, n_out = {n_out}: each must be below 2^31')
        src, dst = src.long(), dst.long()
        if E > 0:
            lo_s, hi_s, lo_d, hi_d = torch.stack([src.min(), src.max(), dst.min(), dst.max()]).tolist()
            if lo_s < 0 or hi_s >= n_out or lo_d < 0 or hi_d >= n_in:
                raise RuntimeError(f'ddk: conv_graph: edge_src must be in [0, {n_out}) and edge_dst in [0, {n_in}); got [{lo_s}, {hi_s}] and [{lo_d}, {hi_d}]')

        def table(idx, n):      # the edge ids sorted by node (stable: ascending edge id within a node), the node's range in them, its edge count
            order = torch.sort(idx, stable=True).indices.to(torch.int32)
            count = torch.bincount(idx, minlength=n)[:n]
            ptr = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
            ptr[1:] = torch.cumsum(count, 0)
            return order.contiguous(), ptr, count

        src_order, src_ptr, src_count = table(src, n_out)
        dst_order, dst_ptr, dst_count = table(dst, n_in)
        return ConvGraph(src.to(torch.int32).contiguous(), dst.to(torch.int32).contiguous(), src_order, dst_order, src_ptr, dst_ptr, src_count, dst_count,
                         n_in, n_out)

    def _rconv_operands(self, layer, graph, x_nodes, sh, h, group_offsets, w2, b2):
        """checked operands of the radial conv: those of ``_rtp_operands`` with x a node table [n_in, Din] and E the graph's"""
        if not isinstance(graph, ConvGraph):
            raise RuntimeError('ddk: the radial conv takes a ConvGraph (Context.conv_graph): its kernels trust the indices')
        ops = self._rtp_operands(layer, x_nodes, sh, h, group_offsets, w2, b2, E=graph.E)
        x_nodes = ops[0]
        if x_nodes.dim() != 2 or x_nodes.shape != (graph.n_in, tp_id_shape(layer, self.cfg.ns, self.cfg.nv)['din']):
            raise RuntimeError(f'ddk: the radial conv takes x_nodes [n_in, Din] for a graph of {graph.n_in} input nodes; got {tuple(x_nodes.shape)}')
        if graph.src.device != x_nodes.device:
            raise RuntimeError('ddk: the radial conv takes a ConvGraph on the device of its operands')
        if ops[3][ops[4]] != graph.E:
            raise RuntimeError(f'ddk: the edge groups hold {ops[3][ops[4]]} edges, the graph {graph.E}')
        return ops

    def rconv_forward(self, layer, graph, x_nodes, sh, h, group_offsets, w2, b2):
        """The radial conv (ddk_rconv_forward): out_nodes [n_out, Dout] = scatter-mean over ``graph.src`` of FasterTensorProduct(x_nodes[graph.dst], sh,
        w2[g] h + b2[g]); neither the per-edge weights nor the gathered rows are stored, the mean is a fixed-order sum (no atomics).  The workspace
        (the tensor product's rows) comes from torch's allocator and is released on return."""
        x_nodes, sh, h, offs, G, w2, b2, E, W = self._rconv_operands(layer, graph, x_nodes, sh, h, group_offsets, w2, b2)
        if w2 is None or b2 is None:
            raise RuntimeError('ddk: rconv_forward needs w2 and b2')
        dout = tp_id_shape(layer, self.cfg.ns, self.cfg.nv)['dout']
        out = torch.empty((graph.n_out, dout), dtype=torch.float32, device=x_nodes.device)
        g = graph
        ws = _workspace(self.L.ddk_rconv_workspace(layer, g.E, G, g.n_in, g.n_out, 0),
                        f'no radial-conv workspace for layer {layer}, E = {g.E}, {G} groups, {g.n_in} -> {g.n_out} nodes', x_nodes.device)
        self._check(self.L.ddk_rconv_forward(self.h, layer, _ptr(x_nodes), g.n_in, g.n_out, _ptr(g.src), _ptr(g.dst), _ptr(g.src_order), _ptr(g.src_ptr),
                                             _ptr(sh), _ptr(h), offs, G, _ptr(w2), _ptr(b2), E, _ptr(out), _ptr(ws), _stream()), 'ddk_rconv_forward')
        return out

    def rconv_backward(self, layer, graph, x_nodes, sh, h, group_offsets, w2, b2, grad_out_nodes, need=(True, True, True, True, True)):
        """The vector-Jacobian product of ``rconv_forward`` (ddk_rconv_backward): (grad_x_nodes [n_in, Din], grad_sh, grad_h, grad_w2, grad_b2), None
        where ``need`` is false; ``w2`` / ``b2`` may be None as in ``rtp_backward``.  The same bits from call to call.  The workspace comes from torch's
        allocator and is released on return."""
        need = _need(need, 'rconv_backward')
        if w2 is None and any(need[:3]):
            raise RuntimeError('ddk: rconv_backward needs w2 for grad_x_nodes, grad_sh and grad_h')
        if b2 is None and any(need[:2]):
            raise RuntimeError('ddk: rconv_backward needs b2 for grad_x_nodes and grad_sh')
        x_nodes, sh, h, offs, G, w2, b2, E, W = self._rconv_operands(layer, graph, x_nodes, sh, h, group_offsets, w2, b2)
        g = graph
        grad_out_nodes = _need_cuda(grad_out_nodes).contiguous().float()
        if grad_out_nodes.dim() != 2 or grad_out_nodes.shape[0] != g.n_out:
            raise RuntimeError('ddk: rconv_backward takes grad_out_nodes [n_out, Dout]')
        outs, live = _outputs(need, ((g.n_in, x_nodes.shape[1]), (E, tp_sh_dim(layer)), (E, 72), (G, W, 72), (G, W)), x_nodes.device)
        if not live:
            return tuple(outs)
        ws = _workspace(self.L.ddk_rconv_workspace(layer, E, G, g.n_in, g.n_out, 1),
                        f'no radial-conv workspace for layer {layer}, E = {E}, {G} groups, {g.n_in} -> {g.n_out} nodes', x_nodes.device)
        self._check(self.L.ddk_rconv_backward(self.h, layer, _ptr(x_nodes), g.n_in, g.n_out, _ptr(g.src), _ptr(g.dst), _ptr(g.src_order), _ptr(g.src_ptr),
                                              _ptr(g.dst_order), _ptr(g.dst_ptr), _ptr(sh), _ptr(h), offs, G, _ptr(w2), _ptr(b2), _ptr(grad_out_nodes), E,
                                              *[_ptr(o) for o in outs], _ptr(ws), _stream()), 'ddk_rconv_backward')
        return tuple(outs)      # (ws goes back to torch's allocator, which orders its reuse after these launches on the current stream)

    # ---- the head convolutions: node features to receiver rows ------------------------------------------
    def _hconv_operands(self, head, graph, x, sh, h, w2, b2):
        """checked operands of a head conv: (shape, x, sh, h, w2, b2)"""
        s = head_tp_shape(head)
        if not isinstance(graph, ConvGraph):
            raise RuntimeError('ddk: the head conv takes a ConvGraph (Context.conv_graph): its kernels trust the indices')
        x, sh, h = (_need_cuda(t).contiguous().float() for t in (x, sh, h))
        if x.shape != (graph.n_in, s['din']):
            raise RuntimeError(f'ddk: the head conv takes x [n_in, {s["din"]}] for a graph of {graph.n_in} input nodes; got {tuple(x.shape)}')
        if sh.shape != (graph.E, 4) or h.shape != (graph.E, s['K']):
            raise RuntimeError(f'ddk: the head conv takes sh [E, 4] and h [E, {s["K"]}] for a graph of {graph.E} edges; got {tuple(sh.shape)} and {tuple(h.shape)}')
        if graph.src.device != x.device or sh.device != x.device or h.device != x.device:
            raise RuntimeError('ddk: the head conv takes a ConvGraph, sh and h on the device of x')
        if w2 is not None:
            w2 = _need_cuda(w2).contiguous().float()
            if w2.shape != (s['W'], s['K']) or w2.device != x.device:
                raise RuntimeError(f'ddk: the head conv takes w2 [W, K] = {(s["W"], s["K"])} on the device of x; got {tuple(w2.shape)}')
        if b2 is not None:
            b2 = _need_cuda(b2).contiguous().float()
            if b2.shape != (s['W'],) or b2.device != x.device:
                raise RuntimeError(f'ddk: the head conv takes b2 [W] = {(s["W"],)} on the device of x; got {tuple(b2.shape)}')
        return s, x, sh, h, w2, b2

    def hconv_forward(self, head, graph, x, sh, h, w2, b2):
        """A head conv (ddk_hconv_forward): out [n_out, dout] = the mean over ``graph.src`` of e3nn's FullyConnectedTensorProduct of ``head_tp_shape(head)``
        on (x[graph.dst], sh, w2 h + b2); the per-edge weights and the gathered rows are never stored, the mean is a fixed-order sum (no atomics).  For
        ``HEAD_TORSION`` ``sh[:, 1:4]`` is the 1o block of the full tensor product of the edge's and the bond's spherical harmonics."""
        s, x, sh, h, w2, b2 = self._hconv_operands(head, graph, x, sh, h, w2, b2)
        if w2 is None or b2 is None:
            raise RuntimeError('ddk: hconv_forward needs w2 and b2')
        g = graph
        out = torch.empty((g.n_out, s['dout']), dtype=torch.float32, device=x.device)
        if out.numel() == 0:
            return out
        ws = _workspace(self.L.ddk_hconv_workspace(head, g.E, g.n_in, g.n_out, 0),
                        f'no head-conv workspace for head {head}, E = {g.E}, {g.n_in} -> {g.n_out} nodes', x.device)
        self._check(self.L.ddk_hconv_forward(self.h, head, _ptr(x), g.n_in, g.n_out, _ptr(g.src), _ptr(g.dst), _ptr(g.src_order), _ptr(g.src_ptr), _ptr(sh),
                                             _ptr(h), _ptr(w2), _ptr(b2), g.E, _ptr(out), _ptr(ws), _stream()), 'ddk_hconv_forward')
        return out

    def hconv_backward(self, head, graph, x, sh, h, w2, b2, grad_out, need=(True, True, True, True)):
        """The vector-Jacobian product of ``hconv_forward`` (ddk_hconv_backward): (grad_x [n_in, din], grad_h [E, K], grad_w2 [W, K], grad_b2 [W]), None
        where ``need`` is false.  ``w2`` may be None when neither grad_x nor grad_h is asked for, ``b2`` unless grad_x is.  There is no grad_sh.  The same
        bits from call to call.  The workspace comes from torch's allocator and is released on return."""
        need = _need(need, 'hconv_backward', four=True)
        if w2 is None and any(need[:2]):
            raise RuntimeError('ddk: hconv_backward needs w2 for grad_x and grad_h')
        if b2 is None and need[0]:
            raise RuntimeError('ddk: hconv_backward needs b2 for grad_x')
        s, x, sh, h, w2, b2 = self._hconv_operands(head, graph, x, sh, h, w2, b2)
        g = graph
        grad_out = _need_cuda(grad_out).contiguous().float()
        if grad_out.shape != (g.n_out, s['dout']) or grad_out.device != x.device:
            raise RuntimeError(f'ddk: hconv_backward takes grad_out [n_out, {s["dout"]}] on the device of x')
        outs, live = _outputs(need, ((g.n_in, s['din']), (g.E, s['K']), (s['W'], s['K']), (s['W'],)), x.device)
        if not live:
            return tuple(outs)
        ws = _workspace(self.L.ddk_hconv_workspace(head, g.E, g.n_in, g.n_out, 1),
                        f'no head-conv workspace for head {head}, E = {g.E}, {g.n_in} -> {g.n_out} nodes', x.device)
        self._check(self.L.ddk_hconv_backward(self.h, head, _ptr(x), g.n_in, g.n_out, _ptr(g.src), _ptr(g.dst), _ptr(g.src_order), _ptr(g.src_ptr),
                                              _ptr(g.dst_order), _ptr(g.dst_ptr), _ptr(sh), _ptr(h), _ptr(w2), _ptr(b2), _ptr(grad_out), g.E,
                                              *[_ptr(o) for o in outs], _ptr(ws), _stream()), 'ddk_hconv_backward')
        return tuple(outs)      # (ws goes back to torch's allocator, which orders its reuse after these launches on the current stream)

    def seg_sum(self, rows, order, ptr):
        """The fixed-order segmented sum (ddk_seg_sum): nodes [N, D] with nodes[n] = the rows ``order[ptr[n] : ptr[n + 1]]`` of ``rows`` [E, D] added in
        that order; a node without rows gets zeros.  ``order`` int32, ``ptr`` int64 [N + 1]: a node-sorted list as ``ConvGraph`` holds them (trusted).
        More than 128 columns are summed 128 at a time."""
        rows = _need_cuda(rows).contiguous().float()
        N, D = ptr.shape[0] - 1, rows.shape[1]
        if rows.dim() != 2 or order.dtype != torch.int32 or ptr.dtype != torch.int64 or order.device != rows.device or ptr.device != rows.device:
            raise RuntimeError('ddk: seg_sum takes rows [E, D], an int32 order and an int64 ptr [N + 1] on the device of rows')
        if rows.shape[0] == 0 or N == 0 or D == 0:
            return torch.zeros((N, D), dtype=torch.float32, device=rows.device)
        if D > 128:
            return torch.cat([self.seg_sum(rows[:, c:c + 128], order, ptr) for c in range(0, D, 128)], dim=1)
        nodes = torch.empty((N, D), dtype=torch.float32, device=rows.device)
        self._check(self.L.ddk_seg_sum(self.h, _ptr(rows), _ptr(order), _ptr(ptr), _ptr(nodes), N, D, _stream()), 'ddk_seg_sum')
        return nodes

    # ---- the radial MLP's hidden layer from the edge embedding and the node table ---------------------
    def _rhid_operands(self, graph, xs, emb, group_offsets, w1, b1, p):
        """checked operands of the radial hidden layer: (xs, emb, offsets as a ctypes int64 array, G, w1, b1, p)"""
        if not isinstance(graph, ConvGraph):
            raise RuntimeError('ddk: the radial hidden layer takes a ConvGraph (Context.conv_graph): its kernels trust the indices')
        xs, emb = (_need_cuda(t).contiguous().float() for t in (xs, emb))
        offs = [int(o) for o in group_offsets]
        G, E = len(offs) - 1, graph.E
        if not 1 <= G <= 4:
            raise RuntimeError(f'ddk: the radial hidden layer takes 1..4 edge groups; got {G}')
        if graph.n_in != graph.n_out or xs.dim() != 2 or xs.shape != (graph.n_in, 24):
            raise RuntimeError(f'ddk: the radial hidden layer takes xs [n_nodes, 24] and a graph with n_in == n_out == n_nodes; got {tuple(xs.shape)} and a '
                               f'graph of {graph.n_in} -> {graph.n_out} nodes')
        if emb.shape != (E, 24):
            raise RuntimeError(f'ddk: the radial hidden layer takes emb [E, 24] for a graph of {E} edges; got {tuple(emb.shape)}')
        if graph.src.device != xs.device or emb.device != xs.device:
            raise RuntimeError('ddk: the radial hidden layer takes a ConvGraph and emb on the device of xs')
        if offs[-1] != E:
            raise RuntimeError(f'ddk: the edge groups hold {offs[-1]} edges, the graph {E}')
        if w1 is not None:
            w1 = _need_cuda(w1).contiguous().float()
            if w1.shape != (G, 72, 72) or w1.device != xs.device:
                raise RuntimeError(f'ddk: the radial hidden layer takes w1 [G, 72, 72] = {(G, 72, 72)} on the device of xs; got {tuple(w1.shape)}')
        if b1 is not None:
            b1 = _need_cuda(b1).contiguous().float()
            if b1.shape != (G, 72) or b1.device != xs.device:
                raise RuntimeError(f'ddk: the radial hidden layer takes b1 [G, 72] = {(G, 72)} on the device of xs; got {tuple(b1.shape)}')
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise RuntimeError(f'ddk: the dropout rate must be in [0, 1); got {p}')
        return xs, emb, (C.c_int64 * (G + 1))(*offs), G, w1, b1, p

    def rhid_forward(self, graph, xs, emb, group_offsets, w1, b1, p=0.0, seed=0):
        """The radial MLP's hidden layer (ddk_rhid_forward): h [E, 72] = dropout_p(relu(w1[g] [emb | xs[graph.src] | xs[graph.dst]] + b1[g])) without the
        concatenated row.  ``xs`` [n_nodes, 24], ``emb`` [E, 24], ``w1`` [G, 72, 72], ``b1`` [G, 72]; the mask is a pure function of (seed, edge, column)
        (DDK_RHID_MASK_LAYOUT of include/ddk.h), ``p == 0`` draws nothing."""
        xs, emb, offs, G, w1, b1, p = self._rhid_operands(graph, xs, emb, group_offsets, w1, b1, p)
        if w1 is None or b1 is None:
            raise RuntimeError('ddk: rhid_forward needs w1 and b1')
        g = graph
        h = torch.empty((g.E, 72), dtype=torch.float32, device=xs.device)
        self._check(self.L.ddk_rhid_forward(self.h, _ptr(xs), g.n_in, _ptr(g.src), _ptr(g.dst), _ptr(emb), offs, G, _ptr(w1), _ptr(b1), p,
                                            _u64(seed, 'seed'), g.E, _ptr(h), _stream()), 'ddk_rhid_forward')
        return h

    def rhid_backward(self, graph, xs, emb, h, group_offsets, w1, grad_h, p=0.0, need=(True, True, True, True)):
        """The vector-Jacobian product of ``rhid_forward`` (ddk_rhid_backward): (grad_xs [n_nodes, 24], grad_emb [E, 24], grad_w1 [G, 72, 72], grad_b1
        [G, 72]), None where ``need`` is false.  ``h``: the forward's output (it carries the pattern of ReLU and Dropout; no seed is needed); ``w1`` may be
        None when only grad_w1 / grad_b1 are asked for.  No atomics: the same bits from call to call.  The workspace comes from torch's allocator and is
        released on return."""
        need = _need(need, 'rhid_backward', four=True)
        if w1 is None and any(need[:2]):
            raise RuntimeError('ddk: rhid_backward needs w1 for grad_xs and grad_emb')
        xs, emb, offs, G, w1, _, p = self._rhid_operands(graph, xs, emb, group_offsets, w1, None, p)
        g = graph
        h, grad_h = (_need_cuda(t).contiguous().float() for t in (h, grad_h))
        if h.shape != (g.E, 72) or grad_h.shape != (g.E, 72) or h.device != xs.device or grad_h.device != xs.device:
            raise RuntimeError('ddk: rhid_backward takes h and grad_h [E, 72] on the device of xs')
        outs, live = _outputs(need, ((g.n_in, 24), (g.E, 24), (G, 72, 72), (G, 72)), xs.device)
        if not live:
            return tuple(outs)
        ws = _workspace(self.L.ddk_rhid_workspace(g.E, G, g.n_in), f'no radial-hidden workspace for E = {g.E}, {G} groups, {g.n_in} nodes', xs.device)
        self._check(self.L.ddk_rhid_backward(self.h, _ptr(xs), g.n_in, _ptr(g.src), _ptr(g.dst), _ptr(g.src_order), _ptr(g.src_ptr), _ptr(g.dst_order),
                                             _ptr(g.dst_ptr), _ptr(emb), _ptr(h), offs, G, _ptr(w1), _ptr(grad_h), p, g.E, *[_ptr(o) for o in outs],
                                             _ptr(ws), _stream()), 'ddk_rhid_backward')
        return tuple(outs)      # (ws goes back to torch's allocator, which orders its reuse after these launches on the current stream)

    # ---- the edge embeddings in front of the conv stack -------------------------------------------------
    # The plain op is the latent op with L = 0 and no unconditional term: one operand checker and one caller serve both pairs of entries.
    def _eemb_operands(self, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p, latent=None):
        """checked operands of the edge embedding: the tensors as the entries take them, (n_a, n_b, F, n_sig, E), the scalars and the latent part
        (lat_a, lat_b, L, zero_latent, unc_a, uemb).  ``latent``: None for the plain op (L = 0, everything None), else (lat_a, lat_b, zero_latent, unc_a,
        uemb) with w1 [24, F + 64 + 2 L]"""
        F, L = 0 if feat is None else 4, 0
        if latent is not None:
            if not torch.is_tensor(w1) or w1.dim() != 2:
                raise RuntimeError('ddk: the latent edge embedding takes w1 [24, F + 64 + 2 L]')
            if w1.shape[1] - F - 64 not in (2, 4, 6, 8):
                raise RuntimeError(f'ddk: the latent edge embedding takes w1 [24, {F + 64} + 2 L] with L in 1..4; got {tuple(w1.shape)}')
            L = (w1.shape[1] - F - 64) // 2
        pos_a, pos_b, sig, w1, b1, w2 = (_need_cuda(t).contiguous().float() for t in (pos_a, pos_b, sig, w1, b1, w2))
        dev = pos_a.device
        if pos_a.dim() != 2 or pos_a.shape[1] != 3 or pos_b.dim() != 2 or pos_b.shape[1] != 3:
            raise RuntimeError(f'ddk: the edge embedding takes pos_a [Na, 3] and pos_b [Nb, 3]; got {tuple(pos_a.shape)} and {tuple(pos_b.shape)}')
        n_a, n_b = pos_a.shape[0], pos_b.shape[0]
        for name, t in (('idx_a', idx_a), ('idx_b', idx_b), ('sig_index', sig_index)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f'ddk: the edge embedding takes {name} as a contiguous int32 vector on the device of pos_a (its kernels trust the indices)')
        E = idx_a.shape[0]
        if idx_b.shape[0] != E or sig_index.shape[0] != n_a:
            raise RuntimeError(f'ddk: the edge embedding takes idx_a and idx_b [E] and sig_index [Na]; got {E}, {idx_b.shape[0]} and {sig_index.shape[0]} for Na = {n_a}')
        if sig.dim() != 2 or sig.shape[1] != 32 or sig.device != dev:
            raise RuntimeError(f'ddk: the edge embedding takes sig [T, 32] on the device of pos_a; got {tuple(sig.shape)}')
        if feat is not None:
            feat = _need_cuda(feat).contiguous().float()
            if feat.shape != (E, 4) or feat.device != dev:
                raise RuntimeError(f'ddk: the edge embedding takes feat [E, 4] = {(E, 4)} on the device of pos_a; got {tuple(feat.shape)}')
        for name, t, shape in (('w1', w1[:, :F + 64] if L else w1, (24, F + 64)), ('b1', b1, (24,)), ('w2', w2, (24, 24))):      # (w1's latent columns were counted above)
            if t.shape != shape or t.device != dev:
                raise RuntimeError(f'ddk: the edge embedding takes {name} {list(shape)} on the device of pos_a; got {tuple(t.shape)}')
        if b2 is not None:
            b2 = _need_cuda(b2).contiguous().float()
            if b2.shape != (24,) or b2.device != dev:
                raise RuntimeError(f'ddk: the edge embedding takes b2 [24] on the device of pos_a; got {tuple(b2.shape)}')
        p, start, stop = float(p), float(start), float(stop)
        if not 0.0 <= p < 1.0:
            raise RuntimeError(f'ddk: the dropout rate must be in [0, 1); got {p}')
        if not start < stop:
            raise RuntimeError(f'ddk: the distance expansion needs start < stop; got {start}, {stop}')
        if E and (n_a == 0 or n_b == 0 or sig.shape[0] == 0):
            raise RuntimeError('ddk: the edge embedding has edges without nodes or graphs')
        t, n, sc = (pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, w1, b1, w2, b2), (n_a, n_b, F, sig.shape[0], E), (start, stop, p)
        if latent is None:
            return t, n, sc, (None, None, 0, False, None, None)
        lat_a, lat_b, zero_latent, unc_a, uemb = latent
        zero_latent = bool(zero_latent)
        if zero_latent:
            lat_a = lat_b = None
        else:
            if lat_a is None or lat_b is None:
                raise RuntimeError('ddk: the latent edge embedding takes lat_a and lat_b unless zero_latent is set')
            lat_a, lat_b = (_need_cuda(x).contiguous().float() for x in (lat_a, lat_b))
            if lat_a.shape != (n_a, L) or lat_b.shape != (n_b, L) or lat_a.device != dev or lat_b.device != dev:
                raise RuntimeError(f'ddk: the latent edge embedding takes lat_a [Na, L] = {(n_a, L)} and lat_b [Nb, L] = {(n_b, L)} on the device of pos_a; got '
                                   f'{tuple(lat_a.shape)} and {tuple(lat_b.shape)}')
        if (unc_a is None) != (uemb is None):
            raise RuntimeError('ddk: the latent edge embedding takes unc_a and uemb together')
        if unc_a is not None:
            unc_a, uemb = _need_cuda(unc_a).contiguous().float().reshape(-1), _need_cuda(uemb).contiguous().float().reshape(-1)
            if unc_a.shape != (n_a,) or uemb.shape != (24,) or unc_a.device != dev or uemb.device != dev:
                raise RuntimeError(f'ddk: the latent edge embedding takes unc_a [Na] = {(n_a,)} and uemb [24] on the device of pos_a; got {tuple(unc_a.shape)} and '
                                   f'{tuple(uemb.shape)}')
        return t, n, sc, (lat_a, lat_b, L, zero_latent, unc_a, uemb)

    def _eemb_call(self, direction, t, n, sc, seed, lat, tail):
        """``ddk_eemb_<direction>`` for L == 0, ``ddk_eemb_latent_<direction>`` with the latent arguments behind the seed otherwise; ``tail``: what follows"""
        pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, w1, b1, w2, b2 = t
        n_a, n_b, F, T, E = n
        start, stop, p = sc
        lat_a, lat_b, L, zero, unc_a, uemb = lat
        who = ('ddk_eemb_latent_' if L else 'ddk_eemb_') + direction
        latent = (_ptr(lat_a), _ptr(lat_b), L, int(zero), _ptr(unc_a), _ptr(uemb)) if L else ()
        self._check(getattr(self.L, who)(self.h, _ptr(pos_a), n_a, _ptr(pos_b), n_b, _ptr(idx_a), _ptr(idx_b), _ptr(feat), F, _ptr(sig), T, _ptr(sig_index),
                                         start, stop, 32, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), p, _u64(seed, 'seed'), *latent, *tail, _stream()), who)

    def eemb_forward(self, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p=0.0, seed=0):
        """One edge group's embedding and spherical harmonics (ddk_eemb_forward): (emb [E, 24], sh [E, 4]) with
        ``emb = w2 dropout_p(relu(w1 [feat | sig[sig_index[idx_a]] | smearing(|pos_b[idx_b] - pos_a[idx_a]|)] + b1)) + b2`` and ``sh = [1 | sqrt3 unit vector]``.
        ``idx_a``, ``idx_b`` [E], ``sig_index`` [Na]: int32, trusted; ``feat`` [E, 4] or None; ``start``, ``stop``: of the 32 Gaussians.  The mask is a pure
        function of (seed, edge position, column) (DDK_EEMB_MASK_LAYOUT of include/ddk.h); nothing per edge is kept for the backward."""
        t, n, sc, lat = self._eemb_operands(pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p)
        if t[-1] is None:
            raise RuntimeError('ddk: eemb_forward needs b2')
        return self._eemb_outputs(t, n, sc, seed, lat)

    def _eemb_outputs(self, t, n, sc, seed, lat):
        """(emb [E, 24], sh [E, 4]) of checked operands"""
        E, dev = n[4], t[0].device
        emb, sh = torch.empty((E, 24), dtype=torch.float32, device=dev), torch.empty((E, 4), dtype=torch.float32, device=dev)
        if E:
            self._eemb_call('forward', t, n, sc, seed, lat, (E, _ptr(emb), _ptr(sh)))
        return emb, sh

    def eemb_backward(self, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, grad_emb, p=0.0, seed=0, need=(True, True, True, True)):
        """The vector-Jacobian product of ``eemb_forward`` for its parameters (ddk_eemb_backward): (grad_w1 [24, K], grad_b1 [24], grad_w2 [24, 24],
        grad_b2 [24]), None where ``need`` is false.  The hidden layer and the mask are recomputed from the coordinates and ``seed``; the workspace holds
        the slice images alone, comes from torch's allocator and is released on return.  No atomics: the same bits from call to call."""
        need = _need(need, 'eemb_backward', four=True)
        t, n, sc, lat = self._eemb_operands(pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, None, p)
        F, E, dev = n[2], n[4], t[0].device
        grad_emb = self._eemb_grad_emb('eemb_backward', grad_emb, E, dev)
        outs, _ = _outputs(need, ((24, F + 64), (24,), (24, 24), (24,)), dev)      # (never empty)
        ws = _workspace(self.L.ddk_eemb_workspace(E, F + 64), f'no edge-embedding workspace for E = {E}, K = {F + 64}', dev)
        self._eemb_call('backward', t, n, sc, seed, lat, (_ptr(grad_emb) if E else None, E, *[_ptr(o) for o in outs], _ptr(ws)))
        return tuple(outs)      # (ws goes back to torch's allocator, which orders its reuse after these launches on the current stream)

    @staticmethod
    def _eemb_grad_emb(who, grad_emb, E, dev):
        grad_emb = _need_cuda(grad_emb).contiguous().float()
        if grad_emb.shape != (E, 24) or grad_emb.device != dev:
            raise RuntimeError(f'ddk: {who} takes grad_emb [E, 24] = {(E, 24)} on the device of pos_a; got {tuple(grad_emb.shape)}')
        return grad_emb

    def eemb_latent_forward(self, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, lat_a, lat_b, zero_latent=False, unc_a=None,
                            uemb=None, p=0.0, seed=0):
        """``eemb_forward`` with the latent columns (ddk_eemb_latent_forward): the row is ``[feat | sig | smearing | lat_a[idx_a] | lat_b[idx_b]]``, ``w1``
        [24, F + 64 + 2 L], and ``emb += unc_a[idx_a][:, None] * uemb`` where ``unc_a`` [Na] and ``uemb`` [24] are given.  ``zero_latent``: the 2 L columns
        hold zeros and the tables are not read (the cross group).  Returns (emb [E, 24], sh [E, 4])."""
        t, n, sc, lat = self._eemb_operands(pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, b2, p,
                                            (lat_a, lat_b, zero_latent, unc_a, uemb))
        if t[-1] is None:
            raise RuntimeError('ddk: eemb_latent_forward needs b2')
        return self._eemb_outputs(t, n, sc, seed, lat)

    def eemb_latent_backward(self, pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, lat_a, lat_b, grad_emb, zero_latent=False,
                             unc_a=None, uemb=None, p=0.0, seed=0, graph=None, need=(True,) * 7):
        """The vector-Jacobian product of ``eemb_latent_forward`` (ddk_eemb_latent_backward): (grad_w1 [24, K], grad_b1 [24], grad_w2 [24, 24], grad_b2 [24],
        grad_uemb [24], grad_lat_a [Na, L], grad_lat_b [Nb, L]), None where ``need`` is false.  ``graph``: ``Context.conv_graph(idx_a, idx_b, Nb, Na)``, the
        node-sorted edge lists the latent's gradient is summed along (needed for grad_lat_a / grad_lat_b unless ``zero_latent``).  Per-edge rows [E, 2 L] and
        the slice images are the whole workspace; no atomics: the same bits from call to call and for every subset of ``need``."""
        need = tuple(bool(x) for x in need)
        if len(need) != 7 or not any(need):
            raise RuntimeError('ddk: eemb_latent_backward needs at least one of its seven gradients to compute')
        t, n, sc, lat = self._eemb_operands(pos_a, pos_b, idx_a, idx_b, feat, sig, sig_index, start, stop, w1, b1, w2, None, p,
                                            (lat_a, lat_b, zero_latent, unc_a, uemb))
        n_a, n_b, F, _, E = n
        dev, L = t[0].device, lat[2]
        K = F + 64 + 2 * L
        grad_emb = self._eemb_grad_emb('eemb_latent_backward', grad_emb, E, dev)
        tables = (None,) * 4
        if E and not lat[3] and (need[5] or need[6]):
            if not isinstance(graph, ConvGraph) or graph.E != E or graph.n_out != n_a or graph.n_in != n_b or graph.src.device != dev:
                raise RuntimeError('ddk: eemb_latent_backward takes graph = Context.conv_graph(idx_a, idx_b, Nb, Na) on the device of pos_a for the latent gradients')
            tables = (graph.src_order, graph.src_ptr, graph.dst_order, graph.dst_ptr)
        shapes = ((24, K), (24,), (24, 24), (24,), (24,), (n_a, L), (n_b, L))
        outs, live = _outputs(need, shapes, dev)
        if not live:
            return tuple(outs)
        outs = [o if o is None or o.numel() else None for o in outs]      # (an empty node table has no address)
        ws = _workspace(self.L.ddk_eemb_latent_workspace(E, K, L), f'no latent edge-embedding workspace for E = {E}, K = {K}, L = {L}', dev)
        self._eemb_call('backward', t, n, sc, seed, lat, (*[_ptr(x) for x in tables], _ptr(grad_emb) if E else None, E, *[_ptr(o) for o in outs], _ptr(ws)))
        return tuple(torch.zeros(s, dtype=torch.float32, device=dev) if (on and o is None) else o for on, o, s in zip(need, outs, shapes))

    # ---- the ragged straight-through Gumbel softmax ------------------------------------------------------
    @staticmethod
    def _gumbel_operands(a_l, a_r, lig_ptr, rec_ptr, temperature, who):
        a_l, a_r = (_need_cuda(x).contiguous().float() for x in (a_l, a_r))
        return (a_l, a_r, *_ragged_tables(who, a_l, a_r, lig_ptr, rec_ptr), _temperature(who, temperature))

    def gumbel_softmax(self, logit_l, logit_r, lig_ptr, rec_ptr, temperature, seed, stream_ids, sample=0, draw=0):
        """The straight-through Gumbel softmax of every graph and latent dimension over the graph's ligand nodes followed by its receptor nodes
        (ddk_gumbel_softmax_batch; the noise is DDK_GUMBEL_LAYOUT of include/ddk.h): (out_l, out_r, y_l, y_r), ``out`` the one-hot sample carrying the soft
        ``y``'s gradient, ``y`` what ``gumbel_softmax_backward`` reads.  ``lig_ptr`` / ``rec_ptr``: int64 [G + 1] on the device; ``stream_ids``: uint64-valued
        [G] (a device int64 tensor holding the bit patterns, or host integers)."""
        logit_l, logit_r, G, D, T = self._gumbel_operands(logit_l, logit_r, lig_ptr, rec_ptr, temperature, 'gumbel_softmax')
        dev = logit_l.device
        if torch.is_tensor(stream_ids):
            st = stream_ids.to(dev).contiguous()
            if st.dtype != torch.int64 or st.shape != (G,):
                raise RuntimeError(f'ddk: gumbel_softmax takes stream_ids as {G} 64-bit integers')
        else:
            st = h2d_async(torch.from_numpy(np.ascontiguousarray([_u64(v, 'rng_stream') for v in stream_ids], dtype=np.uint64).view(np.int64)), dev)
            if st.shape != (G,):
                raise RuntimeError(f'ddk: gumbel_softmax takes {G} stream ids; got {st.shape[0]}')
        _need_int31('gumbel_softmax', draw=draw, sample=sample)
        y_l, y_r, out_l, out_r = torch.empty_like(logit_l), torch.empty_like(logit_r), torch.empty_like(logit_l), torch.empty_like(logit_r)
        self._check(self.L.ddk_gumbel_softmax_batch(self.h, G, D, _ptr(logit_l), logit_l.shape[0], _ptr(logit_r), logit_r.shape[0], _ptr(lig_ptr), _ptr(rec_ptr), T,
                                                    C.c_uint64(_u64(seed, 'seed')), _ptr(st), int(sample), int(draw), _ptr(y_l), _ptr(y_r), _ptr(out_l),
                                                    _ptr(out_r), _stream()), 'ddk_gumbel_softmax_batch')
        return out_l, out_r, y_l, y_r

    def gumbel_pick_samples(self, logit_l, logit_r, B, temperature, seed, stream, sample0=0, draw=0):
        """The one-hot latents of ``B`` samples of ONE complex from its one pair of logit tables [n_lig, D], [n_rec, D] (ddk_gumbel_pick_samples, one launch):
        (lig_latent [B n_lig, D], rec_latent [B n_rec, D], choices int32 [B, D]).  Sample b's rows are, bit for bit, ``gumbel_softmax``'s ``out`` for the one
        graph with ``sample = sample0 + b`` and the same seed, ``stream`` (the complex's 64-bit id), draw and temperature; ``choices`` holds the position of
        the one, ligand nodes first, then n_lig + the receptor index."""
        logit_l, logit_r = (_need_cuda(x).contiguous().float() for x in (logit_l, logit_r))
        dev = logit_l.device
        _, D = _ragged_tables('gumbel_pick_samples', logit_l, logit_r)
        B = int(B)
        if not 1 <= B <= 65536:
            raise RuntimeError(f'ddk: gumbel_pick_samples takes 1..65536 samples; got {B}')
        T = _temperature('gumbel_pick_samples', temperature)
        _need_int31('gumbel_pick_samples', draw=draw, sample0=sample0)
        n_l, n_r = logit_l.shape[0], logit_r.shape[0]
        lat_l, lat_r = torch.empty((B * n_l, D), device=dev), torch.empty((B * n_r, D), device=dev)
        choices = torch.empty((B, D), dtype=torch.int32, device=dev)
        self._check(self.L.ddk_gumbel_pick_samples(self.h, B, D, _ptr(logit_l), n_l, _ptr(logit_r), n_r, T, C.c_uint64(_u64(seed, 'seed')),
                                                   C.c_uint64(_u64(stream, 'rng_stream')), int(sample0), int(draw), _ptr(lat_l), _ptr(lat_r), _ptr(choices),
                                                   _stream()), 'ddk_gumbel_pick_samples')
        return lat_l, lat_r, choices

    def gumbel_softmax_backward(self, y_l, y_r, lig_ptr, rec_ptr, temperature, grad_out_l, grad_out_r):
        """(grad_logit_l, grad_logit_r) = y (g - sum g y) / T per graph and latent dimension from the saved ``y`` (ddk_gumbel_softmax_batch_backward)"""
        y_l, y_r, G, D, T = self._gumbel_operands(y_l, y_r, lig_ptr, rec_ptr, temperature, 'gumbel_softmax_backward')
        g_l, g_r = (_need_cuda(x).contiguous().float() for x in (grad_out_l, grad_out_r))
        if g_l.shape != y_l.shape or g_r.shape != y_r.shape or g_l.device != y_l.device or g_r.device != y_l.device:
            raise RuntimeError('ddk: gumbel_softmax_backward takes grad_out of the shapes of y on its device')
        out_l, out_r = torch.empty_like(y_l), torch.empty_like(y_r)
        self._check(self.L.ddk_gumbel_softmax_batch_backward(self.h, G, D, _ptr(y_l), y_l.shape[0], _ptr(y_r), y_r.shape[0], _ptr(lig_ptr), _ptr(rec_ptr), T,
                                                             _ptr(g_l), _ptr(g_r), _ptr(out_l), _ptr(out_r), _stream()), 'ddk_gumbel_softmax_batch_backward')
        return out_l, out_r

    def latent_keep(self, seed, streams, rate, draw=0, sample=0):
        """keep flag (1.0 / 0.0, float32 host array) of each complex of ``streams`` for noising ``draw``: the uniform of purpose RNG_LATENT_KEEP_PURPOSE
        is at or above ``rate`` (ddk_rng_latent_keep; computed on the host, no kernel)"""
        for k, v in dict(draw=draw, sample=sample).items():
            if not -(1 << 31) <= int(v) < 1 << 31:
                raise ValueError(f'ddk: {k} = {v} does not fit an int32')
        st = np.ascontiguousarray([_u64(v, 'rng_stream') for v in streams], dtype=np.uint64)
        out = np.empty(st.size, dtype=np.float32)
        self._check(self.L.ddk_rng_latent_keep(self.h, C.c_uint64(_u64(seed, 'seed')), st.size, st.ctypes.data_as(C.c_void_p), int(sample), int(draw), float(rate),
                                               out.ctypes.data_as(C.c_void_p)), 'ddk_rng_latent_keep')
        return out

    def decoding_index(self, seed, streams, D, draw=0, sample=0):
        """the decoding index in 0 .. D - 1 (int32 host array) of each complex of ``streams`` for draw ``draw``: purpose RNG_DECODING_INDEX_PURPOSE, in
        integer arithmetic (ddk_rng_decoding_index; computed on the host, no kernel)"""
        for k, v in dict(draw=draw, sample=sample, D=D).items():
            if not -(1 << 31) <= int(v) < 1 << 31:
                raise ValueError(f'ddk: {k} = {v} does not fit an int32')
        st = np.ascontiguousarray([_u64(v, 'rng_stream') for v in streams], dtype=np.uint64)
        out = np.empty(st.size, dtype=np.int32)
        self._check(self.L.ddk_rng_decoding_index(self.h, C.c_uint64(_u64(seed, 'seed')), st.size, st.ctypes.data_as(C.c_void_p), int(sample), int(draw), int(D),
                                                  out.ctypes.data_as(C.c_void_p)), 'ddk_rng_decoding_index')
        return out

    # ---- the AR model's ragged node cross-entropy ------------------------------------------------------
    @staticmethod
    def _node_ce_operands(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft, who):
        """everything the host can see of the operands of the two node cross-entropy calls: shapes, dtypes, D, G, contiguity, the device"""
        for name, t in (('logit_l', logit_l), ('logit_r', logit_r), ('teacher_l', teacher_l), ('teacher_r', teacher_r)):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError(f'ddk: {who} takes {name} as a tensor on the GPU (no CPU fallback)')
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f'ddk: {who} takes {name} as a contiguous float32 tensor; got {t.dtype}, contiguous = {t.is_contiguous()}')
        dev = logit_l.device
        for name, t, rows in (('logit_l', logit_l, teacher_l.shape[0]), ('logit_r', logit_r, teacher_r.shape[0])):
            if not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)) or t.shape[0] != rows:
                raise RuntimeError(f'ddk: {who} takes {name} as one logit per row of its teacher table ([{rows}] or [{rows}, 1]); got {tuple(t.shape)}')
        G, D = _ragged_tables(who, teacher_l, teacher_r, lig_ptr, rec_ptr)      # (the teacher's)
        if not torch.is_tensor(column) or column.dtype != torch.int32 or column.shape != (G,) or not column.is_contiguous():
            raise RuntimeError(f'ddk: {who} takes column as a contiguous int32 vector [G] = [{G}]')
        for name, t in (('logit_r', logit_r), ('teacher_l', teacher_l), ('column', column)):      # (the other three are on teacher_l's)
            if t.device != dev:
                raise RuntimeError(f'ddk: {who} takes every operand on one device; {name} is on {t.device}, logit_l on {dev}')
        if soft not in (0, 1, False, True):
            raise RuntimeError(f'ddk: {who} takes soft as 0 or 1; got {soft!r}')
        return G, D

    def node_cross_entropy(self, logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft=False, out=None):
        """The cross-entropy of every graph over its ligand nodes followed by its receptor nodes (ddk_node_cross_entropy_batch): (loss [G] float32, pick [G],
        target [G] int64, saved [G, 2] float64 = what ``node_cross_entropy_backward`` reads).  ``out``: the four tensors to write into (a graph with a bad
        pointer pair or column is left unwritten); default: fresh ones, loss NaN and the indices -1 where nothing is written."""
        G, D = self._node_ce_operands(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft, 'node_cross_entropy')
        dev = logit_l.device
        if out is None:
            out = (torch.full((G,), float('nan'), dtype=torch.float32, device=dev), torch.full((G,), -1, dtype=torch.int64, device=dev),
                   torch.full((G,), -1, dtype=torch.int64, device=dev), torch.zeros((G, 2), dtype=torch.float64, device=dev))
        loss, pick, target, saved = out
        for name, t, dtype, shape in (('loss', loss, torch.float32, (G,)), ('pick', pick, torch.int64, (G,)), ('target', target, torch.int64, (G,)),
                                      ('saved', saved, torch.float64, (G, 2))):
            if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f'ddk: node_cross_entropy takes out.{name} as a contiguous {dtype} tensor {shape} on the device of the logits')
        self._check(self.L.ddk_node_cross_entropy_batch(self.h, G, D, _ptr(logit_l), logit_l.shape[0], _ptr(logit_r), logit_r.shape[0], _ptr(lig_ptr),
                                                        _ptr(rec_ptr), _ptr(teacher_l), _ptr(teacher_r), _ptr(column), int(bool(soft)), _ptr(loss), _ptr(pick),
                                                        _ptr(target), _ptr(saved), _stream()), 'ddk_node_cross_entropy_batch')
        return loss, pick, target, saved

    def node_cross_entropy_backward(self, grad, logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, target, saved, soft=False, out=None):
        """(grad_logit_l, grad_logit_r) = grad_g (softmax(s) - label) per graph from the saved log-sum-exps (ddk_node_cross_entropy_batch_backward).  ``out``:
        the two tables to write into; default: zeros (rows of no valid graph stay zero)."""
        G, D = self._node_ce_operands(logit_l, logit_r, lig_ptr, rec_ptr, teacher_l, teacher_r, column, soft, 'node_cross_entropy_backward')
        dev = logit_l.device
        grad = _need_cuda(grad).contiguous().float()
        if tuple(grad.shape) != (G,) or grad.device != dev:
            raise RuntimeError(f'ddk: node_cross_entropy_backward takes grad [G] = [{G}] on the device of the logits; got {tuple(grad.shape)}')
        if target.dtype != torch.int64 or tuple(target.shape) != (G,) or saved.dtype != torch.float64 or tuple(saved.shape) != (G, 2) or \
                not target.is_contiguous() or not saved.is_contiguous() or target.device != dev or saved.device != dev:
            raise RuntimeError('ddk: node_cross_entropy_backward takes target (int64 [G]) and saved (float64 [G, 2]) as node_cross_entropy returned them')
        g_l, g_r = (torch.zeros_like(logit_l), torch.zeros_like(logit_r)) if out is None else out
        for name, t, like in (('grad_logit_l', g_l, logit_l), ('grad_logit_r', g_r, logit_r)):
            if t.dtype != torch.float32 or t.shape != like.shape or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f'ddk: node_cross_entropy_backward takes out.{name} as a contiguous float32 tensor of the shape of its logits')
        self._check(self.L.ddk_node_cross_entropy_batch_backward(self.h, G, D, _ptr(logit_l), logit_l.shape[0], _ptr(logit_r), logit_r.shape[0], _ptr(lig_ptr),
                                                                 _ptr(rec_ptr), _ptr(teacher_l), _ptr(teacher_r), _ptr(column), int(bool(soft)), _ptr(grad),
                                                                 _ptr(target), _ptr(saved), _ptr(g_l), _ptr(g_r), _stream()),
                    'ddk_node_cross_entropy_batch_backward')
        return g_l, g_r

    def tp_weight_numel(self, layer):
        """W of conv layer ``layer``: the length of a FasterTensorProduct weight row (tensor_layers.py:56-63)."""
        return tp_id_shape(layer, self.cfg.ns, self.cfg.nv)['W']

    def conv_forward(self, layer, x, edge_src, edge_dst, group_offsets, edge_attr, sh, dout):
        x, edge_attr, sh = x.contiguous().float(), edge_attr.contiguous().float(), sh.contiguous().float()
        edge_src, edge_dst = edge_src.contiguous().int(), edge_dst.contiguous().int()
        N = x.shape[0]
        out = torch.empty((N, dout), dtype=torch.float32, device=x.device)
        go = (C.c_int64 * 5)(*[int(v) for v in group_offsets])
        self._check(self.L.ddk_conv_forward(self.h, layer, _ptr(x), N, _ptr(edge_src), _ptr(edge_dst), go, _ptr(edge_attr),
                                            _ptr(sh), _ptr(out), _stream()), 'ddk_conv_forward')
        return out

    # ---- poses -> distinct modes (no complex is involved: poses from any source) ----------------
    def pairwise_rmsd(self, pos, atom_mask=None, perms=None):
        """All-pairs symmetry-corrected RMSD of the poses pos [B, n_lig, 3] (device) in their common frame, no alignment: tensor [B, B], symmetric
        with a zero diagonal.  atom_mask [n_lig]: the atoms that count (filterHs, evaluate.py:297); perms [K, n_lig] (int): the ligand's graph
        automorphisms, the table of Complex.pose_metrics (None: identity only).  A host table is checked here; a device table is passed as it is (the
        kernel gives a row with an entry outside the ligand +inf).  Nothing is read back."""
        pos = _need_cuda(pos)
        if pos.dim() != 3 or pos.shape[2] != 3:
            raise RuntimeError('ddk: pairwise_rmsd takes poses [B, n_lig, 3]; got ' + str(tuple(pos.shape)))
        pos = pos.contiguous().float()
        B, n_lig = pos.shape[0], pos.shape[1]
        m = None
        if atom_mask is not None:
            m = h2d_async(torch.as_tensor(atom_mask).reshape(-1).ne(0).to(torch.uint8).contiguous(), pos.device)
            if m.shape[0] != n_lig:
                raise RuntimeError(f'ddk: atom_mask has {m.shape[0]} entries for {n_lig} ligand atoms')
        pm = None
        if perms is not None:
            pm = torch.as_tensor(perms)
            if pm.dim() != 2 or pm.shape[0] < 1 or pm.shape[1] != n_lig:
                raise RuntimeError(f'ddk: the permutation table must be [K >= 1, {n_lig}]; got ' + str(tuple(pm.shape)))
            if not pm.is_cuda and (int(pm.min()) < 0 or int(pm.max()) >= n_lig):
                raise RuntimeError('ddk: permutation table entries must be ligand atom indices')
            pm = h2d_async(pm.to(torch.int32).contiguous(), pos.device)
        out = torch.empty((B, B), dtype=torch.float32, device=pos.device)
        self._check(self.L.ddk_pose_pairwise_rmsd(self.h, B, n_lig, _ptr(pos), _ptr(m), _ptr(pm), 0 if pm is None else pm.shape[0], _ptr(out), _stream()),
                    'ddk_pose_pairwise_rmsd')
        return out

    def cluster_poses(self, pos, scores=None, cutoff=2.0, atom_mask=None, perms=None):
        """Which of the poses pos [B, n_lig, 3] are the same binding mode: pairwise_rmsd, then greedy leader clustering by score on the device
        (scores [B], higher is better, None: index order; ties go to the lower index, NaN ranks last): the best-scored unassigned pose leads the next
        cluster and every unassigned pose within `cutoff` of it joins.  Returns PoseClusters(rmsd, cluster, leaders, n_clusters), device tensors;
        nothing is read back.  B <= 1024."""
        rmsd = self.pairwise_rmsd(pos, atom_mask=atom_mask, perms=perms)
        B, dev = rmsd.shape[0], rmsd.device
        sc = None
        if scores is not None:
            sc = _need_cuda(scores).to(dev).float().reshape(-1).contiguous()
            if sc.shape[0] != B:
                raise RuntimeError(f'ddk: {sc.shape[0]} scores for {B} poses')
        cluster, leaders = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        n = torch.empty(1, dtype=torch.int32, device=dev)
        self._check(self.L.ddk_pose_cluster(self.h, B, _ptr(rmsd), _ptr(sc), float(cutoff), _ptr(cluster), _ptr(leaders), _ptr(n), _stream()),
                    'ddk_pose_cluster')
        return PoseClusters(rmsd, cluster, leaders, n)

    def ligand_automorphisms(self, colour, bond_index, atom_mask=None, cap=65536):
        """The automorphism table that pairwise_rmsd, cluster_poses and Complex.pose_metrics take as ``perms``, enumerated on the device
        (ddk_ligand_automorphisms, include/ddk.h): every bijection of the kept atoms that keeps ``colour`` [n_lig] (int) and the bonds
        ``bond_index`` [2, E] (either or both directions, duplicates allowed).  ``atom_mask`` [n_lig]: the kept atoms (None: all); masked-out atoms
        map to themselves.  Returns (perms, count), device tensors: perms is the whole [cap, n_lig] int32 buffer, of which the first count[0] rows are
        written (row 0 the identity); count [2] int32 = (rows, status), status 0 complete, 1 overflow (the search held more than ``cap`` partial maps
        at some level), 2 a bond index outside the ligand; with 1 or 2 the identity is the only row.  Nothing is read back: see usable_automorphisms.
        n_lig <= 256, cap <= 2^20; the call holds about 2 * cap * n_lig bytes of workspace while it runs."""
        dev = torch.device('cuda', self.device)
        col = h2d_async(torch.as_tensor(colour).reshape(-1).to(torch.int32).contiguous(), dev)
        n_lig, cap = col.shape[0], int(cap)
        bi = torch.as_tensor(bond_index)
        if bi.numel() and (bi.dim() != 2 or bi.shape[0] != 2):
            raise RuntimeError('ddk: bond_index must be [2, E]; got ' + str(tuple(bi.shape)))
        E = bi.numel() // 2
        bi = h2d_async(bi.to(torch.int32).contiguous(), dev) if E else None
        m = None
        if atom_mask is not None:
            m = h2d_async(torch.as_tensor(atom_mask).reshape(-1).ne(0).to(torch.uint8).contiguous(), dev)
            if m.shape[0] != n_lig:
                raise RuntimeError(f'ddk: atom_mask has {m.shape[0]} entries for {n_lig} ligand atoms')
        nbytes = self.L.ddk_ligand_automorphisms_workspace(n_lig, cap)
        ok = nbytes >= 0      # a broken limit: the call below says which
        perms = torch.empty((cap, n_lig) if ok else (1, 1), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self._check(self.L.ddk_ligand_automorphisms(self.h, n_lig, _ptr(col), _ptr(bi), E, _ptr(m), _ptr(perms), cap, _ptr(count), _ptr(ws), _stream()),
                    'ddk_ligand_automorphisms')
        return perms, count

    # ---- conformer matching (csrc/k_match.hip; ddk_conformer_rmsd / ddk_conformer_match of include/ddk.h) -------------
    def _match_problem(self, pos0, target, rot_bonds, mask_rotate, atom_mask):
        dev = torch.device('cuda', self.device)
        f = lambda a: h2d_async(torch.as_tensor(a).to(torch.float32).reshape(-1, 3).contiguous(), dev)
        pos0, target = f(pos0), f(target)
        n_lig = pos0.shape[0]
        if target.shape[0] != n_lig:
            raise RuntimeError(f'ddk: the target has {target.shape[0]} atoms, the conformer {n_lig}')
        rb = torch.as_tensor(rot_bonds).reshape(-1, 2)
        n_rot = rb.shape[0]
        mr = torch.as_tensor(mask_rotate).reshape(n_rot, -1) if n_rot else None
        if n_rot and mr.shape[1] != n_lig:
            raise RuntimeError(f'ddk: mask_rotate must be [{n_rot}, {n_lig}]; got ' + str(tuple(mr.shape)))
        rb = h2d_async(rb.to(torch.int32).contiguous(), dev) if n_rot else None
        mr = h2d_async(mr.ne(0).to(torch.uint8).contiguous(), dev) if n_rot else None
        m = None
        if atom_mask is not None:
            m = h2d_async(torch.as_tensor(atom_mask).reshape(-1).ne(0).to(torch.uint8).contiguous(), dev)
            if m.shape[0] != n_lig:
                raise RuntimeError(f'ddk: atom_mask has {m.shape[0]} entries for {n_lig} ligand atoms')
        return dev, n_lig, n_rot, pos0, target, rb, mr, m

    def conformer_rmsd(self, pos0, target, rot_bonds, mask_rotate, torsions, atom_mask=None, return_status=False):
        """The matching objective alone (ddk_conformer_rmsd): for every row of ``torsions`` [M, n_rot] the RMSD to ``target`` [n_lig, 3], after the optimal
        rigid fit, of the conformer ``pos0`` [n_lig, 3] with those torsion increments applied (utils/torsion.py:48-68; ``rot_bonds`` [n_rot, 2] = the
        (u, v) of ``bond_index[:, edge_mask].T``, ``mask_rotate`` [n_rot, n_lig]).  ``atom_mask``: the atoms that count (None: all).  Returns a device
        tensor [M]; with ``return_status`` also the status word [1] int32 (0; 2 a bad rotor table or fewer than 3 kept atoms; 3 a coordinate that is not
        finite: the RMSDs are then not written).  Nothing is read back."""
        dev, n_lig, n_rot, pos0, target, rb, mr, m = self._match_problem(pos0, target, rot_bonds, mask_rotate, atom_mask)
        tor = torch.as_tensor(torsions).to(torch.float32)
        tor = h2d_async(tor.reshape(-1, n_rot).contiguous() if n_rot else tor.reshape(tor.shape[0] if tor.dim() else 1, 0), dev)
        M = tor.shape[0]
        out = torch.empty(max(M, 1), dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        self._check(self.L.ddk_conformer_rmsd(self.h, n_lig, _ptr(pos0), _ptr(target), _ptr(m), _ptr(rb), _ptr(mr), n_rot, M, _ptr(tor) if n_rot else None,
                                              _ptr(out), _ptr(status), _stream()), 'ddk_conformer_rmsd')
        return (out[:M], status) if return_status else out[:M]

    def match_conformer(self, pos0, target, rot_bonds, mask_rotate, atom_mask=None, popsize=15, maxiter=15, polish_iters=128, n_islands=1, seed=0, stream=0,
                        tol=0.01):
        """Conformer matching (ddk_conformer_match; datasets_utils/conformer_matching.py): the torsion increments of the conformer ``pos0`` that bring it
        closest to ``target`` after a rigid fit, by the seeded generation-synchronous differential evolution and compass polish include/ddk.h documents.
        Returns a dict of device tensors: 'pos' [n_lig, 3] the matched conformer in the target's frame, 'torsions' [n_rot], 'rmsd' [] (rmsd_matching),
        'rmsd_rigid' [] (all torsions 0; rmsd <= rmsd_rigid always), 'generations' [], 'status' [] (0; 2 / 3 as conformer_rmsd: the other entries are
        then not written).  ``seed`` and ``stream`` (:func:`stream_id`) select the draws; the result is a pure function of the arguments.  The workspace is
        kept on the context per stream and grows as needed.  Nothing is read back."""
        dev, n_lig, n_rot, pos0, target, rb, mr, m = self._match_problem(pos0, target, rot_bonds, mask_rotate, atom_mask)
        for k, v in dict(popsize=popsize, maxiter=maxiter, polish_iters=polish_iters, n_islands=n_islands).items():
            if not -(1 << 31) <= int(v) < 1 << 31:
                raise ValueError(f'ddk: {k} = {v} does not fit an int32')
        opt = _lib.ddk_match_options(int(popsize), int(maxiter), float(tol), int(polish_iters), int(n_islands), _u64(seed, 'seed'), _u64(stream, 'rng_stream'))
        nbytes = self.L.ddk_conformer_match_workspace(n_lig, n_rot, int(popsize), int(n_islands))      # -1: a broken limit, the call below says which
        key = torch.cuda.current_stream(dev).cuda_stream      # (two calls on one stream run in order and may share the workspace)
        ws = self._match_ws.get(key)
        if ws is None or ws.numel() < max(nbytes, 16):
            ws = self._match_ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        tor = torch.empty(n_rot, dtype=torch.float32, device=dev)
        pos = torch.empty((n_lig, 3), dtype=torch.float32, device=dev)
        rmsd = torch.empty(2, dtype=torch.float32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        self._check(self.L.ddk_conformer_match(self.h, n_lig, _ptr(pos0), _ptr(target), _ptr(m), _ptr(rb), _ptr(mr), n_rot, C.byref(opt),
                                               _ptr(tor) if n_rot else None, _ptr(pos), _ptr(rmsd), _ptr(count), _ptr(ws), _stream()), 'ddk_conformer_match')
        return dict(pos=pos, torsions=tor, rmsd=rmsd[1], rmsd_rigid=rmsd[0], generations=count[0], status=count[1])

    # ---- the sampler's draws from the counter-based generator (csrc/k_rng.hip; DDK_RNG_LAYOUT of include/ddk.h) -------------
    def _rng_args(self, seed, stream, ints):
        for k, v in ints.items():
            if not -(1 << 31) <= int(v) < 1 << 31:      # (ctypes would wrap it silently)
                raise ValueError(f'ddk: {k} = {v} does not fit an int32')
        return C.c_uint64(_u64(seed, 'seed')), C.c_uint64(_u64(stream, 'rng_stream')), torch.device('cuda', self.device)

    def rng_noise(self, seed, stream, sample0, B, steps, n_cols, n_active_cols=None, step0=0, noise_coeff=None):
        """N(0,1) draws [steps, B, n_cols] (fresh device tensor) for ``Complex.sample``'s ``noise``: row (k, b) belongs to step step0 + k of the GLOBAL sample
        sample0 + b of complex ``stream`` (:func:`stream_id`) under ``seed``, whatever B, sample0, step0 and steps cut out of the whole.  Columns from
        ``n_active_cols`` on are 0; with ``noise_coeff`` [steps, 3] (host) a step whose three entries are zero is 0 (draw_noise's rule).  No read-back."""
        n_active_cols = n_cols if n_active_cols is None else n_active_cols
        s, st, dev = self._rng_args(seed, stream, dict(sample0=sample0, B=B, step0=step0, steps=steps, n_cols=n_cols, n_active_cols=n_active_cols))
        nc = None
        if noise_coeff is not None:
            nc = np.ascontiguousarray(noise_coeff, dtype=np.float32)
            if nc.shape != (steps, 3):
                raise ValueError(f'ddk: noise_coeff must be [steps, 3] = [{steps}, 3], got {nc.shape}')
        out = torch.empty((max(steps, 0), max(B, 0), max(n_cols, 0)), dtype=torch.float32, device=dev)
        self._check(self.L.ddk_rng_noise(self.h, s, st, sample0, B, step0, steps, n_cols, n_active_cols, None if nc is None else nc.ctypes.data_as(C.c_void_p),
                                         _ptr(out), _stream()), 'ddk_rng_noise')
        return out

    def rng_initial(self, seed, stream, sample0, B, n_rot, tr_sigma=1.0, torsions=True, translations=True, purpose_rot=RNG_PURPOSES['initial_rotation']):
        """The draws of randomize_position for the global samples sample0 .. sample0 + B - 1: (tor [B, n_rot] uniform in [-pi, pi) or None, rot [B, 3, 3]
        uniformly random rotation matrices, tr [B, 3] = tr_sigma * N(0,1) or None), fresh device tensors that go straight into
        ``Complex.randomize_position``.  ``purpose_rot`` 5: the rotation of ``ar_pos`` under ar_args.no_randomness.  No read-back."""
        s, st, dev = self._rng_args(seed, stream, dict(sample0=sample0, B=B, n_rot=n_rot, purpose_rot=purpose_rot))
        Bs, Rs = max(B, 0), max(n_rot, 0)
        tor = torch.empty((Bs, Rs), dtype=torch.float32, device=dev) if torsions else None
        rot = torch.empty((Bs, 3, 3), dtype=torch.float32, device=dev)
        tr = torch.empty((Bs, 3), dtype=torch.float32, device=dev) if translations else None
        self._check(self.L.ddk_rng_initial(self.h, s, st, sample0, B, n_rot, float(tr_sigma), purpose_rot, _ptr(tor), _ptr(rot), _ptr(tr), _stream()),
                    'ddk_rng_initial')
        return tor, rot, tr

    def rng_uniform(self, seed, stream, sample0, B, decoding_idx):
        """The uniforms [B] in [0, 1) of the AR pick of latent dimension ``decoding_idx`` (``Complex.ar_decode``) for the global samples sample0 ..; fresh
        device tensor, no read-back."""
        s, st, dev = self._rng_args(seed, stream, dict(sample0=sample0, B=B, decoding_idx=decoding_idx))
        out = torch.empty(max(B, 0), dtype=torch.float32, device=dev)
        self._check(self.L.ddk_rng_uniform(self.h, s, st, sample0, B, decoding_idx, _ptr(out), _stream()), 'ddk_rng_uniform')
        return out

    # ---- the forward process and the score-matching loss (csrc/k_so3.hip, csrc/k_noising.hip) -------------
    def so3_rows(self, eps_idx, cdf=True, score=True, exp_score_norm=True):
        """Rows ``eps_idx`` (host integers in [0, 1000), duplicates allowed) of the IGSO(3) tables of utils/so3.py, computed in fp64 on the device
        (ddk_so3_rows, include/ddk.h): (cdf [n, 2000], score [n, 2000], exp_score_norm [n]) float64 device tensors, None where not asked for.  The score
        rows carry the reference's inf / NaN where the density vanishes.  No read-back."""
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(eps_idx)).reshape(-1), dtype=np.int64)
        if idx.size and (idx.min() < -(1 << 31) or idx.max() >= 1 << 31):
            raise ValueError('ddk: an eps_idx entry does not fit an int32')
        idx = idx.astype(np.int32)
        n, dev = idx.size, torch.device('cuda', self.device)
        ok = 1 <= n <= SO3_MAX_ROWS      # a broken limit: the call below says which
        rows = n if ok else 1
        c = torch.empty((rows, SO3_X_N), dtype=torch.float64, device=dev) if cdf else None
        sc = torch.empty((rows, SO3_X_N), dtype=torch.float64, device=dev) if score else None
        e = torch.empty(rows, dtype=torch.float64, device=dev) if exp_score_norm else None
        self._check(self.L.ddk_so3_rows(self.h, n, idx.ctypes.data_as(C.c_void_p), _ptr(c), _ptr(sc), _ptr(e), _stream()), 'ddk_so3_rows')
        return c, sc, e

    def torus_score(self, x, sigma_idx):
        """torus.score(x, sigma) of utils/torus.py:43-52 for the device tensor ``x`` (any shape, fp32) at the table's sigma index ``sigma_idx`` (host
        integer in [0, 5000]: training.torus_sigma_index), evaluated in fp64 without the table (ddk_torus_score): a fresh fp32 tensor of x's shape."""
        x = _need_cuda(x).contiguous().float()
        out = torch.empty_like(x)
        self._rng_args(0, 0, dict(sigma_idx=sigma_idx))
        self._check(self.L.ddk_torus_score(self.h, x.numel(), _ptr(x), int(sigma_idx), _ptr(out), _stream()), 'ddk_torus_score')
        return out

    def rng_perturbation(self, seed, stream, sample0, B, n_rot, tr_sigma, tor_sigma, torus_sigma_idx, so3_cdf_row, so3_score_row=None, draw=0,
                         scores=True):
        """One noising of the global samples sample0 .. sample0 + B - 1 of complex ``stream`` under ``seed`` (ddk_rng_perturbation; purposes
        RNG_FORWARD_PURPOSES, ``draw`` in the step field): :data:`Perturbation` of fresh device tensors, the three updates ``Complex.se3_update`` takes
        and, with ``scores``, data.tr_score / rot_score / tor_score of apply_noise (None otherwise).  ``so3_cdf_row`` / ``so3_score_row``: one row of
        :meth:`so3_rows` (float64 device tensors [2000]) for the rotation's noise level.  No read-back."""
        s, st, dev = self._rng_args(seed, stream, dict(sample0=sample0, B=B, n_rot=n_rot, draw=draw, torus_sigma_idx=torus_sigma_idx))
        rows = []
        for name, row in (('so3_cdf_row', so3_cdf_row), ('so3_score_row', so3_score_row)):
            if row is not None:
                row = _need_cuda(row).contiguous()
                if row.dtype != torch.float64 or row.numel() != SO3_X_N:
                    raise ValueError(f'ddk: {name} must be a float64 tensor of {SO3_X_N} entries (one row of so3_rows)')
            rows.append(row)
        Bs, Rs = max(B, 0), max(n_rot, 0)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = Perturbation(new(Bs, 3), new(Bs, 3), new(Bs, Rs), *([new(Bs, 3), new(Bs, 3), new(Bs, Rs)] if scores else [None] * 3))
        c_out = _lib.ddk_perturbation(**{k: (v.data_ptr() if v is not None and v.numel() else None) for k, v in out._asdict().items()})
        self._check(self.L.ddk_rng_perturbation(self.h, s, st, sample0, B, draw, n_rot, float(tr_sigma), float(tor_sigma), int(torus_sigma_idx),
                                                _ptr(rows[0]), _ptr(rows[1]), C.byref(c_out), _stream()), 'ddk_rng_perturbation')
        return out

    def score_matching_loss(self, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2):
        """The six per-sample terms of loss_function(..., apply_mean=False) (utils/training.py:21-53; ddk_score_matching_loss): device tensor [B, 6] with
        the columns LOSS_COLUMNS.  Predictions and targets [B, 3], [B, 3] and [B, n_rot] (flat is fine); ``tor_pred`` None or n_rot = 0: the torsion
        terms are 0.  The three scalars are host numbers: the translation sigma, so3.score_norm(rot_sigma) and torus.score_norm(tor_sigma)."""
        f = lambda t, cols: _need_cuda(t).contiguous().float().reshape(-1, cols)
        tr_pred, rot_pred, tr_score, rot_score = (f(t, 3) for t in (tr_pred, rot_pred, tr_score, rot_score))
        B = tr_score.shape[0]
        n_rot = 0
        if tor_pred is not None and tor_score is not None and tor_score.numel():
            n_rot = tor_score.numel() // max(B, 1)
            tor_pred, tor_score = f(tor_pred, n_rot), f(tor_score, n_rot)
        else:
            tor_pred = tor_score = None
        for name, t, shape in (('tr_pred', tr_pred, (B, 3)), ('rot_pred', rot_pred, (B, 3)), ('rot_score', rot_score, (B, 3)),
                               ('tor_pred', tor_pred, (B, n_rot)), ('tor_score', tor_score, (B, n_rot))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f'ddk: {name} must hold {shape} values, got {tuple(t.shape)} (the library reads it through a raw pointer)')
        out = torch.empty((B, 6), dtype=torch.float32, device=tr_score.device)
        self._check(self.L.ddk_score_matching_loss(self.h, B, n_rot, _ptr(tr_pred), _ptr(rot_pred), _ptr(tor_pred), _ptr(tr_score), _ptr(rot_score),
                                                   _ptr(tor_score), float(tr_sigma), float(so3_score_norm), float(torus_score_norm2), _ptr(out),
                                                   _stream()), 'ddk_score_matching_loss')
        return out

    # ---- the same for a ragged batch of different complexes at different times (ddk_*_batch of include/ddk.h) -------------
    def _dev(self, a, dtype):
        """host array or tensor -> contiguous device tensor of ``dtype`` (a device tensor passes through without a copy when it already is one)"""
        dev = torch.device('cuda', self.device)
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.dtype(str(dtype).replace('torch.', ''))))
        return h2d_async(t.to(dtype).contiguous(), dev)

    @staticmethod
    def _check_ptr(name, ptr, total, what):
        """a prefix table given as a HOST array is checked here (a device tensor is checked by the kernel that reads it): starts at 0, never decreases,
        ends at the length of the array it cuts"""
        if torch.is_tensor(ptr) and ptr.is_cuda:
            return
        p = np.asarray(ptr.cpu() if torch.is_tensor(ptr) else ptr, dtype=np.int64).reshape(-1)
        if p.size < 2 or p[0] != 0 or (np.diff(p) < 0).any() or (total is not None and p[-1] != total):
            raise ValueError(f'ddk: {name} must be a non-decreasing prefix [G + 1] from 0 to {total if total is not None else "its total"} ({what}), got {p.tolist()}')

    def so3_table(self):
        """The whole IGSO(3) table, (cdf, score) float64 [1000, 2000] on the device (32 MB), computed by ddk_so3_rows on first use and kept on the context: a
        batch's ``so3_row`` entries are then the eps indices themselves, and a second batch pays nothing for its rows."""
        if getattr(self, '_so3_table', None) is None:
            cdf, score, _ = self.so3_rows(np.arange(SO3_N_EPS), exp_score_norm=False)
            self._so3_table = (cdf, score)
        return self._so3_table

    def forward_times(self, seed, streams, draw=0, sample=0):
        """t in [0, 1) of each complex of ``streams`` (:func:`stream_id` values) for noising ``draw`` (ddk_rng_forward_times, purpose RNG_TIME_PURPOSE):
        a float32 host array; computed on the host, no kernel."""
        for k, v in dict(draw=draw, sample=sample).items():
            if not -(1 << 31) <= int(v) < 1 << 31:
                raise ValueError(f'ddk: {k} = {v} does not fit an int32')
        st = np.ascontiguousarray([_u64(v, 'rng_stream') for v in streams], dtype=np.uint64)
        out = np.empty(st.size, dtype=np.float32)
        self._check(self.L.ddk_rng_forward_times(self.h, C.c_uint64(_u64(seed, 'seed')), st.size, st.ctypes.data_as(C.c_void_p), int(sample), int(draw),
                                                 out.ctypes.data_as(C.c_void_p)), 'ddk_rng_forward_times')
        return out

    def rng_perturbation_batch(self, seed, streams, samples, tor_ptr, tr_sigma, tor_sigma, torus_sigma_idx, so3_row, so3_cdf_rows, so3_score_rows=None,
                               draw=0, scores=True, T=None):
        """One noising of G graphs, each at its own noise level (ddk_rng_perturbation_batch): :data:`Perturbation` with tr / rot [G, 3] and the torsion
        members flat [T].  The per-graph tables (``streams`` uint64, ``samples`` / ``tor_ptr`` [G + 1] / ``torus_sigma_idx`` / ``so3_row`` int32, the two
        sigmas float32) are device tensors, or host arrays that are uploaded; ``T`` = tor_ptr[G] as a host integer (needed when tor_ptr is a device
        tensor).  ``so3_cdf_rows`` / ``so3_score_rows``: float64 [n_rows, 2000] (:meth:`so3_table` or :meth:`so3_rows`).  No read-back."""
        if T is None:
            if torch.is_tensor(tor_ptr) and tor_ptr.is_cuda:
                raise ValueError('ddk: rng_perturbation_batch needs T (= tor_ptr[G]) as a host integer when tor_ptr is a device tensor')
            T = int(np.asarray(tor_ptr).reshape(-1)[-1])
        self._check_ptr('tor_ptr', tor_ptr, T, 'the rotor counts of the graphs')
        s, _, dev = self._rng_args(seed, 0, dict(draw=draw, T=T))
        st = self._dev(np.asarray([_u64(v, 'rng_stream') for v in streams], dtype=np.uint64).view(np.int64), torch.int64) if not torch.is_tensor(streams) else streams
        G = st.numel()
        i32 = [self._dev(a, torch.int32) for a in (samples, tor_ptr, torus_sigma_idx, so3_row)]
        f32 = [self._dev(a, torch.float32) for a in (tr_sigma, tor_sigma)]
        for name, t, n in (('samples', i32[0], G), ('tor_ptr', i32[1], G + 1), ('torus_sigma_idx', i32[2], G), ('so3_row', i32[3], G), ('tr_sigma', f32[0], G),
                           ('tor_sigma', f32[1], G)):
            if t.numel() != n:
                raise ValueError(f'ddk: {name} must hold {n} entries for {G} graphs, got {t.numel()} (the library reads it through a raw pointer)')
        rows = []
        for name, t in (('so3_cdf_rows', so3_cdf_rows), ('so3_score_rows', so3_score_rows)):
            if t is not None:
                t = _need_cuda(t).contiguous()
                if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != SO3_X_N:
                    raise ValueError(f'ddk: {name} must be a float64 tensor [n_rows, {SO3_X_N}] (rows of so3_rows)')
            rows.append(t)
        n_rows = rows[0].shape[0] if rows[0] is not None else 0
        if rows[1] is not None and rows[1].shape[0] != n_rows:
            raise ValueError('ddk: so3_cdf_rows and so3_score_rows must have the same number of rows')
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        Ts = max(T, 0)
        out = Perturbation(new(G, 3), new(G, 3), new(Ts), *([new(G, 3), new(G, 3), new(Ts)] if scores else [None] * 3))
        c_out = _lib.ddk_perturbation(**{k: (v.data_ptr() if v is not None and v.numel() else None) for k, v in out._asdict().items()})
        self._check(self.L.ddk_rng_perturbation_batch(self.h, s, G, _ptr(st), _ptr(i32[0]), _ptr(i32[1]), T, draw, _ptr(f32[0]), _ptr(f32[1]), _ptr(i32[2]),
                                                      _ptr(i32[3]), n_rows, _ptr(rows[0]), _ptr(rows[1]), C.byref(c_out), _stream()),
                    'ddk_rng_perturbation_batch')
        return out

    def modify_conformer_batch(self, pos, node_ptr, rot_bonds, mask_rotate, mask_ptr, tor_ptr, tr_update, rot_update, tor_update, T=None, return_status=False):
        """modify_conformer for a ragged batch (ddk_modify_conformer_batch): ``pos`` [N, 3] with graph g's atoms at node_ptr[g] .. node_ptr[g + 1],
        ``rot_bonds`` [T, 2] graph-local (u, v), ``mask_rotate`` the graphs' [R_g, n_g] byte blocks back to back with graph g's at mask_ptr[g], the updates
        [G, 3], [G, 3] and flat [T] (None: rigid moves only).  Returns pos_out [N, 3]; with ``return_status`` also the int32 status [G]
        (CONFORMER_BATCH_STATUS; a graph with a status other than 0 is not written).  Host arrays are uploaded; nothing is read back."""
        dev = torch.device('cuda', self.device)
        pos = self._dev(pos, torch.float32).reshape(-1, 3)
        self._check_ptr('node_ptr', node_ptr, pos.shape[0], 'the nodes must be grouped by graph')
        node_ptr = self._dev(node_ptr, torch.int32)
        G, N = node_ptr.numel() - 1, pos.shape[0]
        tr_update, rot_update = self._dev(tr_update, torch.float32), self._dev(rot_update, torch.float32)
        for name, t in (('tr_update', tr_update), ('rot_update', rot_update)):
            if t.numel() != 3 * G:
                raise ValueError(f'ddk: {name} must be [{G}, 3] for {G} graphs, got {tuple(t.shape)} (the library reads it through a raw pointer)')
        rb = mr = mp = tp = tor = None
        mask_bytes = 0
        if tor_update is not None:
            tor = self._dev(tor_update, torch.float32).reshape(-1)
            T = tor.numel() if T is None else int(T)
            rb = self._dev(rot_bonds, torch.int32).reshape(-1, 2)
            mr = self._dev(mask_rotate, torch.uint8).reshape(-1)
            self._check_ptr('tor_ptr', tor_ptr, T, 'the rotor counts of the graphs')
            self._check_ptr('mask_ptr', mask_ptr, None, 'the mask blocks of the graphs')
            mp, tp = self._dev(mask_ptr, torch.int32), self._dev(tor_ptr, torch.int32)
            mask_bytes = mr.numel()
            for name, t, n in (('tor_update', tor, T), ('rot_bonds', rb, 2 * T), ('mask_ptr', mp, G + 1), ('tor_ptr', tp, G + 1)):
                if t.numel() != n:
                    raise ValueError(f'ddk: {name} must hold {n} entries (G = {G}, T = {T}), got {t.numel()} (the library reads it through a raw pointer)')
        out = torch.empty_like(pos)
        status = torch.empty(max(G, 1), dtype=torch.int32, device=dev)
        self._rng_args(0, 0, dict(G=G, N=N, T=T or 0, mask_bytes=mask_bytes))
        self._check(self.L.ddk_modify_conformer_batch(self.h, G, N, _ptr(pos), _ptr(node_ptr), T or 0, _ptr(rb), _ptr(mr), _ptr(mp), mask_bytes, _ptr(tp),
                                                      _ptr(tr_update), _ptr(rot_update), _ptr(tor), _ptr(out), _ptr(status), _stream()),
                    'ddk_modify_conformer_batch')
        return (out, status) if return_status else out

    def randomize_position_batch(self, seed, pos, node_ptr, rot_bonds, mask_rotate, mask_ptr, tor_ptr, streams, samples, tr_sigma_max, T=None,
                                 no_torsion=False, return_status=False):
        """randomize_position for a ragged batch of different ligands (ddk_randomize_position_batch): the tables of :meth:`modify_conformer_batch`, and per
        graph the stream id (uint64 bit patterns, int64 [G]) and the global sample index (int32 [G]); graph g's pose is bit for bit what
        :meth:`rng_initial` + ``Complex.randomize_position`` give that ligand alone at (seed, stream, sample).  ``no_torsion``: no torsions are drawn and
        the rotor tables are not read.  Returns pos_out [N, 3]; with ``return_status`` also the int32 status [G] (CONFORMER_BATCH_STATUS; a graph with a
        status other than 0 is not written).  Host arrays are uploaded; nothing is read back."""
        dev = torch.device('cuda', self.device)
        pos = self._dev(pos, torch.float32).reshape(-1, 3)
        self._check_ptr('node_ptr', node_ptr, pos.shape[0], 'the nodes must be grouped by graph')
        node_ptr = self._dev(node_ptr, torch.int32)
        G, N = node_ptr.numel() - 1, pos.shape[0]
        st = streams if torch.is_tensor(streams) else np.asarray([_u64(v, 'rng_stream') for v in streams], dtype=np.uint64).view(np.int64)
        st, samples = self._dev(st, torch.int64), self._dev(samples, torch.int32)
        for name, t in (('streams', st), ('samples', samples)):
            if t.numel() != G:
                raise ValueError(f'ddk: {name} must hold {G} entries for {G} graphs, got {t.numel()} (the library reads it through a raw pointer)')
        rb = mr = mp = tp = None
        mask_bytes = 0
        if no_torsion:
            T = 0
        else:
            rb = self._dev(rot_bonds, torch.int32).reshape(-1, 2)
            T = rb.shape[0] if T is None else int(T)
            mr = self._dev(mask_rotate, torch.uint8).reshape(-1)
            self._check_ptr('tor_ptr', tor_ptr, T, 'the rotor counts of the graphs')
            self._check_ptr('mask_ptr', mask_ptr, None, 'the mask blocks of the graphs')
            mp, tp = self._dev(mask_ptr, torch.int32), self._dev(tor_ptr, torch.int32)
            mask_bytes = mr.numel()
            for name, t, n in (('rot_bonds', rb, 2 * T), ('mask_ptr', mp, G + 1), ('tor_ptr', tp, G + 1)):
                if t.numel() != n:
                    raise ValueError(f'ddk: {name} must hold {n} entries (G = {G}, T = {T}), got {t.numel()} (the library reads it through a raw pointer)')
        out = torch.empty_like(pos)
        status = torch.empty(max(G, 1), dtype=torch.int32, device=dev)
        s, _, _ = self._rng_args(seed, 0, dict(G=G, N=N, T=T, mask_bytes=mask_bytes))
        self._check(self.L.ddk_randomize_position_batch(self.h, s, G, N, _ptr(pos), _ptr(node_ptr), T, _ptr(rb), _ptr(mr), _ptr(mp), mask_bytes, _ptr(tp),
                                                        _ptr(st), _ptr(samples), float(tr_sigma_max), _ptr(out), _ptr(status), _stream()),
                    'ddk_randomize_position_batch')
        return (out, status) if return_status else out

    def _loss_batch_args(self, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2, tor_ptr, T):
        f = lambda t, cols: _need_cuda(t).contiguous().float().reshape(-1, cols)
        tr_pred, rot_pred, tr_score, rot_score = (f(t, 3) for t in (tr_pred, rot_pred, tr_score, rot_score))
        G = tr_score.shape[0]
        T = int(T)
        if tor_pred is not None and tor_score is not None and T > 0:
            tor_pred, tor_score = f(tor_pred, 1).reshape(-1), f(tor_score, 1).reshape(-1)
        else:
            tor_pred = tor_score = None
        scal = [self._dev(a, torch.float32).reshape(-1) for a in (tr_sigma, so3_score_norm, torus_score_norm2)]
        self._check_ptr('tor_ptr', tor_ptr, T, 'the rotor counts of the graphs')
        tor_ptr = self._dev(tor_ptr, torch.int32).reshape(-1)
        for name, t, n in (('tr_pred', tr_pred, 3 * G), ('rot_pred', rot_pred, 3 * G), ('rot_score', rot_score, 3 * G), ('tor_pred', tor_pred, T),
                           ('tor_score', tor_score, T), ('tr_sigma', scal[0], G), ('so3_score_norm', scal[1], G), ('torus_score_norm2', scal[2], G),
                           ('tor_ptr', tor_ptr, G + 1)):
            if t is not None and t.numel() != n:
                raise ValueError(f'ddk: {name} must hold {n} values (G = {G}, T = {T}), got {t.numel()} (the library reads it through a raw pointer)')
        return G, T, tor_ptr, (tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score), scal

    def score_matching_loss_batch(self, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2, tor_ptr, T):
        """The six LOSS_COLUMNS per GRAPH of a ragged batch (ddk_score_matching_loss_batch): device tensor [G, 6].  Predictions and targets [G, 3], [G, 3]
        and flat [T]; the three scalars and ``tor_ptr`` [G + 1] per graph (device tensors, or host arrays that are uploaded); ``T`` = tor_ptr[G] as a host
        integer.  ``tor_pred`` None or T = 0: the torsion terms are 0."""
        G, T, tor_ptr, ops, scal = self._loss_batch_args(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2,
                                                         tor_ptr, T)
        out = torch.empty((G, 6), dtype=torch.float32, device=ops[3].device)
        self._check(self.L.ddk_score_matching_loss_batch(self.h, G, _ptr(tor_ptr), T, *[_ptr(t) for t in ops], *[_ptr(t) for t in scal], _ptr(out), _stream()),
                    'ddk_score_matching_loss_batch')
        return out

    def score_matching_loss_batch_backward(self, grad, tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2,
                                           tor_ptr, T, need=(True, True, True)):
        """The gradients of (tr_pred, rot_pred, tor_pred) from ``grad`` [G, 3], the gradient of the three loss columns
        (ddk_score_matching_loss_batch_backward): a tuple of fresh device tensors [G, 3], [G, 3], [T], None where ``need`` is false (or there are no
        torsions)."""
        G, T, tor_ptr, ops, scal = self._loss_batch_args(tr_pred, rot_pred, tor_pred, tr_score, rot_score, tor_score, tr_sigma, so3_score_norm, torus_score_norm2,
                                                         tor_ptr, T)
        grad = _need_cuda(grad).contiguous().float()
        if grad.numel() != 3 * G:
            raise ValueError(f'ddk: grad must be [{G}, 3], got {tuple(grad.shape)} (the library reads it through a raw pointer)')
        dev = grad.device
        g_tr = torch.empty((G, 3), dtype=torch.float32, device=dev) if need[0] else None
        g_rot = torch.empty((G, 3), dtype=torch.float32, device=dev) if need[1] else None
        g_tor = torch.empty(T, dtype=torch.float32, device=dev) if need[2] and ops[2] is not None else None
        self._check(self.L.ddk_score_matching_loss_batch_backward(self.h, G, _ptr(tor_ptr), T, _ptr(grad), *[_ptr(t) for t in ops], *[_ptr(t) for t in scal],
                                                                  _ptr(g_tr), _ptr(g_rot), _ptr(g_tor), _stream()),
                    'ddk_score_matching_loss_batch_backward')
        return g_tr, g_rot, g_tor

    # ---- coordinates + bonds -> the static graph tables of a complex (csrc/k_build.hip) -------------
    def _count(self, count, what):
        """the ONE read-back of a builder: count_out [2] -> (count, status) on the host (8 bytes)"""
        n, status = (int(v) for v in count.tolist())
        if status == 2:
            raise ValueError(f'ddk: {what}: ' + ('a coordinate is not finite' if what != 'transformation_mask' else MASK_STATUS[2]))
        return n, status

    def _points(self, pos, what):
        dev = torch.device('cuda', self.device)
        pos = h2d_async(torch.as_tensor(pos).to(torch.float32).contiguous(), dev)
        if pos.dim() != 2 or pos.shape[1] != 3:
            raise RuntimeError(f'ddk: {what} takes coordinates [n, 3]; got ' + str(tuple(pos.shape)))
        return dev, pos

    def receptor_knn_graph(self, pos, cutoff=15.0, max_neighbor=24):
        """rec_edge_index of the residues pos [n, 3] by the rule of get_calpha_graph (process_mols.py:337-353; ddk_receptor_knn_graph, include/ddk.h):
        every other residue under ``cutoff`` in ascending index, the ``max_neighbor`` nearest by (distance, index) if there are more, the single nearest
        if there is none.  -> device tensor [2, E] int32, columns [i; j] grouped by i: what ddk_complex_create takes.  One 8-byte read-back (E).  A
        coordinate that is not finite is a ValueError.  2 <= n <= 65536, max_neighbor <= 128."""
        dev, pos = self._points(pos, 'receptor_knn_graph')
        n, K = pos.shape[0], int(max_neighbor)
        nbytes = self.L.ddk_receptor_knn_graph_workspace(n, K)
        cap = n * K if nbytes >= 0 else 1      # a broken limit: the call below says which
        out = torch.empty((2, cap), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self._check(self.L.ddk_receptor_knn_graph(self.h, n, _ptr(pos), float(cutoff), K, _ptr(out), cap, _ptr(count), _ptr(ws), _stream()),
                    'ddk_receptor_knn_graph')
        E, _ = self._count(count, 'receptor_knn_graph')
        return out[:, :E]

    def radius_graph(self, pos, r=5.0, max_num_neighbors=8):
        """torch_cluster.radius_graph(pos, r, max_num_neighbors=...) of one graph (atom_edge_index, process_mols.py:471; ddk_radius_graph, include/ddk.h)
        -> device tensor [2, E] int32, columns [neighbour; centre] grouped by centre, neighbours ascending.  One 8-byte read-back (E).  A coordinate that
        is not finite is a ValueError.  n <= 65536, max_num_neighbors <= 1024."""
        dev, pos = self._points(pos, 'radius_graph')
        n, K = pos.shape[0], int(max_num_neighbors)
        nbytes = self.L.ddk_radius_graph_workspace(n, K)
        cap = n * (K + 1) if nbytes >= 0 else 1      # the worst case: the status cannot be 1
        out = torch.empty((2, cap), dtype=torch.int32, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self._check(self.L.ddk_radius_graph(self.h, n, _ptr(pos), float(r), K, _ptr(out), cap, _ptr(count), _ptr(ws), _stream()), 'ddk_radius_graph')
        E, status = self._count(count, 'radius_graph')
        if status != 0:
            raise RuntimeError(f'ddk: radius_graph: status {status} with {E} edges for {cap} columns')
        return out[:, :E]

    def transformation_mask(self, n_lig, bond_index):
        """(edge_mask [M], mask_rotate [R, n_lig]), uint8 device tensors, by the rule of get_transformation_mask (utils/torsion.py:15-45;
        ddk_ligand_transformation_mask, include/ddk.h) from bond_index [2, M], columns 2k / 2k + 1 the two directions of bond k.  One 8-byte read-back
        (R).  A bond column that is out of range, unpaired, a self bond or repeated is a ValueError; a ligand graph that is not connected gives a warning
        and no torsion (edge_mask all 0, R = 0).  n_lig <= 256, M <= 2048."""
        dev = torch.device('cuda', self.device)
        n_lig = int(n_lig)
        bi = torch.as_tensor(bond_index)
        if bi.numel() and (bi.dim() != 2 or bi.shape[0] != 2):
            raise RuntimeError('ddk: bond_index must be [2, M]; got ' + str(tuple(bi.shape)))
        M = bi.numel() // 2
        bi = h2d_async(bi.to(torch.int32).contiguous(), dev) if M else None
        nbytes = self.L.ddk_ligand_transformation_mask_workspace(n_lig, M)
        ok = nbytes >= 0
        cap = max(M // 2, 1)      # a row per bond: the status cannot be 1
        edge_mask = torch.empty(M if ok else 0, dtype=torch.uint8, device=dev)
        mask_rotate = torch.empty((cap, n_lig) if ok else (1, 1), dtype=torch.uint8, device=dev)
        count = torch.empty(2, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        self._check(self.L.ddk_ligand_transformation_mask(self.h, n_lig, _ptr(bi), M, _ptr(edge_mask) if M else None, _ptr(mask_rotate), cap, _ptr(count),
                                                          _ptr(ws), _stream()), 'ddk_ligand_transformation_mask')
        R, status = self._count(count, 'transformation_mask')
        if status != 0:
            warnings.warn(f'ddk: transformation_mask: status {status} ({MASK_STATUS[status]}); the ligand gets no torsion')
            R = 0
        return edge_mask, mask_rotate[:R]


class Complex:
    """Device-resident static data of one complex (ddk_complex): topology, receptor embedding without its
    sigma part, receptor-receptor geometry, and the per-forward workspaces for up to max_batch samples."""

    def __init__(self, ctx, c, max_batch):
        """c: dict with the arrays of SURVEY.md Appendix B.1 (numpy or torch): lig_x [n,16], bond_index [2,M],
        bond_attr [M,4], edge_mask [M], mask_rotate [R,n], rec_x [n_rec,1+lm], rec_pos [n_rec,3], rec_edge_index [2,E]."""
        self.ctx = ctx
        f = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt)
        self.arr = dict(lig_x=f(c['lig_x'], np.int32), bond_index=f(c['bond_index'], np.int32), bond_attr=f(c['bond_attr'], np.float32),
                        edge_mask=f(c['edge_mask'], np.uint8), mask_rotate=f(c['mask_rotate'], np.uint8).reshape(-1, len(c['lig_x'])),
                        rec_x=f(c['rec_x'], np.float32), rec_pos=f(c['rec_pos'], np.float32),
                        rec_edge_index=f(c['rec_edge_index'], np.int32))
        a = self.arr
        self.n_lig, self.n_rec = a['lig_x'].shape[0], a['rec_pos'].shape[0]
        self.M, self.R, self.E_rr = a['bond_index'].shape[1], a['mask_rotate'].shape[0], a['rec_edge_index'].shape[1]
        self.max_batch = max_batch
        self.name = c.get('name') if hasattr(c, 'get') else None
        self._autos = {}
        d = _lib.ddk_complex_desc(n_lig=self.n_lig, n_rec=self.n_rec, n_bond_edges=self.M, n_rot=self.R, n_rec_edges=self.E_rr,
                                  rec_feat_dim=a['rec_x'].shape[1],
                                  **{k: v.ctypes.data_as(C.c_void_p) for k, v in a.items()})
        self.h = C.c_void_p()
        rc = ctx.L.ddk_complex_create(ctx.h, C.byref(d), max_batch, C.byref(self.h))
        if rc != 0:
            msg = ctx.L.ddk_last_error(ctx.h).decode()
            if self.h:
                ctx.L.ddk_complex_destroy(ctx.h, self.h)
                self.h = None
            raise RuntimeError(f'ddk_complex_create: {msg}')

    def close(self):
        if getattr(self, 'h', None) and getattr(self.ctx, 'h', None):
            self.ctx.L.ddk_complex_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_read_patch(self, B):
        """test hook: (exclusive prefix of the layer-0 patch edges per sample [B + 1], receiver mask [B, n_rec]) of the last forward"""
        cnt, mask = np.zeros(B + 1, np.int32), np.zeros((B, self.n_rec), np.uint8)
        self.ctx._check(self.ctx.L.ddk_debug_read_patch(self.ctx.h, self.h, B, cnt.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)),
                        'ddk_debug_read_patch')
        return cnt, mask

    def set_latents(self, lig_latent=None, rec_latent=None, unconditional=0.0):
        """data['ligand'|'receptor'].latent_h of the batch ([B*n, latent_dim], device) for the following forwards."""
        if lig_latent is not None:
            lig_latent, rec_latent = lig_latent.contiguous().float(), rec_latent.contiguous().float()
            ld = int(self.ctx.cfg.latent_dim)
            nb = lig_latent.shape[0] // max(self.n_lig, 1)
            if (lig_latent.dim() != 2 or rec_latent.dim() != 2 or lig_latent.shape[1] != ld or rec_latent.shape[1] != ld or nb < 1
                    or lig_latent.shape[0] != nb * self.n_lig or rec_latent.shape[0] != nb * self.n_rec):
                raise RuntimeError(f'ddk: latent arrays must be [B*{self.n_lig}, {ld}] and [B*{self.n_rec}, {ld}] for one batch size B, got '
                                   f'{tuple(lig_latent.shape)} and {tuple(rec_latent.shape)} (the library reads them through raw pointers)')
        self._latents = (lig_latent, rec_latent)      # keep the device arrays alive
        self.ctx._check(self.ctx.L.ddk_set_latents(self.ctx.h, self.h, _ptr(lig_latent), _ptr(rec_latent), float(unconditional)),
                        'ddk_set_latents')

    def set_guidance(self, weight=0.0, cfg_start=1.0, cfg_end=0.0):
        self.ctx._check(self.ctx.L.ddk_set_guidance(self.ctx.h, self.h, float(weight), float(cfg_start), float(cfg_end)), 'ddk_set_guidance')

    # ---- model.score_model(batch) ------------------------------------------------------------------
    def score_forward(self, pos, t_tr, t_rot, t_tor):
        ctx = self.ctx
        pos = _need_cuda(pos).contiguous().float().reshape(-1, self.n_lig, 3)
        B = pos.shape[0]
        dev = pos.device
        tr = torch.empty((B, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((B, 3), dtype=torch.float32, device=dev)
        tor = torch.empty((B * self.R,), dtype=torch.float32, device=dev)
        ctx._check(ctx.L.ddk_score_forward(ctx.h, self.h, B, _ptr(pos), float(t_tr), float(t_rot), float(t_tor),
                                           _ptr(tr), _ptr(rot), _ptr(tor), _stream()), 'ddk_score_forward')
        return tr, rot, tor

    def se3_update(self, pos, tr, rot, tor):
        ctx = self.ctx
        pos = pos.contiguous().float().reshape(-1, self.n_lig, 3)
        B = pos.shape[0]
        out = torch.empty_like(pos)
        tr, rot = tr.contiguous().float(), rot.contiguous().float()
        tor = tor.contiguous().float() if tor is not None else None
        ctx._check(ctx.L.ddk_se3_update(ctx.h, self.h, B, _ptr(pos), _ptr(tr), _ptr(rot), _ptr(tor), _ptr(out), _stream()),
                   'ddk_se3_update')
        return out

    # ---- AR latent model (ddk_ar_logits / ddk_ar_decode) --------------------------------------------------------------------
    def ar_logits(self, B):
        """predictor logits [B, n_lig + n_rec] on the node features of the last forward (keep_receptor_features(True) before it)"""
        dev = torch.device('cuda', self.ctx.device)
        out = torch.empty((B, self.n_lig + self.n_rec), dtype=torch.float32, device=dev)
        self.ctx._check(self.ctx.L.ddk_ar_logits(self.ctx.h, self.h, B, _ptr(out), _stream()), 'ddk_ar_logits')
        return out

    def ar_decode(self, logits, temperature, uniforms, idx, latent_l, latent_r, choices=None):
        """in place: one-hot of the picked node of every graph into column idx of latent_l / latent_r ([B*n, D], contiguous fp32)"""
        B, D = logits.shape[0], latent_l.shape[1]
        assert logits.is_contiguous() and latent_l.is_contiguous() and latent_r.is_contiguous() and latent_l.dtype == torch.float32
        assert choices is None or (choices.dtype == torch.int32 and choices.is_contiguous() and tuple(choices.shape) == (B, D))
        self.ctx._check(self.ctx.L.ddk_ar_decode(self.ctx.h, self.h, B, _ptr(logits), float(temperature), _ptr(uniforms), int(idx), D,
                                                 _ptr(latent_l), _ptr(latent_r), _ptr(choices), _stream()), 'ddk_ar_decode')

    def set_atoms(self, atom_x, atom_pos, atom_edge_index, atom_rec_index, lig_x=None, rec_x=None):
        """Receptor-atom level of the confidence model's graph (data['atom'] of datasets_utils/process_mols.py:474-477)."""
        f = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=dt)
        at = dict(atom_x=f(atom_x, np.int32), atom_pos=f(atom_pos, np.float32), atom_edge_index=f(atom_edge_index, np.int32),
                  atom_rec_index=f(atom_rec_index, np.int32))
        self.n_atom = at['atom_x'].shape[0]
        d = _lib.ddk_atoms_desc(n_atom=self.n_atom, n_atom_edges=at['atom_edge_index'].shape[1],
                                **{k: v.ctypes.data_as(C.c_void_p) for k, v in at.items()})
        lig_x = self.arr['lig_x'] if lig_x is None else f(lig_x, np.int32)
        rec_x = self.arr['rec_x'] if rec_x is None else f(rec_x, np.float32)
        self.ctx._check(self.ctx.L.ddk_complex_set_atoms(self.ctx.h, self.h, C.byref(d), lig_x.ctypes.data_as(C.c_void_p),
                                                         rec_x.ctypes.data_as(C.c_void_p), rec_x.shape[1]), 'ddk_complex_set_atoms')

    def confidence_forward(self, pos, check=True):
        """confidence_model(batch) for B poses of this complex -> [B, num_confidence_outputs] (device).  check=False skips the host
        read-back of the edge-capacity flag (the caller runs ``confidence_counts()`` at its own synchronisation point)."""
        pos = pos.contiguous().float().reshape(-1, self.n_lig, 3)
        B = pos.shape[0]
        out = torch.empty((B, int(self.ctx.cfg.num_confidence_outputs)), dtype=torch.float32, device=pos.device)
        self.ctx._check(self.ctx.L.ddk_confidence_forward(self.ctx.h, self.h, B, _ptr(pos), _ptr(out), _stream()), 'ddk_confidence_forward')
        if check:
            self.confidence_counts()      # one host sync per confidence batch: fails loudly if the ligand-atom edge capacity overflowed
        return out

    def score_confidence(self, pos, t_tr, t_rot, t_tor):
        """coarse-grained confidence model (ddk_config.confidence_mode) on B poses of this complex at the given complex_t -> [B, num_confidence_outputs]
        (device); utils/sampling.py:239-240."""
        pos = pos.contiguous().float().reshape(-1, self.n_lig, 3)
        B = pos.shape[0]
        out = torch.empty((B, int(self.ctx.cfg.num_confidence_outputs)), dtype=torch.float32, device=pos.device)
        self.ctx._check(self.ctx.L.ddk_score_confidence(self.ctx.h, self.h, B, _ptr(pos), float(t_tr), float(t_rot), float(t_tor), _ptr(out), _stream()),
                        'ddk_score_confidence')
        return out

    def confidence_status_async(self):
        """-> pinned int32[CONF_STATUS_INTS] that holds the group table / overflow flag of the last confidence forward once the current stream has
        passed this point (ddk_confidence_status); no synchronisation here"""
        out = torch.empty(CONF_STATUS_INTS, dtype=torch.int32, pin_memory=True)
        self.ctx._check(self.ctx.L.ddk_confidence_status(self.ctx.h, self.h, C.c_void_p(out.data_ptr()), _stream()), 'ddk_confidence_status')
        return out

    def confidence_counts(self):
        n = len(CONF_GROUPS)
        out = (C.c_int32 * (n + 1))()      # the groups' edge counts, then the overflow flag
        self.ctx._check(self.ctx.L.ddk_debug_conf_counts(self.ctx.h, self.h, out), 'ddk_debug_conf_counts')
        v = list(out)
        if v[n]:
            raise RuntimeError('ddk: ligand-atom edge capacity overflow')
        return dict(zip(CONF_GROUPS, v[:n]))

    def confidence_table(self, which):
        """test hook: edges per group of the table layer `which` ran on (0 full, 1 layer 0, 2 level A, 3 level B, 4 layer 1; include/ddk_debug.h)."""
        out = (C.c_int32 * len(CONF_GROUPS))()
        self.ctx._check(self.ctx.L.ddk_debug_conf_table(self.ctx.h, self.h, which, out), 'ddk_debug_conf_table')
        return dict(zip(CONF_GROUPS, list(out)))

    def confidence_nodes(self):
        n = self.max_batch * self.n_lig + (self.max_batch + 1) * (self.n_atom + self.n_rec)      # (+ the virtual ligand-free sample)
        x, deg = np.zeros((n, 84), np.float32), np.zeros((n, 3), np.int32)
        self.ctx._check(self.ctx.L.ddk_debug_conf_nodes(self.ctx.h, self.h, x.ctypes.data_as(C.c_void_p), deg.ctypes.data_as(C.c_void_p), n), 'ddk_debug_conf_nodes')
        return x, deg

    def confidence_edges(self):
        """test hook: {group: (src, dst, emb, sh)} of the last confidence forward (node ids in the device numbering)."""
        gt = (C.c_int32 * (2 * len(CONF_GROUPS)))()      # first edge of every group, then the end edges
        self.ctx._check(self.ctx.L.ddk_debug_conf_edges(self.ctx.h, self.h, 0, 0, None, None, None, None, gt), 'ddk_debug_conf_edges')
        out = {}
        for k, name in enumerate(CONF_GROUPS):
            n = gt[len(CONF_GROUPS) + k] - gt[k]
            src, dst = np.zeros(n, np.int32), np.zeros(n, np.int32)
            emb, sh = np.zeros((n, 24), np.float32), np.zeros((n, 4), np.float32)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            self.ctx._check(self.ctx.L.ddk_debug_conf_edges(self.ctx.h, self.h, gt[k], n, p(src), p(dst), p(emb), p(sh), None), 'ddk_debug_conf_edges')
            out[name] = (src, dst, emb, sh)
        return out

    def lig_node_features(self, B, device):
        lig = torch.empty((B * self.n_lig, 84), dtype=torch.float32, device=device)
        self.ctx._check(self.ctx.L.ddk_last_node_features(self.ctx.h, self.h, B, _ptr(lig), None, _stream()), 'ddk_last_node_features')
        return lig

    def automorphisms(self, atom_mask=None, cap=65536):
        """This ligand's automorphism table from its own data (Context.ligand_automorphisms): colour = lig_x[:, 0], the bonds = bond_index,
        ``atom_mask`` [n_lig] the kept atoms, by default the heavy atoms lig_x[:, 0] != 0 (filterHs, evaluate.py:297).  Returns (perms [cap, n_lig],
        count [2]) on the device, cached per (mask, cap); nothing is read back.  lig_x[:, 0] is the reference's atomic-number INDEX, whose last bucket
        is 'misc': two different exotic elements in that bucket compare equal here, where spyrmsd compares true atomic numbers."""
        colour = self.arr['lig_x'][:, 0]
        mask = (colour != 0) if atom_mask is None else torch.as_tensor(atom_mask).reshape(-1).ne(0).cpu().numpy()
        key = (mask.tobytes(), int(cap))
        if key not in self._autos:
            self._autos[key] = self.ctx.ligand_automorphisms(colour, self.arr['bond_index'], atom_mask=mask, cap=cap)
        return self._autos[key]

    def pose_metrics(self, pos, ref_pos, atom_mask=None, perms=None, rec_atom_pos=None, auto_cap=65536):
        """evaluate.py:297-338 for B poses: tensor [B,4] = rmsd, centroid distance, min cross distance, min self distance.
        perms [K, n_lig] (int): graph automorphisms of the ligand -> symmetry-corrected RMSD (evaluate.py:308-310); None: uncorrected
        (:313); 'auto': self.automorphisms(cap=auto_cap) over the atoms this call counts (atom_mask; all atoms if it is None), at the price of one
        read-back of its row count (usable_automorphisms; the identity alone and a warning if the table did not fit).
        rec_atom_pos [n, 3]: receptor atom coordinates for the cross distance (default: the C-alpha coordinates)."""
        if isinstance(perms, str):
            if perms != 'auto':
                raise RuntimeError(f"ddk: perms is a table, None or 'auto'; got {perms!r}")
            perms = usable_automorphisms(*self.automorphisms(np.ones(self.n_lig, bool) if atom_mask is None else atom_mask, cap=auto_cap), name=self.name)
        pos = pos.contiguous().float().reshape(-1, self.n_lig, 3)
        ref = ref_pos.contiguous().float().reshape(self.n_lig, 3).to(pos.device)
        m = None if atom_mask is None else atom_mask.to(pos.device).to(torch.uint8).contiguous()
        pm = None if perms is None else torch.as_tensor(perms).to(pos.device).to(torch.int32).reshape(-1, self.n_lig).contiguous()
        if pm is not None and (int(pm.min()) < 0 or int(pm.max()) >= self.n_lig):
            raise RuntimeError('ddk: permutation table entries must be ligand atom indices')
        ra = None if rec_atom_pos is None else torch.as_tensor(rec_atom_pos).to(pos.device).float().reshape(-1, 3).contiguous()
        out = torch.empty((pos.shape[0], 4), dtype=torch.float32, device=pos.device)
        self.ctx._check(self.ctx.L.ddk_pose_metrics(self.ctx.h, self.h, pos.shape[0], _ptr(pos), _ptr(ref), _ptr(m), _ptr(pm),
                                                    0 if pm is None else pm.shape[0], _ptr(ra), 0 if ra is None else ra.shape[0], _ptr(out),
                                                    _stream()), 'ddk_pose_metrics')
        return out

    def randomize_position(self, pos0, rot, tor=None, tr=None):
        """utils/sampling.py:12-34 for B = rot.shape[0] copies of the conformer pos0 [n_lig,3]; returns [B,n_lig,3]."""
        ctx = self.ctx
        pos0 = pos0.contiguous().float().reshape(self.n_lig, 3)
        rot = rot.contiguous().float().reshape(-1, 3, 3)
        B = rot.shape[0]
        tor = tor.contiguous().float().reshape(B, self.R) if tor is not None and self.R > 0 else None
        tr = tr.contiguous().float().reshape(B, 3) if tr is not None else None
        out = torch.empty((B, self.n_lig, 3), dtype=torch.float32, device=pos0.device)
        ctx._check(ctx.L.ddk_randomize_position(ctx.h, self.h, B, _ptr(pos0), _ptr(tor), _ptr(rot), _ptr(tr), _ptr(out), _stream()),
                   'ddk_randomize_position')
        return out

    def sample(self, pos, t, score_coeff, noise_coeff, noise=None, record=None):
        """in-place reverse diffusion of pos [B,n_lig,3]; t/score_coeff/noise_coeff: [steps,3] host arrays.
        record: None / False (default) returns pos; True records the whole trajectory on the device (ddk_sample_trajectory: same launches, no
        synchronisation) and returns a :data:`Trajectory` of freshly allocated device tensors; a tuple of names out of TRAJECTORY_FIELDS, e.g.
        ``('pos', 'edge_counts')``, records that subset (the other members of the result are None)."""
        ctx = self.ctx
        assert pos.is_contiguous() and pos.dtype == torch.float32
        B = pos.numel() // (self.n_lig * 3)
        t = np.ascontiguousarray(t, dtype=np.float32)
        sc = np.ascontiguousarray(score_coeff, dtype=np.float32)
        nc = np.ascontiguousarray(noise_coeff, dtype=np.float32)
        steps = t.shape[0]
        self.keep_receptor_features(False)   # the sampler reads ligand rows only
        if noise is not None:
            noise = noise.contiguous().float()
            assert tuple(noise.shape) == (steps, B, 6 + self.R)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        if record is None or record is False:
            ctx._check(ctx.L.ddk_sample(ctx.h, self.h, B, steps, p(t), p(sc), p(nc), _ptr(noise), _ptr(pos), _stream()), 'ddk_sample')
            return pos
        names = TRAJECTORY_FIELDS if record is True else tuple(record)
        if isinstance(record, str) or not names or any(k not in TRAJECTORY_FIELDS for k in names):
            raise ValueError(f'record: True or a tuple of names out of {TRAJECTORY_FIELDS}, got {record!r}')
        n = max(steps, 0)      # (steps < 1 is refused by the library, with its message)
        shapes = dict(pos=(n + 1, B, self.n_lig, 3), scores=(n, B, 6 + self.R), perturb=(n, B, 6 + self.R), edge_counts=(n, 4))
        rec = Trajectory(*[torch.empty(shapes[k], dtype=torch.int32 if k == 'edge_counts' else torch.float32, device=pos.device) if k in names else None
                           for k in TRAJECTORY_FIELDS])
        c_rec = _lib.ddk_trajectory(**{k: (v.data_ptr() if v is not None else None) for k, v in rec._asdict().items()})
        ctx._check(ctx.L.ddk_sample_trajectory(ctx.h, self.h, B, steps, p(t), p(sc), p(nc), _ptr(noise), _ptr(pos), C.byref(c_rec), _stream()),
                   'ddk_sample_trajectory')
        return rec

    def build_graph(self, pos, t_tr):
        """score_model.py:310-408 + :218-225 alone: ``(edge_index [2, E] int32, group_offsets [5])`` of the merged graph of the B poses
        ``pos`` [B, n_lig, 3] at diffusion time t_tr; groups [lig-lig | lig->rec | rec-rec | rec->lig], each sorted by row 0 (the
        receiving node, tensor_layers.py:159); nodes numbered [all ligand atoms | all residues]."""
        pos = _need_cuda(pos).contiguous().float().reshape(-1, self.n_lig, 3)
        B = pos.shape[0]
        cap = B * (self.M + self.n_lig * 33 + 2 * self.n_lig * self.n_rec + self.E_rr)      # 33: radius(..., 32 + 1) minus a self loop that may not be among them
        src = torch.empty(cap, dtype=torch.int32, device=pos.device)
        dst = torch.empty(cap, dtype=torch.int32, device=pos.device)
        off = torch.empty(5, dtype=torch.int32, device=pos.device)
        self.ctx._check(self.ctx.L.ddk_build_graph(self.ctx.h, self.h, B, _ptr(pos), float(t_tr), _ptr(src), _ptr(dst), cap, _ptr(off),
                                                   _stream()), 'ddk_build_graph')
        off = off.cpu()
        E = int(off[4])
        return torch.stack([src[:E], dst[:E]]), off

    def graph_stats(self):
        out = (C.c_int64 * 12)()
        self.ctx._check(self.ctx.L.ddk_last_graph_stats(self.ctx.h, self.h, out, _stream()), 'ddk_last_graph_stats')
        v = list(out)
        if v[6]:
            raise RuntimeError('ddk: edge capacity overflow')
        if v[11]:
            raise RuntimeError('ddk: the graph count and fill kernels disagreed about an edge count (internal consistency guard)')
        return dict(E_ll=v[0], E_lr=v[1], E_rr=v[2], E_rl=v[3], E_shared=v[4], E=v[5], cap=v[7], E_rr_live=(v[8], v[9], v[10]))

    def keep_receptor_features(self, on=True):
        """Evaluate the receptor rows of the last conv layer too (needed before ``node_features``' receptor output)."""
        self.ctx._check(self.ctx.L.ddk_set_keep_receptor_features(self.ctx.h, self.h, int(bool(on))), 'ddk_set_keep_receptor_features')

    def node_features(self, B, device):
        lig = torch.empty((B * self.n_lig, 84), dtype=torch.float32, device=device)
        rec = torch.empty((B * self.n_rec, 84), dtype=torch.float32, device=device)
        self.ctx._check(self.ctx.L.ddk_last_node_features(self.ctx.h, self.h, B, _ptr(lig), _ptr(rec), _stream()), 'ddk_last_node_features')
        return lig, rec

    def debug_cross_mirror(self):
        """test hook: True when this complex' forwards write the rec->lig rows as mirror copies of the lig->rec rows (include/ddk_debug.h)"""
        rc = self.ctx.L.ddk_debug_cross_mirror(self.ctx.h, self.h)
        if rc < 0:
            raise RuntimeError('ddk_debug_cross_mirror failed')
        return bool(rc)

    def read_edges(self, B, tails=False):
        """test hook: (graph_stats, src, dst, emb [E, 24], sh [E, 4], deg [B * (n_lig + n_rec)]) of the four edge groups of the last score-model
        forward.  tails=True appends a dict of the two edge ranges behind them that layer 0 of a de-duplicated forward reads: 'shared' = (src, dst, emb,
        sh) of the one rec-rec copy in sample 0's numbering, 'patch' = the same for the latent-conditioned model's per-sample patch group, with 'patch_counts'
        [B + 1] (exclusive prefix per sample) and 'patch_mask' [B, n_rec]; None where the last forward built none."""
        st = self.graph_stats()
        E, N = st['E'], B * (self.n_lig + self.n_rec)
        p = lambda a: a.ctypes.data_as(C.c_void_p)

        def rows(first, n, deg=None):
            src, dst = np.zeros(n, np.int32), np.zeros(n, np.int32)
            emb, sh = np.zeros((n, 24), np.float32), np.zeros((n, 4), np.float32)
            self.ctx._check(self.ctx.L.ddk_debug_read_edges(self.ctx.h, self.h, first, n, p(src), p(dst), p(emb), p(sh), None if deg is None else p(deg),
                                                            0 if deg is None else len(deg)), 'ddk_debug_read_edges')
            return src, dst, emb, sh

        deg = np.zeros(N, np.int32)
        out = (st,) + rows(0, E, deg) + (deg,)
        if not tails:
            return out
        tail = dict(shared=rows(E, st['E_shared']) if st['E_shared'] else None, patch=None, patch_counts=None, patch_mask=None)
        if st['E_shared'] and int(self.ctx.cfg.latent_dim) > 0:
            cnt, mask = self.debug_read_patch(B)
            tail.update(patch=rows(st['cap'], int(cnt[B])), patch_counts=cnt, patch_mask=mask)
        return out + (tail,)
