"""Training the AR latent model: the reference's autoregressive/dataset_ar.py and autoregressive/train_ar.py for a
``pretrained_score_encoder.TrainablePretrainedScoreEncoder`` (``model_utils.get_ar_model(training=True)``).

    make_latent_labels   AutoregressiveDataset.preprocessing: the oracle encoder's latents (or, with ``no_sampling``, its logits) of every complex
    draw_decoding_idx    the decoding index of an item (dataset_ar.py:83), from the seeded generator (purpose 14, ddk_rng_decoding_index)
    ar_batch             AutoregressiveDataset.get for a list of complexes followed by collation: decoding index, random start pose
                         (ddk_randomize_position_batch), masked input latent, teacher tables
    ar_loss              the per-graph cross-entropy of train_ar.py:116-127 / 152-177 as one ragged op (ddk_node_cross_entropy_batch)
    train_ar_epoch / test_ar_epoch    train_ar.py:107-194

Every draw comes from the counter-based generator, so a batch is a pure function of (complexes, labels, seed, draw) and an epoch of (the model's state,
complexes, labels, seed, epoch).  Not covered: ``no_randomness`` (the rdkit start pose), ``compute_ar_accuracy``'s ``encode_ar`` sweep (the inference class
has ``encode_ar``), the out-of-memory skip, wandb / scheduler / checkpoint files, DDP."""
import numpy as np
import torch

from . import data as _data
from .runtime import NOISE_BATCH_MAX_LIG, NOISE_BATCH_MAX_ROT, h2d_async, stream_id
from .tensor_layers import _layer_seed, ragged_node_cross_entropy
from .training import _TORCH_OF, _ctx_of, _host_ctx, _pack, _step_seed, epoch_permutation

AR_INPUT_TEMPERATURE = 0.01      # dataset_ar.py:105: the temperature of the fresh draw that makes the input latent under no_sampling
AR_INPUT_SEED_INDEX = 25         # its sub-seed (the model's own Gumbel draw takes 24, pretrained_score_encoder.AR_GUMBEL_SEED_INDEX)


def _names(complexes, who):
    names = [c.get('name') if hasattr(c, 'get') else None for c in complexes]
    if any(n is None for n in names):
        raise ValueError(f'ddk: {who} needs complexes with a name (the stream id is runtime.stream_id(name))')
    return names


def draw_decoding_idx(names, D, seed, draw):
    """The decoding index in 0 .. D - 1 of each complex of ``names`` for draw ``draw`` under ``seed``: an int32 host array, a pure function of (name,
    seed, draw) in integer arithmetic (generator purpose 14, ddk_rng_decoding_index; computed on the host).  dataset_ar.py:83 draws it from an unseeded
    host generator."""
    if not 1 <= int(D) <= 4:
        raise ValueError(f'ddk: draw_decoding_idx: D must be in 1..4, got {D}')
    return _host_ctx().decoding_index(seed, [stream_id(n) for n in names], int(D), draw=draw)


def mask_input_latent(label, decoding_idx):
    """dataset_ar.py:117-119 for one complex: the label table [n, D] with the columns at or past ``decoding_idx`` zeroed (a copy)"""
    out = np.array(label, dtype=np.float32, copy=True)
    out[:, int(decoding_idx):] = 0
    return out


def _ligand_tables(complexes, no_torsion, who):
    """The ragged ligand tables of ``ddk_modify_conformer_batch`` / ``ddk_randomize_position_batch`` for a list of complexes, checked on the host as
    ``training.noise_batch`` checks them (what the device would report as a status raises here): (streams [G] int64 bit patterns, pos [N, 3], node_ptr,
    tor_ptr, mask_ptr [G + 1] int32, bonds [T, 2] int32, masks uint8)."""
    streams, pos, bonds, masks, rotors, atoms = [], [], [], [], [], []
    for g, (c, name) in enumerate(zip(complexes, _names(complexes, who))):
        p = np.asarray(c['lig_pos'], dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        if not 1 <= n <= NOISE_BATCH_MAX_LIG:
            raise ValueError(f'ddk: {who}: n_lig of complex {g} ({name!r}) must be in [1, {NOISE_BATCH_MAX_LIG}], got {n}')
        if not np.isfinite(p).all():
            raise ValueError(f'ddk: {who}: lig_pos of complex {g} ({name!r}) has a coordinate that is not finite')
        em = np.asarray(c['edge_mask']).astype(bool).reshape(-1)
        mr = np.asarray(c['mask_rotate']).astype(np.uint8).reshape(-1, n) if np.size(c['mask_rotate']) else np.zeros((0, n), np.uint8)
        uv = np.asarray(c['bond_index'], dtype=np.int64)[:, em].T.reshape(-1, 2)
        if mr.shape[0] != uv.shape[0]:
            raise ValueError(f'ddk: {who}: complex {g} ({name!r}) has {uv.shape[0]} rotatable bonds in edge_mask and {mr.shape[0]} rows in mask_rotate')
        if no_torsion:
            mr, uv = mr[:0], uv[:0]
        R = uv.shape[0]
        if R > NOISE_BATCH_MAX_ROT:
            raise ValueError(f'ddk: {who}: R_g of complex {g} ({name!r}) must be in [0, {NOISE_BATCH_MAX_ROT}], got {R}')
        if R and ((uv < 0).any() or (uv >= n).any() or (uv[:, 0] == uv[:, 1]).any()):
            raise ValueError(f'ddk: {who}: a rotatable bond of complex {g} ({name!r}) has an atom index outside [0, {n}) or joins an atom to itself')
        streams.append(stream_id(name)); pos.append(p); bonds.append(uv.astype(np.int32)); masks.append(mr.reshape(-1)); rotors.append(R); atoms.append(n)
    prefix = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (np.asarray(streams, np.uint64).view(np.int64), np.concatenate(pos), prefix(atoms), prefix(rotors), prefix([r * n for r, n in zip(rotors, atoms)]),
            np.concatenate(bonds).reshape(-1, 2), np.concatenate(masks))


def _samples(samples, G, who):
    samples = np.asarray(samples, dtype=np.int64).reshape(-1)
    if samples.size != G or (samples < 0).any() or (samples >= (1 << 31) - 1).any():
        raise ValueError(f'ddk: {who}: samples must hold one index in [0, 2^31 - 1) per complex ({G}), got {samples.tolist()}')
    return samples.astype(np.int32)


def _upload(host, dev):
    """host arrays -> their device views in ONE copy"""
    buf, where = _pack(host)
    dbuf = h2d_async(torch.from_numpy(buf), dev)
    return [dbuf[at:at + nbytes].view(_TORCH_OF[dt]).reshape(shape) for at, dt, shape, nbytes in where]


def randomize_position_batch(model, complexes, seed, samples, tr_sigma_max, no_torsion=False):
    """``randomize_position(..., unbatched=True)`` (utils/sampling.py:12-34) for G DIFFERENT complexes: pos [N, 3] on the device, graph g's rows the
    random start pose of global sample ``samples[g]`` of stream ``stream_id(name_g)`` under ``seed``: bit for bit ``sampling.randomize_position([g],
    seed=seed, sample_offset=samples[g])`` of that complex alone, whatever the batch.  One upload, one launch (ddk_randomize_position_batch), nothing read
    back: the tables are checked on the host first."""
    ctx = _ctx_of(model)
    if len(complexes) < 1:
        raise ValueError('ddk: randomize_position_batch needs at least one complex')
    tables = _ligand_tables(complexes, no_torsion, 'randomize_position_batch')
    dev = torch.device('cuda', ctx.device)
    d_streams, d_pos, d_node, d_tor, d_mask_ptr, d_bonds, d_masks, d_samples = _upload(list(tables) + [_samples(samples, len(complexes), 'randomize_position_batch')],
                                                                                      dev)
    return ctx.randomize_position_batch(seed, d_pos, d_node, d_bonds, d_masks, d_mask_ptr, d_tor, d_streams, d_samples, tr_sigma_max, T=int(tables[3][-1]),
                                        no_torsion=no_torsion)


def make_latent_labels(encoder, complexes, temperature=0.01, no_sampling=False, seed=0):
    """AutoregressiveDataset.preprocessing (dataset_ar.py:128-175): the oracle ``latent_encoder.TPEncoder`` in ``.eval()`` on the true pose of every
    complex, one complex at a time as there: name -> (latent_l [n_lig, D], latent_r [n_rec, D]) host tensors, per column a one-hot over the complex's
    nodes drawn at ``temperature``; with ``no_sampling`` the encoder's logit tables instead.  The Gumbel noise is a function of (seed, name), so the result
    is a pure function of (the encoder's state, the complex, seed).  The encoder's mode, temperature and ``apply_gumbel_softmax`` are put back."""
    dev = next(encoder.parameters()).device
    was = (encoder.training, encoder.latent_temperature, encoder.apply_gumbel_softmax)
    encoder.eval()
    encoder.latent_temperature, encoder.apply_gumbel_softmax = float(temperature), not no_sampling
    labels = {}
    try:
        with torch.no_grad():
            for c, name in zip(complexes, _names(complexes, 'make_latent_labels')):
                batch = _data.collate([_data.from_arrays(c)]).to(dev)
                batch['ligand'].orig_pos_torch = batch['ligand'].pos
                if no_sampling:
                    l, r = encoder.logits(batch, seed)[:2]
                else:
                    l, r = ((v > 0.5).float() for v in encoder(batch, seed=seed))      # (hard - y) + y is 1 or 0 to within an ulp: the exact one-hot
                labels[name] = (l.float().cpu(), r.float().cpu())
    finally:
        encoder.train(was[0])
        encoder.latent_temperature, encoder.apply_gumbel_softmax = was[1], was[2]
    return labels


def ar_batch(model, complexes, labels, seed, draw, no_sampling=False):
    """AutoregressiveDataset.get (dataset_ar.py:74-126) for a list of complexes, followed by collation: a ``data.collate`` batch on the model's device with

        data.decoding_idx                   int32 [G], ``draw_decoding_idx(names, D, seed, draw)``
        data['ligand'].pos                  the random start poses, sample = ``draw`` of each complex' stream (``randomize_position_batch``)
        data['ligand' | 'receptor'].input_latent    the label columns at or past the graph's decoding index zeroed; with ``no_sampling`` the one-hot of a
                                            fresh ``ddk_gumbel_softmax_batch`` draw at T = 0.01 over the label logits, masked the same way
        data.teacher_l / data.teacher_r     the label tables [N_lig, D], [N_rec, D] (one-hots, or logits with ``no_sampling``): what ``ar_loss`` reads
        data.lig_ptr / data.rec_ptr         int64 [G + 1], the graphs' rows

    ``labels``: name -> (latent_l, latent_r) of ``make_latent_labels``.  ONE upload of the per-graph tables; nothing is read back."""
    ctx = _ctx_of(model)
    G = len(complexes)
    if G < 1:
        raise ValueError('ddk: ar_batch needs at least one complex')
    names = _names(complexes, 'ar_batch')
    D = int(model.input_latent_dim)
    no_torsion = bool(model.no_torsion)
    idx = draw_decoding_idx(names, D, seed, draw)
    tables = _ligand_tables(complexes, no_torsion, 'ar_batch')
    lab_l, lab_r = [], []
    for c, name in zip(complexes, names):
        if name not in labels:
            raise ValueError(f'ddk: ar_batch: complex {name!r} has no latent label (make_latent_labels makes them)')
        l, r = (np.asarray(v, dtype=np.float32) for v in labels[name])
        n_l, n_r = np.asarray(c['lig_pos']).reshape(-1, 3).shape[0], np.asarray(c['rec_pos']).reshape(-1, 3).shape[0]
        if l.shape != (n_l, D) or r.shape != (n_r, D):
            raise ValueError(f'ddk: ar_batch: the label of {name!r} must be ([{n_l}, {D}], [{n_r}, {D}]), got ({list(l.shape)}, {list(r.shape)})')
        lab_l.append(l); lab_r.append(r)
    prefix64 = lambda parts: np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)
    # the input latent itself (sampled labels), or under no_sampling the 0 / 1 mask that the fresh draw is multiplied by
    in_l = [mask_input_latent(np.ones_like(l) if no_sampling else l, k) for l, k in zip(lab_l, idx)]
    in_r = [mask_input_latent(np.ones_like(r) if no_sampling else r, k) for r, k in zip(lab_r, idx)]
    host = list(tables) + [np.full(G, int(draw), np.int64), idx.astype(np.int32), prefix64(lab_l), prefix64(lab_r), np.concatenate(lab_l), np.concatenate(lab_r),
                           np.concatenate(in_l), np.concatenate(in_r)]
    host[7] = _samples(host[7], G, 'ar_batch')
    dev = torch.device('cuda', ctx.device)
    (d_streams, d_pos, d_node, d_tor, d_mask_ptr, d_bonds, d_masks, d_samples, d_idx, d_lig_ptr, d_rec_ptr, d_teacher_l, d_teacher_r, d_in_l,
     d_in_r) = _upload(host, dev)      # the one copy
    pos = ctx.randomize_position_batch(seed, d_pos, d_node, d_bonds, d_masks, d_mask_ptr, d_tor, d_streams, d_samples, float(model.tr_sigma_max),
                                       T=int(tables[3][-1]), no_torsion=no_torsion)
    if no_sampling:
        out_l, out_r = ctx.gumbel_softmax(d_teacher_l, d_teacher_r, d_lig_ptr, d_rec_ptr, AR_INPUT_TEMPERATURE, _layer_seed(seed, AR_INPUT_SEED_INDEX),
                                          d_streams, sample=int(draw), draw=0)[:2]
        d_in_l, d_in_r = (out_l > 0.5).float() * d_in_l, (out_r > 0.5).float() * d_in_r
    batch = _data.collate([_data.from_arrays(c) for c in complexes]).to(dev)
    batch['ligand'].pos = pos
    batch['ligand'].input_latent, batch['receptor'].input_latent = d_in_l, d_in_r
    batch.decoding_idx, batch.lig_ptr, batch.rec_ptr, batch.teacher_l, batch.teacher_r = d_idx, d_lig_ptr, d_rec_ptr, d_teacher_l, d_teacher_r
    return batch


def ar_loss(pred, data, no_sampling=False):
    """train_ar.py:116-127 / 169-177 for one batch: ``pred`` the :data:`pretrained_score_encoder.ARLogits` of the model, ``data`` the batch of ``ar_batch``.
    Returns (the mean loss over the graphs, loss [G], correct [G] = 1.0 where the student's argmax is the label's); one launch, no read-back.  With
    ``no_sampling`` the label is softmax of the teacher's logits (a soft cross-entropy)."""
    loss, pick, target = ragged_node_cross_entropy(pred.logit_l, pred.logit_r, data.lig_ptr, data.rec_ptr, data.teacher_l, data.teacher_r, data.decoding_idx,
                                                   soft=bool(no_sampling))
    return loss.sum() / loss.shape[0], loss, (pick == target).float()


def train_ar_epoch(model, complexes, labels, optimizer, batch_size, seed, epoch, num_accumulation_steps=1, no_sampling=False):
    """train_ar.py:107-149: one epoch over ``complexes`` in the order ``training.epoch_permutation(len(complexes), seed, epoch)`` in batches of
    ``batch_size``; every item is drawn with draw = epoch (a new decoding index and a new start pose every epoch).  Per batch: ``ar_batch`` ->
    ``model(data, seed=...)`` -> ``ar_loss`` / num_accumulation_steps -> ``backward``; the optimizer steps after every ``num_accumulation_steps`` batches and
    after the last.  The meter is added up on the device and read back ONCE: {'ar_loss': the mean over the batches}.  A pure function of (the model's
    state, complexes, labels, seed, epoch)."""
    ctx = _ctx_of(model)
    model.train()
    order = epoch_permutation(len(complexes), seed, epoch)
    starts = list(range(0, len(order), int(batch_size)))
    total = torch.zeros((), dtype=torch.float64, device=torch.device('cuda', ctx.device))
    optimizer.zero_grad()
    for step, at in enumerate(starts):
        ids = order[at:at + int(batch_size)]
        data = ar_batch(model, [complexes[i] for i in ids], labels, seed, epoch, no_sampling)
        step_seed = _step_seed(seed, epoch, step)
        with torch.random.fork_rng(devices=[ctx.device]):      # the predictors' nn.Dropout layers draw from torch's generators: seeded per step, then put back
            torch.manual_seed(step_seed)
            pred = model(data, seed=step_seed)
        loss = ar_loss(pred, data, no_sampling)[0] / num_accumulation_steps
        loss.backward()
        if (step + 1) % num_accumulation_steps == 0 or step + 1 == len(starts):
            optimizer.step()
            optimizer.zero_grad()
        total += loss.detach().double()
    return {'ar_loss': (total / len(starts)).item() if starts else float('nan')}      # the one read-back


def test_ar_epoch(model, complexes, labels, batch_size, seed, num_latents, no_sampling=False, draw=0):
    """train_ar.py:152-194 without the ``encode_ar`` sweep: the model in ``.eval()`` over ``complexes`` in the order ``epoch_permutation(n, seed, 0)``, items
    drawn with ``draw``.  Returns 'ar_loss' and 'accuracy' (means over the graphs), 'accuracy0' .. 'accuracy{D-1}' (the accuracy of the graphs whose
    decoding index is d; the reference lists these meters and never fills them) and the per-decoding-index interval meters 'int{d}_ar_loss',
    'int{d}_accuracy' (NaN for an index no graph drew).  All sums are kept on the device and read back ONCE."""
    ctx = _ctx_of(model)
    model.eval()
    D = int(num_latents)
    order = epoch_permutation(len(complexes), seed, 0)
    sums = torch.zeros((3, D), dtype=torch.float64, device=torch.device('cuda', ctx.device))      # per decoding index: loss, correct, count
    with torch.no_grad():
        for at in range(0, len(order), int(batch_size)):
            data = ar_batch(model, [complexes[i] for i in order[at:at + int(batch_size)]], labels, seed, draw, no_sampling)
            _, loss, correct = ar_loss(model(data), data, no_sampling)
            hot = torch.nn.functional.one_hot(data.decoding_idx.long(), D).double()      # [G, D]
            sums += torch.stack([loss.double() @ hot, correct.double() @ hot, hot.sum(0)])
    loss, correct, count = (np.asarray(v) for v in sums.tolist())      # the one read-back
    n = count.sum()
    div = lambda a, b: float(a / b) if b > 0 else float('nan')
    out = {'ar_loss': div(loss.sum(), n), 'accuracy': div(correct.sum(), n)}
    for d in range(D):
        out[f'accuracy{d}'] = div(correct[d], count[d])
    for d in range(D):
        out[f'int{d}_ar_loss'], out[f'int{d}_accuracy'] = div(loss[d], count[d]), div(correct[d], count[d])
    return out


test_ar_epoch.__test__ = False      # (a library function, not a test: pytest collects by name)
