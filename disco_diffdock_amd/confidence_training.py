"""Training the all-atom confidence model (the reference's confidence/dataset.py:138-179 and confidence/confidence_train.py:111-200) on
``confidence.TrainableConfidenceModel``; the place ``ar_training.py`` has for the AR model.

* ``confidence_labels(rmsd, cutoff)``: ``y``, ``y_binned`` (list cutoffs) and ``rmsd`` of one pose, dataset.py:162-166
* ``confidence_batch(complexes, conf_set, seed, epoch, cutoff)``: one pose per complex by a seeded draw, the labels, all times 0, collated
* ``confidence_loss(pred, batch, rmsd_prediction, cutoff)``: BCE-with-logits, cross-entropy (list cutoffs) or MSE
* ``roc_auc(labels, scores)``: the rank statistic on the device of its operands, average ranks for ties, 0 with one class present
* ``train_confidence_epoch`` / ``test_confidence_epoch``: an epoch is a pure function of (state, set, seed, epoch); one read-back each

A confidence set is ``{name: (positions [S, n, 3], rmsds [S])}``, what the reference's dataset keeps per complex; sampling one with the project's seeded sampler
(``make_confidence_set``) is not part of this module yet.  Not implemented and refused by name: ``balance``, the pickle caches and ``cache_ids_to_combine``,
DDP, the out-of-memory skip, ``transfer_weights``."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .runtime import stream_id

RNG_CONFIDENCE_POSE_PURPOSE = 15      # the next free purpose of the project's seeded draws (runtime.py: 14 is the AR decoding index)
REFUSED = ('balance', 'cache_ids_to_combine', 'cache_creation_id', 'transfer_weights', 'use_original_model_cache', 'DDP')


def refuse_options(args):
    """the reference's options that this module does not implement, by name"""
    for k in REFUSED:
        if getattr(args, k, None):
            raise RuntimeError(f'ddk: confidence training: {k} is not implemented')


def confidence_labels(rmsd, cutoff):
    """dataset.py:162-166 for one pose: dict(y [1], rmsd [1]) and, with a list of cutoffs, y_binned [1, len + 1] (the bin the rmsd falls in) and y against
    the FIRST cutoff"""
    rmsd = float(rmsd)
    out = dict(rmsd=torch.tensor([rmsd], dtype=torch.float32))
    if isinstance(cutoff, (list, tuple)):
        cut = [float(c) for c in cutoff]
        hi, lo = cut + [math.inf], [0.0] + cut
        out['y_binned'] = torch.tensor([[float(lo[i] <= rmsd < hi[i]) for i in range(len(hi))]], dtype=torch.float32)
        out['y'] = torch.tensor([float(rmsd < cut[0])], dtype=torch.float32)
    else:
        out['y'] = torch.tensor([float(rmsd < float(cutoff))], dtype=torch.float32)
    return out


def pose_draw(name, n_samples, seed, epoch):
    """the pose of complex ``name`` in ``epoch``: a pure function of (seed, complex, epoch), whatever batch or order the complex comes in.  Philox keyed by
    (seed, purpose 15) with the counter (stream id of the name, epoch)"""
    key = [(int(seed) & 0xFFFFFFFFFFFFFFFF), RNG_CONFIDENCE_POSE_PURPOSE]
    g = np.random.Generator(np.random.Philox(key=key, counter=[stream_id(name), int(epoch), 0, 0]))
    return int(g.integers(0, int(n_samples)))


def confidence_batch(graphs, names, conf_set, seed, epoch, cutoff):
    """The graphs of one training batch (dataset.py:159-178 without ``balance``): each all-atom complex graph gets one of its sampled poses by
    ``pose_draw``, its labels (``y``, ``y_binned``, ``rmsd``) and every time set to 0.  Returns the list; the caller collates it."""
    out = []
    for g, name in zip(graphs, names):
        positions, rmsds = conf_set[name]
        s = pose_draw(name, len(rmsds), seed, epoch)
        g['ligand'].pos = torch.as_tensor(np.asarray(positions[s]), dtype=torch.float32)
        for k, v in confidence_labels(rmsds[s], cutoff).items():
            setattr(g, k, v)
        for nt in ('ligand', 'receptor', 'atom'):
            g[nt].node_t = {k: torch.zeros(g[nt].num_nodes) for k in ('tr', 'rot', 'tor')}
        g.complex_t = {k: torch.zeros(1) for k in ('tr', 'rot', 'tor')}
        out.append(g)
    return out


def confidence_loss(pred, batch, rmsd_prediction=False, cutoff=2.0):
    """confidence_train.py:122-131 on [B] (or [B, k]) logits: MSE against ``batch.rmsd``, cross-entropy against ``batch.y_binned`` (a list of cutoffs),
    else BCE-with-logits against ``batch.y``.  Plain torch."""
    dev = pred.device
    if rmsd_prediction:
        return F.mse_loss(pred, batch.rmsd.to(dev))
    if isinstance(cutoff, (list, tuple)):
        return F.cross_entropy(pred, batch.y_binned.to(dev))
    return F.binary_cross_entropy_with_logits(pred, batch.y.to(dev))


def roc_auc(labels, scores):
    """sklearn.metrics.roc_auc_score as a rank statistic on the device of ``scores``, no read-back: (sum of the positives' ranks - n_pos (n_pos + 1) / 2)
    / (n_pos n_neg) with AVERAGE ranks for tied scores; 0 when one class is present (the reference's ``except``).  [B, k] labels and scores (a list of
    cutoffs): the mean over the columns, sklearn's macro average, 0 when any column holds one class.  A 0-dim tensor."""
    if labels.dim() == 2 and labels.shape[1] > 1 and scores.shape == labels.shape:
        cols = torch.stack([roc_auc(labels[:, c], scores[:, c]) for c in range(labels.shape[1])])
        present = torch.stack([(labels[:, c] > 0.5).any() & (labels[:, c] <= 0.5).any() for c in range(labels.shape[1])]).to(cols.device)
        return torch.where(present.all(), cols.mean(), torch.zeros_like(cols[0]))
    y, s = labels.reshape(-1).to(scores.device) > 0.5, scores.reshape(-1).double()
    vals, inv, counts = torch.unique(s, sorted=True, return_inverse=True, return_counts=True)
    end = torch.cumsum(counts, 0).double()      # the last (1-based) rank of each distinct score
    rank = (end - (counts.double() - 1) / 2)[inv]
    n_pos, n_neg = y.sum().double(), (~y).sum().double()
    u = (rank * y.double()).sum() - n_pos * (n_pos + 1) / 2
    return torch.where((n_pos > 0) & (n_neg > 0), u / (n_pos * n_neg).clamp(min=1), torch.zeros((), dtype=torch.float64, device=s.device))


def epoch_order(n, seed, epoch):
    """the seeded permutation of an epoch's complexes"""
    g = np.random.Generator(np.random.Philox(key=[(int(seed) & 0xFFFFFFFFFFFFFFFF), RNG_CONFIDENCE_POSE_PURPOSE], counter=[0, int(epoch), 1, 0]))
    return [int(i) for i in g.permutation(int(n))]


def _batches(make_graph, names, conf_set, collate, batch_size, seed, epoch, cutoff, order):
    for a in range(0, len(order), batch_size):
        pick = [names[i] for i in order[a:a + batch_size]]
        batch = collate(confidence_batch([make_graph(n) for n in pick], pick, conf_set, seed, epoch, cutoff))
        batch.complex_t = {k: torch.zeros(len(pick)) for k in ('tr', 'rot', 'tor')}      # (whatever the collate made of the per-graph dicts)
        yield batch, a // batch_size


def train_confidence_epoch(model, optimizer, make_graph, names, conf_set, collate, batch_size, seed, epoch, cutoff=2.0, rmsd_prediction=False, device=None):
    """confidence_train.py:111-147: a seeded permutation of the complexes, one seeded pose each, a batch of one graph skipped as there (BatchNorm).  The
    meter stays on the device; ONE read-back at the end.  ``make_graph(name)`` -> a fresh all-atom graph, ``collate(list)`` -> the batch.  A pure function
    of (model and optimizer state, set, seed, epoch).  Returns dict(confidence_loss=mean over the batches run, batches=their number)."""
    model.train()
    device = device or next(model.parameters()).device
    total, n = torch.zeros((), dtype=torch.float64, device=device), 0
    for batch, i in _batches(make_graph, names, conf_set, collate, batch_size, seed, epoch, cutoff, epoch_order(len(names), seed, epoch)):
        if int(batch.num_graphs) == 1:      # "Skipping batch of size 1 since otherwise batchnorm would not work."
            continue
        optimizer.zero_grad()
        pred = model(batch.to(device), seed=(int(seed) * 1000003 + int(epoch) * 1009 + i) & ((1 << 63) - 1))
        loss = confidence_loss(pred, batch, rmsd_prediction, cutoff)
        loss.backward()
        optimizer.step()
        total, n = total + loss.detach().double(), n + 1
    return dict(confidence_loss=float(total / max(n, 1)), batches=n)


def test_confidence_epoch(model, make_graph, names, conf_set, collate, batch_size, seed, epoch, cutoff=2.0, rmsd_prediction=False, device=None, return_logits=False):
    """confidence_train.py:149-200 in evaluation mode: per batch the loss, the accuracy (pred > 0 against y) and the ROC AUC (``roc_auc``, 0 with one class),
    averaged over the batches as the reference's unpooled meter does, and the baseline metric (the fraction of positives, or the mean absolute deviation
    of the rmsds) over the whole set.  Everything stays on the device; ONE read-back."""
    model.eval()
    device = device or next(model.parameters()).device
    rows, labels, logits = [], [], []
    for batch, _ in _batches(make_graph, names, conf_set, collate, batch_size, seed, epoch, cutoff, list(range(len(names)))):
        with torch.no_grad():
            pred = model(batch.to(device))
        loss = confidence_loss(pred, batch, rmsd_prediction, cutoff).double()
        zero = torch.zeros((), dtype=torch.float64, device=device)
        if rmsd_prediction:
            lab, acc, auc = batch.rmsd.to(device), zero, zero
        elif isinstance(cutoff, (list, tuple)):
            lab, acc = batch.y_binned.to(device), zero
            auc = roc_auc(lab, pred)
        else:
            lab = batch.y.to(device)
            acc, auc = (lab == (pred > 0).float()).double().mean(), roc_auc(lab, pred)
        rows.append(torch.stack([loss, acc, auc]))
        labels.append(lab.reshape(-1).double())
        logits.append(pred.detach())
    lab = torch.cat(labels)
    base = (lab - lab.mean()).abs().mean() if rmsd_prediction else lab.sum() / lab.numel()
    loss, acc, auc, base = torch.cat([torch.stack(rows).mean(0), base.reshape(1)]).tolist()      # the one read-back
    out = dict(confidence_loss=loss, accuracy=acc, roc_auc=auc, baseline_metric=base)
    if return_logits:
        out['logits'], out['labels'] = logits, labels
    return out
