"""Host mirror of the reference's utils/sampling.py: same ``sampling(...)`` signature and return value
(sampling.py:49-54,249) and ``randomize_position`` (:12-46).  The 20-step loop itself - score model forward,
SDE perturbation, SE(3)/torsion update, Kabsch re-alignment - runs inside libddk.so (``ddk_sample``) without any
host synchronisation; this file only prepares the per-step host scalars exactly as the reference computes them.
``visualization_list`` works as in the reference (:224-228: the poses after every batch), and the extra keyword ``trajectory=[]``
collects what the loop did step by step - poses, scores, perturbations, edge counts - recorded on the device by the launches the
sampler makes anyway (``ddk_sample_trajectory``).  With ``ar_model=None`` a latent-conditioned model samples with ORACLE latents
(``oracle_latents``: the encoder of ``model.encoder`` on the true pose, once per batch, then one ``ddk_gumbel_pick_samples`` launch for the batch's
samples); ``compute_ar_accuracy`` compares them with the AR model's picks."""
import collections

import numpy as np
import torch

from .data import DataLoader
from .diffusion_utils import set_time
from .runtime import CONF_OVERFLOW_WORD, RNG_PURPOSES, h2d_async, stream_id
from .score_model import complex_for_batch


def is_iterable(arr):
    try:
        iter(arr)
        return True
    except TypeError:
        return False


def _rng_stream_of(data_list, rng_stream):
    """the generator's 64-bit complex id of a seeded call: the caller's ``rng_stream``, else runtime.stream_id of the complex name"""
    if rng_stream is not None:
        return int(rng_stream)
    name = getattr(data_list[0], 'name', None)
    while isinstance(name, (list, tuple)) and len(name):
        name = name[0]
    if not isinstance(name, str):
        raise ValueError('ddk: a seeded call needs rng_stream=... or a complex with a name (its stream id is runtime.stream_id(name))')
    return stream_id(name)


def randomize_position(data_list, no_torsion, no_random, tr_sigma_max, unbatched=False, ar_args=None, device=None, seed=None, rng_stream=None,
                       sample_offset=0):
    """utils/sampling.py:12-46 with the reference's signature.  The random draws come from the reference's own RNG streams in
    the reference's order; the geometry (torsion rotations, centring, random rotation, translation) runs on the GPU in one
    ``ddk_randomize_position`` launch (:func:`randomize_position_device`).  Limitation (documented in INTEGRATION.md):
    ``data_list`` must hold copies of ONE complex, which is what evaluate.py:232 passes; ``device`` defaults to the current
    CUDA device.

    ``seed`` (extra, optional): with a seed every draw is made on the device by the counter-based generator (``ddk_rng_initial``): graph i gets the
    draws of global sample ``sample_offset + i`` of complex ``rng_stream`` (default: runtime.stream_id of the complex name), whatever the length of the
    list and whatever was drawn before; no host RNG, scipy or upload is involved."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('ddk: randomize_position runs on the GPU only (no CPU fallback)')
        device = torch.device('cuda', torch.cuda.current_device())
    randomize_position_device(data_list, no_torsion, no_random, tr_sigma_max, device, seed=seed, rng_stream=rng_stream, sample_offset=sample_offset)
    if ar_args is not None and ar_args.no_randomness and seed is not None:   # utils/sampling.py:36-46 with the rotations of purpose 5
        from .tensor_layers import _shape_context
        device = torch.device(device)
        ctx = _shape_context(device.index if device.index is not None else torch.cuda.current_device())
        _, rot, _ = ctx.rng_initial(seed, _rng_stream_of(data_list, rng_stream), sample_offset, len(data_list), 0, torsions=False, translations=False,
                                    purpose_rot=RNG_PURPOSES['ar_rotation'])
        for i, g in enumerate(data_list):
            ar = h2d_async(torch.from_numpy(np.asarray(g['ligand'].orig_rdkit_pos[0])).float(), device)
            g['ligand'].ar_pos = (ar - torch.mean(ar, dim=0, keepdim=True)) @ rot[i].T
    elif ar_args is not None:   # utils/sampling.py:36-46: the pose the AR model sees
        from scipy.spatial.transform import Rotation as R
        for g in data_list:
            if ar_args.no_randomness:
                ar = torch.from_numpy(np.asarray(g['ligand'].orig_rdkit_pos[0])).float()
                center = torch.mean(ar, dim=0, keepdim=True)
                rot = torch.from_numpy(R.random().as_matrix()).float()
                g['ligand'].ar_pos = ((ar - center) @ rot.T).to(device)
            else:
                g['ligand'].ar_pos = g['ligand'].pos.clone()


def randomize_position_device(data_list, no_torsion, no_random, tr_sigma_max, device, seed=None, rng_stream=None, sample_offset=0):
    """``randomize_position`` (utils/sampling.py:12-34) for the usual case that ``data_list`` holds N copies of ONE complex
    (evaluate.py:232): the random draws are taken on the host from the reference's own RNG streams in the reference's
    order (np.random.uniform per graph, then scipy ``Rotation.random()`` and ``torch.normal`` per graph), the geometry of
    all N copies runs in one ``ddk_randomize_position`` launch, and every ``g['ligand'].pos`` becomes a view of the
    resulting device tensor.  With ``seed`` the three arrays come from ONE ``ddk_rng_initial`` launch instead (see :func:`randomize_position`) and go
    straight into ``ddk_randomize_position``: no host loop, no upload of draws."""
    from .data import collate
    from .score_model import complex_for_batch
    if device is None or torch.device(device).type != 'cuda':
        raise RuntimeError('ddk: randomize_position_device needs a cuda device (no CPU fallback)')
    device = torch.device(device)
    g0, N = data_list[0], len(data_list)
    n_lig = g0['ligand'].pos.shape[0]
    if any(g['ligand'].pos.shape[0] != n_lig or getattr(g, 'name', None) != getattr(g0, 'name', None) for g in data_list):
        raise RuntimeError('ddk: randomize_position_device expects copies of one complex')
    n_rot = int(g0['ligand'].edge_mask.sum())
    if seed is not None:
        cx, _ = complex_for_batch(collate([g0]), device, need_model=False)
        tor, rot, tr = cx.ctx.rng_initial(seed, _rng_stream_of(data_list, rng_stream), sample_offset, N, n_rot, tr_sigma=tr_sigma_max,
                                          torsions=not no_torsion, translations=not no_random)
        pos = cx.randomize_position(h2d_async(torch.as_tensor(np.asarray(g0['ligand'].pos.cpu(), np.float32)), device), rot,
                                    tor if n_rot > 0 else None, tr)
        for b, g in enumerate(data_list):
            g['ligand'].pos = pos[b]
        return pos
    from scipy.spatial.transform import Rotation as R
    tor = None
    if not no_torsion:
        tor = np.stack([np.random.uniform(low=-np.pi, high=np.pi, size=n_rot) for _ in data_list]).astype(np.float32)
    rot = np.empty((N, 3, 3), np.float32)
    tr = None if no_random else torch.empty((N, 3))
    for b in range(N):
        rot[b] = R.random().as_matrix()
        if not no_random:
            tr[b] = torch.normal(mean=0, std=tr_sigma_max, size=(1, 3))[0]
    cx, _ = complex_for_batch(collate([g0]), device, need_model=False)
    pos = cx.randomize_position(torch.as_tensor(np.asarray(g0['ligand'].pos.cpu(), np.float32)).to(device), torch.from_numpy(rot).to(device),
                                None if tor is None or n_rot == 0 else torch.from_numpy(tor).to(device),
                                None if tr is None else tr.to(device))
    for b, g in enumerate(data_list):
        g['ligand'].pos = pos[b]
    return pos


_pending = []      # bookkeeping objects whose device read-back has not been looked at yet


class _Bookkeeping:
    """The host-side results of one sampling() batch that need a device read-back: the latent bookkeeping of utils/sampling.py:205-221
    (``latent_str`` / ``latent_pos`` from the AR picks and the final poses) and the confidence model's edge-capacity flag.  The copies
    are enqueued behind the sampler into pinned memory; nothing waits for them inside sampling(), so the host goes on to the next
    complex while the GPU works.  ``resolve()`` (first access of ``d.latent_str`` / ``d.latent_pos`` on this module's graph
    container, the next sampling() call once the copies have landed, or immediately for foreign containers) fills every graph of the
    batch that is still alive (the graphs are held weakly: a batch nobody kept costs nothing).
    The capacity flag cannot be raised by the ligand-atom edge list any more (round 5: ddk_complex_set_atoms sizes it from the receptor's geometry, a bound no pose
    can exceed); it stays as a guard of the other edge groups' worst-case capacities: a batch that raised it would carry NaN confidences (conf_head_kernel),
    returned as -1000 like the reference's nan_to_num, and the warning below."""

    def __init__(self, graphs, choices, flat, len_lig, latent_dim, conf_cx, ar_accuracy=None):
        import weakref
        self.graphs = [weakref.ref(g) for g in graphs]
        self.name = getattr(graphs[0], 'name', None) if graphs else None
        self.len_lig, self.latent_dim = len_lig, latent_dim
        self.done = False
        self._resolving = False
        self.bound = False       # the graphs carry this object as ``_lazy`` (our HeteroData): a graph a later call re-used is skipped
        self.choices = self.flat = self.ar_accuracy = None
        self.conf_status = conf_cx.confidence_status_async() if conf_cx is not None else None
        if choices is not None:
            self.choices = torch.empty(choices.shape, dtype=choices.dtype, pin_memory=True)
            self.choices.copy_(choices, non_blocking=True)
            self.flat = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
            self.flat.copy_(flat.detach(), non_blocking=True)
        if ar_accuracy is not None:      # [1] on the device (utils/sampling.py:90-101): it comes back with the picks
            self.ar_accuracy = torch.empty(ar_accuracy.shape, dtype=ar_accuracy.dtype, pin_memory=True)
            self.ar_accuracy.copy_(ar_accuracy, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def _check_conf(self):
        st, self.conf_status = self.conf_status, None
        if st is not None and int(st[CONF_OVERFLOW_WORD]) != 0:
            import warnings
            warnings.warn(f'ddk: ligand-atom edge capacity overflow in a confidence batch of complex {self.name!r}: its confidences were '
                          'returned as -1000 (NaN on the device)', RuntimeWarning)

    def resolve(self):
        if self.done or self._resolving:
            return
        self._resolving = True       # (done is set only when the bookkeeping below has finished: an exception part-way leaves the object retryable)
        try:
            self._resolve()
            self.done = True
        finally:
            self._resolving = False

    def _resolve(self):
        self.event.synchronize()
        if self in _pending:
            _pending.remove(self)
        self._check_conf()
        if self.choices is None:
            return
        ch, n = self.choices.tolist(), self.len_lig
        accuracy = None if self.ar_accuracy is None else float(self.ar_accuracy.reshape(-1)[0])
        for i, ref in enumerate(self.graphs):
            d_i = ref()
            if d_i is None or (self.bound and d_i.__dict__.get('_lazy') is not self):      # collected, or re-used by a later sampling() call
                continue
            lat_str, lat_pos = "", []
            center = d_i.original_center.detach().cpu()
            for j in range(self.latent_dim):
                idx = ch[i][j]
                if not 0 <= idx < n + d_i['receptor'].pos.shape[0]:
                    raise RuntimeError(f'ddk: AR pick {idx} outside the graph of complex {self.name!r}')
                if idx < n:
                    lat_str += 'L' + str(idx)
                    lat_pos.append(self.flat[i * n + idx:i * n + idx + 1] + center)
                else:
                    idx -= n
                    lat_str += 'R' + str(idx)
                    lat_pos.append(d_i['receptor'].pos[idx:idx + 1].detach().cpu() + center)
            d_i.__dict__.pop('_lazy', None)
            d_i.latent_str = lat_str
            d_i.latent_pos = torch.cat(lat_pos, dim=0)
            if accuracy is not None:
                d_i.ar_accuracy = accuracy
        self.choices = self.flat = self.ar_accuracy = None      # the pinned buffers go back to the allocator


def _poll_pending():
    """look (without waiting) at the read-backs of earlier calls: whatever has landed is resolved and dropped, so nothing accumulates
    when a caller never reads ``latent_str`` (warm-up calls, re-used graphs)"""
    for bk in list(_pending):
        if bk.event.query():
            bk.resolve()


_NO_ENCODER = ('ddk: sampling with oracle latents (ar_model=None, or compute_ar_accuracy) needs model.encoder, and the checkpoint loaded into this model '
               'had no encoder.* keys (ModelWrapper.load_state_dict builds the encoder from them; ModelWrapper.attach_encoder takes a live TPEncoder); '
               'pass ar_model= to sample with the AR model\'s latents instead')


def oracle_latents(model, batch, temperature=0.01, seed=None, rng_stream=None, sample0=0):
    """The oracle latents of a sampling() batch, utils/sampling.py:69-76: ``batch`` is a ``data.collate`` batch of b copies of ONE complex, whose true
    pose the encoder reads and nothing else, so ``model.encoder.logits`` runs ONCE, on the batch's first graph (the reference runs it on all b copies),
    and ONE ``ddk_gumbel_pick_samples`` launch draws the b samples' one-hot latents from that table: (latent_l [b n_lig, D], latent_r [b n_rec, D],
    choices int32 [b, D]) on the device, ``choices`` the picked position, ligand nodes first, then n_lig + the receptor index.  Graph i is global sample
    ``sample0 + i`` of the complex ``rng_stream`` (default: runtime.stream_id of the first graph's name) under ``seed`` (None: one draw from torch's
    default CPU generator, as the encoder makes itself), draw 0, DDK_GUMBEL_LAYOUT: a sample's latents do not depend on the batch it is in.  The first
    graph needs the true centred pose in ``['ligand'].orig_pos_torch`` and a name.  The encoder takes that graph from the host, not from the sampler's
    cached complex: its receptor features go up once per batch ([n_rec, 1281] floats with ESM columns, 1.5 MB at 300 residues), inside the 5 ms the
    encoder's forward takes (profiles/oracle_latents_kernel_stats.md).  ``encoder.latent_temperature`` is set to ``temperature``, as the
    reference does; the encoder runs in ``.eval()`` and is left in the mode it was in."""
    from .data import collate
    from .tensor_layers import _draw_seed
    wrapper = model.module if hasattr(model, 'module') else model
    encoder = getattr(wrapper, 'encoder', None)
    if encoder is None:
        raise RuntimeError(_NO_ENCODER)
    ctx = getattr(wrapper, 'score_model', wrapper).ctx
    dev = torch.device('cuda', ctx.device)
    b = int(batch.num_graphs)
    first = getattr(batch, 'first', None)
    if first is None:
        if b != 1:
            raise RuntimeError('ddk: oracle_latents takes a data.collate batch (it reads the first graph through batch.first)')
        first = batch
    lig = first['ligand']
    name = getattr(first, 'name', None)
    while isinstance(name, (list, tuple)) and len(name):
        name = name[0]
    pose = getattr(lig, 'orig_pos_torch', None) if 'orig_pos_torch' in lig else None
    if pose is None or not isinstance(name, str):
        raise RuntimeError("ddk: oracle latents need the complex's true centred pose in data['ligand'].orig_pos_torch ([n_lig, 3], the frame of "
                           "data['receptor'].pos) and its name in data.name (the stream of its Gumbel noise); the first graph of the batch has "
                           + ('neither' if pose is None and not isinstance(name, str) else 'no orig_pos_torch' if pose is None else 'no name'))
    pose = torch.as_tensor(np.asarray(pose, np.float32) if not torch.is_tensor(pose) else pose).float().reshape(-1, 3)
    if pose.shape[0] != lig.pos.shape[0]:
        raise RuntimeError(f"ddk: data['ligand'].orig_pos_torch must hold one row per ligand atom ({lig.pos.shape[0]}); got {pose.shape[0]}")
    one = first if first is batch else collate([first])
    kept = lig.orig_pos_torch
    one['ligand'].orig_pos_torch = h2d_async(pose, dev)
    encoder.latent_temperature = temperature
    was = encoder.training
    encoder.eval()
    try:
        with torch.no_grad():
            logit_l, logit_r, _, _ = encoder.logits(one)
    finally:
        encoder.train(was)
        if one is first:      # (a lone graph handed in as it is: the caller's pose stays the caller's tensor)
            lig.orig_pos_torch = kept
    if seed is None:
        seed = _draw_seed()
    if rng_stream is None:
        rng_stream = stream_id(name)
    return ctx.gumbel_pick_samples(logit_l, logit_r, b, temperature, seed, rng_stream, sample0=sample0, draw=0)


def draw_noise(inference_steps, b, R_total, R, nc, device):
    """N(0,1) draws of one batch from the device generator, [steps, b, 6 + R_total] (tr xyz, rot xyz, torsions; utils/sampling.py:146-164
    draws them step by step on the host): one launch per contiguous run of steps that use noise - normally ONE for the whole trajectory.
    Steps whose noise coefficients are all zero (no_final_step_noise) draw nothing, like the reference; torsion columns past R stay zero."""
    z = torch.empty((inference_steps, b, 6 + R_total), device=device)
    active = [bool(nc[t].any()) for t in range(inference_steps)]
    t = 0
    while t < inference_steps:
        u = t
        while u < inference_steps and active[u] == active[t]:
            u += 1
        if active[t]:
            z[t:u].normal_(mean=0, std=1)
        else:
            z[t:u].zero_()
        t = u
    if R != R_total:
        z[:, :, 6 + R:] = 0
    return z


def step_coefficients(inference_steps, tr_schedule, rot_schedule, tor_schedule, t_to_sigma, model_args, ode, no_random,
                      no_final_step_noise, temp_sampling, temp_psi, temp_sigma_data):
    """Host scalars of every reverse step, formed with the reference's expressions and dtypes
    (utils/sampling.py:106-111,137-192): perturb = score_coeff*score + noise_coeff*z per tr/rot/tor."""
    if not is_iterable(temp_sampling):
        temp_sampling = [temp_sampling] * 3
    if not is_iterable(temp_psi):
        temp_psi = [temp_psi] * 3
    if not is_iterable(temp_sigma_data):
        temp_sigma_data = [temp_sigma_data] * 3
    assert len(temp_sampling) == 3 and len(temp_psi) == 3 and len(temp_sigma_data) == 3
    scheds = (tr_schedule, rot_schedule, tor_schedule)
    lims = ((model_args.tr_sigma_min, model_args.tr_sigma_max), (model_args.rot_sigma_min, model_args.rot_sigma_max),
            (model_args.tor_sigma_min, model_args.tor_sigma_max))
    t_arr = np.zeros((inference_steps, 3), np.float32)
    sc = np.zeros((inference_steps, 3), np.float32)
    nc = np.zeros((inference_steps, 3), np.float32)
    for t_idx in range(inference_steps):
        ts = [s[t_idx] for s in scheds]
        sig = t_to_sigma(*ts)
        zero = no_random or (no_final_step_noise and t_idx == inference_steps - 1)
        for k in range(3):
            s = scheds[k]
            dt = s[t_idx] - s[t_idx + 1] if t_idx < inference_steps - 1 else s[t_idx]
            lo, hi = lims[k]
            g = sig[k] * torch.sqrt(torch.tensor(2 * np.log(hi / lo)))
            if ode:
                a, b = 0.5 * g ** 2 * dt, 0.0 * g
                if temp_sampling[k] != 1.0:
                    raise RuntimeError('ode=True with temp_sampling != 1 is undefined in the reference (sampling.py:142-144 vs :182)')
            else:
                a, b = g ** 2 * dt, g * np.sqrt(dt)
            if temp_sampling[k] != 1.0:
                sd = np.exp(temp_sigma_data[k] * np.log(hi) + (1 - temp_sigma_data[k]) * np.log(lo))
                lam = (sd + sig[k]) / (sd + sig[k] / temp_sampling[k])
                a = g ** 2 * dt * (lam + temp_sampling[k] * temp_psi[k] / 2)
                b = g * np.sqrt(dt * (1 + temp_psi[k]))
            t_arr[t_idx, k] = ts[k]
            sc[t_idx, k] = float(a)
            nc[t_idx, k] = 0.0 if zero else float(b)
    return t_arr, sc, nc


def _host_single_thread(fn):
    """The host side of a call is a few ms of small tensor bookkeeping that must stay ahead of the GPU; it runs with ONE torch CPU thread:
    on a 128-thread host an OpenMP-parallel torch CPU op (a collate ``torch.cat``, a checksum) was measured to stall for a whole
    reverse-diffusion loop (70-100 ms) while the HIP runtime is busy, which starves the GPU queue (tools/host_calls.py).  The caller's
    thread setting is restored on return."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        n_thr = torch.get_num_threads()
        if n_thr > 1:
            torch.set_num_threads(1)
        try:
            return fn(*args, **kwargs)
        finally:
            if n_thr > 1:
                torch.set_num_threads(n_thr)
    return wrapper


@_host_single_thread
def sampling(data_list, model, inference_steps, tr_schedule, rot_schedule, tor_schedule, device, t_to_sigma, model_args,
             no_random=False, ode=False, visualization_list=None, confidence_model=None, confidence_data_list=None,
             confidence_model_args=None, batch_size=32, no_final_step_noise=False, use_latent=True,
             gumbel_latent_temperature=0.01, ar_model=None, ar_args=None, temp_sampling=1.0, temp_psi=0.0, temp_sigma_data=0.5,
             classifier_free_guidance_weight=0.0, softmax_latent_temperature=1.0, cfg_start=1.0, cfg_end=0.0,
             compute_ar_accuracy=False, noise=None, trajectory=None, seed=None, rng_stream=None, sample_offset=0):
    """``ar_model=None`` on a latent-conditioned model (utils/sampling.py:69-78, ``evaluate.py --oracle``): the latents are ORACLE latents, ``model.encoder``
    on the true pose (every graph's ``['ligand'].orig_pos_torch``) once per batch and one draw per sample at ``gumbel_latent_temperature``
    (:func:`oracle_latents`); with ``seed`` graph i draws as global sample ``sample_offset + i``, whatever the batch.  ``compute_ar_accuracy=True`` with an
    ``ar_model`` runs both, samples with the AR latents and stores ``ar_accuracy`` on every graph of a batch: the share of its samples whose AR pick for
    latent dimension 0 is the oracle's (filled with ``latent_str`` / ``latent_pos`` from the one read-back).

    ``noise`` (extra, optional): list with one tensor [steps, b, 6+R] per batch of N(0,1) draws (tr xyz, rot xyz,
    torsions) to replace the device generator - used by the parity tests (the reference never seeds its RNGs).

    ``seed`` (extra, optional): None draws as above, from torch's device generator.  With a seed every draw of the call - the step noise and the AR picks -
    is made on the device by the counter-based generator (``ddk_rng_noise`` / ``ddk_rng_uniform``, DDK_RNG_LAYOUT of include/ddk.h) as a pure function of
    (seed, ``rng_stream``, global sample index, step, column): graph i of ``data_list`` is global sample ``sample_offset + i`` of the complex with the 64-bit id
    ``rng_stream`` (default: runtime.stream_id of the complex name).  Its draws are then the same bits whatever ``batch_size``, however the samples of the
    complex are spread over calls or ranks (a rank that holds samples 5..9 passes ``sample_offset=5``) and whatever ran before; the POSES are the same bits
    when the model's context is also ``deterministic = 1``.  ``noise=`` together with ``seed=`` is a ValueError.

    ``visualization_list`` (utils/sampling.py:224-228; evaluate.py --save_visualisation): the caller's objects, anything with
    ``.add(coords, part, order)``.  As in the reference the WHOLE list is walked after EVERY batch: with n batches entry ``idx`` receives n calls
    ``add(data_list[idx]['ligand'].pos.cpu() + data_list[idx].original_center.cpu(), part=1, order=2)``, in batch order and, within a batch, in list order; the
    calls made before graph ``idx``'s own batch has run carry its start pose, the others its final pose (so the last call always does).  The ``.cpu()``
    waits for the batch, as it does in the reference; here it comes after the batch's confidence model has been enqueued.

    ``trajectory`` (extra, optional): a list that receives one :data:`runtime.Trajectory` per batch - device tensors ``pos`` [steps + 1, b, n_lig, 3]
    (row k: before step k, centred coordinates like ``['ligand'].pos``; row ``steps`` = the returned poses), ``scores`` / ``perturb`` [steps, b, 6 + R] and
    ``edge_counts`` [steps, 4] - recorded by the sampler's own launches; sampling() adds no synchronisation for it."""
    if seed is not None and noise is not None:
        raise ValueError('ddk: sampling() takes noise= (the draws themselves) or seed= (the generator), not both')
    if seed is not None:
        rng_stream = _rng_stream_of(data_list, rng_stream)
    confidence, confidence_loader = None, None
    if confidence_model is not None:      # utils/sampling.py:59-62
        cg_conf = getattr(confidence_model, 'score_model', confidence_model)
        if confidence_data_list is None:
            # utils/sampling.py:239-240: a coarse-grained confidence model (TensorProductScoreModel in confidence_mode, reached by evaluate.py's
            # use_original_model_cache / transfer_weights flags) evaluated on the score batch itself
            if not getattr(cg_conf, 'confidence_mode', False):
                raise RuntimeError('ddk: an all-atom confidence model needs confidence_data_list (the score graphs carry no atoms); only a '
                                   'coarse-grained confidence model (get_model(args, ..., confidence_mode=True) without all_atoms) runs on the score batch')
        else:
            cg_conf = None
        confidence_loader = iter(DataLoader(confidence_data_list, batch_size=batch_size)) if confidence_data_list is not None else None
        confidence = []
    conf_checks = []
    latent_model = use_latent and getattr(model_args, 'latent_dim', 0) > 0
    if classifier_free_guidance_weight != 0.0 and not latent_model:
        raise RuntimeError('ddk: classifier-free guidance needs the latent-conditioned model (sampling.py:119-135)')
    oracle = latent_model and (ar_model is None or compute_ar_accuracy)      # utils/sampling.py:70
    if oracle and getattr(model.module if hasattr(model, 'module') else model, 'encoder', None) is None:
        raise RuntimeError(_NO_ENCODER)
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('ddk sampling runs on the GPU only (no CPU fallback)')
    _poll_pending()
    N = len(data_list)
    loader = DataLoader(data_list, batch_size=batch_size)
    score_model = model.module.score_model if hasattr(model, 'module') else getattr(model, 'score_model', model)
    t_arr, sc, nc = step_coefficients(inference_steps, tr_schedule, rot_schedule, tor_schedule, t_to_sigma, model_args, ode,
                                      no_random, no_final_step_noise, temp_sampling, temp_psi, temp_sigma_data)
    with torch.no_grad():
        for batch_id, batch in enumerate(loader):
            b = batch.num_graphs
            if b != min(batch_size, N):
                raise RuntimeError('ragged last batch: the reference draws noise of size min(batch_size, N) (sampling.py:146-153)')
            cx, _ = complex_for_batch(batch, device, ctx=score_model.ctx)
            latent_h = ar_accuracy = None
            if oracle:         # utils/sampling.py:70-78: the encoder on the true pose, once for the batch, then the b samples' draws in one launch
                true_l, true_r, choices = oracle_latents(model, batch, gumbel_latent_temperature, seed, rng_stream, sample_offset + batch_id * batch_size)
                latent_h = (true_l, true_r)
            if latent_model and ar_model is not None:   # utils/sampling.py:80-85: AR decoding on the ar_pos pose
                true_choices = choices if oracle else None
                lig_st = batch['ligand']      # only the poses go to the device: the encoder's score-model copy takes everything else
                lig_st.pos = h2d_async(lig_st.pos, device)      # from the cached ddk_complex (a batch.to(device) moved 61 MB of ESM features)
                if 'ar_pos' in lig_st:
                    lig_st.ar_pos = h2d_async(lig_st.ar_pos, device)
                temp_lig_pos = batch['ligand'].pos
                if 'ar_pos' in batch['ligand']:
                    batch['ligand'].pos = batch['ligand'].ar_pos
                if seed is None:
                    latent_h = ar_model.encode_ar(batch, softmax_latent_temperature)
                else:
                    latent_h = ar_model.encode_ar(batch, softmax_latent_temperature, rng=(seed, rng_stream, sample_offset + batch_id * batch_size))
                batch['ligand'].pos = temp_lig_pos
                choices = ar_model.last_choices          # [b, latent_dim] picked nodes (device): read back ONCE, after the sampler is enqueued
                if true_choices is not None:             # utils/sampling.py:90-101: the share of the samples whose FIRST latent is the oracle's
                    ar_accuracy = (choices[:, 0].long() == true_choices[:, 0].long()).double().mean().reshape(1)
            if latent_model:   # utils/sampling.py:87-88: the latents condition every step
                batch['ligand'].latent_h, batch['receptor'].latent_h = latent_h
                cx.set_latents(latent_h[0], latent_h[1], 0.0)
                cx.set_guidance(classifier_free_guidance_weight, cfg_start, cfg_end)
            elif score_model.cfg['latent_dim'] > 0:
                raise RuntimeError('ddk: a latent-conditioned score model was given but use_latent / model_args.latent_dim disable the latents')
            pos = h2d_async(batch['ligand'].pos.float(), device).reshape(b, -1, 3).contiguous()
            if pos.data_ptr() == batch['ligand'].pos.data_ptr():
                pos = pos.clone()       # ddk_sample updates in place; the caller's start poses stay intact (the reference rebinds, never mutates)
            R = cx.R if not model_args.no_torsion else 0
            if noise is not None:
                z = noise[batch_id].to(device)
            elif no_random or ode:
                z = None
            elif seed is not None:
                z = score_model.ctx.rng_noise(seed, rng_stream, sample_offset + batch_id * batch_size, b, inference_steps, 6 + cx.R, 6 + R, noise_coeff=nc)
            else:
                z = draw_noise(inference_steps, b, cx.R, R, nc, device)
            if trajectory is not None:
                trajectory.append(cx.sample(pos, t_arr, sc, nc, z, record=True))
            else:
                cx.sample(pos, t_arr, sc, nc, z)
            if confidence_model is not None and cg_conf is not None:
                # utils/sampling.py:239-240: the score batch itself at the final poses; its times are those of the LAST EXECUTED step
                # (t_idx = inference_steps - 1, utils/sampling.py:105-111: the reference resets them only in the confidence_data_list branch),
                # which confidence_mode reads as sigmas.  evaluate.py:269 passes the full schedule with inference_steps = actual_steps, so this
                # is schedule[inference_steps - 1], not schedule[-1]
                last = inference_steps - 1
                out = cg_conf.confidence(batch, pos, (float(tr_schedule[last]), float(rot_schedule[last]), float(tor_schedule[last])))
                confidence.append(out)
            elif confidence_model is not None:   # utils/sampling.py:230-243: final poses into the all-atom graphs, t = 0
                cbatch = next(confidence_loader)
                cbatch['ligand'].pos = pos.reshape(-1, 3)
                set_time(cbatch, 0, 0, 0, b, confidence_model_args.all_atoms if confidence_model_args is not None else True, device)
                from .confidence import ConfidenceModel
                if isinstance(confidence_model, ConfidenceModel):
                    out = confidence_model(cbatch, check=False)       # the capacity flag is read once per call, below
                    conf_checks.append(confidence_model.last_complex)
                else:
                    out = confidence_model(cbatch)
                confidence.append(out[0] if type(out) is tuple else out)
            len_lig = pos.shape[1]
            flat = pos.reshape(-1, 3)
            graphs = [data_list[batch_id * batch_size + i] for i in range(b)]
            for i, d_i in enumerate(graphs):
                d_i['ligand'].pos = flat[i * len_lig:len_lig * (i + 1)]
            if visualization_list is not None:       # utils/sampling.py:224-228: every entry, after every batch
                for idx, visualization in enumerate(visualization_list):
                    visualization.add((data_list[idx]['ligand'].pos.detach().cpu() + data_list[idx].original_center.detach().cpu()),
                                      part=1, order=2)
            if latent_model or conf_checks:
                # latent bookkeeping of utils/sampling.py:205-221 and the confidence model's capacity flag: ONE read-back, enqueued behind the
                # sampler and not awaited here (the reference synchronises 6x per pose)
                from .data import HeteroData
                bk = _Bookkeeping(graphs, choices if latent_model else None, flat, len_lig, getattr(model_args, 'latent_dim', 0),
                                  conf_checks.pop() if conf_checks else None, ar_accuracy=ar_accuracy)
                if latent_model and all(isinstance(d_i, HeteroData) for d_i in graphs):
                    for d_i in graphs:
                        d_i.__dict__.pop('latent_str', None)
                        d_i.__dict__.pop('latent_pos', None)
                        if ar_accuracy is not None:
                            d_i.__dict__.pop('ar_accuracy', None)
                        d_i.__dict__['_lazy'] = bk
                    bk.bound = True
                    _pending.append(bk)
                elif latent_model:
                    bk.resolve()              # foreign graph containers (PyG) cannot fill attributes lazily: wait now
                else:
                    _pending.append(bk)
    if confidence_model is not None:          # utils/sampling.py:245-247
        confidence = torch.nan_to_num(torch.cat(confidence, dim=0), nan=-1000)
    return data_list, confidence


def cluster_poses(data_list, confidence=None, cutoff=2.0, perms=None, heavy_atoms_only=True, ctx=None, auto_cap=65536):
    """The step every consumer of sampling()'s poses takes next: which of them are the same binding mode.  ``data_list``: the graphs sampling()
    returned (poses of ONE ligand, on the device, in the common receptor frame); ``confidence``: its second result, [B] or [B, k] (column 0 ranks, as in
    evaluate.py:317-318), None: list order.  All-pairs RMSD over the heavy atoms (``heavy_atoms_only``: the filterHs mask of evaluate.py:297,
    ``x[:, 0] != 0``), symmetry-corrected when ``perms`` [K, n_lig] holds the ligand's graph automorphisms, then greedy leader clustering
    by confidence within ``cutoff`` A.  ``perms='auto'``: the table is enumerated on the device from the first graph's own ``x[:, 0]`` and bonds over the
    same atoms (runtime.Context.ligand_automorphisms, at most ``auto_cap`` rows); that costs one read-back of its row count, and a ligand whose table does
    not fit is clustered uncorrected, with a warning.  Returns :data:`runtime.PoseClusters` (rmsd [B, B], cluster [B], leaders [B], n_clusters [1]), device tensors: like
    sampling() itself this enqueues and reads nothing back.  ``ctx``: a runtime.Context or a model that owns one (default: a weightless context on the
    poses' device)."""
    lig0 = data_list[0]['ligand']
    pos = torch.stack([d['ligand'].pos for d in data_list])
    if not pos.is_cuda:
        raise RuntimeError('ddk: cluster_poses takes the device poses sampling() returned (no CPU path exists)')
    ctx = getattr(ctx, 'ctx', ctx)
    if ctx is None:
        from .tensor_layers import _shape_context
        ctx = _shape_context(pos.device.index if pos.device.index is not None else torch.cuda.current_device())
    mask = (lig0.x[:, 0] != 0) if heavy_atoms_only else None
    if confidence is not None:
        confidence = torch.as_tensor(confidence)
        if confidence.dim() > 1:
            confidence = confidence[:, 0]
        confidence = h2d_async(confidence.float(), pos.device)
    if isinstance(perms, str):
        if perms != 'auto':
            raise RuntimeError(f"ddk: perms is a table, None or 'auto'; got {perms!r}")
        from .runtime import usable_automorphisms
        table = ctx.ligand_automorphisms(lig0.x[:, 0], data_list[0]['ligand', 'lig_bond', 'ligand'].edge_index, atom_mask=mask, cap=auto_cap)
        perms = usable_automorphisms(*table, name=getattr(data_list[0], 'name', None))
    return ctx.cluster_poses(pos, scores=confidence, cutoff=cutoff, atom_mask=mask, perms=perms)
