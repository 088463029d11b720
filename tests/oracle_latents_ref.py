"""Host fp64 restatement of what ddk_gumbel_pick_samples picks (include/ddk.h): for sample b and latent dimension d the position of the maximum of
logit + gumbel over the ligand nodes followed by the receptor nodes, the noise of DDK_GUMBEL_LAYOUT 1 for global sample ``sample0 + b``
(tests/philox_ref.py for the words, tests/latent_embedding_ref.py for the conversion).  Dividing by the temperature does not move the maximum, so the pick
is a draw from softmax(logits) whatever T.  The test constants that both the GPU tests and the host test read live here, so that the host test can check
on the CPU that the seeds chosen leave no case out."""
import copy

import numpy as np
import torch

import latent_embedding_ref as lref
import philox_ref

# the kernel test's cases (tests/test_gpu_gumbel_samples.py)
SHAPES = ((7, 23), (1, 0), (0, 5), (300, 800))
DIMS, BATCHES, SAMPLE0S, TEMPERATURES = (1, 4), (1, 5), (0, 3), (0.01, 1.0)
SEED, STREAM_NAME, DRAW = 0x0123456789ABCDEF, 'gumbel_samples', 5
GAP = 1e-6
# the statistics case: B samples of six classes, one dimension; chi-square with 5 degrees of freedom below 25.74 (p = 1e-4)
STAT_B, STAT_N, STAT_SEED, STAT_CHI2 = 4096, 6, 20240607, 25.74
STAT_LOGITS = np.array([0.5, -0.25, 1.0, 0.0, -1.0, 0.25], np.float32)


def case_logits(n_lig, n_rec, D):
    """[n_lig + n_rec, D] fp32: values on a grid of 0.5, so that equal logits are common and the noise decides between them, and (from two nodes on) one
    row of -inf, which can never be picked"""
    n = n_lig + n_rec
    rng = np.random.default_rng(1000 * n_lig + 10 * n_rec + D)
    logits = (np.round(rng.standard_normal((n, D)) * 2) / 2).astype(np.float32)
    if n >= 2:
        logits[n // 2] = -np.inf
    return logits


def uniforms(seed, stream, samples, draw, d, n):
    """u [len(samples), n] in fp32, bit-exact: lref.gumbel_uniforms for every sample at once"""
    samples = np.asarray(samples, dtype=np.uint64)
    key = philox_ref.block(seed, stream, samples, lref.GUMBEL_PURPOSE, draw, d)                       # [B, 4]
    quads = np.arange((n + 3) // 4, dtype=np.uint64)
    words = philox_ref.philox4x32_10((quads[None, :], 0, 0, lref.GUMBEL_TAG), (key[:, 0:1], key[:, 1:2]))      # [B, quads, 4]
    return philox_ref.uniform32(words).reshape(len(samples), -1)[:, :n]


def host_picks(logits, seed, stream, sample0, B, draw=0):
    """(picks int64 [B, D], gaps float64 [B, D]): the fp64 argmax of logit + gumbel and the distance to the runner-up (inf for a single node)"""
    logits = np.asarray(logits, np.float64)      # (fp32 tables are exact in fp64; the encoder's fp64 restatement comes as it is)
    n, D = logits.shape
    picks, gaps = np.zeros((B, D), np.int64), np.full((B, D), np.inf)
    for d in range(D):
        v = logits[None, :, d] + lref.gumbel_noise(uniforms(seed, stream, sample0 + np.arange(B), draw, d, n))      # [B, n]
        picks[:, d] = np.argmax(v, axis=1)
        if n > 1:
            top = np.sort(v, axis=1)[:, -2:]
            gaps[:, d] = top[:, 1] - top[:, 0]
    return picks, gaps


def chi_square(picks, logits):
    """Pearson's statistic of the picks' histogram against softmax(logits)"""
    logits = np.asarray(logits, np.float64)
    p = np.exp(logits - logits.max())
    p /= p.sum()
    counts = np.bincount(np.asarray(picks).reshape(-1), minlength=len(p))
    expect = p * counts.sum()
    return float(((counts - expect) ** 2 / expect).sum())


# ---- the oracle-sampling tests (tests/test_gpu_oracle_sampling.py): one complex, a random-init encoder of 3 layers at ns 24 / nv 4, latent_dim 2 ----------------
COMPLEX = dict(seed=31, n_res=40, n_lig=22)
ENCODER = dict(latent_dim=2, latent_vocab=1, sh_lmax=1, ns=24, nv=4, num_conv_layers=3, lig_max_radius=5.0, rec_max_radius=30.0, cross_max_distance=80.0,
               lm_embedding_type='esm', batch_norm=True, dropout=0.1)
ENCODER_SEED, SAMPLING_SEED, SAMPLES, SAMPLING_T, SAMPLING_GAP = 17, 7, 8, 0.01, 1e-3


def sampling_complex():
    from disco_diffdock_amd import synthetic
    return synthetic.make_complex(COMPLEX['seed'], n_res=COMPLEX['n_res'], n_lig=COMPLEX['n_lig'])


def host_encoder(seed=ENCODER_SEED):
    """a TPEncoder on the host with seeded weights, in .eval(); the norm layers' parameters and running buffers are moved off their initial values"""
    from disco_diffdock_amd.latent_encoder import TPEncoder
    torch.manual_seed(seed)
    enc = TPEncoder(None, **ENCODER)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in enc.state_dict().items():
            if 'batch_norm.' in k or k.split('.')[-2] in ('1', '5') and k.startswith('latent_'):
                if k.endswith(('weight', 'running_var')):
                    v.copy_(torch.rand(v.shape, generator=gen) + 0.5)
                elif k.endswith(('bias', 'running_mean')):
                    v.copy_(torch.randn(v.shape, generator=gen) * 0.1)
    return enc.eval()


def logits64(enc, c):
    """[n_lig + n_rec, D] fp64: tests/latent_encoder_ref.encoder_logits (the evaluation branch) on the complex's true pose"""
    import latent_encoder_ref as ler
    from helpers import to_graph
    from oracle import graph_lite
    b = graph_lite.collate([to_graph(c)])
    b['ligand'].orig_pos_torch = b['ligand'].pos.clone()
    b.name = [c['name']]
    cfg = dict(nv=enc.nv, num_conv_layers=enc.num_conv_layers, lig_max_radius=enc.lig_max_radius, rec_max_radius=enc.rec_max_radius,
               cross_max_distance=enc.cross_max_distance, batch_norm=ENCODER['batch_norm'], latent_batchnorm=True)
    P = {k: (v.detach().double() if v.is_floating_point() else v.clone()) for k, v in enc.state_dict().items()}
    with torch.no_grad():
        logit_l, logit_r, _ = ler.encoder_logits(P, cfg, copy.deepcopy(b), torch.float64, training=False)
    return torch.cat([logit_l, logit_r]).numpy()
