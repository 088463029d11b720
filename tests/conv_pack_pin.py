"""What tests/test_conv_pack_pinned.py pins and tests/golden/make_golden_conv_pack.py records: every array csrc/conv_pack.hip packs for a score model and
an all-atom (confidence) model, under each conv_kernel, as it comes back through ddk_debug_export from a host-only context.

The inputs are the same bits on every machine: the keys and shapes of the two random state dicts, every floating tensor overwritten in sorted key order
by an integer pattern (uint64 arithmetic, exact in fp32), so no random generator decides a value."""
import hashlib

import numpy as np
import torch

from oracle import confidence_ref
from oracle import score_model_ref as smr

# context name -> (model, Context keyword arguments)
AA = dict(all_atoms=1, embedding_scale=10000.0, num_confidence_outputs=2)
CONTEXTS = {f'{m}_k{k}': (m, dict(conv_kernel=k, **(AA if m == 'aa' else {}))) for m in ('score', 'aa') for k in (0, 1, 3)}
LAYERS = {'score': [0, 1, 2, 3, 4, 100, 101], 'aa': [0, 1, 2, 3, 4]}          # 100 / 101: tor_bond_conv / final_conv
PER_GROUP = ['w1p', 'b1p', 'w2p', 'b2p']
PER_LAYER = ['wn', 'bnp', 'tiles', 'w1x', 'w2x', 'w1sx', 'xscale', 'bn_mean', 'bn_scale', 'bn_bias']
BN_ITEMS = ('bn_mean', 'bn_scale', 'bn_bias')       # pass through libm powf: pinned as values, within 1 ulp
N_ITEMS = {'score': 158, 'aa': 230}


def pattern_state_dict(P):
    """P with every floating tensor overwritten, in sorted key order, by ((i * 2654435761 + 12345) mod 2^24) / 2^24 - 0.5 (i runs on across tensors);
    a running_var becomes abs(value) + 0.5"""
    out, i0 = dict(P), 0
    for k in sorted(P):
        v = P[k]
        if not torch.is_tensor(v) or not v.is_floating_point():
            continue
        i = np.arange(i0, i0 + v.numel(), dtype=np.uint64)
        i0 += v.numel()
        a = ((i * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(1 << 24)).astype(np.float64) / float(1 << 24) - 0.5
        if k.endswith('running_var'):
            a = np.abs(a) + 0.5
        out[k] = torch.from_numpy(a.astype(np.float32).reshape(tuple(v.shape)))
    return out


def state_dicts():
    return {'score': pattern_state_dict(smr.random_state_dict(smr.ScoreModelConfig(), seed=19)),
            'aa': pattern_state_dict(confidence_ref.random_state_dict(confidence_ref.ConfidenceModelConfig(), seed=40))}


def item_names(model):
    groups = {'score': 4, 'aa': 9}[model]
    names = []
    for l in LAYERS[model]:
        names += [f'conv.{l}.{it}.{g}' for g in range(1 if l >= 100 else groups) for it in PER_GROUP]
        names += [f'conv.{l}.{it}' for it in PER_LAYER]
    assert len(names) == N_ITEMS[model]
    return names


def export_all(name, P):
    """{item: uint32 words} of context `name` loaded with the state dict P"""
    from disco_diffdock_amd.runtime import Context
    model, kw = CONTEXTS[name]
    ctx = Context(device=-1, **kw)
    ctx.load_state_dict(P)
    out = {it: ctx.export(it, np.uint32) for it in item_names(model)}
    ctx.close()
    return out


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()
