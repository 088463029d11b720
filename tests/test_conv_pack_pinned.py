"""Byte-identity pin of the conv weight packer (csrc/conv_pack.hip): every array a host-only context packs for the conv layers (and, for the score
model, the two heads), under conv_kernel 0, 1 and 3, for a score model and an all-atom model, against tests/golden/conv_pack_records.npz.

The fixture was made by tests/golden/make_golden_conv_pack.py from the library of commit f05a739, the last one whose packer lived in ddk_capi.hip, on
the pinned state dicts of tests/conv_pack_pin.py.  Every item of conv_pack_pin.item_names() is held against it: the word count and the sha256 of the
exported words, exactly - an item a form does not have (w1sx under conv_kernel = 3, the limb records under conv_kernel = 1, wn of a head) is pinned
as empty.  The one comparison that is not exact: bn_mean / bn_scale / bn_bias pass through libm's powf, so they are stored as values and must agree
to 1 ulp of fp32."""
import numpy as np
import pytest

import conv_pack_pin as pin


@pytest.fixture(scope='module')
def built():
    from disco_diffdock_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope='module')
def inputs():
    return pin.state_dicts()


@pytest.fixture(scope='module')
def pinned(golden):
    z = golden('conv_pack_records')
    table = {str(n): (int(w), str(s)) for n, w, s in zip(z['names'], z['words'], z['sha256'])}
    return table, z


def test_fixture_lists_every_item(pinned):
    table, _ = pinned
    want = [f'{name}/{it}' for name, (model, _) in pin.CONTEXTS.items() for it in pin.item_names(model)]
    assert sorted(table) == sorted(want) and len(want) == 3 * 158 + 3 * 230
    empty = {n for n, (w, _) in table.items() if w == 0}
    assert {'score_k3/conv.0.w1sx', 'score_k1/conv.0.w1x', 'score_k1/conv.0.w2x', 'aa_k0/conv.0.w1sx', 'score_k0/conv.100.wn'} <= empty
    assert not {'score_k0/conv.0.w1sx', 'score_k3/conv.0.w1x', 'aa_k3/conv.4.w2x', 'score_k0/conv.101.w2x'} & empty


@pytest.mark.parametrize('name', list(pin.CONTEXTS))
def test_packed_arrays_are_the_pinned_bytes(built, inputs, pinned, name):
    table, z = pinned
    model = pin.CONTEXTS[name][0]
    got = pin.export_all(name, inputs[model])
    assert list(got) == pin.item_names(model)
    bad = []
    for it, w in got.items():
        words, sha = table[f'{name}/{it}']
        if w.size != words:
            bad.append((it, 'words', w.size, words))
        elif it.endswith(pin.BN_ITEMS):
            a, b = w.view(np.float32), z[f'{name}/{it}']
            if not (np.abs(a.astype(np.float64) - b) <= np.spacing(np.abs(b))).all():       # 1 ulp of the pinned value
                bad.append((it, 'value', float(np.abs(a - b).max())))
        elif pin.digest(w) != sha:
            bad.append((it, 'sha256'))
    assert not bad, bad


def test_one_flipped_weight_changes_the_digests(built, inputs, pinned):
    """the pin can fail: one value of layer 2's second linear layer, group 1, with its sign flipped moves that group's fragments and limb records
    (the layer's range scale and its BatchNorm stay) and nothing of another layer"""
    table, _ = pinned
    P = dict(inputs['score'])
    w = P['conv_layers.2.fc.1.4.weight'].clone()
    assert w[5, 7] != 0
    w[5, 7] = -w[5, 7]
    P['conv_layers.2.fc.1.4.weight'] = w
    got = pin.export_all('score_k0', P)
    changed = {it for it, a in got.items() if not it.endswith(pin.BN_ITEMS) and pin.digest(a) != table[f'score_k0/{it}'][1]}
    assert changed == {'conv.2.w2p.1', 'conv.2.w2x'}
