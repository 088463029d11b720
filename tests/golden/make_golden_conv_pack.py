#!/usr/bin/env python
"""Generate tests/golden/conv_pack_records.npz: what the library of THIS checkout packs for the pinned state dicts of tests/conv_pack_pin.py.

The file is the yardstick of a refactor of the packer, so it is made from the commit BEFORE the change: check that commit out, copy this script and
tests/conv_pack_pin.py into it, build, run, and commit the file the run leaves.  Needs no reference checkout and no GPU (host-only contexts).

    names   [n] '<context>/<export item>', the six contexts of conv_pack_pin.CONTEXTS
    words   [n] int64   number of 32-bit words of the item (0: the form has no such records)
    sha256  [n] hex digest of the words; '' for the three bn_* items, which are stored as values:
    '<context>/conv.<l>.bn_{mean,scale,bias}'  float32

    python tests/golden/make_golden_conv_pack.py
"""
import os
import sys

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import conv_pack_pin as pin  # noqa: E402


def main():
    from disco_diffdock_amd import build
    build.build(verbose=False)
    P = pin.state_dicts()
    names, words, sha, values = [], [], [], {}
    for name, (model, _) in pin.CONTEXTS.items():
        for it, w in pin.export_all(name, P[model]).items():
            is_bn = it.endswith(pin.BN_ITEMS)
            names.append(f'{name}/{it}')
            words.append(w.size)
            sha.append('' if is_bn else pin.digest(w))
            if is_bn:
                values[f'{name}/{it}'] = w.view(np.float32)
    out = os.path.join(REPO, 'tests', 'golden', 'conv_pack_records.npz')
    np.savez_compressed(out, names=np.array(names), words=np.array(words, np.int64), sha256=np.array(sha), **values)
    print('wrote', out, len(names), 'items,', sum(1 for w in words if w == 0), 'of them empty')


if __name__ == '__main__':
    main()
