"""The bits of the training ops: every output of rtp, rconv, rhid, hconv, eemb and seg_sum on the cases of tests/golden/make_golden_train_ops_bits.py is
recomputed and its SHA-256 compared with tests/golden/train_ops_bits.json.  The fp64 tests of these ops hold them to 1e-5 and to run-to-run agreement;
neither would see a changed order of additions in a parameter gradient or in a node sum.  This test does.

The file pins this toolchain: every number is an fmaf chain or a fixed sequence of adds that any correct build reproduces, except ``expf`` in the edge
embedding, which comes from the device library.  After a ROCm change the file is regenerated (the generator's docstring) from a commit known to be
good, never from the commit under test.  A missing entry is a failure, not a skip: an output without a pinned digest is an unchecked output."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_train_ops_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu
OPS = ('rtp', 'rconv', 'rhid', 'hconv', 'eemb', 'seg_sum')


@pytest.fixture(scope='module')
def got():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return gen.digests(_shape_context(0), torch.device('cuda:0'))


@pytest.fixture(scope='module')
def want():
    with open(os.path.join(GOLDEN, 'train_ops_bits.json')) as f:
        return json.load(f)['sha256']


def test_every_output_is_pinned(got, want):
    assert sorted(got) == sorted(want)
    assert {k.split('.')[0] for k in want} == set(OPS)


@pytest.mark.parametrize('op', OPS)
def test_bits(got, want, op):
    names = [k for k in got if k.split('.')[0] == op]
    assert names, op
    missing = [k for k in names if k not in want]
    assert not missing, missing
    changed = [k for k in names if got[k] != want[k]]
    print(op, f'{len(names)} outputs, {len(changed)} changed')
    assert not changed, changed
