"""The bits of the latent-choice ops: every output of the ragged Gumbel softmax, the per-sample Gumbel pick and the ragged node cross-entropy, forward
and backward, on the cases of tests/golden/make_golden_latent_choice_bits.py is recomputed and its SHA-256 compared with
tests/golden/latent_choice_bits.json.  The kernels of csrc/k_gumbel.hip and csrc/k_node_ce.hip share their pointer-pair rule, their walk over a
graph's positions and their halving trees through csrc/k_ragged.h; the fp64 tests of these ops would not see a changed order of additions or a changed
answer where nothing compares.  This test does.

The file pins this toolchain (``log`` and ``exp`` come from the device library).  After a ROCm change it is regenerated (the generator's docstring) from
a commit known to be good, never from the commit under test.  A missing entry is a failure, not a skip: an output without a pinned digest is an
unchecked output."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_latent_choice_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def got():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    from disco_diffdock_amd.tensor_layers import _shape_context
    return gen.digests(_shape_context(0), torch.device('cuda:0'))


@pytest.fixture(scope='module')
def want():
    with open(os.path.join(GOLDEN, 'latent_choice_bits.json')) as f:
        return json.load(f)


def test_every_output_is_pinned(got, want):
    assert not want['unstable'], want['unstable']      # (every output was the same twice where the file was written)
    assert sorted(got) == sorted(want['sha256'])
    assert {k.split('.')[0] for k in want['sha256']} == set(gen.OPS)


@pytest.mark.parametrize('op', gen.OPS)
def test_bits(got, want, op):
    want = want['sha256']
    names = [k for k in got if k.split('.')[0] == op]
    assert names, op
    missing = [k for k in names if k not in want]
    assert not missing, missing
    changed = [k for k in names if got[k] != want[k]]
    print(op, f'{len(names)} outputs, {len(changed)} changed')
    assert not changed, changed
