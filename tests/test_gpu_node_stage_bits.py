"""The bits of the plain node finalize behind ddk_conv_forward: the output of every case of tests/golden/make_golden_node_stage_bits.py (score-model
layers 0 and 3 on a conv_kernel = 0 and a conv_kernel = 1 context, layer 3 without edges, one conv of an all-atom layer) is recomputed and its SHA-256
compared with tests/golden/node_stage_bits.json.  These are the three shapes of the launch that tests/test_gpu_pose_bits.py does not reach: a row stride
of dout, no residual with a BatchNorm offset, and dout = 0.  The finalize expression is stated once (csrc/k_node.h: node_finalize_value) and inlined into
three kernels; the fp64 tests hold their outputs to fp32 grade and would see nothing of a multiply-add contracted differently in one of them.

The file pins this toolchain; after a ROCm change it is regenerated (the generator's docstring) from a commit known to be good, never from the commit
under test.  A missing entry is a failure, not a skip."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_golden_node_stage_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def got():
    assert torch.cuda.is_available(), 'GPU tests need a MI355X'
    from disco_diffdock_amd import build
    build.build(verbose=False)
    return gen.digests(torch.device('cuda:0'))


@pytest.fixture(scope='module')
def want():
    with open(os.path.join(GOLDEN, 'node_stage_bits.json')) as f:
        return json.load(f)['sha256']


def test_every_output_is_pinned(got, want):
    assert sorted(got) == sorted(want) == sorted(gen.CASES)


@pytest.mark.parametrize('case', gen.CASES)
def test_bits(got, want, case):
    assert case in got and case in want, case
    print(case, got[case], want[case])
    assert got[case] == want[case]
