"""The H.265 residual path on the GPU (-m gpu): every case of tests/analytic_hevc_resid.py through the C ABI with codec 1, I420 and NV12, against the
expectation that tests/hevc_resid_ref.py computes from clauses 8.6.1 - 8.6.4.2 -- not against the oracle.  HevcPicParser::residual_coding, residual_block(),
k_hevc_resid, k_hevc_iresid and the add in k_hevc_intra wrong in the way the oracle and the generator are wrong pass the parity tests; they do not pass
these.  tests/test_hevc_resid_host.py holds the CPU oracle to the same expectation and asserts what the cases cover."""
import pytest

import hevc_resid_ref as rr
from test_analytic_gpu import decode
from test_hevc_resid_host import NAMES, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decodes_the_hevc_residual_expectation(name, fmt):
    seq, pics, data, planes, records, _ = case(name)
    frames, _ = decode(data, fmt, codec=1)
    diff = rr.difference(seq, pics, frames, fmt, planes, records)
    assert diff is None, f"{name} format {fmt}: {diff}"
