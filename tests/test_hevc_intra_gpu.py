"""H.265 intra prediction on the GPU (-m gpu): every case of tests/analytic_hevc_intra.py through the C ABI with codec 1, I420 and NV12, against the
expectation that tests/hevc_intra_ref.py computes from clause 8.4.4.2 -- not against the oracle.  k_hevc_intra and HevcPicParser::emit_intra_tb wrong
in the way the oracle and the generator are wrong pass the parity tests; they do not pass these.  tests/test_hevc_intra_host.py holds the CPU oracle
to the same expectation and asserts what the cases cover."""
import pytest

import hevc_intra_ref as ir
from test_analytic_gpu import decode
from test_hevc_intra_host import NAMES, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decodes_the_hevc_intra_expectation(name, fmt):
    seq, pics, data, planes, records = case(name)
    frames, _ = decode(data, fmt, codec=1)
    diff = ir.difference(seq, pics, frames, fmt, planes, records)
    assert diff is None, f"{name} format {fmt}: {diff}"
