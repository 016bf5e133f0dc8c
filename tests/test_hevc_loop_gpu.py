"""H.265 deblocking and SAO on the GPU (-m gpu): every case of tests/analytic_hevc_loop.py through the C ABI with codec 1, I420 and NV12, against the
expectation that tests/hevc_loop_ref.py computes from clause 8.7 -- not against the oracle.  k_hevc_bs, k_hevc_deblock and k_hevc_sao (and the
db_flags / nb_mask / qp8 tables the host writes for them) wrong in the way the oracle and the generator are wrong pass the parity tests; they do not pass
these.  tests/test_hevc_loop_host.py holds the CPU oracle and the product's syntax digest to the same expectation and asserts what the cases cover."""
import pytest

import analytic_hevc_loop as al
import hevc_loop_ref as lr
from test_analytic_gpu import decode
from test_hevc_loop_host import NAMES, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decodes_the_hevc_loop_expectation(name, fmt):
    seq, pics, data, planes, records, _ = case(name)
    frames, _ = decode(data, fmt, codec=1)
    diff = lr.difference(seq, pics, frames, fmt, planes, records)
    assert diff is None, f"{name} format {fmt}: {diff}"


@pytest.mark.parametrize("name", al.GROUPS["loop_launch"] + al.GROUPS["loop_reference"])
def test_gpu_decodes_the_launch_and_reference_cases_with_pictures_in_flight(name):
    """The whole stream in one call: pictures with and without the filters share a batch, and a picture predicts from one whose filters are still queued"""
    seq, pics, data, planes, records, _ = case(name)
    frames, _ = decode(None, 1, chunks=[data], codec=1)
    diff = lr.difference(seq, pics, frames, 1, planes, records)
    assert diff is None, f"{name} in one call: {diff}"
