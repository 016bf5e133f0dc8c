"""H.265 inter prediction on the GPU (-m gpu): every case of tests/analytic_hevc_inter.py through the C ABI with codec 1, I420 and NV12, against the
expectation that tests/hevc_inter_ref.py computes from clauses 6.4.2 and 8.5.3.2.2 - 8.5.3.2.9 and the interpolation of 8.5.3.3.3 -- not against the
oracle.  k_hevc_mc (every tile shape, fraction, window alignment, border, job count) and the host derivation wrong in the way the oracle and the
generator are wrong pass the parity tests; they do not pass these.  tests/test_hevc_inter_host.py holds the CPU oracle and the product's syntax digest
to the same expectation and asserts what the cases cover."""
import pytest

import analytic_hevc_inter as ai
import hevc_inter_ref as hr
from jmcodec_amd import api
from test_analytic_gpu import decode
from test_hevc_inter_host import NAMES, case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_decodes_the_hevc_inter_expectation(name, fmt):
    seq, pics, data, planes, records = case(name)
    frames, _ = decode(data, fmt, codec=1)
    diff = hr.difference(seq, pics, frames, fmt, planes, records)
    assert diff is None, f"{name} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ai.GROUPS["tmvp"])
def test_gpu_decodes_the_temporal_cases_with_pictures_in_flight(name):
    """The whole stream in one call: the parser runs ahead of the device and reads a collocated picture's motion while later pictures are in flight"""
    seq, pics, data, planes, records = case(name)
    frames, _ = decode(None, 1, chunks=[data], codec=1)
    diff = hr.difference(seq, pics, frames, 1, planes, records)
    assert diff is None, f"{name} in one call: {diff}"


def test_the_surface_pitch_equals_the_width_of_the_128_wide_case():
    """inter_borders-128x32 is there for a picture whose rows follow each other without padding: a window that runs over the right edge reads the next
    row's samples unless it is clamped.  (By arithmetic the pitch term of the kernel's `inside` test cannot decide on its own: the coded width is a
    multiple of 8, the pitch a multiple of 128, so a window inside the picture always ends inside the pitch.)"""
    seq, pics, data, planes, records = case("inter_borders-128x32")
    with api.JmAmdDec(1, 1) as d:
        d.decode_stream(data)
        pitch = d.stat("pitch")
    assert pitch == seq["width"] == 128, (f"the surfaces of a {seq['width']}-wide picture now have a pitch of {pitch}: the decode above is still right, but the case no "
                                          "longer has rows without padding -- give inter_borders-128x32 a width that equals the pitch the allocator gives it")
