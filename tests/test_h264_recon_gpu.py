"""H.264 intra prediction and residual reconstruction on the GPU (-m gpu), bit for bit against the restated clauses (tests/h264_recon_ref.py through
tests/analytic_expect.py) -- not against the oracle.  The scripted cases of tests/analytic_h264_recon.py go through mb_residual_to_lds (every
reconstruction kernel), intra_luma_mb (k_intra_band, the intra role of k_chain_i), k_recon_intra and the packed Intra8x8 routine; a kernel that is wrong
in the same way as the oracle passes the parity tests, it does not pass these.  tests/test_h264_recon_host.py checks the expectations themselves.

There are no tolerances: the expected pictures are integers from the clauses."""
import pytest

import analytic_expect as ae
import analytic_h264_recon as hr
from jmcodec_amd import api
from test_analytic_gpu import decode
from test_gpu_parity import _chains_must_have_formed, _wait_until_the_gpu_is_ours

pytestmark = pytest.mark.gpu

# every case at 96x80 (6 x 5 macroblocks: wider than the ring of four macroblock bottoms); the intra-only cases also at 48x288 (18 macroblock rows: two
# bands of kIBandRows = 16) and at 16x48 (one macroblock wide: mb_w_magic == 0); p_intra_islands also at 128x128, where three islands stay below 1/16
CASES = [(n, s) for n in sorted(hr.CASES) for s in hr.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_gpu_decodes_the_restated_expectation(name, size, fmt):
    seq, pics, data, planes, _ = hr.scripted(name, size)
    frames, _ = decode(data, fmt)
    diff = ae.first_difference(seq, pics, frames, fmt, planes)
    assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", hr.P_CASES)
def test_sparse_intra_takes_the_spin_wait_kernel_and_dense_intra_the_band_kernel(name):
    """decoder.cpp:1970 sends a picture to k_intra_band when at least 1/16 of its macroblocks are intra (I_PCM not counted) and to k_recon_intra when
    fewer are.  No counter tells the two apart (class `intra` counts both), so the selecting condition is asserted from the script, picture by picture,
    and the decoder's own count of intra macroblocks is held to the script's: with both, each P picture of p_intra_islands* ran k_recon_intra and each
    of p_intra_dense* ran k_intra_band (inter macroblocks publish their right column and bottom row to the intra neighbours there)."""
    for size in hr.case_sizes(name):
        seq, pics, data, planes, _ = hr.scripted(name, size)
        counts = hr.intra_counts(seq, pics)
        for n_intra, n_mbs in counts[1:]:
            assert n_intra > 0 and ((n_intra * 16 >= n_mbs) if "dense" in name else (n_intra * 16 < n_mbs)), (name, size, n_intra, n_mbs)
        with api.JmAmdDec(0, 1) as d:
            before = d.stat("intra_mbs")
            frames = d.decode_stream(data)
            assert d.stat("errors") == 0 and d.stat("device_wait_errors") == 0
            assert d.stat("intra_mbs") - before == sum(n for n, _ in counts)
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} {size}: {diff}"


@pytest.mark.parametrize("name", hr.ROUTE_CASES)
def test_chain_launches_decode_the_cases_with_deblocking_on(name):
    """The cases with the deblocking filter on in every picture (tests/deblock_ref.py filters the expectation: bS from the coded blocks of the script,
    no inner 4x4 edges under the 8x8 transform, each chroma plane with its own QP offset), all pictures fed in one call, chain depth 1 (the stage
    kernels: k_intra_band / k_recon_intra, k_deblock_band) and 8 (k_chain_i, whose intra role is intra_luma_mb): both equal the expectation.  On a GPU
    the engine owns, depth 8 must have run k_chain_i; on a shared one the comparison ran on the stage kernels only: a visible skip."""
    seq, pics, data, planes, _ = hr.scripted_deblocked(name)
    ours = _wait_until_the_gpu_is_ours()
    for depth in (1, 8):
        with api.JmAmdDec(0, 1) as d:
            before = d.stat("eng_chain_i_batches")                  # the engine and its counters are the process's, not the handle's
        frames, chained = decode(None, 1, chunks=[data], chain_depth=depth, chain_lag=24)
        with api.JmAmdDec(0, 1) as d:
            with_intra = d.stat("eng_chain_i_batches") - before
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} chain depth {depth}: {diff}"
        assert (chained == 0 and with_intra == 0) or depth > 1, (name, depth, chained, with_intra)
        assert (chained > 0 and with_intra > 0) or depth == 1 or not ours, f"{name}: depth {depth}: no picture ran inside k_chain_i on a GPU the engine owns"
    _chains_must_have_formed(ours, name)


def test_tall_intra4x4_picture_through_the_spin_wait_kernel():
    """16x8208 (513 macroblock rows): above 512 rows k_recon_intra predicts every macroblock -- here Intra4x4 with levels in every block (the tall
    stream of tests/test_analytic_gpu.py has Intra16x16 without levels)."""
    seq, pics, data, planes = hr.tall_intra_script()
    frames, chained = decode(data, 1)
    diff = ae.first_difference(seq, pics, frames, 1, planes)
    assert diff is None, diff
    assert chained == 0
