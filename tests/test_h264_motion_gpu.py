"""H.264 motion vector derivation and direct prediction on the GPU (-m gpu), bit for bit against the restated clauses (tests/h264_motion_ref.py through
tests/analytic_expect.py) -- never against the oracle.  The scripted cases of tests/analytic_h264_motion.py put the host's derivation (h264_cavlc.cpp:
nb, predict, skip_mb, direct_pred, col_block, write_motion) and the job format it decides (per-4x4 vectors, per-quadrant references and lists)
in front of k_recon_inter: the per-4x4 vector fetch of P pictures, the fast / literal decision of B pictures and the window test of P pictures exactly
at and one sample past each border of the coded picture, bi-prediction whose lists differ per quadrant (a quadrant with only list 1 among them) under
default, implicit and explicit weights.  tests/test_h264_motion_host.py checks the expectations themselves.

There are no tolerances: the expected pictures are integers from the clauses."""
import threading

import pytest

import analytic_expect as ae
import analytic_h264_motion as hm
from test_analytic_gpu import decode, scripted as progressive
from test_gpu_parity import _chains_must_have_formed, _wait_until_the_gpu_is_ours

pytestmark = pytest.mark.gpu

CASES = [(n, s) for n in sorted(hm.CASES) for s in hm.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_gpu_decodes_the_restated_expectation(name, size, fmt):
    seq, pics, data, planes, _, _ = hm.scripted(name, size)
    frames, _ = decode(data, fmt)
    diff = ae.first_difference(seq, pics, frames, fmt, planes)
    assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ["reach_chain", "p_partitions"])
def test_chain_launches_wait_for_what_the_derived_vectors_reach(name):
    """The deblocking filter on in every picture, all pictures fed in one call, chain depth 1 (stage kernels) and 8 (chain launches): both equal the
    expectation.  In reach_chain how far a picture reaches into the one before is decided by ONE 4x4 sub-partition inside a macroblock (the host
    test asserts it); a launch that spaced the pictures by the corner blocks' vectors would read samples the filter has not finished.  Chains really
    formed on a GPU the engine owns, else a visible skip."""
    seq, pics, data, planes = hm.scripted_deblocked(name)
    ours = _wait_until_the_gpu_is_ours()
    for depth in (1, 8):
        frames, chained = decode(None, 1, chunks=[data], chain_depth=depth, chain_lag=24)
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} chain depth {depth}: {diff}"
        assert chained == 0 or depth > 1, (name, depth, chained)
        assert chained > 0 or depth == 1 or not ours, f"{name}: depth {depth}: no picture ran inside a chain launch on a GPU the engine owns"
    _chains_must_have_formed(ours, name)


def test_motion_streams_beside_progressive_known_answer_streams():
    """b_partitions and b_spatial_direct decoded by four handles in parallel threads, beside two progressive known-answer streams: each equals its
    own expectation"""
    jobs = [(hm.scripted(n)[:4], n) for n in ("b_partitions", "b_spatial_direct", "b_partitions_implicit", "b_spatial_direct_no_inference")]
    jobs += [(progressive(n, (96, 80)), n) for n in ("fractional_positions_noise", "bipred_default")]
    got = [None] * len(jobs)

    def run(i):
        got[i] = decode(jobs[i][0][2], 1)[0]
    for _ in range(2):
        ts = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
        [t.start() for t in ts]
        [t.join() for t in ts]
        for ((seq, pics, data, planes), name), frames in zip(jobs, got):
            diff = ae.first_difference(seq, pics, frames, 1, planes)
            assert diff is None, f"{name}: {diff}"
