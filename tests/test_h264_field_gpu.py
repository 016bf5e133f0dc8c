"""H.264 field pictures on the GPU (-m gpu), bit for bit against the restated clauses (tests/h264_field_ref.py through tests/analytic_expect.py) -- never
against the oracle.  The scripted cases of tests/analytic_h264_field.py go through k_recon_inter<*, FIELD = true> (doubled pitch, parity offset, the
reference byte's parity bit, the Table 8-9 offset, the window clamped at the field's border), the field rules of boundary_strength, k_intra_band,
k_recon_intra and k_deblock_band on pictures of half the rows, and k_packout's lone_field path.  A kernel that is wrong in the same way as the oracle
passes the parity tests; it does not pass these.  tests/test_h264_field_host.py checks the expectations themselves.

There are no tolerances: the expected pictures are integers from the clauses."""
import threading

import pytest

import analytic_expect as ae
import analytic_h264_field as hf
import analytic_h264_recon as hr
import h264_field_ref as fr
from jmcodec_amd import api
from test_analytic_gpu import decode, scripted as progressive
from test_gpu_parity import _wait_until_the_gpu_is_ours

pytestmark = pytest.mark.gpu

# every case at 96x160 (6 x 5 field macroblocks); the intra, border and deblocking cases also at 16x96 (one macroblock wide) and 48x544 (17 field rows:
# two bands of kIBandRows / kBandRows = 16)
CASES = [(n, s) for n in sorted(hf.CASES) for s in hf.case_sizes(n)]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_gpu_decodes_the_restated_expectation(name, size, fmt):
    seq, pics, data, planes, _, _ = hf.scripted(name, size)
    frames, chained = decode(data, fmt)
    diff = ae.first_difference(seq, pics, frames, fmt, planes)
    assert diff is None, f"{name} {size} format {fmt}: {diff}"
    assert chained == 0, "field pictures never chain (and a picture fed alone has nothing to chain with)"


@pytest.mark.parametrize("name", ["field_intra", "paff_mixed", "paff_mixed_sparse"])
def test_field_pictures_through_both_intra_kernels(name):
    """decoder.cpp sends a picture to k_intra_band when at least 1 / 16 of its macroblocks are intra (I_PCM not counted) and to k_recon_intra when fewer
    are; no counter tells the two apart, so the selecting condition is asserted from the script and the decoder's own counts are held to it: every
    field of field_intra and every P picture of paff_mixed ran k_intra_band, every P picture of paff_mixed_sparse k_recon_intra -- fields of half the
    rows at twice the pitch among them."""
    for size in hf.case_sizes(name):
        seq, pics, data, planes, _, _ = hf.scripted(name, size)
        counts = hr.intra_counts(seq, pics)
        for p, (n_intra, n_mbs) in zip(pics, counts):
            if n_intra:
                assert (n_intra * 16 < n_mbs) == (name == "paff_mixed_sparse"), (name, size, n_intra, n_mbs)
        assert sum(1 for n_intra, _ in counts if n_intra) >= 5
        with api.JmAmdDec(0, 1) as d:
            before = d.stat("intra_mbs"), d.stat("field_pictures")
            frames = d.decode_stream(data)
            assert d.stat("errors") == 0 and d.stat("device_wait_errors") == 0
            assert d.stat("intra_mbs") - before[0] == sum(n for n, _ in counts)
            assert d.stat("field_pictures") - before[1] == fr.counts(pics)[0]
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} {size}: {diff}"


@pytest.mark.parametrize("name", ["paff_mixed", "paff_mixed_sparse"])
def test_chain_depth_8_leaves_the_fields_of_a_mixed_stream_alone(name):
    """Frame pictures and field pairs with the deblocking filter on, all pictures fed in one call, chain depth 1 and 8: both equal the expectation
    (tests/test_h264_field_host.py holds this variant to the oracle too).  The three frame pictures may chain; the four fields must not."""
    seq, pics, data, planes, _ = hf.scripted_deblocked(name)
    _wait_until_the_gpu_is_ours()
    for depth in (1, 8):
        frames, chained = decode(None, 1, chunks=[data], chain_depth=depth, chain_lag=24)
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} chain depth {depth}: {diff}"
        assert chained <= sum(1 for p in pics if not p.get("field")) and (depth > 1 or chained == 0), (name, depth, chained)


def test_field_streams_beside_progressive_known_answer_streams():
    """Field streams and progressive scripted streams decoded by handles in parallel: a batch that holds a field picture sends its frame pictures through
    k_recon_inter<*, FIELD = true> too (engine.cpp), and this is what puts a known-answer FRAME picture through that instantiation.  Each stream
    equals its own expectation."""
    jobs = [(hf.scripted(n)[:4], n) for n in ("field_p_parities", "field_b", "paff_mixed", "field_p_borders")]
    jobs += [(progressive(n, (96, 80)), n) for n in ("fractional_positions_noise", "bipred_default", "fractional_positions_noise", "bipred_default")]
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


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name", ["field_lone_top", "field_lone_bottom"])
def test_lone_field_goes_out_with_its_lines_repeated(name, fmt):
    """k_packout's lone_field path: the last frame is the lone field's lines, each twice (this decoder's convention)"""
    seq, pics, data, planes, _, _ = hf.scripted(name)
    with api.JmAmdDec(0, fmt) as d:
        before = d.stat("lone_fields")
        frames = d.decode_stream(data)
        assert d.stat("errors") == 0 and d.stat("lone_fields") - before == 0        # (the counter is for a field that a following picture leaves alone)
    assert len(frames) == 2 and fr.counts(pics) == (3, 1)
    diff = ae.first_difference(seq, pics, frames, fmt, planes)
    assert diff is None, f"{name} format {fmt}: {diff}"
