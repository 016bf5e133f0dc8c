"""Analytic known-answer streams on the GPU (-m gpu): every scripted stream of tests/analytic_cases.py through the C ABI, I420 and NV12, against the
ANALYTIC expectation of tests/analytic_expect.py -- not the oracle's output.  A kernel that is wrong in the same way as the oracle passes the parity
tests; it does not pass these.  tests/test_analytic_host.py checks the expectations themselves (closed forms, restatements, the CPU oracle)."""
import functools

import numpy as np
import pytest

import analytic_cases as ac
import analytic_expect as ae
import analytic_hevc as ah
import scripted_h264 as sw
import scripted_hevc as hw
from jmcodec_amd import api
from test_gpu_parity import _chains_must_have_formed, _wait_until_the_gpu_is_ours

pytestmark = pytest.mark.gpu

CASES = [(n, s) for n in sorted(ac.H264_CASES) for s in ac.case_sizes(n)]     # the deblock_filters_* cases also at 48x288: two deblocking bands
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]


def decode(data, fmt, chunks=None, codec=0, **opts):
    with api.JmAmdDec(codec, fmt) as d:
        for k, v in opts.items():
            assert api.lib().jm_amddec_set_option(d.h, k.encode(), v) == 0
        before = d.stat("eng_chain_pics")
        frames = d.decode_stream(data, chunks=chunks)
        assert d.stat("errors") == 0 and d.stat("device_wait_errors") == 0
        chained = d.stat("eng_chain_pics") - before
        for k in opts:
            api.lib().jm_amddec_set_option(d.h, k.encode(), 0 if k == "chain_depth" else 24)     # the engine's settings outlive the handle: defaults again
        return frames, chained


@functools.lru_cache(maxsize=None)
def scripted(name, size):
    """(seq, pics, stream, expected planes) of a case: computed once for both output formats and for the chain test, never modified"""
    seq, pics = ac.H264_CASES[name](*size)
    return seq, pics, sw.write(seq, pics), ae.expect_h264(seq, pics)


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_gpu_decodes_the_analytic_expectation(name, size, fmt):
    seq, pics, data, planes = scripted(name, size)
    frames, _ = decode(data, fmt)
    diff = ae.first_difference(seq, pics, frames, fmt, planes)
    assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("name", ac.H264_INTER_CASES)
def test_chain_launches_decode_the_analytic_expectation(name):
    """The inter cases with the filter on at a QP where it must be the identity (analytic_cases.with_filter_on), all pictures fed in one call, chain
    depth 1 (stage kernels) and 8 (k_chain): both equal the analytic expectation; chains really formed on a GPU the engine owns, else a visible skip."""
    seq, pics = ac.H264_CASES[name](96, 80)
    pics = ac.with_filter_on(pics)
    data = sw.write(seq, pics)
    planes = ae.expect_h264(seq, pics)
    ours = _wait_until_the_gpu_is_ours()
    for depth in (1, 8):
        frames, chained = decode(None, 1, chunks=[data], chain_depth=depth, chain_lag=24)
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} chain depth {depth}: {diff}"
        assert chained == 0 or depth > 1, (name, depth, chained)
        assert chained > 0 or depth == 1 or not ours, f"{name}: depth {depth}: no picture ran inside a chain launch on a GPU the engine owns"
    _chains_must_have_formed(ours, name)


@pytest.mark.parametrize("name", ac.H264_FILTER_CASES)
def test_chain_launches_decode_the_filtering_cases(name):
    """The deblock_filters_* cases AS SCRIPTED -- the filter changes most macroblocks of every picture (tests/deblock_ref.py) -- all pictures fed in one
    call, chain depth 1 (k_deblock_band) and 8 (the deblocking role of k_chain, write-through stores): both equal the analytic expectation.  With the
    identity filter of the test above, a reconstruction group of k_chain that read its reference window before the deblocking band had made those
    samples final read the same bytes either way; here it does not (deblock_filters_refs: the host test shows that every P picture differs from what
    the unfiltered reference gives).  Chains really formed on a GPU the engine owns, else a visible skip."""
    seq, pics, data, planes = scripted(name, (96, 80))
    ours = _wait_until_the_gpu_is_ours()
    for depth in (1, 8):
        frames, chained = decode(None, 1, chunks=[data], chain_depth=depth, chain_lag=24)
        diff = ae.first_difference(seq, pics, frames, 1, planes)
        assert diff is None, f"{name} chain depth {depth}: {diff}"
        assert chained == 0 or depth > 1, (name, depth, chained)
        assert chained > 0 or depth == 1 or not ours, f"{name}: depth {depth}: no picture ran inside a chain launch on a GPU the engine owns"
    _chains_must_have_formed(ours, name)


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
def test_full_hd_rows_decode_the_analytic_expectation(fmt):
    """1920x1080, one slice per macroblock row, a vector per row over noise: the band / multi-workgroup paths against the vectorised restatement."""
    seq, pics = ac.full_hd_rows()
    frames, _ = decode(sw.write(seq, pics), fmt)
    diff = ae.first_difference(seq, pics, frames, fmt)
    assert diff is None, diff


def test_255_slices_decode_exactly_and_256_fail_the_handle():
    """The slice limit of the job list on the device: 272x240 with one slice per macroblock (255 slices) decodes exactly; the 256th slice of a picture
    (256x256) fails the handle with the text that names the limit before any kernel of that picture is launched
    (tests/test_analytic_host.py shows the same on a parse_only handle)."""
    from test_analytic_host import one_slice_per_mb_stream
    seq, pics = one_slice_per_mb_stream(272, 240)
    frames, _ = decode(sw.write(seq, pics), 1)
    diff = ae.first_difference(seq, pics, frames, 1)
    assert diff is None, diff
    seq, pics = one_slice_per_mb_stream(256, 256)
    with api.JmAmdDec(0, 1) as d:
        with pytest.raises(RuntimeError, match="255 slices"):
            d.decode_stream(sw.write(seq, pics))
        assert d.stat("errors") >= 1 and "255 slices" in api.lib().jm_amddec_last_error(d.h).decode()


def test_tall_picture_through_the_spin_wait_kernels():
    """16x8208 (1 x 513 macroblocks): above 512 macroblock rows the decoder launches k_deblock and, for the Intra16x16 macroblocks, k_recon_intra -- the
    kernels with a progress word per macroblock row in LDS (kMaxMbRows, kernels.h); rows 512 and up used to index past that array.  Against the numpy
    expectation (tests/deblock_ref.py); tests/test_analytic_host.py holds the CPU oracle to the same script."""
    from test_analytic_host import tall_script
    seq, pics, data, planes = tall_script()
    frames, chained = decode(data, 1)
    diff = ae.first_difference(seq, pics, frames, 1, planes)
    assert diff is None, diff
    assert chained == 0


# ---- H.265 -------------------------------------------------------------------------------------------------------------------------------------
HCASES = [(n, s) for n in sorted(ah.HEVC_CASES) for s in ah.SIZES]
HIDS = [f"{n}-{s[0]}x{s[1]}" for n, s in HCASES]


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
@pytest.mark.parametrize("name,size", HCASES, ids=HIDS)
def test_gpu_decodes_the_hevc_analytic_expectation(name, size, fmt):
    seq, pics = ah.HEVC_CASES[name](*size)
    frames, _ = decode(hw.write(seq, pics), fmt, codec=1)
    diff = ae.first_difference(seq, pics, frames, fmt, ah.expect_hevc(seq, pics), "cus")
    assert diff is None, f"{name} {size} format {fmt}: {diff}"


@pytest.mark.parametrize("fmt", [1, 0], ids=["i420", "nv12"])
def test_hevc_full_hd_rows_decode_the_analytic_expectation(fmt):
    """1920x1080, one slice per CTB row, a vector per row over noise, against the vectorised restatement of 8.5.3.3.3."""
    seq, pics = ah.full_hd_rows()
    frames, _ = decode(hw.write(seq, pics), fmt, codec=1)
    diff = ae.first_difference(seq, pics, frames, fmt, ah.expect_hevc(seq, pics), "cus")
    assert diff is None, diff


def test_hevc_272_slice_segments_per_picture_decode_exactly():
    """272x256, one slice per 16x16 CTB: 272 slice segments in a picture (the H.265 path has no 255 limit; tests/test_analytic_host.py pins its own)."""
    seq, pics = ah.one_slice_per_ctb_stream(272, 256)
    frames, _ = decode(hw.write(seq, pics), 1, codec=1)
    diff = ae.first_difference(seq, pics, frames, 1, ah.expect_hevc(seq, pics), "cus")
    assert diff is None, diff
