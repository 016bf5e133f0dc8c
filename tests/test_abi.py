"""The drop-in boundary: the library loads, exports every symbol include/jm_amd_dec.h declares plus the ten
C++-mangled jm_nvdec_* names of the reference header, and the reference's own harness links against it."""
import os
import re
import subprocess

import pytest

from jmcodec_amd import api
from util import ROOT

MANGLED = ["_Z22jm_nvdec_create_handlev", "_Z13jm_nvdec_initiiPciPv", "_Z15jm_nvdec_deinitPv", "_Z21jm_nvdec_decode_framePhiPiPv",
           "_Z21jm_nvdec_output_framePhPiPv", "_Z20jm_nvdec_stream_infoPiS_Pv", "_Z16jm_nvdec_set_eofbPv", "_Z16jm_nvdec_is_exitPv",
           "_Z22jm_nvdec_show_dec_infoPv", "_Z22jm_nvdec_is_hw_supportv"]


def _exports():
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.lib_path()], text=True)
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "jm_amd_dec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(jm_amddec_\w+)\s*\(", hdr))
    assert len(declared) >= 14
    exp = _exports()
    assert declared <= exp, declared - exp
    assert set(MANGLED) <= exp, set(MANGLED) - exp
    L = api.lib()
    for name in declared:
        assert getattr(L, name)


def test_no_gpu_means_loud_failure_not_fallback():
    """Without a HIP device init must fail (the reference would return 0); nothing decodes on the CPU."""
    if api.jm_nvdec_is_hw_support():
        pytest.skip("a GPU is present")
    h = api.jm_nvdec_create_handle()
    assert api.jm_nvdec_init(0, 1, None, 0, h) != 0
    assert b"no HIP device" in api.lib().jm_amddec_last_error(h)
    assert api.jm_nvdec_decode_frame(b"\x00\x00\x01\x09\x10", 5, h)[0] != 0
    api.jm_nvdec_deinit(h)


def test_product_does_not_link_the_oracle():
    out = subprocess.check_output(["nm", "-D", api.lib_path()], text=True)
    assert "orc_" not in out
    for f in os.listdir(os.path.join(ROOT, "jmcodec_amd", "csrc")):
        src = open(os.path.join(ROOT, "jmcodec_amd", "csrc", f)).read()
        assert "oracle/" not in src and "orc_h264" not in src, f


def _ref_binary(name):
    """A reference harness that build() compiled in place against this library into oracle/_ref/ (oracle/Makefile `ref`; the sources are never
    copied into the repository)."""
    exe = os.path.join(ROOT, "oracle", "_ref", name)
    assert os.path.exists(exe), f"oracle/_ref/{name} is missing: build() makes it with `make -C oracle ref`"
    return exe


def test_reference_harness_links_against_the_library():
    """The reference's test_nv_dec.cpp, built with a two-file shim for <Windows.h>/<conio.h> and linked against libjm_amd_dec.so: every jm_nvdec_*
    symbol it uses is one the library exports."""
    und = subprocess.check_output(["nm", "-u", _ref_binary("test_nv_dec")], text=True)
    used = set(re.findall(r"_Z\d+jm_nvdec_\w+", und))
    assert len(used) == 8 and used <= set(MANGLED)
    assert used <= _exports(), used - _exports()


# ---- push/pull API of intel_dec/jm_intel_dec.h ----
INTEL_MANGLED = ["_Z26jm_intel_dec_create_handlev", "_Z17jm_intel_dec_initiiPv", "_Z19jm_intel_dec_deinitPv",
                 "_Z29jm_intel_dec_set_yuv_callbackPvPFiPhiS_ES_", "_Z23jm_intel_dec_input_dataPhiPv", "_Z25jm_intel_dec_output_framePhPiPv",
                 "_Z20jm_intel_dec_set_eofiPv", "_Z17jm_intel_dec_infoPv", "_Z24jm_intel_get_stream_infoPiS_PfPv",
                 "_Z27jm_intel_dec_need_more_dataPv", "_Z25jm_intel_dec_free_buf_lenPv", "_Z20jm_intel_dec_is_exitPv", "_Z22jm_intel_is_hw_supportv"]


def test_intel_api_symbols():
    hdr = open(os.path.join(ROOT, "include", "jm_amd_intel_dec.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(jm_amdintel_\w+)\s*\(", hdr))
    assert len(declared) == 15         # the reference's 13 + jm_amdintel_run_pushpull + jm_amdintel_decoder (additions, no reference counterpart)
    exp = _exports()
    assert declared <= exp, declared - exp
    assert set(INTEL_MANGLED) <= exp, set(INTEL_MANGLED) - exp


def test_reference_intel_harness_links_against_the_library(tmp_path):
    """The reference's test_intel_dec.cpp, built the same way, links against the library and runs its own loop on the host."""
    exe = _ref_binary("test_intel_dec")
    und = subprocess.check_output(["nm", "-u", exe], text=True)
    used = set(re.findall(r"_Z\d+jm_intel_\w+", und))
    assert len(used) >= 9 and used <= set(INTEL_MANGLED), used - set(INTEL_MANGLED)
    assert used <= _exports(), used - _exports()
    # host-side run of the reference's own loop (parse-only: no kernels): it must terminate and report the frame count
    from util import golden_stream
    src = tmp_path / "in.h264"
    src.write_bytes(golden_stream("ip_fuzz_96x80"))
    env = dict(os.environ, JM_AMD_DEC_PARSE_ONLY="1")
    # (the harness opens its hard-coded output name in the cwd)
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, env=env, timeout=60, cwd=str(tmp_path))
    assert "Frame Count:\t8" in r.stdout, r.stdout + r.stderr


def _harness():
    return os.path.join(ROOT, "tools", "_build", "test_amd_dec")


def test_native_harness_fails_loudly_without_a_gpu(tmp_path):
    """tools/test_amd_dec (the test_nv_dec counterpart) links the drop-in jm_nvdec_* symbols; with no HIP device it must
    refuse (exit 3) instead of decoding on the CPU."""
    import jmcodec_amd
    if jmcodec_amd.jm_nvdec_is_hw_support():
        pytest.skip("a GPU is present")
    from tools import streams
    p = tmp_path / "s.h264"
    p.write_bytes(streams.generate(width=96, height=80, frames=4, gop=4))
    r = subprocess.run([_harness(), str(p)], capture_output=True, text=True)
    assert r.returncode == 3 and "no HIP device" in r.stderr


def test_native_harness_loop_in_parse_only_mode(tmp_path):
    """The harness's sliding-window NAL loop (small window, multi-loop) drives the library's host stages correctly: frame count and
    the reference's info block format (nv_dec.cpp:666-680)."""
    from tools import streams
    p = tmp_path / "s.h264"
    p.write_bytes(streams.generate(width=96, height=80, frames=5, gop=5, num_ref=2, mode=1))
    env = dict(os.environ, JM_AMD_DEC_PARSE_ONLY="1")
    for extra, frames in ((["--chunk", "64"], 5), (["--loops", "3"], 15), ([], 5)):
        r = subprocess.run([_harness(), str(p), "--no-hw-check"] + extra, capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert f"Frame Count:\t{frames}\n" in r.stdout and "Display:\t96 x 80\n" in r.stdout and "Pixel Format:\tYV12\n" in r.stdout
        assert f"frames fetched = {frames} " in r.stdout
