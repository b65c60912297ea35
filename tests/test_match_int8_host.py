"""int8 selection of the gallery match, host side: the ISA of the shipped build flags (csrc/build.sh) must contain the int8 filter GEMM
instantiations on v_mfma_i32_32x32x32_i8, with no private segment and no scratch instruction (the filter's counted waits and its register
budget — 16 extra gallery scales per lane in the epilogue — leave no room for a spill)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pets-face-recognition_amd", "csrc")


@pytest.fixture(scope="module")
def igemm_isa(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    flags = re.search(r'^FLAGS="([^"]*)"', open(os.path.join(CSRC, "build.sh")).read(), re.M).group(1)
    flags = flags.replace("$ARCH", "gfx950").replace("${PFR_EXTRA_FLAGS}", "").split()
    out = tmp_path_factory.mktemp("isa") / "pfr_igemm.s"
    subprocess.run(["hipcc", *flags, "--cuda-device-only", "-S", os.path.join(CSRC, "pfr_igemm.hip"), "-o", str(out)], check=True,
                   stderr=subprocess.DEVNULL)
    return out.read_text()


def _bodies(text, pattern):
    """{mangled kernel name: its instruction text} for the kernels whose name matches `pattern`"""
    out = {}
    for m in re.finditer(r"^(?P<n>" + pattern + r"):.*?$(?P<b>.*?)^\s+\.size\s+(?P=n),", text, re.M | re.S):
        out[m.group("n")] = m.group("b")
    return out


# igemm_kernel<int8_t (a), float (f), BQ, BP, PRO=0, FAST=1, KCH=8, NW, WP=2, NST=2, FILT, BNB=0, EPRE=0>
I8_FILT = r"_Z12igemm_kernelIafLi(\d+)ELi(\d+)ELb0ELb1ELi8ELi(\d)ELi2ELi2ELb1ELb0ELb0EEv11IgemmParams"
I8_TILE = r"_Z12igemm_kernelIafLi128ELi128ELb0ELb1ELi8ELi4ELi2ELi2ELb0ELb0ELb0EEv11IgemmParams"


def test_int8_filter_kernels_exist_use_i8_mfma_and_no_scratch(igemm_isa):
    filt = _bodies(igemm_isa, I8_FILT)
    geoms = sorted((re.match(I8_FILT, n).groups()) for n in filt)
    # the bf16 geometries: 256x256 with 8 waves, 128x128 with 4
    assert geoms == [("128", "128", "4"), ("256", "256", "8")], geoms
    tile = _bodies(igemm_isa, I8_TILE)
    assert len(tile) == 1, "the materialised int8 score chunk (pfr_match_scores_i8) is not instantiated"
    for name, body in {**filt, **tile}.items():
        assert "v_mfma_i32_32x32x32_i8" in body, name
        assert "v_mfma_f32_32x32x16_bf16" not in body, name
        assert not re.search(r"^\s+scratch_", body, re.M), name
    seg = dict(re.findall(r"\.name:\s+(_Z12igemm_kernelIaf\S+)\s+\.private_segment_fixed_size:\s+(\d+)", igemm_isa))
    assert set(seg) == set(filt) | set(tile), seg
    assert all(int(v) == 0 for v in seg.values()), seg
