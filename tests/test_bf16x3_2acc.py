"""The bf16x3_2acc precision (ASR_CONV16_BF16X3_2ACC = 4) without a GPU: the constant in the header and in Python, the
export, the register / LDS budget of its bench instances read from the built object, and the refusal of unknown
precision names by the user surfaces before any GPU work."""
import os
import re
import subprocess
import sys

import pytest

from asr_hip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "csrc", "asr_conv16.o")
TOOL = os.path.join(REPO, "adaptive-surface-reconstruction_amd", "asrtool.py")
sys.path.insert(0, os.path.join(REPO, "scripts"))

# k_sconv_plan16<NT, KC, WAVES, MODE = 4, IMP, DUAL, SPLIT> instances of the bench shapes (tests/sconv_instances.py
# BENCH_SHAPES16 and BENCH_SPLIT16 with MODE 4): VGPR + AGPR per lane, LDS bytes and workgroups per CU as built
# (bf16x3 in brackets where it differs: DESIGN 4.3)
REPORTED = {
    "k_sconv_plan16<8, 32, 8, 4, false, false, false>": (114, 49216, 2),  # (80, 3)
    "k_sconv_plan16<8, 32, 8, 4, false, false, true>": (114, 49216, 2),   # (80, 3)
    "k_sconv_plan16<8, 32, 8, 4, false, true, false>": (121, 65536, 2),   # (108)
    "k_sconv_plan16<4, 32, 8, 4, false, false, false>": (80, 40960, 3),   # (62, 4)
    "k_sconv_plan16<4, 32, 8, 4, false, true, false>": (87, 40960, 2),    # (92)
    "k_sconv_plan16<2, 32, 8, 4, false, false, false>": (62, 28672, 4),   # (54)
    "k_sconv_plan16<8, 32, 4, 4, false, false, false>": (204, 49184, 2),  # (124, 3)
    "k_sconv_plan16<8, 32, 4, 4, false, true, false>": (220, 49184, 2),   # (160, 3)
    "k_sconv_plan16<2, 32, 4, 4, false, true, false>": (102, 20512, 4),   # (97)
}


def _blocks_per_cu(regs, lds, waves):
    """workgroups of `waves` waves one CU holds: 512 registers per SIMD lane in granules of 8, 8 waves per SIMD, 160 KB of LDS"""
    per_simd = min(8, 512 // ((regs + 7) // 8 * 8)) if regs else 8
    return min(per_simd * 4 // waves, 160 * 1024 // max(lds, 1))


def _bench_instances():
    from sconv_instances import BENCH_SHAPES16, BENCH_SPLIT16
    b = lambda v: "true" if v else "false"  # noqa: E731
    out = {"k_sconv_plan16<%d, %d, %d, 4, %s, %s, false>" % (nt, kc, w, b(imp), b(dual))
           for nt, kc, imp, w, dual in BENCH_SHAPES16}
    out |= {"k_sconv_plan16<%d, %d, %d, 4, %s, %s, true>" % (nt, kc, w, b(imp), b(dual)) for nt, kc, imp, w, dual in BENCH_SPLIT16}
    return out


def test_mode_constant_in_header_and_python():
    text = open(os.path.join(REPO, "include", "asr_hip.h")).read()
    assert re.search(r"^#define ASR_CONV16_BF16X3_2ACC 4$", text, re.M)
    assert _lib.CONV16_BF16X3_2ACC == 4 and _lib.PRECISIONS["bf16x3_2acc"] == 4
    # the four other precisions keep their numbers
    assert {k: v for k, v in _lib.PRECISIONS.items() if k != "bf16x3_2acc"} == {"f32": 0, "f16": 1, "bf16x3": 2, "f16x2": 3}


def test_library_exports_the_entry_point():
    lib = _lib.load()
    assert hasattr(lib, "asr_hip_sparse_conv_bf16x3_2acc")
    assert "asr_hip_sparse_conv_bf16x3_2acc" in _lib.EXPORTS
    # packing: the same size as bf16x3 (three bf16 planes), an unknown mode is refused
    f = lib.asr_hip_sparse_conv_packed_bytes
    for shape in ((55, 128, 120, 8), (55, 64, 64, 0), (9, 256, 256, 0)):
        assert f(4, *shape) == f(2, *shape) > 0
    assert f(5, 55, 64, 64, 0) == 0


@pytest.mark.skipif(not os.path.exists(OBJ), reason="asr_conv16.o has not been built")
def test_bench_instances_register_and_lds_budget():
    """every bench instance in the new mode: no spill, no scratch; the 8-wave ones within 128 VGPR + AGPR (two blocks per CU)
    and none below the blocks per CU reported above"""
    import kernel_regs
    ks = {k["demangled"]: k for k in kernel_regs.kernels(OBJ)}
    assert set(REPORTED) == _bench_instances()
    for name, (regs_rep, lds_rep, blocks_rep) in REPORTED.items():
        k = ks[name]
        waves = int(name.split(", ")[2])
        regs = k.get("vgpr_count", 0) + k.get("agpr_count", 0)
        lds = k.get("group_segment_fixed_size", 0)
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (name, k)
        if waves == 8:
            assert regs <= 128, (name, regs)
        assert regs <= regs_rep and lds <= lds_rep, (name, regs, lds)
        assert _blocks_per_cu(regs, lds, waves) >= blocks_rep, (name, regs, lds)


def test_reconstruct_surface_refuses_an_unknown_precision():
    import numpy as np
    import adaptivesurfacereconstruction as asr
    pts = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError, match="precision"):
        asr.reconstruct_surface(pts, pts, precision="nope")


def test_asrtool_precision_option(tmp_path):
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "in.ply"), "--out", str(tmp_path / "out.ply"),
                        "--precision", "nope"], capture_output=True, text=True)
    assert r.returncode == 1 and "precision" in r.stderr and "bf16x3_2acc" in r.stderr
    assert not os.path.exists(tmp_path / "out.ply")
    sys.path.insert(0, os.path.dirname(TOOL))
    import asrtool
    assert asrtool.HELP.startswith("usage: asrtool --in point_cloud.ply --out mesh.ply")
    assert "--precision" in asrtool.HELP
