"""The fp64 tile-centred single layer after its source pre-pass (sctl_amd/csrc/centered_kernel.hpp: fold_prepass_kernel and the FOLD branch of
centered_kernel), read off the device assembly hipcc makes of centered.hip with the Makefile's flags (no GPU needed): the far loops are the ones
tests/test_centred_fold_isa.py holds — 128 fp64 instructions + 16 v_rsq_f64 per 16 pairs at full precision —, every accuracy mode now fits four waves
per SIMD (at most 128 vector registers) without scratch and with 16 waves' LDS per CU, the per-wave classification of densities (an IEEE division)
is gone from the kernel, and the pre-pass kernel uses no scratch."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_loop_counts import count, loops  # noqa: E402

SYM = "_ZN8sctl_amd15centered_kernelINS_11CenteredFxUIdEEdLi%dELi4ELi4EEEvNS_8EvalArgsIT0_EE"   # centered_kernel<CenteredFxU<double>, double, MODE, T = 4, UNR = 4>
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    extra = subprocess.run(["make", "-s", "-C", CSRC, "print-unit-flags", "UNIT=centered"], capture_output=True, text=True, check=True).stdout.split()
    out = str(tmp_path_factory.mktemp("isa") / "centered.s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra + ["--offload-device-only", "-S", os.path.join(CSRC, "centered.hip"), "-o", out],
                   capture_output=True, check=True, timeout=900)
    return open(out).read()


def _meta(src, sym):
    meta = re.search(r"\.amdhsa_kernel " + re.escape(sym) + r"\n(.*?)\.end_amdhsa_kernel", src, re.S).group(1)
    return {k: int(re.search(r"\.amdhsa_" + k + r" (\d+)", meta).group(1)) for k in ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")}


def _body(src, sym):
    i0 = src.index("\n" + sym + ":")
    return src[i0:src.index(".Lfunc_end", i0)].split("\n")


@pytest.mark.parametrize("mode,f64_per_pair", [(2, 8), (1, 7), (0, 5)])
def test_folded_kernel_far_loops_and_resources(asm, mode, f64_per_pair):
    sym = SYM % mode
    body = _body(asm, sym)
    far = []
    for a, b in loops(body):
        c = count(body, a, b)
        if c["rsq"] >= 4 and c["branches"] == 1 and not any("v_cndmask" in l for l in body[a:b + 1]):
            far.append(c)
    # UNR = 4 sources of one list (16 pairs), a group of either sign (32 pairs), the one-source tail loops (4 pairs)
    assert sorted(c["rsq"] for c in far) == [4, 4, 16, 16, 32], (mode, far)
    for c in far:
        assert c["f64"] == f64_per_pair * c["rsq"], (mode, c)
    m = _meta(asm, sym)
    assert m["private_segment_fixed_size"] == 0, m
    assert m["next_free_vgpr"] <= 128, m                              # four waves per SIMD
    assert 16 * m["group_segment_fixed_size"] <= LDS_PER_CU, m        # ... and their LDS
    # no density is classified in the kernel any more: the division k = 1 / f^2 is the pre-pass's
    assert not any(re.search(r"\bv_(div_scale|div_fmas|div_fixup|rcp)_f64\b", l) for l in body), mode


def test_prepass_kernel_has_no_scratch(asm):
    syms = re.findall(r"\.amdhsa_kernel (\S*fold_prepass_kernel\S*)", asm)
    assert len(syms) == 1, syms
    m = _meta(asm, syms[0])
    assert m["private_segment_fixed_size"] == 0 and m["next_free_vgpr"] <= 128, m   # (its 1024-lane workgroup is four waves per SIMD)
    assert any("v_div_scale_f64" in l for l in _body(asm, syms[0]))    # the IEEE division lives here
