"""The folded far pair of the fp64 tile-centred single layer (sctl_amd/csrc/centered_kernel.hpp, CenteredFxU<double>::FOLD), counted in the device
assembly hipcc makes of centered.hip with the Makefile's flags (no GPU needed): per far pair 8 fp64 VALU instructions + 1 v_rsq_f64 at full precision
(MODE 2) and 7 + 1 in the 10-digit mode (MODE 1), no scratch, and at full precision four waves per SIMD (at most 128 vector registers)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sctl_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isa_loop_counts import count, loops  # noqa: E402

SYM = "_ZN8sctl_amd15centered_kernelINS_11CenteredFxUIdEEdLi%dELi4ELi4EEEvNS_8EvalArgsIT0_EE"   # centered_kernel<CenteredFxU<double>, double, MODE, T = 4, UNR = 4>


def _centered_asm(tmp_path):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    extra = subprocess.run(["make", "-s", "-C", CSRC, "print-unit-flags", "UNIT=centered"], capture_output=True, text=True, check=True).stdout.split()
    out = str(tmp_path / "centered.s")
    subprocess.run(["/opt/rocm/bin/hipcc"] + flags + extra + ["--offload-device-only", "-S", os.path.join(CSRC, "centered.hip"), "-o", out],
                   capture_output=True, check=True, timeout=900)
    return open(out).read()


def test_folded_far_loop_counts(tmp_path):
    src = _centered_asm(tmp_path)
    for mode, f64_per_pair in ((2, 8), (1, 7)):
        sym = SYM % mode
        i0 = src.index("\n" + sym + ":")
        body = src[i0:src.index(".Lfunc_end", i0)].split("\n")
        # the far loops: single-branch loops with v_rsq_f64 and no masking select (the exact near loop has one); the unrolled ones take UNR = 4 sources
        # of one list (16 pairs) or a group of either sign (32 pairs), the tail loop one source (4 pairs)
        far = []
        for a, b in loops(body):
            c = count(body, a, b)
            if c["rsq"] >= 4 and c["branches"] == 1 and not any("v_cndmask" in l for l in body[a:b + 1]):
                far.append(c)
        assert sorted(c["rsq"] for c in far) == [4, 4, 16, 16, 32], (mode, far)
        for c in far:
            assert c["f64"] == f64_per_pair * c["rsq"], (mode, c)
        meta = re.search(r"\.amdhsa_kernel " + sym + r"\n(.*?)\.end_amdhsa_kernel", src, re.S).group(1)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, mode
        if mode == 2:
            assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128
