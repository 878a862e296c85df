"""The host helpers that every host-buffer entry and the operator handle share (sctl_amd/csrc/staging.hpp): adding or storing a staged result, scattering
a device's slab of density rows into the caller's target order, and the slices of the staging buffer.  The header has no HIP in it, so the library's own
functions run here on the CPU through a small host program (tests/cpp/staging_main.cpp) built with the address and undefined-behaviour sanitizers:
nd in {1, 3}, k1 in {1, 3}, nt in {0, 1, 5}, with and without a permutation, accumulate 0 and 1, fp32 and fp64, each against a three-line loop."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("staging") / "staging_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "staging_main.cpp"), "-o", out], check=True, timeout=300)
    return out


def test_host_helpers_match_reference_loops_under_sanitizers(prog):
    res = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    scatter64, scatter32, staging = (int(v) for v in res.stdout.split())
    assert scatter64 == scatter32 == 2 * 2 * 3 * 2 * 2     # every combination ran
    assert staging == 6
