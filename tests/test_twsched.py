"""The TW contraction's balanced schedule (pyfasst_amd/csrc/fasst_twsched.h) on
the host: tools/twsched_check.cpp, compiled here with the system C++ compiler,
walks every block's range the way k_tw_contract_lds does and checks the
partition (every step owned once, no empty block, a unit's slots dense from 0,
nslot the largest count, the owner formula the inverse of the range formula,
k_tw_update's per-block count the unit's).  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("twsched") / "twsched_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           os.path.join(ROOT, "tools", "twsched_check.cpp"), "-o", exe])
    return exe


def _one(exe, J, G, nft, nb):
    out = subprocess.run([exe, str(J), str(G), str(nft), str(nb)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return tuple(int(v) for v in out.stdout.split())


def test_partition_sweep(checker):
    """J 1-4 x G 1-9 x nft 1-9 x every NB from 1 to U, and the benchmark's
    shape with its neighbours and clamps."""
    out = subprocess.run([checker], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "schedules ok" in out.stdout
    # the sweep's own count: sum over the grid of U = J G nft, plus the 11 extras
    n = sum(J * G * nft for J in range(1, 5) for G in range(1, 10) for nft in range(1, 10)) + 11
    assert "%d schedules" % n in out.stdout


def test_benchmark_shape(checker):
    """F = 2049, T = 10000, J = 4 on 512 resident blocks: U = 4 x 79 x 129
    steps, 79 or 80 per block, at most three partials per unit (the static
    split wrote four everywhere)."""
    assert _one(checker, 4, 79, 129, 512) == (512, 3)
    # one block: one partial; one step per block: a slot per bin step
    assert _one(checker, 4, 79, 129, 1) == (1, 1)
    assert _one(checker, 4, 79, 129, 4 * 79 * 129) == (4 * 79 * 129, 129)


def test_block_count_is_clamped(checker):
    """NB outside [1, U] is clamped, not refused."""
    assert _one(checker, 3, 2, 5, 0) == (1, 1)
    assert _one(checker, 3, 2, 5, -7) == (1, 1)
    assert _one(checker, 3, 2, 5, 1000) == (30, 5)
