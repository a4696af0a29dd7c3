"""The device-memory tools of csrc/sm_devmem.h (grow and DevList), without a GPU.

tests/devmem_probe.cpp includes the header with SM_DEVMEM_STUB: the raw operations are host ones that count live allocations,
log every free and fail the k-th allocation.  For a three-buffer grow group and a five-buffer list, and every k: a failed
growth from empty and from a smaller size leaves null pointers, capacity 0, nothing live and nothing freed twice; the next
growth succeeds; a call that needs no growth makes no raw call; release is idempotent.  The program is built with the
address and undefined-behaviour sanitizers (host code only: the flag goes behind -Xarch_host) and must leave no report."""
import os
import shutil
import subprocess

import pytest

from util import ROOT


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("devmem_probe") / "devmem_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "devmem_probe.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_failed_growth_leaves_nothing_behind(probe):
    # (leaks are judged by the stub's count of live allocations, not by LeakSanitizer)
    r = subprocess.run([probe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 500, r.stdout
