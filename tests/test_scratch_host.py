"""ns3d_scratch, the owner type of the library's lazily grown device buffers, without a GPU: tests/c_host/scratch_host.cpp includes
navierstokes3d_amd/csrc/ns3d_scratch.h, supplies hipMalloc / hipFree / ns3d_fail itself (malloc and free behind counters) and is
built WITHOUT the HIP runtime, with AddressSanitizer and UBSan, as a stand-alone program.  It checks: room enough means no call;
the first reserve allocates and does not drain; growth drains exactly once and before the free; a refusing drain keeps buffer and
size and hands its value back; a failed allocation leaves {nullptr, 0} and a later reserve succeeds; release twice frees once; a
std::vector of owners grows and dies without a double free or a leak."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokes3d_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c_host", "scratch_host.cpp")


def _hip_include():
    cands = [os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    cands.append("/opt/rocm")
    for c in cands:
        if c and os.path.exists(os.path.join(c, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(c, "include")
    raise AssertionError("hip/hip_runtime_api.h not found (looked under %s)" % [c for c in cands if c])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is absent")
def test_scratch_owner_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "scratch_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing to preload, no link-order check
                    "-D__HIP_PLATFORM_AMD__", "-I", _hip_include(), "-I", CSRC, SRC, "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("scratch OK:"), run.stdout
