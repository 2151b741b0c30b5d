"""Ownership logic of radtxfr_amd/csrc/rtx_devmem.h (DevBuf, StreamScratch, DevTableCache) on the host, under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/devmem_host_main.cpp is a stand-alone program that defines the four
rtx_dev_* functions over malloc, with a count of live allocations, a switch that makes the next allocation or copy fail
and a per-thread "current device". No GPU, no HIP."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_cxx():
    """The host C++ compiler: $CXX, the clang++ that hipcc drives (it links the sanitizer runtime statically, so the program
    runs whatever else the environment preloads), or g++."""
    cands = [os.environ.get("CXX")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        cands += [os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")]
    cands += ["clang++", "g++"]
    for c in cands:
        if c and shutil.which(c):
            return shutil.which(c)
    raise AssertionError("no host C++ compiler found (tried %s)" % [c for c in cands if c])


def test_devmem_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_host")
    build = subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                            os.path.join(HERE, "devmem_host_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr  # failed checks and every sanitizer report go to stderr
    assert "devmem host checks passed" in run.stdout
