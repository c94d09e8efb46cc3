"""The plan-file validator under AddressSanitizer and UBSan: tests/native/asan_planfile.cpp, a stand-alone
host program built from cfs_planfile.hpp and cfs_plan.hpp alone, is compiled here with
-fsanitize=address,undefined (the sanitizer runtimes linked statically) and run once.  It is never loaded into Python and needs no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validator_survives_truncations_flips_and_bad_sizes(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is what the C++ surface of this project is built with"
    exe = str(tmp_path / "asan_planfile")
    subprocess.run([cxx, "-std=c++17", "-O0", "-fopenmp", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "cfs_spmv_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "asan_planfile.cpp"), "-o", exe], check=True)
    # (leak detection needs ptrace, which a container may not grant; everything else stays on)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               OMP_NUM_THREADS="2")
    r = subprocess.run([exe, str(tmp_path)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all returned" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
