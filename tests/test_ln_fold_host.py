"""Host arithmetic of the folded edge LayerNorm (gamd_amd/csrc/gamd_ln_fold_host.h) without a GPU and without Python in the
loop: tools/ln_fold_host_check.cpp, built once with the address and undefined-behaviour sanitizers, checks on seeded 128 x 128
weights that the six skipped blocks of R are exactly zero, that |R x + c_q| = |B x + c| and the staged and folded first-GEMM
pre-activations agree to 1e-12 in double, and that the packed fragment images round-trip."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_arithmetic_and_packing_pass_a_stand_alone_program_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed to build tools/ln_fold_host_check.cpp"
    exe = tmp_path / "ln_fold_host_check"
    # the sanitizer runtimes linked into the program itself (clang's default): it needs nothing preloaded
    static = [] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    os.path.join(ROOT, "tools", "ln_fold_host_check.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "ln_fold_host_check: ok" in run.stdout, run.stdout + run.stderr
    for line in ("width 128: skipped blocks of R are zero", "width 128: packed images round-trip", "width 96: packed images round-trip"):
        assert line in run.stdout, run.stdout
