"""The address arithmetic of the genome-value ring (frisk_amd/csrc/ring_rows.h, included by scan8_kernel.h) on the CPU:
tools/exp/ring_rows_host.cpp, a stand-alone program, checks exhaustively that the row-aligned form that windows with rb_r = 0 take is
the general form (every it < ITS, tid < 256, rb_q < FRISK8_RING_COLS), that the general form is the ring's definition, and that for
rb_r = 1..ITS-1 no two positions of a window share a slot.  Built with the host compiler - under AddressSanitizer + UBSan where the
compiler has their runtime, plain otherwise; nothing of it is loaded into Python, nothing touches a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_aligned_ring_offsets_equal_the_general_form(tmp_path):
    cxx = next((p for p in map(shutil.which, ("g++", "c++", "clang++")) if p), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "ring_rows_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "frisk_amd", "csrc"),
            os.path.join(ROOT, "tools", "exp", "ring_rows_host.cpp"), "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:        # (a compiler without the sanitizers' runtime: the plain program)
        build = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith("ring_rows_host ok"), (run.stdout[-2000:], run.stderr[-3000:])
