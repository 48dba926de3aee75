"""The window geometry of the narrow-counter scan kernel (frisk_amd/csrc/win_step.h, included by scan8_kernel.h) on the CPU:
tools/exp/win_step_host.cpp, a stand-alone program, checks that a window advanced from its predecessor by additions (win_next) has the
fields of the window computed from its candidate index (win_fresh) - every inc in 1..2600, w in {600, 2000, 2048, 5000, 5120}, 40
consecutive windows of scaffolds whose resident position, start and ring base straddle 2^32 and multiples of ITS x COLS - and that the
32-bit lane arithmetic of stage 1's sequence addressing gives the word indices and shift amounts of the 64-bit formulas for every lane
and every base offset 0..31.  Built with the host compiler - under AddressSanitizer + UBSan where the compiler has their runtime, plain
otherwise; nothing of it is loaded into Python, nothing touches a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_window_advanced_by_additions_is_the_window_computed_afresh(tmp_path):
    cxx = next((p for p in map(shutil.which, ("g++", "c++", "clang++")) if p), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "win_step_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "frisk_amd", "csrc"),
            os.path.join(ROOT, "tools", "exp", "win_step_host.cpp"), "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:        # (a compiler without the sanitizers' runtime: the plain program)
        build = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith("win_step_host ok"), (run.stdout[-2000:], run.stderr[-3000:])
    # every (w, inc, placement) walked all its 39 successors: 5 x 2600 x 4 at ITS = 20, 3 x 2047 x 4 at ITS = 8
    assert "%d + %d successors" % (5 * 2600 * 4 * 39, 3 * 2047 * 4 * 39) in run.stdout, run.stdout
