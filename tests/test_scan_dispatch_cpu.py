"""Which scans take the K = 8 4-bit bulk kernels compiled for kmin = 1 is a statement of the launch schedule (scan_schedule.h,
ScanSchedule::kmin1_form), so it is checked on the CPU: tools/exp/scan_dispatch_host.cpp, a stand-alone program, sweeps ScanShapes over
kmin 1..5, K 6..8, both counter widths and the adaptive choice, FRISK_SCAN_GENERIC on and off and the debug dump, and requires the
form to be named exactly for K = 8, kmin = 1, no debug dump, flag off - and the flag to move nothing else of a schedule.  Built with
the host compiler - under AddressSanitizer + UBSan where the compiler has their runtime, plain otherwise; nothing of it is loaded
into Python, nothing touches a GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_schedule_names_the_kmin1_form_exactly_where_it_exists(tmp_path):
    cxx = next((p for p in map(shutil.which, ("g++", "c++", "clang++")) if p), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "scan_dispatch_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "frisk_amd", "csrc"),
            os.path.join(ROOT, "tools", "exp", "scan_dispatch_host.cpp"), "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:        # (a compiler without the sanitizers' runtime: the plain program)
        build = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith("scan_dispatch_host ok"), (run.stdout[-2000:], run.stderr[-3000:])
    # 5 kmin x 3 K x 5 n x 3 w x 2 inc x 3 widths x 4 hints x 2 chunk flags x 2 debug x 2 generic
    plans, named = map(int, re.search(r"ok: (\d+) schedules, (\d+) name", run.stdout).groups())
    assert plans == 5 * 3 * 5 * 3 * 2 * 3 * 4 * 2 * 2 * 2
    # K = 8, kmin = 1, w <= 5120, no debug dump, flag off
    assert named == 5 * 2 * 2 * 3 * 4 * 2
