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


def _build_and_run(tmp_path, name, *args):
    """tools/exp/<name>.cpp built and run the way the test above does it; its standard output"""
    cxx = next((p for p in map(shutil.which, ("g++", "c++", "clang++")) if p), None)
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / name)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "frisk_amd", "csrc"),
            os.path.join(ROOT, "tools", "exp", name + ".cpp"), "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:        # (a compiler without the sanitizers' runtime: the plain program)
        build = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip().startswith(name + " ok"), (run.stdout[-2000:], run.stderr[-3000:])
    return run.stdout


def test_every_launch_of_a_schedule_names_a_row_of_the_form_tables(tmp_path):
    """Which instantiation a launch runs is the schedule's statement too (ScanSchedule::form_*, form16; scan_forms.h), and the launchers
    only look it up: tools/exp/scan_forms_host.cpp sweeps the shapes above and shapes off the narrow-counter path and requires that every
    launch has a form, that the form is a row of its family's table and what the rule - restated there per launch kind - says, and that
    the kmin = 1 role sits on the 4-bit bulk launches of the schedules that name it alone.  tests/golden/scan8_dispatch_parent.tsv holds
    what the launcher before the tables (launch_narrow, an if-ladder over eleven arguments) launched for each of 1 536 requests: the
    rule gives each the same form, or none - and none to no request that a schedule of the sweep makes."""
    out = _build_and_run(tmp_path, "scan_forms_host", os.path.join(ROOT, "tests", "golden", "scan8_dispatch_parent.tsv"))
    m = re.search(r"ok: (\d+) schedules, (\d+) narrow-counter launches \((\d+) with the kmin = 1 role\), (\d+) of 34 \+ (\d+) of 14 rows reached; "
                  r"fixture: (\d+) requests keep their form, (\d+) that no schedule makes have none", out)
    assert m, out[-2000:]
    plans, launches, kmin1, rows8, rows16, same, none = map(int, m.groups())
    # the sweep of the test above, then 4 K x 5 w x 2 debug x 4 variants off the narrow-counter path
    assert plans == 5 * 3 * 5 * 3 * 2 * 3 * 4 * 2 * 2 * 2 + 4 * 5 * 2 * 4
    assert launches > plans // 2 and 0 < kmin1 < launches
    # every row is reached today; a row that no schedule reaches is reported in the program's output, not an error
    assert 0 < rows8 <= 34 and 0 < rows16 <= 14
    # kmax {6, 7, 8} x bits {4, 8} x small_w x debug x sample x side x kmin1 x slides x listed x kmin {1, 2}
    assert same + none == 3 * 2 ** 9 and same > 0
