"""The frame's plan (csrc/b32_frame_plan.h) on the host: the header holds the decisions of enqueue_frame and launch_fill as pure functions
and includes nothing of HIP, so g++ compiles it.  tests/cpp/frame_plan_host.cpp checks the documented cases as literals and compares every
decision with the expressions it replaced (the parent commit's text, carried in the program) over a grid of inputs.  No GPU."""
import atexit
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the grid of tests/cpp/frame_plan_host.cpp
N_NTILES, N_CU, N_PERMILLE, N_BANDS, N_TILES_X = 9, 3, 7, 6, 3
WANT_CASES = {
    "cut_grid": N_BANDS * N_TILES_X * N_CU,
    "gate": N_PERMILLE * N_NTILES * N_CU,
    "hand_over": 2 ** 9 * N_NTILES * N_CU,       # nine bools: rotated, batched, join_ok, a stream not seen yet, direct_bin, want_inline, wire_front, ordered_all, narrow
    "fused": 2 ** 3 * N_NTILES,
    "wide": N_NTILES * N_CU * 2,
}


def _run():
    d = tempfile.mkdtemp(prefix="b32_frame_plan_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "frame_plan_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bonnie-32_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "frame_plan_host.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_frame_plan_documented_cases_and_the_parents_expressions():
    r = _run()
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert "ok" in lines
    # every grid really ran: a loop of zero iterations compares nothing and would pass
    got = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("cases ")}
    assert got == WANT_CASES, got


def test_frame_plan_header_includes_nothing_of_hip():
    text = open(os.path.join(ROOT, "bonnie-32_amd", "csrc", "b32_frame_plan.h")).read()
    includes = [ln.strip() for ln in text.split("\n") if ln.strip().startswith("#include")]
    assert includes == ["#include <cstdint>"], includes
