"""The handle table behind the library's five registries (csrc/rrt_handles.h: sky, workspace, noise table, tile map, tile order)
driven on the CPU through tests/handles/handle_exerciser.cpp: plain C++, no HIP.  The return codes of the entry points built on it
are pinned in tests/test_capi.py and tests/sanitize/host_exerciser.cpp; these are the table's own checks."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "tests", "handles", "handle_exerciser.cpp")
CXX = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"]


@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("handles") / "handle_exerciser")
    subprocess.run(CXX + [SRC, "-o", exe], check=True)

    def run(case, binary=exe):
        r = subprocess.run([binary, case], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == case + " ok", (r.stdout[-500:], r.stderr[-3000:])
    return run


def test_ids_count_up_from_the_start_and_are_never_reused(exerciser):
    exerciser("ids")


def test_unknown_ids_fail_and_change_nothing(exerciser):
    exerciser("unknown")


def test_a_refused_take_leaves_the_element_registered(exerciser):
    exerciser("refuse")


def test_a_shared_element_outlives_its_take(exerciser):
    exerciser("pinned")


def test_eight_threads_of_mixed_operations(exerciser, tmp_path):
    """8 threads x 10 000 mixed insert / get / take: the element count that is left and every id issued exactly once.  Built with
    -fsanitize=thread where the host toolchain links it (it does on the project's build image: this case then runs under
    ThreadSanitizer, whose report fails the run), and run plain where it does not -- never skipped."""
    tsan = str(tmp_path / "handle_exerciser_tsan")
    r = subprocess.run(CXX + ["-g", "-fsanitize=thread", SRC, "-o", tsan], capture_output=True, text=True)
    if r.returncode == 0:
        probe = subprocess.run([tsan, "ids"], capture_output=True, text=True, timeout=300)
        if "FATAL: ThreadSanitizer" not in probe.stderr:          # the runtime cannot map its shadow on some kernels: no finding
            return exerciser("threads", tsan)
    exerciser("threads")
