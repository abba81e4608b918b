"""The two bisections of frave_amd/csrc/quality_search.hpp, which every fri_hip_search_quality* entry point runs, against the loops those entry points had written out
(tests/tools/quality_search_check.cpp): the same probes in the same order, the same quality, value and return code, the closed form on step functions. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_templates_are_the_loops_they_replace(tmp_path):
    """A stand-alone program with its own main, built with the host compiler and both sanitizers: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "quality_search_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "frave_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "tools", "quality_search_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    last = out.stdout.strip().split("\n")[-1]
    assert last.startswith("ok ") and int(last.split()[1]) > 2000, last
