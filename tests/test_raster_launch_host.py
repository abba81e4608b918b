"""The launch geometry of the raster kernels (csrc/raster_launch.hpp: tile-shape limits, strips to workgroups, regions and their sub-grids, strips per lane of
the measuring kernels) on the host: tests/tools/raster_launch_check.cpp includes that header alone and checks it against a plain restatement and against
verdicts written out as constants. No GPU involved, nothing allocated, nothing launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_raster_launch_geometry_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "raster_launch_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "frave_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "tools", "raster_launch_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
