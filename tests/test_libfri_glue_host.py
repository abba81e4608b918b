"""The pure helpers of the C++ host mirror's glue (frave_amd/host/libfri_glue.hpp) on the host: tests/tools/libfri_glue_check.cpp includes that header and checks
the refused-plane texts of the four routes that word them, the size target's step-down against scripted coders, channel_params, the lossless fall-back, the plane
buffers, and load_coded against direct emit::parse_tiled_coded calls on a 2 x 2-tile `frit` file written here with the host emitter. No GPU involved, nothing
launched: the program links the emitter alone, so nothing of the C ABI is called."""
import os
import subprocess

from tests.coded_cases import tiled_file
from tests.test_coded_parse_host import H, TH, TW, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_glue_helpers_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    host, csrc = os.path.join(ROOT, "frave_amd", "host"), os.path.join(ROOT, "frave_amd", "csrc")
    frv, _, _ = tiled_file(W, H, 3, TW, TH, 50)  # the smallest lattice with 2 x 2 tiles of those tests, RGB and lossy: twelve planes
    path = tmp_path / "four_tiles.frv"
    path.write_bytes(frv)
    exe = tmp_path / "libfri_glue_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", host,
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), os.path.join(ROOT, "tests", "tools", "libfri_glue_check.cpp"),
                           os.path.join(host, "emit.cpp"), os.path.join(csrc, "geometry.cpp")])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
