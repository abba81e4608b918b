"""The tile grid and the region tables of K15 and K17 (csrc/region_table.hpp: TileGrid::region, cover_of, preview_size, build_region_table, the remembered
table) on the host: tests/tools/region_table_check.cpp includes that header alone and checks it against a per-pixel and per-sample restatement, and every
refusal at its edge beside the accepted case next to it. No GPU involved, nothing launched; the largest allocation is a table of 65536 rows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_tables_under_the_sanitizers(tmp_path):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "region_table_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "frave_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "tools", "region_table_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
