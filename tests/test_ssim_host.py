"""SSIM (fri_hip_measure_ssim*, fri_hip_search_quality_ssim*), host side: the numpy oracle of tests/ssim_ref.py against an independent per-window
restatement in Python integers and floats, against the textbook float SSIM, its exact properties, the argument checks of the C ABI on host-only plans and
the driver's option checks. CPU only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import frave_amd as fa
from frave_amd import api
from tests import ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8, 1), (9, 13, 3), (37, 20, 1), (64, 8, 3)]  # (width, height, channels)
NEW_SYMBOLS = ["fri_hip_measure_ssim_dev", "fri_hip_measure_ssim", "fri_hip_search_quality_ssim", "fri_hip_search_quality_ssim_dev"]


def py_measure(a, b, w, h, c):
    """the definition of include/fri_hip.h, one window at a time: Python integers, float(n) / float(d), round() (half to even)"""
    a = [int(x) for x in np.asarray(a, np.uint8).ravel()]
    b = [int(x) for x in np.asarray(b, np.uint8).ravel()]
    nx, ny = w // 4 - 1, h // 4 - 1
    out, values = [], []
    for ch in range(c):
        total = 0
        for j in range(ny):
            for i in range(nx):
                sa = sb = saa = sbb = sab = 0
                for y in range(4 * j, 4 * j + 8):
                    for x in range(4 * i, 4 * i + 8):
                        p, q = a[(y * w + x) * c + ch], b[(y * w + x) * c + ch]
                        sa, sb, saa, sbb, sab = sa + p, sb + q, saa + p * p, sbb + q * q, sab + p * q
                n = (2 * sa * sb + 26634) * (2 * (64 * sab - sa * sb) + 239708)
                d = (sa * sa + sb * sb + 26634) * (64 * saa - sa * sa + 64 * sbb - sb * sb + 239708)
                assert abs(n) < 2 ** 57 and 0 < d < 2 ** 63
                v = round(float(n) / float(d) * 2 ** 32)
                assert abs(v) <= 2 ** 32
                values.append(v)
                total += v
        out.append(total)
    return out + [nx * ny], values


def rasters(w, h, c, seed):
    """(name, a, b) pairs: random, extreme and structured"""
    rng = np.random.default_rng(seed)
    n = w * h * c
    noise = rng.integers(0, 256, n, dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    smooth = np.repeat(((xx * 3 + yy * 5) & 255).astype(np.uint8)[..., None], c, axis=2).ravel()
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], c, axis=2).ravel()
    bits = (rng.integers(0, 2, n) * 255).astype(np.uint8)
    zeros, full = np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    near = np.clip(smooth.astype(np.int32) + rng.integers(-3, 4, n), 0, 255).astype(np.uint8)
    return [("noise-noise", noise, rng.integers(0, 256, n, dtype=np.uint8)), ("noise-smooth", noise, smooth), ("smooth-near", smooth, near),
            ("0-255", zeros, full), ("255-0", full, zeros), ("0-0", zeros, zeros), ("checker-inverse", checker, 255 - checker), ("bits-bits", bits, bits[::-1].copy()),
            ("identical", noise, noise.copy()), ("checker-255", checker, full)]


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_equals_the_per_window_restatement(shape):
    w, h, c = shape
    for name, a, b in rasters(w, h, c, sum(shape)):
        want, values = py_measure(a, b, w, h, c)
        got = ssim_ref.measure(a, b, w, h, c)
        assert [int(x) for x in got] == want, name
        assert [int(x) for x in ssim_ref.window_values(a, b, w, h, c).ravel()] == values, name
        mean, per = fa.ssim_of(got, c)
        assert mean == float(sum(want[:c])) / (float(c * want[c]) * 2.0 ** 32) == ssim_ref.ssim(a, b, w, h, c), name
        assert per == [float(s) / (float(want[c]) * 2.0 ** 32) for s in want[:c]]


@pytest.mark.parametrize("shape", SHAPES + [(333, 130, 3)])
def test_oracle_is_the_textbook_ssim_to_1e_5(shape):
    """means, population variances and covariance in float, C1 = (0.01 x 255)^2, C2 = (0.03 x 255)^2, on the same windows"""
    w, h, c = shape
    for name, a, b in rasters(w, h, c, 7 + sum(shape)):
        sa, sb, saa, sbb, sab = (x.astype(np.float64) / 64.0 for x in ssim_ref.window_sums(a, b, w, h, c))
        va, vb, cov = saa - sa * sa, sbb - sb * sb, sab - sa * sb
        k1, k2 = 6.5025, 58.5225
        text = (2 * sa * sb + k1) * (2 * cov + k2) / ((sa * sa + sb * sb + k1) * (va + vb + k2))
        v = ssim_ref.window_values(a, b, w, h, c) / 2.0 ** 32
        assert np.abs(v - text).max() < 1e-5, name
        mean, per = fa.ssim_of(ssim_ref.measure(a, b, w, h, c), c)
        assert abs(mean - text.mean()) < 1e-5 and np.allclose(per, text.reshape(c, -1).mean(axis=1), atol=1e-5, rtol=0)


@pytest.mark.parametrize("shape", SHAPES + [(130, 77, 3)])
def test_identical_rasters_and_symmetry(shape):
    w, h, c = shape
    nx, ny = ssim_ref.windows(w, h)
    for name, a, b in rasters(w, h, c, 3):
        m = ssim_ref.measure(a, a, w, h, c)
        assert list(m) == [nx * ny * 2 ** 32] * c + [nx * ny]
        assert fa.ssim_of(m, c) == (1.0, [1.0] * c)
        assert np.array_equal(ssim_ref.measure(a, b, w, h, c), ssim_ref.measure(b, a, w, h, c)), name


def test_constant_windows_closed_form():
    """constant windows a and b: SSIM = (8192 ab + 26634) / (4096 (a^2 + b^2) + 26634), exactly; n and d carry the common factor c2 through their
    conversions, so v is within one unit of 2^-32 of it - checked in exact integers for every pair of byte values"""
    av, bv = (x.ravel().astype(np.int64) for x in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    v = ssim_ref.values_of_sums(64 * av, 64 * bv, 64 * av * av, 64 * bv * bv, 64 * av * bv)
    num, den = 8192 * av * bv + 26634, 4096 * (av * av + bv * bv) + 26634
    assert np.all(np.abs(v * den - num * 2 ** 32) <= den)  # |v - 2^32 num / den| <= 1
    assert np.all(v[av == bv] == 2 ** 32)
    # and through rasters: two flat images
    for p, q in ((0, 255), (17, 200), (128, 129)):
        m = ssim_ref.measure(np.full(16 * 12, p, np.uint8), np.full(16 * 12, q, np.uint8), 16, 12, 1)
        k = np.flatnonzero((av == p) & (bv == q))[0]
        assert list(m) == [6 * int(v[k]), 6]


def test_symbols_are_exported_and_declared():
    from tests.test_abi_symbols import declared_symbols

    lib = fa.load_library()
    for name in NEW_SYMBOLS:
        assert name in api.SYMBOLS and name in declared_symbols()
        assert C.cast(getattr(lib, name), C.c_void_p).value


def test_host_only_plans_pin_the_refusals():
    """arguments and shapes are checked before the device: -1 for W < 8, H < 8 and a target that is NaN, <= 0 or > 1, or an RCT plan; -3 otherwise"""
    L = api.load_library()
    q, v = C.c_int32(0), C.c_double(0)
    out = np.zeros(4, np.int64)

    def calls(P):
        px = np.zeros(P.pixel_bytes, np.uint8)
        return {
            "measure": lambda t: L.fri_hip_measure_ssim(P._h, api._p(px), api._p(px), api._p(out)),
            "measure_dev": lambda t: L.fri_hip_measure_ssim_dev(P._h, 1, 16, 16, 0, 16, None),
            "search": lambda t: L.fri_hip_search_quality_ssim(P._h, api._p(px), t, C.byref(q), C.byref(v)),
            "search_dev": lambda t: L.fri_hip_search_quality_ssim_dev(P._h, 16, t, C.byref(q), C.byref(v), None),
        }

    for w, h, c in ((7, 20, 1), (20, 7, 3), (4, 4, 1), (8, 3, 1)):
        P = fa.Plan(None, w, h, c)
        for name, f in calls(P).items():
            assert f(0.9) == -1, (w, h, name)
        P.close()
    for w, h, c in ((8, 8, 1), (64, 48, 3), (9, 13, 3)):
        P = fa.Plan(None, w, h, c)
        fs = calls(P)
        assert fs["measure"](0.9) == -3 and fs["measure_dev"](0.9) == -3
        for t in (0.5, 0.95, 1.0, 1e-9):
            assert fs["search"](t) == -3 and fs["search_dev"](t) == -3, t
        for t in (math.nan, 0.0, -0.5, 1.5, 1.0000001, math.inf):
            assert fs["search"](t) == -1 and fs["search_dev"](t) == -1, t
        with pytest.raises(fa.FriHipError) as e:
            P.search_quality_ssim(np.zeros(P.pixel_bytes, np.uint8), 1.5)
        assert e.value.code == -1
        with pytest.raises(fa.FriHipError) as e:
            P.measure_ssim(np.zeros(P.pixel_bytes, np.uint8), np.zeros(P.pixel_bytes, np.uint8))
        assert e.value.code == -3
        if c == 3:  # the colour transforms: YCbCr plans search (no device: -3), RCT plans do not (-1); measuring does not look at the transform
            P.set_colour_transform(api.COLOUR_YCBCR)
            assert fs["search"](0.9) == -3 and fs["search_dev"](0.9) == -3
            P.set_colour_transform(api.COLOUR_RCT)
            assert fs["search"](0.9) == -1 and fs["search_dev"](0.9) == -1
            assert fs["measure"](0.9) == -3 and fs["measure_dev"](0.9) == -3
        # null pointers and batch arguments
        assert L.fri_hip_measure_ssim_dev(P._h, 0, 16, 16, 0, 16, None) == -1
        assert L.fri_hip_measure_ssim_dev(P._h, 2, 16, 16, P.pixel_bytes - 1, 16, None) == -1
        assert L.fri_hip_measure_ssim_dev(P._h, 2, 16, 16, P.pixel_bytes, 16, None) == -3
        assert L.fri_hip_measure_ssim_dev(P._h, 1, None, 16, 0, 16, None) == -1
        assert L.fri_hip_search_quality_ssim(P._h, None, 0.9, C.byref(q), C.byref(v)) == -1
        P.close()
    assert L.fri_hip_measure_ssim(None, None, None, None) == -1


def _driver():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    return os.path.join(ROOT, "frave_amd", "host", "fri_driver")


def test_driver_refuses_ssim_combinations(tmp_path):
    """encode-file --ssim S: 0 < S <= 1, and not with --quality, --psnr, --size, --bpp or --rct (checked before any device is needed)"""
    driver = _driver()
    w, h = 40, 24
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.arange(w * h * 3, dtype=np.uint8).tobytes())
    for bad in (["--ssim", "0.9", "--psnr", "40"], ["--ssim", "0.9", "--size", "1000"], ["--ssim", "0.9", "--rct"], ["--ssim", "0"], ["--ssim", "1.5"],
                ["--ssim", "0.9", "--quality", "50"], ["--ssim", "0.9", "--bpp", "2"], ["--ssim", "nan"], ["--psnr", "40", "--ssim", "0.9", "--ycbcr"]):
        out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv")] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2, (bad, out.stdout, out.stderr)
        assert "--ssim" in out.stderr, bad
    out = subprocess.run([driver], capture_output=True, text=True, timeout=60)
    assert "--ssim S" in out.stderr
