"""Lossy coding to a target size, host side: the size estimate (tests/rate_model.py, the formula of fri_hip_estimate_size_dev) against the files the product
emitter writes from oracle-made planes, and the argument checks of the estimate and search entry points on host-only plans. CPU only."""
import ctypes as C

import numpy as np
import pytest

import frave_amd as fa
from frave_amd import api
from tests import rate_model


@pytest.mark.parametrize("shape", [(300, 200, 1), (640, 480, 1), (1024, 768, 1), (160, 120, 3), (320, 240, 3)])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_estimate_is_within_24_bytes_per_channel_of_the_file(oracle, shape, kind):
    import frave_amd.emit as emit
    from tests.common import gen_image

    w, h, c = shape
    img = gen_image(kind, w, h, c, 1)
    for q in (100, 1, 50, 90):
        centers, coefs, bucket, pred, hist, oob, vp, wp = rate_model.oracle_arrays(img, w, h, c, q)
        assert not oob.any()
        est = rate_model.estimate_image(hist, oob)
        frv = emit.encode_image(w, h, centers, coefs, bucket, pred, hist, vp, wp, quality=q if q < 100 else 0)
        assert abs(est - len(frv)) <= 24 * c, (q, est, len(frv))


def test_container_bytes_are_exact():
    """The estimate is the container (18 + per channel 218 + 14 per context without off-distribution values) plus the ideal bits rounded up to bytes."""
    hist = np.zeros((3, 10, 1024), np.uint32)
    hist[:, :, 0] = 256  # one used symbol per context, near the Laplace peak: no off-distribution values
    for b in range(10):
        f, n_off, bits = rate_model.context_model(hist[0, b], b)
        assert n_off == 0 and bits == 8
    est = rate_model.estimate_image(hist)
    fixed = sum(rate_model.context_cost(hist[ch, b], b)[0] for ch in range(3) for b in range(10))
    assert est == 18 + 3 * (218 + 10 * 14) + -(-fixed // 2 ** 19)


def test_uncodable_histograms():
    hist = np.zeros((1, 10, 1024), np.uint32)
    hist[0, :, 3] = 1000
    assert rate_model.estimate_image(hist) != rate_model.UNCODABLE
    assert rate_model.estimate_image(hist, np.array([1], np.uint64)) == rate_model.UNCODABLE  # an out-of-alphabet symbol
    hist[0, 7] = 0
    assert rate_model.estimate_image(hist) == rate_model.UNCODABLE  # a context without symbols


def test_off_distribution_values_cost_two_bytes_each():
    hist = np.zeros((1, 10, 1024), np.uint32)
    hist[0, :, 0] = 5000
    base = rate_model.estimate_image(hist)
    f, n_off, _ = rate_model.context_model(hist[0, 2], 2)
    assert n_off == 0
    hist[0, 2, 1000] = 1  # far in the tail: the shape gives it 0, so it is listed
    f, n_off, _ = rate_model.context_model(hist[0, 2], 2)
    assert n_off == 1 and f[1000] >= 1
    assert rate_model.estimate_image(hist) >= base + 2


def _host_plan(c=1):
    return fa.Plan(None, 64, 48, c)


def test_host_only_plan_refuses_estimate():
    L = api.load_library()
    P = _host_plan(3)
    hist = np.ones((3, 10, 1024), np.uint32)
    out = C.c_uint64(7)
    assert L.fri_hip_estimate_size(P._h, api._p(hist), None, C.byref(out)) == -3
    assert L.fri_hip_estimate_size_dev(P._h, 1, 16, None, 16, None, None) == -3
    assert out.value == 7
    with pytest.raises(fa.FriHipError) as e:
        P.estimate_size(hist)
    assert e.value.code == -3
    P.close()


def test_host_only_plan_refuses_search():
    L = api.load_library()
    P = _host_plan(1)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, est = C.c_int32(-7), C.c_uint64(0)
    assert L.fri_hip_search_quality_for_size(P._h, api._p(px), 10000, C.byref(qual), C.byref(est)) == -3
    assert L.fri_hip_search_quality_for_size_dev(P._h, 16, 10000, C.byref(qual), C.byref(est), None) == -3
    assert qual.value == -7
    with pytest.raises(fa.FriHipError) as e:
        P.search_quality_for_size(px, 10000)
    assert e.value.code == -3
    P.close()


def test_search_refuses_bad_budgets_and_rct_plans():
    L = api.load_library()
    P = _host_plan(3)
    px = np.zeros(P.pixel_bytes, np.uint8)
    qual, est = C.c_int32(0), C.c_uint64(0)
    assert L.fri_hip_search_quality_for_size(P._h, api._p(px), 0, C.byref(qual), C.byref(est)) == -1
    assert L.fri_hip_search_quality_for_size_dev(P._h, 16, 0, C.byref(qual), C.byref(est), None) == -1
    assert L.fri_hip_search_quality_for_size(P._h, None, 1000, C.byref(qual), C.byref(est)) == -1
    assert L.fri_hip_search_quality_for_size(P._h, api._p(px), 1000, None, C.byref(est)) == -1
    P.set_colour_transform(api.COLOUR_RCT)
    assert L.fri_hip_search_quality_for_size(P._h, api._p(px), 10 ** 6, C.byref(qual), C.byref(est)) == -1
    assert L.fri_hip_search_quality_for_size_dev(P._h, 16, 10 ** 6, C.byref(qual), C.byref(est), None) == -1
    P.close()


def test_estimate_refuses_bad_arguments():
    L = api.load_library()
    assert L.fri_hip_estimate_size(None, None, None, None) == -1
    assert L.fri_hip_estimate_size_dev(None, 1, 16, None, 16, None, None) == -1
