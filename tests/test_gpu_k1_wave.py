"""K1's wave form (fwd_wave_kernel): every wave stages and transforms its own pairs of cells, no tiles and no workgroup barrier. Pinned through
FRI_HIP_K1_WAVE=1 (read under FRI_HIP_TUNING=1 when the plan is created) it must give the oracle's coefficients bit for bit wherever it runs, the launches it
does not serve must fall back to the tile kernel, and a plan that measured it (fri_hip_plan_tune_forward) must stay right whichever form won.

The output is pre-filled with a sentinel no coefficient can take, so a cell nobody wrote shows as well as a wrong one. FRI_HIP_TARGET_WGS=8 cuts the same
images into eight shares (two CUs' worth): several pairs per wave, the double buffer in use; the default cut of a small image is one pair per share."""
import os

import numpy as np
import pytest

from tests.common import gen_image

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KEYS = ("FRI_HIP_TUNING", "FRI_HIP_K1_WAVE", "FRI_HIP_TARGET_WGS")


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def make_plan(ctx, w, h, c, wave="1", target_wgs=None):
    """A plan created with the form pinned (the knobs are read once, at creation); the environment is put back before it is used."""
    import frave_amd as fa

    saved = {k: os.environ.get(k) for k in KEYS}
    try:
        os.environ["FRI_HIP_TUNING"] = "1"
        os.environ["FRI_HIP_K1_WAVE"] = wave
        os.environ.pop("FRI_HIP_TARGET_WGS", None)
        if target_wgs:
            os.environ["FRI_HIP_TARGET_WGS"] = str(target_wgs)
        return fa.Plan(ctx, w, h, c)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def gradient(w, h, c=1):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((3 * x + 5 * y) & 255).astype(np.uint8)[:, :, None], c, axis=2)


Q_ONES = np.ones(32, np.int32)
Q_MIXED = np.ones(32, np.int32)
Q_MIXED[:10] = [3, 2, 5, 1, 7, 2, 4, 1, 6, 3]

_wanted = {}


def wanted(oracle, name, img, q):
    """The oracle's coefficients of an image under a matrix, computed once per module."""
    key = (name, img.shape, q.tobytes())
    if key not in _wanted:
        h, w, c = img.shape
        W = oracle.Wavelet(img, h, w, c)
        if not np.all(q == 1):
            W.quantize(q)
        _wanted[key] = W.coefficients()
    return _wanted[key]


def launch(P, images, q, offset=0):
    """One launch over `images` on device buffers whose output holds the sentinel; `offset` shifts the pixel pointer off its alignment."""
    import torch

    n = len(images)
    stride = P.pixel_bytes
    d_px = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    flat = np.concatenate([np.ascontiguousarray(i).reshape(-1) for i in images])
    d_px[offset:offset + n * stride] = torch.from_numpy(flat).cuda()
    d_co = torch.full((n, P.coef_count), SENTINEL, dtype=torch.int32, device="cuda")
    P.transform_quant_dev(d_px.data_ptr() + offset, d_co.data_ptr(), q, n_images=n, pixel_stride=stride if n > 1 else 0, coef_stride=P.coef_count if n > 1 else 0)
    torch.cuda.synchronize()
    return d_co.cpu().numpy().reshape(n, P.channels, P.num_cells, 512)


def images_of(w, h, c=1):
    return {"noise": gen_image("noise", w, h, c, 77), "gradient": gradient(w, h, c)}


# 16 x 16: every cell is a boundary cell; 272 x 80: an odd cell count (61), the mirrored last item; 512 x 512: interior plus rim; 1024 x 48: one band
@pytest.mark.parametrize("target_wgs", [None, 8])
@pytest.mark.parametrize("shape", [(16, 16), (48, 80), (272, 80), (512, 512), (1024, 48)])
def test_wave_form_gives_the_oracles_coefficients(ctx, oracle, shape, target_wgs):
    w, h = shape
    P = make_plan(ctx, w, h, 1, target_wgs=target_wgs)
    rep = P.tune_forward()
    assert rep["tuned"] is False and rep["kept"].startswith("wave/"), rep  # pinned, and the plan carries the form
    for name, img in images_of(w, h).items():
        for q in (Q_ONES, Q_MIXED):
            got = launch(P, [img], q)[0]
            assert not np.any(got == SENTINEL), (name, "cells nobody wrote")
            assert np.array_equal(got, wanted(oracle, name, img, q)), (shape, name)
    P.close()


def test_wave_form_three_images_in_one_launch(ctx, oracle):
    w, h = 272, 80
    P = make_plan(ctx, w, h, 1, target_wgs=8)
    assert P.tune_forward()["kept"].startswith("wave/")
    imgs = images_of(w, h)
    batch = [imgs["noise"], imgs["gradient"], imgs["noise"][::-1].copy()]
    got = launch(P, batch, Q_MIXED)
    for k, (name, img) in enumerate(zip(("noise", "gradient", "noise flipped"), batch)):
        assert np.array_equal(got[k], wanted(oracle, name, img, Q_MIXED)), name
    P.close()


@pytest.mark.parametrize("case", ["not FAST: 100 x 70", "pixel pointer off by one byte", "C = 3"])
def test_launches_the_form_does_not_serve_fall_back_to_the_tile_kernel(ctx, oracle, case):
    w, h, c, offset = {"not FAST: 100 x 70": (100, 70, 1, 0), "pixel pointer off by one byte": (272, 80, 1, 1), "C = 3": (48, 80, 3, 0)}[case]
    P = make_plan(ctx, w, h, c)
    for name, img in images_of(w, h, c).items():
        got = launch(P, [img], Q_MIXED, offset=offset)[0]
        assert np.array_equal(got, wanted(oracle, name, img, Q_MIXED)), (case, name)
    P.close()


def test_knob_zero_keeps_the_tile_kernel(ctx, oracle):
    w, h = 272, 80
    P = make_plan(ctx, w, h, 1, wave="0")
    rep = P.tune_forward()
    assert rep["tuned"] is False and not rep["kept"].startswith("wave/")
    img = images_of(w, h)["noise"]
    assert np.array_equal(launch(P, [img], Q_ONES)[0], wanted(oracle, "noise", img, Q_ONES))
    P.close()


def test_tuned_plan_measures_the_wave_form_and_stays_right(ctx, oracle):
    import frave_amd as fa

    w, h = 512, 512
    P = fa.Plan(ctx, w, h, 1)
    rep = P.tune_forward(24)
    assert rep["tuned"] is True and rep["winner"] in rep["candidates_us"]
    waves = {k: v for k, v in rep["candidates_us"].items() if k.startswith("wave/")}
    assert len(waves) >= 2 and all(v > 0 for v in waves.values()), rep  # the form was a candidate, whoever won
    print("winner", rep["winner"], "candidates_us", rep["candidates_us"])
    imgs = images_of(w, h)
    for _ in range(2):  # the measured plan, then the same plan again
        for name, img in imgs.items():
            got = launch(P, [img], Q_ONES)[0]
            assert np.array_equal(got, wanted(oracle, name, img, Q_ONES)), name
    assert np.array_equal(launch(P, [imgs["noise"]], Q_MIXED)[0], wanted(oracle, "noise", imgs["noise"], Q_MIXED))
    P.close()
