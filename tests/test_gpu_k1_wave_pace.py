"""The paced instance of K1's wave form (fwd_wave_kernel<.., PACED>): a wave that is ahead of the line entry + T i / n sleeps in short steps before its
pair i >= 1, at most a fixed number of steps per pair. Pacing moves WHEN a wave stores, never what: pinned through FRI_HIP_K1_WAVE_PACE=<ticks of the 100 MHz
counter> (read under FRI_HIP_TUNING=1 when the plan is created) the form must give the oracle's coefficients bit for bit for every T - one that never holds,
one that holds every pair to its bound, and the largest the pin takes, which the host clamps.

As in tests/test_gpu_k1_wave.py the output is pre-filled with a sentinel no coefficient can take, and FRI_HIP_TARGET_WGS=8 cuts an image into eight shares so
that a wave has several pairs (only pairs after a wave's first can be held)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.common import gen_image

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
KEYS = ("FRI_HIP_TUNING", "FRI_HIP_K1_WAVE", "FRI_HIP_K1_WAVE_PACE", "FRI_HIP_TARGET_WGS")
SHADER_MHZ = 2400.0  # MI355X: peak engine clock
T_NEVER, T_20US, T_LARGEST = 1, 2000, 2 ** 31 - 1  # one tick: every line is behind the wave; 20 us; the largest int the pin parses


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def make_plan(ctx, w, h, pace, target_wgs=None):
    """A plan with the paced form pinned (the knobs are read once, at creation); the environment is put back before it is used."""
    import frave_amd as fa

    saved = {k: os.environ.get(k) for k in KEYS}
    try:
        os.environ["FRI_HIP_TUNING"] = "1"
        os.environ["FRI_HIP_K1_WAVE_PACE"] = str(pace)
        os.environ.pop("FRI_HIP_K1_WAVE", None)
        os.environ.pop("FRI_HIP_TARGET_WGS", None)
        if target_wgs:
            os.environ["FRI_HIP_TARGET_WGS"] = str(target_wgs)
        return fa.Plan(ctx, w, h, 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def pinned(P):
    """The pinned plan's own account of its wave form: shares, pairs of its longest wave, pace and the bound of a hold."""
    rep = P.tune_forward()
    assert rep["tuned"] is False and rep["kept"].startswith("wave/") and "/pace" in rep["kept"], rep
    return rep["wave_form"]


def gradient(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((3 * x + 5 * y) & 255).astype(np.uint8)[:, :, None]


Q_ONES = np.ones(32, np.int32)
Q_MIXED = np.ones(32, np.int32)
Q_MIXED[:10] = [3, 2, 5, 1, 7, 2, 4, 1, 6, 3]

_images, _wanted = {}, {}


def images_of(w, h):
    if (w, h) not in _images:
        _images[(w, h)] = {"noise": gen_image("noise", w, h, 1, 77), "gradient": gradient(w, h)}
    return _images[(w, h)]


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


def launch(P, images, q):
    """One launch over `images` on device buffers whose output holds the sentinel."""
    import torch

    n = len(images)
    stride = P.pixel_bytes
    d_px = torch.from_numpy(np.concatenate([np.ascontiguousarray(i).reshape(-1) for i in images])).cuda()
    d_co = torch.full((n, P.coef_count), SENTINEL, dtype=torch.int32, device="cuda")
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), q, n_images=n, pixel_stride=stride if n > 1 else 0, coef_stride=P.coef_count if n > 1 else 0)
    torch.cuda.synchronize()
    return d_co.cpu().numpy().reshape(n, P.channels, P.num_cells, 512)


# 16 x 16: every cell is a boundary cell; 272 x 80 in eight shares: several pairs per wave, holds happen; 512 x 512: interior plus rim, the default cut
@pytest.mark.parametrize("pace", [T_NEVER, T_20US, T_LARGEST], ids=["one tick", "20 us", "largest, clamped"])
@pytest.mark.parametrize("shape", [(16, 16, None), (272, 80, 8), (512, 512, None)], ids=["16x16", "272x80 in 8 shares", "512x512"])
def test_pinned_paced_form_gives_the_oracles_coefficients(ctx, oracle, shape, pace):
    w, h, target_wgs = shape
    P = make_plan(ctx, w, h, pace, target_wgs=target_wgs)
    form = pinned(P)
    assert form["pace_ticks"] == min(pace, form["pace_max_ticks"]), form  # the host clamps T
    if target_wgs:
        assert form["max_pairs_per_wave"] >= 2, form  # some wave has a pair that can be held
    for name, img in images_of(w, h).items():
        for q in (Q_ONES, Q_MIXED):
            got = launch(P, [img], q)[0]
            assert not np.any(got == SENTINEL), (name, "cells nobody wrote")
            assert np.array_equal(got, wanted(oracle, name, img, q)), (shape, pace, name)
    P.close()


def test_a_hold_is_bounded_by_its_count_of_steps(ctx, oracle):
    """512 x 512 in eight shares: a dozen pairs per wave. With the largest T (clamped to 2^16 ticks = 655 us) every pair after the first is due tens of
    microseconds after the one before, so every hold runs to its bound; were a hold bounded by the clock alone, the launch would last about T (n - 1) / n.
    The bound comes from the two hold constants and the longest wave's pair count alone: a step is one s_sleep of pace_step_cycles shader cycles at the
    nominal clock, a wave takes at most pace_max_steps steps before each of its pairs but the first, and the waves hold side by side - times two for the
    clock, the only slack (it also covers the read of the counter behind each step, measured at about a quarter of a step) - on top of the same launch
    with a T that never holds. Measured: 15.8 us never held, 39.1 us every pair held, a difference of 23 us against a bound of 37.5 us."""
    import torch

    w, h = 512, 512
    slow, fast = make_plan(ctx, w, h, T_LARGEST, target_wgs=8), make_plan(ctx, w, h, T_NEVER, target_wgs=8)
    form = pinned(slow)
    assert pinned(fast)["max_pairs_per_wave"] == form["max_pairs_per_wave"] and form["max_pairs_per_wave"] >= 4, form
    img = images_of(w, h)["noise"]
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_co = torch.full((slow.coef_count,), SENTINEL, dtype=torch.int32, device="cuda")

    def per_launch_us(P):
        P.time_transform_quant_dev(1, d_px.data_ptr(), P.pixel_bytes, d_co.data_ptr(), P.coef_count, 10)  # clocks up
        return min(P.time_transform_quant_dev(1, d_px.data_ptr(), P.pixel_bytes, d_co.data_ptr(), P.coef_count, 10) for _ in range(3))

    t_fast, t_slow = per_launch_us(fast), per_launch_us(slow)
    step_us = form["pace_step_cycles"] / SHADER_MHZ
    bound = 2.0 * (form["max_pairs_per_wave"] - 1) * form["pace_max_steps"] * step_us  # the factor of two is the only slack
    unbounded = form["pace_ticks"] / 100.0 * (form["max_pairs_per_wave"] - 1) / form["max_pairs_per_wave"]
    print(f"never holds {t_fast:.2f} us, every pair held {t_slow:.2f} us, bound on the difference {bound:.1f} us, a hold by the clock alone {unbounded:.0f} us, form {form}")
    assert bound < 0.5 * unbounded  # the bound tells the two apart
    assert t_slow > t_fast  # holds did happen
    assert t_slow - t_fast <= bound
    torch.cuda.synchronize()
    assert np.array_equal(d_co.cpu().numpy().reshape(1, -1, 512), wanted(oracle, "noise", img, Q_ONES))
    slow.close(), fast.close()


def test_three_images_in_one_launch_on_a_paced_plan(ctx, oracle):
    """(they run the unpaced instance: the dispatcher meters the later images' workgroups in)"""
    w, h = 272, 80
    P = make_plan(ctx, w, h, T_20US, target_wgs=8)
    pinned(P)
    imgs = images_of(w, h)
    batch = [imgs["noise"], imgs["gradient"], imgs["noise"][::-1].copy()]
    got = launch(P, batch, Q_MIXED)
    for k, (name, img) in enumerate(zip(("noise", "gradient", "noise flipped"), batch)):
        assert not np.any(got[k] == SENTINEL), name
        assert np.array_equal(got[k], wanted(oracle, name, img, Q_MIXED)), name
    P.close()


def test_paced_launch_replays_from_a_graph(ctx, oracle):
    """The form keeps no host-side state: a captured launch, replayed three times, transforms what the pixel buffer holds at each replay."""
    import torch

    hip = C.CDLL("libamdhip64.so")
    w, h = 272, 80
    P = make_plan(ctx, w, h, T_20US, target_wgs=8)
    pinned(P)
    imgs = images_of(w, h)
    replays = [("noise", imgs["noise"]), ("gradient", imgs["gradient"]), ("noise", imgs["noise"])]
    d_px = torch.from_numpy(imgs["noise"].reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, 2) == 0  # hipStreamCaptureModeRelaxed
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), Q_MIXED, stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    for name, img in replays:
        d_px.copy_(torch.from_numpy(img.reshape(-1).copy()))
        d_co.fill_(SENTINEL)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_co.cpu().numpy().reshape(1, -1, 512), wanted(oracle, name, img, Q_MIXED)), name
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    P.close()


def test_tuned_plan_measures_paced_candidates_and_stays_right(ctx, oracle):
    import frave_amd as fa

    w, h = 512, 512
    P = fa.Plan(ctx, w, h, 1)
    rep = P.tune_forward(24)
    assert rep["tuned"] is True and rep["winner"] in rep["candidates_us"]
    paced = {k: v for k, v in rep["candidates_us"].items() if k.startswith("wave/") and "/pace" in k}
    assert len(paced) >= 2 and all(v > 0 for v in paced.values()), rep  # paced variants were candidates, whoever won
    print("winner", rep["winner"], "paced candidates_us", paced)
    imgs = images_of(w, h)
    for _ in range(2):  # the measured plan, then the same plan again
        for name, img in imgs.items():
            got = launch(P, [img], Q_ONES)[0]
            assert not np.any(got == SENTINEL), name
            assert np.array_equal(got, wanted(oracle, name, img, Q_ONES)), name
    assert np.array_equal(launch(P, [imgs["noise"]], Q_MIXED)[0], wanted(oracle, "noise", imgs["noise"], Q_MIXED))
    P.close()
