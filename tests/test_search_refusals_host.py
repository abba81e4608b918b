"""What the quality searches and the tiled host forms refuse, and with which code, before they touch a device (include/fri_hip.h). CPU only, on host-only plans
(ctx = None): a table over the 24 search entry points - three searches (PSNR, SSIM, size) x four plan kinds (ordinary, 4:2:0, tiled, tiled 4:2:0) x the host
and the _dev form - and over fri_hip_estimate_size_tiled*, fri_hip_encode_image_tiled*_coded:

- every pointer argument null in turn: -1, also on a plan without a device;
- a target that is NaN, 0 or negative, an SSIM target above 1, max_bytes == 0: -1;
- the SSIM searches on an image under 8 pixels wide or high: -1, before the device is asked for;
- the reversible colour transform on the ordinary and the tiled kind: -1;
- an otherwise valid call: -3, no device."""
import ctypes as C

import numpy as np
import pytest

from frave_amd import api

INVALID, NO_DEVICE = -1, -3
W = H = 16
TILE = 8
NAN = float("nan")

KINDS = {  # suffix of the entry points, the plan on W x H, the plan on w x h for the SSIM shape refusal
    "": lambda w, h: api.Plan(None, w, h, 3),
    "420": lambda w, h: api.Plan420(None, w, h),
    "_tiled": lambda w, h: api.PlanTiled(None, w, h, 3, TILE, TILE, api.TILED_ALLOW_HOLES),
    "_tiled420": lambda w, h: api.PlanTiled420(None, w, h, TILE, TILE, api.TILED_ALLOW_HOLES),
}
SEARCHES = {  # stem of the entry points: (the target's ctype, a good target, the refused targets)
    "fri_hip_search_quality": (C.c_double, 30.0, (NAN, 0.0, -1.0)),
    "fri_hip_search_quality_ssim": (C.c_double, 0.9, (NAN, 0.0, -0.5, 1.5)),
    "fri_hip_search_quality_for_size": (C.c_uint64, 10 ** 6, (0,)),
}
ENTRY_POINTS = [(stem, kind, dev) for stem in SEARCHES for kind in KINDS for dev in (False, True)]
assert len(ENTRY_POINTS) == 24


@pytest.fixture(scope="module")
def plans():
    made = {kind: make(W, H) for kind, make in KINDS.items()}
    yield made
    for p in made.values():
        p.close()


def _call(stem, kind, dev, plan, target=None, null=None, pixels=None):
    """the return code of one search call; null: the index of the pointer argument to pass as NULL (0 the plan, 1 the pixels, 2 the quality, 3 the value)"""
    ctype, good, _ = SEARCHES[stem]
    fn = getattr(api.load_library(), stem + kind + ("_dev" if dev else ""))
    px = np.zeros((plan.height, plan.width, 3), np.uint8) if pixels is None else pixels
    quality, value = C.c_int32(-7), ctype(0)
    # (a _dev form never reads its pixels here: any non-null address stands for a device pointer)
    args = [plan._h, C.c_void_p(4096) if dev else px.ctypes.data_as(C.c_void_p), C.cast(C.byref(quality), C.c_void_p), C.cast(C.byref(value), C.c_void_p)]
    if null is not None:
        args[null] = None
    rc = fn(args[0], args[1], ctype(good if target is None else target), args[2], args[3], *([None] if dev else []))
    assert quality.value == -7, "a refused search wrote its output"
    return rc


@pytest.mark.parametrize("stem,kind,dev", ENTRY_POINTS)
def test_search_refusals(plans, stem, kind, dev):
    plan = plans[kind]
    for null in range(4):
        assert _call(stem, kind, dev, plan, null=null) == INVALID, null
    for target in SEARCHES[stem][2]:
        assert _call(stem, kind, dev, plan, target=target) == INVALID, target
    assert _call(stem, kind, dev, plan) == NO_DEVICE


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dev", (False, True))
def test_ssim_search_refuses_an_image_without_a_window_before_it_asks_for_the_device(kind, dev):
    for w, h in ((7, 16), (16, 7)):
        small = KINDS[kind](w, h)
        assert _call("fri_hip_search_quality_ssim", kind, dev, small) == INVALID, (w, h)
        assert _call("fri_hip_search_quality", kind, dev, small) == NO_DEVICE, (w, h)  # (only SSIM needs a window)
        small.close()


@pytest.mark.parametrize("kind", ("", "_tiled"))
def test_searches_refuse_the_reversible_colour_transform(kind):
    plan = KINDS[kind](W, H)
    inner = plan.tile if kind else plan
    for mode, want in ((api.COLOUR_RCT, INVALID), (api.COLOUR_YCBCR, NO_DEVICE), (api.COLOUR_NONE, NO_DEVICE)):
        inner.set_colour_transform(mode)
        for stem in SEARCHES:
            for dev in (False, True):
                assert _call(stem, kind, dev, plan) == want, (mode, stem, dev)
    plan.close()


# ---- the tiled host forms: the size estimate and the coded encode -------------------------------------------------------------------------------------------

def _tiled_forms(kind, plan):
    """(name, argument list, {index of a pointer argument: the code when it is NULL on a host-only plan}) of the kind's two host forms"""
    n = plan.n_tiles
    planes = 3 * n
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = [np.zeros((planes, 10, 1024), np.uint32), np.zeros(planes, np.uint64), np.zeros(1, np.uint64), np.zeros(n, np.uint64), np.zeros((H, W, 3), np.uint8),
            np.ones(32, np.int32), np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 3, 6), np.float32), np.zeros((planes, 64), np.uint32), np.zeros(planes, np.uint32),
            np.zeros((planes, 10, 4), np.uint32), np.zeros((planes, 10, 1024), np.uint16), np.zeros((planes, 4), np.uint32)]
    hist, oob, total, tiles, px, qm, vp, wp, words, n_words, models, off, status = keep
    quality = C.c_int(50) if kind == "_tiled420" else P(qm)  # (the 4:4:4 form takes a matrix, a pointer; the 4:2:0 form a quality)
    # the estimate looks at its arguments first (the counts and the tiles' bytes are optional), the coded form at the device first
    estimate = ("fri_hip_estimate_size" + kind, [plan._h, P(hist), P(oob), P(total), P(tiles)], {0: INVALID, 1: INVALID, 2: NO_DEVICE, 3: INVALID, 4: NO_DEVICE})
    coded = ("fri_hip_encode_image" + kind + "_coded", [plan._h, P(px), quality, P(vp), P(wp), P(words), C.c_size_t(64), P(n_words), P(models), P(off), P(status)],
             {0: INVALID, **{k: NO_DEVICE for k in (1, 3, 4, 5, 7, 8, 9, 10) + (() if kind == "_tiled420" else (2,))}})
    return keep, (estimate, coded)


@pytest.mark.parametrize("kind", ("_tiled", "_tiled420"))
def test_tiled_host_forms_refusals(plans, kind):
    plan = plans[kind]
    L = api.load_library()
    keep, forms = _tiled_forms(kind, plan)
    for name, args, nulls in forms:
        fn = getattr(L, name)
        assert fn(*args) == NO_DEVICE, name
        for k, want in nulls.items():
            assert fn(*args[:k], None, *args[k + 1:]) == want, (name, k)
    if kind == "_tiled420":  # (a quality outside 1..99 is refused behind the device check)
        name, args, _ = forms[1]
        assert getattr(L, name)(*args[:2], C.c_int(0), *args[3:]) == NO_DEVICE
    del keep
