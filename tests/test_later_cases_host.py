"""What the later kernels' cases reach, checked on the host (CPU only): the launch arithmetic of K7 and K10 and the strip classes of K8, K10 and K12, restated in
tests/later_cases.py from the kernels' constants; the deterministic cases of test_gpu_ssim.py, test_gpu_tiled_search.py and test_gpu_chroma420.py reach exactly
the cells they are there for; the fixed-seed dry run of every kind of tests/tools/fuzz_later.py, with the case counts test_gpu_fuzz.py uses, reaches every strip
class of its kernels, skips nothing and draws only what the headers document as valid."""
import functools

import pytest

from tests import later_cases as LC
from tests.tools import fuzz_later as F


# ---- the restated arithmetic on shapes whose answer is known ---------------------------------------------------------------------------------------------------

def test_k7_arithmetic_on_the_shapes_of_the_fixed_list():
    """the band is 4 on every shape tests/test_gpu_ssim.py had before these cases, its n-image form included"""
    for w, h, n in [(8, 8, 1), (9, 13, 1), (8, 300, 1), (300, 9, 1), (640, 480, 1), (1001, 613, 1), (4096, 4096, 1), (2048, 1536, 1), (300, 9, 3), (640, 480, 3), (1001, 613, 3)]:
        assert LC.k7_launch(w, h, n)["band"] == 4, (w, h, n)
    L = LC.k7_launch(4096, 4096, 1)
    assert (L["bx"], L["nx"], L["ny"], L["n_strips"], L["unclamped"]) == (1024, 1023, 1023, 8, 2)
    assert {LC.k7_launch(w, 8, 1)["bx"] for w in (8, 300, 640, 1001, 2048, 4096)} == {2, 75, 160, 250, 512, 1024}


def test_k10_arithmetic_on_the_largest_shape_of_the_fixed_list():
    G = LC.k10_grid(1023, 767, 3, 512, 512)
    assert (G["groups"], G["per_lane"], G["groups"] % G["per_lane"]) == (768, 2, 0)
    assert LC.k10_measure_cells(1023, 767, 3, 512, 512) == {"1<per_lane<32"}


# ---- the deterministic cases -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", LC.SSIM_BAND_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_ssim_band_cases_reach_their_cells(case):
    (w, h, c, n), want = case
    L = LC.k7_launch(w, h, n)
    got = LC.k7_cells(w, h, n)
    assert want <= got, (L, got)
    assert not {"band=4"} & got
    if "4<band<64" in want:
        assert 4 < L["band"] < 64 and L["ny"] % L["band"] != 0
    else:
        assert L["band"] == 64 and L["ny"] * L["n_strips"] * n > 63 * 4096 and L["unclamped"] > 64
    assert w * h * c * n <= 20 << 20  # a few MB per raster


def test_ssim_edge_shapes_reach_both_remainders_for_both_channel_counts():
    got = {(c, LC.k7_launch(w, h)["bx"] % 128) for w, h, c in LC.SSIM_EDGE_SHAPES}
    assert got == {(1, 1), (1, 2), (3, 1), (3, 2)}
    for w, h, c in LC.SSIM_EDGE_SHAPES:
        cells = LC.k7_cells(w, h)
        if LC.k7_launch(w, h)["bx"] % 128 == 1:
            assert "last strip full, its third block the row's last" in cells and LC.k7_launch(w, h)["n_strips"] == 1
        else:
            assert "last strip: a single lane with 2 blocks" in cells and "a full strip" in cells


def test_measure_cases_reach_the_ragged_round_and_the_clamp():
    shape, want = LC.MEASURE_RAGGED
    G = LC.k10_grid(*shape)
    assert LC.k10_measure_cells(*shape) == want and G["per_lane"] > 1 and G["groups"] % G["per_lane"] != 0
    shape, want = LC.MEASURE_CLAMPED
    G = LC.k10_grid(*shape)
    w, h, c, tw, th = shape
    assert want <= LC.k10_measure_cells(*shape) and G["groups"] > 16384 and c == 1 and G["nx"] * G["ny"] * tw * th > 64 << 20
    # the kernel's 32-bit partial sums at the worst case, every difference 255: a lane, then a wave
    lane = LC.K10_MEASURE_STRIPS * LC.K10_STRIP * 255 * 255
    assert lane < 1 << 25 and 64 * lane < 1 << 31


def test_saturated_420_case_fills_whole_workgroups_with_whole_strips():
    w, h = LC.C420_SATURATED
    assert w % LC.K8_STRIP == 0 and (w // LC.K8_STRIP * h) % LC.K8_THREADS == 0 and w // LC.K8_STRIP * h > LC.K8_THREADS
    assert LC.K8_THREADS * LC.K8_STRIP * 255 * 255 < 1 << 29  # the kernel's bound on a workgroup's sum


# ---- the sweep's dry run ---------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dry(kind):
    return F.sweep(kind, LC.N_CASES[kind], LC.SEED, dry=True)


REQUIRED = {
    "ycbcr": set(),
    "ssim": F.SSIM_CELLS,
    "rate": {"synthetic histograms", "the chain's histograms", "C1", "C3"},
    "c420": LC.K8_CELLS | {"composed encode"},
    "rgba": F.RGBA_CELLS,
    "tiled": LC.K10_CELLS | LC.K10_REGION_CELLS | {"C%d region: touches the last row and column" % c for c in (1, 3)} | {"C%d: composed encode" % c for c in (1, 3)},
    "tiled420": LC.K12_SPLIT_CELLS | LC.K12_REGION_CELLS | {"region: %s x, %s y" % (a, b) for a in ("odd", "even") for b in ("odd", "even")} | {"composed encode"},
    "rans": {"a refused plane", "every plane coded", "streams further than their length apart", "streams no further than their length apart"},
    "decode": F.DECODE_CELLS,  # every cell of tests/decode_cases.py, both tile shapes, every level, family and symbol rule
}


def test_every_kind_has_a_count_and_a_stream_of_its_own():
    assert set(LC.N_CASES) == set(F.KINDS) == set(REQUIRED)
    assert all(n >= 40 for n in LC.N_CASES.values())
    ks = [v[0] for v in F.KINDS.values()]
    assert len(set(ks)) == len(ks) and 1 not in ks[1:] and all(k >= 1 for k in ks)


@pytest.mark.parametrize("kind", sorted(F.KINDS))
def test_dry_run_reaches_every_cell_and_draws_only_valid_cases(kind):
    bad, reached, cases = _dry(kind)
    assert bad == 0 and len(cases) == LC.N_CASES[kind]  # every case drawn, none skipped
    missing = REQUIRED[kind] - reached
    assert not missing, sorted(missing)
    for i, p in enumerate(cases):
        assert F.violated(kind, p) == [], (kind, i, p)
    if kind in ("c420", "rgba", "tiled", "tiled420"):  # the composed encode on one case in four
        assert sum(p["composed"] for p in cases) == (len(cases) + 3) // 4
    if kind == "decode":  # the count is the smallest that reaches every cell: one case fewer misses one
        assert LC.N_CASES[kind] == 40 or REQUIRED[kind] - F.sweep(kind, LC.N_CASES[kind] - 1, LC.SEED, dry=True, only=-1)[1]
    if kind == "rans":
        p = next(p for p in cases if p["inject"] == "bad")  # an injected entry makes the reference refuse that plane, and only that one
        assert [bool(r.status) for r in F._rans_ref(p)["refs"]] == [k == p["inject_plane"] for k in range(p["planes"])]


def test_a_new_kind_moves_no_other_kinds_draws():
    """a kind's cases depend on its own stream only: the first cases of a shorter sweep are those of the full one"""
    for kind in ("ssim", "tiled420"):
        assert F.sweep(kind, 5, LC.SEED, dry=True, only=-1)[2] == _dry(kind)[2][:5]
