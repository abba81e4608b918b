"""The grid and tile-walk table of tests/test_gpu_predict_walks.py, checked on the host: every coverage case makes the K2 / K4 launches it claims (by the
launchers' rules, restated in tests/predict_cases.py from host-only plans), the cases together reach every cell of the matrix and each is needed, and the
restated walks hand out every tile exactly once. CPU only."""
import numpy as np
import pytest

from tests.predict_cases import (CASES, COVERAGE, GRID_KNOBS, covered_cells, grid_size, k2_walks, k4_walks, knobs, launches, required_cells, split_active,
                                 walk_is_a_partition)
from tests.instance_cases import ALL_KNOBS


def _claim(case):
    import frave_amd as fa

    with knobs(case.env()):
        P = fa.Plan(None, *case.shape)
    grid, F = P.predict_grid(), P.num_cells
    P.close()
    return grid, launches(case, grid, F)


@pytest.fixture(scope="module")
def predictions():
    return {case.id: _claim(case) for case in CASES}


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_grid_knobs_are_reset_between_cases():
    assert set(GRID_KNOBS) <= set(ALL_KNOBS)


def test_host_only_plan_reports_the_pinned_grid(predictions):
    for case in COVERAGE:
        grid, _ = predictions[case.id]
        assert (grid["pred_blocks"], grid["hist_blocks"], grid["k4_older_eighths"]) == case.grid, case.id
        assert grid["n_pred_tiles"] > 0, case.id


@pytest.mark.parametrize("case", COVERAGE, ids=lambda c: c.id)
def test_case_reaches_its_claim(case, predictions):
    assert predictions[case.id][1] == case.claim


def test_cases_cover_the_matrix():
    got = covered_cells([(case, case.claim) for case in COVERAGE])
    for name, want in required_cells().items():
        assert want <= got[name], (name, sorted(want - got[name], key=str))


def test_every_coverage_case_is_needed():
    """no case is redundant: without any one of them some cell of the matrix is no longer reached"""
    req = required_cells()
    for i, case in enumerate(COVERAGE):
        rest = covered_cells([(c, c.claim) for j, c in enumerate(COVERAGE) if j != i])
        assert any(not (req[k] <= rest[k]) for k in req), case.id


def test_default_cases_claim_nothing(predictions):
    defaults = [c for c in CASES if not c.pinned]
    assert defaults and all(c.claim == () and c.env() is None for c in defaults)
    for c in defaults:  # a host-only plan without knobs knows the tiles but no grid: the device decides
        grid, _ = predictions[c.id]
        assert (grid["pred_blocks"], grid["hist_blocks"], grid["k4_older_eighths"]) == (0, 0, 0), c.id
    assert all(c.shape[0] * c.shape[1] * c.n_images <= 1 << 20 for c in CASES)  # at most a megapixel


def test_case_walks_hand_out_every_tile_once(predictions):
    for case in CASES:
        grid, claim = predictions[case.id]
        n = grid["n_pred_tiles"]
        for L in claim:
            if L[0] == "k2":
                assert walk_is_a_partition(k2_walks(n, L[2]), n), case.id
            elif L[0] == "k4":
                assert walk_is_a_partition(k4_walks(n, L[4], L[6]), n), case.id


def test_walks_hand_out_every_tile_once_over_a_sweep():
    for n in list(range(1, 70)) + [127, 159, 160, 161, 1000, 4097]:
        for limit in list(range(1, 41)) + [64, 96, 128, 256, 512]:
            for planes in (1, 2, 3, 8):
                G, _ = grid_size(n, limit, planes)
                assert 1 <= G <= min(n, limit), (n, limit, planes)
                assert walk_is_a_partition(k2_walks(n, G), n), (n, G)
                for e in range(0, 9):
                    split = e if split_active(n, G, planes, limit, e) else 0
                    assert walk_is_a_partition(k4_walks(n, G, split), n), (n, G, e)
