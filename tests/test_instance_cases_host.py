"""The instance table of tests/test_gpu_instances.py, checked on the host: every coverage case reaches the K1 / K3 instance it claims (by the launchers' rules,
restated in tests/instance_cases.instance_of from host-only plans), and together the cases reach every cell of the instance matrix. CPU only."""
import numpy as np
import pytest

from tests.instance_cases import BASE_KNOBS, CASES, COVERAGE, covered_cells, instance_of, knobs, plan_facts, required_cells
from tests.oracle_ref import oracle_owned


def _predict(case, oracle):
    import frave_amd as fa

    w, h, c = case.shape
    with knobs(case.env()):
        P = fa.Plan(None, w, h, c)
    facts = plan_facts(P)
    P.close()
    return instance_of(case, facts, not oracle_owned(oracle, w, h, c).all())


@pytest.fixture(scope="module")
def predictions(oracle):
    return {case.id: _predict(case, oracle) for case in COVERAGE}


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_coverage_cases_pin_the_tiling_and_the_shared_inverse_tiling():
    """instance_of reads the forward tiling of a host-only plan: valid for what ran only with the tiling pinned and K3 on the forward tiling"""
    for case in COVERAGE:
        env = case.env()
        assert env["FRI_HIP_INV_SHARED"] == "1" and env["FRI_HIP_TUNING"] == "1", case.id
        assert all(env[k] == v for k, v in BASE_KNOBS.items()), case.id
        assert "FRI_HIP_BAND_ROWS" in env and "FRI_HIP_CELLS_PER_TILE" in env, case.id
        assert case.claim is not None, case.id
    for case in CASES:
        if not case.pinned:
            assert case.claim is None and case.env() is None, case.id


@pytest.mark.parametrize("case", COVERAGE, ids=lambda c: c.id)
def test_case_reaches_its_instance(case, predictions):
    assert predictions[case.id] == case.claim


def test_cases_cover_the_matrix(predictions):
    got = covered_cells([(case, predictions[case.id]) for case in COVERAGE])
    for name, want in required_cells().items():
        assert want <= got[name], (name, sorted(want - got[name], key=str))


def test_every_coverage_case_is_needed(predictions):
    """no case is redundant: without any one of them some cell of the matrix is no longer reached"""
    req = required_cells()
    for i, case in enumerate(COVERAGE):
        rest = covered_cells([(c, predictions[c.id]) for j, c in enumerate(COVERAGE) if j != i])
        assert any(not (req[k] <= rest[k]) for k in req), case.id


def test_default_cases_run_on_default_plans():
    defaults = [c for c in CASES if not c.pinned]
    assert {c.kind for c in defaults} == {"k1", "c16", "k3", "measure"}
    assert any(c.shape == (4096, 4096, 1) and c.kind == "measure" and c.deq == 2 for c in defaults)  # the one large MID + MEASURE case
    assert all(np.prod(c.shape) < 1 << 20 for c in CASES if c.shape != (4096, 4096, 1))
