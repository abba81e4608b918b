"""Randomised parity on the GPU: shapes (incl. thin and tiny images), contents, channel counts, quantisers and predictor
parameters drawn from a fixed seed, every kernel against the CPU oracle (tests/tools/fuzz_parity.py runs longer sweeps); and the second sweep,
tests/tools/fuzz_later.py, one test per kind: the kernels and plan kinds that came later, against their restatements (the counts: tests/later_cases.py, where
tests/test_later_cases_host.py holds them to what the cases must reach)."""
import pytest

from tests.later_cases import N_CASES, SEED


@pytest.mark.gpu
def test_random_cases_match_the_oracle():
    from tests.tools.fuzz_parity import run

    assert run(80, 20261004) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(N_CASES))
def test_later_kernels_match_their_restatements(kind):
    from tests.tools.fuzz_later import run

    assert run(kind, N_CASES[kind], SEED) == 0
