"""tests/fit_ref.py - the bit-exact numpy restatement of the width fit's sums that the GPU tests compare W^T r with - anchored without the kernel: its
fused multiply-add against rational arithmetic, the prediction tiles it walks (fri_hip_plan_pred_slots) against the plan's other getters, its W^T W
against the plain sums over the oracle's neighbour values (every row exactly once) and its W^T r against the float64 sum. No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

from tests import fit_ref
from tests.common import gen_image, random_params
from tests.oracle_ref import cpu_fit_sums

SATURATION_SHAPE, SATURATION_SEED, SATURATION_SCALE = (320, 200, 1), 6, 2048.0  # the GPU suite's saturation case (tests/test_gpu_fit.py)


def plan(w, h, c):
    import frave_amd

    return frave_amd.Plan(None, w, h, c)


def saturating_params():
    """value parameters of ordinary shape, scaled so that residuals reach ~1e5: on noise the level-8 partial sums stay below 2^24, some of levels 0..7 do not"""
    vp, _ = random_params(3, scale=0.2)
    return (vp * np.float32(SATURATION_SCALE)).astype(np.float32)


# ---- fma32 --------------------------------------------------------------------------------------------------------------------------------------------
def _round_f32(x):
    """the float32 nearest to the Fraction x, ties to even"""
    near = np.float32(float(x))
    cands = sorted({float(near), float(np.nextafter(near, np.float32(-np.inf))), float(np.nextafter(near, np.float32(np.inf)))})
    best = min(abs(Fraction(c) - x) for c in cands)
    tied = [c for c in cands if abs(Fraction(c) - x) == best]
    if len(tied) > 1:
        tied = [c for c in tied if (int(np.float32(c).view(np.uint32)) & 1) == 0]
    assert len(tied) == 1
    return np.float32(tied[0])


def _check_fma(a, b, c):
    a, b, c = (np.asarray(v, np.float32) for v in (a, b, c))
    got = fit_ref.fma32(a, b, c)
    for k in range(a.size):
        want = _round_f32(Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k])))
        assert got[k].view(np.uint32) == want.view(np.uint32), (float(a[k]).hex(), float(b[k]).hex(), float(c[k]).hex(), float(got[k]).hex(), float(want).hex())


def test_fma32_on_drawn_inputs():
    rng = np.random.default_rng(1)
    n = 6000
    # the kernel's operands (integer features, residuals, sums of them) and operands of unrelated magnitudes and signs
    _check_fma(rng.integers(0, 512, n), np.abs(rng.normal(0, 40, n)), np.abs(rng.normal(0, 3000, n)))
    _check_fma(rng.normal(0, 1, n) * 2.0 ** rng.integers(-20, 20, n), rng.normal(0, 1, n) * 2.0 ** rng.integers(-20, 20, n),
               rng.normal(0, 1, n) * 2.0 ** rng.integers(-30, 30, n))
    # products that cancel all but the last bits of c
    a, b = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    _check_fma(a, b, -(a * b))


def test_fma32_on_constructed_ties():
    assert 8392705 * 8384513 == 2 ** 46 + 1 and max(8392705, 8384513) < 2 ** 24
    eps = 2.0 ** -23
    a, b, c = [], [], []
    for k in (-10, 0, 1, 7, 23, 30):
        for sign in (1.0, -1.0):
            one = sign * 2.0 ** k
            half_ulp = 2.0 ** (k - 24)
            cases = [
                (half_ulp, 1.0, one),  # c a power of two, a b = half an ulp of c: the tie goes to c (even)
                (half_ulp, 1.0 + eps, one),  # just above the tie: c + ulp
                (half_ulp, 1.0, one * (1.0 + eps)),  # c odd: the tie goes up
                (half_ulp * (1.0 - eps), 1.0 + eps, one * (1.0 + eps)),  # 2^-46 below the tie: a float64 sum rounded to nearest lands ON it and then goes up
                (half_ulp * 8392705 * 2.0 ** -23, 8384513 * 2.0 ** -23, one),  # 2^-46 above the tie: ... lands on it and then goes down
                (-half_ulp / 2, 1.0, one),  # below a power of two the spacing halves: a tie again
                (-half_ulp / 2 * (1.0 + eps), 1.0, one),
            ]
            for x, y, z in cases:
                a.append(sign * x), b.append(y), c.append(z)
    _check_fma(a, b, c)
    # the two cases a double rounding gets wrong are among them: the helper must differ from the plain float64 expression there
    naive = (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)
    assert (naive != fit_ref.fma32(a, b, c)).sum() >= 2 * 6 * 2


# ---- the prediction tiles -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(10, 10, 1), (3, 300, 1), (128, 96, 3), (320, 200, 1), (700, 500, 3)])
def test_pred_slots(shape):
    P = plan(*shape)
    F = P.num_cells
    raw = P.pred_slots()
    assert raw.shape == (P.predict_grid()["n_pred_tiles"], 36) and raw.dtype == np.int32
    cell = np.where(raw < 0, -1, raw & (fit_ref.INTERIOR - 1)).reshape(-1, 6, 6)
    assert ((raw == -1) | ((raw >= 0) & (cell.reshape(-1, 36) < F))).all()
    # every cell is a block cell of exactly one tile, and every tile has one
    inner = cell[:, 1:5, 1:5].reshape(len(cell), -1)
    assert sorted(inner[inner >= 0].tolist()) == list(range(F))
    assert (inner >= 0).any(axis=1).all()
    # the slots the restatement walks are the sixteen block cells, each once
    walked = sorted(fit_ref.block_slot(h, c) for h in range(2) for c in range(8))
    assert walked == sorted(6 * i + j for i in range(1, 5) for j in range(1, 5))
    # the interior flag, the same in every slot that holds the cell: all 512 leaves inside the image. The kernels do not mask such a cell, so all its
    # coefficients must be Some (a cell that misses a leaf or two can have all of them Some as well: it is masked with all ones); a cell whose 46 x 21
    # bounding box of leaves lies inside the image is one
    has = raw >= 0
    ids, flags = cell.reshape(-1, 36)[has], (raw[has] & fit_ref.INTERIOR) != 0
    flagged = np.zeros(F, bool)
    flagged[ids] = flags
    assert np.array_equal(flagged[ids], flags)
    assert int(flagged.sum()) == P.num_interior_cells
    assert P.valid_bits()[flagged].all()
    cen, (w, h, _) = P.centers(), shape
    inside = (cen[:, 0] - 15 >= 0) & (cen[:, 0] + 30 < w) & (cen[:, 1] - 8 >= 0) & (cen[:, 1] + 12 < h)
    assert flagged[inside].all() and (shape[0] < 320 or inside.any())
    # halo and block slots alike hold the lattice: a slot's six neighbour cells (neighbour_cells()) sit at six fixed distances inside the square
    nb = P.neighbour_cells()
    assert np.array_equal(nb[:, 0], np.arange(F))
    big = plan(700, 500, 1)
    bcell = np.where(big.pred_slots() < 0, -1, big.pred_slots() & (fit_ref.INTERIOR - 1)).reshape(-1, 6, 6)
    bnb = big.neighbour_cells()
    t = int(np.flatnonzero((bcell >= 0).all(axis=(1, 2)))[0])  # a tile without holes gives the distances
    delta = []
    for k in range(1, 7):
        where = np.argwhere(bcell[t] == bnb[bcell[t, 2, 2], k])
        assert len(where) == 1
        delta.append((int(where[0, 0]) - 2, int(where[0, 1]) - 2))
    assert len(set(delta)) == 6 and all(max(abs(a), abs(b)) == 1 for a, b in delta)
    checked = 0
    for k, (da, db) in enumerate(delta, start=1):
        for i in range(max(0, -da), min(6, 6 - da)):
            for j in range(max(0, -db), min(6, 6 - db)):
                here, there = cell[:, i, j], cell[:, i + da, j + db]
                m = here >= 0
                assert np.array_equal(nb[here[m], k], there[m]), (k, i, j)
                checked += int(m.sum())
    assert checked > 0


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(100, 37, 1), (300, 200, 3)])
@pytest.mark.parametrize("kind", ["noise", "smooth", "const"])
def test_restatement_counts_every_row_once_and_sums_to_the_float64_total(oracle, shape, kind):
    w, h, c = shape
    img = gen_image(kind, w, h, c, 21)
    P = plan(w, h, c)
    W = oracle.Wavelet(img, h, w, c)
    F = P.num_cells
    for ch in range(c):
        vp, _ = random_params(3 + ch, scale=0.2)
        _, want_wtw, want_wtr = cpu_fit_sums(oracle, W, ch, vp)
        wtw, fixed, wtr, n_sat = fit_ref.oracle_width_sums(W, ch, P, vp)
        assert np.array_equal(wtw, want_wtw)  # all three groups: every row of the fit once, none twice
        assert n_sat == 0
        assert np.array_equal(wtr, fixed.astype(np.float64) * 2.0 ** -20)
        # a partial sum is 16 f32 additions (17 roundings of 2^-24 relative) and one truncation below 2^-20, at most 32 partial sums per cell and group
        assert np.allclose(wtr, want_wtr, rtol=1e-6, atol=1e-3 + F * 32 * 2.0 ** -20), (ch, np.abs(wtr - want_wtr).max())
    W.close()


def test_the_saturation_case_saturates_some_partial_sums_and_not_others(oracle):
    w, h, c = SATURATION_SHAPE
    P = plan(w, h, c)
    W = oracle.Wavelet(gen_image("noise", w, h, c, SATURATION_SEED), h, w, c)
    s, _ = fit_ref.partial_sums(W.coefficients()[0], W.neighbour_values(0), P.valid_bits(), P.pred_slots(), saturating_params())
    W.close()
    assert np.isfinite(s).all()
    assert (s >= 2.0 ** 24).any() and ((s > 0) & (s < 2.0 ** 24)).any()
    fixed, sat = fit_ref.to_fixed(s)
    assert (fixed[sat] == 1 << 44).all() and (fixed[~sat] < 1 << 44).all()
