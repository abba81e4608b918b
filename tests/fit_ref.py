"""The width fit's sums (fri_hip_fit_width_sums) restated in numpy BIT FOR BIT, from inputs that involve no GPU code: the oracle's coefficients and
neighbour values, the plan's Some / None bits and its prediction tiles (fri_hip_plan_pred_slots). Written from the definition in include/fri_hip.h:

- a partial sum belongs to (tile, half h, pair group pg, lane); its cells are block rows 2 h and 2 h + 1 of the tile, four columns each, in the order
  C = 0..7: slot (1 + 2 h + (C >> 2)) * 6 + 1 + (C & 3); its nodes are n0 and n0 + 1 (N0 below);
- per cell, first node a then node b: p = v0 x0, p = rn(p + rn(vk xk)), r = |rn(value - p)|, d_j = |v_D0[j] - v_D1[j]|, s0 = rn(rn(s0 + ra) + rb),
  s_{1+j} = fma(da_j, ra, s_{1+j}) then fma(db_j, rb, .); a None node, heap nodes 0 and 1 and an absent cell are all zeros;
- every one of the six f32 sums becomes min(s, 2^24) in 64-bit fixed point with 20 fraction bits (truncated); W^T r[g][k] is the integer total of the
  group's partial sums times 2^-20 as a double.
tests/test_fit_ref_host.py anchors this restatement without the kernel: its W^T W is tests/oracle_ref.cpu_fit_sums' exactly (every row once), its W^T r the
float64 sum to within the roundings stated there."""
import numpy as np

NONE = -(2 ** 31)
FIX_BITS = 20
SATURATE = np.float32(2.0 ** 24)
LANE = np.arange(64)
N0 = np.stack([128 + 2 * LANE, 2 * LANE, 256 + 4 * LANE, 256 + 4 * LANE + 2])  # [pair group][lane]: first node of the pair
GROUP_OF_PG = np.array([1, 2, 0, 0])  # level 7, levels 0..6, level 8, level 8
D0, D1 = [0, 1, 4, 1, 2], [3, 2, 5, 5, 4]
INTERIOR = 0x40000000


def fma32(a, b, c):
    """rn_f32(a * b + c) for float32 arrays, one rounding. The float64 product of two float32 is exact; TwoSum gives the exact error of the float64 add;
    the float64 sum is forced to round-to-odd (a sum that is not exact gets an odd last bit), after which the cast to float32 rounds as if from the exact
    value: 53 bits are more than 24 + 2."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err = p + c exactly
    bits = np.ascontiguousarray(s).view(np.uint64)
    fix = (err != 0) & ((bits & np.uint64(1)) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)  # the exact value lies further from zero than s: the magnitude's bit pattern goes up
    bits = np.where(fix, np.where(away, bits + np.uint64(1), bits - np.uint64(1)), bits)
    return bits.view(np.float64).astype(np.float32)


def block_slot(h, c):
    """slot of cell C = 0..7 of half h inside a tile's 6 x 6 slot square"""
    return (1 + 2 * h + (c >> 2)) * 6 + 1 + (c & 3)


def partial_sums(co, nv, valid, slots, value_params):
    """(s float32 [T][2][4][64][6], wtw int64 [3][6][6]): the f32 partial sums of every (tile, half, pair group, lane), and the integer W^T W.
    co [F][512] coefficients (None = NONE), nv [F][512][6] neighbour values, valid bool [F][512], slots int32 [T][36], value_params [3][6]."""
    co, nv, valid = np.asarray(co), np.asarray(nv), np.asarray(valid, bool)
    slots = np.asarray(slots, np.int64).reshape(-1, 36)
    cell = np.where(slots < 0, -1, slots & (INTERIOR - 1))
    T = cell.shape[0]
    x = np.asarray(value_params, np.float32).reshape(3, 6)[GROUP_OF_PG][None, None, :, None, :]  # [1][1][4][1][6]
    s = np.zeros((T, 2, 4, 64, 6), np.float32)
    wtw = np.zeros((3, 6, 6), np.int64)
    for c in range(8):
        ids = np.stack([cell[:, block_slot(0, c)], cell[:, block_slot(1, c)]], axis=1)  # [T][2]
        at = np.clip(ids, 0, None)[:, :, None, None]
        for second in (0, 1):
            n = (N0 + second)[None, None]  # [1][1][4][64]
            row = (ids >= 0)[:, :, None, None] & valid[at, n] & (n >= 2)  # a row of the fit: a Some node of heap index >= 2 in a retained cell
            v = np.where(row[..., None], nv[at, n], 0).astype(np.float32)  # [T][2][4][64][6]
            own = np.where(row, co[at, n], 0).astype(np.float32)
            p = v[..., 0] * x[..., 0]
            for k in range(1, 6):
                p = p + v[..., k] * x[..., k]  # float32 arrays: every product and every sum rounds once
            r = np.abs(own - p)
            d = np.abs(v[..., D0] - v[..., D1])  # exact: integers below 512
            s[..., 0] = s[..., 0] + r
            s[..., 1:] = fma32(d, r[..., None], s[..., 1:])
            w = np.concatenate([row[..., None].astype(np.float64), d.astype(np.float64)], axis=-1)
            for pg in range(4):
                wp = w[:, :, pg].reshape(-1, 6)
                wtw[GROUP_OF_PG[pg]] += (wp.T @ wp).astype(np.int64)  # float64 holds these sums of integer products (< 2^18 each) exactly
    return s, wtw


def to_fixed(s):
    """(uint64 fixed-point values, saturated flags) of float32 partial sums: min(s, 2^24) with 20 fraction bits, truncated; NaN counts as 2^24"""
    s = np.asarray(s, np.float32)
    fits = s < SATURATE
    v = np.where(fits, s, SATURATE).astype(np.float64)
    return np.floor(v * 2.0 ** FIX_BITS).astype(np.uint64), ~fits  # (the scaling is exact: at most 24 significant bits, 20 places up)


def exact_width_sums(co, nv, valid, slots, value_params):
    """(wtw int64 [3][6][6], wtr_fixed uint64 [3][6], wtr float64 [3][6], n_saturated) as fri_hip_fit_width_sums defines them"""
    s, wtw = partial_sums(co, nv, valid, slots, value_params)
    fixed, sat = to_fixed(s)
    total = np.zeros((3, 6), np.uint64)
    for pg in range(4):
        total[GROUP_OF_PG[pg]] += fixed[:, :, pg].reshape(-1, 6).sum(axis=0, dtype=np.uint64)
    return wtw, total, total.astype(np.float64) * 2.0 ** -FIX_BITS, int(sat.sum())


def oracle_width_sums(W, ch, plan, value_params, nv=None):
    """exact_width_sums for channel ch of the oracle Wavelet W on `plan` (any plan of W's shape, host-only ones included); nv: W.neighbour_values(ch), if
    the caller has it"""
    return exact_width_sums(W.coefficients()[ch], W.neighbour_values(ch) if nv is None else nv, plan.valid_bits(), plan.pred_slots(), value_params)
