"""The K2 / K4 grid and tile-walk matrix as a table of cases (tests/test_gpu_predict_walks.py runs them, tests/test_predict_cases_host.py checks what they
reach).

launch_predict_histogram (frave_amd/csrc/k2_predict.hip) and launch_fit_accumulate (k4_fit.hip) size their grids from the plan's prediction tiles and two
grid limits (FRI_HIP_PRED_BLOCKS, FRI_HIP_HIST_BLOCKS; by default the CU count and twice that), pick one template instance from the entry point's trust and
buffers, and every workgroup walks its tiles by PredTileWalk (gather_common.hpp) - K4 on a full one-plane grid by its older / younger split instead
(FRI_HIP_K4_OLDER_EIGHTHS). This module restates those rules from what a host-only plan exposes (fri_hip_plan_predict_grid), so that each case can claim
the launches it makes: a tuple of

    ("k2", instance, G, n_planes, share, max tiles, min tiles)      instance: "<CHECK><WORDS><C16><STREAM>" as T / F; share: "one", "eighth", "share"
    ("exact", G, n_planes)                                          exact_predict_kernel behind K2 on coefficients nobody vouched for
    ("k4", mode, check, c16, G, n_planes, eighths, max, min)        eighths: the split's share of the older workgroup, 0 when the split is off
    ("tail", mode)                                                  the chains' solve in the tail of K4
    ("solve", mode)                                                 fit_solve_kernel (fri_hip_fit_{value,width}_params_batch_dev)

Coverage cases pin FRI_HIP_TUNING=1 and the three grid knobs, so a host-only plan knows the grid a device plan launches. Default cases (`pinned = False`)
run on default plans, as users do, and claim nothing.
"""
from dataclasses import dataclass, field

import numpy as np

from tests.instance_cases import knobs  # noqa: F401  (the GPU module and the host test set the knobs through it)

ROUTES = {
    # route: (K2 instance, K4 instances (check, c16) when the case fits, planes per image: C, or the case's n_planes)
    "predict": ("TFFF", None),  # fri_hip_predict_histogram_batch_dev, any int32 coefficients: CHECK + the exact kernel
    "predict_pp3": ("TFFF", None),  # fri_hip_predict_image(fit = 0): the C planes' parameters travel in the launch (pp3)
    "predict_assume": ("TFFF", None),  # the same behind fri_hip_plan_assume_forward_coefficients: still CHECK (trusted), no exact kernel
    "encode_batch": ("FFFF", (False, False)),  # fri_hip_encode_image_batch_dev
    "symbols_words": ("FTFF", (False, False)),  # fri_hip_encode_symbols_batch_dev with d_coefs and d_node_words
    "symbols_compact": ("FTTF", (False, True)),  # ... d_coefs = NULL: the compact int16 planes
    "symbols_direct": ("FTTT", (False, True)),  # ... d_node_words = NULL as well: the scan writes the streams
    "fit_sums": (None, (True, False)),  # fri_hip_fit_{value,width}_sums_batch_dev + fri_hip_fit_{value,width}_params_batch_dev
    "fit_chain": (None, (True, False)),  # fri_hip_fit_params_batch_dev: the sums with the solve in their tail, CHECK
}
GRID_KNOBS = ("FRI_HIP_PRED_BLOCKS", "FRI_HIP_HIST_BLOCKS", "FRI_HIP_K4_OLDER_EIGHTHS")


@dataclass
class Case:
    id: str
    route: str
    shape: tuple  # (width, height, channels)
    n_images: int = 1  # images of an encode route, planes of the predict / fit routes (times C)
    grid: tuple = None  # (pred_blocks, hist_blocks, older eighths); None: a default plan, no claim
    fit: bool = False  # the encode routes: with the device-side fit
    inexact: int = 0  # coefficients outside [-256, 255] injected per plane (predict / fit routes)
    claim: tuple = ()
    seed: int = 0
    note: str = field(default="", compare=False)

    @property
    def pinned(self):
        return self.grid is not None

    def env(self):
        if not self.pinned:
            return None
        return {"FRI_HIP_TUNING": "1", "FRI_HIP_PRED_BLOCKS": str(self.grid[0]), "FRI_HIP_HIST_BLOCKS": str(self.grid[1]),
                "FRI_HIP_K4_OLDER_EIGHTHS": str(self.grid[2])}

    @property
    def n_planes(self):
        return self.n_images * self.shape[2]


# ---- the launchers' rules, restated -------------------------------------------------------------------------------------------------------------------
def grid_size(n_tiles, limit, n_planes):
    """launch_predict_histogram / launch_fit_accumulate: (workgroups per plane, which branch of the rule sized it)"""
    blocks, share = min(n_tiles, limit), "one"
    if n_planes > 1:  # a plane on an eighth of the machine
        per, eighth = (n_tiles + 7) // 8, max(limit // 8, 1)
        share = "share" if per >= eighth else "eighth"
        blocks = min(max(per, eighth), limit, n_tiles)
    return max(blocks, 1), share


def pred_walk(n_tiles, G, b):
    """PredTileWalk: the tiles workgroup b of G walks"""
    groups = min(G, 8)
    xcd, wg_in_xcd = b % groups, b // groups
    step = (G - xcd + groups - 1) // groups
    first = n_tiles * xcd // groups + wg_in_xcd
    end = n_tiles * (xcd + 1) // groups
    return list(range(first, end, step))


def split_active(n_tiles, G, n_planes, hist_blocks, eighths):
    """k4_fit.hip: the older / younger split runs for one plane on a full grid (hist_blocks <= tiles) of a multiple of 16 workgroups"""
    return n_planes == 1 and hist_blocks <= n_tiles and eighths > 0 and G >= 16 and G % 16 == 0


def k4_split_walk(n_tiles, G, b, eighths):
    """the split: workgroups b and b + G / 2 of an XCD range walk one strided sequence, the older its first eighths / 8 (rounded up at 5/8)"""
    per_xcd = G // 8
    pairs = per_xcd // 2
    xcd, in_xcd = b % 8, b // 8
    pair, younger = in_xcd % pairs, in_xcd // pairs
    lo, hi = n_tiles * xcd // 8, n_tiles * (xcd + 1) // 8
    n_pair = (hi - lo - pair + pairs - 1) // pairs if lo + pair < hi else 0
    n_older = min(n_pair, (n_pair * eighths + 3) // 8)
    first = lo + pair + (n_older * pairs if younger else 0)
    end = hi if younger else min(hi, lo + pair + n_older * pairs)
    return list(range(min(first, end), end, pairs))


def k2_walks(n_tiles, G):
    return [pred_walk(n_tiles, G, b) for b in range(G)]


def k4_walks(n_tiles, G, split_eighths):
    if split_eighths:
        return [k4_split_walk(n_tiles, G, b, split_eighths) for b in range(G)]
    return [pred_walk(n_tiles, G, b) for b in range(G)]


def exact_grid(F, G):
    return max(min(F, G), 1)


def launches(case, grid, num_cells):
    """the claim of `case`: the launches its entry points make, from a plan's predict_grid() (a host-only plan under the case's knobs)"""
    n = grid["n_pred_tiles"]
    k2_inst, k4 = ROUTES[case.route]
    planes = case.n_planes
    out = []
    if k4 is not None and (case.fit or case.route.startswith("fit")):
        G, _ = grid_size(n, grid["hist_blocks"], planes)
        e = grid["k4_older_eighths"] if split_active(n, G, planes, grid["hist_blocks"], grid["k4_older_eighths"]) else 0
        counts = [len(w) for w in k4_walks(n, G, e)]
        for mode in (0, 1):
            out.append(("k4", mode, k4[0], k4[1], G, planes, e, max(counts), min(counts)))
            out.append(("solve", mode) if case.route == "fit_sums" else ("tail", mode))
    if k2_inst is not None:
        G, share = grid_size(n, grid["pred_blocks"], planes)
        counts = [len(w) for w in k2_walks(n, G)]
        out.append(("k2", k2_inst, G, planes, share, max(counts), min(counts)))
        if case.route in ("predict", "predict_pp3"):  # any int32 (kPredAnyInt32): the exact kernel follows
            out.append(("exact", exact_grid(num_cells, G), planes))
    return tuple(out)


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------------
S_SMALL = (128, 96, 1)  # 7 tiles
S_MID = (256, 192, 1)  # 14 tiles
S_MID3 = (256, 192, 3)  # 14 tiles, RGB
S_16 = (320, 200, 1)  # 16 tiles
S_BIG = (512, 384, 1)  # 41 tiles
S_LARGE = (1000, 1000, 1)  # 159 tiles
S_WIDE3 = (700, 500, 3)  # 61 tiles, RGB


def _cases():
    C = Case
    return [
        # K2: the instances by route, and the grid sizes / tiles per workgroup / planes between them
        C("predict-g1-t41", "predict", S_BIG, grid=(1, 1, 5), claim=(("k2", "TFFF", 1, 1, "one", 41, 41), ("exact", 1, 1)),
          note="one workgroup clears all ten chunks and walks 41 tiles: third LF pass, odd count"),
        C("predict-g5-t41-inexact", "predict", S_BIG, grid=(5, 5, 5), inexact=3, claim=(("k2", "TFFF", 5, 1, "one", 9, 8), ("exact", 5, 1)),
          note="out-of-range coefficients: the exact kernel redoes the plane"),
        C("predict-g14-t14", "predict", S_MID, grid=(14, 14, 5), claim=(("k2", "TFFF", 14, 1, "one", 2, 0), ("exact", 14, 1)),
          note="G = tiles, not a multiple of 8: a workgroup without a tile"),
        C("predict-planes4-eighth", "predict", S_SMALL, n_images=4, grid=(64, 64, 5), claim=(("k2", "TFFF", 7, 4, "eighth", 1, 1), ("exact", 7, 4)),
          note="four planes from a parameter array, the eighth of 64 beats the share: one tile each"),
        C("pp3-eighth", "predict_pp3", S_MID3, grid=(40, 40, 5), claim=(("k2", "TFFF", 5, 3, "eighth", 3, 2), ("exact", 5, 3)),
          note="three planes from pp3"),
        C("assume-g8-t41", "predict_assume", S_BIG, grid=(8, 8, 5), claim=(("k2", "TFFF", 8, 1, "one", 6, 5),),
          note="eight workgroups, fewer than ten clearing ones"),
        C("encode-fit-g11-t159", "encode_batch", S_LARGE, grid=(11, 32, 5), fit=True,
          claim=(("k4", 0, False, False, 32, 1, 5, 6, 3), ("tail", 0), ("k4", 1, False, False, 32, 1, 5, 6, 3), ("tail", 1), ("k2", "FFFF", 11, 1, "one", 20, 9)),
          note="the split at 5/8 on 32 workgroups; K2: 20 tiles, second LF pass"),
        C("words-fit-split8", "symbols_words", S_LARGE, grid=(10, 16, 8), fit=True,
          claim=(("k4", 0, False, False, 16, 1, 8, 20, 0), ("tail", 0), ("k4", 1, False, False, 16, 1, 8, 20, 0), ("tail", 1), ("k2", "FTFF", 10, 1, "one", 20, 9)),
          note="the split at 8/8: the younger workgroups walk nothing"),
        C("compact-fit-split1", "symbols_compact", S_16, grid=(12, 16, 1), fit=True,
          claim=(("k4", 0, False, True, 16, 1, 1, 2, 0), ("tail", 0), ("k4", 1, False, True, 16, 1, 1, 2, 0), ("tail", 1), ("k2", "FTTF", 12, 1, "one", 2, 1)),
          note="the split at 1/8 with two tiles per pair: the older workgroup walks nothing"),
        C("direct-fit-rgb", "symbols_direct", S_MID3, grid=(16, 20, 5), fit=True,
          claim=(("k4", 0, False, True, 2, 3, 0, 7, 7), ("tail", 0), ("k4", 1, False, True, 2, 3, 0, 7, 7), ("tail", 1), ("k2", "FTTT", 2, 3, "share", 7, 7)),
          note="three planes: the split is off, both grids by the share"),
        # K4 on its own: the CHECK instances, the solve kernel, plain walks below and above 16 workgroups
        C("fitsums-g5-t41", "fit_sums", S_BIG, grid=(5, 5, 5), claim=(("k4", 0, True, False, 5, 1, 0, 9, 8), ("solve", 0), ("k4", 1, True, False, 5, 1, 0, 9, 8), ("solve", 1)),
          note="plain walk on five workgroups: shards 5-15 unused"),
        C("fitsums-g20-t159-inexact", "fit_sums", S_LARGE, grid=(20, 20, 5), inexact=4,
          claim=(("k4", 0, True, False, 20, 1, 0, 10, 6), ("solve", 0), ("k4", 1, True, False, 20, 1, 0, 10, 6), ("solve", 1)),
          note="plain walk on 20 workgroups (not a multiple of 16), out-of-range coefficients"),
        C("fitchain-split7-inexact", "fit_chain", S_16, grid=(8, 16, 7), inexact=3,
          claim=(("k4", 0, True, False, 16, 1, 7, 2, 0), ("tail", 0), ("k4", 1, True, False, 16, 1, 7, 2, 0), ("tail", 1)),
          note="the split at 7/8 with two tiles per pair: the younger workgroup walks nothing"),
        # default plans (no knobs): what users run
        C("default-predict", "predict", S_BIG, inexact=2),
        C("default-words-fit", "symbols_words", S_WIDE3, fit=True),
        C("default-fit-chain", "fit_chain", S_LARGE),
    ]


CASES = _cases()
for _i, _c in enumerate(CASES):
    _c.seed = 500 + _i
COVERAGE = [c for c in CASES if c.pinned]


def _tiles_class(t):
    if t in (1, 2):
        return t
    if 17 <= t <= 32:
        return "17-32"
    if t >= 33:
        return "33+"
    return "odd3+" if t % 2 else None


def _g_class(G):
    return "1" if G == 1 else "2-7" if G < 8 else "8-9" if G < 10 else "10+" if G % 8 else None


def required_cells():
    return {
        "k2-route": {("predict", "TFFF"), ("predict_pp3", "TFFF"), ("predict_assume", "TFFF"), ("encode_batch", "FFFF"), ("symbols_words", "FTFF"),
                     ("symbols_compact", "FTTF"), ("symbols_direct", "FTTT")},
        "exact-inexact": {True},
        "k2-grid": {"1", "2-7", "8-9", "10+"},
        "k2-tiles": {1, 2, "odd3+", "17-32", "33+"},
        "k2-empty": {True},
        "k2-planes": {"1", "3pp3", ">3"},
        "k2-share": {"eighth", "share"},
        "k4": {(m, ch, c16) for m in (0, 1) for ch, c16 in ((True, False), (False, False), (False, True))},
        "k4-solve": {("tail", 0), ("tail", 1), ("solve", 0), ("solve", 1)},
        "k4-walk": {"plain<16", "plain>=16", "split1", "split5", "split8", "split-empty", "multi"},
        "k4-range": {"split", "plain"},  # out-of-range coefficients counted by a CHECK instance on either walk
    }


def covered_cells(cases_and_claims):
    got = {k: set() for k in required_cells()}
    for case, claim in cases_and_claims:
        for L in claim:
            if L[0] == "k2":
                _, inst, G, planes, share, mx, mn = L
                got["k2-route"].add((case.route, inst))
                got["k2-grid"].add(_g_class(G))
                got["k2-tiles"].add(_tiles_class(mx))
                if mn == 0:
                    got["k2-empty"].add(True)
                got["k2-planes"].add("1" if planes == 1 else "3pp3" if planes == 3 and case.route == "predict_pp3" else ">3" if planes > 3 else None)
                if planes > 1:
                    got["k2-share"].add(share)
            elif L[0] == "exact":
                if case.inexact:
                    got["exact-inexact"].add(True)
            elif L[0] == "k4":
                _, mode, check, c16, G, planes, e, mx, mn = L
                got["k4"].add((mode, check, c16))
                if case.inexact and check:
                    got["k4-range"].add("split" if e else "plain")
                if planes > 1:
                    got["k4-walk"].add("multi")
                elif e:
                    got["k4-walk"].add(f"split{e}")
                    if mn == 0:
                        got["k4-walk"].add("split-empty")
                else:
                    got["k4-walk"].add("plain<16" if G < 16 else "plain>=16" if G % 16 else None)
            else:
                got["k4-solve"].add(L)
    for v in got.values():
        v.discard(None)
    return got


def walk_is_a_partition(walks, n_tiles):
    """every tile exactly once over the workgroups' walks"""
    seen = np.zeros(n_tiles, np.int64)
    for w in walks:
        for t in w:
            if not 0 <= t < n_tiles:
                return False
            seen[t] += 1
    return bool((seen == 1).all())
