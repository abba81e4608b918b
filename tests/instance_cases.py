"""The K1 / K3 instance matrix as a table of cases (tests/test_gpu_instances.py runs them, tests/test_instance_cases_host.py checks what they reach).

launch_fwd_transform_quant (frave_amd/csrc/k1_forward.hip) and launch_inverse_transform (k3_inverse.hip, with the midpoint and measuring instances of
k3_lossy.hip) pick one template instance per launch from the plan, the caller's pointers and the plan's modes. Every case names the instance it targets as a
`claim` tuple of the launchers' axes:

    ("k1", mode, staging, N, quant, stores)    mode: "1", "3", "3rct"; staging: "edge", "fast", "generic"; N: 4, 6; quant: "qi", "gen"; stores: "nt", "plain"
    ("c16", mode, staging, N, quant)           the int16 compact planes of fri_hip_encode_symbols_batch_dev(d_coefs = NULL)
    ("k3", deq, rct, kernel, NI, batch, holes) deq: "ref", "mul", "mid"; kernel: "lists", "scan"; NI: 1, 2, 4; batch: n_images > 1
    ("measure", deq, rct, kernel, NI, holes)   fri_hip_measure_distortion_dev

instance_of() restates the selection rules from what a host-only plan exposes. A host-only plan is cut like a device plan only when the tiling is pinned
(fri_hip_plan_create passes the CU count to choose_forward_tiling only with a context), and the restatement reads the forward tiling for K3 too, so every
coverage case pins the tiling and FRI_HIP_INV_SHARED=1. Cases with `pinned = False` run on default plans, as users do, and claim nothing.

Not reachable through the public ABI, so not in the matrix: the K1 MEASURE instances (only fri_hip_plan_tune_forward launches them, k1_forward.hip:687),
plain versus nontemporal stores of the C16 instances (one kind, k1_forward.hip:693), and MEASURE with n_images > 1 (refused, k3_inverse.hip:724).
"""
import contextlib
import os
from dataclasses import dataclass, field

import numpy as np

_HAND = np.ones(32, np.int32)
_HAND[:10] = [3, 2, 5, 2, 3, 4, 7, 11, 13, 17]  # divisors on layers 0-2 too, which the quality table leaves at 1


def qmatrix(name):
    """"qi": all ones (the identity-quantiser instances); "qN": fri_hip_quality_matrix(N); "hand": a matrix with divisors on every layer"""
    if name == "qi":
        return np.ones(32, np.int32)
    if name == "hand":
        return _HAND.copy()
    import frave_amd as fa

    return fa.quality_matrix(int(name[1:]))


# the knobs every coverage case sets: a host-only plan then cuts the same tiling as a device plan, and K3 walks the forward tiling
BASE_KNOBS = {"FRI_HIP_TUNING": "1", "FRI_HIP_INV_SHARED": "1", "FRI_HIP_STRIDED_SHARES": "0", "FRI_HIP_RANK_WEIGHTS": "1,1,1,1", "FRI_HIP_TARGET_WGS": "64"}
# tilings by what they give on the table's shapes (instance_of says what they really give)
TILINGS = {
    "p_ni1": {"FRI_HIP_BAND_ROWS": "16", "FRI_HIP_CELLS_PER_TILE": "4"},  # planes: <= 4 cells per tile -> NI 1
    "p_ni2": {"FRI_HIP_BAND_ROWS": "16", "FRI_HIP_CELLS_PER_TILE": "8"},  # planes: NI 2, N 4
    "p_ni4": {"FRI_HIP_BAND_ROWS": "32", "FRI_HIP_CELLS_PER_TILE": "16"},  # planes: NI 4, N 4
    "p_n6": {"FRI_HIP_BAND_ROWS": "64", "FRI_HIP_CELLS_PER_TILE": "16", "FRI_HIP_TILE_BYTES": "24576"},  # planes: > 1024 staged chunks -> N 6
    "c_ni1": {"FRI_HIP_BAND_ROWS": "16", "FRI_HIP_CELLS_PER_TILE": "1"},  # RGB: 3 items per tile -> NI 1
    "c_ni2": {"FRI_HIP_BAND_ROWS": "32", "FRI_HIP_CELLS_PER_TILE": "2"},  # RGB: NI 2, N 4
    "c_ni4": {"FRI_HIP_BAND_ROWS": "48", "FRI_HIP_CELLS_PER_TILE": "3"},  # RGB: NI 4, N 4
    "c_n6": {"FRI_HIP_BAND_ROWS": "16", "FRI_HIP_CELLS_PER_TILE": "4"},  # RGB: N 6
}
ALL_KNOBS = sorted(set(BASE_KNOBS) | {k for t in TILINGS.values() for k in t} | {"FRI_HIP_K3_SCAN", "FRI_HIP_K1_CACHED_STORES", "FRI_HIP_CELLS_PER_WG"}
                  | {"FRI_HIP_PRED_BLOCKS", "FRI_HIP_HIST_BLOCKS", "FRI_HIP_K4_OLDER_EIGHTHS"})  # (the K2 / K4 grid knobs of tests/predict_cases.py)


@dataclass
class Case:
    id: str
    kind: str  # "k1", "c16", "k3", "measure"
    shape: tuple  # (width, height, channels)
    claim: tuple = None  # the instance the case targets (None: a default plan, no claim)
    rct: bool = False
    tiling: str = None  # key of TILINGS; None = the plan's own tiling
    offset: int = 0  # byte offset of the pixel buffer from a 256-byte aligned allocation
    n_images: int = 1
    gap: int = 0  # bytes between the images of a batch: pixel_stride = pixel bytes + gap
    quant: str = "q37"
    deq: int = 0  # fri_hip_plan_set_dequantiser mode (K3 / MEASURE)
    knobs: dict = field(default_factory=dict)  # FRI_HIP_K3_SCAN, FRI_HIP_K1_CACHED_STORES
    seed: int = 0

    @property
    def pinned(self):
        return self.tiling is not None

    def env(self):
        """the environment the case's plans are created under (None: no tuning knobs at all)"""
        if not self.pinned:
            return None
        return dict(BASE_KNOBS, **TILINGS[self.tiling], **self.knobs)

    @property
    def pixel_stride(self):
        w, h, c = self.shape
        return w * h * c + self.gap


@contextlib.contextmanager
def knobs(env):
    """the tuning knobs are read when a plan is created: set them for the block, restore what was there before"""
    saved = {k: os.environ.get(k) for k in ALL_KNOBS}
    try:
        for k in ALL_KNOBS:
            os.environ.pop(k, None)
        if env:
            os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


DEQ = {"ref": 0, "mul": 1, "mid": 2}
DEQ_NAME = {v: k for k, v in DEQ.items()}


def plan_facts(plan):
    """the host-side values instance_of reads: the forward tiling, whether the write-out lists exist, the shares' largest tile and cell counts"""
    t = plan.tiling()
    tiles, _, wg = plan.tile_table()
    max_wg_tiles = int(np.max(np.diff(wg)))
    max_wg_cells = max(int(tiles[wg[s + 1] - 1, 4] + tiles[wg[s + 1] - 1, 5] - tiles[wg[s], 4]) for s in range(len(wg) - 1))
    lists = plan.inverse_lists()
    return dict(t, lists_built=bool(lists["built"]), rect_bytes=lists["rect_bytes"], max_wg_tiles=max_wg_tiles, max_wg_cells=max_wg_cells)


def instance_of(case, facts, holes):
    """the instance the launchers pick for `case`, from a host-only plan's `facts` (plan_facts) and whether the lattice leaves pixels uncovered (`holes`:
    the plan's covers_image, which the host cannot read, from the oracle)"""
    w, h, c = case.shape
    env = case.env() or {}
    mode = "1" if c == 1 else "3rct" if case.rct else "3"
    quant = "qi" if (qmatrix(case.quant)[:10] == 1).all() else "gen"  # layers 0-9 only (k1_forward.hip:669, k3_inverse.hip:754)
    if case.kind in ("k1", "c16"):
        img_bytes = w * h * c
        # k1_forward.hip:677-679
        edge = case.offset % 16 != 0 or img_bytes % 16 != 0 or (case.n_images > 1 and case.pixel_stride % 16 != 0)
        fast = not edge and (w * c) % 16 == 0
        n = 4 if facts["lds_rows"] * (facts["lds_pitch"] // 16) <= 4 * 256 else 6
        staging = "edge" if edge else "fast" if fast else "generic"
        if case.kind == "c16":  # k1_forward.hip:693-697: coefs16 overrides the store kind
            return ("c16", mode, staging, n, quant)
        # k1_forward.hip:647 (k1_cached_stores from FRI_HIP_K1_CACHED_STORES, fri_hip.cpp); transform_quant_batch_dev asks for nontemporal stores
        stores = "plain" if env.get("FRI_HIP_K1_CACHED_STORES", "0") not in ("", "0") else "nt"
        return ("k1", mode, staging, n, quant, stores)
    # K3, k3_inverse.hip:758-764 (FRI_HIP_INV_SHARED=1: the inverse kernel walks the forward tiling; one share per workgroup)
    ipw = (facts["max_tile_cells"] * c + 3) // 4
    ni = 1 if ipw <= 1 else 2 if ipw == 2 else 4  # pick_inverse, k3_inverse.hip:686
    lists_lds = facts["rect_bytes"] + facts["max_wg_tiles"] * (24 + 24) + facts["max_wg_cells"] * 16  # inv_plan_fits(p, true), k3_inverse.hip:712
    lists = (facts["lists_built"] and env.get("FRI_HIP_K3_SCAN", "0") in ("", "0") and lists_lds <= 160 * 1024 and case.offset % 16 == 0 and (w * c) % 16 == 0
             and (case.n_images == 1 or case.pixel_stride % 16 == 0) and w * c < (1 << 24))
    kernel = "lists" if lists else "scan"
    deq = DEQ_NAME[case.deq]
    if case.kind == "measure":
        return ("measure", deq, case.rct, kernel, ni, holes)
    return ("k3", deq, case.rct, kernel, ni, case.n_images > 1, holes)


# ---- the table -------------------------------------------------------------------------------------------------------------------------------------------
_GEN_Q = ["q1", "q37", "q90", "hand"]
_SHAPE = {("1", "aligned"): (256, 192, 1), ("1", "generic"): (200, 128, 1), ("3", "aligned"): (256, 192, 3), ("3", "generic"): (264, 192, 3)}


def _k1_cases():
    out = []
    i = 0
    for mode in ("1", "3", "3rct"):
        c = 1 if mode == "1" else 3
        for staging in ("edge", "fast", "generic"):
            for n in (4, 6):
                for quant in ("qi", "gen"):
                    stores = "plain" if i % 2 else "nt"
                    shape = _SHAPE[(str(c), "generic" if staging == "generic" else "aligned")]
                    kw = {}
                    if staging == "edge":  # an unaligned pointer, or an aligned first image and an odd stride between images
                        kw = dict(offset=1 + (i % 15)) if i % 4 < 2 else dict(n_images=2, gap=7 + 2 * (i % 5))
                    q = "qi" if quant == "qi" else _GEN_Q[i % 4]
                    tiling = ("p_" if c == 1 else "c_") + ("n6" if n == 6 else "ni2")
                    out.append(Case(f"k1-{mode}-{staging}-n{n}-{quant}-{stores}", "k1", shape, ("k1", mode, staging, n, quant, stores), rct=mode == "3rct",
                                    tiling=tiling, quant=q, knobs={"FRI_HIP_K1_CACHED_STORES": "1" if stores == "plain" else "0"}, seed=i, **kw))
                    i += 1
    return out


def _c16_cases():
    out = []
    i = 0
    for mode in ("1", "3", "3rct"):
        c = 1 if mode == "1" else 3
        for staging in ("edge", "fast", "generic"):
            for quant in ("qi", "gen"):
                n = 6 if (i % 3 == 0) else 4
                shape = _SHAPE[(str(c), "generic" if staging == "generic" else "aligned")]
                kw = {}
                if staging == "edge":
                    kw = dict(offset=3 + i % 13) if quant == "qi" else dict(n_images=2, gap=5 + i % 7)
                q = "qi" if quant == "qi" else _GEN_Q[i % 4]
                tiling = ("p_" if c == 1 else "c_") + ("n6" if n == 6 else "ni2")
                out.append(Case(f"c16-{mode}-{staging}-n{n}-{quant}", "c16", shape, ("c16", mode, staging, n, quant), rct=mode == "3rct", tiling=tiling, quant=q,
                                seed=100 + i, **kw))
                i += 1
    return out


# Cells of the K3 / MEASURE matrix that are reached on a batch or on a thin shape whose lattice has holes (K3 zero-fills every image first, MEASURE counts only
# owned bytes) instead of the plain single image: (kind, dequantiser group, RCT, kernel, NI) -> what the case changes.
_K3_SPECIAL = {
    ("k3", "mid", False, "lists", 2): dict(shape=(256, 192, 1), n_images=3, gap=48),  # gaps of a multiple of 16 keep the lists kernel
    ("k3", "mid", True, "scan", 4): dict(shape=(256, 192, 3), n_images=3, gap=13),  # an odd gap takes the scanning kernel
    ("k3", "mid", False, "scan", 1): dict(shape=(3, 300, 1)),
    ("k3", "mid", False, "scan", 2): dict(shape=(3, 300, 1), n_images=3, gap=9, tiling="p_n6"),
    ("k3", "mid", True, "scan", 1): dict(shape=(2, 257, 3)),
    ("k3", "mid", True, "scan", 2): dict(shape=(2, 257, 3), n_images=3, gap=5),
    ("measure", "mid", False, "scan", 1): dict(shape=(3, 300, 1)),
    ("measure", "mid", True, "scan", 2): dict(shape=(2, 257, 3)),
    ("measure", "refmul", False, "scan", 4): dict(shape=(2, 257, 3)),
}


def _k3_cases(kind):
    out = []
    i = 0
    deqs = ("ref", "mul", "mid") if kind == "k3" else ("refmul", "mid")
    for deq in deqs:
        for rct in (False, True):
            for kernel in ("lists", "scan"):
                for ni in (1, 2, 4):
                    special = dict(_K3_SPECIAL.get((kind, deq, rct, kernel, ni), {}))
                    is_special = bool(special)
                    c = 3 if rct or i % 2 else 1
                    shape = special.pop("shape", _SHAPE[(str(c), "aligned")])
                    c = shape[2]
                    d = ("ref" if i % 2 == 0 else "mul") if deq == "refmul" else deq
                    kw, knobs_ = dict(special), {}
                    tiling = kw.pop("tiling", ("p_" if c == 1 else "c_") + f"ni{ni}")
                    if kernel == "scan" and not is_special:  # the scanning kernel: forced by the knob, an unaligned output pointer, or rows that are not a multiple of 16 bytes
                        way = i % 3
                        if way == 0:
                            knobs_ = {"FRI_HIP_K3_SCAN": "1"}
                        elif way == 1:
                            kw = dict(offset=1 + i % 15)
                        else:
                            shape = _SHAPE[(str(c), "generic")]
                    holes = shape[0] < 16
                    batch = kw.get("n_images", 1) > 1
                    claim = ("k3", d, rct, kernel, ni, batch, holes) if kind == "k3" else ("measure", d, rct, kernel, ni, holes)
                    tag = ("-batch" if batch else "") + ("-holes" if holes else "")
                    out.append(Case(f"{kind}-{d}-{'rct' if rct else 'plain'}-{kernel}-ni{ni}-c{c}{tag}", kind, shape, claim, rct=rct, tiling=tiling, quant=_GEN_Q[i % 4],
                                    deq=DEQ[d], knobs=knobs_, seed=200 + i, **kw))
                    i += 1
    return out


def _default_cases():
    """default plans (no knobs), what users run: no claim, the launchers choose"""
    mid = DEQ["mid"]
    return [
        Case("default-k1-rct", "k1", (320, 200, 3), rct=True, quant="q37", seed=400),
        Case("default-c16-plain", "c16", (320, 200, 1), offset=5, quant="q90", seed=401),
        Case("default-k3-mid-rct-batch", "k3", (320, 200, 3), rct=True, n_images=3, gap=16, quant="q37", deq=mid, seed=402),
        Case("default-measure-mul-rct", "measure", (320, 200, 3), rct=True, quant="q1", deq=DEQ["mul"], seed=403),
        Case("default-measure-mid-4096", "measure", (4096, 4096, 1), quant="q37", deq=mid, seed=404),
        Case("default-k3-mid-4096", "k3", (4096, 4096, 1), quant="q37", deq=mid, seed=404),
    ]


CASES = _k1_cases() + _c16_cases() + _k3_cases("k3") + _k3_cases("measure") + _default_cases()
COVERAGE = [c for c in CASES if c.pinned]


def required_cells():
    """every cell the coverage cases must reach, by kind: (name of the requirement, set of claims or predicate)"""
    modes, stagings = ("1", "3", "3rct"), ("edge", "fast", "generic")
    req = {
        "k1": {(m, s, n, q) for m in modes for s in stagings for n in (4, 6) for q in ("qi", "gen")},
        "k1-stores": {(m, st) for m in modes for st in ("nt", "plain")},
        "c16": {(m, s, q) for m in modes for s in stagings for q in ("qi", "gen")},
        "c16-n6": {6},
        "k3": {(d, r, k, ni) for d in ("ref", "mul", "mid") for r in (False, True) for k in ("lists", "scan") for ni in (1, 2, 4)},
        # MID and RCT + MID (first field) with n_images > 1 (second) and on a lattice with holes (third), each way
        "k3-mid-batch-holes": {(r, b, hl) for r in (False, True) for b in (False, True) for hl in (False, True) if b or hl},
        "measure": {(d, r, k, ni) for d in ("refmul", "mid") for r in (False, True) for k in ("lists", "scan") for ni in (1, 2, 4)},
        "measure-refmul": {"ref", "mul"},
        "measure-holes": {(1, False), (3, False), (3, True)},  # thin shapes with holes: (channels, RCT)
    }
    return req


def covered_cells(cases_and_claims):
    """the cells a list of (case, claim) pairs reach, keyed like required_cells()"""
    got = {k: set() for k in required_cells()}
    for case, cl in cases_and_claims:
        kind = cl[0]
        if kind == "k1":
            got["k1"].add(cl[1:5])
            got["k1-stores"].add((cl[1], cl[5]))
        elif kind == "c16":
            got["c16"].add((cl[1], cl[2], cl[4]))
            got["c16-n6"].add(cl[3])
        elif kind == "k3":
            got["k3"].add(cl[1:5])
            if cl[1] == "mid" and (cl[5] or cl[6]):
                got["k3-mid-batch-holes"].add((cl[2], cl[5], cl[6]))
        elif kind == "measure":
            got["measure"].add(("mid" if cl[1] == "mid" else "refmul",) + cl[2:5])
            if cl[1] != "mid":
                got["measure-refmul"].add(cl[1])
            if cl[5]:
                got["measure-holes"].add((case.shape[2], cl[2]))
    return got
