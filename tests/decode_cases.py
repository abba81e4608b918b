"""Crafted planes for the device decoder (K13, k13_decode.hip): coefficient planes that no encoder of ours would make, built on the CPU by running the decoder's
recurrence forward on the oracle. tests/test_decode_cases_host.py holds them to the host decoder and to the cells they are here for, without a GPU;
tests/test_gpu_decode.py decodes them on the device; tests/tools/fuzz_later.py draws more of them (kind "decode").

The walk (`walk`, and `synth` for its first three results): start from the oracle's Wavelet of an all-zero tile - Some(0) on every node - and visit
emit_oracle.stream_nodes. At a Some node fri_oracle's context_at (the literal get_lf / get_hf_context_bucket) gives (bucket, prediction) from the coefficients
written so far; any symbol s may follow: the node takes unpack_signed(s) + prediction wrapped to int32, the stream takes bucket << 10 | s. Plane and stream are
then consistent for every parameter set and every choice of symbols, and the histogram of the stream, multiplied by a constant, is still a histogram the emitter
accepts - with max_freq_bits as large as the constant makes it.

Generator conditions, enforced here and asserted in the host test:
  - symbols lie in 0..1022: a used symbol 1023, or a Laplace value >= 1 in slot 1023, makes the model's last frequency wrap (AnsContext::finalize, the reference's
    own line), and the format no longer reads back what it wrote;
  - the scaled histogram is accepted only if emit.finalize_context gives every used symbol a frequency and slot 1023 none, and its counts stay below 2^32; otherwise
    the case halves its multiplier until they do;
  - a value that would become INT32_MIN takes the next symbol instead: a flat plane holds None as INT32_MIN, so it cannot hold Some(i32::MIN) (include/fri_hip.h).
    The `sentinel` plane alone turns that off.

Tile shapes: 40 x 30 (F = 7, num_some = 1333: DC, root and level 1 in one 64-entry chunk) and 440 x 16 (F = 34, num_some = 7902: the 68 DC and root entries fill
more than one chunk), picked with a host-only Plan(None, ...): the shortest stream with F >= 33 found among widths 60..680 and heights 1..80."""
import functools

import numpy as np

import frave_amd as fa
import frave_amd.emit as emit
from oracle import emit_oracle, fri_oracle
from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS

NONE = -(2 ** 31)
INT_MAX = 2 ** 31 - 1
SMALL, LARGE = (40, 30), (440, 16)
SHAPE_COUNTS = {SMALL: (7, 1333), LARGE: (34, 7902)}  # (F, num_some)
EDGE_SYMBOLS = (0, 1, 15, 16, 17, 1007, 1008, 1022)
RULES = ("geometric", "uniform", "edge", "alternate")
MULTIPLIERS = (1, 64, 4096, 1 << 20)
MAX_PLANES = 16


# ---- the lattice of a tile shape -------------------------------------------------------------------------------------------------------------------------------

class Lattice:
    """what a walk needs of a tile shape, computed once: the oracle's node walk, and the plan's tables for the contexts' neighbours (cells only: the walk itself
    asks the oracle)"""

    def __init__(self, tw, th):
        self.shape = (tw, th)
        W = fri_oracle.Wavelet(np.zeros(tw * th, np.uint8), th, tw, 1)
        self.F = W.num_cells
        self.some = W.coefficients()[0] != NONE
        self.nodes = [(c, h) for c, h in emit_oracle.stream_nodes(W) if self.some[c, h]]
        W.close()
        P = fa.Plan(None, tw, th, 1)
        assert P.num_cells == self.F and P.num_some == len(self.nodes) and np.array_equal(P.valid_bits(), self.some)
        order = emit.stream_order(P.centers(), P.valid_mask())
        assert [(int(o) >> 9, int(o) & 511) for o in order] == self.nodes, "the plan's stream order is not the oracle's walk"
        self.levels = [P.num_some_levels(k) for k in range(10)]
        table, cells = P.neighbour_table().astype(np.int64), P.neighbour_cells().astype(np.int64)
        P.close()
        cell, heap = np.array(self.nodes).T
        self.cell, self.heap = cell, heap
        self.own = cell * 512 + heap
        t = table[heap]  # [n][6]
        c = cells[cell[:, None], (t >> 9) & 7]
        self.off = np.where((t & 0x8000).astype(bool) | (c < 0), -1, c * 512 + (t & 511))
        self.off[heap < 2, 3:] = -1  # the LF context reads three
        self.pos = np.full(self.F * 512, 1 << 30, np.int64)  # the step that writes a node (never, for a None node)
        self.pos[self.own] = np.arange(len(self.nodes))
        self.group = np.where(heap >= 256, 0, np.where(heap >= 128, 1, 2))  # the layer group of an HF entry (prediction.rs:165-179)

    def seen(self, plane):
        """int64 [n][6]: what each step's context read - a neighbour written by an earlier step holds its final value, every other one the initial 0"""
        flat = np.asarray(plane, np.int64).reshape(-1)
        off = np.maximum(self.off, 0)
        early = (self.off >= 0) & (self.pos[off] < np.arange(len(self.nodes))[:, None])
        return np.where(early, flat[off], 0)


@functools.lru_cache(maxsize=None)
def lattice(tw, th):
    return Lattice(tw, th)


# ---- the walk --------------------------------------------------------------------------------------------------------------------------------------------------

def _params(p):
    a = np.ascontiguousarray(p, np.float32).reshape(3, 6)
    return a.copy()


def draw_symbols(rule, n, seed):
    """the symbol of every step, 0..1022. rule: "geometric" or ("geometric", p); "uniform"; "edge"; "alternate" """
    rng = np.random.default_rng([seed, 13])
    name, arg = (rule, None) if isinstance(rule, str) else rule
    if name == "geometric":
        s = np.minimum(rng.geometric(arg or 0.3, n) - 1, 1022)
    elif name == "uniform":
        s = rng.integers(0, 1023, n)
    elif name == "edge":
        s = np.array(EDGE_SYMBOLS)[rng.integers(0, len(EDGE_SYMBOLS), n)]
    elif name == "alternate":
        s = np.where(np.arange(n) & 1, 1022, 0)
    else:
        raise ValueError(rule)
    return s.astype(np.int64)


def walk(tile_w, tile_h, value_params, width_params, symbols, seed, avoid_int_min=True):
    """dict(plane int32 [F][512] with None = INT32_MIN, stream uint16 [num_some], hist uint32 [10][1024], and per step: bucket, prediction, symbol, unwrapped (the
    sum before it wraps), moved (steps whose symbol gave way to the next one))"""
    L = lattice(tile_w, tile_h)
    vp, wp = _params(value_params), _params(width_params)
    n = len(L.nodes)
    sym = draw_symbols(symbols, n, seed)
    W = fri_oracle.Wavelet(np.zeros(tile_w * tile_h, np.uint8), tile_h, tile_w, 1)
    bucket, pred, unwrapped, moved = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64), []
    for i, (cell, heap) in enumerate(L.nodes):
        b, p = W.context_at(0, cell, heap, vp, wp)
        s = int(sym[i])
        value = emit_oracle.unpack_signed(s) + p
        if avoid_int_min and (value + 2 ** 31) % 2 ** 32 - 2 ** 31 == NONE:
            s = (s + 1) % 1023  # (the neighbouring symbol's value differs by one or by the sign: never INT32_MIN again)
            sym[i] = s
            moved.append(i)
            value = emit_oracle.unpack_signed(s) + p
        bucket[i], pred[i], unwrapped[i] = b, p, value
        W.set_coefficient(0, cell, heap, (value + 2 ** 31) % 2 ** 32 - 2 ** 31)
    plane = W.coefficients()[0]
    W.close()
    assert sym.min() >= 0 and sym.max() <= 1022
    hist = np.zeros((10, 1024), np.uint32)
    np.add.at(hist, (bucket, sym), 1)
    return dict(plane=plane, stream=(bucket << 10 | sym).astype(np.uint16), hist=hist, bucket=bucket, prediction=pred, symbol=sym, unwrapped=unwrapped, moved=moved)


def synth(tile_w, tile_h, value_params, width_params, symbols, seed):
    """(the oracle's plane int32 [F][512], the stream uint16 [num_some], the histogram uint32 [10][1024])"""
    r = walk(tile_w, tile_h, value_params, width_params, symbols, seed)
    return r["plane"], r["stream"], r["hist"]


def models_of(hist):
    """per context None (no symbols) or emit.finalize_context's (freqs, cdf, off, max_freq_bits)"""
    return [emit.finalize_context(h, b) if h.any() else None for b, h in enumerate(hist)]


def histogram_violations(hist):
    """the generator conditions a (scaled) histogram does not meet"""
    bad = []
    hist = np.asarray(hist)
    if hist[:, 1023].any():
        bad.append("symbol 1023 is used")
    if (hist.astype(np.uint64).sum(axis=1) >= 1 << 32).any():
        bad.append("a context's counts reach 2^32")
    if not bad:
        for b, m in enumerate(models_of(hist.astype(np.uint32))):
            if m is not None and ((m[0][hist[b] > 0] == 0).any() or m[0][1023] != 0):
                bad.append("context %d: a used symbol without a frequency, or a frequency in slot 1023" % b)
    return bad


def scaled_histogram(hist, multiplier):
    """(hist * m, m): m = the multiplier, halved until the generator conditions hold"""
    m = int(multiplier)
    while m > 1 and histogram_violations(hist.astype(np.uint64) * m):
        m //= 2
    out = hist.astype(np.uint64) * m
    assert not histogram_violations(out), histogram_violations(out)
    return out.astype(np.uint32), m


# ---- the parameter families --------------------------------------------------------------------------------------------------------------------------------------

def _all(v):
    return np.full((3, 6), v, np.float32)


def _intercepts(a, b, c):
    """width parameters with zero slopes: the bucket is the intercept's, per layer group"""
    wp = np.zeros((3, 6), np.float32)
    wp[:, 0] = (a, b, c)
    return wp


KAT_V, KAT_W = _params(KAT_VALUE_PARAMS), _params(KAT_WIDTH_PARAMS)
INF_W = np.tile(np.array([np.inf, -np.inf, 1, 1, 1, 1], np.float32), (3, 1))
# one set per layer group, each unlike the other two: a wrong group index decodes other coefficients
GROUP_V = np.stack([KAT_V[0], -KAT_V[1] * np.float32(0.5), np.array([0.75, 0, 0, 0.25, 0, 0], np.float32)])
GROUP_W = np.stack([np.array([1.0, 0.9, 0.1, 0.1, 0.1, 0.1], np.float32), np.array([7.0, 0.05, 0.3, 0.02, 0.2, 0.1], np.float32),
                    np.array([13.0, 0.3, 0.0, 0.4, 0.0, 0.2], np.float32)])
MILD_W = np.tile(np.array([0.5, 0.12, 0.1, 0.08, 0.1, 0.1], np.float32), (3, 1))  # widths that follow the neighbours' differences through every bucket

# name -> dict(shape, vp, wp, rule, multiplier, seed)
CASES = {}


def _case(name, vp, wp, rule, multiplier, shape=SMALL, seed=1):
    CASES[name] = dict(name=name, shape=shape, vp=_params(vp), wp=_params(wp), rule=rule, multiplier=multiplier, seed=seed)


_case("kat_geometric", KAT_V, KAT_W, "geometric", 1)
_case("kat_uniform_x64", KAT_V, KAT_W, "uniform", 64)
_case("mild_geometric_x4096", KAT_V, MILD_W, ("geometric", 0.06), 4096, seed=2)  # (the seed whose DC and root differences include a 5: LF bucket 2)
_case("grow_1.5", _all(1.5), KAT_W, "uniform", 1)  # coefficients grow until the predictions saturate
_case("grow_-2.5", _all(-2.5), MILD_W, "edge", 64)
_case("saturated_3e9", _all(3e9), _all(1e30), "geometric", 1)  # both conversions saturated
_case("saturated_1e30", _all(1e30), _all(3e9), "alternate", 4096)
_case("negative_width_x2^20", KAT_V, _all(-1.0), "uniform", 1 << 20)  # a negative width is u32 0: every HF symbol in bucket 0
_case("negative_width_lists", KAT_V, _all(-1.0), "uniform", 1)  # ... with max_freq_bits 10: most of the used symbols are off the distribution
_case("all_nan", _all(np.nan), _all(np.nan), "edge", 1)
_case("inf", _all(np.inf), INF_W, "uniform", 64)  # inf x 0 on a zero neighbour is NaN
_case("edges_low", KAT_V, _intercepts(2.999, 3.0, 29.999), "edge", 1)
_case("edges_high", KAT_V, _intercepts(30.0, 31.0, 32.0), "edge", 4096)
_case("edges_2^32", _all(1.5), _intercepts(4294967296.0, 2.999, 31.0), "alternate", 1)
_case("edges_turned", KAT_V, _intercepts(32.0, 29.999, 3.0), "geometric", 64)
_case("groups", GROUP_V, GROUP_W, ("geometric", 0.1), 1)
_case("large_kat", KAT_V, MILD_W, ("geometric", 0.05), 64, shape=LARGE)
_case("large_groups", GROUP_V, GROUP_W, "edge", 1, shape=LARGE)
_case("large_grow", _all(1.5), MILD_W, "uniform", 4096, shape=LARGE)

# the batch files: name -> the cases that are its tiles, one shape each
BATCHES = {"small": [n for n, c in CASES.items() if c["shape"] == SMALL], "large": [n for n, c in CASES.items() if c["shape"] == LARGE]}
assert all(len(v) <= MAX_PLANES for v in BATCHES.values())


@functools.lru_cache(maxsize=None)
def built(name):
    """a case walked: walk()'s dict and hist_scaled, multiplier_used, models (models_of the scaled histogram)"""
    c = CASES[name]
    r = walk(*c["shape"], c["vp"], c["wp"], c["rule"], c["seed"])
    r["hist_scaled"], r["multiplier_used"] = scaled_histogram(r["hist"], c["multiplier"])
    r["models"] = models_of(r["hist_scaled"])
    r.update(vp=c["vp"], wp=c["wp"], shape=c["shape"], name=name)
    return r


def file_of(cases):
    """the `frit` bytes of up to 16 planes (walk() dicts with hist_scaled, vp, wp) of one shape as the tiles of a one-row image: each its own parameters, histogram
    and stream"""
    cases = list(cases)
    assert 1 <= len(cases) <= MAX_PLANES and len({c["shape"] for c in cases}) == 1
    tw, th = cases[0]["shape"]
    streams = np.stack([c["stream"] for c in cases])[:, None]
    hist = np.stack([c["hist_scaled"] for c in cases])[:, None]
    vp, wp = (np.stack([c[k] for c in cases])[:, None] for k in ("vp", "wp"))
    return emit.tiled_encode_from_streams(tw * len(cases), th, tw, th, streams, hist, vp, wp)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(frit bytes, tile_w, tile_h, the oracle's planes int32 [P][F][512]) of a batch file"""
    cases = [built(n) for n in BATCHES[name]]
    return (file_of(cases), *cases[0]["shape"], np.stack([c["plane"] for c in cases]))


@functools.lru_cache(maxsize=None)
def sentinel():
    """the INT32_MIN plane: value parameters 1.5 on uniform symbols with the avoidance off, the first seed whose walk writes INT32_MIN into a node that a later
    context reads. (walk() dict with hist_scaled, vp, wp, shape, seed)"""
    L = lattice(*SMALL)
    for seed in range(64):
        r = walk(*SMALL, _all(1.5), KAT_W, "uniform", seed, avoid_int_min=False)
        if (L.seen(r["plane"]) == NONE).any():
            r["hist_scaled"], r["multiplier_used"] = scaled_histogram(r["hist"], 1)
            r.update(vp=_all(1.5), wp=KAT_W.copy(), shape=SMALL, seed=seed, name="sentinel")
            return r
    raise AssertionError("no seed below 64 writes a Some(INT32_MIN) that is read again")


# ---- the cells ---------------------------------------------------------------------------------------------------------------------------------------------------

# Two cells that cannot exist. Denormal parameters: their product with an integer-valued float never reaches 1, so they change no result. An LF context with
# |v0 - v2| >= 2^31: the LF prediction is v0, v2 or v0 + v2 - v1 with v1 strictly between them, so it lies in [min(v0, v2), max(v0, v2)], and a DC or root value
# is that plus unpack_signed(symbol), at most 512 away. By induction the i-th LF value of a plane is within 512 (i + 1) of 0, whatever the file holds: no stream
# makes the decoder, host or device, take that difference past 2^31. LF_BOUND states it and the host test checks it on every case.
LF_BOUND = 512

CELLS = (["prediction == INT32_MAX", "prediction <= INT32_MIN + 1", "a sum that left int32", "HF neighbour with |v| > 2^24"]
         + ["LF bucket %d" % b for b in range(10)] + ["HF group %d bucket %d" % (g, b) for g in range(3) for b in range(10)]
         + ["max_freq_bits >= 17", "max_freq_bits >= 24", "n_off >= 512"] + ["symbol %d in two buckets" % s for s in EDGE_SYMBOLS])


def _hf(groups):
    """{group: "buckets as digits"} -> cell names"""
    return {"HF group %d bucket %s" % (g, b) for g, digits in groups.items() for b in digits}


_SATURATED = {"prediction == INT32_MAX", "prediction <= INT32_MIN + 1", "a sum that left int32", "HF neighbour with |v| > 2^24"}
_EDGES = {"symbol %d in two buckets" % s for s in EDGE_SYMBOLS}
# case -> the cells it is there to reach (it may reach more); tests/test_decode_cases_host.py holds every case to its row and the rows together to CELLS
WANT = {
    "kat_geometric": _hf({0: "01234", 1: "01234", 2: "01234"}) | {"LF bucket 0", "LF bucket 1"},
    "kat_uniform_x64": _hf({0: "9", 1: "9", 2: "9"}) | {"LF bucket 7", "LF bucket 9"},
    "mild_geometric_x4096": _hf({0: "01234567", 1: "01234567", 2: "01234567"}) | {"max_freq_bits >= 17", "LF bucket 2", "LF bucket 5", "LF bucket 6"},
    "grow_1.5": _SATURATED | {"n_off >= 512"},
    "grow_-2.5": _SATURATED | _EDGES,
    "saturated_3e9": _SATURATED | _hf({0: "09", 1: "09", 2: "09"}),
    "saturated_1e30": _SATURATED | {"max_freq_bits >= 17"},
    "negative_width_x2^20": _hf({0: "0", 1: "0", 2: "0"}) | {"max_freq_bits >= 24", "n_off >= 512"},
    "negative_width_lists": _hf({0: "0", 1: "0", 2: "0"}) | {"n_off >= 512"},
    "all_nan": _hf({0: "0", 1: "0", 2: "0"}) | {"LF bucket 4"},
    "inf": _SATURATED | {"n_off >= 512"},
    "edges_low": _hf({0: "0", 1: "1", 2: "8"}) | _EDGES,
    "edges_high": _hf({0: "9", 1: "9", 2: "9"}) | {"max_freq_bits >= 17"},
    "edges_2^32": _hf({0: "9", 1: "0", 2: "9"}) | _SATURATED,
    "edges_turned": _hf({0: "9", 1: "8", 2: "1"}),
    "groups": _hf({0: "0123456789", 1: "34567", 2: "56789"}) | {"LF bucket 3", "LF bucket 8"},
    "large_kat": _hf({0: "0123456789", 1: "012345678", 2: "01234567"}) | {"LF bucket %d" % b for b in (0, 1, 3, 4, 5, 6, 7, 8, 9)},
    "large_groups": _hf({0: "13456789", 1: "3456789", 2: "9"}) | _EDGES,
    "large_grow": _SATURATED | {"max_freq_bits >= 24"} | _hf({1: "9", 2: "89"}),
}


def cells_of(r):
    """the cells a walked plane (with hist_scaled) reaches, from the oracle's contexts and the plane itself"""
    L = lattice(*r["shape"])
    lf = L.heap < 2
    out = set()
    pred, bucket = r["prediction"], r["bucket"]
    if (pred[~lf] == INT_MAX).any():
        out.add("prediction == INT32_MAX")
    if (pred[~lf] <= NONE + 1).any():
        out.add("prediction <= INT32_MIN + 1")
    if ((r["unwrapped"] > INT_MAX) | (r["unwrapped"] < NONE)).any():
        out.add("a sum that left int32")
    seen = L.seen(r["plane"])
    if (np.abs(seen[~lf]) > 1 << 24).any():
        out.add("HF neighbour with |v| > 2^24")
    out |= {"LF bucket %d" % b for b in np.unique(bucket[lf])}
    out |= {"HF group %d bucket %d" % (g, b) for g, b in set(zip(L.group[~lf].tolist(), bucket[~lf].tolist()))}
    models = r.get("models") or models_of(r["hist_scaled"])
    bits = [m[3] for m in models if m is not None]
    if max(bits) >= 17:
        out.add("max_freq_bits >= 17")
    if max(bits) >= 24:
        out.add("max_freq_bits >= 24")
    if max(len(m[2]) for m in models if m is not None) >= 512:
        out.add("n_off >= 512")
    for s in EDGE_SYMBOLS:
        if np.count_nonzero(r["hist"][:, s]) >= 2:
            out.add("symbol %d in two buckets" % s)
    return out


def contexts_restated(r):
    """(bucket, prediction) of every step recomputed in numpy from Lattice.seen - the plan's neighbour tables on the finished plane - in the decoder's arithmetic:
    wrapping int32, f32 with one rounding per operation, saturating conversions. Equal to the oracle's contexts of the walk unless the tables or `seen` are wrong,
    which is what ties the cells above to the walk."""
    L = lattice(*r["shape"])
    v = L.seen(r["plane"])
    w32 = lambda x: (x + 2 ** 31) % 2 ** 32 - 2 ** 31  # noqa: E731
    wabs = lambda x: w32(np.abs(x))  # noqa: E731  (|INT32_MIN| stays INT32_MIN)
    f = np.float32
    vp, wp = r["vp"][L.group], r["wp"][L.group]  # [n][6]
    with np.errstate(all="ignore"):
        d = [wabs(w32(v[:, a] - v[:, b])).astype(f) for a, b in ((0, 3), (1, 2), (4, 5), (1, 5), (2, 4))]
        width = wp[:, 0].copy()
        for k in range(5):
            width = (width + (wp[:, k + 1] * d[k]).astype(f)).astype(f)
        pf = (v[:, 0].astype(f) * vp[:, 0]).astype(f)
        for k in range(1, 6):
            pf = (pf + (v[:, k].astype(f) * vp[:, k]).astype(f)).astype(f)
        hf_pred = np.where(np.isnan(pf), 0, np.clip(np.nan_to_num(pf.astype(np.float64), nan=0.0), NONE, INT_MAX)).astype(np.int64)  # trunc toward zero, saturating
        lf_w = wabs(w32(v[:, 0] - v[:, 2])) % 2 ** 32  # as u32
        lf_width = lf_w.astype(f)
    mx, mn = np.maximum(v[:, 0], v[:, 2]), np.minimum(v[:, 0], v[:, 2])
    lf_pred = np.where(v[:, 1] >= mx, mx, np.where(v[:, 1] <= mn, mn, w32(w32(v[:, 0] + v[:, 2]) - v[:, 1])))
    lf = L.heap < 2

    def bucket_of(x):
        with np.errstate(all="ignore"):
            u = np.where(np.isnan(x) | (x <= 0), 0, np.minimum(np.nan_to_num(x.astype(np.float64), nan=0.0), 2.0 ** 32 - 1)).astype(np.uint64)
        return np.searchsorted(np.array([3, 5, 6, 8, 12, 16, 20, 25, 30]), u, side="right")

    return np.where(lf, bucket_of(lf_width), bucket_of(width)), np.where(lf, lf_pred, hf_pred)


# ---- the coder replayed --------------------------------------------------------------------------------------------------------------------------------------------

def word_steps(words, stream, models):
    """the step at which the decoder takes each body word: int [n_words], -1 for the twenty words of the initial states. The loop of
    oracle/emit_oracle.decode_image on known symbols, the models emit.finalize_context's (models_of)."""
    words = [int(w) for w in words]
    x = [words[2 * i] | words[2 * i + 1] << 32 for i in range(10)]
    pos, out = 20, [-1] * len(words)
    for step, e in enumerate(np.asarray(stream).tolist()):
        b, sym = e >> 10, e & 1023
        freqs, cdf, _, bits = models[b]
        s = 9 - b
        v = x[s] & ((1 << bits) - 1)
        assert int(cdf[sym]) <= v < int(cdf[sym]) + int(freqs[sym]), "the words do not hold the stream"
        x[s] = int(freqs[sym]) * (x[s] >> bits) + v - int(cdf[sym])
        if x[s] < 1 << 31:
            x[s] = x[s] << 32 | words[pos]
            out[pos] = step
            pos += 1
    assert pos == len(words)
    return np.array(out)
