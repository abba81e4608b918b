"""The crafted planes of tests/decode_cases.py on the host (CPU only): every batch file parses, the host decoder (emit.tiled_decode) returns the oracle walk's
planes exactly, None entries included, emit.tiled_parse_coded returns every plane's parameters byte for byte, NaN payloads included, the generator conditions
held, and the cases reach the cells they are there for - one table, decode_cases.WANT, case by cells. That makes the comparison of tests/test_gpu_decode.py
three-way (oracle, host, device) and keeps a generator mistake from reading as a kernel bug. The `sentinel` plane, a decoded Some(i32::MIN), is held to what the
host decoder does with it today."""
import numpy as np
import pytest

import frave_amd.emit as emit
from oracle import emit_oracle
from tests import decode_cases as D

# what emit.tiled_decode does with the sentinel file today: "plane" (it returns one, unlike the oracle's), "truncated" or "mismatch" (it refuses: "stream
# truncated" / "stream does not match the model"). Recorded here; tests/test_gpu_decode.py compares the device with it.
SENTINEL_HOST = "plane"


@pytest.mark.parametrize("name", sorted(D.BATCHES))
def test_the_host_decoder_returns_the_oracle_walks_planes(name):
    frv, tw, th, planes = D.batch(name)
    ti, coefs = emit.tiled_decode(frv)
    assert tuple(ti[:6]) == (tw * len(planes), th, tw, th, len(planes), 1) and ti[6] == 1 and ti[7] == D.SHAPE_COUNTS[(tw, th)][0]
    coefs = coefs.reshape(len(planes), ti[7], 512)
    for k, case in enumerate(D.BATCHES[name]):
        bad = np.argwhere(coefs[k] != planes[k])
        assert not bad.size, "%s: %d nodes differ from the oracle's walk, first %s" % (case, len(bad), bad[0])
    assert (planes == D.NONE).any()  # None entries are part of the comparison ...
    some = D.lattice(tw, th).some
    assert all(np.array_equal(p == D.NONE, ~some) for p in planes)  # ... and no Some node holds their value


@pytest.mark.parametrize("name", sorted(D.BATCHES))
def test_the_parser_returns_the_parameters_byte_for_byte(name):
    frv = D.batch(name)[0]
    ti, words, n_words, models, off, vp, wp = emit.tiled_parse_coded(frv)
    for k, case in enumerate(D.BATCHES[name]):
        r = D.built(case)
        assert vp[k].tobytes() == r["vp"].tobytes() and wp[k].tobytes() == r["wp"].tobytes(), case
        for b, m in enumerate(r["models"]):  # the models the file carries are the scaled histogram's
            if m is not None:
                assert (int(models[k, b, 0]), int(models[k, b, 1])) == (m[3], len(m[2])) and np.array_equal(off[k, b, : len(m[2])], m[2]), (case, b)
    nan = D.built("all_nan")
    assert np.isnan(nan["vp"]).all() and np.isnan(nan["wp"]).all()


def test_the_shapes_are_the_ones_the_docstring_states():
    for shape, (f, n_some) in D.SHAPE_COUNTS.items():
        L = D.lattice(*shape)
        assert (L.F, len(L.nodes)) == (f, n_some)
    assert D.lattice(*D.SMALL).levels[2] < 64, "DC, root and level 1 share one chunk"
    assert D.lattice(*D.LARGE).levels[1] > 64 and D.lattice(*D.LARGE).F >= 33, "DC and root entries fill more than one chunk"


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_generator_conditions_and_cells(name):
    c, r = D.CASES[name], D.built(name)
    L = D.lattice(*c["shape"])
    # the generator conditions
    assert r["symbol"].min() >= 0 and r["symbol"].max() <= 1022
    assert D.histogram_violations(r["hist_scaled"]) == []
    assert c["multiplier"] in D.MULTIPLIERS and np.array_equal(r["hist_scaled"], r["hist"] * np.uint32(r["multiplier_used"]))
    assert int(r["hist"].sum()) == len(L.nodes) and not (r["plane"][L.some] == D.NONE).any()
    for i in r["moved"]:  # a moved symbol stepped off INT32_MIN and nothing else
        assert emit_oracle.unpack_signed((int(r["symbol"][i]) - 1) % 1023) + int(r["prediction"][i]) in (D.NONE, D.NONE + 2 ** 32, D.NONE - 2 ** 32)
    # the stream is the plane's: the wrapped sum of every step is what the node holds
    assert np.array_equal((r["unwrapped"] + 2 ** 31) % 2 ** 32 - 2 ** 31, r["plane"].reshape(-1)[L.own])
    # the cells are computed from the neighbours the plan's tables name: they give the oracle's contexts
    bucket, prediction = D.contexts_restated(r)
    assert np.array_equal(bucket, r["bucket"]) and np.array_equal(prediction, r["prediction"])
    lf = np.flatnonzero(L.heap < 2)  # (the bound that makes an LF difference of 2^31 unreachable)
    assert (np.abs(r["plane"].reshape(-1)[L.own[lf]].astype(np.int64)) <= D.LF_BOUND * (np.arange(lf.size) + 1)).all()
    got = D.cells_of(r)
    assert D.WANT[name] <= got, sorted(D.WANT[name] - got)


def test_the_cases_reach_every_cell_and_every_family():
    assert set(D.WANT) == set(D.CASES) and sorted(D.BATCHES["small"] + D.BATCHES["large"]) == sorted(D.CASES)
    reached = set().union(*D.WANT.values())
    assert not set(D.CELLS) - reached, sorted(set(D.CELLS) - reached)
    assert len(D.CELLS) == 4 + 10 + 30 + 3 + 8
    rules = {c["rule"] if isinstance(c["rule"], str) else c["rule"][0] for c in D.CASES.values()}
    assert rules == set(D.RULES) and {c["multiplier"] for c in D.CASES.values()} == set(D.MULTIPLIERS)
    used = {D.built(n)["multiplier_used"] for n in D.CASES}
    assert 1 << 20 in used, "no case keeps the largest multiplier"
    intercepts = {float(v) for n in D.CASES if n.startswith("edges") for v in D.CASES[n]["wp"][:, 0]}
    assert intercepts == {float(np.float32(v)) for v in (2.999, 3.0, 29.999, 30.0, 31.0, 32.0, 4294967296.0)}


def test_symbol_1023_is_what_the_generator_must_stay_clear_of():
    """a used symbol 1023 makes the model's last frequency wrap: histogram_violations names it, and the scaled histogram of a wide bucket is halved until its
    Laplace value in slot 1023 is gone"""
    hist = np.zeros((10, 1024), np.uint32)
    hist[9, :8] = 100
    hist[9, 1023] = 1
    assert "symbol 1023 is used" in D.histogram_violations(hist)
    hist[9, 1023] = 0
    scaled, m = D.scaled_histogram(hist, 1 << 20)
    assert m < 1 << 20 and D.histogram_violations(scaled) == [] and D.histogram_violations(hist.astype(np.uint64) * (1 << 20))


def test_a_some_int_min_is_read_as_none_by_the_host_decoder():
    """value parameters 1.5 on uniform symbols, the avoidance off: the oracle holds Some(i32::MIN) apart from None, a flat plane cannot. What the host does today:
    it differs from the oracle, and it either returns a plane or refuses with one of its two messages."""
    s = D.sentinel()
    L = D.lattice(*D.SMALL)
    assert (s["plane"][L.some] == D.NONE).any() and (L.seen(s["plane"]) == D.NONE).any()
    assert all(not (L.seen(D.walk(*D.SMALL, s["vp"], s["wp"], "uniform", seed, avoid_int_min=False)["plane"]) == D.NONE).any() for seed in range(s["seed"]))
    frv = D.file_of([s])
    assert emit.tiled_info(frv)[7] == L.F
    try:
        coefs = emit.tiled_decode(frv)[1].reshape(L.F, 512)
        verdict = "plane"
        assert not np.array_equal(coefs, s["plane"]), "the host decoder read a Some(i32::MIN) as the oracle does"
        # decode_channel's written rule, `x == kNone ? 0 : x`: up to the first step whose context read the value, the planes agree
        first = int(np.flatnonzero((L.seen(s["plane"]) == D.NONE).any(axis=1))[0])
        assert np.array_equal(coefs.reshape(-1)[L.own[:first]], s["plane"].reshape(-1)[L.own[:first]])
    except emit.EmitError as e:
        verdict = "truncated" if "stream truncated" in str(e) else "mismatch"
        assert verdict == "truncated" or "stream does not match the model" in str(e), e
    assert verdict == SENTINEL_HOST, "the host decoder's verdict on the sentinel file changed: %s" % verdict
