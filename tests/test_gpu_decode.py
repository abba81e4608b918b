"""The rANS and context decoder on the device (K13, k13_decode.hip; include/fri_hip.h "the rANS and context decoder on the device"). The reference throughout is
the host decoder, emit.tiled_decode, which tests/test_emit.py holds to the oracle's literal decoder:

- the planes entry on the coded planes of whole files (emit.tiled_parse_coded): coefficients exact, None entries included, every status 0, with strides larger
  than needed and every array between guard bytes;
- damaged planes - cut short, one word flipped - give the host decoder's verdict as a status, the other planes of the batch stay exact, and the run ends clean;
- crafted planes (tests/decode_cases.py: parameters, symbols and models no encoder of ours makes) three ways - the oracle's walk, the host decoder, the device -
  whole and bounded by a level; cut short, the status names the very step at which a Python replay of the coder runs dry; a decoded Some(i32::MIN); model lists
  the host parser never produces, against the file that carries the same list;
- the composed entries against the inverse kernel on the host decoder's planes, byte for byte; files K11 coded parse back to the planes that went in;
- the same bytes in every run, and from a captured graph; argument errors; fri_driver decode-file --device-rans."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import frave_amd as fa
import frave_amd.api as api
import frave_amd.emit as emit
from frave_amd.api import DECODE_BAD_MODEL, DECODE_BAD_SLOT, DECODE_TRUNCATED, PlanTiled, PlanTiled420  # noqa: F401  (without the feature the module fails here)
from tests import decode_cases as D
from tests import preview_ref
from tests.coded_cases import file_of_image, tiled420_file, tiled_file
from tests.common import gen_image
from tests.test_gpu_instances import Guarded
from tests.tiled_ref import mixed_image, parse_frit

tiled_parse_coded = emit.tiled_parse_coded  # (without the feature the module fails here)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3
NONE = -(2 ** 31)


@pytest.fixture(scope="module")
def ctx():
    c = fa.Context(0)
    yield c
    c.close()


# ---- the files ------------------------------------------------------------------------------------------------------------------------------------------------

def _flat_tiles_image():
    """104 x 100 in 52 x 50 tiles: tiles 0 and 3 are black - every coefficient is 0 (a grey tile is not flat at its rim, where cells reach past the pixels), and
    every context is empty but the ones the zeros fall into"""
    img = mixed_image(104, 100, 1, 52, 11).copy()
    img[:50, :52], img[50:, 52:] = 0, 0
    return img


@functools.lru_cache(maxsize=None)
def _case(name):
    """(frit bytes, tile_w, tile_h) of a named file"""
    if name == "flat":
        return file_of_image(_flat_tiles_image(), 52, 50, 100)[0], 52, 50
    if name == "noise":
        return file_of_image(gen_image("noise", 100, 70, 1, 9), 52, 50, 100)[0], 52, 50
    if name == "one_tile_512":
        tw, th = api.tile_shape(512, 512, 512)
        return file_of_image(gen_image("smooth", tw, th, 1, 2), tw, th, 100)[0], tw, th
    w, h, c, tw, th, quality = (int(v) for v in name.split("x"))
    flags = {}
    if c == 3 and w == 334:  # the planes are labelled Y, Cb, Cr: the reversible transform for the lossless file, JFIF for the lossy one
        flags = dict(rct=True) if quality == 100 else dict(ycbcr=True)
    return tiled_file(w, h, c, tw, th, quality, **flags)[0], tw, th


PLANE_CASES = ["100x70x1x52x50x100", "100x70x1x52x50x50", "250x250x1x125x125x100", "250x250x1x125x125x50", "334x350x3x167x117x100", "334x350x3x167x117x50", "flat", "noise",
               "one_tile_512"]


@functools.lru_cache(maxsize=None)
def _reference(frv):
    """the host decoder's planes [P][F][512]"""
    ti, coefs = emit.tiled_decode(frv)
    return coefs.reshape(-1, ti[7], 512)


# ---- the planes entry -----------------------------------------------------------------------------------------------------------------------------------------

class Decode:
    """one fri_hip_decode_planes_dev call on the coded planes of a file: every array in a Guarded buffer of its own, strides larger than needed"""

    def __init__(self, ctx, tw, th, coded, word_pad=3, coef_pad=8):
        import torch

        self.torch = torch
        words, n_words, models, off, vp, wp = coded[-6:]
        self.planes = n_words.size
        self.plan = fa.Plan(ctx, tw, th, 1)
        self.plan.set_stream_order()
        self.F = self.plan.num_cells
        self.word_stride, self.coef_stride = words.shape[1] + word_pad, self.F * 512 + coef_pad
        p = self.planes
        self.inputs = {}
        for i, (name, a, row) in enumerate((("words", words, 4 * self.word_stride), ("n_words", n_words, 4), ("models", models, 160), ("off", off, 20480), ("vp", vp, 72),
                                            ("wp", wp, 72))):
            rows = np.ascontiguousarray(a).reshape(p, -1).view(np.uint8)
            g = Guarded(torch, rows.shape[1], p, row, salt=20 + i)
            g.put(torch, list(rows))
            self.inputs[name] = (g, rows.copy())
        self.coefs = Guarded(torch, 4 * self.F * 512, p, 4 * self.coef_stride, salt=31)
        self.status = Guarded(torch, 16, p, 16, salt=32)
        scratch = api.decode_scratch_bytes(p)
        assert scratch >= p * 2 * 10 * 1024 * 4
        self.d_scratch = torch.empty(scratch + 256, dtype=torch.uint8, device="cuda")
        self.scratch_ptr = (self.d_scratch.data_ptr() + 255) & ~255

    def launch(self, stream=0, **override):
        i = {name: g for name, (g, rows) in self.inputs.items()}
        a = dict(plan=self.plan, n_planes=self.planes, word_stride=self.word_stride, coef_stride=self.coef_stride, coefs=self.coefs.ptr, scratch=self.scratch_ptr, words=i["words"].ptr)
        a.update(override)
        return api.decode_planes_dev(a["plan"], a["n_planes"], a["words"], a["word_stride"], i["n_words"].ptr, i["models"].ptr, i["off"].ptr, i["vp"].ptr, i["wp"].ptr, a["coefs"],
                                     a["coef_stride"], self.status.ptr, a["scratch"], stream, timed=override.get("timed", False), levels=override.get("levels"))

    def read(self):
        """(coefs int32 [P][F][512], status uint32 [P][4]); asserts that nothing outside the outputs changed, the inputs included"""
        for name, (g, rows) in self.inputs.items():
            regions, intact = g.get(self.torch)
            assert intact and np.array_equal(np.stack(regions), rows), "K13 wrote to its input %s or around it" % name
        regions, intact = self.coefs.get(self.torch)
        assert intact, "K13 wrote outside a plane's coefficients"
        coefs = np.stack(regions).view(np.int32).reshape(self.planes, self.F, 512)
        regions, intact = self.status.get(self.torch)
        assert intact, "K13 wrote outside the status"
        return coefs, np.stack(regions).view(np.uint32).reshape(self.planes, 4)

    def raw(self):
        self.torch.cuda.synchronize()
        return [g.raw.cpu().numpy().copy() for g in (self.coefs, self.status)]

    def clear(self):
        for g in (self.coefs, self.status):
            g.raw.copy_(self.torch.from_numpy(g.fill))

    def close(self):
        self.plan.close()


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return "" if not bad.size else "%d differ, first at plane %d cell %d node %d: %d, want %d" % (len(bad), *bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", PLANE_CASES)
def test_planes_equal_the_host_decoder(ctx, name):
    frv, tw, th = _case(name)
    coded = tiled_parse_coded(frv)
    want = _reference(frv)
    models = coded[3]
    if name == "flat":  # FRI_EMIT_EMPTY_OK's context: max_freq_bits 8, nothing listed
        assert ((models[[0, 3], :, 0] == 8) & (models[[0, 3], :, 1] == 0)).sum(axis=1).min() >= 9
    if name == "noise":  # long off-distribution lists: the normalisation has slots to collapse
        assert models[:, :, 1].max() >= 100
    if name == "one_tile_512":  # the largest context holds 2^16 symbols or more: its model is scaled to 2^16, and frequencies up to that need more than 16 bits
        assert want.shape[0] == 1 and models[0, :, 0].max() >= 16
    d = Decode(ctx, tw, th, coded)
    d.launch()
    coefs, status = d.read()
    d.close()
    assert not status.any(), status[status.any(axis=1)]
    assert (want == NONE).any() or name == "one_tile_512"
    assert _first_difference(coefs, want) == ""


# ---- damaged planes -------------------------------------------------------------------------------------------------------------------------------------------

def _with_plane_data(frv, plane_words, channels, plane, new_words):
    """the file with plane `plane`'s rANS data replaced by new_words: the DAT segment's length and bytes, and the table behind it"""
    f = parse_frit(frv)
    t = plane // channels
    old = plane_words.astype("<u4").tobytes()
    payload = f["payloads"][t]
    at = payload.index(old)
    assert payload.count(old) == 1 and payload[at - 10 : at - 8] == b"\xff\xb4" and struct.unpack_from("<Q", payload, at - 8)[0] == len(old)
    new = np.asarray(new_words, np.uint32).astype("<u4").tobytes()
    payloads = list(f["payloads"])
    payloads[t] = payload[: at - 8] + struct.pack("<Q", len(new)) + new + payload[at + len(old):]
    table, pos = [], f["offsets"][0]
    for p in payloads:
        table.append(pos)
        pos += len(p)
    return frv[:32] + struct.pack("<%dQ" % (len(table) + 1), *table, pos) + b"".join(payloads)


def _host_verdict(frv):
    """(planes or None, the host decoder's error or "")"""
    try:
        return _reference(frv), ""
    except emit.EmitError as e:
        return None, str(e)


def test_truncated_planes_report_it_and_the_rest_of_the_batch_is_exact(ctx):
    frv, tw, th = _case("334x350x3x167x117x50")
    ti, words, n_words, models, off, vp, wp = tiled_parse_coded(frv)
    want = _reference(frv)
    assert n_words.size == 18
    cuts = {4: 7, 11: 20 + int(n_words[11]) // 2}
    for plane, n in cuts.items():  # the host decoder refuses the same tiles
        planes, err = _host_verdict(_with_plane_data(frv, words[plane, : n_words[plane]], 3, plane, words[plane, :n]))
        assert planes is None and err.startswith("tile %d: channel %d: " % divmod(plane, 3)) and "truncated" in err, err
    cut = n_words.copy()
    for plane, n in cuts.items():
        cut[plane] = n
    d = Decode(ctx, tw, th, (words, cut, models, off, vp, wp))
    d.launch()
    coefs, status = d.read()
    d.close()
    for plane in range(18):
        if plane in cuts:
            assert status[plane, 0] == DECODE_TRUNCATED and status[plane, 1] >= 1 and not status[plane, 2:].any()
        else:
            assert not status[plane].any() and _first_difference(coefs[plane : plane + 1], want[plane : plane + 1]) == "", plane
    assert status[4, 1] == 1  # fewer words than the ten states: decoding never started


# seed -> True where the host decoder refuses the file with that flip, chosen on the CPU by running emit.tiled_decode on the flips of seeds 0 .. 1499 of FLIP_CASE
# (`_flip` is the whole recipe): the first four seeds, and the first four of the eight whose file still decodes to the end - to other coefficients.
FLIP_CASE = "100x70x1x52x50x50"
FLIPS = {0: True, 1: True, 2: True, 3: True, 298: False, 487: False, 506: False, 575: False}


def _flip(frv, seed):
    """(damaged file, plane): one bit of one word of the body of one plane flipped. (The host nearly always runs out of words behind a flip: an intact stream
    leaves every state at exactly 2^31 behind its last symbol, a damaged one below it more often than not, and that renormalisation finds no word. About one seed
    in two hundred decodes to the end.)"""
    ti, words, n_words, *_ = tiled_parse_coded(frv)
    rng = np.random.default_rng(seed)
    plane = int(rng.integers(n_words.size))
    at = int(rng.integers(20, n_words[plane]))
    new = words[plane, : n_words[plane]].copy()
    new[at] ^= np.uint32(1 << int(rng.integers(32)))
    return _with_plane_data(frv, words[plane, : n_words[plane]], ti[6], plane, new), plane


@pytest.mark.parametrize("seed", sorted(FLIPS))
def test_a_flipped_word_gives_the_host_decoders_verdict(ctx, seed):
    frv, tw, th = _case(FLIP_CASE)
    bad, plane = _flip(frv, seed)
    planes, err = _host_verdict(bad)
    assert (planes is None) == FLIPS[seed], "the host decoder's verdict on seed %d changed: %r" % (seed, err)
    d = Decode(ctx, tw, th, tiled_parse_coded(bad))
    d.launch()
    coefs, status = d.read()  # (the run ended clean, and inside its buffers)
    d.close()
    others = [k for k in range(4) if k != plane]
    assert not status[others].any() and _first_difference(coefs[others], _reference(frv)[others]) == ""
    if planes is None:
        assert status[plane, 0] in (DECODE_TRUNCATED, DECODE_BAD_SLOT) and status[plane, 1] >= 1, (err, status[plane])
        assert ("truncated" in err) == (status[plane, 0] == DECODE_TRUNCATED)
    else:
        assert not status[plane].any() and _first_difference(coefs, planes) == ""


def test_the_flips_cover_both_verdicts():
    assert len(FLIPS) == 8 and sum(FLIPS.values()) >= 3 and sum(not v for v in FLIPS.values()) >= 3


def test_a_bad_model_is_reported_and_nothing_is_decoded(ctx):
    frv, tw, th = _case("100x70x1x52x50x50")
    ti, words, n_words, models, off, vp, wp = tiled_parse_coded(frv)
    bad = models.copy()
    bad[1, 3, 1] = 1025  # a list longer than the alphabet
    d = Decode(ctx, tw, th, (words, n_words, bad, off, vp, wp))
    d.launch()
    coefs, status = d.read()
    d.close()
    want = _reference(frv)
    assert status[1].tolist() == [DECODE_BAD_MODEL, 1, 0, 0] and not status[[0, 2, 3]].any()
    assert _first_difference(coefs[[0, 2, 3]], want[[0, 2, 3]]) == ""
    assert np.array_equal(coefs[1], np.where(want[1] == NONE, NONE, 0))  # the initial values: 0 on a Some node, None elsewhere


# ---- crafted planes (tests/decode_cases.py) ---------------------------------------------------------------------------------------------------------------------
# Planes no encoder of ours makes: saturated, NaN and infinite parameters, widths on the bucket edges, coefficients at the int32 limits, models scaled up to
# max_freq_bits 30 and lists of 700 symbols. tests/test_decode_cases_host.py holds them to the host decoder and to the cells they reach.

@pytest.mark.parametrize("name", sorted(D.BATCHES))
def test_crafted_planes_equal_the_host_decoder(ctx, name):
    frv, tw, th, oracle = D.batch(name)
    want = _reference(frv)
    assert _first_difference(want, oracle) == ""
    d = Decode(ctx, tw, th, tiled_parse_coded(frv))  # one launch: every plane its own parameters, models and word count
    assert d.planes == len(D.BATCHES[name]) <= 16
    d.launch()
    coefs, status = d.read()
    d.close()
    assert not status.any(), [(D.BATCHES[name][k], status[k].tolist()) for k in np.flatnonzero(status.any(axis=1))]
    for k, case in enumerate(D.BATCHES[name]):
        assert _first_difference(coefs[k : k + 1], want[k : k + 1]) == "", case


def test_crafted_planes_level_bounded(ctx):
    frv, tw, th, oracle = D.batch("small")
    d = Decode(ctx, tw, th, tiled_parse_coded(frv))
    bits = d.plan.valid_bits()
    for levels in (0, 1, 2, 5, 8):
        d.clear()
        d.launch(levels=levels)
        coefs, status = d.read()
        assert not status.any(), (levels, status)
        compact = emit.tiled_decode_levels(frv, levels)[1].reshape(-1, d.F, 1 << levels)
        assert np.array_equal(compact, oracle[:, :, : 1 << levels])
        want = preview_ref.expand(compact, bits)
        for k, case in enumerate(D.BATCHES["small"]):
            assert _first_difference(coefs[k : k + 1], want[k : k + 1]) == "", (levels, case)
    d.close()


TRUNCATED_CASES = ("groups", "negative_width_x2^20")  # every context at max_freq_bits 8; one at 30


def _cut_plane(L, plane, step):
    """what a plane refused at `step` holds: the reference up to that step, the initial values behind it"""
    out = np.where(L.some, 0, NONE).astype(np.int32).reshape(-1)
    out[L.own[:step]] = plane.reshape(-1)[L.own[:step]]
    return out.reshape(plane.shape)


def test_truncated_crafted_planes_stop_at_the_step_the_coder_runs_dry(ctx):
    frv, tw, th, oracle = D.batch("small")
    ti, words, n_words, models, off, vp, wp = tiled_parse_coded(frv)
    L = D.lattice(tw, th)
    rows, cuts, steps = [], [], {}
    for name in TRUNCATED_CASES:
        k, r = D.BATCHES["small"].index(name), D.built(name)
        bits = [m[3] for m in r["models"] if m is not None]
        assert (max(bits) == 8) if name == "groups" else (max(bits) >= 24)
        n = int(n_words[k])
        steps[k] = D.word_steps(words[k, :n], r["stream"], r["models"])
        assert n > 20 + 65 and (steps[k][:20] == -1).all() and (np.diff(steps[k][20:]) >= 0).all()
        # no body word, one, the 64th and the 65th (the window of 64 stream words turns there), all but the last; and the plane as it is
        for cut in (20, 21, 20 + 63, 20 + 64, n - 1, n):
            rows.append(k), cuts.append(cut)
    rows = np.array(rows)
    d = Decode(ctx, tw, th, (words[rows], np.array(cuts, np.uint32), models[rows], off[rows], vp[rows], wp[rows]))
    d.launch()
    coefs, status = d.read()
    d.close()
    for p, (k, cut) in enumerate(zip(rows, cuts)):
        if cut == n_words[k]:
            assert not status[p].any() and _first_difference(coefs[p : p + 1], oracle[k : k + 1]) == "", (D.BATCHES["small"][k], cut)
            continue
        step = int(steps[k][cut])  # the step that takes word `cut`
        assert status[p].tolist() == [DECODE_TRUNCATED, 1 + step, 0, 0], (D.BATCHES["small"][k], cut, step, status[p].tolist())
        assert _first_difference(coefs[p : p + 1], _cut_plane(L, oracle[k], step)[None]) == "", (D.BATCHES["small"][k], cut)
    # the same through a word_stride smaller than n_words: no word is read at or past the stride
    pair = np.array([D.BATCHES["small"].index(name) for name in TRUNCATED_CASES])
    shortest = int(n_words[pair].min())
    for stride in (20, 21, 20 + 63, 20 + 64, shortest - 1):
        d = Decode(ctx, tw, th, (np.ascontiguousarray(words[pair, :stride]), n_words[pair], models[pair], off[pair], vp[pair], wp[pair]), word_pad=0)
        assert d.word_stride == stride
        d.launch()
        coefs, status = d.read()
        d.close()
        for p, k in enumerate(pair):
            step = int(steps[k][stride])
            assert status[p].tolist() == [DECODE_TRUNCATED, 1 + step, 0, 0], (D.BATCHES["small"][k], stride, step, status[p].tolist())
            assert _first_difference(coefs[p : p + 1], _cut_plane(L, oracle[k], step)[None]) == "", (D.BATCHES["small"][k], stride)


def _verdict_matches(status, err):
    """a refusal of the host decoder as a status: non-zero, and "stream truncated" is DECODE_TRUNCATED (as for the flipped words)"""
    return status[0] != 0 and status[1] >= 1 and ("truncated" in err) == (status[0] == DECODE_TRUNCATED)


def test_a_some_int_min_decodes_as_the_host_decodes_it(ctx):
    """a decoded Some(i32::MIN) is a value the planes cannot hold (None is INT32_MIN): decode_channel reads it back as None, `x == kNone ? 0 : x`, and so does K13.
    The oracle, which keeps the two apart, decodes other coefficients from there on (tests/test_decode_cases_host.py)."""
    s = D.sentinel()
    tw, th = s["shape"]
    frv = D.file_of([s])
    planes, err = _host_verdict(frv)
    d = Decode(ctx, tw, th, tiled_parse_coded(frv))
    d.launch()
    coefs, status = d.read()
    d.close()
    if planes is None:
        assert _verdict_matches(status[0], err), (err, status[0].tolist())
    else:
        assert not status.any() and _first_difference(coefs, planes) == ""
        assert (planes[0][D.lattice(tw, th).some] == NONE).any() and _first_difference(coefs, s["plane"][None]) != ""


def _list_variants(models, off):
    """model lists the host parser never produces, from one plane's models [10][4] and lists [10][1024]: name -> (models, off, the model is unchanged)"""
    out = {}

    def variant(name, same):
        m, o = models.copy(), off.copy()
        out[name] = (m, o, same)
        return m, o

    b = int(np.argmax(models[:, 1]))  # the longest list
    n = int(models[b, 1])
    listed = off[b, :n].copy()
    assert 512 <= n < 1024 and len(set(listed.tolist())) == n and (np.diff(listed.astype(int)) > 0).all() and listed.max() < 1024
    variant("as the file carries it", True)
    m, o = variant("duplicates up to n_off = 1024", True)
    o[b, n:] = listed[: 1024 - n]
    m[b, 1] = 1024
    m, o = variant("every entry twice, side by side", True)
    q = min(n, 1024 - n) - 1
    o[b, : n + q] = np.concatenate([np.repeat(listed[:q], 2), listed[q:]])
    m[b, 1] = n + q
    m, o = variant("descending", True)
    o[b, :n] = listed[::-1]
    m, o = variant("values 1024..65535 between the entries", True)
    extra = np.array([1024, 65535, 1023 + 1024, 2048, 40000, 1025], np.uint16)
    o[b, : n + extra.size] = np.insert(listed, [0, 1, n // 2, n // 2, n - 1, n], extra)
    m[b, 1] = n + extra.size
    m, o = variant("n_off = 1024, the rest above the alphabet", True)
    o[b, n:] = (1024 + 61 * np.arange(1024 - n)).astype(np.uint16)
    m[b, 1] = 1024
    assert o[b, n:].min() >= 1024
    m, o = variant("entries moved above the alphabet", False)  # those symbols lose their slot: another model
    o[b, : n : 5] += np.uint16(1024)
    m, o = variant("symbols listed that the plane never used", False)  # they take a slot each: another model
    unused = np.setdiff1d(np.arange(600, 1023), listed)[: 1024 - n].astype(np.uint16)
    o[b, n : n + unused.size] = unused
    m[b, 1] = n + unused.size
    low = [c for c in range(10) if models[c, 0] == 8]
    assert len(low) >= 8
    m, o = variant("max_freq_bits 0..7 where the file has 8", True)  # finalize's floor to 8
    for i, c in enumerate(low):
        m[c, 0] = i % 8
    return out


def test_model_lists_the_host_parser_never_produces(ctx):
    """duplicates, values past the alphabet, descending order, n_off = 1024 exactly, a max_freq_bits below the floor: in at the planes entry directly. The reference
    is the file that carries the same list (emit.tiled_encode_from_coded) through the host decoder; where the host refuses it, a status."""
    frv, tw, th, oracle = D.batch("small")
    ti, words, n_words, models, off, vp, wp = tiled_parse_coded(frv)
    k = D.BATCHES["small"].index("negative_width_lists")
    variants = _list_variants(models[k], off[k])
    names = sorted(variants)
    assert len(names) <= 16
    host = []
    for name in names:
        m, o, same = variants[name]
        one = emit.tiled_encode_from_coded(tw, th, tw, th, words[k : k + 1], n_words[k : k + 1], m[None], o[None], vp[k : k + 1], wp[k : k + 1])
        p_models, p_off = tiled_parse_coded(one)[3:5]
        assert np.array_equal(p_models[0, :, :2], m[:, :2]) and all(np.array_equal(p_off[0, c, : m[c, 1]], o[c, : m[c, 1]]) for c in range(10)), name
        planes, err = _host_verdict(one)
        if same:  # the host reads the same model out of it: the oracle's plane
            assert planes is not None and _first_difference(planes, oracle[k : k + 1]) == "", (name, err)
        host.append((planes, err))
    rows = np.full(len(names), k)
    d = Decode(ctx, tw, th, (words[rows], n_words[rows], np.stack([variants[n][0] for n in names]), np.stack([variants[n][1] for n in names]), vp[rows], wp[rows]))
    d.launch()
    coefs, status = d.read()  # (every guard untouched)
    d.close()
    for p, (name, (planes, err)) in enumerate(zip(names, host)):
        if planes is None:
            assert _verdict_matches(status[p], err), (name, err, status[p].tolist())
        else:
            assert not status[p].any() and _first_difference(coefs[p : p + 1], planes) == "", (name, status[p].tolist())


# ---- the composed entries ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,transform", [("100x70x1x52x50x100", COLOUR_NONE), ("334x350x3x167x117x50", COLOUR_YCBCR), ("334x350x3x167x117x100", COLOUR_RCT)])
def test_composed_decode_equals_the_inverse_of_the_host_decoders_planes(ctx, name, transform):
    frv, tw, th = _case(name)
    coded = tiled_parse_coded(frv)
    ti = coded[0]
    assert (ti.rct, ti.ycbcr) == (transform == COLOUR_RCT, transform == COLOUR_YCBCR)
    T = PlanTiled(ctx, ti[0], ti[1], ti[6], tw, th)
    with pytest.raises(fa.FriHipError) as e:  # without the stream order: the encodes' error
        T.decode_coded(coded)
    assert e.value.code == -1
    T.set_stream_order()
    T.tile.set_colour_transform(transform)
    T.tile.set_dequantiser(fa.DEQUANT_MIDPOINT if ti.quality else fa.DEQUANT_REFERENCE)
    qm = fa.quality_matrix(ti.quality) if ti.quality else None
    want = T.decode_image_tiled(emit.tiled_decode(frv)[1], qm)
    got, status = T.decode_coded(coded, qm)
    assert not status.any() and np.array_equal(got, want)
    # a refused plane: -1 with the status filled
    ti, words, n_words, models, off, vp, wp = coded
    cut = n_words.copy()
    cut[1] = 19
    with pytest.raises(fa.FriHipError) as e:
        T.decode_coded((words, cut, models, off, vp, wp), qm)
    assert e.value.code == -1 and e.value.status[1].tolist() == [DECODE_TRUNCATED, 1, 0, 0] and not np.delete(e.value.status, 1, axis=0).any()
    T.close()


def test_composed_decode_of_a_tiled_420_file(ctx):
    quality = 60
    frv = tiled420_file(100, 70, 52, 50, quality)[0]
    coded = tiled_parse_coded(frv)
    assert coded[0].s420
    T = PlanTiled420(ctx, 100, 70, 52, 50)
    T.set_stream_order()
    want = T.decode_image_tiled420(emit.tiled_decode(frv)[1], quality)
    got, status = T.decode_coded(coded, quality)
    assert status.shape == (12, 4) and not status.any() and np.array_equal(got, want)
    T.close()


def test_files_k11_coded_parse_back_to_the_planes_that_went_in(ctx):
    w, h, c, tw, th = 334, 350, 3, 167, 117
    img = mixed_image(w, h, c, tw, 3)
    T = PlanTiled(ctx, w, h, c, tw, th)
    T.set_stream_order()
    T.tile.set_colour_transform(COLOUR_RCT)
    words, n_words, models, off, status, vp, wp = T.encode_image_tiled_coded(img)
    assert not status.any()
    frv = emit.tiled_encode_from_coded(w, h, tw, th, words, n_words, models, off, vp, wp, rct=True)
    ti, p_words, p_n, p_models, p_off, p_vp, p_wp = tiled_parse_coded(frv)
    assert np.array_equal(p_n, n_words) and np.array_equal(p_models[:, :, :2], models[:, :, :2]) and not p_models[:, :, 2:].any()
    assert p_vp.tobytes() == vp.tobytes() and p_wp.tobytes() == wp.tobytes()
    for k in range(n_words.size):
        assert np.array_equal(p_words[k, : n_words[k]], words[k, : n_words[k]]), k
        for b in range(10):
            assert np.array_equal(p_off[k, b, : models[k, b, 1]], off[k, b, : models[k, b, 1]]), (k, b)
    got, dstatus = T.decode_coded((p_words, p_n, p_models, p_off, p_vp, p_wp))  # ... and decode to the image: the file is lossless
    assert not dstatus.any() and np.array_equal(got, img.reshape(-1))
    T.close()


# ---- the same bytes in every run, and from a graph -----------------------------------------------------------------------------------------------------------------

def test_reproducible_and_capturable(ctx):
    import torch

    hip = C.CDLL("libamdhip64.so")
    frv, tw, th = _case("334x350x3x167x117x100")
    d = Decode(ctx, tw, th, tiled_parse_coded(frv))
    d.launch()
    first = d.raw()
    coefs, status = d.read()
    assert not status.any() and _first_difference(coefs, _reference(frv)) == ""
    d.clear()
    d.launch()
    assert all(np.array_equal(a, b) for a, b in zip(first, d.raw())), "a second run wrote other bytes"
    us = d.launch(timed=True)
    assert us.shape == (2,) and (us > 0).all()
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    d.launch(stream=s.cuda_stream)  # a linear chain on one stream: two kernel nodes
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 2
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    d.clear()
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(ex, sp) == 0
    s.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(first, d.raw())), "the replay wrote other bytes"
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    d.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing(ctx):
    frv, tw, th = _case("100x70x1x52x50x100")
    d = Decode(ctx, tw, th, tiled_parse_coded(frv))
    before = d.raw()
    for kwargs in (dict(n_planes=0), dict(n_planes=65536), dict(words=0), dict(coefs=0), dict(scratch=0), dict(scratch=d.scratch_ptr + 8), dict(coefs=d.coefs.ptr + 4),
                   dict(coef_stride=d.F * 512 - 4), dict(coef_stride=d.F * 512 + 2), dict(plan=None)):
        with pytest.raises(fa.FriHipError) as e:
            d.launch(**kwargs)
        assert e.value.code == -1, kwargs
    bare = fa.Plan(ctx, tw, th, 1)  # no stream order: the error the encodes return
    with pytest.raises(fa.FriHipError) as e:
        d.launch(plan=bare)
    assert e.value.code == -1
    bare.close()
    host_only = fa.Plan(None, tw, th, 1)
    with pytest.raises(fa.FriHipError) as e:
        d.launch(plan=host_only)
    assert e.value.code == -3
    host_only.close()
    assert all(np.array_equal(a, b) for a, b in zip(before, d.raw()))
    assert api.decode_scratch_bytes(0) == 0 and api.decode_scratch_bytes(65536) == 0
    d.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_driver_decode_file_device_rans(ctx, tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    files = {"444": _case("334x350x3x167x117x50")[0], "420": tiled420_file(100, 70, 52, 50, 60)[0]}
    for name, frv in files.items():
        src, host, device = tmp_path / f"{name}.frv", tmp_path / f"{name}_host.ppm", tmp_path / f"{name}_device.ppm"
        src.write_bytes(frv)
        for dst, extra in ((host, []), (device, ["--device-rans"])):
            out = subprocess.run([driver, "decode-file", str(src), str(dst)] + extra, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0, out.stdout + out.stderr
        assert device.read_bytes() == host.read_bytes()
    src = tmp_path / "444.frv"
    out = subprocess.run([driver, "decode-file", str(src), str(tmp_path / "r.ppm"), "--device-rans", "--region", "0,0,8,8"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "out of scope" in out.stderr and not (tmp_path / "r.ppm").exists()
    frif = tmp_path / "tile.frv"
    frif.write_bytes(parse_frit(files["444"])["payloads"][0])
    out = subprocess.run([driver, "decode-file", str(frif), str(tmp_path / "t.ppm"), "--device-rans"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "one dependent chain per channel" in out.stderr and not (tmp_path / "t.ppm").exists()
    out = subprocess.run([driver, "decode-file", str(frif), str(tmp_path / "t.ppm")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
