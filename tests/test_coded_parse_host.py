"""fri_tiled_parse_coded (include/fri_emit.h): a `frit` file back to the coded planes it is made of, the inverse of fri_tiled_encode_from_coded and
fri_tiled_encode_from_coded420 - round trips byte for byte, the parameters, `info`, the size query and the refusals. CPU only."""
import ctypes as C

import numpy as np
import pytest

import frave_amd.emit as emit
from tests.coded_cases import tiled420_file, tiled_file
from tests.tiled_ref import parse_frit

tiled_parse_coded = emit.tiled_parse_coded  # (without the feature the module fails here)

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
W, H, TW, TH = 100, 70, 52, 50
CASES = [(1, 100), (1, 50), (3, 100), (3, 50)]  # (C, quality; 100: lossless)


def _file(case):
    c, quality = case
    return tiled_file(W, H, c, TW, TH, quality)


@pytest.mark.parametrize("case", CASES)
def test_parse_then_encode_from_coded_gives_the_file_back(case):
    c, quality = case
    frv, vp, wp = _file(case)
    ti, words, n_words, models, off, got_vp, got_wp = tiled_parse_coded(frv)
    info = emit.tiled_info(frv)
    assert tuple(ti) == tuple(info) and (ti.rct, ti.ycbcr, ti.quality, ti.s420) == (info.rct, info.ycbcr, info.quality, info.s420) == (False, False, quality % 100, False)
    planes = 4 * c
    assert words.shape == (planes, int(n_words.max())) and models.shape == (planes, 10, 4) and off.shape == (planes, 10, 1024)
    assert got_vp.tobytes() == np.ascontiguousarray(vp, np.float32).tobytes() and got_wp.tobytes() == np.ascontiguousarray(wp, np.float32).tobytes()
    assert (n_words >= 20).all() and not models[:, :, 2:].any() and (models[:, :, 1] <= 1024).all()
    # the words are the bytes between DAT and EOC: the payload carries them verbatim
    payloads = parse_frit(frv)["payloads"]
    for p in range(planes):
        assert words[p, : n_words[p]].astype("<u4").tobytes() in payloads[p // c]
    again = emit.tiled_encode_from_coded(W, H, TW, TH, words, n_words, models, off, got_vp, got_wp, quality=quality % 100)
    assert again == frv
    # a wider stride changes nothing
    ti2, words2, n2, models2, off2, vp2, wp2 = tiled_parse_coded(frv, int(n_words.max()) + 5)
    assert np.array_equal(n2, n_words) and np.array_equal(words2[:, : words.shape[1]], words) and not words2[:, words.shape[1]:].any()
    assert np.array_equal(models2, models) and np.array_equal(off2, off)
    assert emit.tiled_encode_from_coded(W, H, TW, TH, words2, n2, models2, off2, vp2, wp2, quality=quality % 100) == frv


def test_a_tiled_420_file_comes_back_in_plane_order():
    quality = 60
    frv, vp, wp = tiled420_file(W, H, TW, TH, quality)
    ti, words, n_words, models, off, got_vp, got_wp = tiled_parse_coded(frv)
    info = emit.tiled_info(frv)
    assert tuple(ti) == tuple(info) and ti.s420 and ti.ycbcr and ti.quality == quality
    assert n_words.shape == (12,) and got_vp.tobytes() == vp.astype(np.float32).tobytes() and got_wp.tobytes() == wp.astype(np.float32).tobytes()
    payloads = parse_frit(frv)["payloads"]
    for t in range(4):  # plane(t, Y) = t, plane(t, Cb) = n + 2 t, plane(t, Cr) = n + 2 t + 1
        at = 0
        for p in (t, 4 + 2 * t, 4 + 2 * t + 1):
            found = payloads[t].find(words[p, : n_words[p]].astype("<u4").tobytes(), at)
            assert found >= at
            at = found + 4 * int(n_words[p])
    assert emit.tiled_encode_from_coded420(W, H, TW, TH, words, n_words, models, off, got_vp, got_wp, quality) == frv


def _call(data, planes, stride, with_words=True):
    """fri_tiled_parse_coded through the C ABI: (rc, message, info, n_words)"""
    data = np.frombuffer(bytes(data), np.uint8)
    info, nw = np.zeros(8, np.uint32), np.zeros(max(planes, 1), np.uint32)
    words, models, off = np.zeros((max(planes, 1), max(stride, 1)), np.uint32), np.zeros((max(planes, 1), 10, 4), np.uint32), np.zeros((max(planes, 1), 10, 1024), np.uint16)
    vp, wp = np.zeros((max(planes, 1), 3, 6), np.float32), np.zeros((max(planes, 1), 3, 6), np.float32)
    err = C.create_string_buffer(256)
    rc = emit.load_library().fri_tiled_parse_coded(P(data), data.size, P(info), planes, P(words) if with_words else None, stride, P(nw), P(models), P(off), P(vp), P(wp), err, 256)
    return rc, err.value.decode(), [int(x) for x in info], nw, words


def test_size_query_and_a_short_stride():
    frv, vp, wp = _file((3, 50))
    ti, words, n_words, *_ = tiled_parse_coded(frv)
    want_info = [int(x) for x in np.asarray(tuple(ti))]
    want_info[6] = 3 | emit.QUALITY(50)
    # no room for the counts: -3 with info filled; words == NULL: info and the counts only
    rc, msg, info, nw, _ = _call(frv, 11, 0, with_words=False)
    assert rc == -3 and info == want_info and not nw.any()
    rc, msg, info, nw, words_out = _call(frv, 12, 0, with_words=False)
    assert rc == 0 and info == want_info and np.array_equal(nw, n_words) and not words_out.any()
    # one word short of the longest plane: the error names it, the counts are complete, the planes that fit are written
    longest = int(np.argmax(n_words))
    stride = int(n_words[longest]) - 1
    rc, msg, info, nw, words_out = _call(frv, 12, stride)
    assert rc == -2 and f"plane {longest}:" in msg and np.array_equal(nw, n_words)
    for p in range(12):
        if n_words[p] <= stride:
            assert np.array_equal(words_out[p, : n_words[p]], words[p, : n_words[p]])
    with pytest.raises(emit.EmitError) as e:
        tiled_parse_coded(frv, stride)
    assert f"plane {longest}:" in str(e.value) and np.array_equal(e.value.n_words, n_words)
    rc, msg, info, nw, words_out = _call(frv, 12, stride + 1)
    assert rc == 0 and np.array_equal(words_out, words)


def test_refusals():
    frv, vp, wp = _file((1, 100))
    f = parse_frit(frv)
    o = f["offsets"]
    dat = frv.index(b"\xff\xb4", o[1])  # tile 1's DAT marker
    bad = {
        "a frif file": f["payloads"][0],
        "cut in the table": frv[: 32 + 8 * 2 + 3],
        "cut in a payload header": frv[: o[2] + 9],
        "cut inside a DAT segment": frv[: dat + 2 + 8 + 40],
        "empty": b"",
    }
    for name, data in bad.items():
        rc, msg, info, nw, _ = _call(data, 4, 1 << 16)
        assert rc == -2 and "Malformed tiled image" in msg, (name, rc, msg)
        with pytest.raises(emit.EmitError):
            tiled_parse_coded(data)
    # the table and the headers intact, a payload's markers damaged: the payload's own parser refuses it, and the error names the tile
    b = bytearray(frv)
    b[dat + 1] = 0xB5
    rc, msg, info, nw, _ = _call(b, 4, 1 << 16)
    assert rc == -2 and msg.startswith("tile 1: ")
    # null pointers
    L = emit.load_library()
    data = np.frombuffer(frv, np.uint8)
    info = np.zeros(8, np.uint32)
    assert L.fri_tiled_parse_coded(None, data.size, P(info), 0, None, 0, None, None, None, None, None, None, 0) == -1
    assert L.fri_tiled_parse_coded(P(data), data.size, None, 0, None, 0, None, None, None, None, None, None, 0) == -1
    words = np.zeros((4, 16), np.uint32)
    assert L.fri_tiled_parse_coded(P(data), data.size, P(info), 4, P(words), 16, None, None, None, None, None, None, 0) == -1
