"""The device rANS coder's host side (K11, include/fri_hip.h "the rANS coder on the device"; fri_tiled_encode_from_coded / fri_coded_encode_image of
include/fri_emit.h). CPU only:

- tests/rans_ref.py - the reference the GPU tests hold K11 to - equals what the host emitter writes on the synthetic planes of tests/rans_cases.py, refusals
  included, and the oracle's independent division-form coder where that is defined;
- the container assembled from coded planes is byte for byte the container coded from streams, and decodes to the coefficients;
- csrc/rans_step.hpp, compiled with a main of its own (plain and with the host sanitizers): the reciprocal form of the step against the division form, and
  the Python restatement against both."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import frave_amd.emit as emit
from oracle import emit_oracle
from tests import rans_cases, rans_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ZERO_PARAMS = np.zeros((1, 3, 6), np.float32)


def parse_channel(frif):
    """(max_freq_bits [10], off lists [10], data bytes) of the single channel of a Luma `frif` file (serialize.rs:40-117)"""
    assert frif[:4] == b"frif" and frif[16:18] == b"\xff\xbb"
    o = 18 + 36 * 4
    bits, off = [], []
    for _ in range(10):
        assert frif[o:o + 2] == b"\xff\xb2"
        m, n = struct.unpack_from("<IQ", frif, o + 2)
        o += 14
        bits.append(m), off.append(list(struct.unpack_from("<%dH" % n, frif, o)))
        o += 2 * n
    assert frif[o:o + 2] == b"\xff\xb4"
    (n,) = struct.unpack_from("<Q", frif, o + 2)
    data = frif[o + 10:o + 10 + n]
    assert frif[o + 10 + n:] == b"\xff\xb8\xff\xdf"
    return bits, off, data


def host_plane(stream, hist, empty_ok=True):
    return emit.encode_image_from_streams(8, 8, stream[None], hist[None], ZERO_PARAMS, ZERO_PARAMS, empty_ok=empty_ok)


NAMES = ["n:%d" % n for n in rans_cases.LENGTHS] + ["batch:3"] + rans_cases.SPECIAL


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_what_the_host_emitter_writes(name):
    streams, hist = rans_cases.case(name)
    for s, h, ref in zip(streams, hist, rans_cases.reference(name)):
        if ref.status:  # the same outcome as the host: a refusal
            with pytest.raises(emit.EmitError):
                host_plane(s, h)
            continue
        bits, off, data = parse_channel(host_plane(s, h))
        assert bits == ref.max_freq_bits and off == ref.off
        assert data == ref.words.astype("<u4").tobytes(), name
        assert len(ref.words) <= len(s) + 20


def test_reference_equals_the_oracles_division_form_coder():
    """oracle/emit_oracle.py's rans_encode divides where the product multiplies by a reciprocal: an independent statement of the same stream"""
    for name in ("n:257", "n:4097", "one_each", "freq_one", "off_heavy", "collapse"):
        streams, hist = rans_cases.case(name)
        for s, h, ref in zip(streams, hist, rans_cases.reference(name)):
            ctxs = rans_ref.contexts_from_hist(h)
            assert ref.status == 0 and emit_oracle.rans_encode(rans_ref.split(s), ctxs) == ref.words.astype("<u4").tobytes()


def test_the_cases_are_what_their_names_say():
    ref = rans_cases.reference("nine_empty")[0]
    flush = ref.words[:20].reshape(10, 2)  # state 9 first: (low, high)
    assert all((int(lo), int(hi)) == (1 << 31, 0) for s, (lo, hi) in zip(range(9, -1, -1), flush) if s != 6) and (int(flush[3][0]), int(flush[3][1])) != (1 << 31, 0)
    assert ref.max_freq_bits == [8] * 10 and ref.off == [[]] * 10
    streams, hist = rans_cases.case("freq_one")
    c = rans_ref.contexts_from_hist(hist[0])[0]
    sym = int(streams[0][0]) & 1023
    assert c.freqs[sym] == 1 and c.max_freq_bits == 8 and hist[0][0].sum() == hist[0][0][sym] == 3
    streams, hist = rans_cases.case("off_heavy")
    assert sum(len(o) for o in rans_cases.reference("off_heavy")[0].off) > 400
    streams, hist = rans_cases.case("collapse")
    for h, b in zip(hist, (0, 1)):  # used slots collapse, and every one of them steals its count back
        final = rans_ref.contexts_from_hist(h)[b]
        assert rans_ref.collapsed_slots(h[b], b) > 5 and all(final.freqs[j] >= 1 for j in np.flatnonzero(h[b]))
    assert rans_ref.collapsed_slots(rans_cases.case("one_context")[1][0][3], 3) == 0
    streams, hist = rans_cases.case("symbol_1023")
    assert (hist[0][:, 1023] > 0).any()


def test_refusals_match_the_host():
    s, h = (a[0] for a in rans_cases.case("nine_empty"))
    ref = rans_ref.encode_plane(s, h, empty_ok=False)  # without the rule an empty context is the emitter's division by zero
    assert ref.status == rans_ref.BAD_MODEL
    with pytest.raises(emit.EmitError, match="empty context"):
        host_plane(s, h, empty_ok=False)
    s, h = (a[0].copy() for a in rans_cases.case("n:257"))
    s[100], s[31] = 12 << 10 | 5, 15 << 10 | 1  # buckets above 9: the histogram has no row for them
    ref = rans_ref.encode_plane(s, h)
    assert ref.status == rans_ref.BAD_BUCKET and ref.bucket_at == 101
    with pytest.raises(emit.EmitError, match="bucket"):
        host_plane(s, h)
    s, h = (a[0].copy() for a in rans_cases.case("n:257"))
    s[200] = (s[200] & ~np.uint16(1023)) | 1021  # a symbol the histogram does not count: its slot is empty
    s[17] = s[200]
    ref = rans_ref.encode_plane(s, h)
    assert ref.status == rans_ref.ZERO_FREQ and ref.zero_at == 201
    with pytest.raises(emit.EmitError, match="zero model frequency"):
        host_plane(s, h)


# ---- the container from coded planes --------------------------------------------------------------------------------------------------------------------------

def _coded_planes(streams, hist):
    """(words [planes][stride], n_words, models [planes][10][4], off [planes][10][1024]) from tests/rans_ref.py: every plane coded on the host"""
    planes = streams.reshape(-1, streams.shape[-1])
    refs = [rans_ref.encode_plane(s, h) for s, h in zip(planes, hist.reshape(-1, 10, 1024))]
    assert all(r.status == 0 for r in refs)
    stride = max(len(r.words) for r in refs) + 3
    words = np.full((len(refs), stride), 0xDEADBEEF, np.uint32)
    n_words = np.array([len(r.words) for r in refs], np.uint32)
    models = np.full((len(refs), 10, 4), 77, np.uint32)  # (the last two words are not read)
    off = np.full((len(refs), 10, 1024), 0xFFFF, np.uint16)
    for p, r in enumerate(refs):
        words[p, :len(r.words)] = r.words
        for b in range(10):
            models[p, b, :2] = r.max_freq_bits[b], len(r.off[b])
            off[p, b, :len(r.off[b])] = r.off[b]
    return words, n_words, models, off


@pytest.mark.parametrize("case", [(250, 250, 1, 125, 125), (334, 350, 3, 167, 117)])
def test_container_from_coded_planes_is_the_container_from_streams(case):
    from tests.test_tiled_host import _inputs

    w, h, c, tw, th = case
    streams, hist, vp, wp, coefs = _inputs(case)
    words, n_words, models, off = _coded_planes(streams, hist)
    for kwargs in (dict(), dict(quality=50), dict(rct=True)) if c == 3 else (dict(), dict(quality=37)):
        want = emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp, **kwargs)
        for threads in (1, 3):
            assert emit.tiled_encode_from_coded(w, h, tw, th, words, n_words, models, off, vp, wp, threads=threads, **kwargs) == want
    frit = emit.tiled_encode_from_coded(w, h, tw, th, words, n_words, models, off, vp, wp)
    ti, got = emit.tiled_decode(frit)
    assert tuple(ti)[:7] == (w, h, tw, th, -(-w // tw), -(-h // th), c) and np.array_equal(got, coefs)
    # one ordinary image from its planes: a tile's own file
    t = streams.shape[0] - 1
    sl = slice(t * c, (t + 1) * c)
    assert emit.coded_encode_image(tw, th, words[sl], n_words[sl], models[sl], off[sl], vp[t], wp[t]) == emit.encode_image_from_streams(tw, th, streams[t], hist[t], vp[t], wp[t], empty_ok=True)


def test_coded_assembly_refuses_what_cannot_be_a_plane():
    from tests.test_tiled_host import _inputs

    w, h, c, tw, th = case = (250, 250, 1, 125, 125)
    streams, hist, vp, wp, coefs = _inputs(case)
    words, n_words, models, off = _coded_planes(streams, hist)
    L = emit.load_library()
    n, err, out = C.c_size_t(0), C.create_string_buffer(256), np.zeros(1 << 20, np.uint8)

    def call(channels=1, nw=n_words, m=models, cap=out.size, tile_w=tw):
        nw, m = np.ascontiguousarray(nw, np.uint32), np.ascontiguousarray(m, np.uint32)
        return L.fri_tiled_encode_from_coded(w, h, tile_w, th, channels, P(words), words.shape[1], P(nw), P(m), P(off), P(vp), P(wp), 1, P(out), cap, C.addressof(n), err, 256)

    assert call() == 0 and bytes(out[:n.value]) == emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp)
    assert call(cap=100) == -3 and n.value == len(emit.tiled_encode_from_streams(w, h, tw, th, streams, hist, vp, wp))
    assert call(channels=2) == -1 and call(channels=3 | emit.ALPHA) == -1 and call(tile_w=0) == -1 and call(channels=1 | emit.EMPTY_OK) == 0
    short, long_ = n_words.copy(), n_words.copy()
    short[2], long_[1] = 19, words.shape[1] + 1
    assert call(nw=short) == -2 and b"tile 2" in err.value
    assert call(nw=long_) == -2 and b"tile 1" in err.value
    many = models.copy()
    many[3, 4, 1] = 1025
    assert call(m=many) == -2 and b"tile 3" in err.value


# ---- the shared step header ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitized"])
def test_step_header_reciprocal_form_equals_division_form(tmp_path, flags):
    """A stand-alone program with its own main: nothing loaded into python is run under a sanitizer."""
    exe = tmp_path / "rans_step_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", os.path.join(ROOT, "frave_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "rans_step_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 100000
    steps = [tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("step ")]
    assert len(steps) > 200
    for start, freq, scale, x0, x1, emitted, word in steps:  # the Python restatement computes what the header computes, odd models included
        x, w = rans_ref.put_symbol(x0, rans_ref.make_symbol(start, freq, scale))
        assert (x, w is not None, w or 0) == (x1, bool(emitted), word), (start, freq, scale, x0)
        if freq <= 1 << 31 and scale < 32 and start + freq <= 1 << scale and (1 << 31) <= x0 < (1 << 63):
            assert rans_ref.put_division(x0, start, freq, scale) == (x, w)
