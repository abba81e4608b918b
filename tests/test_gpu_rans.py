"""The rANS coder on the device (K11, k11_rans.hip; include/fri_hip.h "the rANS coder on the device"):

- synthetic planes straight into fri_hip_rans_encode_planes_dev against tests/rans_ref.py (which tests/test_rans_host.py holds to the host emitter): words, counts,
  max_freq_bits and off-distribution lists exact, every output between guard bytes, nothing written behind a plane's words or a context's list; lengths around
  the wave, the scan chunk, the LDS queue, the stitch's step and the host's switch to its context-parallel coder; batches of 1, 3 and 41 planes; the odd models;
- planes the reference refuses come back with their status and no fault; a stride one word short reports the count and writes nothing past the stride;
- whole files: fri_hip_encode_image_tiled_coded + fri_tiled_encode_from_coded is byte for byte fri_hip_encode_image_tiled_symbols + fri_tiled_encode_from_streams;
- the same bytes in every run, and from a captured graph;
- fri_driver encode-file --tile-size --device-rans writes the file the plain route writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frave_amd.api as api
from frave_amd.api import RANS_BAD_BUCKET, RANS_BAD_MODEL, RANS_EMPTY_OK, RANS_TOO_SMALL, RANS_ZERO_FREQ, TILED_ALLOW_HOLES, PlanTiled  # noqa: F401  (without the feature the module fails here)
from tests import rans_cases, rans_ref
from tests.common import gen_image
from tests.test_gpu_instances import Guarded
from tests.tiled_ref import mixed_image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAXED = 2  # hipStreamCaptureModeRelaxed
COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR = 0, 1, 3


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


class Run:
    """one fri_hip_rans_encode_planes_dev call on host arrays: every output in a Guarded buffer of its own"""

    def __init__(self, ctx, streams, hist, flags=RANS_EMPTY_OK, word_stride=None, symbol_stride=None):
        import torch

        self.torch, self.ctx = torch, ctx
        streams = np.ascontiguousarray(streams, np.uint16)
        self.planes, self.n = streams.shape
        self.stride = self.n + 20 if word_stride is None else word_stride
        self.symbol_stride = self.n if symbol_stride is None else symbol_stride
        padded = np.full((self.planes, self.symbol_stride), 0xFFFF, np.uint16)  # (what lies between the streams is never read as a symbol)
        padded[:, : self.n] = streams
        self.d_sym = torch.from_numpy(padded.view(np.int16).reshape(-1).copy()).cuda()
        self.d_hist = torch.from_numpy(np.ascontiguousarray(hist, np.uint32).view(np.int32).reshape(-1).copy()).cuda()
        p = self.planes
        self.sizes = dict(words=p * self.stride * 4, n_words=p * 4, models=p * 160, off=p * 10 * 1024 * 2, status=p * 16)
        self.out = {k: Guarded(torch, v, salt=i + 1) for i, (k, v) in enumerate(self.sizes.items())}
        scratch = api.rans_scratch_bytes(p, self.n)
        assert scratch >= p * (10 * 1024 * 32 + 5 * self.n)
        self.d_scratch = torch.empty(scratch + 256, dtype=torch.uint8, device="cuda")
        self.scratch_ptr = (self.d_scratch.data_ptr() + 255) & ~255
        self.flags = flags

    def launch(self, stream=0):
        o = self.out
        api.rans_encode_planes_dev(self.ctx, self.planes, self.d_sym.data_ptr(), self.symbol_stride, self.n, self.d_hist.data_ptr(), self.flags, o["words"].ptr, self.stride,
                                   o["n_words"].ptr, o["models"].ptr, o["off"].ptr, o["status"].ptr, self.scratch_ptr, stream)

    def read(self):
        """the outputs as arrays, and `fill`: what the words and list buffers held before the call"""
        got, fill = {}, {}
        for k, g in self.out.items():
            (region,), intact = g.get(self.torch)
            assert intact, "K11 wrote outside its %s buffer" % k
            got[k], fill[k] = region, g.fill[g.start : g.start + g.size]
        p = self.planes
        self.words, self.words_fill = got["words"].view(np.uint32).reshape(p, self.stride), fill["words"].view(np.uint32).reshape(p, self.stride)
        self.n_words = got["n_words"].view(np.uint32)
        self.models = got["models"].view(np.uint32).reshape(p, 10, 4)
        self.off, self.off_fill = got["off"].view(np.uint16).reshape(p, 10, 1024), fill["off"].view(np.uint16).reshape(p, 10, 1024)
        self.status = got["status"].view(np.uint32).reshape(p, 4)
        return self

    def raw(self):
        self.torch.cuda.synchronize()
        return [g.raw.cpu().numpy().copy() for g in self.out.values()]

    def differences(self, first, again):
        """"" when two raw() snapshots are the same bytes, else which outputs differ and where"""
        out = []
        for (name, g), a, b in zip(self.out.items(), first, again):
            bad = np.flatnonzero(a != b)
            if bad.size:
                at = bad[:6] - g.start
                out.append("%s: %d bytes from offset %d (first %s: %s -> %s)" % (name, bad.size, at[0], at.tolist(), a[bad[:6]].tolist(), b[bad[:6]].tolist()))
        return "; ".join(out)

    def clear(self):
        for g in self.out.values():
            g.raw.copy_(self.torch.from_numpy(g.fill))

    def check_plane(self, k, ref, where):
        """plane k against the reference: everything exact, nothing written behind the words or the lists"""
        assert ref.status == 0
        assert self.status[k].tolist() == [0, 0, 0, 0], (where, k, self.status[k])
        n = len(ref.words)
        assert int(self.n_words[k]) == n, (where, k)
        bad = np.flatnonzero(self.words[k, :n] != ref.words)
        assert bad.size == 0, (where, k, bad[:8].tolist())
        assert np.array_equal(self.words[k, n:], self.words_fill[k, n:]), (where, k, "words behind the stream")
        for b in range(10):
            n_off = len(ref.off[b])
            assert (int(self.models[k, b, 0]), int(self.models[k, b, 1])) == (ref.max_freq_bits[b], n_off), (where, k, b)
            assert self.off[k, b, :n_off].tolist() == ref.off[b] and np.array_equal(self.off[k, b, n_off:], self.off_fill[k, b, n_off:]), (where, k, b)


NAMES = ["n:%d" % n for n in rans_cases.LENGTHS] + ["batch:%d" % n for n in rans_cases.BATCHES] + rans_cases.SPECIAL


@pytest.mark.parametrize("name", NAMES)
def test_synthetic_planes_equal_the_reference(ctx, name):
    streams, hist = rans_cases.case(name)
    refs = rans_cases.reference(name)
    r = Run(ctx, streams, hist)
    r.launch()
    r.read()
    for k, ref in enumerate(refs):
        if ref.status:  # the same outcome as the host: a refusal, and no claim of success
            assert r.status[k, 0] == ref.status and (int(r.status[k, 1]), int(r.status[k, 2])) == (ref.zero_at, ref.bucket_at), (name, k)
        else:
            r.check_plane(k, ref, name)
    if name == "collapse":
        want = [rans_ref.collapsed_slots(hist[k][b], b) for k, b in ((0, 0), (1, 1))]
        assert min(want) > 5 and [int(r.models[0, 0, 2]), int(r.models[1, 1, 2])] == want
    if name == "nine_empty":  # an untouched state flushes 2^31; a context without symbols reports K6's status word 1 and is coded all the same
        assert r.models[0, :, 3].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]


def test_streams_further_apart_than_their_length(ctx):
    streams, hist = rans_cases.case("batch:3")
    r = Run(ctx, streams, hist, symbol_stride=streams.shape[1] + 37)
    r.launch()
    r.read()
    for k, ref in enumerate(rans_cases.reference("batch:3")):
        r.check_plane(k, ref, "symbol_stride")


def test_refused_planes_report_their_status_and_good_planes_are_coded(ctx):
    base, hist0 = (a[0] for a in rans_cases.case("n:257"))
    bucket, zero = base.copy(), base.copy()
    bucket[100], bucket[31] = 12 << 10 | 5, 15 << 10 | 1  # entries of no chain
    zero[200] = (zero[200] & ~np.uint16(1023)) | 1021       # a symbol the histogram does not count
    zero[17] = zero[200]
    streams, hist = np.stack([base, bucket, zero, base]), np.stack([hist0] * 4)
    refs = [rans_ref.encode_plane(s, h) for s, h in zip(streams, hist)]
    assert [x.status for x in refs] == [0, RANS_BAD_BUCKET, RANS_ZERO_FREQ, 0]
    r = Run(ctx, streams, hist)
    r.launch()
    r.read()
    r.check_plane(0, refs[0], "good plane 0")
    r.check_plane(3, refs[3], "good plane 3")
    assert r.status[1].tolist() == [RANS_BAD_BUCKET, 0, 101, 0] and r.status[2].tolist() == [RANS_ZERO_FREQ, 201, 0, 0]
    # without the empty-context rule a context without counts is the emitter's division by zero
    streams, hist = rans_cases.case("nine_empty")
    assert rans_ref.encode_plane(streams[0], hist[0], empty_ok=False).status == RANS_BAD_MODEL
    r = Run(ctx, streams, hist, flags=0)
    r.launch()
    r.read()
    assert r.status[0].tolist() == [RANS_BAD_MODEL, 0, 0, 0] and r.models[0, :, 3].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]
    # argument checks: nothing is enqueued
    import frave_amd as fa

    o = r.out
    for kwargs in (dict(flags=2), dict(n_planes=0), dict(n_planes=65536), dict(n_symbols=0), dict(symbol_stride=r.n - 1), dict(scratch=r.scratch_ptr + 8)):
        a = dict(n_planes=r.planes, symbol_stride=r.n, n_symbols=r.n, flags=RANS_EMPTY_OK, scratch=r.scratch_ptr)
        a.update(kwargs)
        with pytest.raises(fa.FriHipError) as e:
            api.rans_encode_planes_dev(ctx, a["n_planes"], r.d_sym.data_ptr(), a["symbol_stride"], a["n_symbols"], r.d_hist.data_ptr(), a["flags"], o["words"].ptr, r.stride,
                                       o["n_words"].ptr, o["models"].ptr, o["off"].ptr, o["status"].ptr, a["scratch"], 0)
        assert e.value.code == -1, kwargs
    assert api.rans_scratch_bytes(0, 10) == 0 and api.rans_scratch_bytes(1, 0) == 0 and api.rans_scratch_bytes(1, 1 << 31) == 0


@pytest.mark.parametrize("name,short", [("batch:3", 1), ("n:4097", 1), ("n:64", 19)])
def test_a_stride_too_small_reports_the_count_and_writes_nothing_past_it(ctx, name, short):
    streams, hist = rans_cases.case(name)
    refs = rans_cases.reference(name)
    stride = max(len(x.words) for x in refs) - short  # `short` words short of the longest plane's need (19: not even the flush fits)
    r = Run(ctx, streams, hist, word_stride=stride)
    r.launch()
    r.read()  # (asserts the guard bytes around every output)
    assert any(len(x.words) > stride for x in refs)
    for k, ref in enumerate(refs):
        if len(ref.words) <= stride:
            r.check_plane(k, ref, name)
            continue
        assert r.status[k].tolist() == [RANS_TOO_SMALL, 0, 0, 0] and int(r.n_words[k]) == len(ref.words)
        assert np.array_equal(r.words[k], ref.words[:stride])  # what fits is the stream's beginning
        for b in range(10):
            assert (int(r.models[k, b, 0]), int(r.models[k, b, 1])) == (ref.max_freq_bits[b], len(ref.off[b]))


# ---- whole files ------------------------------------------------------------------------------------------------------------------------------------------------

def _both_routes(ctx, img, case, transform=COLOUR_NONE, quality=0, flags=0, **kwargs):
    import frave_amd as fa
    import frave_amd.emit as emit

    w, h, c, tw, th = case
    T = PlanTiled(ctx, w, h, c, tw, th, flags)
    T.set_stream_order()
    T.tile.set_colour_transform(transform)
    qm = fa.quality_matrix(quality) if quality else None
    sym, vp, wp, hist, oob = T.encode_image_tiled_symbols(img, qm)
    assert not oob.any()
    want = emit.tiled_encode_from_streams(w, h, tw, th, sym, hist, vp, wp, quality=quality, **kwargs)
    words, n_words, models, off, status, cvp, cwp = T.encode_image_tiled_coded(img, qm)
    assert not status.any() and np.array_equal(cvp, vp) and np.array_equal(cwp, wp)
    got = emit.tiled_encode_from_coded(w, h, tw, th, words, n_words, models, off, cvp, cwp, quality=quality, **kwargs)
    return T, got, want, n_words


@pytest.mark.parametrize("case,mode", [((250, 250, 1, 125, 125), "lossless"), ((250, 250, 1, 125, 125), "q50"), ((334, 350, 3, 167, 117), "lossless"),
                                       ((334, 350, 3, 167, 117), "rct"), ((334, 350, 3, 167, 117), "ycbcr50"), ((5, 3, 3, 2, 2), "lossless")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_whole_files_are_byte_identical_to_the_host_coders(ctx, case, mode):
    w, h, c, tw, th = case
    img = mixed_image(w, h, c, tw, 3) if w > 8 else gen_image("noise", w, h, c, 4)
    transform, quality, kwargs = {"lossless": (COLOUR_NONE, 0, {}), "q50": (COLOUR_NONE, 50, {}), "rct": (COLOUR_RCT, 0, dict(rct=True)),
                                  "ycbcr50": (COLOUR_YCBCR, 50, dict(ycbcr=True))}[mode]
    T, got, want, n_words = _both_routes(ctx, img, case, transform, quality, TILED_ALLOW_HOLES if w <= 8 else 0, **kwargs)
    assert got == want
    if w <= 8:  # tiles of a handful of symbols: mostly empty contexts
        assert T.num_some < 64 and (n_words <= T.num_some + 20).all()
    T.close()


def test_a_plane_that_needs_more_than_the_first_pass_holds_and_a_callers_stride_too_small(ctx):
    """noise codes to more than 8 bits per symbol: the library's second pass with the hard bound gives the same file; a caller's stride below a plane's need is
    out of range, with the need reported"""
    import frave_amd as fa

    case = (250, 250, 1, 125, 125)
    img = gen_image("noise", 250, 250, 1, 9)
    T, got, want, n_words = _both_routes(ctx, img, case)
    assert got == want and (n_words > T.num_some // 4 + 20).any()
    with pytest.raises(fa.FriHipError) as e:
        T.encode_image_tiled_coded(img, word_stride=int(n_words.max()) - 1)
    assert e.value.code == -7
    T.close()


# ---- the same bytes in every run, and from a graph -----------------------------------------------------------------------------------------------------------------

def test_reproducible_and_capturable(ctx):
    import torch

    hip = C.CDLL("libamdhip64.so")
    streams, hist = rans_cases.case("batch:41")
    r = Run(ctx, streams, hist)
    r.launch()
    first = r.raw()
    r.read()
    r.check_plane(40, rans_cases.reference("batch:41")[40], "batch:41")
    r.clear()
    r.launch()
    assert r.differences(first, r.raw()) == "", "a second run wrote other bytes"
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    r.launch(stream=s.cuda_stream)  # a linear chain on one stream: three kernel nodes
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    n_nodes = C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 3
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    for _ in range(2):
        r.clear()
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert r.differences(first, r.raw()) == "", "a replay wrote other bytes"
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_driver_device_rans_writes_the_plain_routes_file(ctx, tmp_path):
    driver = os.path.join(ROOT, "frave_amd", "host", "fri_driver")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "frave_amd", "host")])
    w, h = 300, 260
    img = mixed_image(w, h, 3, 128, 6)
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + img.tobytes())
    for name, flags in (("rct", ["--rct"]), ("ycc", ["--ycbcr", "--quality", "60"])):
        plain, coded, back = tmp_path / f"{name}_host.frv", tmp_path / f"{name}_device.frv", tmp_path / f"{name}.ppm"
        for dst, extra in ((plain, []), (coded, ["--device-rans"])):
            out = subprocess.run([driver, "encode-file", str(src), str(dst), "--tile-size", "128"] + flags + extra, capture_output=True, text=True, timeout=300)
            assert out.returncode == 0 and "self-check" in out.stdout, out.stdout + out.stderr
        assert coded.read_bytes() == plain.read_bytes()
        out = subprocess.run([driver, "decode-file", str(coded), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        got = np.frombuffer(back.read_bytes()[-3 * w * h:], np.uint8)
        if name == "rct":
            assert np.array_equal(got, img.reshape(-1))
        else:
            assert np.abs(got.astype(np.int64) - img.reshape(-1)).max() < 128
    out = subprocess.run([driver, "encode-file", str(src), str(tmp_path / "bad.frv"), "--device-rans"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and not (tmp_path / "bad.frv").exists()
