"""Random-shape sweep of the kernels and plan kinds that came after tests/tools/fuzz_parity.py: YCbCr in K1 / K3, K6 (size estimate), K7 (SSIM), K8 (4:2:0),
K9 (RGBA), K10 (tiles, region merge, measure), K11 (device rANS), K12 (tiled 4:2:0), K13 (the device decoder, on the crafted planes of tests/decode_cases.py,
bounded by a drawn level), and the composed encode entry points. Every comparison is bit-exact against
a restatement that involves no GPU code (tests/*_ref.py, tests/rate_model.py, the CPU oracle); K6's bytes keep the +-1 byte of tests/test_gpu_rate.py. Every
device buffer is a tests.test_gpu_instances.Guarded one, outputs start as a fill pattern, guards are checked after every call. The byte rasters, for which the
headers promise any alignment, sit at a drawn byte offset of 0..15; the typed arrays (coefficients, histograms, streams, words, models) keep the 16-byte alignment
of every allocation, which is all the headers' typed pointers allow a caller to rely on, and the 64-bit sums are 8-byte aligned.

Each kind draws from np.random.default_rng([seed, k]) with a k of its own, so a new kind moves no other kind's cases. run(kind, n_cases, seed, dry=True) makes
the draws, the references and the coverage record (tests/later_cases.py names the cells) without a device call; tests/test_later_cases_host.py runs that.
usage: fuzz_later.py kind [n_cases] [seed]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import frave_amd
from frave_amd.api import TILED_ALLOW_HOLES, FriHipError
from tests import decode_cases as DC
from tests import later_cases as LC
from tests import preview_ref, rans_cases, rans_ref, rate_model, ssim_ref
from tests.alpha_ref import alpha_plane, merge_rgba, rgba_image, split_rgba
from tests.chroma420_ref import chroma_shape, measure420, merge420, planes_flat, split420
from tests.common import gen_image
from tests.oracle_ref import numpy_measure, oracle_owned
from tests.test_gpu_instances import Guarded
from tests.test_rct_host import correlated_image
from tests.tiled420_ref import merge_tiles420, plane_index, split_tiles420
from tests.tiled420_ref import sub_grid as sub_grid420
from tests.tiled_ref import grid, merge_tiles, mixed_image, split_tiles
from tests.tiled_region_ref import merge_region, region_tiles, sub_grid
from tests.ycbcr_ref import COLOUR_YCBCR, oracle_coefficients_ycc, oracle_raster_ycc

UNCODABLE = rate_model.UNCODABLE
REGION_AREA = 6000  # pixels of a K10 region at most: tests.tiled_region_ref.merge_region walks them one by one
MAX_TILES, MAX_TILES_420, MAX_TILES_COMPOSED = 4096, 1024, 16


# ---- draws and buffers ---------------------------------------------------------------------------------------------------------------------------------------

def _int(rng, lo, hi):
    """an int in lo..hi, both included"""
    return int(rng.integers(lo, hi + 1))


def _shape(rng, lo=1):
    """about 30 % thin or tiny (lo..40 by lo..900, either way round), otherwise up to 400 x 300"""
    if rng.random() < 0.3:
        w, h = _int(rng, lo, 40), _int(rng, lo, 900)
        if rng.random() < 0.5:
            w, h = h, w
    else:
        w, h = _int(rng, lo, 400), _int(rng, lo, 300)
    return w, h


def _offsets(rng, n):
    return [_int(rng, 0, 15) for _ in range(n)]


class _Dev:
    """the Guarded buffers of one case and what went wrong with them"""

    def __init__(self):
        import torch

        self.torch, self.salt, self.msgs = torch, 0, []

    def put(self, data, offset, unit=1, n=1, stride=0):
        """an input: `data` (n arrays, `stride` bytes apart) between guards, `offset` bytes (rounded down to the element size `unit`) off a 256-byte boundary"""
        arrays = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in (data if n > 1 else [data])]
        self.salt += 1
        g = Guarded(self.torch, arrays[0].size, n, stride, offset // unit * unit, self.salt)
        g.put(self.torch, arrays)
        g.data = arrays
        return g

    def out(self, size, offset, unit=1, n=1, stride=0):
        self.salt += 1
        return Guarded(self.torch, size, n, stride, offset // unit * unit, self.salt)

    def get(self, g, name):
        regions, intact = g.get(self.torch)
        if not intact:
            self.msgs.append(name + ": bytes outside the buffer were written")
        return regions if g.n > 1 else regions[0]

    def same(self, name, got, want):
        got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad = np.flatnonzero(got != want) if got.shape == want.shape else []
            self.msgs.append("%s (%d differ, first at %s)" % (name, len(bad), list(bad[:4])))

    def untouched(self, g, name):
        """an input holds what it held"""
        regions, intact = g.get(self.torch)
        if not intact or any(not np.array_equal(a, b) for a, b in zip(regions, g.data)):
            self.msgs.append(name + ": the input was written")

    def sums(self, n, unit_offset):
        """a uint64 [n] output, pre-filled"""
        return self.out(8 * n, unit_offset, 8)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _plain(ctx, plane, w, h, c, qm):
    """fri_hip_encode_image_symbols with the fit on an ordinary plan of the plane's shape"""
    Q = frave_amd.Plan(ctx, w, h, c)
    Q.set_stream_order()
    out = Q.encode_image_symbols(plane, qm, fit=True)
    Q.close()
    return out


def _qm(quality):
    return frave_amd.quality_matrix(quality) if quality else np.ones(32, np.int32)


# ---- ycbcr: K1, K3 and MEASURE on a YCbCr plan ----------------------------------------------------------------------------------------------------------------

def _ycbcr_draw(rng, case):
    w, h = _shape(rng)
    return dict(w=w, h=h, dequantiser=_int(rng, 0, 2), quality=_int(rng, 1, 99), seed=_int(rng, 0, 1 << 30), band=round(float(rng.uniform(0.1, 0.6)), 3), off=_offsets(rng, 5))


def _ycbcr_image(p):
    w, h = p["w"], p["h"]
    img = correlated_image(w, h, p["seed"])
    rows = max(1, int(h * p["band"]))
    img[:rows] = gen_image("noise", w, rows, 3, p["seed"])  # saturated colours: the clamps of the inverse
    return np.ascontiguousarray(img)


def _ycbcr_ref(p):
    from oracle import fri_oracle as O

    w, h = p["w"], p["h"]
    img, qm = _ycbcr_image(p), _qm(p["quality"])
    want = oracle_coefficients_ycc(O, img, w, h, qm)
    owned = oracle_owned(O, w, h, 3)
    recon = oracle_raster_ycc(O, want, qm, p["dequantiser"], w, h, owned)
    return dict(img=img.reshape(-1), coefs=want, recon=recon, sums=numpy_measure(recon, img.reshape(-1), owned, 3))


def _ycbcr_dev(ctx, p, r):
    D, qm, off = _Dev(), _qm(p["quality"]), p["off"]
    P = frave_amd.Plan(ctx, p["w"], p["h"], 3)
    P.set_colour_transform(COLOUR_YCBCR)
    P.set_dequantiser(p["dequantiser"])
    px = D.put(r["img"], off[0])
    co = D.out(4 * P.coef_count, off[1], 16)
    P.transform_quant_dev(px.ptr, co.ptr, qm)
    D.same("K1", D.get(co, "K1 coefficients").view(np.int32), r["coefs"])
    ci = D.put(r["coefs"], off[2], 16)
    back = D.out(P.pixel_bytes, off[3])
    P.inverse_transform_dev(ci.ptr, back.ptr, qm)
    D.same("K3", D.get(back, "K3 raster"), r["recon"])
    out = D.sums(7, off[4])
    P.measure_distortion_dev(ci.ptr, px.ptr, out.ptr, qm)
    got = [int(v) for v in D.get(out, "MEASURE sums").view(np.uint64)]
    if got != r["sums"]:
        D.msgs.append("MEASURE %s != %s" % (got, r["sums"]))
    D.untouched(px, "pixels"), D.untouched(ci, "coefficients")
    P.close()
    return D.msgs


# ---- ssim: K7 ------------------------------------------------------------------------------------------------------------------------------------------------

PAIRS = ["identical", "noise / smooth", "source / source + small noise"]


def _ssim_draw(rng, case):
    w, h = _shape(rng, 8)
    n = _int(rng, 1, 4)
    return dict(w=w, h=h, c=1 if rng.random() < 0.5 else 3, n_images=n, gap=_int(rng, 0, 40), pairs=[_int(rng, 0, 2) for _ in range(n)], amplitude=_int(rng, 1, 12),
                seed=_int(rng, 0, 1 << 30), off=_offsets(rng, 3))


def _ssim_pairs(p):
    w, h, c = p["w"], p["h"], p["c"]
    rng = np.random.default_rng(p["seed"])
    out = []
    for k, kind in enumerate(p["pairs"]):
        s = p["seed"] % 100000 + k
        if kind == 0:
            a = gen_image("noise", w, h, c, s).reshape(-1)
            b = a.copy()
        elif kind == 1:
            a, b = gen_image("noise", w, h, c, s).reshape(-1), gen_image("smooth", w, h, c, s + 1).reshape(-1)
        else:
            src = correlated_image(w, h, s)
            a = np.ascontiguousarray(src if c == 3 else src[:, :, 1:2]).reshape(-1)
            b = np.clip(a.astype(np.int32) + rng.integers(-p["amplitude"], p["amplitude"] + 1, a.size), 0, 255).astype(np.uint8)
        out.append((a, b))
    return out


def _ssim_ref(p):
    pairs = _ssim_pairs(p)
    return dict(pairs=pairs, want=np.stack([ssim_ref.measure(a, b, p["w"], p["h"], p["c"]) for a, b in pairs]))


def _ssim_cells(p):
    bx = p["w"] // 4
    out = {"C%d: %s" % (p["c"], v) for v in LC.k7_cells(p["w"], p["h"], p["n_images"])}
    out.add("C%d: last lane sees %d block%s" % (p["c"], 2 - bx % 2, "s" if bx % 2 == 0 else ""))
    out.add("C%d: row bytes mod 4 = %d" % (p["c"], p["w"] * p["c"] % 4))
    out.add("C%d: %d image%s" % (p["c"], min(p["n_images"], 2), "s" if p["n_images"] > 1 else ""))
    return out


SSIM_CELLS = {"C%d: %s" % (c, v) for c in (1, 3) for v in ["band=4", "last lane sees 1 block", "last lane sees 2 blocks", "1 image", "2 images", "a wave's band starts past ny"]
              + ["row bytes mod 4 = %d" % k for k in range(4)]}


def _ssim_dev(ctx, p, r):
    D, off, c, n = _Dev(), p["off"], p["c"], p["n_images"]
    P = frave_amd.Plan(ctx, p["w"], p["h"], c)
    stride = P.pixel_bytes + p["gap"]
    a = D.put([x for x, _ in r["pairs"]], off[0], n=n, stride=stride) if n > 1 else D.put(r["pairs"][0][0], off[0])
    b = D.put([y for _, y in r["pairs"]], off[1], n=n, stride=stride) if n > 1 else D.put(r["pairs"][0][1], off[1])
    out = D.sums(n * (c + 1), off[2])
    P.measure_ssim_dev(a.ptr, b.ptr, out.ptr, n_images=n, pixel_stride=stride)
    D.same("K7", D.get(out, "K7 sums").view(np.int64), r["want"])
    D.untouched(a, "raster a"), D.untouched(b, "raster b")
    P.close()
    return D.msgs


# ---- rate: K6 ------------------------------------------------------------------------------------------------------------------------------------------------

def _rate_draw(rng, case):
    c = 1 if rng.random() < 0.5 else 3
    if rng.random() < 1 / 3:  # synthetic histograms
        return dict(crafted=True, c=c, n_images=_int(rng, 1, 4), empty=round(float(rng.uniform(0.0, 0.02)), 4), oob=rng.random() < 0.3, seed=_int(rng, 0, 1 << 30), off=_offsets(rng, 4))
    w, h = _shape(rng, 8)
    return dict(crafted=False, c=c, w=w, h=h, quality=_int(rng, 1, 100), kind=["noise", "smooth", "mixed"][_int(rng, 0, 2)], seed=_int(rng, 0, 1 << 20), off=_offsets(rng, 4))


def _crafted(p):
    """[n][C][10][1024] in the manner of tests/test_gpu_rate.py's _crafted(), every context's shape and parameters drawn; (hist, oob or None)"""
    rng = np.random.default_rng(p["seed"])
    n, c = p["n_images"], p["c"]
    hist = np.zeros((n, c, 10, 1024), np.uint32)
    for h in hist.reshape(-1, 1024):
        v = _int(rng, 0, 5)
        if rng.random() < p["empty"]:
            continue  # a context without symbols: the image is uncodable
        if v == 0:  # every symbol once, a peak of drawn height and width
            h[:] = 1
            h[: _int(rng, 1, 16)] = _int(rng, 2, 500)
        elif v == 1:  # a single symbol, anywhere, up to 2^26 of it
            h[_int(rng, 0, 1023)] = 1 << _int(rng, 0, 26)
        elif v == 2:  # a heavy head over a long tail
            h[:] = (rng.random(1024) < rng.uniform(0.1, 0.9)) * rng.integers(1, 4, 1024)
            h[: _int(rng, 1, 64)] = 1 << _int(rng, 8, 20)
        else:  # geometric counts, sparse
            h[:] = rng.geometric(rng.uniform(0.01, 0.3), 1024) * (rng.random(1024) < rng.uniform(0.05, 0.8))
            h[0] += 1
    oob = None
    if p["oob"]:
        oob = np.zeros((n, c), np.uint64)
        oob[_int(rng, 0, n - 1), _int(rng, 0, c - 1)] = _int(rng, 1, 9)
    return hist, oob


def _rate_image(p):
    w, h, c = p["w"], p["h"], p["c"]
    return mixed_image(w, h, c, max(2, w // 2), p["seed"]) if p["kind"] == "mixed" else gen_image(p["kind"], w, h, c, p["seed"])


def _rate_ref(p):
    if not p["crafted"]:
        return dict(img=_rate_image(p))  # the histograms are the device chain's own: the estimate of them is made in _rate_dev, by tests/rate_model.py on the host
    hist, oob = _crafted(p)
    return dict(hist=hist, oob=oob, want=rate_model.estimate(hist, oob))


def _rate_cells(p):
    return {"synthetic histograms" if p["crafted"] else "the chain's histograms", "C%d" % p["c"]}


def _model_mismatches(hist, models):
    """tests/test_gpu_rate.py's _check_models as a list of messages"""
    import frave_amd.emit as emit

    out = []
    hist, models = hist.reshape(-1, 10, 1024), models.reshape(-1, 10, 4)
    for k in range(hist.shape[0]):
        for b in range(10):
            try:
                f, _cdf, off, bits = emit.finalize_context(hist[k, b], b)
            except emit.EmitError:
                if models[k, b, 3] != 1:
                    out.append("model status of the empty context (%d, %d)" % (k, b))
                continue
            used = hist[k, b] > 0
            if (int(models[k, b, 0]), int(models[k, b, 1])) != (bits, len(off)) or int(models[k, b, 3]) != (2 if (f[used] == 0).any() else 0):
                out.append("model of context (%d, %d): %s" % (k, b, models[k, b].tolist()))
    return out


def _rate_dev(ctx, p, r):
    D, off, c = _Dev(), p["off"], p["c"]
    if p["crafted"]:
        hist, oob, want = r["hist"], r["oob"], r["want"]
        P = frave_amd.Plan(ctx, 64, 48, c)
    else:
        P = frave_amd.Plan(ctx, p["w"], p["h"], c)
        P.set_stream_order()
        _, _, _, hist, oob = P.encode_image_symbols(r["img"], _qm(p["quality"] if p["quality"] < 100 else 0))
        hist, oob = hist[None], oob[None]
        want = rate_model.estimate(hist, oob)
    n = hist.shape[0]
    d_hist = D.put(hist, off[0], 16)
    d_oob = None if oob is None else D.put(np.ascontiguousarray(oob, np.uint64), off[1], 8)
    d_bytes, d_models = D.sums(n, off[2]), D.out(n * c * 160, off[3], 16)
    P.estimate_size(d_hist.ptr, None if d_oob is None else d_oob.ptr, n_images=n, d_bytes=d_bytes.ptr, d_models=d_models.ptr)
    got = D.get(d_bytes, "K6 bytes").view(np.uint64)
    models = D.get(d_models, "K6 models").view(np.uint32).reshape(n, c, 10, 4)
    D.msgs += _model_mismatches(hist, models)
    for k in range(n):
        g, w = int(got[k]), int(want[k])
        if (g == UNCODABLE) != (w == UNCODABLE) or (w != UNCODABLE and abs(g - w) > 1):  # the bound of tests/test_gpu_rate.py
            D.msgs.append("K6 bytes of image %d: %d, the model %d" % (k, g, w))
    D.untouched(d_hist, "histograms")
    P.close()
    return D.msgs


# ---- c420: K8 ------------------------------------------------------------------------------------------------------------------------------------------------

def _c420_draw(rng, case):
    composed = case % 4 == 0
    w, h = _shape(rng, 8 if composed else 1)
    return dict(w=w, h=h, kind=["noise", "smooth", "correlated"][_int(rng, 0, 2)], seed=_int(rng, 0, 1 << 20), composed=composed, quality=_int(rng, 1, 99), off=_offsets(rng, 6))


def _c420_ref(p):
    w, h = p["w"], p["h"]
    img = np.ascontiguousarray(correlated_image(w, h, p["seed"]) if p["kind"] == "correlated" else gen_image(p["kind"], w, h, 3, p["seed"]))
    y, cb, cr = split420(img, w, h)
    cw, ch = chroma_shape(w, h)
    rng = np.random.default_rng(p["seed"])  # independent bytes in all three planes: the saturating corners of the inverse transform
    fy, fb, fr = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    recon = merge420(fy, fb, fr, w, h)
    return dict(img=img.reshape(-1), planes=planes_flat(y, cb, cr), split=(y, cb, cr), fed=planes_flat(fy, fb, fr), recon=recon, sums=measure420(recon, img.reshape(-1)))


def _c420_cells(p):
    return LC.k8_cells(p["w"], p["h"]) | ({"composed encode"} if p["composed"] else set())


def _c420_dev(ctx, p, r):
    D, off, w, h = _Dev(), p["off"], p["w"], p["h"]
    P = frave_amd.Plan420(ctx, w, h)
    n_y = w * h
    src = D.put(r["img"], off[0])
    out = D.out(P.plane_bytes, off[1])
    P.split420_dev(src.ptr, out.ptr, out.ptr + n_y)
    D.same("split", D.get(out, "split planes"), r["planes"])
    fed = D.put(r["fed"], off[2])
    rgb = D.out(P.pixel_bytes, off[3])
    P.merge420_dev(fed.ptr, fed.ptr + n_y, rgb.ptr)
    D.same("merge", D.get(rgb, "merge raster"), r["recon"])
    sums = D.sums(7, off[4])
    P.measure_distortion420_dev(fed.ptr, fed.ptr + n_y, src.ptr, sums.ptr)
    got = [int(v) for v in D.get(sums, "measure sums").view(np.uint64)]
    if got != r["sums"]:
        D.msgs.append("measure %s != %s" % (got, r["sums"]))
    D.untouched(src, "pixels"), D.untouched(fed, "planes")
    if p["composed"]:
        P.set_stream_order()
        sym, vp, wp, hist, oob = P.encode_image420_symbols(r["img"], p["quality"])
        at = 0
        for k, plane in enumerate(r["split"]):  # the restatement's planes, in the order the header defines: Y, Cb, Cr
            ph, pw = plane.shape
            rsym, rvp, rwp, rhist, roob = _plain(ctx, plane, pw, ph, 1, _qm(p["quality"]))
            ok = _same_bits(sym[at: at + rsym.size], rsym.reshape(-1)) and _same_bits(hist[k], rhist[0]) and _same_bits(vp[k], rvp[0]) and _same_bits(wp[k], rwp[0])
            if not (ok and int(oob[k]) == int(roob[0])):
                D.msgs.append("encode_image420_symbols, plane %d" % k)
            at += rsym.size
        if at != sym.size:
            D.msgs.append("encode_image420_symbols: %d symbols, the planes have %d" % (sym.size, at))
    P.close()
    return D.msgs


# ---- rgba: K9 ------------------------------------------------------------------------------------------------------------------------------------------------

ALPHAS = ["zeros", "opaque", "random", "runs"]


def _rgba_draw(rng, case):
    composed = case % 4 == 0
    w, h = _shape(rng, 8 if composed else 1)
    if not composed and rng.random() < 0.15:  # fewer pixels than one lane takes
        w, h = _int(rng, 1, 5), _int(rng, 1, 3)
    return dict(w=w, h=h, alpha=ALPHAS[_int(rng, 0, 3)], clean=_int(rng, 0, 1), seed=_int(rng, 0, 1 << 20), composed=composed, quality=[0, _int(rng, 1, 99)][_int(rng, 0, 1)],
                off=_offsets(rng, 4))


def _rgba_ref(p):
    w, h = p["w"], p["h"]
    colour = gen_image("noise", w, h, 3, p["seed"]) if not p["composed"] else correlated_image(w, h, p["seed"])
    img = rgba_image(colour, alpha_plane(p["alpha"], w, h, p["seed"]))
    rgb, a = split_rgba(img, w, h, p["clean"])
    return dict(img=np.ascontiguousarray(img).reshape(-1), rgb=np.ascontiguousarray(rgb), a=np.ascontiguousarray(a), merged=merge_rgba(rgb, a, w, h))


def _rgba_cells(p):
    n = p["w"] * p["h"]
    return {"N mod 16 = %d" % (n % 16) if n % 16 in (0, 1, 15) else "N mod 16 in 2..14", "N < 16" if n < 16 else "N >= 16", "clean" if p["clean"] else "keep", p["alpha"]} | (
        {"composed encode"} if p["composed"] else set())


RGBA_CELLS = {"N mod 16 = 0", "N mod 16 in 2..14", "N < 16", "N >= 16", "clean", "keep", "composed encode"} | set(ALPHAS)


def _rgba_dev(ctx, p, r):
    D, off, w, h = _Dev(), p["off"], p["w"], p["h"]
    n = w * h
    R = frave_amd.PlanRGBA(ctx, w, h)
    src = D.put(r["img"], off[0])
    rgb, a = D.out(3 * n, off[1]), D.out(n, off[2])
    R.split_rgba_dev(src.ptr, rgb.ptr, a.ptr, clean=p["clean"])
    D.same("split colour", D.get(rgb, "split colour"), r["rgb"])
    D.same("split alpha", D.get(a, "split alpha"), r["a"])
    back = D.out(4 * n, off[3])
    R.merge_rgba_dev(rgb.ptr, a.ptr, back.ptr)
    D.same("merge", D.get(back, "merge raster"), r["merged"])
    D.untouched(src, "pixels")
    D.same("colour after the merge", D.get(rgb, "colour raster"), r["rgb"])
    D.same("alpha after the merge", D.get(a, "alpha plane"), r["a"])
    if p["composed"]:
        R.set_stream_order()
        qm = _qm(p["quality"])
        got = R.encode_image_rgba_symbols(r["img"], qm, clean=p["clean"])
        colour = _plain(ctx, r["rgb"], w, h, 3, qm)  # the header's order: the colour channels, then alpha with the all-ones matrix
        alpha = _plain(ctx, r["a"], w, h, 1, np.ones(32, np.int32))
        for name, g, cc, aa in zip(("streams", "value parameters", "width parameters", "histograms", "out-of-alphabet counts"), got, colour, alpha):
            if not (_same_bits(g[:3], cc) and _same_bits(g[3:], aa)):
                D.msgs.append("encode_image_rgba_symbols: " + name)
    R.close()
    return D.msgs


# ---- tiled: K10 ----------------------------------------------------------------------------------------------------------------------------------------------

def _cap_tiles(w, h, tw, th, most):
    while -(-w // tw) * -(-h // th) > most:
        if -(-h // th) > 1:
            th *= 2
        else:
            tw *= 2
    return tw, th


def _region(rng, w, h, tw, th, area=REGION_AREA):
    """biased as tests/test_gpu_tiled_region.py's kernel_regions: a pixel, a full row, whole tiles, any rectangle (most cross tiles), one that touches the
    image's last row and column"""
    nx, ny = grid(w, h, tw, th)
    k = _int(rng, 0, 4)
    if k == 0:
        x, y, rw, rh = _int(rng, 0, w - 1), _int(rng, 0, h - 1), 1, 1
    elif k == 1:
        x, y, rw, rh = 0, _int(rng, 0, h - 1), w, 1
    elif k == 2:
        i, j = _int(rng, 0, nx - 1), _int(rng, 0, ny - 1)
        x, y = i * tw, j * th
        rw, rh = min(_int(rng, 1, 3) * tw, w - x), min(_int(rng, 1, 3) * th, h - y)
    else:
        x, y = _int(rng, 0, w - 1), _int(rng, 0, h - 1)
        rw, rh = (w - x, h - y) if k == 4 else (_int(rng, 1, w - x), _int(rng, 1, h - y))
    if rw * rh > area:
        rh = max(1, area // rw)
    if rw * rh > area:
        rw = area
    if k == 4:
        x, y = w - rw, h - rh
    return ["one pixel", "full row", "whole tiles", "rectangle", "last row and column"][k], x, y, rw, rh


def _tiled_draw(rng, case):
    composed = case % 4 == 0
    c = 1 if rng.random() < 0.5 else 3
    if composed:  # few tiles, each large enough to be an image with symbols
        tw, th = _int(rng, 8, 72), _int(rng, 8, 72)
        w, h = _int(rng, 1, 4 * tw), _int(rng, 1, 4 * th)
        bias = "composed"
    else:
        w, h = _shape(rng)
        bias = ["tile_w c < 16", "tile_w c no multiple of 16", "tile larger than the image", "w a multiple of tile_w", "any", "any"][_int(rng, 0, 5)]
        if bias == "tile_w c < 16":
            tw = _int(rng, 1, 15 // c)
        elif bias == "tile larger than the image":
            tw = w + _int(rng, 1, 23)
        elif bias == "w a multiple of tile_w":
            k = _int(rng, 2, 5)
            tw = max(1, w // k)
            w = tw * k
        else:
            tw = _int(rng, 1, w)
            while bias != "any" and tw * c % 16 == 0:
                tw += 1
        th = _int(rng, 1, h) if rng.random() < 0.8 else h + _int(rng, 1, 23)
        tw, th = _cap_tiles(w, h, tw, th, MAX_TILES)
    return dict(w=w, h=h, c=c, tile_w=tw, tile_h=th, bias=bias, composed=composed, quality=[0, _int(rng, 1, 99)][_int(rng, 0, 1)], seed=_int(rng, 0, 1 << 20),
                regions=[_region(rng, w, h, tw, th) for _ in range(3)], off=_offsets(rng, 8))


def _tile_measure(tiles, ref, w, h, c):
    d = merge_tiles(tiles, w, h).astype(np.int64) - ref.reshape(h, w, c).astype(np.int64)
    out = []
    for ch in range(c):
        out += [int((d[:, :, ch] ** 2).sum()), int(np.abs(d[:, :, ch]).max())]
    return out + [w * h]


def _tiled_ref(p):
    w, h, c, tw, th = p["w"], p["h"], p["c"], p["tile_w"], p["tile_h"]
    nx, ny = grid(w, h, tw, th)
    img = mixed_image(w, h, c, tw, p["seed"]) if p["composed"] else gen_image("noise", w, h, c, p["seed"])
    tiles = split_tiles(img, tw, th)
    # a tile raster of its own noise: a replicated pixel that is copied or counted shows
    other = np.random.default_rng(p["seed"]).integers(0, 256, tiles.shape, dtype=np.uint8)
    regions = []
    for _, x, y, rw, rh in p["regions"]:
        i0, j0, ni, nj = region_tiles(w, h, tw, th, x, y, rw, rh)
        sub = sub_grid(other, nx, i0, j0, ni, nj)
        regions.append((sub, merge_region(sub, tw, th, i0, j0, ni, x, y, rw, rh)))
    return dict(img=img, tiles=tiles, other=other, merged=merge_tiles(other, w, h), sums=_tile_measure(other, img, w, h, c), regions=regions)


def _tiled_cells(p):
    w, h, c, tw, th = p["w"], p["h"], p["c"], p["tile_w"], p["tile_h"]
    out = LC.k10_cells(w, h, c, tw, th)
    for _, x, y, rw, rh in p["regions"]:
        out |= LC.k10_region_cells(c, tw, th, x, y, rw, rh)
        if x + rw == w and y + rh == h:
            out.add("C%d region: touches the last row and column" % c)
    if p["composed"]:
        out.add("C%d: composed encode" % c)
    return out


def _tiled_dev(ctx, p, r):
    D, off = _Dev(), p["off"]
    w, h, c, tw, th = p["w"], p["h"], p["c"], p["tile_w"], p["tile_h"]
    T = frave_amd.api.PlanTiled(ctx, w, h, c, tw, th, TILED_ALLOW_HOLES)
    src = D.put(r["img"], off[0])
    cut = D.out(T.tile_bytes, off[1])
    T.split_tiles_dev(src.ptr, cut.ptr)
    D.same("split", D.get(cut, "split tiles"), r["tiles"])
    other = D.put(r["other"], off[2])
    back = D.out(T.pixel_bytes, off[3])
    T.merge_tiles_dev(other.ptr, back.ptr)
    D.same("merge", D.get(back, "merge raster"), r["merged"])
    sums = D.sums(2 * c + 1, off[4])
    T.measure_distortion_tiled_dev(other.ptr, src.ptr, sums.ptr)
    got = [int(v) for v in D.get(sums, "measure sums").view(np.uint64)]
    if got != r["sums"]:
        D.msgs.append("measure %s != %s" % (got, r["sums"]))
    D.untouched(src, "raster"), D.untouched(other, "tiles")
    for k, ((name, x, y, rw, rh), (sub, want)) in enumerate(zip(p["regions"], r["regions"])):
        if T.region_tiles(x, y, rw, rh) != region_tiles(w, h, tw, th, x, y, rw, rh):
            D.msgs.append("region %d: tiles" % k)
        d_sub = D.put(sub, off[5 + k % 2])
        dst = D.out(want.size, off[6 + k % 2])
        T.merge_tiles_region_dev(d_sub.ptr, x, y, rw, rh, dst.ptr)
        D.same("region %d (%s)" % (k, name), D.get(dst, "region %d raster" % k), want)
        D.untouched(d_sub, "region %d's tiles" % k)
    if p["composed"]:
        T.set_stream_order()
        qm = _qm(p["quality"])
        got = T.encode_image_tiled_symbols(r["img"], qm)
        Q = frave_amd.Plan(ctx, tw, th, c)
        Q.set_stream_order()
        for t in range(T.n_tiles):  # tile after tile, as the header lays the outputs out
            want = Q.encode_image_symbols(r["tiles"][t], qm, fit=True)
            if not all(_same_bits(g[t], v) for g, v in zip(got, want)):
                D.msgs.append("encode_image_tiled_symbols, tile %d" % t)
        Q.close()
    T.close()
    return D.msgs


# ---- tiled420: K12 -------------------------------------------------------------------------------------------------------------------------------------------

def _tiled420_draw(rng, case):
    composed = case % 4 == 0
    if composed:
        tw, th = _int(rng, 16, 72), _int(rng, 16, 72)
        w, h = _int(rng, 1, 4 * tw), _int(rng, 1, 4 * th)
        bias = "composed"
    else:
        w, h = _shape(rng)
        bias = ["tile_w < 16", "tile larger than the image", "w a multiple of tile_w", "tile_w >= 16", "any"][_int(rng, 0, 4)]
        if bias == "tile_w < 16":
            tw = _int(rng, 1, 15)
        elif bias == "tile larger than the image":
            tw = w + _int(rng, 1, 23)
        elif bias == "w a multiple of tile_w":
            k = _int(rng, 2, 5)
            tw = max(1, w // k)
            w = tw * k
        elif bias == "tile_w >= 16":
            tw = _int(rng, 16, max(16, w))
        else:
            tw = _int(rng, 1, w)
        th = _int(rng, 1, h) if rng.random() < 0.8 else h + _int(rng, 1, 23)
        tw, th = _cap_tiles(w, h, tw, th, MAX_TILES_420)
    return dict(w=w, h=h, tile_w=tw, tile_h=th, bias=bias, composed=composed, quality=_int(rng, 1, 99), seed=_int(rng, 0, 1 << 20),
                regions=[_region(rng, w, h, tw, th, 1 << 30) for _ in range(3)], off=_offsets(rng, 8))


def _tiled420_ref(p):
    w, h, tw, th = p["w"], p["h"], p["tile_w"], p["tile_h"]
    img = mixed_image(w, h, 3, tw, p["seed"]) if p["composed"] else gen_image("noise", w, h, 3, p["seed"])
    y, c = split_tiles420(img, tw, th)
    rng = np.random.default_rng(p["seed"])  # random planes: replicated pixels and other tiles' samples hold other values
    ry, rc = rng.integers(0, 256, y.shape, dtype=np.uint8), rng.integers(0, 256, c.shape, dtype=np.uint8)
    return dict(img=img, y=y, c=c, ry=ry, rc=rc, merged=merge_tiles420(ry, rc, w, h))


def _tiled420_cells(p):
    w, h, tw, th = p["w"], p["h"], p["tile_w"], p["tile_h"]
    out = LC.k12_split_cells(w, h, tw, th) | LC.k12_region_cells(tw, th, 0, 0, w, h, "whole merge")
    for _, x, y, rw, rh in p["regions"]:
        out |= LC.k12_region_cells(tw, th, x, y, rw, rh)
        out.add("region: %s x, %s y" % ("odd" if x & 1 else "even", "odd" if y & 1 else "even"))
    if p["composed"]:
        out.add("composed encode")
    return out


def _tiled420_dev(ctx, p, r):
    D, off = _Dev(), p["off"]
    w, h, tw, th = p["w"], p["h"], p["tile_w"], p["tile_h"]
    nx, ny = grid(w, h, tw, th)
    T = frave_amd.api.PlanTiled420(ctx, w, h, tw, th, TILED_ALLOW_HOLES)
    src = D.put(r["img"], off[0])
    dy, dc = D.out(T.y_tile_bytes, off[1]), D.out(T.c_tile_bytes, off[2])
    T.split_tiles420_dev(src.ptr, dy.ptr, dc.ptr)
    D.same("split, luma", D.get(dy, "y_tiles"), r["y"])
    D.same("split, chroma", D.get(dc, "c_tiles"), r["c"])
    D.untouched(src, "pixels")
    sy, sc = D.put(r["ry"], off[3]), D.put(r["rc"], off[4])
    dst = D.out(3 * w * h, off[5])
    T.merge_tiles420_dev(sy.ptr, sc.ptr, dst.ptr)
    D.same("whole merge", D.get(dst, "merge raster"), r["merged"])
    D.untouched(sy, "y_tiles"), D.untouched(sc, "c_tiles")
    for k, (name, x, y, rw, rh) in enumerate(p["regions"]):
        i0, j0, ni, nj = region_tiles(w, h, tw, th, x, y, rw, rh)
        if T.region_tiles(x, y, rw, rh) != (i0, j0, ni, nj):
            D.msgs.append("region %d: tiles" % k)
        want = np.ascontiguousarray(r["merged"][y: y + rh, x: x + rw])
        uy, uc = D.put(sub_grid420(r["ry"], nx, i0, j0, ni, nj), off[6]), D.put(sub_grid420(r["rc"], nx, i0, j0, ni, nj), off[7])
        out = D.out(want.size, off[(5 + k) % 8])
        T.merge_tiles420_region_dev(uy.ptr, uc.ptr, x, y, rw, rh, out.ptr)
        D.same("region %d (%s)" % (k, name), D.get(out, "region %d raster" % k), want)
        D.untouched(uy, "region %d's y_tiles" % k), D.untouched(uc, "region %d's c_tiles" % k)
    if p["composed"]:
        T.set_stream_order()
        sym, vp, wp, hist, oob = T.encode_image_tiled420_symbols(r["img"], p["quality"])
        n, n_y, n_c = T.n_tiles, T.n_luma, T.n_chroma
        luma, chroma = sym[: n * n_y].reshape(n, n_y), sym[n * n_y:].reshape(n, 2, n_c)
        cw, ch = chroma_shape(tw, th)
        qm = _qm(p["quality"])
        for t in range(n):  # the restatement's planes of every tile through the plain route, compared in plane order
            for k, plane in enumerate((r["y"][t], r["c"][t, 0], r["c"][t, 1])):
                rsym, rvp, rwp, rhist, roob = _plain(ctx, plane, tw if k == 0 else cw, th if k == 0 else ch, 1, qm)
                i = plane_index(n, t, k)
                got = luma[t] if k == 0 else chroma[t, k - 1]
                if not (_same_bits(got, rsym.reshape(-1)) and _same_bits(hist[i], rhist[0]) and _same_bits(vp[i], rvp[0]) and _same_bits(wp[i], rwp[0]) and int(oob[i]) == int(roob[0])):
                    D.msgs.append("encode_image_tiled420_symbols, tile %d plane %d" % (t, k))
    T.close()
    return D.msgs


# ---- rans: K11 -----------------------------------------------------------------------------------------------------------------------------------------------

def _rans_draw(rng, case):
    n = _int(rng, 1, 20000) if rng.random() < 0.25 else _int(rng, 1, 2000)  # (the reference codes symbol by symbol in Python: long streams are few ...
    planes = [1, 1, 1, 2, 2, 3, 6][_int(rng, 0, 6 if n <= 4000 else 4)]  # ... and most batches small: a plane's ten models cost the reference more than its symbols)
    share = rng.dirichlet(np.full(10, rng.uniform(0.2, 3.0)))
    inject = ["none"] * 5 + ["bad"]
    return dict(n=n, planes=planes, share=[round(float(v), 6) for v in share], outliers=round(float(rng.uniform(0.0, 0.08)), 4), symbol_stride=n + (0 if rng.random() < 0.3 else _int(rng, 1, 40)),
                inject=inject[_int(rng, 0, 5)], inject_kind=["bucket", "uncounted"][_int(rng, 0, 1)], inject_plane=_int(rng, 0, planes - 1), inject_at=[_int(rng, 0, n - 1) for _ in range(2)],
                seed=_int(rng, 0, 1 << 30), off=_offsets(rng, 7))


def _rans_ref(p):
    share = np.array(p["share"])
    streams = np.stack([rans_cases.random_stream(p["n"], p["seed"] + k, p["outliers"], share / share.sum()) for k in range(p["planes"])])
    hist = np.stack([rans_ref.histogram(s) for s in streams])
    if p["inject"] == "bad":
        s, k = streams[p["inject_plane"]], p["inject_plane"]
        for at in p["inject_at"]:
            if p["inject_kind"] == "bucket":
                s[at] = (10 + at % 6) << 10 | (s[at] & 1023)  # an entry of no chain
            else:
                b = int(s[at]) >> 10
                free = np.flatnonzero(hist[k, min(b, 9)] == 0)
                if free.size and b < 10:
                    s[at] = b << 10 | int(free[-1])  # a symbol the histogram does not count
    return dict(streams=streams, hist=hist, refs=[rans_ref.encode_plane(s, hh) for s, hh in zip(streams, hist)])


def _rans_cells(p):
    return {"a refused plane" if p["inject"] == "bad" else "every plane coded", "streams %s than their length apart" % ("further" if p["symbol_stride"] > p["n"] else "no further")}


def _rans_dev(ctx, p, r):
    import frave_amd.api as api

    D, off, n, planes = _Dev(), p["off"], p["n"], p["planes"]
    stride = n + 20
    padded = np.full((planes, p["symbol_stride"]), 0xFFFF, np.uint16)
    padded[:, :n] = r["streams"]
    d_sym, d_hist = D.put(padded, off[0], 16), D.put(r["hist"], off[1], 16)
    sizes = dict(words=planes * stride * 4, n_words=planes * 4, models=planes * 160, off=planes * 10 * 1024 * 2, status=planes * 16)
    out = {k: D.out(v, off[2 + i], 16) for i, (k, v) in enumerate(sizes.items())}
    scratch = D.torch.empty(api.rans_scratch_bytes(planes, n) + 256, dtype=D.torch.uint8, device="cuda")
    api.rans_encode_planes_dev(ctx, planes, d_sym.ptr, p["symbol_stride"], n, d_hist.ptr, api.RANS_EMPTY_OK, out["words"].ptr, stride, out["n_words"].ptr, out["models"].ptr,
                               out["off"].ptr, out["status"].ptr, (scratch.data_ptr() + 255) & ~255, 0)
    got = {k: D.get(g, "K11 " + k) for k, g in out.items()}
    fill = {k: g.fill[g.start: g.start + g.size] for k, g in out.items()}
    words, words_fill = got["words"].view(np.uint32).reshape(planes, stride), fill["words"].view(np.uint32).reshape(planes, stride)
    lists, lists_fill = got["off"].view(np.uint16).reshape(planes, 10, 1024), fill["off"].view(np.uint16).reshape(planes, 10, 1024)
    n_words, models, status = got["n_words"].view(np.uint32), got["models"].view(np.uint32).reshape(planes, 10, 4), got["status"].view(np.uint32).reshape(planes, 4)
    for k, ref in enumerate(r["refs"]):
        if ref.status:  # the reference's refusal, with its positions
            if status[k].tolist() != [ref.status, ref.zero_at, ref.bucket_at, 0]:
                D.msgs.append("plane %d: status %s, the reference %s" % (k, status[k].tolist(), [ref.status, ref.zero_at, ref.bucket_at, 0]))
            continue
        m = len(ref.words)
        if status[k].tolist() != [0, 0, 0, 0] or int(n_words[k]) != m:
            D.msgs.append("plane %d: status %s, %d words, the reference %d" % (k, status[k].tolist(), int(n_words[k]), m))
            continue
        if not np.array_equal(words[k, :m], ref.words):
            D.msgs.append("plane %d: words" % k)
        if not np.array_equal(words[k, m:], words_fill[k, m:]):
            D.msgs.append("plane %d: words behind the stream were written" % k)
        for b in range(10):
            n_off = len(ref.off[b])
            if (int(models[k, b, 0]), int(models[k, b, 1])) != (ref.max_freq_bits[b], n_off) or lists[k, b, :n_off].tolist() != ref.off[b]:
                D.msgs.append("plane %d context %d: model or list" % (k, b))
            if not np.array_equal(lists[k, b, n_off:], lists_fill[k, b, n_off:]):
                D.msgs.append("plane %d context %d: entries behind the list were written" % (k, b))
    D.untouched(d_sym, "streams"), D.untouched(d_hist, "histograms")
    return D.msgs


# ---- decode: K13 on crafted planes ----------------------------------------------------------------------------------------------------------------------------

DECODE_FAMILIES = ["kat", "mild", "grow", "saturated", "negative width", "nan", "inf", "edges", "groups"]
DECODE_EDGES = [2.999, 3.0, 29.999, 30.0, 31.0, 32.0, 4294967296.0]


def _decode_params(rng, family):
    """(value_params, width_params) float32 [3][6] of a family of tests/decode_cases.py, the magnitudes drawn"""
    f = np.float32
    sign = lambda: f(1 if rng.random() < 0.5 else -1)  # noqa: E731
    vp, wp = DC.KAT_V.copy(), DC.KAT_W.copy()
    if family == "kat":
        vp, wp = vp * f(rng.uniform(0.5, 1.5)), wp * f(rng.uniform(0.5, 2.0))
    elif family == "mild":
        wp = DC.MILD_W * rng.uniform(0.3, 3.0, (3, 1)).astype(f)
    elif family == "grow":
        vp = np.full((3, 6), sign() * f(rng.uniform(1.1, 3.0)), f)
        wp = DC.MILD_W.copy() if rng.random() < 0.5 else wp
    elif family == "saturated":
        vp, wp = np.full((3, 6), sign() * f(10.0 ** rng.uniform(9, 38)), f), np.full((3, 6), sign() * f(10.0 ** rng.uniform(9, 38)), f)
    elif family == "negative width":
        wp = np.full((3, 6), -f(10.0 ** rng.uniform(-1, 2)), f)
    elif family == "nan":
        k = _int(rng, 0, 2)
        vp, wp = (np.full((3, 6), np.nan, f) if k != 1 else vp), (np.full((3, 6), np.nan, f) if k != 0 else wp)
    elif family == "inf":
        vp, wp = np.full((3, 6), sign() * f(np.inf), f), DC.INF_W * sign()
    elif family == "edges":
        wp = np.zeros((3, 6), f)
        wp[:, 0] = [DECODE_EDGES[_int(rng, 0, 6)] if rng.random() < 0.6 else rng.uniform(0, 40) for _ in range(3)]
    else:
        vp, wp = DC.GROUP_V * rng.uniform(0.5, 1.5, (3, 1)).astype(f), DC.GROUP_W * rng.uniform(0.5, 1.5, (3, 1)).astype(f)
    return vp.astype(f), wp.astype(f)


def _decode_draw(rng, case):
    family = DECODE_FAMILIES[case % len(DECODE_FAMILIES)] if case < 2 * len(DECODE_FAMILIES) else DECODE_FAMILIES[_int(rng, 0, len(DECODE_FAMILIES) - 1)]
    vp, wp = _decode_params(rng, family)
    rule = DC.RULES[_int(rng, 0, 3)]
    return dict(shape=list(DC.LARGE if rng.random() < 0.2 else DC.SMALL), family=family, vp=[[float(v) for v in row] for row in vp], wp=[[float(v) for v in row] for row in wp],
                rule=rule, p=round(float(rng.uniform(0.04, 0.5)), 3), multiplier=DC.MULTIPLIERS[_int(rng, 0, 3)], level=_int(rng, 0, 9), seed=_int(rng, 0, 1 << 30), off=_offsets(rng, 8))


_decode_walks = {}


def _decode_walk(p):
    """the case's plane walked on the oracle (tests/decode_cases.walk), once per case"""
    key = repr(sorted(p.items()))
    if key not in _decode_walks:
        rule = ("geometric", p["p"]) if p["rule"] == "geometric" else p["rule"]
        vp, wp = np.array(p["vp"], np.float32), np.array(p["wp"], np.float32)
        r = DC.walk(*p["shape"], vp, wp, rule, p["seed"])
        r["hist_scaled"], r["multiplier_used"] = DC.scaled_histogram(r["hist"], p["multiplier"])
        r.update(vp=vp, wp=wp, shape=tuple(p["shape"]))
        _decode_walks[key] = r
    return _decode_walks[key]


def _decode_ref(p):
    import frave_amd.emit as emit

    r = _decode_walk(p)
    frv = DC.file_of([r])
    L = DC.lattice(*p["shape"])
    compact = emit.tiled_decode_levels(frv, p["level"])[1].reshape(L.F, 1 << p["level"])
    if not np.array_equal(compact, r["plane"][:, : 1 << p["level"]]):
        raise AssertionError("the host decoder does not return the oracle walk's plane: %s" % p)
    return dict(coded=emit.tiled_parse_coded(frv), want=preview_ref.expand(compact, L.some))


def _decode_cells(p):
    return DC.cells_of(_decode_walk(p)) | {"%d x %d" % tuple(p["shape"]), "level %d" % p["level"], "family: " + p["family"], "rule: " + p["rule"]}


DECODE_CELLS = set(DC.CELLS) | {"%d x %d" % s for s in (DC.SMALL, DC.LARGE)} | {"level %d" % k for k in range(10)} | {"family: " + f for f in DECODE_FAMILIES} | {"rule: " + r for r in DC.RULES}


def _decode_dev(ctx, p, r):
    import frave_amd.api as api

    D, off = _Dev(), p["off"]
    ti, words, n_words, models, lists, vp, wp = r["coded"]
    stride = words.shape[1]
    P = frave_amd.Plan(ctx, *p["shape"], 1)
    P.set_stream_order()
    ins = [D.put(a, off[i], 16) for i, a in enumerate((words, n_words, models, lists, vp, wp))]
    coefs, status = D.out(4 * P.num_cells * 512, off[6], 16), D.out(16, off[7], 16)
    scratch = D.torch.empty(api.decode_scratch_bytes(1) + 256, dtype=D.torch.uint8, device="cuda")
    api.decode_planes_dev(P, 1, ins[0].ptr, stride, *(g.ptr for g in ins[1:]), coefs.ptr, P.num_cells * 512, status.ptr, (scratch.data_ptr() + 255) & ~255, 0, levels=p["level"])
    got_status = D.get(status, "K13 status").view(np.uint32)
    if got_status.any():
        D.msgs.append("K13 status %s" % got_status.tolist())
    D.same("K13 coefficients", D.get(coefs, "K13 coefficients").view(np.int32), r["want"])
    for g, name in zip(ins, ("words", "n_words", "models", "lists", "value parameters", "width parameters")):
        D.untouched(g, name)
    P.close()
    return D.msgs


# ---- preconditions and the sweep -----------------------------------------------------------------------------------------------------------------------------

def violated(kind, p):
    """the documented preconditions (include/fri_hip.h) a drawn case does not satisfy: [] for every case the sweep may run"""
    bad = []
    if "w" in p and not (p["w"] >= 1 and p["h"] >= 1):
        bad.append("zero size")
    if "quality" in p and not 0 <= p["quality"] <= 100:
        bad.append("quality")
    if kind in ("c420", "tiled420", "ycbcr") and not 1 <= p["quality"] <= 99:
        bad.append("a YCbCr quality is 1..99")
    if kind == "ssim" and not (p["w"] >= 8 and p["h"] >= 8 and 1 <= p["n_images"] <= 65535 and p["c"] in (1, 3)):
        bad.append("K7 needs W, H >= 8")
    if kind in ("tiled", "tiled420"):
        nx, ny = grid(p["w"], p["h"], p["tile_w"], p["tile_h"])
        if nx * ny > (MAX_TILES if kind == "tiled" else MAX_TILES_420) or nx * ny * 3 > 65535:
            bad.append("tiles")
        if p["composed"] and nx * ny > MAX_TILES_COMPOSED:
            bad.append("tiles of a composed case")
        for _, x, y, rw, rh in p["regions"]:
            if not (rw >= 1 and rh >= 1 and x >= 0 and y >= 0 and x + rw <= p["w"] and y + rh <= p["h"]):
                bad.append("region")
    if kind == "rans" and not (1 <= p["planes"] <= 65535 and 1 <= p["n"] <= 20000 and p["symbol_stride"] >= p["n"]):
        bad.append("K11 counts")
    if kind == "decode":  # the generator conditions of tests/decode_cases.py
        if tuple(p["shape"]) not in (DC.SMALL, DC.LARGE) or p["rule"] not in DC.RULES or p["multiplier"] not in DC.MULTIPLIERS or not 0 <= p["level"] <= 9:
            bad.append("K13 draw")
        else:
            r = _decode_walk(p)
            if r["symbol"].min() < 0 or r["symbol"].max() > 1022:
                bad.append("a symbol outside 0..1022")
            bad += DC.histogram_violations(r["hist_scaled"])
            if (r["plane"][DC.lattice(*p["shape"]).some] == DC.NONE).any():
                bad.append("a Some(INT32_MIN)")
    if any(not 0 <= o <= 15 for o in p["off"]):
        bad.append("offset")
    return bad


def _no_cells(p):
    return set()


# kind -> (k of default_rng([seed, k]), draw, reference, cells, device checks)
KINDS = {"ycbcr": (1, _ycbcr_draw, _ycbcr_ref, _no_cells, _ycbcr_dev), "ssim": (2, _ssim_draw, _ssim_ref, _ssim_cells, _ssim_dev),
         "rate": (3, _rate_draw, _rate_ref, _rate_cells, _rate_dev), "c420": (4, _c420_draw, _c420_ref, _c420_cells, _c420_dev),
         "rgba": (5, _rgba_draw, _rgba_ref, _rgba_cells, _rgba_dev), "tiled": (6, _tiled_draw, _tiled_ref, _tiled_cells, _tiled_dev),
         "tiled420": (7, _tiled420_draw, _tiled420_ref, _tiled420_cells, _tiled420_dev), "rans": (8, _rans_draw, _rans_ref, _rans_cells, _rans_dev),
         "decode": (9, _decode_draw, _decode_ref, _decode_cells, _decode_dev)}


def sweep(kind, n_cases, seed, ctx=None, dry=False, only=None):
    """(mismatching cases, the cells the cases reach, the drawn cases); only = a case index: the draws run as always, that case alone is checked"""
    k, draw, reference, cells, device = KINDS[kind]
    rng = np.random.default_rng([seed, k])
    if not dry:
        ctx = ctx or frave_amd.Context(0)
    bad, reached, cases = 0, set(), []
    for case in range(n_cases):
        p = draw(rng, case)
        cases.append(p)
        reached |= cells(p)
        if only is not None and case != only:
            continue
        r = reference(p)
        if dry:
            continue
        try:
            msgs = device(ctx, p, r)
        except FriHipError as e:  # every drawn case is valid: an error is a mismatch (anything else propagates and ends the run)
            msgs = ["error: %s" % e]
        if msgs:
            bad += 1
            print("%s case %d seed %d: %s: MISMATCH in %s" % (kind, case, seed, p, msgs), flush=True)
    print("%s: %d cases, %d mismatching%s" % (kind, n_cases, bad, " (dry run: no device call)" if dry else ""), flush=True)
    return bad, reached, cases


def run(kind, n_cases, seed, ctx=None, dry=False):
    """n_cases random cases of one kind; returns the number of mismatching ones and prints a line for each, with everything that replays it"""
    return sweep(kind, n_cases, seed, ctx, dry)[0]


if __name__ == "__main__":
    kind = sys.argv[1]
    sys.exit(1 if run(kind, int(sys.argv[2]) if len(sys.argv) > 2 else LC.N_CASES[kind], int(sys.argv[3]) if len(sys.argv) > 3 else LC.SEED) else 0)
