"""Every reachable K1 and K3 instance against references that involve no GPU code (the case table and what each case reaches: tests/instance_cases.py,
checked on the host by tests/test_instance_cases_host.py). Bit-exact throughout.

- K1 (int32 planes): the oracle's quantised coefficients of the image, of rct(image) on a colour-transformed plan.
- K1 C16 (the compact int16 planes of fri_hip_encode_symbols_batch_dev with d_coefs = NULL), through the gather route and the direct route: the symbol
  streams against the oracle's buckets and predictions, the histograms and the out-of-alphabet counts against oracle.Wavelet.predict.
- K3: the oracle's raster of numpy-dequantised oracle coefficients (inverse_rct on top for RCT plans), written between guard bytes.
- MEASURE: the [2 C + 1] sums over that raster and the oracle's own covered pixels, recomputed in numpy.
Every device buffer a case touches has guard bytes of a fill pattern around it (and between the images of a batch), which must be intact afterwards."""
import numpy as np
import pytest

from tests.common import gen_image, random_params
from tests.instance_cases import CASES, knobs, qmatrix
from tests.oracle_ref import numpy_measure, oracle_coefficients, oracle_owned, oracle_raster
from tests.test_rct_host import correlated_image

pytestmark = pytest.mark.gpu
GUARD = 64  # bytes of fill pattern in front of and behind every buffer


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


def _plan(ctx, case):
    """the device plan of the case, created under its knobs; a pinned tiling is asserted to be the host-only plan's, which instance_of reads"""
    import frave_amd as fa

    w, h, c = case.shape
    with knobs(case.env()):
        P = fa.Plan(ctx, w, h, c)
        H = fa.Plan(None, w, h, c) if case.pinned else None
    if H is not None:
        assert P.tiling() == H.tiling(), case.id
        for a, b in zip(P.tile_table(), H.tile_table()):
            assert np.array_equal(a, b), case.id
        assert P.inverse_lists() == H.inverse_lists(), case.id
        H.close()
    if case.rct:
        P.set_colour_transform(1)
    P.set_dequantiser(case.deq)
    return P


def _images(case):
    w, h, c = case.shape
    out = []
    for k in range(case.n_images):
        s = 1000 * case.seed + k
        if case.rct:
            img = correlated_image(w, h, s)
            img[: h // 3] = gen_image("noise", w, h // 3, c, s)  # and a band no colour transform can predict
        else:
            img = gen_image("noise", w, h, c, s)
            img[: h // 2] = gen_image("smooth", w, h // 2, c, s + 1)
        out.append(np.ascontiguousarray(img).reshape(-1))
    return out


def _pattern(n, salt):
    return ((np.arange(n, dtype=np.int64) * 151 + 7 * salt + 13) & 255).astype(np.uint8)


class Guarded:
    """a device byte buffer: GUARD bytes, then the case's `offset` past a 256-byte boundary, n_images regions of `size` bytes `stride` apart, GUARD bytes;
    every byte starts as a fill pattern"""

    def __init__(self, torch, size, n_images=1, stride=0, offset=0, salt=0):
        self.size, self.n, self.stride = size, n_images, stride if n_images > 1 else size
        span = (self.n - 1) * self.stride + size
        self.raw = torch.empty(span + 2 * GUARD + 512 + offset, dtype=torch.uint8, device="cuda")
        self.start = (-self.raw.data_ptr()) % 256 + 256 + offset  # >= GUARD bytes in front
        self.fill = _pattern(self.raw.numel(), salt)
        self.raw.copy_(torch.from_numpy(self.fill))
        self.ptr = self.raw.data_ptr() + self.start

    def put(self, torch, arrays):
        host = self.fill.copy()
        for k, a in enumerate(arrays):
            host[self.start + k * self.stride : self.start + k * self.stride + self.size] = a
        self.raw.copy_(torch.from_numpy(host))

    def get(self, torch):
        """(the n_images regions, bool: every byte outside them - guards and gaps - is still the fill pattern)"""
        torch.cuda.synchronize()
        host = self.raw.cpu().numpy()
        inside = np.zeros(host.size, bool)
        for k in range(self.n):
            inside[self.start + k * self.stride : self.start + k * self.stride + self.size] = True
        regions = [host[self.start + k * self.stride : self.start + k * self.stride + self.size].copy() for k in range(self.n)]
        return regions, bool(np.array_equal(host[~inside], self.fill[~inside]))


def _guarded_coefs(torch, P, n):
    """int32 coefficient planes [n][C][F][512] with GUARD bytes of a known int32 on both sides"""
    g = GUARD // 4
    buf = torch.full((n * P.coef_count + 2 * g,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    return buf, buf.data_ptr() + GUARD


def _check_guards_i32(buf):
    host = buf.cpu().numpy()
    g = GUARD // 4
    return bool((host[:g] == 0x5A5A5A5A).all() and (host[-g:] == 0x5A5A5A5A).all())


def _run_k1(ctx, oracle, case):
    import torch

    w, h, c = case.shape
    P = _plan(ctx, case)
    qm = qmatrix(case.quant)
    imgs = _images(case)
    px = Guarded(torch, P.pixel_bytes, case.n_images, case.pixel_stride, case.offset, case.seed)
    px.put(torch, imgs)
    co, co_ptr = _guarded_coefs(torch, P, case.n_images)
    P.transform_quant_dev(px.ptr, co_ptr, qm, n_images=case.n_images, pixel_stride=case.pixel_stride, coef_stride=P.coef_count)
    torch.cuda.synchronize()
    got = co.cpu().numpy()[GUARD // 4 : GUARD // 4 + case.n_images * P.coef_count].reshape(case.n_images, c, P.num_cells, 512)
    assert _check_guards_i32(co), "K1 wrote outside the coefficient planes"
    _, intact = px.get(torch)
    assert intact, "K1 wrote into its pixels' guards"
    for k, img in enumerate(imgs):
        want = oracle_coefficients(oracle, img, w, h, c, qm, case.rct)
        assert np.array_equal(got[k], want), (case.id, k, int((got[k] != want).sum()))
    P.close()


def _oracle_symbols(oracle, img, w, h, c, qm, rct, params, order):
    """the streams, histograms and out-of-alphabet counts of the oracle: per channel bucket << 10 | zigzag(coefficient - prediction) & 1023 in stream order"""
    from tests.test_rct_host import rct as forward_rct

    W = oracle.Wavelet(forward_rct(img) if rct else img, h, w, c)
    W.quantize(qm)
    co = W.coefficients()
    syms, hists, oobs = [], [], []
    for ch in range(c):
        b, p, hist, oob = W.predict(ch, params[ch, 0], params[ch, 1])
        d = (co[ch].reshape(-1)[order].astype(np.int64) - p.reshape(-1)[order].astype(np.int64)).astype(np.int32)
        syms.append((b.reshape(-1)[order].astype(np.uint32) << 10 | (((d.astype(np.uint32) << 1) ^ (d >> 31).astype(np.uint32)) & 1023)).astype(np.uint16))
        hists.append(hist)
        oobs.append(oob)
    W.close()
    return np.stack(syms), np.stack(hists), np.array(oobs, np.int64)


def _run_c16(ctx, oracle, case):
    import torch

    w, h, c = case.shape
    P = _plan(ctx, case)
    order = P.set_stream_order()
    qm = qmatrix(case.quant)
    imgs = _images(case)
    vp, wp = random_params(11 + case.seed, 0.1)
    params = np.broadcast_to(np.stack([np.asarray(vp, np.float32).reshape(3, 6), np.asarray(wp, np.float32).reshape(3, 6)]), (c, 2, 3, 6)).copy()
    want = [_oracle_symbols(oracle, img, w, h, c, qm, case.rct, params, order) for img in imgs]
    n_img, n, plane = case.n_images, P.num_some, P.num_cells * 512
    px = Guarded(torch, P.pixel_bytes, n_img, case.pixel_stride, case.offset, case.seed)
    px.put(torch, imgs)
    for direct in (False, True):  # node words + gather kernel, or the scan writing the streams itself
        d_w = torch.full((n_img * c * plane,), 0xEEEE, dtype=torch.uint16, device="cuda")
        d_st = torch.full((n_img * c * n + 16,), 0xFFFF, dtype=torch.uint16, device="cuda")
        d_h = torch.full((n_img, c, 10, 1024), -1, dtype=torch.int32, device="cuda")
        d_o = torch.full((n_img, c), -1, dtype=torch.int64, device="cuda")
        d_par = torch.from_numpy(np.broadcast_to(params, (n_img, c, 2, 3, 6)).copy()).cuda()
        P.encode_symbols_batch_dev(n_img, px.ptr, case.pixel_stride, qm, False, d_par.data_ptr(), 0, c * plane, 0 if direct else d_w.data_ptr(), c * plane,
                                   d_st.data_ptr(), c * n, d_h.data_ptr(), d_o.data_ptr(), None)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy()
        assert (st[n_img * c * n :] == 0xFFFF).all(), "the streams' tail was written"
        st = st[: n_img * c * n].reshape(n_img, c, n)
        hist, oob = d_h.cpu().numpy().view(np.uint32), d_o.cpu().numpy()
        for k in range(n_img):
            wsym, whist, woob = want[k]
            assert np.array_equal(hist[k], whist), (case.id, direct, k, "histograms")
            assert np.array_equal(oob[k], woob), (case.id, direct, k, "out-of-alphabet counts")
            for ch in range(c):
                if woob[ch] == 0:  # (a symbol out of the alphabet has no defined stream word)
                    assert np.array_equal(st[k, ch], wsym[ch]), (case.id, direct, k, ch, int((st[k, ch] != wsym[ch]).sum()))
        assert direct or (d_w.cpu().numpy() != 0xEEEE).any()
        assert not direct or (d_w.cpu().numpy() == 0xEEEE).all()
    _, intact = px.get(torch)
    assert intact
    assert sum(int(woob.sum()) for _, _, woob in want) == 0, "the case's parameters should keep every symbol inside the alphabet"
    P.close()


def _k3_inputs(oracle, case, P):
    import torch

    w, h, c = case.shape
    qm = qmatrix(case.quant)
    imgs = _images(case)
    owned = oracle_owned(oracle, w, h, c)
    coefs = [oracle_coefficients(oracle, img, w, h, c, qm, case.rct) for img in imgs]
    recon = [oracle_raster(oracle, co, qm, case.deq, w, h, c, case.rct, owned) for co in coefs]
    d_co = torch.from_numpy(np.stack([co.reshape(-1) for co in coefs])).cuda()
    return qm, imgs, owned, recon, d_co


def _run_k3(ctx, oracle, case):
    import torch

    P = _plan(ctx, case)
    qm, imgs, owned, recon, d_co = _k3_inputs(oracle, case, P)
    out = Guarded(torch, P.pixel_bytes, case.n_images, case.pixel_stride, case.offset, case.seed)
    P.inverse_transform_batch_dev(case.n_images, d_co.data_ptr(), P.coef_count, out.ptr, case.pixel_stride, qm)
    got, intact = out.get(torch)
    assert intact, "K3 wrote into the guards or the gaps between images"
    for k in range(case.n_images):
        bad = got[k] != recon[k]
        assert not bad.any(), (case.id, k, int(bad.sum()), np.flatnonzero(bad)[:8].tolist(), "covered" if owned[np.flatnonzero(bad)[0]] else "hole")
    P.close()


def _run_measure(ctx, oracle, case):
    import torch

    w, h, c = case.shape
    P = _plan(ctx, case)
    qm, imgs, owned, recon, d_co = _k3_inputs(oracle, case, P)
    ref = Guarded(torch, P.pixel_bytes, 1, 0, case.offset, case.seed)
    ref.put(torch, imgs)
    d_out = torch.full((2 * c + 1,), 77, dtype=torch.int64, device="cuda")  # the entry point zeroes it
    P.measure_distortion_dev(d_co.data_ptr(), ref.ptr, d_out.data_ptr(), qm)
    torch.cuda.synchronize()
    got = [int(x) for x in d_out.cpu().numpy().astype(np.uint64)]
    want = numpy_measure(recon[0], imgs[0], owned, c)
    assert got == want, (case.id, got, want)
    assert any(want[2 * ch] for ch in range(c)), "a lossy case: some sum must not be zero"
    _, intact = ref.get(torch)
    assert intact
    P.close()


RUN = {"k1": _run_k1, "c16": _run_c16, "k3": _run_k3, "measure": _run_measure}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_instance(ctx, oracle, case):
    RUN[case.kind](ctx, oracle, case)
