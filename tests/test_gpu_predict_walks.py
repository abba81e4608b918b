"""Every K2 / K4 instance on the grids and tile walks of tests/predict_cases.py, against references that involve no GPU code (the table and what each case
reaches are checked on the host by tests/test_predict_cases_host.py).

- K2: buckets, predictions, histograms and out-of-alphabet counts bit for bit against oracle.Wavelet.predict; the word and stream forms through the symbol
  streams, as tests/test_gpu_instances.py checks them.
- K4: the integer sums (gram, wtw) exactly against the numpy sums over the oracle's neighbour values; W^T r bit for bit against the restatement of its f32
  partial sums and fixed-point total (tests/fit_ref.py), hence the same on a default plan and as plane 0 of a two-plane launch; value and width parameters
  from the tail solve and the solve kernel bit for bit the host solves of those sums; the out-of-range count of injected coefficients the default plan's,
  and not zero.
Every device output starts as a non-zero fill pattern between guard bytes, the histogram too (the kernel clears it). Every case runs twice on one plan, with
a launch of another plane count in between, and must give the same results the second time (hand-over serial numbers, tickets, accumulator shards)."""
import numpy as np
import pytest

from tests import fit_ref
from tests.common import gen_image, random_params
from tests.oracle_ref import cpu_fit_sums, oracle_coefficients
from tests.predict_cases import CASES, knobs
from tests.test_gpu_instances import _oracle_symbols

pytestmark = pytest.mark.gpu
GUARD = 64  # bytes of fill pattern in front of and behind every buffer
QI = np.ones(32, np.int32)
IU7, IU6 = np.triu_indices(7), np.triu_indices(6)


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


class Buf:
    """a device array of n elements of `dtype` between GUARD bytes, every element (guards included) first set to `fill`"""

    def __init__(self, torch, n, dtype, fill):
        self.dtype, self.n = np.dtype(dtype), n
        self.g = GUARD // self.dtype.itemsize
        self.fill = np.array(fill).astype(self.dtype)
        host = np.full(n + 2 * self.g, self.fill, self.dtype)
        self.raw = torch.from_numpy(host.view(np.uint8)).cuda()
        self.ptr = self.raw.data_ptr() + GUARD

    def get(self):
        """the n elements; asserts the guards are intact"""
        import torch

        torch.cuda.synchronize()
        host = self.raw.cpu().numpy().view(self.dtype)
        assert (host[: self.g] == self.fill).all() and (host[self.g + self.n :] == self.fill).all(), "written outside the buffer"
        return host[self.g : self.g + self.n].copy()


def _dev(torch, arr, dtype):
    b = Buf(torch, arr.size, dtype, 0)
    host = np.full(arr.size + 2 * b.g, b.fill, b.dtype)
    host[b.g : b.g + arr.size] = np.asarray(arr, dtype).reshape(-1)
    b.raw.copy_(torch.from_numpy(host.view(np.uint8)))
    return b


def _plan(ctx, case, pinned=True):
    import frave_amd as fa

    with knobs(case.env() if pinned else None):
        P = fa.Plan(ctx, *case.shape)
    if pinned and case.pinned:
        g = P.predict_grid()
        assert (g["pred_blocks"], g["hist_blocks"], g["k4_older_eighths"]) == case.grid, case.id
    return P


def _images(case):
    w, h, c = case.shape
    out = []
    for k in range(case.n_images):
        s = 1000 * case.seed + k
        img = gen_image("noise", w, h, c, s)
        img[: h // 2] = gen_image("smooth", w, h // 2, c, s + 1)
        out.append(np.ascontiguousarray(img).reshape(-1))
    return out


def _params(case, planes):
    out = np.zeros((planes, 2, 3, 6), np.float32)
    for k in range(planes):
        out[k] = random_params(7 + case.seed + k, 0.15)
    return out


def _inject(co, count, seed):
    """`count` Some coefficients of every plane set outside [-256, 255]"""
    co = co.copy()
    rng = np.random.default_rng(seed)
    for plane in co.reshape(-1, co.shape[-2], 512):
        some = np.flatnonzero(plane.reshape(-1) != -(2 ** 31))
        at = rng.choice(some, count, replace=False)
        plane.reshape(-1)[at] = rng.choice([-1, 1], count) * rng.integers(300, 70000, count)
    return co


def _wavelet(oracle, case, co):
    w, h, c = case.shape
    W = oracle.Wavelet(np.zeros(w * h * c, np.uint8), h, w, c)
    W.set_coefficients(co)
    return W


# ---- the routes ---------------------------------------------------------------------------------------------------------------------------------------
def _coefs(oracle, case):
    w, h, c = case.shape
    return np.stack([oracle_coefficients(oracle, img, w, h, c, QI) for img in _images(case)])  # [n_images][C][F][512]


def _k2_expect(oracle, case, co, params):
    """[(bucket, prediction, hist, oob)] per plane"""
    c = case.shape[2]
    out = []
    for i in range(co.shape[0]):
        W = _wavelet(oracle, case, co[i])
        for ch in range(c):
            out.append(W.predict(ch, params[i * c + ch, 0], params[i * c + ch, 1]))
        W.close()
    return out


def _check_k2(case, got, want):
    b, p, hist, oob = got
    for k, (wb, wp, wh, wo) in enumerate(want):
        assert np.array_equal(hist[k], wh), (case.id, k, "histogram")
        assert int(oob[k]) == int(wo), (case.id, k, "out of alphabet")
        assert np.array_equal(b[k], wb.reshape(-1)), (case.id, k, "buckets")
        assert np.array_equal(p[k], wp.reshape(-1)), (case.id, k, "predictions")


def _run_predict(torch, P, case, co, params):
    n, plane = co.reshape(-1, P.num_cells * 512).shape[0], P.num_cells * 512
    d_co = _dev(torch, co, np.int32)
    d_par = _dev(torch, params, np.float32)
    d_b, d_p = Buf(torch, n * plane, np.uint8, 0xA7), Buf(torch, n * plane, np.int32, 0x5A5A5A5A)
    d_h, d_o = Buf(torch, n * 10 * 1024, np.uint32, 0x3C3C3C3C), Buf(torch, n, np.uint64, 0x1234567)
    P.predict_histogram_batch_dev(n, d_co.ptr, plane, d_par.ptr, d_b.ptr, d_p.ptr, plane, d_h.ptr, d_o.ptr)
    return d_b.get().reshape(n, plane), d_p.get().reshape(n, plane), d_h.get().reshape(n, 10, 1024), d_o.get()


def _fit_sums(torch, P, co, params):
    """(gram [n][3][28], wtw [n][3][21], wtr [n][3][6]) of fit_{value,width}_sums_batch_dev"""
    n, plane = co.reshape(-1, P.num_cells * 512).shape[0], P.num_cells * 512
    d_co, d_par = _dev(torch, co, np.int32), _dev(torch, params, np.float32)
    d_g, d_w, d_r = Buf(torch, n * 84, np.int64, 0x77), Buf(torch, n * 63, np.int64, 0x77), Buf(torch, n * 18, np.float64, -3.0)
    P.fit_value_sums_batch_dev(n, d_co.ptr, plane, d_g.ptr)
    P.fit_width_sums_batch_dev(n, d_co.ptr, plane, d_par.ptr, d_w.ptr, d_r.ptr)
    return d_g.get().reshape(n, 3, 28), d_w.get().reshape(n, 3, 21), d_r.get().reshape(n, 3, 6)


def _fit_chain(torch, P, co):
    """(params [n][2][3][6], out-of-range counts [n]) of fit_params_batch_dev"""
    n, plane = co.reshape(-1, P.num_cells * 512).shape[0], P.num_cells * 512
    d_co = _dev(torch, co, np.int32)
    d_par, d_rng = Buf(torch, n * 36, np.float32, 1.5), Buf(torch, n, np.uint64, 99)
    P.fit_params_batch_dev(n, d_co.ptr, plane, d_par.ptr, d_rng.ptr)
    return d_par.get().reshape(n, 2, 3, 6), d_rng.get()


def _encode(torch, P, case, imgs, route, params_in):
    """the chains: (coefficients or None, params out, K2 outputs or symbol streams, hist, oob)"""
    w, h, c = case.shape
    n_img, plane = case.n_images, P.num_cells * 512
    n = n_img * c
    d_px = _dev(torch, np.concatenate(imgs), np.uint8)
    d_par = _dev(torch, params_in, np.float32)
    d_h, d_o, d_rng = Buf(torch, n * 10 * 1024, np.uint32, 0x3C3C3C3C), Buf(torch, n, np.uint64, 0x1234567), Buf(torch, n, np.uint64, 99)
    if route == "encode_batch":
        d_co = Buf(torch, n * plane, np.int32, 0x5A5A5A5A)
        d_b, d_p = Buf(torch, n * plane, np.uint8, 0xA7), Buf(torch, n * plane, np.int32, 0x5A5A5A5A)
        P.encode_image_batch_dev(n_img, d_px.ptr, w * h * c, d_par.ptr, d_co.ptr, c * plane, d_b.ptr, d_p.ptr, c * plane, d_h.ptr, d_o.ptr, fit=case.fit,
                                 d_fit_out_of_range=d_rng.ptr)
        out = (d_co.get().reshape(n_img, c, P.num_cells, 512), d_b.get().reshape(n, plane), d_p.get().reshape(n, plane))
    else:
        ns = P.num_some
        d_co = Buf(torch, n * plane, np.int32, 0x5A5A5A5A) if route == "symbols_words" else None
        d_w = Buf(torch, n * plane, np.uint16, 0xEEEE) if route != "symbols_direct" else None
        d_st = Buf(torch, n * ns, np.uint16, 0xFFFF)
        P.encode_symbols_batch_dev(n_img, d_px.ptr, w * h * c, QI, case.fit, d_par.ptr, d_co.ptr if d_co else 0, c * plane, d_w.ptr if d_w else 0, c * plane,
                                   d_st.ptr, c * ns, d_h.ptr, d_o.ptr, d_rng.ptr)
        out = (d_co.get().reshape(n_img, c, P.num_cells, 512) if d_co else None, d_st.get().reshape(n_img, c, ns))
        if d_w:
            d_w.get()  # (guards)
    return out, d_par.get().reshape(n, 2, 3, 6), d_h.get().reshape(n, 10, 1024), d_o.get(), d_rng.get()


def _interlude(torch, P, case, co, params):
    """a K2 and a K4 launch of another plane count on the same plan (the accumulators, serial numbers and tickets carry over); returns the W^T r of its
    plane 0 (the case's plane 0)"""
    flat = co.reshape(-1, P.num_cells * 512)
    n = 1 if flat.shape[0] > 1 else 2
    planes = np.stack([flat[min(k, flat.shape[0] - 1)] for k in range(n)])
    if n == 2:
        planes[1] = np.roll(planes[1], 512)  # another plane: the cells' coefficients shifted by one cell
    par = np.concatenate([params.reshape(-1, 2, 3, 6)] * 2)[:n]
    _run_predict(torch, P, case, planes, par)
    _, _, wtr = _fit_sums(torch, P, planes, par)
    return wtr[0]


def _run_case(torch, oracle, P, case):
    """everything the case's route returns, checked against the references; returns what the repeat must reproduce"""
    w, h, c = case.shape
    planes = case.n_planes
    params = _params(case, planes)
    res = {}
    if case.route in ("predict", "predict_assume", "predict_pp3"):
        co = _coefs(oracle, case)
        if case.inexact:
            co = _inject(co, case.inexact, case.seed)
        want = _k2_expect(oracle, case, co, params)
        if case.route == "predict_pp3":
            vp, wp, b, p, hist, oob = P.predict_image(co[0], fit=False, value_params=params[:, 0], width_params=params[:, 1])
            got = (b.reshape(c, -1), p.reshape(c, -1), hist, oob)
        else:
            if case.route == "predict_assume":
                P.assume_forward_coefficients(True)
            got = _run_predict(torch, P, case, co, params)
        _check_k2(case, got, want)
        if case.inexact:
            assert all(int(o) > 0 for _, _, _, o in want), "the injected values should fall outside the alphabet"
        res["k2"] = got
        return res, co, params
    if case.route == "fit_sums":
        co = _coefs(oracle, case)
        gram, wtw, wtr = _fit_sums(torch, P, co, params)
        F = P.num_cells
        rows = np.array([F * 256, F * 128, F * 128], np.uint64)
        for i in range(case.n_images):
            W = _wavelet(oracle, case, co[i])
            for ch in range(c):
                k = i * c + ch
                nv = W.neighbour_values(ch)
                wg, ww, _ = cpu_fit_sums(oracle, W, ch, params[k, 0], nv)
                assert np.array_equal(gram[k], np.stack([wg[g][IU7] for g in range(3)])), (case.id, k, "gram")
                assert np.array_equal(wtw[k], np.stack([ww[g][IU6] for g in range(3)])), (case.id, k, "wtw")
                xw, xfixed, xr, n_sat = _exact_width(case, W, ch, k, P, params[k, 0], nv)
                assert np.array_equal(xw, ww) and n_sat == 0, (case.id, k, "restated wtw")
                assert np.array_equal(wtr[k].view(np.uint64), xr.view(np.uint64)), (case.id, k, "wtr", (np.round(wtr[k] * 2.0 ** 20).astype(np.int64) - xfixed.astype(np.int64)).tolist())
            W.close()
        import frave_amd as fa

        d_g, d_w, d_r = _dev(torch, gram, np.int64), _dev(torch, wtw, np.int64), _dev(torch, wtr, np.float64)
        d_par = Buf(torch, planes * 36, np.float32, 1.5)
        P.fit_value_params_batch_dev(planes, d_g.ptr, d_par.ptr)
        P.fit_width_params_batch_dev(planes, d_w.ptr, d_r.ptr, d_par.ptr)
        got = d_par.get().reshape(planes, 2, 3, 6)
        for k in range(planes):
            assert np.array_equal(got[k, 0].view(np.uint32), fa.fit_value_params(gram[k]).view(np.uint32)), (case.id, k, "solve: value")
            assert np.array_equal(got[k, 1].view(np.uint32), fa.fit_width_params(wtw[k], wtr[k], rows).view(np.uint32)), (case.id, k, "solve: width")
        res.update(gram=gram, wtw=wtw, wtr=wtr.view(np.uint64), params=got.view(np.uint32))
        if case.inexact:
            res["range"] = _fit_chain(torch, P, _inject(co, case.inexact, case.seed))[1]
        return res, co, params
    if case.route == "fit_chain":
        co = _coefs(oracle, case)
        got, rng = _fit_chain(torch, P, co)
        assert (rng == 0).all(), (case.id, rng)
        _check_fitted_params(oracle, case, co, got, P)
        res.update(params=got.view(np.uint32))
        if case.inexact:
            res["range"] = _fit_chain(torch, P, _inject(co, case.inexact, case.seed))[1]
        return res, co, params
    # the encode chains
    imgs = _images(case)
    co = _coefs(oracle, case)
    out, par, hist, oob, rng = _encode(torch, P, case, imgs, case.route, params)
    if not case.fit:
        assert np.array_equal(par, params)
    par = par if case.fit else params
    if out[0] is not None:
        assert np.array_equal(out[0], co), (case.id, "K1 coefficients")
    if case.fit:
        assert (rng == 0).all(), (case.id, rng)
        _check_fitted_params(oracle, case, co, par, P)
    if case.route == "encode_batch":
        want = _k2_expect(oracle, case, co, par)
        _check_k2(case, (out[1], out[2], hist, oob), want)
    else:
        for i, img in enumerate(imgs):
            wsym, whist, woob = _oracle_symbols(oracle, img, w, h, c, QI, False, par[i * c : (i + 1) * c], ORDER[id(P)])
            assert np.array_equal(hist[i * c : (i + 1) * c], whist), (case.id, i, "histograms")
            assert np.array_equal(oob[i * c : (i + 1) * c].astype(np.int64), woob), (case.id, i, "out of alphabet")
            for ch in range(c):
                if woob[ch] == 0:
                    assert np.array_equal(out[1][i, ch], wsym[ch]), (case.id, i, ch, int((out[1][i, ch] != wsym[ch]).sum()))
    res.update(params=par.view(np.uint32), hist=hist, oob=oob, out=[o for o in out if o is not None])
    return res, co, par


ORDER = {}


EXACT = {}  # (case id, plane, value parameters' bytes) -> fit_ref.oracle_width_sums: a case runs up to three times on the same inputs


def _exact_width(case, W, ch, k, P, vp, nv=None):
    key = (case.id, k, np.asarray(vp, np.float32).tobytes())
    if key not in EXACT:
        EXACT[key] = fit_ref.oracle_width_sums(W, ch, P, vp, nv)
    return EXACT[key]


def _check_fitted_params(oracle, case, co, par, P):
    """the parameters of the device fit = the host solves of sums that involve no GPU code, bit for bit: the value parameters of the numpy Gram sums, the
    width parameters of the restated W^T W and W^T r (tests/fit_ref.py) for those value parameters"""
    import frave_amd as fa

    c = case.shape[2]
    F = P.num_cells
    rows = np.array([F * 256, F * 128, F * 128], np.uint64)
    for i in range(co.shape[0]):
        W = _wavelet(oracle, case, co[i])
        for ch in range(c):
            k = i * c + ch
            nv = W.neighbour_values(ch)
            wg, ww, _ = cpu_fit_sums(oracle, W, ch, np.zeros((3, 6), np.float32), nv)
            want = fa.fit_value_params(np.stack([wg[g][IU7] for g in range(3)]))
            assert np.array_equal(par[k, 0].view(np.uint32), want.view(np.uint32)), (case.id, i, ch, "value parameters")
            xw, _, xr, n_sat = _exact_width(case, W, ch, k, P, want, nv)
            assert n_sat == 0 and np.array_equal(xw, ww)
            want = fa.fit_width_params(np.stack([xw[g][IU6] for g in range(3)]), xr, rows)
            assert np.array_equal(par[k, 1].view(np.uint32), want.view(np.uint32)), (case.id, i, ch, "width parameters")
        W.close()


def _same(a, b, where):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{k}]")
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), where


def _grid_free(res):
    """what must not depend on the grid: the parameters' and W^T r's bits, the out-of-range counts"""
    return {k: res[k] for k in ("params", "wtr", "range") if k in res}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_predict_walk(ctx, oracle, case):
    import torch

    P = _plan(ctx, case)
    if case.route.startswith("symbols"):
        ORDER[id(P)] = P.set_stream_order()
    first, co, params = _run_case(torch, oracle, P, case)
    wtr0 = _interlude(torch, P, case, co, params)
    if case.route == "predict_assume":
        P.assume_forward_coefficients(True)
    second, _, _ = _run_case(torch, oracle, P, case)
    _same(first, second, case.id + " (repeat)")
    if "wtr" in first and case.n_planes == 1:  # plane 0 of a two-plane launch
        assert np.array_equal(wtr0.view(np.uint64), first["wtr"][0]), (case.id, "W^T r inside a two-plane launch")
    if "range" in first:
        assert (first["range"] > 0).all(), (case.id, first["range"])
    if case.pinned and _grid_free(first):  # the same on a default plan, bit for bit
        D = _plan(ctx, case, pinned=False)
        if case.route.startswith("symbols"):
            ORDER[id(D)] = D.set_stream_order()
        ref, _, _ = _run_case(torch, oracle, D, case)
        _same(_grid_free(first), _grid_free(ref), case.id + " (default plan)")
        ORDER.pop(id(D), None)
        D.close()
    ORDER.pop(id(P), None)
    P.close()
