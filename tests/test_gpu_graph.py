"""HIP-graph capture: the forward kernel alone can be captured and replayed (its launch carries no host-side state); every entry point that
launches the scan (predict + histogram) refuses a capturing stream - its histogram hand-over numbers launches on the host, a replay would reuse a number."""
import ctypes as C

import numpy as np
import pytest

from tests.common import KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, gen_image

pytestmark = pytest.mark.gpu
RELAXED = 2  # hipStreamCaptureModeRelaxed


@pytest.fixture(scope="module")
def ctx():
    import frave_amd as fa

    c = fa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


def test_forward_kernel_replays_from_a_graph(ctx, oracle, hip):
    import torch

    import frave_amd as fa

    w, h, c = 640, 360, 1
    P = fa.Plan(ctx, w, h, c)
    imgs = [gen_image("noise", w, h, c, 40 + k) for k in range(3)]
    d_px = torch.from_numpy(imgs[0].reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), stream=s.cuda_stream)
    graph, ex = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0 and graph.value
    assert hip.hipGraphInstantiate(C.byref(ex), graph, None, None, 0) == 0
    for img in imgs:  # every replay transforms what the pixel buffer holds NOW
        d_px.copy_(torch.from_numpy(img.reshape(-1).copy()))
        d_co.fill_(7)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(ex, sp) == 0
        s.synchronize()
        assert np.array_equal(d_co.cpu().numpy().reshape(c, -1, 512), oracle.Wavelet(img, h, w, c).coefficients())
    hip.hipGraphExecDestroy(ex)
    hip.hipGraphDestroy(graph)
    P.close()


def test_the_scan_refuses_a_capturing_stream(ctx, hip):
    import torch

    import frave_amd as fa

    w, h, c = 320, 200, 1
    P = fa.Plan(ctx, w, h, c)
    F = P.num_cells
    d_px = torch.from_numpy(gen_image("smooth", w, h, c, 3).reshape(-1).copy()).cuda()
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    d_b = torch.empty(F * 512, dtype=torch.uint8, device="cuda")
    d_p = torch.empty(F * 512, dtype=torch.int32, device="cuda")
    d_h = torch.empty(10 * 1024, dtype=torch.int32, device="cuda")
    d_o = torch.empty(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    # once outside any capture: scratch and accumulators exist, the result is the reference for what follows
    P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), stream=s.cuda_stream)
    P.predict_histogram_dev(d_co.data_ptr(), 0, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, d_b.data_ptr(), d_p.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    want = d_h.clone()
    assert int(want.sum()) + int(d_o) == P.num_some
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        with pytest.raises(fa.FriHipError) as e:
            P.predict_histogram_dev(d_co.data_ptr(), 0, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, d_b.data_ptr(), d_p.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), stream=s.cuda_stream)
        assert e.value.code == -1 and "graph" in str(e.value)  # FRI_HIP_ERR_INVALID_ARGUMENT
    finally:
        graph = C.c_void_p()
        hip.hipStreamEndCapture(sp, C.byref(graph))
        if graph.value:
            hip.hipGraphDestroy(graph)
    # the plan is unharmed: the next ordinary launch counts exactly what the first did
    d_h.fill_(99)
    P.predict_histogram_dev(d_co.data_ptr(), 0, KAT_VALUE_PARAMS, KAT_WIDTH_PARAMS, d_b.data_ptr(), d_p.data_ptr(), d_h.data_ptr(), d_o.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert torch.equal(d_h, want)
    P.close()


def _symbol_chain(P, torch, d_px, params, fit, direct, stream):
    """one image through fri_hip_encode_symbols_batch_dev on the compact planes (d_coefs = NULL); the caller's buffers, allocated before any capture"""
    plane, n = P.num_cells * 512, P.num_some
    out = dict(w=torch.full((plane,), 0xEEEE, dtype=torch.uint16, device="cuda"), st=torch.full((n,), 0xFFFF, dtype=torch.uint16, device="cuda"),
               h=torch.full((10, 1024), -1, dtype=torch.int32, device="cuda"), o=torch.full((1,), -1, dtype=torch.int64, device="cuda"),
               r=torch.full((1,), -1, dtype=torch.int64, device="cuda"), par=torch.from_numpy(params.reshape(-1).copy()).cuda())
    torch.cuda.synchronize()

    def run():
        P.encode_symbols_batch_dev(1, d_px.data_ptr(), P.pixel_bytes, None, fit, out["par"].data_ptr(), 0, plane, 0 if direct else out["w"].data_ptr(), plane, out["st"].data_ptr(), n,
                                   out["h"].data_ptr(), out["o"].data_ptr(), out["r"].data_ptr() if fit else None, stream=stream)

    return out, run


def test_a_refused_symbol_chain_leaves_the_graph_empty(ctx, hip):
    # the compact chains refuse a capturing stream before K1 is queued: nothing of them lands in the caller's graph, with the fit or without it
    import torch

    import frave_amd as fa
    from tests.common import random_params

    w, h, c = 320, 200, 1
    d_px = torch.from_numpy(gen_image("smooth", w, h, c, 9).reshape(-1).copy()).cuda()
    vp, wp = random_params(5)
    params = np.stack([np.asarray(vp, np.float32).reshape(3, 6), np.asarray(wp, np.float32).reshape(3, 6)])
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    forms = [(False, True), (True, False)]  # (fit, direct): the stream form without the fit, the node-word form with it
    R = fa.Plan(ctx, w, h, c)  # a plan that never sees a capture
    R.set_stream_order()
    want = []
    for fit, direct in forms:
        out, run = _symbol_chain(R, torch, d_px, params, fit, direct, s.cuda_stream)
        run()
        s.synchronize()
        want.append(out)
    P = fa.Plan(ctx, w, h, c)
    P.set_stream_order()
    chains = [_symbol_chain(P, torch, d_px, params, fit, direct, s.cuda_stream) for fit, direct in forms]
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(sp, RELAXED) == 0
    try:
        for _, run in chains:
            with pytest.raises(fa.FriHipError) as e:
                run()
            assert e.value.code == -1 and "graph" in str(e.value)  # FRI_HIP_ERR_INVALID_ARGUMENT
    finally:
        assert hip.hipStreamEndCapture(sp, C.byref(graph)) == 0
    n_nodes = C.c_size_t(12345)
    rc = hip.hipGraphGetNodes(graph, None, C.byref(n_nodes))
    hip.hipGraphDestroy(graph)
    assert rc == 0 and n_nodes.value == 0
    # outside the capture the same chains compute what the other plan computed
    for (fit, _), (out, run), ref in zip(forms, chains, want):
        run()
        s.synchronize()
        for k in ("st", "h", "o") + (("par", "r") if fit else ()):
            assert torch.equal(out[k], ref[k]), (fit, k)
    P.close()
    R.close()
