"""Random-shape parity sweep of K1 / K2 / K3 / K4 against the CPU oracle (GPU box), and on about half the cases the lossy paths (colour transform,
dequantisers, quality matrices, MEASURE), and on about half K2 / K4 on a random pinned grid. Complements tests/test_gpu_parity.py, whose shapes are fixed. usage: fuzz_parity.py [n_cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import frave_amd
from oracle import fri_oracle as O
from tests import fit_ref
from tests.common import gen_image, random_params
from tests.instance_cases import knobs
from tests.oracle_ref import numpy_measure, oracle_coefficients, oracle_owned, oracle_raster


def lossy_checks(ctx, img, w, h, c, rng):
    """a colour transform (3 channels), a dequantiser and a quality drawn from rng: K1 against the oracle on rct(img), K3 against the oracle's raster of the
    numpy-dequantised oracle coefficients, MEASURE against numpy's sums over that raster and the oracle's covered pixels. Returns the names of the mismatches."""
    rct = c == 3 and rng.random() < 0.5
    mode = int(rng.integers(0, 3))  # reference division, multiply, midpoint
    quality = int(rng.integers(1, 100))
    qm = frave_amd.quality_matrix(quality)
    P = frave_amd.Plan(ctx, w, h, c)
    if rct:
        P.set_colour_transform(1)
    P.set_dequantiser(mode)
    tag = f"(rct={int(rct)} dequantiser={mode} quality={quality})"
    msgs = []
    want = oracle_coefficients(O, img, w, h, c, qm, rct)
    if not np.array_equal(P.transform_quant(img, qm), want):
        msgs.append("K1-lossy" + tag)
    owned = oracle_owned(O, w, h, c)
    recon = oracle_raster(O, want, qm, mode, w, h, c, rct, owned)
    if not np.array_equal(P.inverse_transform(want, qm), recon):
        msgs.append("K3-lossy" + tag)
    d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
    d_co = torch.from_numpy(want.reshape(-1).copy()).cuda()
    d_out = torch.full((2 * c + 1,), 77, dtype=torch.int64, device="cuda")
    P.measure_distortion_dev(d_co.data_ptr(), d_px.data_ptr(), d_out.data_ptr(), qm)
    torch.cuda.synchronize()
    if [int(x) for x in d_out.cpu().numpy().astype(np.uint64)] != numpy_measure(recon, img, owned, c):
        msgs.append("MEASURE" + tag)
    P.close()
    return msgs


def run(n_cases, seed, ctx=None):
    """n_cases random (shape, content, channel count, quantiser, parameters) cases; returns the number of mismatching ones."""
    rng = np.random.default_rng(seed)
    lossy_rng = np.random.default_rng([seed, 1])  # the lossy checks draw from a stream of their own: the cases rng draws stay those of earlier sweeps
    grid_rng = np.random.default_rng([seed, 2])  # and so do the K2 / K4 grid knobs
    ctx = ctx or frave_amd.Context(0)
    bad = chains = lossy = 0
    t0 = time.time()
    for case in range(n_cases):
        kind = ["noise", "smooth", "const"][int(rng.integers(0, 3))]
        if rng.random() < 0.3:  # thin / tiny images
            w, h = int(rng.integers(1, 60)), int(rng.integers(1, 900))
            if rng.random() < 0.5:
                w, h = h, w
        elif os.environ.get("FUZZ_LARGE") == "1":  # mid-size and large planes (round 5): other share counts, band layouts and list sizes than the small shapes reach
            w, h = int(rng.integers(1400, 6000)), int(rng.integers(900, 4500))
        else:
            w, h = int(rng.integers(46, 1400)), int(rng.integers(46, 900))
        c = 1 if rng.random() < 0.5 else 3
        img = gen_image(kind, w, h, c, int(rng.integers(0, 1 << 30)))
        grid = None
        if grid_rng.random() < 0.5:  # about half the plans launch K2 / K4 on a pinned grid: other workgroup counts, tile walks and K4 splits
            hist = int(grid_rng.integers(1, 40)) * (16 if grid_rng.random() < 0.5 else 1)
            grid = {"FRI_HIP_TUNING": "1", "FRI_HIP_PRED_BLOCKS": str(int(grid_rng.integers(1, 300))), "FRI_HIP_HIST_BLOCKS": str(hist),
                    "FRI_HIP_K4_OLDER_EIGHTHS": str(int(grid_rng.integers(0, 9)))}
        try:
            with knobs(grid):
                P = frave_amd.Plan(ctx, w, h, c)
        except frave_amd.api.FriHipError as e:
            print(f"case {case}: {w}x{h}x{c}: plan error {e}")
            continue
        if os.environ.get("FUZZ_TUNE") == "1" and case % 2 == 0:  # every other plan measures its forward tiling first (round 5): any winner must give the oracle's coefficients
            P.tune_forward(8)
        W = O.Wavelet(img, h, w, c)
        q = np.ones(32, np.int32)
        if rng.random() < 0.3:
            q[:10] = rng.integers(1, 9, 10)
        co = P.transform_quant(img, q)
        W.quantize(q)
        ok = np.array_equal(co, W.coefficients())
        msgs = [] if ok else ["K1"]
        ch = int(rng.integers(0, c))
        vp, wp = random_params(int(rng.integers(0, 1000)))
        b, p, hist, oob = P.predict_histogram(co, ch, vp, wp)
        wb, wpred, whist, woob = W.predict(ch, vp, wp)
        if not (np.array_equal(b, wb) and np.array_equal(p, wpred) and np.array_equal(hist, whist) and oob == woob):
            msgs.append("K2")
        back = P.inverse_transform(co)  # the oracle's inverse takes the coefficients as they are (identity dequantiser)
        if not np.array_equal(back, W.to_raster()):
            msgs.append("K3")
        # nine images in ONE launch: the merged batch shares of the plan
        d_px = torch.from_numpy(np.tile(img.reshape(1, -1), (9, 1))).cuda()
        d_co = torch.empty((9, P.coef_count), dtype=torch.int32, device="cuda")
        P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qmatrix=q, n_images=9, pixel_stride=P.pixel_bytes, coef_stride=P.coef_count)
        torch.cuda.synchronize()
        if not bool((d_co.cpu().numpy().reshape(9, -1) == co.reshape(1, -1)).all()):
            msgs.append("K1-batch")
        # the chain with the fit (device-side solves) and the symbol stream route on the same image: the fitted parameters equal the host solves of the
        # stage-by-stage sums bit for bit, the scan with them equals the oracle's, the stream is the gather of the array route's outputs
        if P.num_some > 0 and not (kind == "const" and rng.random() < 0.5):
            try:
                co2, vpf, wpf, b2, p2, h2, oob2 = P.encode_image(img, q, fit=True)
                chains += 1
                if not np.array_equal(co2, co):
                    msgs.append("chain-K1")
                ok_fit = True
                for cc in range(c):
                    gram = P.fit_value_sums(co, cc)
                    iu = np.triu_indices(7)
                    vh = frave_amd.api.fit_value_params(np.stack([gram[g][iu] for g in range(3)]))
                    wtw, wtr, rows = P.fit_width_sums(co, cc, vh)
                    # W^T W and W^T r against their restatement from the oracle's neighbour values (tests/fit_ref.py), bit for bit
                    xw, xfixed, xr, n_sat = fit_ref.oracle_width_sums(W, cc, P, vh)
                    if not (np.array_equal(wtw, xw) and n_sat == 0 and np.array_equal(wtr.view(np.uint64), xr.view(np.uint64))):
                        units = (np.round(wtr * 2.0 ** 20).astype(np.int64) - xfixed.astype(np.int64)).tolist()
                        msgs.append(f"K4 width sums ch{cc} (value params {vh.tolist()}, saturated {n_sat}, W^T r off by {units} fixed-point units)")
                    iu6 = np.triu_indices(6)
                    wh = frave_amd.api.fit_width_params(np.stack([wtw[g][iu6] for g in range(3)]), wtr, rows)
                    ok_fit = ok_fit and np.array_equal(vh.view(np.uint32), vpf[cc].view(np.uint32)) and np.array_equal(wh.view(np.uint32), wpf[cc].view(np.uint32))
                if not ok_fit:
                    msgs.append("fit(device solve != host solve)")
                if np.isfinite(vpf).all() and np.isfinite(wpf).all():
                    wb2, wp2, wh2, wo2 = W.predict(ch, vpf[ch].reshape(-1), wpf[ch].reshape(-1))
                    if not (np.array_equal(b2[ch], wb2) and np.array_equal(p2[ch], wp2) and np.array_equal(h2[ch], wh2) and int(oob2[ch]) == wo2):
                        msgs.append("chain-K2")
                order = P.set_stream_order()
                sym, vps, wps, hs, oobs = P.encode_image_symbols(img, q, fit=True)
                if not (np.array_equal(vps.view(np.uint32), vpf.view(np.uint32)) and np.array_equal(wps.view(np.uint32), wpf.view(np.uint32)) and np.array_equal(hs, h2)):
                    msgs.append("symbols-route(params/hist)")
                if int(oob2.sum()) == 0:
                    for cc in range(c):
                        d = (co[cc].reshape(-1)[order].astype(np.int64) - p2[cc].reshape(-1)[order].astype(np.int64)).astype(np.int32)
                        ref = (b2[cc].reshape(-1)[order].astype(np.uint32) << 10 | (((d.astype(np.uint32) << 1) ^ (d >> 31).astype(np.uint32)) & 1023)).astype(np.uint16)
                        if not np.array_equal(sym[cc], ref):
                            msgs.append(f"K5 ch{cc}")
            except frave_amd.api.FriHipError as e:
                msgs.append(f"chain error {e}")
        if lossy_rng.random() < 0.5:
            lossy += 1
            msgs += lossy_checks(ctx, img, w, h, c, lossy_rng)
        if msgs:
            bad += 1
            print(f"case {case}: {w}x{h}x{c} {kind} q={q[:10].tolist()} grid={grid}: MISMATCH in {msgs}", flush=True)
        if (case + 1) % (10 if os.environ.get("FUZZ_LARGE") == "1" else 250) == 0:  # a sign of life for long runs (a silent command is taken to be hung after a few minutes)
            print(f"... {case + 1} cases, {bad} mismatching, {time.time() - t0:.0f} s", flush=True)
        P.close()
        W.close()
    print(f"{n_cases} cases ({chains} with the fitted chain and the symbol stream route, {lossy} with the lossy checks), {bad} mismatching, {time.time() - t0:.0f} s")
    return bad


if __name__ == "__main__":
    sys.exit(1 if run(int(sys.argv[1]) if len(sys.argv) > 1 else 100, int(sys.argv[2]) if len(sys.argv) > 2 else 1) else 0)
