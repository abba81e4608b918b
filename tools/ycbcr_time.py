"""What the lossy YCbCr colour transform (fri_hip_plan_set_colour_transform(FRI_HIP_COLOUR_YCBCR)) costs K1, K3 and the searches on RGB images, against plain
RGB and the RCT, and what it gives in bits per pixel at a PSNR.

K1: fri_hip_time_transform_quant_dev (bench.py's loop) over rotating slots, as tools/rct_time.py - 24 at 4096^2, 3 at 16384^2 - with the all-ones matrix.
K3: the inverse entry point with the midpoint dequantiser and quality 75's matrix on the same rotation, and fri_hip_measure_distortion_dev (K3 MEASURE) on
it, timed with events around n launches. The three modes in interleaved rounds in one process; medians in microseconds per launch. The searches
(fri_hip_search_quality_dev at 40 dB, fri_hip_search_quality_for_size_dev at 10 bits per pixel) on a correlated image, wall clock of one call, median of
`rounds`; the RCT refuses both. Then bits per pixel / PSNR (in R, G, B) against quality for synthetic images, RGB and YCbCr rows.

usage: python3 tools/ycbcr_time.py [launches per measurement = 200] [rounds = 5] [out = profiles/ycbcr_time.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import frave_amd  # noqa: E402
import frave_amd.emit as emit  # noqa: E402
from frave_amd.api import COLOUR_NONE, COLOUR_RCT, COLOUR_YCBCR, DEQUANT_MIDPOINT  # noqa: E402
from tests.common import gen_image  # noqa: E402
from tests.test_rct_host import correlated_image  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ycbcr_time.txt")
ctx = frave_amd.Context(0)
s = torch.cuda.current_stream()
MODES = {COLOUR_NONE: "plain", COLOUR_RCT: "RCT", COLOUR_YCBCR: "YCbCr"}
lines = [f"python3 tools/ycbcr_time.py {n} {rounds} (one process; medians of {rounds} interleaved rounds, us per launch unless stated)"]


def emit_line(text):
    lines.append(text)
    print(text, flush=True)


def time_launches(fn, slots, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(launches):
        fn(i % slots)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


q75 = frave_amd.quality_matrix(75)
for size, slots in ((4096, 24), (16384, 3)):
    plan = frave_amd.Plan(ctx, size, size, 3)
    plan.set_dequantiser(DEQUANT_MIDPOINT)
    d_px = torch.randint(0, 256, (slots, plan.pixel_bytes), dtype=torch.uint8, device="cuda")
    d_co = torch.empty((slots, plan.coef_count), dtype=torch.int32, device="cuda")
    d_out = torch.empty_like(d_px)
    d_m = torch.zeros(8, dtype=torch.int64, device="cuda")
    launches = max(slots, n if size == 4096 else n // 8)
    plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, 4 * launches, stream=s.cuda_stream)  # spin-up
    res = {(k, m): [] for k in ("K1", "K3 midpoint", "K3 measure") for m in MODES}
    for r in range(rounds):
        for m in MODES:
            plan.set_colour_transform(m)
            plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, 2 * slots, stream=s.cuda_stream)
            res["K1", m].append(plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, launches,
                                                              stream=s.cuda_stream))
            inv = lambda k: plan.inverse_transform_dev(d_co[k].data_ptr(), d_out[k].data_ptr(), q75, stream=s.cuda_stream)  # noqa: E731
            mea = lambda k: plan.measure_distortion_dev(d_co[k].data_ptr(), d_px[k].data_ptr(), d_m.data_ptr(), q75, stream=s.cuda_stream)  # noqa: E731
            time_launches(inv, slots, slots)
            res["K3 midpoint", m].append(time_launches(inv, slots, launches))
            time_launches(mea, slots, slots)
            res["K3 measure", m].append(time_launches(mea, slots, launches))
    for k in ("K1", "K3 midpoint", "K3 measure"):
        med = {m: statistics.median(res[k, m]) for m in MODES}
        a = med[COLOUR_NONE]
        emit_line(f"{k} {size}x{size} RGB, {slots} slots, {launches} launches: plain {a:.2f} us, RCT {med[COLOUR_RCT]:.2f} us "
                  f"({100 * (med[COLOUR_RCT] / a - 1):+.1f} %), YCbCr {med[COLOUR_YCBCR]:.2f} us ({100 * (med[COLOUR_YCBCR] / a - 1):+.1f} %); rounds "
                  + " / ".join(f"{MODES[m]} " + " ".join(f"{x:.2f}" for x in res[k, m]) for m in MODES))
    # the searches on one correlated image (plain RGB and YCbCr; the RCT refuses them)
    img = correlated_image(size, size, 5) if size == 4096 else np.tile(correlated_image(4096, 4096, 5), (4, 4, 1))
    d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
    for name, fn in (("PSNR search (40 dB)", lambda: plan.search_quality(d_img.data_ptr(), 40.0, stream=s.cuda_stream)),
                     ("size search (10 bpp)", lambda: plan.search_quality_for_size(d_img.data_ptr(), size * size * 10 // 8, stream=s.cuda_stream))):
        got = {}
        for m in (COLOUR_NONE, COLOUR_YCBCR):
            plan.set_colour_transform(m)
            r0 = fn()
            ts = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            got[m] = (statistics.median(ts), r0)
        a, b = got[COLOUR_NONE], got[COLOUR_YCBCR]
        emit_line(f"{name} {size}x{size} correlated: plain {a[0]:.2f} ms -> {a[1]}, YCbCr {b[0]:.2f} ms -> {b[1]} (wall clock per call)")
    del d_px, d_co, d_out, d_img
    torch.cuda.empty_cache()
    plan.close()

# bits per pixel / PSNR (R, G, B) against quality
QUALITIES = (25, 50, 75, 90, 99)
w, h = 1024, 768
emit_line(f"bits per pixel (.frv, device chain + host emitter) / PSNR dB in R, G, B (midpoint dequantiser) against quality, {w}x{h}")
emit_line("| image | mode | " + " | ".join(f"q={q}" for q in QUALITIES) + " |")
emit_line("|---|---|" + "---|" * len(QUALITIES))
images = {"correlated": correlated_image(w, h, 7), "smooth": gen_image("smooth", w, h, 3, 1), "noise": gen_image("noise", w, h, 3, 1)}
for name, img in images.items():
    for m in (COLOUR_NONE, COLOUR_YCBCR):
        P = frave_amd.Plan(ctx, w, h, 3)
        P.set_colour_transform(m)
        P.set_dequantiser(DEQUANT_MIDPOINT)
        P.set_stream_order()
        cells = []
        for q in QUALITIES:
            qm = frave_amd.quality_matrix(q)
            sym, vp, wp, hist, oob = P.encode_image_symbols(img, qm, fit=True)
            frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q, ycbcr=m == COLOUR_YCBCR)
            back = P.inverse_transform(P.transform_quant(img, qm), qm)
            e = back.astype(np.float64) - img.reshape(-1)
            db = 10 * np.log10(255.0 ** 2 / max(float((e * e).mean()), 1e-30))
            cells.append(f"{8.0 * len(frv) / (w * h):.3f} / {db:.1f}")
        P.close()
        emit_line(f"| {name} | {'RGB' if m == COLOUR_NONE else 'YCbCr'} | " + " | ".join(cells) + " |")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
