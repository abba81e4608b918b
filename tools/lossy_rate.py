"""Rate and distortion of lossy coding against quality, for the synthetic generators of tests/common.py (noise, smooth, const) at C = 1 and 3.

Each image goes through the device chain (fri_hip_encode_image_symbols with fitted parameters, the quality's matrix) and the host emitter (the quality
field set): bits per pixel of the .frv. PSNR: fri_hip_measure_distortion_dev of K1 with the quality's matrix against the source, midpoint dequantiser,
pooled over the channels. Synthetic images only - natural photographs are not measured.

usage: python3 tools/lossy_rate.py [width = 1024] [height = 768] [out = profiles/lossy_rate.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import frave_amd  # noqa: E402
import frave_amd.emit as emit  # noqa: E402
from frave_amd.api import DEQUANT_MIDPOINT  # noqa: E402
from tests.common import gen_image  # noqa: E402

w = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
h = int(sys.argv[2]) if len(sys.argv) > 2 else 768
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "lossy_rate.txt")
QUALITIES = (1, 25, 50, 75, 90, 99, 100)
ctx = frave_amd.Context(0)
lines = [f"# tools/lossy_rate.py {w} {h}: bits per pixel (.frv, device chain + host emitter) / PSNR dB (midpoint dequantiser) against quality; 100 = lossless",
         "| image | C | " + " | ".join(f"q={q}" for q in QUALITIES) + " |", "|---|---|" + "---|" * len(QUALITIES)]
for c in (1, 3):
    P = frave_amd.Plan(ctx, w, h, c)
    P.set_stream_order()
    P.set_dequantiser(DEQUANT_MIDPOINT)
    d_co = torch.empty(P.coef_count, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for kind in ("noise", "smooth", "const"):
        img = gen_image(kind, w, h, c, 1)
        d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
        cells = []
        for q in QUALITIES:
            qm = frave_amd.quality_matrix(q)
            sym, vp, wp, hist, oob = P.encode_image_symbols(img, qm, fit=True)
            frv = emit.encode_image_from_streams(w, h, sym, hist, vp, wp, quality=q if q < 100 else 0)
            P.transform_quant_dev(d_px.data_ptr(), d_co.data_ptr(), qm)
            P.measure_distortion_dev(d_co.data_ptr(), d_px.data_ptr(), d_out.data_ptr(), qm)
            torch.cuda.synchronize()
            db = frave_amd.distortion_psnr(d_out.cpu().numpy().astype(np.uint64), c)
            cells.append(f"{8.0 * len(frv) / (w * h):.3f} / {'inf' if db == float('inf') else f'{db:.1f}'}")
        lines.append(f"| {kind} | {c} | " + " | ".join(cells) + " |")
        print(lines[-1], flush=True)
    P.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
