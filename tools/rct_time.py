"""What the reversible colour transform (fri_hip_plan_set_colour_transform) costs K1 and K3 on RGB images, and what it saves in the file.

K1: fri_hip_time_transform_quant_dev (bench.py's loop) over rotating slots - 24 at 4096^2 (1.2 GB of pixels, far beyond the 256 MiB Infinity Cache, as in
tools/k1_slots.py); at 16384^2 one image alone is 805 MB of pixels and 3.9 GB of coefficients, so 3 slots already read every input from HBM. K3: the inverse
entry point on the same rotation, timed with events around n launches. Plain and RCT in interleaved rounds in one process; medians in microseconds per launch.
Then the .frv sizes of synthetic images through the device chain (fitted parameters) and the host emitter, without and with the flag.

usage: python3 tools/rct_time.py [launches per measurement = 200] [rounds = 5]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import frave_amd  # noqa: E402
import frave_amd.emit as emit  # noqa: E402
from frave_amd.api import COLOUR_NONE, COLOUR_RCT  # noqa: E402
from tests.common import gen_image  # noqa: E402
from tests.test_rct_host import correlated_image  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ctx = frave_amd.Context(0)
s = torch.cuda.current_stream()


def time_inverse(plan, d_co, d_px, slots, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(launches):
        k = i % slots
        plan.inverse_transform_dev(d_co[k].data_ptr(), d_px[k].data_ptr(), stream=s.cuda_stream)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


for size, slots in ((4096, 24), (16384, 3)):
    plan = frave_amd.Plan(ctx, size, size, 3)
    d_px = torch.randint(0, 256, (slots, plan.pixel_bytes), dtype=torch.uint8, device="cuda")
    d_co = torch.empty((slots, plan.coef_count), dtype=torch.int32, device="cuda")
    d_out = torch.empty_like(d_px)
    launches = max(slots, n if size == 4096 else n // 8)
    plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, 4 * launches, stream=s.cuda_stream)  # spin-up
    res = {(k, m): [] for k in ("K1", "K3") for m in (COLOUR_NONE, COLOUR_RCT)}
    for r in range(rounds):
        for m in (COLOUR_NONE, COLOUR_RCT):
            plan.set_colour_transform(m)
            plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, 2 * slots, stream=s.cuda_stream)
            res["K1", m].append(plan.time_transform_quant_dev(slots, d_px.data_ptr(), plan.pixel_bytes, d_co.data_ptr(), plan.coef_count, launches, stream=s.cuda_stream))
            # d_co now holds this mode's coefficients of every slot: K3 inverts them (and must give the pixels back)
            time_inverse(plan, d_co, d_out, slots, slots)
            res["K3", m].append(time_inverse(plan, d_co, d_out, slots, launches))
            assert torch.equal(d_out, d_px), "round trip"
    for k in ("K1", "K3"):
        a, b = statistics.median(res[k, COLOUR_NONE]), statistics.median(res[k, COLOUR_RCT])
        print(f"{k} {size}x{size} RGB, {slots} slots, {launches} launches: plain {a:.2f} us, RCT {b:.2f} us ({100 * (b / a - 1):+.1f} %); "
              f"rounds plain {' '.join(f'{x:.2f}' for x in res[k, COLOUR_NONE])} / RCT {' '.join(f'{x:.2f}' for x in res[k, COLOUR_RCT])}", flush=True)
    del d_px, d_co, d_out
    torch.cuda.empty_cache()
    plan.close()


def frv_size(img, mode):
    h, w, c = img.shape
    plan = frave_amd.Plan(ctx, w, h, c)
    plan.set_colour_transform(mode)
    coefs, vp, wp, bucket, pred, hist, oob = plan.encode_image(img, fit=True)
    assert not oob.any()
    frv = emit.encode_image(w, h, plan.centers(), coefs, bucket, pred, hist, vp, wp, rct=mode == COLOUR_RCT)
    plan.close()
    return len(frv)


images = {
    "correlated 1024x768 (G texture + noise, R = G + 23, B = G - 31, small noise each)": correlated_image(1024, 768, 7),
    "correlated 256x192 (the host test's image)": correlated_image(256, 192, 7),
    "noise 1024x768 (independent channels)": gen_image("noise", 1024, 768, 3, 1),
    "smooth 1024x768 (gen_image: the same ramp in every channel, independent noise)": gen_image("smooth", 1024, 768, 3, 1),
}
for name, img in images.items():
    a, b = frv_size(img, COLOUR_NONE), frv_size(img, COLOUR_RCT)
    print(f".frv {name}: RGB {a} B, RCT {b} B ({b / a:.3f})", flush=True)
