"""What lossy coding to a target size costs on the device: the rate kernel (fri_hip_estimate_size_dev: a memset, K6 with one workgroup per (plane,
context), the bytes kernel) for one image of C = 1 and C = 3 and for a batch of 8 RGB images, and fri_hip_search_quality_for_size_dev at 4096^2 C = 1 / 3
and 16384^2 C = 1.

The rate kernel: histograms of the chain at quality 50 of a smooth + noise image (fri_hip_encode_image_batch_dev with the fit), copied into 64 rotating
HBM slots, timed with events around n launches; medians over the rounds in microseconds per call. The search is synchronous (one read-back per probe):
wall-clock time per call with the budget of quality 50's estimate.

usage: python3 tools/rate_time.py [launches per measurement = 400] [rounds = 5] [out = profiles/rate_time.txt]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import frave_amd  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rate_time.txt")
ctx = frave_amd.Context(0)
s = torch.cuda.current_stream()
lines = [f"# tools/rate_time.py {n} {rounds}: medians over {rounds} rounds, microseconds per call"]
SLOTS = 64


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for i in range(launches):
        fn(i)
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def smooth_noise(size, c, seed=5):
    """a smooth gradient with noise on top (+-8), on the device"""
    y = torch.arange(size, device="cuda", dtype=torch.float32).view(-1, 1, 1)
    x = torch.arange(size, device="cuda", dtype=torch.float32).view(1, -1, 1)
    ch = torch.arange(c, device="cuda", dtype=torch.float32).view(1, 1, -1)
    base = 128 + 90 * torch.sin(x / 97.0 + ch) * torch.cos(y / 131.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    noise = torch.randint(-8, 9, (size, size, c), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    return (base + noise).clamp(0, 255).to(torch.uint8).view(-1)


def chain_hist(plan, img, quality):
    """the chain's histograms [C][10][1024] (int32 view) and out-of-alphabet counts of one image, on the device"""
    c = plan.channels
    d_co = torch.empty(plan.coef_count, dtype=torch.int32, device="cuda")
    d_params = torch.zeros(c * 36, dtype=torch.float32, device="cuda")
    d_hist = torch.empty(c * 10 * 1024, dtype=torch.int32, device="cuda")
    d_oob = torch.empty(c, dtype=torch.int64, device="cuda")
    plan.encode_image_batch_dev(1, img.data_ptr(), 0, d_params.data_ptr(), d_co.data_ptr(), 0, 0, 0, 0, d_hist.data_ptr(), d_oob.data_ptr(),
                                qmatrix=frave_amd.quality_matrix(quality), fit=True, stream=s.cuda_stream)
    torch.cuda.synchronize()
    return d_hist, d_oob


# the rate kernel
for c, batch in ((1, 1), (3, 1), (3, 8)):
    plan = frave_amd.Plan(ctx, 4096, 4096, c)
    hists, oobs = [], []
    for k in range(batch):
        h, o = chain_hist(plan, smooth_noise(4096, c, seed=5 + k), 50)
        hists.append(h), oobs.append(o)
    one_h, one_o = torch.cat(hists), torch.cat(oobs)
    d_hist = one_h.repeat(SLOTS).view(SLOTS, -1).contiguous()
    d_oob = one_o.repeat(SLOTS).view(SLOTS, -1).contiguous()
    d_bytes = torch.empty((SLOTS, batch), dtype=torch.int64, device="cuda")

    def rate(i):
        k = i % SLOTS
        plan.estimate_size(d_hist[k].data_ptr(), d_oob[k].data_ptr(), stream=s.cuda_stream, n_images=batch, d_bytes=d_bytes[k].data_ptr())

    timed(rate, SLOTS)  # spin-up
    ts = [timed(rate, n) for _ in range(rounds)]
    torch.cuda.synchronize()
    est = d_bytes[0].cpu().tolist()
    m = statistics.median(ts)
    lines.append(f"rate kernel C={c} x {batch} image{'s' if batch > 1 else ''}  {m:8.2f} us per call  ({m / batch:.2f} us per image; runs {min(ts):.2f}-{max(ts):.2f};"
                 f" 4096^2 quality-50 histograms, estimate {est[0]} bytes)")
    print(lines[-1], flush=True)
    del plan, d_hist, d_oob, d_bytes, hists, oobs
    torch.cuda.empty_cache()

# the search
for size, c in ((4096, 1), (4096, 3), (16384, 1)):
    plan = frave_amd.Plan(ctx, size, size, c)
    img = smooth_noise(size, c)
    h, o = chain_hist(plan, img, 50)
    budget = plan.estimate_size(h.cpu().numpy().view("uint32"), o.cpu().numpy().view("uint64"))
    del h, o
    plan.search_quality_for_size(img.data_ptr(), budget, stream=s.cuda_stream)  # spin-up (the probes' buffers)
    ts = []
    for r in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q, est = plan.search_quality_for_size(img.data_ptr(), budget, stream=s.cuda_stream)
        ts.append((time.perf_counter() - t0) * 1e6)
    m = statistics.median(ts)
    lines.append(f"search {size}^2 C={c}  {m:10.1f} us per call  (7 probes: {m / 7:.1f} us each; budget {budget} bytes -> quality {q}, estimate {est};"
                 f" runs {min(ts):.1f}-{max(ts):.1f})")
    print(lines[-1], flush=True)
    del plan, img
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
