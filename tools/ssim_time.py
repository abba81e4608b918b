"""What SSIM costs on the device: K7 (fri_hip_measure_ssim_dev) at 4096^2 C = 1 and 3 and at 16384^2 C = 1, and the wall time of
fri_hip_search_quality_ssim_dev next to fri_hip_search_quality_dev on the same 4096^2 image.

K7: each shape runs in a child process of its own under `rocprofv3 --kernel-trace --stats`; the child launches K7 on pairs (a smooth image with noise,
and a copy with +-3 of noise on top) in enough rotating HBM slots that the pairs do not fit in the 256 MiB Infinity Cache, and the kernel statistics of
`ssim_kernel` are reported with the byte floor 2 W H C / 8 TB/s. The searches are synchronous (one read-back per probe): wall-clock time per call,
median over the rounds, the two searches alternating.

usage: python3 tools/ssim_time.py [launches per shape = 200] [rounds = 5] [out = profiles/ssim_time.txt]
       python3 tools/ssim_time.py --k7 SIZE C LAUNCHES        (the child: one shape's launches, nothing printed but a line)"""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K7_SHAPES = ((4096, 1), (4096, 3), (16384, 1))
HBM_BYTES_PER_S = 8e12


def smooth_noise(torch, size, c, seed, amp=8):
    """a smooth gradient with noise on top (+-amp), on the device"""
    y = torch.arange(size, device="cuda", dtype=torch.float32).view(-1, 1, 1)
    x = torch.arange(size, device="cuda", dtype=torch.float32).view(1, -1, 1)
    ch = torch.arange(c, device="cuda", dtype=torch.float32).view(1, 1, -1)
    base = 128 + 90 * torch.sin(x / 97.0 + ch) * torch.cos(y / 131.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    noise = torch.randint(-amp, amp + 1, (size, size, c), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    return (base + noise).clamp(0, 255).to(torch.uint8).view(-1)


def k7_child(size, c, launches):
    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    plan = frave_amd.Plan(ctx, size, size, c)
    n = size * size * c
    slots = max(1, -(-(512 << 20) // (2 * n)))  # at least 512 MiB of pairs: every launch reads HBM
    a = [smooth_noise(torch, size, c, 5 + k) for k in range(slots)]
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    b = [(x.to(torch.int32) + torch.randint(-3, 4, (n,), device="cuda", generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8) for x in a]
    d_out = torch.empty((slots, c + 1), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    for i in range(slots + launches):  # the first `slots` launches: spin-up
        k = i % slots
        plan.measure_ssim_dev(a[k].data_ptr(), b[k].data_ptr(), d_out[k].data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    ssim, _ = frave_amd.ssim_of(d_out[0].cpu().numpy(), c)
    print(f"k7 {size}^2 C={c}: {slots} slots, SSIM of slot 0 {ssim:.6f}")


def profile_k7(size, c, launches):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "k7", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--k7", str(size), str(c), str(launches)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        note = [ln for ln in r.stdout.splitlines() if ln.startswith("k7 ")]
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "ssim_kernel" in row["Name"]:
                    return row, note[0] if note else ""
    raise RuntimeError("no ssim_kernel row in the kernel statistics")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--k7":
        k7_child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
        return
    launches = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ssim_time.txt")
    lines = [f"# tools/ssim_time.py {launches} {rounds}"]
    for size, c in K7_SHAPES:  # each in a child process of its own, before this process opens the GPU
        row, note = profile_k7(size, c, launches)
        avg, floor = float(row["AverageNs"]) / 1e3, 2 * size * size * c / HBM_BYTES_PER_S * 1e6
        lines.append(f"K7 {size}^2 C={c}  {avg:8.2f} us per launch (rocprofv3 --kernel-trace --stats: {row['Calls']} calls, min {float(row['MinNs']) / 1e3:.2f}, "
                     f"max {float(row['MaxNs']) / 1e3:.2f}; {row['Name'][:40]}); byte floor {floor:.1f} us at 8 TB/s -> {avg / floor:.2f}x; {note}")
        print(lines[-1], flush=True)

    import torch

    import frave_amd

    ctx = frave_amd.Context(0)
    for c in (1, 3):
        plan = frave_amd.Plan(ctx, 4096, 4096, c)
        img = smooth_noise(torch, 4096, c, 5)
        s = torch.cuda.current_stream().cuda_stream
        calls = {"fri_hip_search_quality_ssim (0.95)": lambda: plan.search_quality_ssim(img.data_ptr(), 0.95, stream=s),
                 "fri_hip_search_quality (40 dB)": lambda: plan.search_quality(img.data_ptr(), 40.0, stream=s)}
        results = {k: f() for k, f in calls.items()}  # spin-up (the probes' buffers)
        ts = {k: [] for k in calls}
        for _ in range(rounds):
            for k, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                ts[k].append((time.perf_counter() - t0) * 1e6)
        for k in calls:
            m = statistics.median(ts[k])
            q, v = results[k]
            lines.append(f"search 4096^2 C={c} {k:36s} {m:9.1f} us per call  (7 probes: {m / 7:.1f} us each; quality {q}, {v:.6f}; runs {min(ts[k]):.1f}-{max(ts[k]):.1f})")
            print(lines[-1], flush=True)
        del plan, img
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()
