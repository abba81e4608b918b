"""The launch arithmetic and the strip classes of the later raster kernels (K7, K8, K10, K12) restated on the host, the deterministic cases that reach what a
small random shape cannot, and the case counts of the second sweep (tests/tools/fuzz_later.py). tests/test_later_cases_host.py checks, without a GPU, that the
cases reach the cells they are here for; the GPU tests (test_gpu_ssim.py, test_gpu_tiled_search.py, test_gpu_chroma420.py, test_gpu_fuzz.py) run them.

Constants copied from the kernels (change both together):
  k7_ssim.hip       kSsimNB = 2 (blocks per lane), kSsimWaves = 4, a strip = 64 kSsimNB block columns, target_waves = 4096, band clamped to [4, 64]
  k8_chroma420.hip  kC420Strip = 16 pixels per lane, kC420Threads = 256
  k10_tiles.hip     kTileStrip = 16 bytes per lane, kTileThreads = 256, kMeasureStrips = 32, kMeasureGroups = 512
  k12_tiles420.hip  kT420Strip = 16 pixels per lane"""
import numpy as np

K7_NB, K7_WAVES, K7_STRIP, K7_TARGET_WAVES, K7_BAND_MIN, K7_BAND_MAX = 2, 4, 128, 4096, 4, 64
K8_STRIP, K8_THREADS = 16, 256
K10_STRIP, K10_THREADS, K10_MEASURE_STRIPS, K10_MEASURE_GROUPS = 16, 256, 32, 512
K12_STRIP = 16

SEED = 20261019
# cases per kind of the second sweep: the smallest counts (not below 40) at which the fixed-seed dry run reaches every cell test_later_cases_host.py asks for
N_CASES = {"ycbcr": 40, "ssim": 40, "rate": 40, "c420": 40, "rgba": 40, "tiled": 60, "tiled420": 60, "rans": 40, "decode": 59}


def _ceil(a, b):
    return -(-a // b)


# ---- K7 ------------------------------------------------------------------------------------------------------------------------------------------------------

def k7_launch(w, h, n_images=1):
    """launch_ssim's arithmetic: dict(bx, nx, ny, n_strips, band, bands, groups)"""
    bx = w // 4
    nx, ny = bx - 1, h // 4 - 1
    n_strips = _ceil(nx, K7_STRIP)
    band = min(max(_ceil(ny * n_strips * n_images, K7_TARGET_WAVES), K7_BAND_MIN), K7_BAND_MAX)
    bands = _ceil(ny, band)
    return dict(bx=bx, nx=nx, ny=ny, n_strips=n_strips, band=band, bands=bands, groups=n_strips * _ceil(bands, K7_WAVES),
                unclamped=_ceil(ny * n_strips * n_images, K7_TARGET_WAVES))


def k7_cells(w, h, n_images=1):
    """the cells of ssim_kernel a launch reaches: the band size's range, a ragged last band, waves whose band starts past ny, strips that are `full`, and what
    the last strip holds"""
    L = k7_launch(w, h, n_images)
    bx, ny, band = L["bx"], L["ny"], L["band"]
    out = {"band=4" if band == K7_BAND_MIN else "band=64" if band == K7_BAND_MAX else "4<band<64"}
    if L["unclamped"] > K7_BAND_MAX:
        out.add("band clamped from above")
    if ny % band:
        out.add("ragged last band")
    if K7_WAVES * _ceil(L["bands"], K7_WAVES) > L["bands"]:
        out.add("a wave's band starts past ny")
    last = L["n_strips"] - 1
    if any((s + 1) * K7_STRIP < bx for s in range(L["n_strips"])):
        out.add("a full strip")
    if (last + 1) * K7_STRIP < bx:  # only bx = 128 n_strips + 1: the last lane's third block is the row's last
        out.add("last strip full, its third block the row's last")
    in_last = bx - last * K7_STRIP  # block columns the last strip's lanes see
    if last > 0 and in_last <= K7_NB:
        out.add("last strip: a single lane with %d block%s" % (in_last, "s" if in_last > 1 else ""))
    return out


# test_gpu_ssim.py, the n-image form: (W, H, C, n_images) -> the cells it is here for
SSIM_BAND_CASES = [((16, 4100, 1, 23), {"4<band<64", "ragged last band", "a wave's band starts past ny"}),
                   ((16, 4100, 3, 38), {"4<band<64", "ragged last band", "a wave's band starts past ny"}),
                   ((16, 4104, 1, 260), {"band=64", "band clamped from above", "ragged last band", "a wave's band starts past ny"})]
# test_gpu_ssim.py, test_k7_equals_the_oracle: (W, H, C) with bx % 128 = 1 and 2
SSIM_EDGE_SHAPES = [(516, 24, 1), (520, 20, 1), (516, 20, 3), (520, 24, 3)]


# ---- K8 ------------------------------------------------------------------------------------------------------------------------------------------------------

def k8_cells(w, h):
    """split420_kernel / merge420_kernel: whole strips (three 16-byte accesses a row), the row's last, partial strip (byte by byte, the column clamped), an odd
    last column and row (replicated)"""
    out = set()
    if w >= K8_STRIP:
        out.add("whole strip")
    if w % K8_STRIP:
        out.add("partial last strip")
    out.add("odd w" if w & 1 else "even w")
    out.add("odd h" if h & 1 else "even h")
    if _ceil(w, K8_STRIP) * h > K8_THREADS:
        out.add("more than one workgroup")
    return out


K8_CELLS = {"whole strip", "partial last strip", "odd w", "even w", "odd h", "even h", "more than one workgroup"}
# test_gpu_chroma420.py: the measuring merge on the saturated pair; whole strips only, whole workgroups only
C420_SATURATED = (1024, 64)


# ---- K10 -----------------------------------------------------------------------------------------------------------------------------------------------------

def k10_grid(w, h, c, tw, th):
    """grid_of and launch_measure_tiles: dict(nx, ny, row_bytes, strips_per_row, n_strips, groups, per_lane, measure_groups)"""
    nx, ny = _ceil(w, tw), _ceil(h, th)
    row_bytes = tw * c
    spr = _ceil(row_bytes, K10_STRIP)
    n_strips = nx * ny * th * spr
    groups = _ceil(n_strips, K10_THREADS)
    per_lane = min(K10_MEASURE_STRIPS, _ceil(groups, K10_MEASURE_GROUPS))
    return dict(nx=nx, ny=ny, row_bytes=row_bytes, strips_per_row=spr, n_strips=n_strips, groups=groups, per_lane=per_lane, measure_groups=_ceil(groups, per_lane),
                unclamped=_ceil(groups, K10_MEASURE_GROUPS))


def k10_measure_cells(w, h, c, tw, th):
    G = k10_grid(w, h, c, tw, th)
    out = {"per_lane=1" if G["per_lane"] == 1 else "per_lane=32" if G["per_lane"] == K10_MEASURE_STRIPS else "1<per_lane<32"}
    if G["unclamped"] > K10_MEASURE_STRIPS:
        out.add("per_lane clamped from above")
    if G["per_lane"] > 1 and G["groups"] % G["per_lane"]:
        out.add("ragged last round")
    return out


def k10_cells(w, h, c, tw, th):
    """the strip classes of split_tiles_kernel / merge_tiles_kernel / measure_tiles_kernel<c>, each prefixed with the channel count"""
    G = k10_grid(w, h, c, tw, th)
    i, s = np.meshgrid(np.arange(G["nx"]), np.arange(G["strips_per_row"]), indexing="ij")
    b0 = s * K10_STRIP
    n = np.minimum(K10_STRIP, G["row_bytes"] - b0)
    at0 = i * tw * c + b0
    image_row = w * c
    fast = (n == K10_STRIP) & (at0 + K10_STRIP <= image_row)
    out = set()
    for name, mask in (("fast 16-byte strip", fast), ("partial last strip inside the row", ~fast & (n < K10_STRIP) & (at0 + n <= image_row)),
                       ("whole strip across the clamped edge", ~fast & (n == K10_STRIP) & (at0 < image_row)),
                       ("partial last strip across the clamped edge", ~fast & (n < K10_STRIP) & (at0 < image_row) & (at0 + n > image_row)),
                       ("strip past the image row", at0 >= image_row)):
        if mask.any():
            out.add(name)
    if G["ny"] * th > h:
        out.add("replicated rows")
    if G["row_bytes"] < K10_STRIP:
        out.add("tile_w c < 16")
    if G["row_bytes"] % K10_STRIP:
        out.add("tile_w c no multiple of 16")
    if tw > w or th > h:
        out.add("tile larger than the image")
    if w % tw == 0 and G["nx"] > 1:
        out.add("w a multiple of tile_w")
    if G["groups"] > 1:
        out.add("more than one workgroup")
    return {"C%d: %s" % (c, x) for x in out}


K10_CLASSES = ["fast 16-byte strip", "partial last strip inside the row", "whole strip across the clamped edge", "partial last strip across the clamped edge",
               "strip past the image row", "replicated rows", "tile_w c < 16", "tile_w c no multiple of 16", "tile larger than the image", "w a multiple of tile_w",
               "more than one workgroup"]
K10_CELLS = {"C%d: %s" % (c, x) for c in (1, 3) for x in K10_CLASSES}


def k10_region_cells(c, tw, th, x, y, rw, rh):
    """the strip classes of merge_tiles_region_kernel<c> for one region"""
    row_bytes, region_row = tw * c, rw * c
    b0 = np.arange(0, region_row, K10_STRIP)
    n = np.minimum(K10_STRIP, region_row - b0)
    xb = ((x % tw) * c + b0) % row_bytes
    inside = xb + n <= row_bytes
    out = set()
    for name, mask in (("fast 16-byte strip", (n == K10_STRIP) & inside), ("whole strip across a tile column", (n == K10_STRIP) & ~inside),
                       ("partial last strip in one tile", (n < K10_STRIP) & inside), ("partial last strip across a tile column", (n < K10_STRIP) & ~inside)):
        if mask.any():
            out.add(name)
    if y // th != (y + rh - 1) // th:
        out.add("rows of more than one tile row")
    if row_bytes < K10_STRIP and region_row >= K10_STRIP:
        out.add("tile_w c < 16")
    return {"C%d region: %s" % (c, v) for v in out}


K10_REGION_CLASSES = ["fast 16-byte strip", "whole strip across a tile column", "partial last strip in one tile", "partial last strip across a tile column",
                      "rows of more than one tile row", "tile_w c < 16"]
K10_REGION_CELLS = {"C%d region: %s" % (c, x) for c in (1, 3) for x in K10_REGION_CLASSES}

# test_gpu_tiled_search.py, the measuring kernel: (W, H, C, tile_w, tile_h) -> the cells it is here for
MEASURE_RAGGED = ((1500, 1000, 3, 500, 333), {"1<per_lane<32", "ragged last round"})
MEASURE_CLAMPED = ((8300, 8250, 1, 1024, 1024), {"per_lane=32", "per_lane clamped from above"})


# ---- K12 -----------------------------------------------------------------------------------------------------------------------------------------------------

def k12_split_cells(w, h, tw, th):
    """split_tiles420_kernel: whole strips (no clamp of either kind), a tile row's last strip past the tile, a strip inside the tile but past the image,
    the parities of the tile's sides (an odd one replicates the tile's last column or row in the chroma mean), the image's clamped bottom edge"""
    nx, ny = _ceil(w, tw), _ceil(h, th)
    ti, x0 = np.meshgrid(np.arange(nx), np.arange(0, tw, K12_STRIP), indexing="ij")
    in_tile, in_image = x0 + K12_STRIP <= tw, ti * tw + x0 + K12_STRIP <= w
    out = set()
    for name, mask in (("whole strip", in_tile & in_image), ("strip past the tile row", ~in_tile), ("strip in the tile, past the image", in_tile & ~in_image)):
        if mask.any():
            out.add(name)
    out.add("odd tile_w" if tw & 1 else "even tile_w")
    out.add("odd tile_h" if th & 1 else "even tile_h")
    if ny * th > h:
        out.add("clamped bottom edge")
    if nx * tw > w:
        out.add("clamped right edge")
    return {"split: " + v for v in out}


K12_SPLIT_CELLS = {"split: " + v for v in ("whole strip", "strip past the tile row", "strip in the tile, past the image", "odd tile_w", "even tile_w", "odd tile_h",
                                           "even tile_h", "clamped bottom edge", "clamped right edge")}


def k12_region_cells(tw, th, x, y, rw, rh, prefix="region"):
    """merge_tiles420_region_kernel for one region: per strip the parity of its first tile column and whether it lies in one tile row (the 16-pixel instance
    of that parity), crosses a tile column, or is the row's last, partial strip (both pixel by pixel); the parity of the first tile row"""
    rx0 = np.arange(0, rw, K12_STRIP)
    n = np.minimum(K12_STRIP, rw - rx0)
    tx = (x % tw + rx0) % tw
    odd = (tx & 1).astype(bool)
    out = set()
    for name, mask in (("one tile row", (n == K12_STRIP) & (tx + K12_STRIP <= tw)), ("crossing", (n == K12_STRIP) & (tx + K12_STRIP > tw)), ("partial", n < K12_STRIP)):
        for parity, pm in (("even", ~odd), ("odd", odd)):
            if (mask & pm).any():
                out.add("%s, %s start" % (name, parity))
    out.add("odd first row" if (y % th) & 1 else "even first row")
    return {"%s: %s" % (prefix, v) for v in out}


K12_REGION_CELLS = {"region: %s, %s start" % (a, b) for a in ("one tile row", "crossing", "partial") for b in ("even", "odd")} | {"region: odd first row", "region: even first row"}
