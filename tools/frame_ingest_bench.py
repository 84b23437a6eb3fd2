#!/usr/bin/env python
"""Developer tool: time of the frame ingest (sp_frame_ingest: undistort, crop, convert, downsample in one launch) at the working size,
480 x 640 -> crop 32 / 16 -> 224 x 288 with the camera of tests/golden/tum_fr1_camera.json, for B = 1, 16 and 64 frames per call, in us
per frame (HIP events; buffers allocated once for the native call, and the Python call, which allocates) with the achieved bytes/s over
the algorithmic bytes (the raw frame read once, the output written once).  Beside it the same stage composed from torch device ops --
F.grid_sample on a float copy of the frame with a precomputed float32 grid of the cropped pixels, F.interpolate, flip, / 255: what a
user would otherwise write -- in the same call, alternating blocks of 100 calls; the depth ingest; and the numpy restatement's CPU time
as context.

    python tools/frame_ingest_bench.py [--out profiles/frame_ingest.txt] [--rounds 5]

``--kernels CSV``: no GPU needed; per-kernel times of a ``rocprofv3 --kernel-trace`` run of this tool (its *_kernel_trace.csv), by
kernel and grid size.
"""
import argparse
import csv
import ctypes
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frame_ingest_ref as ref  # noqa: E402

BLOCK = 100           # calls per timed block


def algorithmic_bytes(H, W, Ho, Wo):
    return 3 * H * W + 4 * 3 * Ho * Wo


def torch_composition(case, dev):
    """The stage from torch device ops; returns fn(raw (B,H,W,3) u8) -> (B,3,Ho,Wo)."""
    import torch
    import torch.nn.functional as F
    H, W = case["size"]
    mh, mw = case["margins"]
    mx, my = ref.undistort_map(H, W, case["K"], case["dist"])
    grid = np.stack([2 * mx / (W - 1) - 1, 2 * my / (H - 1) - 1], -1)[mh:H - mh, mw:W - mw]
    grid = torch.from_numpy(grid.astype(np.float32)).to(dev)[None]
    Ho, Wo = (H - 2 * mh) // 2 ** case["downsample_pow"], (W - 2 * mw) // 2 ** case["downsample_pow"]

    def run(raw):
        x = raw.permute(0, 3, 1, 2).float()
        x = F.grid_sample(x, grid.expand(raw.shape[0], -1, -1, -1), mode="bilinear", padding_mode="zeros", align_corners=True)
        return F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False).flip(1) / 255.0
    return run


def bench(rounds):
    import torch
    from super_primitive_amd import _lib
    from super_primitive_amd.frontend.frame_ingest import FrameIngest
    assert torch.cuda.is_available(), "the timings need a GPU"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    case = ref.tum_case()
    H, W = case["size"]
    mh, mw = case["margins"]
    fi = FrameIngest(case["K"], case["dist"], size=case["size"], crop=case["margins"], downsample_pow=case["downsample_pow"])
    Ho, Wo = fi.out_size
    composed = torch_composition(case, dev)
    per_frame = algorithmic_bytes(H, W, Ho, Wo)

    def blocks(fns, B):
        """us per frame of each fn: ``rounds`` alternating blocks of BLOCK calls, HIP events around every block; (mean, min, max)."""
        for fn in fns:                                                             # warm-up of every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(rounds):
            for k, fn in enumerate(fns):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(BLOCK):
                    fn()
                stop.record()
                torch.cuda.synchronize()
                times[k].append(1e3 * start.elapsed_time(stop) / BLOCK / B)
        return [(float(np.mean(t)), min(t), max(t)) for t in times]

    lines = [f"frame ingest, {H} x {W} x 3 u8 -> crop {mh} / {mw} -> 3 x {Ho} x {Wo} f32, us per frame: mean (min - max) over {rounds} alternating "
             f"blocks of {BLOCK} calls, HIP events",
             f"algorithmic bytes per frame: {per_frame} (raw read once + output written once)",
             f"{'B':>3} {'sp_frame_ingest':>24} {'GB/s':>7} {'FrameIngest.images':>24} {'torch composition':>24} {'torch / native':>15} "
             f"{'max |torch - native|':>21}"]
    for B in (1, 16, 64):
        raw = torch.from_numpy(ref.noise_frames(B, H, W, 7)).to(dev)
        out = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=dev)

        def native():
            _lib.check(lib.sp_frame_ingest(_lib.ptr(raw), B, H, W, ctypes.addressof(fi.camera), mh, mw, H - 2 * mh, W - 2 * mw, Ho, Wo, 1, _lib.ptr(out),
                                           _lib.stream_ptr()), "sp_frame_ingest")

        (n, n0, n1), (p, p0, p1), (t, t0, t1) = blocks([native, lambda: fi.images(raw), lambda: composed(raw)], B)
        diff = float((composed(raw) - fi.images(raw)).abs().max())
        want = ref.ingest(raw[0].cpu().numpy(), case["K"], case["dist"], case["margins"], case["downsample_pow"])
        assert np.abs(out[0].cpu().numpy() - want).max() <= 2e-6, "the timed ingest is not the restatement's"
        lines.append(f"{B:>3} {f'{n:.2f} ({n0:.2f} - {n1:.2f})':>24} {per_frame / n / 1e3:>7.0f} {f'{p:.2f} ({p0:.2f} - {p1:.2f})':>24} "
                     f"{f'{t:.2f} ({t0:.2f} - {t1:.2f})':>24} {t / n:>14.1f}x {diff:>21.1e}")

    lines += ["", f"depth ingest, {H} x {W} u16 -> crop -> nearest {Ho} x {Wo} f32, us per frame (FrameIngest.depth)"]
    for B in (1, 16, 64):
        raw16 = torch.from_numpy(ref.depth_frames(B, H, W, 8)).to(dev)
        (d, d0, d1), = blocks([lambda: fi.depth(raw16, size=(Ho, Wo))], B)
        lines.append(f"{B:>3} {f'{d:.2f} ({d0:.2f} - {d1:.2f})':>24}")

    raw = ref.noise_frames(1, H, W, 7)[0]
    best = np.inf
    for _ in range(3):
        t0 = time.perf_counter()
        ref.ingest(raw, case["K"], case["dist"], case["margins"], case["downsample_pow"])
        best = min(best, time.perf_counter() - t0)
    lines += ["", f"numpy float64 restatement (tests/frame_ingest_ref.py), one frame, one CPU core, best of 3: {1e3 * best:.0f} ms (context only)",
              "the reference's own cv2.undistort + crop + image_tt + F.interpolate: not measured (cv2 is not available here)"]
    return lines


def kernels(path):
    """Per-kernel durations of a rocprofv3 --kernel-trace csv, by kernel name and grid size."""
    groups = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = re.search(r"k_(frame|depth)_ingest", row["Kernel_Name"])
            if name is None:
                continue
            name = name.group(0)
            grid = tuple(int(row[k]) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = ["per kernel, us per launch (rocprofv3 --kernel-trace, a run of its own; grid in work-items)",
             f"{'kernel':<40} {'grid':>20} {'calls':>6} {'avg':>8} {'min':>8} {'max':>8}"]
    for (name, grid), t in sorted(groups.items(), key=lambda kv: (kv[0][0], kv[0][1][2])):
        lines.append(f"{name:<40} {'x'.join(map(str, grid)):>20} {len(t):>6} {np.mean(t):>8.2f} {min(t):>8.2f} {max(t):>8.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels")
    args = ap.parse_args()
    lines = kernels(args.kernels) if args.kernels else bench(args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
