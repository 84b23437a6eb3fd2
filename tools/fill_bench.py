#!/usr/bin/env python
"""Developer tool: time of the depth fill (sp_depth_fill_nearest) and the depth metrics (sp_depth_metrics) at the reference's
working size, 480 x 640 -- B = 1 and B = 64, with 5 % and 15 % random holes and a 58 % blob mask -- in us per image (HIP events
around the native calls, buffers allocated once; and around the Python call, which allocates), next to scipy's
distance_transform_edt on one CPU core of the same machine.

    python tools/fill_bench.py [--out profiles/depth_fill.txt] [--reps 50]

``--gap`` needs no GPU: on synthetic scenes, how far the scores of a nearest-only fill (what this package provides) lie from those
of the reference's griddata + nearest fill (fill_in_tools.py:9-21, restated with scipy).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_fill_ref as ref  # noqa: E402

H, W = 480, 640


def blob_mask(fraction, seed, h=H, w=W):
    """Invalid discs until `fraction` of the image is covered; border rows and columns invalid."""
    rng = np.random.default_rng(seed)
    r, c = np.mgrid[:h, :w]
    m = np.zeros((h, w), dtype=bool)
    m[[0, -1], :] = True
    m[:, [0, -1]] = True
    while m.mean() < fraction:
        r0, c0, rad = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, min(h, w) / 5)
        m |= (r - r0) ** 2 + (c - c0) ** 2 <= rad ** 2
    return m


def masks_for(kind, B):
    if kind == "58 % blobs":
        distinct = [blob_mask(0.58, s) for s in range(min(B, 8))]
        return np.stack([distinct[b % len(distinct)] for b in range(B)])
    p = {"5 % holes": 0.05, "15 % holes": 0.15}[kind]
    return np.random.default_rng(1).uniform(size=(B, H, W)) < p


def device_times(kind, B, reps):
    import torch
    from super_primitive_amd import _lib
    from super_primitive_amd.depth_completion import fill_in_tools, void
    lib = _lib.load()
    dev = torch.device("cuda:0")
    invalid = masks_for(kind, B)
    depth = np.random.default_rng(2).uniform(0.3, 5.0, size=(B, H, W)).astype(np.float32)
    d, inv = torch.from_numpy(depth).to(dev), torch.from_numpy(invalid).to(dev)
    inv8 = inv.view(torch.uint8)
    ws = torch.empty(lib.sp_depth_fill_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    filled, index = torch.empty_like(d), torch.empty(B, H, W, dtype=torch.int32, device=dev)
    counts = torch.empty(B, 2, dtype=torch.int32, device=dev)
    mws = torch.empty(lib.sp_depth_metrics_workspace_doubles(B, H, W), dtype=torch.float64, device=dev)
    mout = torch.empty(B, 12, dtype=torch.float64, device=dev)
    valid8 = (~inv).view(torch.uint8)

    def native_fill():
        _lib.check(lib.sp_depth_fill_nearest(_lib.ptr(d), _lib.ptr(inv8), B, H, W, _lib.ptr(ws), _lib.ptr(filled), _lib.ptr(index),
                                             _lib.ptr(counts), _lib.stream_ptr()), "sp_depth_fill_nearest")

    def native_metrics():
        _lib.check(lib.sp_depth_metrics(_lib.ptr(filled), _lib.ptr(d), _lib.ptr(valid8), B, H, W, _lib.ptr(mws), _lib.ptr(mout),
                                        _lib.stream_ptr()), "sp_depth_metrics")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return 1e3 * start.elapsed_time(stop) / reps / B                      # us per image

    out = {"fill": timed(native_fill), "fill_py": timed(lambda: fill_in_tools.fill_depth(d, inv)),
           "metrics": timed(native_metrics), "metrics_py": timed(lambda: void.depth_metrics(filled, d, ~inv))}
    want = ref.scipy_index(invalid[0])
    assert np.array_equal(index[0].cpu().numpy(), want), "the timed fill is not scipy's"
    return out, invalid


def scipy_time(invalid, reps=3):
    from scipy import ndimage
    best = np.inf
    for _ in range(reps):
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(invalid, return_distances=False, return_indices=True)
        best = min(best, time.perf_counter() - t0)
    return 1e6 * best


def bench(reps):
    lines = [f"depth fill and depth metrics, {H} x {W}, us per image (device: HIP events over {reps} calls; scipy: best of 3, one core)",
             f"{'mask':<12} {'B':>3} {'fill':>9} {'fill (Python call)':>19} {'metrics':>9} {'metrics (Python call)':>22} {'scipy edt':>10} {'scipy / fill':>13}"]
    for kind in ("5 % holes", "15 % holes", "58 % blobs"):
        for B in (1, 64):
            t, invalid = device_times(kind, B, reps)
            cpu = scipy_time(invalid[0])
            lines.append(f"{kind:<12} {B:>3} {t['fill']:>9.1f} {t['fill_py']:>19.1f} {t['metrics']:>9.1f} {t['metrics_py']:>22.1f} {cpu:>10.0f} "
                         f"{cpu / t['fill']:>12.0f}x")
    return lines


# ---- --gap: nearest only against griddata + nearest, on the CPU ---------------------------------------------------------
def griddata_fill(depth, invalid):
    """fill_in_tools.py:9-21: linear interpolation over the Delaunay triangulation of the valid pixels, then the nearest valid pixel
    for what lies outside their convex hull."""
    from scipy.interpolate import griddata
    r, c = np.indices(depth.shape)
    out = depth.astype(np.float32).copy()
    out[invalid] = griddata((r[~invalid], c[~invalid]), depth[~invalid], (r[invalid], c[invalid]))
    return ref.scipy_fill(out, np.isnan(out))


def gap():
    from super_primitive_amd import synth
    names = ref.METRIC_NAMES[1:7]
    lines = ["nearest-only fill (this package) against griddata + nearest (the reference), CPU, scipy; estimate = the scene's depth on",
             "the valid pixels, target = the scene's depth everywhere, scored over every pixel",
             f"{'scene':<28} {'fill':<18} " + " ".join(f"{n:>10}" for n in names)]
    scenes = []
    for seed in (81, 82, 83):                                                 # the scenes and holes of tests/test_gpu_depth_fill.py
        pair = synth.make_pair(60, 80, 12, seed=seed, overlap=2)
        rng = np.random.default_rng(seed)
        hole = rng.uniform(size=pair.depth.shape) < 0.03
        hole[[0, -1], :] = True
        hole[:, [0, -1]] = True
        hole[10:16, 30:50] = True
        scenes.append((f"60 x 80, seed {seed}, {100 * hole.mean():.0f} % holes", pair.depth.astype(np.float32), hole))
    pair = synth.make_pair(H, W, 48, seed=7, overlap=2)
    scenes.append((f"{H} x {W}, 58 % blobs", pair.depth.astype(np.float32), blob_mask(0.58, 0)))
    for name, depth, invalid in scenes:
        everywhere = np.ones_like(invalid)
        rows = {"nearest": ref.metrics(ref.scipy_fill(depth, invalid), depth, everywhere),
                "griddata + nearest": ref.metrics(griddata_fill(depth, invalid), depth, everywhere)}
        for fill, m in rows.items():
            lines.append(f"{name:<28} {fill:<18} " + " ".join(f"{v:>10.4g}" for v in m[1:7]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--gap", action="store_true")
    args = ap.parse_args()
    lines = gap() if args.gap else bench(args.reps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
