#!/usr/bin/env python
"""Developer tool: time of the footprint render (csrc/sp_views.hip, sp_render_splats) on the GPU, by the protocol of
tools/map_render_bench.py: its 1.2-million-point cloud into V = 1 and V = 8 posed views at 224 x 288 and 480 x 640, ONE call on
preallocated buffers, HIP events around blocks of calls, warm-up of every shape first, then the median (min - max) over alternating
rounds.

Per size and V one line per footprint: radii r = h z / f, i.e. half-widths of about h = 0, 0.5, 1, 2 and 4 px in every view; a MIXED
cloud (every 8th point h = 4, the others h = 0.5: the rectangle sizes within a wave differ by a factor of 20) and the uniform cloud
with about the same number of covered pixels (h = 1.34).  Beside each: ``sp_render_views`` in mode 1 on the same inputs, alternating
with it in the same run (the baseline: the point render); the covered (point, view, pixel) triples -- an upper bound of the atomics
issued: a pixel the point already loses is skipped after a plain load -- and triples per second; the coverage of the views.

    python tools/map_splat_bench.py [--out profiles/map_splat.txt] [--rounds 7]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from map_render_bench import Q, fmt, make_scene, timed  # noqa: E402

MAX_PX = 8
FOOTPRINTS = [("h = 0", 0.0), ("h = 0.5", 0.5), ("h = 1", 1.0), ("h = 2", 2.0), ("h = 4", 4.0), ("mixed 4 | 0.5", None), ("h = 1.34", 1.34)]


def radii_of(pts, f, h):
    """(Q,) float32: h z / f; ``h`` None: the mixed cloud."""
    import torch
    if h is None:
        hs = torch.full((pts.shape[0],), 0.5, device=pts.device)
        hs[::8] = 4.0
    else:
        hs = torch.full((pts.shape[0],), float(h), device=pts.device)
    return (hs * pts[:, 2] / f).contiguous()


def count_triples(pts, radii, K, pose, H, W):
    """The header's arithmetic with torch ops in float64: the kept points and the pixels of their rectangles, one view."""
    import torch
    p = pts.double()
    pc = (p - pose[:3, 3].double()) @ pose[:3, :3].double()
    z = pc[:, 2]
    fx, fy = K[0, 0].double(), K[1, 1].double()
    u = pc[:, 0] * fx / z + K[0, 2].double()
    v = pc[:, 1] * fy / z + K[1, 2].double()
    ru = (radii.double() * fx / z).clamp(min=0, max=MAX_PX).nan_to_num(nan=0.0)
    rv = (radii.double() * fy / z).clamp(min=0, max=MAX_PX).nan_to_num(nan=0.0)
    keep = torch.isfinite(u) & torch.isfinite(v) & (z > 1e-6) & (u + ru >= 0) & (u - ru < W) & (v + rv >= 0) & (v - rv < H)
    nc = torch.floor(u + ru).clamp(max=W - 1) - torch.floor(u - ru).clamp(min=0) + 1
    nr = torch.floor(v + rv).clamp(max=H - 1) - torch.floor(v - rv).clamp(min=0) + 1
    return int(keep.sum()), int((nc * nr)[keep].sum())


def lines_of(rounds):
    import torch
    from super_primitive_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"footprint render of {Q} points, max_px {MAX_PX}, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_render_splats = ONE call for the V views on preallocated buffers; sp_render_views = mode 1 on the same inputs, alternating in the same run",
             f"{'size':>9} {'V':>2} {'footprint':>14} {'kept pairs':>10} {'triples':>11} {'coverage':>8} {'sp_render_splats':>24} {'Gtriples/s':>10} "
             f"{'sp_render_views mode 1':>24} {'splats / points':>15}"]
    print("\n".join(lines), flush=True)
    for H, W in ((224, 288), (480, 640)):
        for V in (1, 8):
            pts, cols, K, poses = make_scene(dev, V, H, W)
            views = torch.cat((K.reshape(1, 9).expand(V, 9), poses.reshape(V, 16)), dim=1).contiguous()
            keys = torch.empty(V * H * W, dtype=torch.int64, device=dev)
            image = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
            depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
            index = torch.empty(V, H, W, dtype=torch.int32, device=dev)
            stream = _lib.stream_ptr()

            def points_only():
                _lib.check(lib.sp_render_views(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, 1, 1e-6, _lib.ptr(keys),
                                               _lib.ptr(image), _lib.ptr(depth), _lib.ptr(index), stream), "sp_render_views")
            points_only()
            d0, i0 = depth.clone(), index.clone()
            for name, h in FOOTPRINTS:
                radii = radii_of(pts, float(K[0, 0]), h)

                def splats(radii=radii):
                    _lib.check(lib.sp_render_splats(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, 1e-6, _lib.ptr(radii), MAX_PX,
                                                    _lib.ptr(keys), _lib.ptr(image), _lib.ptr(depth), _lib.ptr(index), stream), "sp_render_splats")
                splats()
                if h == 0.0:
                    assert torch.equal(d0, depth) and torch.equal(i0, index), "radius 0 is not the point render"
                coverage = float((index >= 0).float().mean())
                kept, triples = 0, 0
                for pose in poses:
                    k, t = count_triples(pts, radii, K, pose, H, W)
                    kept, triples = kept + k, triples + t
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                splats()
                stop.record()
                torch.cuda.synchronize()
                block = int(min(40, max(3, 60.0 / max(start.elapsed_time(stop), 1e-3))))       # blocks of about 60 ms
                ts, tp = timed([splats, points_only], rounds, block=block)
                lines.append(f"{H}x{W:>4} {V:>2} {name:>14} {kept:>10} {triples:>11} {coverage:>8.4f} {fmt(ts):>24} {triples / (ts[0] * 1e-3) / 1e9:>10.2f} "
                             f"{fmt(tp):>24} {ts[0] / tp[0]:>14.2f}x")
                print(lines[-1], flush=True)
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    text = "\n".join(lines_of(args.rounds)) + "\n"                       # (printed line by line as it is measured)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
