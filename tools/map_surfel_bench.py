#!/usr/bin/env python
"""Developer tool: time of the map normals and of the surfel render (csrc/sp_surfel.hip, csrc/sp_views.hip) on the GPU, by the protocol of
tools/map_splat_bench.py: ONE call on preallocated buffers, HIP events around blocks of calls, warm-up of every shape first, then the
median (min - max) over alternating rounds.

Normals: ``sp_map_normals`` beside ``sp_map_points`` on the SAME records -- the 60 keyframes of 224 x 288 x 40 segments of
tools/results_bench.py, strides 1 and 4 --, alternating in the same run.

Surfels: ``sp_render_surfels`` beside ``sp_render_splats`` (the yardstick) on the clouds and footprints of profiles/map_splat.txt -- the
1.2-million-point cloud into V = 1 and V = 8 posed views at 224 x 288 and 480 x 640 --, alternating in the same run, two-sided
(cull = 0), with tilted unit normals ((0.5 g, 0.5 g, -1) normalised, g standard normal).  A third column runs ``sp_render_surfels`` with
ALL NORMALS ZERO: the surfel kernel's flat path, which offers sp_render_splats' keys -- the same atomics on the same pixels -- and
divides nothing.  What the tilted surfels cost beyond it is the per-pixel float64 arithmetic (and whatever the per-pixel depths do to
the contention of the atomics); what it costs beyond sp_render_splats is the kernel's own overhead (normals staged, a longer loop body).

    python tools/map_surfel_bench.py [--out profiles/map_surfel.txt] [--rounds 7]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from map_render_bench import Q, fmt, make_scene, timed  # noqa: E402
from map_splat_bench import FOOTPRINTS, MAX_PX, count_triples, radii_of  # noqa: E402


def normals_lines(rounds):
    import torch
    from results_bench import N_KF, H, W, N_SEG, make_keyframes
    from super_primitive_amd import _lib
    from super_primitive_amd.tool import viz
    dev = torch.device("cuda:0")
    lib = _lib.load()
    kfs, klds, poses = make_keyframes(dev)
    lines = [f"map normals of {N_KF} keyframes of {H} x {W} x {N_SEG}, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_map_normals and sp_map_points = ONE launch each on the same records and preallocated outputs, alternating in the same run",
             f"{'stride':>6} {'rows':>9} {'sp_map_normals':>26} {'sp_map_points':>26} {'normals / points':>17} {'rows without a normal':>22}"]
    print("\n".join(lines), flush=True)
    for stride in (1, 4):
        recs_d, keep, offsets, blocks = viz.keyframe_records("map_surfel_bench", kfs, klds, stride, poses.contiguous().float(), None)
        total = offsets[-1]
        points, colours = torch.empty(total, 3, device=dev), torch.empty(total, 3, device=dev)
        kf_index, seg_ids = torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev)
        normals = torch.empty(total, 3, device=dev)
        stream = _lib.stream_ptr()

        def map_points():
            _lib.check(lib.sp_map_points(_lib.ptr(recs_d), N_KF, blocks, stride, None, 0, _lib.ptr(points), _lib.ptr(colours), _lib.ptr(kf_index),
                                         _lib.ptr(seg_ids), total, stream), "sp_map_points")

        def map_normals():
            _lib.check(lib.sp_map_normals(_lib.ptr(recs_d), N_KF, blocks, stride, None, 0, _lib.ptr(normals), total, stream), "sp_map_normals")
        map_normals()
        none = int((normals == 0).all(dim=1).sum())
        tn, tp = timed([map_normals, map_points], rounds, block=20)
        lines.append(f"{stride:>6} {total:>9} {fmt(tn):>26} {fmt(tp):>26} {tn[0] / tp[0]:>16.2f}x {none:>22}")
        print(lines[-1], flush=True)
        del keep
    return lines


def surfel_lines(rounds):
    import torch
    from super_primitive_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["", f"surfel render of {Q} points, max_px {MAX_PX}, cull 0, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_render_surfels (tilted unit normals), sp_render_surfels with all normals zero (its flat path: sp_render_splats' keys, no division) and",
             "sp_render_splats = ONE call each for the V views on preallocated buffers, alternating in the same run",
             f"{'size':>9} {'V':>2} {'footprint':>14} {'triples':>11} {'sp_render_surfels':>24} {'Gtriples/s':>10} {'... normals zero':>24} "
             f"{'sp_render_splats':>24} {'surfels / splats':>16} {'zero / splats':>13}"]
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
            g = torch.Generator(device="cpu").manual_seed(12)
            tilt = torch.randn(Q, 3, generator=g) * torch.tensor([0.5, 0.5, 0.0]) + torch.tensor([0.0, 0.0, -1.0])
            tilted = (tilt / tilt.norm(dim=1, keepdim=True)).to(dev).contiguous()
            zero = torch.zeros_like(tilted)
            for name, h in FOOTPRINTS:
                radii = radii_of(pts, float(K[0, 0]), h)

                def splats(radii=radii):
                    _lib.check(lib.sp_render_splats(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, 1e-6, _lib.ptr(radii), MAX_PX,
                                                    _lib.ptr(keys), _lib.ptr(image), _lib.ptr(depth), _lib.ptr(index), stream), "sp_render_splats")

                def surfels(radii=radii, normals=tilted):
                    _lib.check(lib.sp_render_surfels(_lib.ptr(pts), _lib.ptr(cols), _lib.ptr(normals), Q, _lib.ptr(views), V, H, W, 1e-6, _lib.ptr(radii),
                                                     MAX_PX, 0, _lib.ptr(keys), _lib.ptr(image), _lib.ptr(depth), _lib.ptr(index), stream),
                               "sp_render_surfels")

                def flat(radii=radii):
                    surfels(radii, zero)
                splats()
                d0, i0 = depth.clone(), index.clone()
                flat()
                assert torch.equal(d0, depth) and torch.equal(i0, index), "zero normals are not the footprint render"
                triples = sum(count_triples(pts, radii, K, pose, H, W)[1] for pose in poses)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                surfels()
                stop.record()
                torch.cuda.synchronize()
                block = int(min(40, max(3, 60.0 / max(start.elapsed_time(stop), 1e-3))))       # blocks of about 60 ms
                ts, tz, tf = timed([surfels, flat, splats], rounds, block=block)
                lines.append(f"{H}x{W:>4} {V:>2} {name:>14} {triples:>11} {fmt(ts):>24} {triples / (ts[0] * 1e-3) / 1e9:>10.2f} {fmt(tz):>24} {fmt(tf):>24} "
                             f"{ts[0] / tf[0]:>15.2f}x {tz[0] / tf[0]:>12.2f}x")
                print(lines[-1], flush=True)
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    text = "\n".join(normals_lines(args.rounds) + surfel_lines(args.rounds)) + "\n"       # (printed line by line as it is measured)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
