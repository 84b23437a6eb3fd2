#!/usr/bin/env python
"""Developer tool: time of the mesh views (csrc/sp_mesh_render.hip: sp_mesh_render) on the GPU.

Three meshes, each rasterised into 16 views of 480 x 640 from cameras on a small circle inside a room of 6 x 4 x 3 m, all four outputs:

  (a) the room's six walls subdivided into about ``--faces`` triangles (2 M: a centimetre each, a pixel or two at these distances):
      nearly every item is one tile of one small face;
  (b) ``extract_mesh`` of the volume fused (``fuse_tsdf``, 2.5 cm voxels) from (a)'s own depth images at the same views; as context, NOT a
      bar -- another algorithm on another representation --, ``render_surface`` on the volume it came from;
  (c) the same room as 12 triangles: every face is hundreds of tiles.

Per line the time of ONE call on preallocated buffers, HIP events around blocks of calls, warm-up first, then the median (min - max) over
alternating rounds; items (the (face, view, tile) triples, read back from the scratch's first word) per second; the bytes the count pass
must move (12 B of indices per (face, view), 8 B of prefix written, the vertices once) against the whole call's time -- the kernels'
own times come from a kernel trace of this tool, whose CSV ``--kernel-stats`` folds into the report.

``--lib NAME=PATH`` (repeatable) names another build of the library, timed in the same rounds, alternating with the shipped one; its
outputs must equal the shipped library's word for word:
    make -C super_primitive_amd/csrc MESH_RENDER_FLAGS="-DSP_MESH_RENDER_TILE_W=64"     a tile of 64 x 1 (16: 16 x 4; the default 8: 8 x 8)
    make -C super_primitive_amd/csrc MESH_RENDER_FLAGS="-DSP_MESH_RENDER_COUNTERS"      counts the keys offered and the atomics issued
(touch sp_mesh_render.hip between builds and copy each library aside).  A build with counters reports them; it is not timed.

    python tools/mesh_render_bench.py [--out profiles/mesh_render.txt] [--rounds 5] [--faces 2000000] [--cases abc] [--lib 64x1=/path/lib.so]
    python tools/mesh_render_bench.py --dry      (no GPU: the three meshes at a tiny size through tests/mesh_render_ref.py on the CPU)"""
import argparse
import csv
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTPUTS = ('depth', 'normals', 'image', 'index')
ROOM = (6.0, 4.0, 3.0)


def room(n_faces):
    """The inside of a box of ROOM metres centred at the origin, every wall a grid of squares of one side cut into two triangles that look
    into the room; about ``n_faces`` faces in all.  Vertices are per wall (walls do not share them); colours vary smoothly."""
    area = 2.0 * (ROOM[0] * ROOM[1] + ROOM[0] * ROOM[2] + ROOM[1] * ROOM[2])
    side = (2.0 * area / n_faces) ** 0.5
    verts, faces, base = [], [], 0
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        nu, nv = max(1, round(ROOM[u] / side)), max(1, round(ROOM[v] / side))
        for sign in (-1.0, 1.0):
            gu, gv = np.meshgrid(np.linspace(-0.5, 0.5, nu + 1) * ROOM[u], np.linspace(-0.5, 0.5, nv + 1) * ROOM[v], indexing='ij')
            p = np.zeros((nu + 1, nv + 1, 3))
            p[..., u], p[..., v], p[..., axis] = gu, gv, sign * 0.5 * ROOM[axis]
            verts.append(p.reshape(-1, 3))
            i = (np.arange(nu)[:, None] * (nv + 1) + np.arange(nv)[None, :]).reshape(-1) + base
            a, b, c, d = i, i + (nv + 1), i + (nv + 1) + 1, i + 1
            quads = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
            # (e_u x e_v points along +axis for (u, v) = (1, 2) and (0, 1), along -axis for (0, 2); det < 0 is the front: the side the
            # normal points to, and the normal must point into the room)
            outward = (sign > 0) == (axis != 1)
            faces.append(quads[:, ::-1] if outward else quads)
            base += (nu + 1) * (nv + 1)
    v = np.concatenate(verts).astype(np.float32)
    f = np.ascontiguousarray(np.concatenate(faces)).astype(np.int32)
    colours = (0.5 + 0.5 * np.sin(v * np.array([1.3, 2.1, 2.9], np.float32) + np.array([0.0, 1.0, 2.0], np.float32))).astype(np.float32)
    return v, f, colours


def cameras(V, H, W):
    """V cameras on a circle of 0.5 m around the room's centre, each looking outwards along its radius, tilted a little."""
    import mesh_render_ref as ref
    K = np.array([[0.625 * W, 0, 0.5 * (W - 1)], [0, 0.625 * W, 0.5 * (H - 1)], [0, 0, 1]], np.float32)
    poses = []
    for k in range(V):
        angle = 2.0 * np.pi * k / V
        T = ref.pose((0.0, angle, 0.0), (0.5 * np.sin(angle), 0.1 * np.cos(3 * angle), 0.5 * np.cos(angle)))
        T[:3, :3] = T[:3, :3] @ ref.pose((0.15 * np.sin(2 * angle), 0.0, 0.0))[:3, :3]
        poses.append(T)
    return np.stack([K] * V), np.stack(poses)


def other_library(path):
    from super_primitive_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in ("sp_mesh_render", "sp_mesh_render_scratch_units"):
        getattr(lib, name).argtypes = _lib.SIGNATURES[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def kernel_stats_lines(path):
    """The k_mr_* rows of a kernel-stats CSV (a kernel trace with statistics of one run of this tool), as lines of the report."""
    if not path:
        return []
    out = [f"\nkernel trace of one run of this tool ({os.path.basename(path)}): kernel, calls, total, average, min, max in microseconds"]
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_mr_" in row.get("Name", ""):
                name = row["Name"].split("k_mr_")[1].split("(")[0]
                us = lambda key: float(row[key]) / 1e3
                out.append(f"  k_mr_{name:10s} {int(row['Calls']):5d} {us('TotalDurationNs'):12.1f} {us('AverageNs'):10.1f} {us('MinNs'):10.1f} {us('MaxNs'):10.1f}")
    return out


def dry():
    import mesh_render_ref as ref
    Ks, poses = cameras(4, 24, 32)
    for name, n in (("(a)", 3000), ("(c)", 12)):
        v, f, c = room(n)
        out = ref.render(v, f, Ks, poses, 24, 32, colours=c)
        culled = ref.render(v, f, Ks, poses, 24, 32, cull=1)
        assert all(k['hits'] == 24 * 32 for k in out['counts']), out['counts']          # inside a closed room every pixel is hit
        assert np.array_equal(out['index'], culled['index'])                            # and every wall is seen from its front
        print(f"{name} {len(f)} faces, 4 views of 24 x 32: {out['counts']}")
    print("dry run ok")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed block")
    ap.add_argument("--faces", type=int, default=2_000_000)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH of another build of libsp_hip.so, timed beside the shipped one")
    ap.add_argument("--kernel-stats", help="a kernel-stats CSV of a trace of this tool: its k_mr_* rows are appended to the report")
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    if args.dry:
        return dry()
    if not any(c in args.cases for c in "abc"):                                         # --cases "" --kernel-stats CSV --out REPORT: appended
        with open(args.out, "a") as fh:
            fh.write("\n".join(kernel_stats_lines(args.kernel_stats)) + "\n")
        return None
    import torch
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    dev = torch.device("cuda:0")
    H, W = (int(x) for x in args.size.split("x"))
    V = args.views
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ks_np, poses_np = cameras(V, H, W)
    Ks, poses = T(Ks_np), T(poses_np)
    views = torch.cat((Ks.reshape(V, 9), poses.reshape(V, 16)), dim=1).contiguous()
    libs = [("shipped", _lib.load())] + [(spec.split("=", 1)[0], other_library(spec.split("=", 1)[1])) for spec in args.lib]
    lines = [f"mesh views: sp_mesh_render, {V} views of {H} x {W}, all four outputs; {torch.cuda.get_device_name(0)}",
             f"time of one call: median (min - max) over {args.rounds} rounds of {args.reps} calls, the libraries alternating"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def run_case(title, v, f, c):
        M, F = int(v.shape[0]), int(f.shape[0])
        normals = viz.mesh_faces(v, f)['normals']
        out = dict(depth=torch.empty(V, H, W, dtype=torch.float32, device=dev), normals=torch.empty(V, H, W, 3, dtype=torch.float32, device=dev),
                   image=torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev), index=torch.empty(V, H, W, dtype=torch.int32, device=dev))
        scratch = torch.empty(8 * libs[0][1].sp_mesh_render_scratch_units(F), dtype=torch.int64, device=dev)
        keys = torch.empty(V * H * W, dtype=torch.int64, device=dev)

        def call(lib):
            scratch[:8].zero_()                                                         # (words 1 and 2: only a build with counters writes them)
            _lib.check(lib.sp_mesh_render(_lib.ptr(v), _lib.ptr(c), M, _lib.ptr(f), F, _lib.ptr(normals), _lib.ptr(views), V, H, W, viz.Z_MIN, 0,
                                          _lib.ptr(scratch), _lib.ptr(keys), *(_lib.ptr(out[k]) for k in OUTPUTS), _lib.stream_ptr()), "sp_mesh_render")
        say(f"\n{title}: {F} faces, {M} vertices")
        shipped, timed = None, []
        for name, lib in libs:
            call(lib)
            torch.cuda.synchronize()
            words = scratch[:3].tolist()
            got = {k: out[k].clone() for k in OUTPUTS}
            if shipped is None:
                shipped = got
                hits = int((got['index'] >= 0).sum())
                say(f"  {hits} of {V * H * W} pixels hit, {int(torch.unique(got['index']).numel()) - int(hits < V * H * W)} faces win a pixel")
            else:
                same = all(torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                                       shipped[k].view(torch.int32) if shipped[k].dtype == torch.float32 else shipped[k]) for k in ('depth', 'image', 'index'))
                assert same, f"{name}: the outputs differ from the shipped library's"
            if words[1] or words[2]:
                say(f"  {name:10s} {words[0]} items; keys offered {words[1]}, atomics issued {words[2]} ({words[2] / max(words[1], 1):.3f} of offered; "
                    f"{hits} pixels hit)")
            else:
                timed.append((name, lib, words[0]))
        times = {name: [] for name, _, _ in timed}
        for _ in range(2):
            for _, lib, _ in timed:
                call(lib)
        for _ in range(args.rounds):
            for name, lib, _ in timed:
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.reps):
                    call(lib)
                end.record()
                end.synchronize()
                times[name].append(start.elapsed_time(end) / args.reps)
        count_bytes = V * F * (12 + 8) + M * 12
        for name, _, items in timed:
            t = np.array(times[name])
            med = float(np.median(t))
            say(f"  {name:10s} {med:8.3f} ms ({t.min():.3f} - {t.max():.3f})   {items} items, {items / med / 1e3:8.2f} M items/s, {V * H * W / med / 1e3:8.2f} M pixels/s; "
                f"count pass: {count_bytes / 1e6:.1f} MB at least, {count_bytes / med / 1e6:.1f} GB/s if it were the whole call")
        return shipped

    v, f, c = room(args.faces)
    fine = (T(v), T(f), T(c))
    if "a" in args.cases:
        first = run_case("(a) the tessellated room", *fine)
    if "b" in args.cases:
        depth = viz.mesh_render(*fine[:2], Ks, poses, H, W, index=False)['depth']
        lo, hi = tuple(-0.5 * s - 0.1 for s in ROOM), tuple(0.5 * s + 0.1 for s in ROOM)
        vol = results.fuse_tsdf(depth, Ks, poses, 0.025, bounds=(lo, hi))
        mesh = results.extract_mesh(vol)
        run_case(f"(b) extract_mesh of the room fused from (a)'s depth ({'x'.join(str(n) for n in vol['dims'])} nodes of 2.5 cm)",
                 mesh['points'], mesh['faces'], mesh['colours'])
        t = []
        for r in range(args.rounds + 1):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            surface = results.render_surface(vol, Ks, poses, (H, W), 6.0)
            end.record()
            end.synchronize()
            if r:
                t.append(start.elapsed_time(end))
        say(f"  context    {float(np.median(t)):8.3f} ms ({min(t):.3f} - {max(t):.3f})   render_surface on the volume, z_max 6 m, one sample per voxel: "
            f"{int((surface['index'] >= 0).sum())} pixels hit (another algorithm, not a bar)")
    if "c" in args.cases:
        v, f, c = room(12)
        run_case("(c) the room as 12 triangles", T(v), T(f), T(c))
    for line in kernel_stats_lines(args.kernel_stats):
        say(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
