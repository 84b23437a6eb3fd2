#!/usr/bin/env python
"""Developer tool: time of the mesh surfaces (csrc/sp_mesh.hip: sp_mesh_faces, sp_mesh_sample) on the GPU.

TWO meshes.  The first is the one a user would sample: the mesh ``sp_tsdf_mesh`` cuts out of the fused 256 x 256 x 256 volume of
tools/tsdf_bench.py (16 views of a slanted plane), sampled at the density that gives about ``--rows`` rows.  The second is synthetic:
``--small`` small triangles and, in their middle, ONE triangle that takes about ``--big-rows`` rows on its own -- the shape on which a sampler
with one thread per face would serialise.

Per line the time of ONE call on preallocated buffers, HIP events around blocks of calls, warm-up first, then the median (min - max) over
alternating rounds: the face pass (area, normals, state; no cross products), the counting call of the sampler (2 launches) and its filling
call (3 launches, all four outputs), and ``viz.mesh_sample`` as a user calls it (both calls, the allocations, the host read of the count).

The bytes the rule must move, each counted once (the gathers of vertices, colours and face normals are served by the caches):
    face pass      per face 12 (indices) + 36 (nine coordinates) + 8 + 12 + 1 (area, normal, state)
    filling call   per face 12 + 8 + 1 read and 8 written by the count, 36 + 36 + 12 gathered by the rows; per row 12 + 12 + 12 + 4 written
They are stated against the HBM peak of the MI355X: 8.0 TB/s by the data sheet, 6.29 TB/s as a float4 copy reaches it.

    python tools/mesh_sample_bench.py [--out profiles/mesh_sample.txt] [--rounds 5] [--nodes 256] [--rows 10000000] [--small 100000] [--big-rows 1000000]
    python tools/mesh_sample_bench.py --dry       (no GPU: the synthetic mesh at a tiny size through tests/mesh_ref.py on the CPU)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                       # bytes per second: the data sheet, a measured float4 copy


def dominated_mesh(small, seed=9):
    """``small`` triangles of side about 0.01 scattered in the unit cube and, as face small // 2, one triangle of area 0.5."""
    rng = np.random.default_rng(seed)
    F = small + 1
    tri = rng.uniform(0.0, 1.0, (F, 1, 3)) + rng.uniform(-0.005, 0.005, (F, 3, 3))
    tri[small // 2] = [[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]]
    vertices = tri.reshape(-1, 3).astype(np.float32)
    return vertices, np.arange(3 * F, dtype=np.int32).reshape(F, 3), rng.uniform(0.0, 1.0, (3 * F, 3)).astype(np.float32)


def faces_bytes(F):
    return F * (12 + 36 + 8 + 12 + 1)


def sample_bytes(F, N):
    return F * (12 + 8 + 1 + 8 + 36 + 36 + 12) + N * (12 + 12 + 12 + 4)


def rate_lines(what, t_ms, nbytes, rows, unit):
    s = t_ms * 1e-3
    return (f"{what}: {rows / s / 1e9:.3f} G {unit} / s; {nbytes / 1e6:.1f} MB at {HBM_SPEC / 1e12:.1f} TB/s (data sheet) are {nbytes / HBM_SPEC * 1e3:.4f} ms, at "
            f"{HBM_COPY / 1e12:.2f} TB/s (a float4 copy) {nbytes / HBM_COPY * 1e3:.4f} ms; achieved {nbytes / s / 1e12:.3f} TB/s = "
            f"{nbytes / s / HBM_SPEC:.3f} of the data sheet, {nbytes / s / HBM_COPY:.3f} of the copy")


def dry():
    import mesh_ref as ref
    v, f, c = dominated_mesh(200)
    rec = ref.face_records(v, f)
    density = 2000 / rec['area'][100]
    s = ref.sample(v, f, rec, density, 1, colours=c)
    print(f"dry run on the CPU (no time is measured): {len(f)} faces, states {rec['counts'].tolist()}, the large face holds {rec['area'][100] / rec['area'].sum():.4f} "
          f"of the area and takes {int(s['n'][100])} of {s['total']} rows; at 10^5 + 1 faces and 10^6 rows the face pass moves {faces_bytes(100001) / 1e6:.1f} MB and the "
          f"filling call {sample_bytes(100001, 10 ** 6) / 1e6:.1f} MB")
    assert rec['counts'][0] == len(f) and abs(int(s['n'][100]) - 2000) <= 1


def measure(name, vertices, faces, colours, rows, rounds, lines):
    import torch
    from tools.map_render_bench import fmt, timed
    from super_primitive_amd import _lib
    from super_primitive_amd.tool import viz
    lib = _lib.load()
    dev = vertices.device
    M, F = int(vertices.shape[0]), int(faces.shape[0])
    rec = viz.mesh_faces(vertices, faces)
    area_total = float(rec['area'].sum())
    counts = rec['summary'][:5].tolist()
    density = rows / area_total
    scratch = torch.empty(8 * lib.sp_mesh_sample_scratch_units(F), dtype=torch.int64, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)

    def face_pass():
        _lib.check(lib.sp_mesh_faces(_lib.ptr(vertices), M, _lib.ptr(faces), F, _lib.ptr(rec['area']), _lib.ptr(rec['normals']), _lib.ptr(rec['state']), None,
                                     _lib.ptr(rec['summary']), _lib.stream_ptr()), "sp_mesh_faces")

    def sample(cap, points, normals, cols, face):
        _lib.check(lib.sp_mesh_sample(_lib.ptr(vertices), _lib.ptr(colours), M, _lib.ptr(faces), F, _lib.ptr(rec['area']), _lib.ptr(rec['normals']),
                                      _lib.ptr(rec['state']), density, 1, _lib.ptr(scratch), cap, _lib.ptr(points), _lib.ptr(normals), _lib.ptr(cols),
                                      _lib.ptr(face), _lib.ptr(n_out), _lib.stream_ptr()), "sp_mesh_sample")
    sample(0, None, None, None, None)
    N = int(n_out.item())
    out = [torch.empty(N, 3, device=dev) for _ in range(3)] + [torch.empty(N, dtype=torch.int32, device=dev)]
    sample(N, *out)
    per_face = torch.bincount(out[3].long(), minlength=F)
    t_faces, t_count, t_fill = timed([face_pass, lambda: sample(0, None, None, None, None), lambda: sample(N, *out)], rounds, block=5)
    t_whole = timed([lambda: viz.mesh_sample(vertices, faces, rec, density, seed=1, colours=colours)], rounds, block=1)[0]
    again = [torch.empty_like(t) for t in out]
    sample(N, *again)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, again))
    lines += [f"{name}: {M} vertices, {F} faces (per state {counts}), total area {area_total:.6g}, density {density:.6g} -> {N} rows; the busiest face takes "
              f"{int(per_face.max())} rows, {int((per_face == 0).sum())} faces take none; scratch {scratch.numel() * 8 / 2 ** 20:.2f} MiB; two fills give the same bits: {same}",
              f"  sp_mesh_faces (1 launch, a 48-byte memset)   : {fmt(t_faces)} ms",
              "  " + rate_lines("    face pass", t_faces[0], faces_bytes(F), F, "faces"),
              f"  sp_mesh_sample, counting call (2 launches)   : {fmt(t_count)} ms",
              f"  sp_mesh_sample, filling call (3 launches)    : {fmt(t_fill)} ms",
              "  " + rate_lines("    filling call", t_fill[0], sample_bytes(F, N), N, "rows"),
              f"  viz.mesh_sample (both calls, allocations, the host read of the count): {fmt(t_whole)} ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--small", type=int, default=100_000)
    ap.add_argument("--big-rows", type=int, default=1_000_000)
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    if args.dry:
        return dry()
    import torch
    from tools.tsdf_bench import fresh, make_scene
    from super_primitive_amd.tool import viz
    assert torch.cuda.is_available(), "the timings need a GPU"
    dev = torch.device("cuda:0")
    lines = [f"mesh surfaces, ms per call: median (min - max) over {args.rounds} alternating rounds, HIP events around blocks of 5 calls"]
    n, V = args.nodes, 16
    scene = make_scene(n, V, 480, 640, 0.02)
    vol = fresh(scene, dev)
    viz.tsdf_integrate(vol, *(torch.from_numpy(scene[k]).to(dev) for k in ('depth', 'Ks', 'poses')), images=torch.from_numpy(scene['images']).to(dev),
                       z_min=scene['z_min'], depth_max=scene['depth_max'])
    mesh = viz.tsdf_mesh(vol)
    del vol
    measure(f"the mesh of the fused {n}^3 volume", mesh['vertices'], mesh['faces'], mesh['colours'], args.rows, args.rounds, lines)
    del mesh
    v, f, c = dominated_mesh(args.small)
    v, f, c = (torch.from_numpy(a).to(dev) for a in (v, f, c))
    rec = viz.mesh_faces(v, f)
    big = float(rec['area'][args.small // 2])
    # the density at which the one large face takes args.big_rows rows; the small ones share what their area gives them
    measure(f"{args.small} small triangles around one of area {big:.3f}", v, f, c, args.big_rows * float(rec['area'].sum()) / big, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
