#!/usr/bin/env python
"""Developer tool: one sha256 per output tensor of the map entry points (csrc/sp_views.hip, sp_results.hip, sp_fuse.hip, sp_tsdf.hip,
sp_raycast.hip, sp_mesh_render.hip through ``tool/viz.py`` and ``odometery/results.py``) on the small cases the tests define.  Every
output is an integer, decided by integer maxima, or one thread's float arithmetic in a fixed order, so two builds that compute the same
give the same listing, line for line: run it on both (``SP_HIP_LIB`` names the library) and compare.

Cases: map_render_ref posed / collide / duplicates in both modes; map_splat_ref splat_posed / splat_views17 / splat_edges; map_surfel_ref's
four cases at cull 0 and 1; tsdf_ref's main case integrated into a fresh volume, and that volume ray-cast from its own three cameras;
mesh_render_ref's mixed, skewed and strip meshes with face normals and, where the mesh has them, colours; map_consistency_ref posed /
owners / many_views / collide at windows 0, 1, 2; its keyframes through ``keyframe_depths``; the lift cases; map_fuse_ref's random case
at every setting and at Q = 70001; ``metrics_inputs``; the scene of tests/test_gpu_map_points.py at strides 1 and 3.  Capacity buffers
are trimmed to their counts.

    python tools/map_bits.py [--out listing.txt]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINES = []


def put(name, t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t))
    LINES.append(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {name} {a.dtype} {list(a.shape)}")


def put_all(name, out, keys=None):
    for k in keys or sorted(out):
        if out[k] is not None:
            put(f"{name}.{k}", out[k])


def main():
    import torch
    import map_consistency_ref as cons_ref
    import map_fuse_ref as fuse_ref
    import map_render_ref as render_ref
    import map_splat_ref as splat_ref
    import map_surfel_ref as surfel_ref
    import mesh_render_ref
    import test_gpu_map_points as points_test
    import tsdf_ref
    from gpu_util import T
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the map kernels need a GPU"
    eye = np.eye(4, dtype=np.float32)[None]

    for name, c in (("posed", render_ref.case_posed()), ("collide", render_ref.case_collide()), ("duplicates", render_ref.case_duplicates()[0])):
        for mode in (0, 1):
            out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', eye)), c['H'], c['W'], depth_buffer=bool(mode))
            put_all(f"render.{name}.mode{mode}", out)
    for name in ("splat_posed", "splat_views17", "splat_edges"):
        c = splat_ref.CASES[name]()
        out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', eye)), c['H'], c['W'], depth_buffer=True,
                               radii=T(c['radii']), max_px=c['max_px'])
        put_all(f"render.{name}", out)
    for name, make in surfel_ref.CASES.items():
        c = make()
        for cull in (0, 1):
            out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', eye)), c['H'], c['W'], depth_buffer=True,
                                   radii=T(c['radii']), max_px=c['max_px'], normals=T(c['normals']), cull=bool(cull))
            put_all(f"render.{name}.cull{cull}", out)
    c = tsdf_ref.case_main()
    nx, ny, nz = c['dims']
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    vol = dict(tsdf=zeros(nz, ny, nx), weight=zeros(nz, ny, nx), colour=zeros(nz, ny, nx, 3), origin=c['origin'], voxel=c['voxel'], trunc=c['trunc'],
               dims=c['dims'])
    viz.tsdf_integrate(vol, T(c['depth']), T(c['Ks']), T(c['poses']), images=T(c['images']), z_min=c['z_min'], depth_max=c['depth_max'])
    put_all("tsdf.main", vol, keys=('tsdf', 'weight', 'colour'))
    put_all("tsdf.main.raycast", viz.tsdf_raycast(vol, T(c['Ks']), T(c['poses']), c['H'], c['W'], 3.0, z_min=0.0, step=0.125))
    for name in ("mixed", "skewed", "strip"):
        mesh, Ks, poses, h, w = mesh_render_ref.cases()[name]
        rec = viz.mesh_faces(T(mesh['vertices']), T(mesh['faces']))
        out = viz.mesh_render(T(mesh['vertices']), T(mesh['faces']), T(Ks.astype(np.float32)), T(poses.astype(np.float32)), h, w,
                              colours=None if mesh['colours'] is None else T(mesh['colours']), face_normals=rec['normals'])
        put_all(f"mesh_render.{name}", out)
    for name, make in cons_ref.RANDOM_CASES.items():
        c = make()
        own = lambda key: None if c.get(key) is None else T(c[key])
        for window in (0, 1, 2):
            put(f"consistency.{name}.window{window}", viz.map_consistency(T(c['points']), T(c['K']), T(c['poses']), T(c['depth']), owner=own('owner'),
                                                                          view_owner=own('view_owner'), tol=c['tol'], window=window))
    cases = cons_ref.case_keyframes()
    kfs = [KeyFrame(T(k['image']), T(k['K']), T(k['L']), T(k['keypoints']), T(k['masks'])) for k in cases]
    put_all("keyframe_depths", viz.keyframe_depths(kfs, [T(k['kld']) for k in cases]))
    for name in ("lift_case_small", "lift_case_single", "lift_case_blocks", "lift_case_blocks_odd"):
        depth, K, poses, image = getattr(render_ref, name)()
        out = viz.lift_depth_images(T(depth), T(K), T(poses), T(image))
        n = int(out['offsets'][-1])
        put_all(f"lift.{name}", dict(out, points=out['points'][:n], colours=out['colours'][:n], pixel=out['pixel'][:n]))
    fuse_cases = [(f"setting{k}", fuse_ref.case_random(), s) for k, s in enumerate(fuse_ref.SETTINGS)]
    fuse_cases.append(("Q70001", fuse_ref.case_random(70001), fuse_ref.SETTINGS[2]))
    for name, (p, c), (voxel, origin) in fuse_cases:
        out = viz.fuse_points(T(p), T(c), voxel=voxel, origin=origin)
        M = int(out['n'])
        put_all(f"fuse.{name}", dict(out, **{k: out[k][:M] for k in ('points', 'colours', 'count', 'first')}))
    for V, H, W in ((3, 19, 23), (1, 64, 80)):
        rendered, target, index = splat_ref.metrics_inputs(V, H, W, 204 + V)
        put(f"image_metrics.{V}x{H}x{W}", viz.image_metrics(T(rendered), T(target), T(index)))
    kfs, klds, _ = points_test._scene()
    rng = np.random.default_rng(7)
    poses = np.stack([points_test._pose(rng) for _ in kfs])
    for stride in (1, 3):
        put_all(f"keyframe_points.stride{stride}", results.keyframe_points(kfs, klds, T(poses), stride=stride))
    torch.cuda.synchronize()
    text = "\n".join(LINES) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
