#!/usr/bin/env python
"""Developer tool: time of the map surfaces (csrc/sp_tsdf.hip: sp_tsdf_integrate, sp_tsdf_mesh) on the GPU.

ONE shape, chosen as a map a user would fuse: a volume of 256 x 256 x 256 nodes of 2 cm (a 5.12 m cube, 2^24 nodes, with colour: 320 MiB
of state) and 16 keyframes of 480 x 640 on an arc in front of a slanted plane through the cube's middle, truncation 4 voxels.

Per line the time of ONE call on preallocated buffers, HIP events around blocks of calls, warm-up first, then the median (min - max) over
alternating rounds.  The integrate starts every block of calls from the same cleared volume (a ``zero_`` of the state is inside the timed
block for both contestants and is timed on its own, so that it can be taken off).

The yardstick of the integrate, timed in the same run on the same card: the same rule written with torch ops -- float64 geometry, float32
update, view after view -- as a user would write it today.  Its result is compared with the kernel's bit for bit and the number of
differing words is printed (torch rounds every operation on its own too; its float64 division need not be the kernel's).

The integrate's bytes: the volume state (tsdf, weight, three colours: 20 bytes per node) read once and written once, plus the depth
images and the colour images read once -- gathers that the caches serve, counted once.  They are stated against the HBM peak of the
MI355X: 8.0 TB/s by the data sheet, 6.29 TB/s as a float4 copy reaches it.

    python tools/tsdf_bench.py [--out profiles/tsdf.txt] [--rounds 5] [--nodes 256] [--views 16]
    python tools/tsdf_bench.py --dry          (no GPU: the scene and the torch rule at a tiny size on the CPU, against tests/tsdf_ref.py)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                       # bytes per second: the data sheet, a measured float4 copy


def make_scene(n, V, H, W, voxel):
    """A cube of n^3 nodes whose middle is (0, 0, 3); V cameras on an arc of radius 3 around the middle, looking at it; the depth images
    of the plane 0.2 x + 0.1 y + z = 3 through the middle; random colour images."""
    import tsdf_ref as ref
    half = n * voxel / 2
    origin = (-half, -half, 3.0 - half)
    f = 0.8 * W
    K = np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], np.float32)
    poses = []
    for k in range(V):
        a = 0.08 * (k - (V - 1) / 2)
        poses.append(ref.look_at((3.0 * np.sin(a), 0.05 * (k % 3 - 1), 3.0 - 3.0 * np.cos(a)), (0.0, 0.0, 3.0)))
    poses = np.stack(poses)
    Ks = np.tile(K, (V, 1, 1))
    depth = np.stack([ref.plane_depth(K, poses[k], H, W, (0.2, 0.1, 1.0), 3.0) for k in range(V)])
    images = np.random.default_rng(3).uniform(0.0, 1.0, (V, 3, H, W)).astype(np.float32)
    return dict(dims=(n, n, n), voxel=voxel, origin=origin, trunc=4 * voxel, z_min=1e-6, depth_max=float("inf"), H=H, W=W, Ks=Ks, poses=poses,
                depth=depth, images=images)


def torch_integrate(vol, depth, images, Ks, poses, z_min, depth_max):
    """sp_tsdf_integrate's rule (include/sp_hip.h) with torch ops, view after view, in place."""
    import torch
    tsdf, weight, colour = vol['tsdf'], vol['weight'], vol['colour']
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
    voxel, trunc, zmin = f32(vol['voxel']), f32(vol['trunc']), f32(z_min)
    centre = lambda n, o: (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * voxel + f32(o)
    px, py, pz = centre(nx, vol['origin'][0])[None, None, :], centre(ny, vol['origin'][1])[None, :, None], centre(nz, vol['origin'][2])[:, None, None]
    V, H, W = depth.shape
    for v in range(V):
        T, K = poses[v].double(), Ks[v].double()
        d0, d1, d2 = px - T[0, 3], py - T[1, 3], pz - T[2, 3]
        x = (T[0, 0] * d0 + T[1, 0] * d1) + T[2, 0] * d2
        y = (T[0, 1] * d0 + T[1, 1] * d1) + T[2, 1] * d2
        z = (T[0, 2] * d0 + T[1, 2] * d1) + T[2, 2] * d2
        col, row = torch.floor((x * K[0, 0]) / z + K[0, 2] + 0.5), torch.floor((y * K[1, 1]) / z + K[1, 2] + 0.5)
        inside = (z > zmin) & (col >= 0) & (col < W) & (row >= 0) & (row < H)              # (NaN and inf fail the comparisons)
        pix = torch.where(inside, row * W + col, torch.zeros_like(col)).long()
        D = depth[v].reshape(-1)[pix]
        sdf = D.double() - z
        kept = inside & torch.isfinite(D) & (D > 0) & (D <= depth_max) & ~(sdf < -trunc)
        s = torch.clamp(sdf / trunc, max=1.0).float()
        wn = weight + 1.0
        new = (tsdf * weight + s) / wn
        if colour is not None:
            e = torch.nan_to_num(images[v].reshape(3, -1)[:, pix], nan=0.0, posinf=float("inf"), neginf=-float("inf"))
            colour.copy_(torch.where(kept[..., None], (colour * weight[..., None] + e.permute(1, 2, 3, 0)) / wn[..., None], colour))
        tsdf.copy_(torch.where(kept, new, tsdf))
        weight.copy_(torch.where(kept, wn, weight))
    return vol


def fresh(scene, dev):
    import torch
    nx, ny, nz = scene['dims']
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    return dict(tsdf=z(nz, ny, nx), weight=z(nz, ny, nx), colour=z(nz, ny, nx, 3), origin=scene['origin'], voxel=scene['voxel'], trunc=scene['trunc'],
                dims=scene['dims'])


def clear(vol):
    for k in ('tsdf', 'weight', 'colour'):
        vol[k].zero_()


def integrate_bytes(nodes, V, H, W):
    """(the state read and written once, the depth and colour images read once), in bytes."""
    return 2 * 20 * nodes, V * H * W * 4 * (1 + 3)


def dry():
    import torch
    import tsdf_ref as ref
    scene = make_scene(12, 3, 24, 32, 0.25)
    vol = torch_integrate(fresh(scene, "cpu"), *(torch.from_numpy(scene[k]) for k in ('depth', 'images', 'Ks', 'poses')), scene['z_min'], scene['depth_max'])
    want = ref.reference(scene)
    same = all(np.array_equal(vol[k].numpy().view(np.uint32), want[k].view(np.uint32)) for k in ('tsdf', 'weight', 'colour'))
    state, views = integrate_bytes(256 ** 3, 16, 480, 640)
    print(f"dry run on the CPU (no time is measured): the torch rule equals tests/tsdf_ref.py bit for bit: {same}; {int((want['weight'] > 0).sum())} of "
          f"{want['weight'].size} nodes updated; at 256^3 nodes and 16 views of 480x640 the call moves {state / 2 ** 20:.0f} MiB of state and {views / 2 ** 20:.0f} MiB of images")
    assert same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    if args.dry:
        return dry()
    import torch
    from tools.map_render_bench import fmt, timed
    from super_primitive_amd import _lib
    from super_primitive_amd.tool import viz
    assert torch.cuda.is_available(), "the timings need a GPU"
    dev = torch.device("cuda:0")
    n, V, H, W, voxel = args.nodes, args.views, 480, 640, 0.02
    scene = make_scene(n, V, H, W, voxel)
    depth, images, Ks, poses = (torch.from_numpy(scene[k]).to(dev) for k in ('depth', 'images', 'Ks', 'poses'))
    vol, other = fresh(scene, dev), fresh(scene, dev)

    def kernel():
        clear(vol)
        viz.tsdf_integrate(vol, depth, Ks, poses, images=images, z_min=scene['z_min'], depth_max=scene['depth_max'])

    def yardstick():
        clear(other)
        torch_integrate(other, depth, images, Ks, poses, scene['z_min'], scene['depth_max'])

    kernel()
    yardstick()
    torch.cuda.synchronize()
    differ = {k: int((vol[k].view(torch.int32) != other[k].view(torch.int32)).sum()) for k in ('tsdf', 'weight', 'colour')}
    updated, wmax = int((vol['weight'] > 0).sum()), float(vol['weight'].max())
    t_k, t_y, t_c = timed([kernel, yardstick, lambda: clear(vol)], args.rounds, block=3)
    net = t_k[0] - t_c[0]
    nodes = n ** 3
    state, views = integrate_bytes(nodes, V, H, W)
    lines = [f"map surfaces, ms per call: median (min - max) over {args.rounds} alternating rounds, HIP events around blocks of 3 calls",
             f"volume {n} x {n} x {n} nodes of {voxel} m ({nodes} nodes, tsdf + weight + colour = {20 * nodes / 2 ** 20:.0f} MiB), truncation {scene['trunc']:.2f} m; "
             f"{V} views of {H} x {W} on an arc in front of a slanted plane; {updated} nodes updated, largest weight {wmax:.0f}",
             f"sp_tsdf_integrate + clear : {fmt(t_k)}",
             f"torch rule + clear        : {fmt(t_y)}",
             f"clear (three zero_) alone : {fmt(t_c)}",
             f"sp_tsdf_integrate alone   : {net:.3f} ms = {nodes * V / (net * 1e-3) / 1e9:.2f} G node-views / s; torch rule alone {t_y[0] - t_c[0]:.3f} ms: "
             f"{(t_y[0] - t_c[0]) / net:.1f} x the kernel",
             f"words that differ between the two results (of {nodes} / {nodes} / {3 * nodes}): tsdf {differ['tsdf']}, weight {differ['weight']}, colour {differ['colour']}",
             f"bytes of the call: state read and written once {state / 1e6:.0f} MB + depth and colour images {views / 1e6:.0f} MB = {(state + views) / 1e6:.0f} MB; "
             f"at {HBM_SPEC / 1e12:.1f} TB/s (data sheet) that is {(state + views) / HBM_SPEC * 1e3:.3f} ms, at {HBM_COPY / 1e12:.2f} TB/s (a float4 copy) "
             f"{(state + views) / HBM_COPY * 1e3:.3f} ms",
             f"achieved {(state + views) / (net * 1e-3) / 1e12:.3f} TB/s = {(state + views) / (net * 1e-3) / HBM_SPEC:.3f} of the data sheet, "
             f"{(state + views) / (net * 1e-3) / HBM_COPY:.3f} of the copy; the call takes {net / ((state + views) / HBM_COPY * 1e3):.1f} x its bandwidth bound: "
             f"{V} projections per node in float64, two divisions each, are what it spends"]
    # ---- the mesh of the fused volume
    kernel()
    lib = _lib.load()
    scratch = torch.empty(lib.sp_tsdf_mesh_scratch_bytes(n, n, n) // 4, dtype=torch.int32, device=dev)
    n_out = torch.empty(2, dtype=torch.int64, device=dev)
    o = [float(np.float32(a)) for a in scene['origin']]

    def mesh(nv, nf, vertices, colours, faces):
        _lib.check(lib.sp_tsdf_mesh(_lib.ptr(vol['tsdf']), _lib.ptr(vol['weight']), _lib.ptr(vol['colour']), n, n, n, float(np.float32(voxel)), o[0], o[1], o[2],
                                    1.0, _lib.ptr(scratch), nv, nf, _lib.ptr(vertices), _lib.ptr(colours), _lib.ptr(faces), _lib.ptr(n_out),
                                    _lib.stream_ptr()), "sp_tsdf_mesh")
    mesh(0, 0, None, None, None)
    nv, nf = n_out.tolist()
    vertices, colours, faces = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev), torch.empty(nf, 3, dtype=torch.int32, device=dev)
    t_count, t_fill = timed([lambda: mesh(0, 0, None, None, None), lambda: mesh(nv, nf, vertices, colours, faces)], args.rounds, block=3)
    t_whole = timed([lambda: viz.tsdf_mesh(vol)], args.rounds, block=1)[0]
    lines += [f"sp_tsdf_mesh of that volume: {nv} vertices, {nf} faces, scratch {scratch.numel() * 4 / 2 ** 20:.0f} MiB",
              f"counting call (3 launches)        : {fmt(t_count)}",
              f"filling call (5 launches)         : {fmt(t_fill)} = {nodes / (t_fill[0] * 1e-3) / 1e9:.2f} G nodes / s",
              f"viz.tsdf_mesh (both, allocations, the host read of the counts): {fmt(t_whole)}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
