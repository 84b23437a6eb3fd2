#!/usr/bin/env python
"""Developer tool: time of the surface views (csrc/sp_raycast.hip: sp_tsdf_raycast) on the GPU.

ONE shape, the map of tools/tsdf_bench.py: its volume of 256 x 256 x 256 nodes of 2 cm with colour, fused by sp_tsdf_integrate from its 16
keyframes of 480 x 640 on an arc in front of a slanted plane, then ray-cast back into those 16 views: one ray per pixel, a sample every
voxel of camera depth from 1e-6 to 6 m (301 samples: the far corner of the cube lies within reach), all four outputs.

Per line the time of ONE call on preallocated buffers, HIP events around blocks of calls, warm-up first, then the median (min - max) over
alternating rounds.  Rays per second count every pixel; samples per second count the samples THE RULE defines for a ray -- k = 0 up to
the one that ends it, or all of them -- although the kernel leaves out those it can prove to lie outside the volume.

The yardstick, timed in the same run on the same card: the same rule written with torch ops -- float64 arithmetic, one gather per corner,
every k marched for all rays at once -- as a user would write it today.  Its four outputs are compared with the kernel's word for word
and the number of differing words is printed (torch rounds every operation on its own too; its float64 division and square root need
not be the kernel's).

``--lib PATH`` names another build of the library whose tile order differs (``make -C super_primitive_amd/csrc
RAYCAST_FLAGS="-DSP_RAYCAST_XCD_CHUNKS=0"``, the library copied aside): its ``sp_tsdf_raycast`` is timed in the same rounds, alternating
with the shipped one -- the A/B that decides the shipped order.  Its outputs must equal the shipped library's.

    python tools/tsdf_raycast_bench.py [--out profiles/tsdf_raycast.txt] [--rounds 5] [--nodes 256] [--views 16] [--lib other/libsp_hip.so]
    python tools/tsdf_raycast_bench.py --dry      (no GPU: the torch rule at a tiny size on the CPU, against tests/tsdf_raycast_ref.py)"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUTPUTS = ('depth', 'normals', 'image', 'index')


def torch_raycast(tsdf, weight, colour, voxel, origin, min_weight, Ks, poses, H, W, z_start, step, n_steps):
    """sp_tsdf_raycast's rule (include/sp_hip.h) with torch ops, all rays of all views at once, every k marched.  Returns depth, normals,
    image, index as the kernel writes them, and ``samples``: per ray the number of samples the rule defines for it."""
    import torch
    dev = tsdf.device
    nz, ny, nx = tsdf.shape
    V = poses.shape[0]
    f32 = lambda x: float(torch.tensor(float(x), dtype=torch.float32))
    vx, o, z0, st = f32(voxel), [f32(a) for a in origin], f32(z_start), f32(step)
    node_ok = ((weight >= f32(min_weight)) & torch.isfinite(tsdf)).reshape(-1)
    flat, flat_colour = tsdf.reshape(-1), None if colour is None else colour.reshape(-1, 3)
    Kd, T = Ks.double(), poses.double()
    rows = torch.arange(H, dtype=torch.float64, device=dev)[None, :, None].expand(V, H, W)
    cols = torch.arange(W, dtype=torch.float64, device=dev)[None, None, :].expand(V, H, W)
    xr = ((cols - Kd[:, 0, 2, None, None]) / Kd[:, 0, 0, None, None]).reshape(-1)
    yr = ((rows - Kd[:, 1, 2, None, None]) / Kd[:, 1, 1, None, None]).reshape(-1)
    eye = torch.eye(4, dtype=torch.float64, device=dev)[:3]
    ident = (T[:, :3] == eye).all(dim=2).all(dim=1)[:, None, None].expand(V, H, W).reshape(-1)
    R = [[T[:, a, b, None, None].expand(V, H, W).reshape(-1) for b in range(4)] for a in range(3)]

    def world(z):
        q = (xr * z, yr * z, z + torch.zeros_like(xr))
        return tuple(torch.where(ident, q[a], ((R[a][0] * q[0] + R[a][1] * q[1]) + R[a][2] * q[2]) + R[a][3]) for a in range(3))

    def lerp3(corner, f):
        x = [corner[2 * k] + f[0] * (corner[2 * k + 1] - corner[2 * k]) for k in range(4)]
        y = [x[2 * k] + f[1] * (x[2 * k + 1] - x[2 * k]) for k in range(2)]
        return y[0] + f[2] * (y[1] - y[0])

    def sample(p, with_colour=False):
        g = [((p[a] - o[a]) / vx) - 0.5 for a in range(3)]
        i = [torch.floor(ga) for ga in g]
        inside = torch.ones_like(xr, dtype=torch.bool)
        for a, n in enumerate((nx, ny, nz)):
            inside &= (i[a] >= 0) & (i[a] + 1 <= n - 1)                        # (NaN and inf fail)
        ii = [torch.where(inside, ia, torch.zeros_like(ia)).long() for ia in i]
        f = [torch.where(inside, ga - ia, torch.zeros_like(ga)) for ga, ia in zip(g, i)]
        node = (ii[2] * ny + ii[1]) * nx + ii[0]
        corners = [node + (c & 1) + ((c >> 1) & 1) * nx + (c >> 2) * nx * ny for c in range(8)]
        ok = inside.clone()
        for c in corners:
            ok &= node_ok[c]
        F = torch.where(ok, lerp3([flat[c].double() for c in corners], f), torch.zeros_like(xr))
        if not with_colour:
            return ok, F, node
        C = [lerp3([flat_colour[c, ch].double() for c in corners], f) for ch in range(3)]
        return ok, F, node, C

    running = torch.ones_like(xr, dtype=torch.bool)
    hit = torch.zeros_like(running)
    prev_ok, prev_F = torch.zeros_like(running), torch.zeros_like(xr)
    k_end = torch.full_like(xr, -1, dtype=torch.int64)
    F_before, F_end = torch.zeros_like(xr), torch.zeros_like(xr)
    for k in range(n_steps):
        ok, F, _ = sample(world(z0 + float(k) * st))
        ends = running & ok & (F < 0)
        now = ends & prev_ok & (prev_F >= 0) if k >= 1 else torch.zeros_like(ends)
        hit |= now
        F_before, F_end = torch.where(now, prev_F, F_before), torch.where(now, F, F_end)
        k_end = torch.where(ends, torch.full_like(k_end, k), k_end)
        running &= ~ends
        prev_ok, prev_F = ok, F
    samples = torch.where(k_end >= 0, k_end + 1, torch.full_like(k_end, n_steps))
    t = F_before / (F_before - F_end)
    z_before, z_at = z0 + (k_end - 1).double() * st, z0 + k_end.double() * st
    zs = t * st + z_before
    nan = torch.full_like(xr, float("nan"), dtype=torch.float32)
    depth = torch.where(hit, zs.float(), torch.zeros_like(nan))
    at_end = sample(world(z_at), with_colour=colour is not None)
    index = torch.where(hit, at_end[2], torch.full_like(k_end, -1)).int()
    image = None
    if colour is not None:
        before = sample(world(z_before), with_colour=True)
        chans = []
        for ch in range(3):
            c = (before[3][ch] + t * (at_end[3][ch] - before[3][ch])).float().double() * 255.0
            c = torch.where(c > 0, torch.clamp(c, max=255.0), torch.zeros_like(c))                 # (NaN fails c > 0)
            chans.append(torch.where(hit, torch.trunc(c), torch.zeros_like(c)).to(torch.uint8))
        image = torch.stack(chans, dim=-1).reshape(V, H, W, 3)
    p = world(zs)
    g, all_ok = [], hit.clone()
    for a in range(3):
        plus = sample(tuple(p[b] + vx if b == a else p[b] for b in range(3)))
        minus = sample(tuple(p[b] - vx if b == a else p[b] for b in range(3)))
        all_ok &= plus[0] & minus[0]
        g.append(plus[1] - minus[1])
    length = torch.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    good = all_ok & torch.isfinite(length) & (length > 0)
    normals = torch.stack([torch.where(good, (ga / length).float(), nan) for ga in g], dim=-1).reshape(V, H, W, 3)
    return dict(depth=depth.reshape(V, H, W), normals=normals, image=image, index=index.reshape(V, H, W), samples=samples)


def words_that_differ(a, b):
    """Per output the number of differing words (the NaNs of the normals by isnan agreement)."""
    import torch
    out = {}
    for key in OUTPUTS:
        x, y = a[key], b[key]
        if key == 'normals':
            nx_, ny_ = torch.isnan(x), torch.isnan(y)
            out[key] = int((nx_ != ny_).sum()) + int(((x.view(torch.int32) != y.view(torch.int32)) & ~nx_ & ~ny_).sum())
        elif x.dtype == torch.float32:
            out[key] = int((x.view(torch.int32) != y.view(torch.int32)).sum())
        else:
            out[key] = int((x != y).sum())
    return out


def dry():
    import torch
    import tsdf_raycast_ref as ref
    case, vol = ref.main_volume()
    t = torch.from_numpy
    same = True
    for name, (K, pose, steps) in ref.cameras().items():
        want = ref.raycast(vol, K[None], pose[None], case['H'], case['W'], **steps)
        got = torch_raycast(t(vol.tsdf), t(vol.weight), t(vol.colour), vol.voxel, vol.origin, vol.min_weight, t(K[None]), t(pose[None]), case['H'], case['W'],
                            **steps)
        differ = words_that_differ(got, {k: t(want[k]) for k in OUTPUTS})
        print(f"dry run on the CPU (no time is measured): camera '{name}': words of the torch rule that differ from tests/tsdf_raycast_ref.py: {differ}; "
              f"{want['counts'][0]['hits']} hits")
        same = same and not any(differ.values())
    assert same


def load_other(path):
    from super_primitive_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.sp_tsdf_raycast.argtypes = _lib.SIGNATURES["sp_tsdf_raycast"]
    lib.sp_tsdf_raycast.restype = ctypes.c_int
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--lib", help="another build of libsp_hip.so (another tile order) whose sp_tsdf_raycast is timed beside the shipped one")
    ap.add_argument("--dry", action="store_true")
    args = ap.parse_args()
    if args.dry:
        return dry()
    import torch
    from tools.map_render_bench import fmt, timed
    from tools.tsdf_bench import fresh, make_scene
    from super_primitive_amd import _lib
    from super_primitive_amd.tool import viz
    assert torch.cuda.is_available(), "the timings need a GPU"
    dev = torch.device("cuda:0")
    n, V, H, W, voxel, z_max = args.nodes, args.views, 480, 640, 0.02, 6.0
    scene = make_scene(n, V, H, W, voxel)
    depth, images, Ks, poses = (torch.from_numpy(scene[k]).to(dev) for k in ('depth', 'images', 'Ks', 'poses'))
    vol = viz.tsdf_integrate(fresh(scene, dev), depth, Ks, poses, images=images, z_min=scene['z_min'], depth_max=scene['depth_max'])
    vx = float(np.float32(voxel))
    n_steps = int(np.ceil((z_max - viz.Z_MIN) / vx)) + 1
    o = [float(np.float32(a)) for a in scene['origin']]
    views = viz._views(Ks, poses, V)
    lib = _lib.load()

    def buffers():
        return dict(depth=torch.empty(V, H, W, device=dev), normals=torch.empty(V, H, W, 3, device=dev),
                    image=torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev), index=torch.empty(V, H, W, dtype=torch.int32, device=dev))

    def call(which, out):
        _lib.check(which.sp_tsdf_raycast(_lib.ptr(vol['tsdf']), _lib.ptr(vol['weight']), _lib.ptr(vol['colour']), n, n, n, vx, o[0], o[1], o[2], 1.0,
                                         _lib.ptr(views), V, H, W, viz.Z_MIN, vx, n_steps, *(_lib.ptr(out[k]) for k in OUTPUTS), _lib.stream_ptr()),
                   "sp_tsdf_raycast")
    mine, theirs = buffers(), buffers()
    call(lib, mine)
    rule = {}

    def yardstick():
        rule.update(torch_raycast(vol['tsdf'], vol['weight'], vol['colour'], voxel, scene['origin'], 1.0, Ks, poses, H, W, viz.Z_MIN, vx, n_steps))
    yardstick()
    torch.cuda.synchronize()
    differ = words_that_differ(mine, rule)
    rays, hits, samples = V * H * W, int((mine['index'] >= 0).sum()), int(rule['samples'].sum())
    nan_normals = int((torch.isnan(mine['normals']).any(dim=-1) & (mine['index'] >= 0)).sum())
    t_k = timed([lambda: call(lib, mine)], args.rounds, block=5)[0]
    t_y = timed([yardstick], min(args.rounds, 3), block=1)[0]
    nodes = n ** 3
    lines = [f"surface views, ms per call: median (min - max) over alternating rounds, HIP events around blocks of calls (5 for the kernel, 1 for the torch rule)",
             f"volume {n} x {n} x {n} nodes of {voxel} m (tsdf + weight {8 * nodes / 2 ** 20:.0f} MiB, colour {12 * nodes / 2 ** 20:.0f} MiB) fused from {V} views of "
             f"{H} x {W}; ray-cast into the same {V} views, {n_steps} samples a ray from {viz.Z_MIN} m, step {voxel} m; depth, normals, image and index",
             f"{rays} rays: {hits} hits ({nan_normals} of them without a normal), {samples} samples by the rule ({samples / rays:.1f} a ray)",
             f"sp_tsdf_raycast : {fmt(t_k)} = {rays / (t_k[0] * 1e-3) / 1e9:.3f} G rays / s, {samples / (t_k[0] * 1e-3) / 1e9:.2f} G samples / s",
             f"torch rule      : {fmt(t_y)} = {t_y[0] / t_k[0]:.0f} x the kernel",
             f"words that differ between the two (of {rays} / {3 * rays} / {3 * rays} / {rays}): depth {differ['depth']}, normals {differ['normals']}, "
             f"image {differ['image']}, index {differ['index']}"]
    if args.lib:
        other = load_other(args.lib)
        call(other, theirs)
        torch.cuda.synchronize()
        ab_differ = words_that_differ(mine, theirs)
        assert not any(ab_differ.values()), ab_differ
        t_a, t_b = timed([lambda: call(lib, mine), lambda: call(other, theirs)], args.rounds, block=5)
        name = os.path.basename(args.lib)
        lines += [f"tile order, the shipped library against {name} in the same rounds (alternating), identical outputs:",
                  f"shipped : {fmt(t_a)}",
                  f"other   : {fmt(t_b)} = {t_b[0] / t_a[0]:.3f} x the shipped"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
