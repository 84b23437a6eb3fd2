#!/usr/bin/env python
"""Developer tool: time of the map views (csrc/sp_views.hip) on the GPU.

Render: a 1.2-million-point cloud into V = 1 and V = 8 posed views at 224 x 288 and 480 x 640, in both modes -- ONE ``sp_render_views``
call on preallocated buffers (what ``tool.viz.render_views`` adds is three ``torch.empty`` and one ``cat``) -- and, for V = 8, eight
V = 1 calls.  Beside every line the same work with torch ops on the device, per view: the float64 projection, the bounds mask, then
``index_put_`` of the point index (mode 0; which of several writers of a pixel wins is not defined there) or ``scatter_reduce_(amax)``
on packed int64 keys (mode 1), and gathers of depth and colour at the winners.  The two give the same depth buffer (checked in mode 1).

Lift: 8 depth images of 480 x 640 with poses and colours through ONE ``sp_depth_lift`` call, against mask + ``nonzero`` + gathers + the
float64 formula in torch.

Per line: the bytes that must move (points read once, keys zeroed, keys read by the resolve pass, outputs written, the winners' colours
gathered; for the lift: depth read twice, image read once at the valid pixels, outputs written) over the time as a share of the HBM
peak (8 TB/s), and the kept (point, view) pairs -- an upper bound of the atomics issued: a point that already loses is skipped after a
plain load -- over the time.

Clock: HIP events around blocks of calls, warm-up of every shape first, then the median (min - max) over alternating rounds.

    python tools/map_render_bench.py [--out profiles/map_render.txt] [--rounds 7]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 1_200_000
HBM_PEAK = 8.0e12


def timed(fns, rounds, block):
    """ms per call of each fn: ``rounds`` alternating blocks of ``block`` calls, HIP events around every block: (median, min, max)."""
    import torch
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(block):
                fn()
            stop.record()
            torch.cuda.synchronize()
            times[k].append(start.elapsed_time(stop) / block)
    return [(float(np.median(t)), min(t), max(t)) for t in times]


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} - {t[2]:.3f})"


def make_scene(dev, V, H, W):
    """A cloud in the box [-2, 2] x [-1.5, 1.5] x [1.5, 5] and V cameras near the origin looking down +z."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(11)
    lo, hi = torch.tensor([-2.0, -1.5, 1.5]), torch.tensor([2.0, 1.5, 5.0])
    pts = (lo + (hi - lo) * torch.rand(Q, 3, generator=g)).to(dev)
    cols = torch.rand(Q, 3, generator=g).to(dev)
    f = 0.9 * W
    K = torch.tensor([[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], dtype=torch.float32, device=dev)
    poses = []
    for k in range(V):
        a = 0.06 * (k - (V - 1) / 2)
        T = torch.eye(4, dtype=torch.float64)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
        T[:3, 3] = torch.tensor([0.15 * k - 0.5, 0.02 * k, -0.1 * k])
        poses.append(T.float())
    return pts, cols, K, torch.stack(poses).to(dev)


def torch_project(pts, K, pose, H, W, z_test):
    import torch
    p = pts.double()
    R, t = pose[:3, :3].double(), pose[:3, 3].double()
    pc = (p - t) @ R                                        # R^T (p - t), row vectors
    z = pc[:, 2]
    u = pc[:, 0] * K[0, 0].double() / z + K[0, 2].double()
    v = pc[:, 1] * K[1, 1].double() / z + K[1, 2].double()
    keep = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    if z_test:
        keep &= z > 1e-6
    idx = torch.nonzero(keep).squeeze(1)
    lin = v[idx].long() * W + u[idx].long()
    return idx, lin, z[idx].float()


def torch_render(pts, cols, K, poses, H, W, mode):
    """The same outputs with torch ops, view by view."""
    import torch
    images, depths, indices = [], [], []
    for pose in poses:
        idx, lin, zf = torch_project(pts, K, pose, H, W, mode == 1)
        if mode == 0:
            index = torch.full((H * W,), -1, dtype=torch.int64, device=pts.device)
            index.index_put_((lin,), idx)
        else:
            key = ((0x7f800000 - zf.view(torch.int32).long()) << 32) | (idx + 1)
            keys = torch.zeros(H * W, dtype=torch.int64, device=pts.device).scatter_reduce_(0, lin, key, 'amax', include_self=True)
            index = (keys & 0xffffffff) - 1
        hit = index >= 0
        safe = index.clamp(min=0)
        depth = torch.where(hit, ((pts[safe].double() - pose[:3, 3].double()) @ pose[:3, :3].double())[:, 2].float(), torch.zeros((), device=pts.device))
        image = torch.where(hit[:, None], (cols[safe].double() * 255).clamp(0, 255).to(torch.uint8), torch.zeros((), dtype=torch.uint8, device=pts.device))
        images.append(image.view(H, W, 3)), depths.append(depth.view(H, W)), indices.append(index.int().view(H, W))
    return torch.stack(images), torch.stack(depths), torch.stack(indices)


def render_lines(rounds):
    import torch
    from super_primitive_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"render of {Q} points, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_render_views = ONE call for the V views on preallocated buffers; 8 x (V = 1) = one call per view; torch = float64 projection + "
             "index_put_ (mode 0) / scatter_reduce_(amax) on int64 keys (mode 1), per view",
             f"{'size':>9} {'V':>2} {'mode':>4} {'kept pairs':>10} {'MB moved':>9} {'sp_render_views':>24} {'of HBM peak':>11} {'Gpairs/s':>8} "
             f"{'8 x (V = 1)':>24} {'torch ops':>26} {'torch / one call':>16}"]
    for H, W in ((224, 288), (480, 640)):
        for V in (1, 8):
            pts, cols, K, poses = make_scene(dev, V, H, W)
            views = torch.cat((K.reshape(1, 9).expand(V, 9), poses.reshape(V, 16)), dim=1).contiguous()
            keys = torch.empty(V * H * W, dtype=torch.int64, device=dev)
            image = torch.empty(V, H, W, 3, dtype=torch.uint8, device=dev)
            depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
            index = torch.empty(V, H, W, dtype=torch.int32, device=dev)
            stream = _lib.stream_ptr()
            for mode in (0, 1):
                def one(mode=mode):
                    _lib.check(lib.sp_render_views(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, mode, 1e-6, _lib.ptr(keys),
                                                   _lib.ptr(image), _lib.ptr(depth), _lib.ptr(index), stream), "sp_render_views")

                def each(mode=mode):
                    for k in range(V):
                        _lib.check(lib.sp_render_views(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views[k]), 1, H, W, mode, 1e-6, _lib.ptr(keys[k * H * W:]),
                                                       _lib.ptr(image[k]), _lib.ptr(depth[k]), _lib.ptr(index[k]), stream), "sp_render_views")
                many = lambda mode=mode: torch_render(pts, cols, K, poses, H, W, mode)
                one()
                d1, i1 = depth.clone(), index.clone()
                each()
                assert torch.equal(d1, depth) and torch.equal(i1, index), "one call and a call per view disagree"
                _, dt, it = many()
                if mode == 1:                              # (mode 0 through index_put_ has no defined winner)
                    same = float((it == i1).float().mean())
                    assert same > 0.999 and float((dt - d1).abs()[it == i1].max()) < 1e-5, f"the timed paths disagree: {same}"
                kept = sum(int(torch_project(pts, K, pose, H, W, mode == 1)[0].numel()) for pose in poses)
                hit = int((i1 >= 0).sum())
                moved = 12 * Q + (8 + 8 + 11) * V * H * W + 12 * hit
                fns = [one, each, many] if V > 1 else [one, many]
                t = timed(fns, rounds, block=40)
                t1, tn = t[0], t[-1]
                te = fmt(t[1]) if V > 1 else "-"
                lines.append(f"{H}x{W:>4} {V:>2} {mode:>4} {kept:>10} {moved / 1e6:>9.1f} {fmt(t1):>24} {100 * moved / (t1[0] * 1e-3) / HBM_PEAK:>10.2f}% "
                             f"{kept / (t1[0] * 1e-3) / 1e9:>8.2f} {te:>24} {fmt(tn):>26} {tn[0] / t1[0]:>15.1f}x")
    return lines


def lift_lines(rounds):
    import torch
    from super_primitive_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, H, W = 8, 480, 640
    g = torch.Generator(device="cpu").manual_seed(12)
    d = (0.5 + 4.0 * torch.rand(B, H, W, generator=g))
    d[torch.rand(B, H, W, generator=g) < 0.2] = 0.0
    d, img = d.to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
    _, _, K, poses = make_scene(dev, B, H, W)
    Ks, Ts = K.reshape(1, 9).expand(B, 9).contiguous(), poses.reshape(B, 16).contiguous()
    cap = B * H * W
    scratch = torch.empty(lib.sp_depth_lift_blocks(B, H, W), dtype=torch.int32, device=dev)
    points, colours = torch.empty(cap, 3, device=dev), torch.empty(cap, 3, device=dev)
    pixel, counts = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    stream = _lib.stream_ptr()

    def one():
        _lib.check(lib.sp_depth_lift(_lib.ptr(d), _lib.ptr(Ks), _lib.ptr(Ts), _lib.ptr(img), B, H, W, 100.0, _lib.ptr(scratch), _lib.ptr(points),
                                     _lib.ptr(colours), _lib.ptr(pixel), _lib.ptr(counts), _lib.ptr(offsets), stream), "sp_depth_lift")

    def many():
        valid = (d > 0) & (d <= 100.0)
        b, r, c = torch.nonzero(valid, as_tuple=True)                         # (synchronises: the count comes to the host)
        z = d[b, r, c].double()
        x = (c.double() - K[0, 2].double()) * z / K[0, 0].double()
        y = (r.double() - K[1, 2].double()) * z / K[1, 1].double()
        T = poses.double()[b]
        p = (T[:, :3, 0] * x[:, None] + T[:, :3, 1] * y[:, None] + T[:, :3, 2] * z[:, None] + T[:, :3, 3]).float()
        return p, img[b, :, r, c], (r * W + c).int()
    one()
    p, col, pix = many()
    n = int(offsets[-1])
    assert n == p.shape[0] and torch.equal(pixel[:n], pix) and torch.equal(colours[:n], col) and float((points[:n] - p).abs().max()) < 1e-5
    moved = 2 * 4 * cap + n * (12 + 12 + 12 + 4)
    t1, tn = timed([one, many], rounds, block=40)
    return ["", f"lift of {B} depth images of {H} x {W} with poses and colours ({n} of {cap} pixels valid), ms per call",
            f"{'MB moved':>9} {'sp_depth_lift':>24} {'of HBM peak':>11} {'torch ops (with its sync)':>28} {'ratio':>7}",
            f"{moved / 1e6:>9.1f} {fmt(t1):>24} {100 * moved / (t1[0] * 1e-3) / HBM_PEAK:>10.2f}% {fmt(tn):>28} {tn[0] / t1[0]:>6.1f}x"]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    text = "\n".join(render_lines(args.rounds) + lift_lines(args.rounds)) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
