#!/usr/bin/env python
"""Developer tool: time of the map consistency test (csrc/sp_views.hip sp_map_consistency) on the GPU.

Scene: V cameras on an arc in front of a wavy surface; the map is Q points of that surface in V blocks, block k a row-major grid over
what camera k sees (neighbouring points are neighbouring pixels of their keyframe, as in a real map), a twentieth of them moved off the
surface by up to +-20 %.  The depth image of a view is the depth buffer of the map in it (``sp_render_views`` mode 1: with holes where
the map is sparser than the view, as a keyframe's own depth image has them outside its segments).  Every point carries its block as
owner, so it is not tested against its own view.

Per line ONE ``sp_map_consistency`` call on preallocated buffers, for window 0, 1 and 2, and beside it the yardstick: ``sp_render_views``
mode 1 with a depth output on the same points and views in the same run -- the same float64 projection per pair, plus one 64-bit atomic
per kept pair and the resolve pass, instead of the window gather.  There is no earlier implementation to compare with.

Per line: ms per call, the (point, view) pairs of the call over the time, the seen pairs (those that read a window) over the time.

Clock: HIP events around blocks of calls, warm-up of every shape first, then the median (min - max) over alternating rounds.

    python tools/map_consistency_bench.py [--out profiles/map_consistency.txt] [--rounds 5]
    python tools/map_consistency_bench.py --one 1000000,64,224,288,0 --calls 5       (one shape, for a counter pass around it)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_render_bench import fmt, timed  # noqa: E402


def make_scene(dev, Q, V, H, W):
    """points (Q,3), owner (Q,), views (V,25), on the device."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(21)
    f = 0.9 * W
    K = torch.tensor([[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], dtype=torch.float32)
    per = (Q + V - 1) // V
    rows = int(np.ceil(np.sqrt(per * H / W)))
    cols = (per + rows - 1) // rows
    pts, owner, poses = [], [], []
    for k in range(V):
        a = 0.5 * (k / max(V - 1, 1) - 0.5)                 # the cameras turn through half a radian about the surface's middle
        c, s = float(np.cos(a)), float(np.sin(a))
        T = torch.eye(4, dtype=torch.float64)
        T[0, 0], T[0, 2], T[2, 0], T[2, 2] = c, s, -s, c
        T[:3, 3] = torch.tensor([-3.0 * s, 0.02 * k, 3.0 - 3.0 * c])
        poses.append(T.float())
        n = min(per, Q - k * per)
        i = torch.arange(n)
        r, cc = (i // cols).double(), (i % cols).double()
        ray = torch.stack(((cc * (W / cols) - K[0, 2]) / K[0, 0], (r * (H / rows) - K[1, 2]) / K[1, 1], torch.ones(n, dtype=torch.float64)), dim=1) @ T[:3, :3].T
        d = 3.0 / ray[:, 2]                                  # onto the plane z = 3, then along z onto the surface
        p = T[:3, 3] + d[:, None] * ray
        p[:, 2] = 3.0 + 0.3 * torch.sin(1.3 * p[:, 0]) * torch.cos(1.7 * p[:, 1])
        off = torch.rand(n, generator=g) < 0.05
        scale = torch.where(off, 1.0 + 0.4 * (torch.rand(n, generator=g) - 0.5), torch.ones(n)).double()
        p = T[:3, 3] + scale[:, None] * (p - T[:3, 3])
        pts.append(p.float())
        owner.append(torch.full((n,), k, dtype=torch.int32))
    poses = torch.stack(poses)
    views = torch.cat((K.reshape(1, 9).expand(V, 9), poses.reshape(V, 16)), dim=1).contiguous()
    return torch.cat(pts).contiguous().to(dev), torch.cat(owner).to(dev), views.to(dev)


class Shape:
    def __init__(self, dev, Q, V, H, W):
        import torch
        from super_primitive_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.Q, self.V, self.H, self.W = Q, V, H, W
        self.pts, self.owner, self.views = make_scene(dev, Q, V, H, W)
        self.view_owner = torch.arange(V, dtype=torch.int32, device=dev)
        self.keys = torch.empty(V * H * W, dtype=torch.int64, device=dev)
        self.depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
        self.scratch_depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
        self.counts = torch.empty(Q, 3, dtype=torch.int32, device=dev)
        self.stream = _lib.stream_ptr()
        self.render(self.depth)                              # the views' own depth images

    def render(self, depth=None):
        L = self._lib
        L.check(self.lib.sp_render_views(L.ptr(self.pts), None, self.Q, L.ptr(self.views), self.V, self.H, self.W, 1, 1e-6, L.ptr(self.keys), None,
                                         L.ptr(self.scratch_depth if depth is None else depth), None, self.stream), "sp_render_views")

    def consistency(self, window):
        L = self._lib
        L.check(self.lib.sp_map_consistency(L.ptr(self.pts), L.ptr(self.owner), self.Q, L.ptr(self.views), L.ptr(self.view_owner), self.V,
                                            L.ptr(self.depth), self.H, self.W, 0.05, window, 1e-6, L.ptr(self.counts), self.stream), "sp_map_consistency")


def lines_of(rounds):
    import torch
    dev = torch.device("cuda:0")
    lines = [f"map consistency, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_map_consistency = ONE call (tol 0.05, owners given) on preallocated buffers; sp_render_views = mode 1 with a depth output on the same points and views, in the same run",
             f"{'size':>9} {'V':>3} {'Q':>8} {'window':>6} {'seen pairs':>11} {'agree':>6} {'sp_map_consistency':>24} {'Gpairs/s':>8} {'seen Gpairs/s':>13} "
             f"{'sp_render_views':>24} {'consistency / render':>20}"]
    for H, W in ((224, 288), (480, 640)):
        for V in (8, 64):
            for Q in (1_000_000, 4_000_000):
                s = Shape(dev, Q, V, H, W)
                fns = [s.render] + [lambda w=w: s.consistency(w) for w in (0, 1, 2)]
                seen, agree = [], []
                for w in (0, 1, 2):
                    s.consistency(w)
                    c = s.counts.sum(dim=0, dtype=torch.int64).tolist()
                    seen.append(sum(c)), agree.append(c[0] / max(sum(c), 1))
                t = timed(fns, rounds, block=10)
                for w in (0, 1, 2):
                    tc = t[1 + w]
                    lines.append(f"{H}x{W:>4} {V:>3} {Q:>8} {w:>6} {seen[w]:>11} {agree[w]:>6.3f} {fmt(tc):>24} {Q * V / (tc[0] * 1e-3) / 1e9:>8.2f} "
                                 f"{seen[w] / (tc[0] * 1e-3) / 1e9:>13.2f} {fmt(t[0]):>24} {tc[0] / t[0][0]:>19.2f}x")
                del s
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--one", help="Q,V,H,W,window: only this shape, --calls times (plus one render), nothing timed")
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    if args.one:
        Q, V, H, W, window = (int(x) for x in args.one.split(","))
        s = Shape(torch.device("cuda:0"), Q, V, H, W)
        for _ in range(args.calls):
            s.consistency(window)
        s.render()
        torch.cuda.synchronize()
        c = s.counts.sum(dim=0, dtype=torch.int64).tolist()
        print(f"{Q} points, {V} views of {H}x{W}, window {window}: {Q * V} pairs, {sum(c)} seen, counts {c}")
        return
    text = "\n".join(lines_of(args.rounds)) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
