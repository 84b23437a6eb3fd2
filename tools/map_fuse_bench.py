#!/usr/bin/env python
"""Developer tool: time of the map fusion (csrc/sp_fuse.hip sp_map_fuse) on the GPU, and what it does to a sequence's map.

Scene: the synthetic multi-keyframe surface of tools/map_consistency_bench.py -- 16 cameras on an arc in front of a wavy surface, the
map Q points of it in 16 blocks, block k a row-major grid over what camera k sees (neighbouring rows are neighbouring pixels of their
keyframe, and every part of the surface is stored by most keyframes) -- with random colours.  The voxel sizes are found by bisection so
that the mean number of points per occupied voxel is about 1, 4, 16 and 64.

Per line ONE ``sp_map_fuse`` call on preallocated buffers (scratch included), and beside it the yardstick, timed in the same run: what a
user would write today with torch on the same device -- the keys by torch ops in float64, ``torch.unique(return_inverse=True,
return_counts=True)``, and ``index_add_`` of positions and colours in float64, divided by the counts.  It sorts by key instead of by
first row (and reads the number of voxels back to size its result), so only the time is compared, not the order.

Clock: HIP events around blocks of calls, warm-up of every shape first, then the median (min - max) over alternating rounds.

    python tools/map_fuse_bench.py [--out profiles/map_fuse.txt] [--rounds 5] [--sequence]
    python tools/map_fuse_bench.py --one 1000000,4 --calls 5       (one shape -- Q, points per voxel --, for a counter pass around it)

``--sequence`` appends the 30-frame sequence of tests/test_gpu_sequence_results.py: Q -> M at three voxel sizes, and ``score_map``'s
coverage and rmse of the fused map against the unfused one, both splatted with the fused map's footprint (radius voxel / 2)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_consistency_bench import make_scene  # noqa: E402
from tools.map_render_bench import fmt, timed  # noqa: E402

V, H, W = 16, 224, 288


class Shape:
    def __init__(self, dev, Q):
        import torch
        from super_primitive_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.Q = Q
        self.pts = make_scene(dev, Q, V, H, W)[0]
        self.cols = torch.rand(Q, 3, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
        self.units = self.lib.sp_map_fuse_scratch_units(Q)
        self.scratch = torch.empty(self.units, 8, dtype=torch.int64, device=dev)
        self.out_p, self.out_c = torch.empty(Q, 3, device=dev), torch.empty(Q, 3, device=dev)
        self.count, self.first, self.label = (torch.empty(Q, dtype=torch.int32, device=dev) for _ in range(3))
        self.n = torch.zeros((), dtype=torch.int64, device=dev)
        self.stream = _lib.stream_ptr()

    def fuse(self, voxel):
        L = self._lib
        L.check(self.lib.sp_map_fuse(L.ptr(self.pts), L.ptr(self.cols), self.Q, voxel, 0.0, 0.0, 0.0, L.ptr(self.scratch), L.ptr(self.out_p),
                                     L.ptr(self.out_c), L.ptr(self.count), L.ptr(self.first), L.ptr(self.label), L.ptr(self.n), self.stream), "sp_map_fuse")

    def torch_fuse(self, voxel):
        """The composition a user would write: the mean position and colour per voxel, voxels in key order."""
        import torch
        p = self.pts.double()
        g = torch.floor(p / voxel)
        kept = torch.isfinite(g).all(dim=1) & (g.abs() < 2 ** 20).all(dim=1)
        cell = g[kept].long() + 2 ** 20
        key = cell[:, 0] << 42 | cell[:, 1] << 21 | cell[:, 2]
        uniq, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
        M = uniq.shape[0]
        pos = torch.zeros(M, 3, dtype=torch.float64, device=p.device).index_add_(0, inverse, p[kept])
        col = torch.zeros(M, 3, dtype=torch.float64, device=p.device).index_add_(0, inverse, self.cols[kept].double())
        n = counts.double()[:, None]
        return (pos / n).float(), (col / n).float(), counts

    def fused_count(self, voxel):
        self.fuse(voxel)
        return int(self.n)

    def voxel_for(self, per_voxel):
        """The voxel size at which Q / M is about ``per_voxel``: bisection on log(voxel) (M falls as the voxel grows)."""
        lo, hi = 1e-4, 1.0
        for _ in range(24):
            mid = float(np.sqrt(lo * hi))
            if self.Q / self.fused_count(mid) < per_voxel:
                lo = mid
            else:
                hi = mid
        return float(np.float32(np.sqrt(lo * hi)))


def lines_of(rounds):
    import torch
    dev = torch.device("cuda:0")
    lines = [f"map fusion, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             "sp_map_fuse = ONE call (positions and colours) on preallocated buffers, scratch included; torch = keys by torch ops in float64, "
             "torch.unique(return_inverse, return_counts), index_add_ of positions and colours, in the same run (sorted by key: only the time compares)",
             f"{'Q':>8} {'voxel':>9} {'M':>8} {'Q / M':>6} {'scratch MiB':>11} {'sp_map_fuse':>24} {'Mpoints/s':>9} {'torch':>27} {'torch / sp_map_fuse':>19}"]
    for Q in (1_000_000, 4_000_000):
        s = Shape(dev, Q)
        for per_voxel in (1, 4, 16, 64):
            voxel = s.voxel_for(per_voxel) if per_voxel > 1 else float(np.float32(2e-4))       # (mean 1: every point alone, as good as)
            M = s.fused_count(voxel)
            assert s.torch_fuse(voxel)[2].shape[0] == M                       # the two agree on the voxels
            t = timed([lambda: s.fuse(voxel), lambda: s.torch_fuse(voxel)], rounds, block=5)
            lines.append(f"{Q:>8} {voxel:>9.6f} {M:>8} {Q / M:>6.2f} {s.units * 64 / 2 ** 20:>11.1f} {fmt(t[0]):>24} {Q / (t[0][0] * 1e-3) / 1e6:>9.0f} "
                         f"{fmt(t[1]):>27} {t[1][0] / t[0][0]:>18.2f}x")
        del s
    return lines


def sequence_lines():
    """Q -> M and the score of the fused against the unfused map on the 30-frame test sequence."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import T, npy
    from test_gpu_sequence import make_sequence_inputs
    from super_primitive_amd.odometery import results
    from super_primitive_amd.odometery.sequence import run_sequence
    from super_primitive_amd.tool import viz
    seq, frames, to_kf = make_sequence_inputs()
    out = run_sequence(frames, to_kf, T(seq[0].T_wc), T(seq[0].kld_gt), engine="gn", keep_keyframes=True, window_size=2, translation_thresh=0.1)
    G = np.stack([f.T_wc for f in seq]).astype(np.float32)
    world = results.sequence_map(out, 1, T(G))
    ids = world['ids']
    Ks, gt = T(np.stack([seq[i].K for i in ids]).astype(np.float32)), T(np.stack([seq[i].depth for i in ids]).astype(np.float32))
    Q = world['points'].shape[0]
    lines = ["", f"the 30-frame sequence of tests/test_gpu_sequence_results.py: {Q} points of {len(ids)} keyframes {ids}; score_map against the ground-truth depths "
             "in the keyframe views, every point splatted with radius voxel / 2: mean coverage and mean rmse (mm) over the views",
             f"{'voxel':>7} {'Q':>8} {'M':>8} {'Q / M':>6} {'max count':>9} {'coverage unfused':>16} {'fused':>7} {'rmse unfused':>12} {'fused':>8} {'fuse_points ms':>24}"]
    for voxel in (0.01, 0.02, 0.05):
        fused = results.fuse_map(world, voxel)
        M = fused['points'].shape[0]
        score = {}
        for name, w in (("unfused", world), ("fused", fused)):
            radii = torch.full((w['points'].shape[0],), voxel / 2, device="cuda")
            s = results.score_map(w, gt, Ks, T(G[ids]), radii=radii)
            col = {c: k for k, c in enumerate(s['columns'])}
            score[name] = (float(npy(s['coverage']).mean()), float(npy(s['metrics'])[:, col['rmse']].mean()))
        t = timed([lambda: viz.fuse_points(world['points'], world['colours'], voxel=voxel)], 5, block=5)[0]     # (allocations included)
        lines.append(f"{voxel:>7.3f} {Q:>8} {M:>8} {Q / M:>6.2f} {int(fused['count'].max()):>9} {score['unfused'][0]:>16.4f} {score['fused'][0]:>7.4f} "
                     f"{score['unfused'][1]:>12.2f} {score['fused'][1]:>8.2f} {fmt(t):>24}")
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sequence", action="store_true", help="append the 30-frame test sequence: Q -> M and the fused map's score")
    ap.add_argument("--one", help="Q,points per voxel: only this shape, --calls times, nothing timed")
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    if args.one:
        Q, per_voxel = (int(x) for x in args.one.split(","))
        s = Shape(torch.device("cuda:0"), Q)
        voxel = s.voxel_for(per_voxel) if per_voxel > 1 else float(np.float32(2e-4))
        for _ in range(args.calls):
            s.fuse(voxel)
        torch.cuda.synchronize()
        print(f"{Q} points at voxel {voxel}: {int(s.n)} fused points, {s.units * 64} bytes of scratch")
        return
    lines = lines_of(args.rounds)
    if args.sequence:
        lines += sequence_lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
