#!/usr/bin/env python
"""Developer tool: time of the map distances (csrc/sp_nearest.hip sp_cloud_grid_build / sp_cloud_grid_nearest) on the GPU, and the 3D
scores of a sequence's map.

Scene: the synthetic multi-keyframe surface of tools/map_consistency_bench.py -- 16 cameras on an arc in front of a wavy surface, a
cloud of Q points of it in 16 blocks, block k a row-major grid over what camera k sees (neighbouring rows are neighbouring pixels of
their keyframe: the lanes of a wave mostly walk the same cells).  The reference cloud is that scene at Q = 1 M or 4 M; the queries are
the scene at 1 M with Gaussian noise of 2 mm on every coordinate.  The radii are found by bisection so that the mean number of
neighbours per query is about 1, 4, 16 and 64.

Per line ONE ``sp_cloud_grid_build`` call and ONE ``sp_cloud_grid_nearest`` call on preallocated buffers (scratch included), timed
apart.  The bytes a query moves are computed, not counted: 27 probes of 16 bytes, its 12 bytes in and 12 out, and 16 bytes per member
of the 27 cells (their number found with torch on the device); over the query's time, as a share of the 8 TB/s HBM peak -- most of it
is served by the caches, so the share says how far the walk is from being limited by memory at all.  Beside it the yardstick on the
host, in the same run: ``scipy.spatial.cKDTree(reference).query(queries, k=1, distance_upper_bound=r, workers=16)`` (the tree is built
once per cloud and not timed), whose index must agree with the kernel's on every query whose winning distance is unique, and whose
``query_ball_point(..., return_length=True)`` must agree with ``count``.

Clock: HIP events around blocks of calls, warm-up of every shape first, then the median (min - max) over alternating rounds; the host
yardstick by perf_counter, once.

    python tools/map_nearest_bench.py [--out profiles/map_nearest.txt] [--rounds 5] [--sequence] [--no-host]
    python tools/map_nearest_bench.py --one 4000000,16 --calls 5      (one shape -- Q, neighbours per query --, for a counter pass around it)

``--sequence`` appends the 30-frame sequence of tests/test_gpu_sequence_results.py: the raw, the filtered and the fused map (voxel
0.02), each against the lifted ground-truth depths of its keyframes at radius 0.1 and threshold 0.05."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_consistency_bench import make_scene  # noqa: E402
from tools.map_render_bench import fmt, timed  # noqa: E402

V, H, W = 16, 224, 288
QA = 1_000_000
HBM_PEAK = 8.0e12


class Shape:
    def __init__(self, dev, Q):
        import torch
        from super_primitive_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.Q = Q
        self.ref = make_scene(dev, Q, V, H, W)[0]
        noise = 0.002 * torch.randn(QA, 3, generator=torch.Generator(device="cpu").manual_seed(7))
        self.qs = (make_scene(dev, QA, V, H, W)[0] + noise.to(dev)).contiguous()
        self.units = self.lib.sp_cloud_grid_scratch_units(Q)
        self.scratch = torch.empty(self.units, 8, dtype=torch.int64, device=dev)
        self.index, self.count = (torch.empty(QA, dtype=torch.int32, device=dev) for _ in range(2))
        self.dist = torch.empty(QA, dtype=torch.float32, device=dev)
        self.stream = _lib.stream_ptr()
        self.tree = None

    def build(self, radius):
        L = self._lib
        L.check(self.lib.sp_cloud_grid_build(L.ptr(self.ref), self.Q, radius, 0.0, 0.0, 0.0, L.ptr(self.scratch), self.stream), "sp_cloud_grid_build")

    def query(self):
        L = self._lib
        L.check(self.lib.sp_cloud_grid_nearest(L.ptr(self.qs), QA, self.Q, L.ptr(self.scratch), 0, L.ptr(self.index), L.ptr(self.dist), L.ptr(self.count),
                                               self.stream), "sp_cloud_grid_nearest")

    def mean_count(self, radius):
        self.build(radius)
        self.query()
        return float(self.count.double().mean())

    def radius_for(self, neighbours):
        """The radius at which the mean neighbour count is about ``neighbours``: bisection on log(radius)."""
        lo, hi = 1e-4, 1.0
        for _ in range(24):
            mid = float(np.sqrt(lo * hi))
            if self.mean_count(mid) < neighbours:
                lo = mid
            else:
                hi = mid
        return float(np.float32(np.sqrt(lo * hi)))

    def visited(self, radius):
        """The members of the 27 cells around every query, summed over the queries: what the walks load (torch, float64 as the kernel)."""
        import torch
        cell = float(np.float32(radius)) * 1.0009765625

        def keys(p, shift):
            g = torch.floor(p.double() / cell).long() + shift + 2 ** 20
            return g[:, 0] << 42 | g[:, 1] << 21 | g[:, 2]
        zero = torch.zeros(3, dtype=torch.int64, device=self.ref.device)
        uniq, counts = torch.unique(keys(self.ref, zero), return_counts=True)
        total = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    k = keys(self.qs, torch.tensor([dx, dy, dz], dtype=torch.int64, device=self.ref.device))
                    at = torch.searchsorted(uniq, k).clamp(max=uniq.shape[0] - 1)
                    total += int(torch.where(uniq[at] == k, counts[at], torch.zeros_like(at)).sum())
        return total

    def host(self, radius):
        """The k-d tree on the host: seconds of the k = 1 query, and the agreement of index and count with the last kernel result."""
        from scipy.spatial import cKDTree
        if self.tree is None:
            self.tree = cKDTree(self.ref.cpu().numpy().astype(np.float64))
        q = self.qs.cpu().numpy().astype(np.float64)
        r = float(np.float32(radius))
        t0 = time.perf_counter()
        d1, i1 = self.tree.query(q, k=1, distance_upper_bound=r, workers=16)
        seconds = time.perf_counter() - t0
        d2, _ = self.tree.query(q, k=2, distance_upper_bound=r, workers=16)
        n = self.tree.query_ball_point(q, r, workers=16, return_length=True)
        index, count = self.index.cpu().numpy(), self.count.cpu().numpy()
        unique = d2[:, 0] != d2[:, 1]                                           # (inf, inf: no neighbour -- compared through the count)
        want = np.where(np.isfinite(d1), i1, -1)
        assert np.array_equal(index[unique], want[unique]), "the kernel's index differs from the k-d tree's where the winner is unique"
        assert np.array_equal(index < 0, ~np.isfinite(d1)) and np.array_equal(count, n), "the kernel's count differs from the k-d tree's"
        return seconds, int(unique.sum())


def lines_of(rounds, host):
    import torch
    dev = torch.device("cuda:0")
    lines = [f"map distances, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls",
             f"build = ONE sp_cloud_grid_build of the reference cloud (Q points), query = ONE sp_cloud_grid_nearest of {QA} queries, on preallocated "
             "buffers, scratch included; bytes per query = 27 x 16 (probes) + 24 (the query and its answer) + 16 per member of the 27 cells; "
             "cKDTree = scipy.spatial.cKDTree.query(k=1, distance_upper_bound=r, workers=16) on the host in the same run (tree built before the clock), "
             "index and count checked against the kernel on every query",
             f"{'Q':>8} {'radius':>9} {'mean count':>10} {'none':>6} {'scratch MiB':>11} {'build':>24} {'query':>24} {'Mqueries/s':>10} "
             f"{'B / query':>9} {'TB/s':>6} {'of HBM peak':>11} {'cKDTree s':>9} {'cKDTree / query':>15}"]
    for Q in (1_000_000, 4_000_000):
        s = Shape(dev, Q)
        for neighbours in (1, 4, 16, 64):
            radius = s.radius_for(neighbours)
            mean = s.mean_count(radius)
            none = float((s.index < 0).double().mean())
            t = timed([lambda: s.build(radius), s.query], rounds, block=5)
            per_query = 27 * 16 + 24 + 16 * s.visited(radius) / QA
            rate = per_query * QA / (t[1][0] * 1e-3)
            tree = ""
            if host:
                s.build(radius)
                s.query()
                torch.cuda.synchronize()
                seconds, _ = s.host(radius)
                tree = f"{seconds:>9.2f} {seconds * 1e3 / t[1][0]:>14.0f}x"
            lines.append(f"{Q:>8} {radius:>9.6f} {mean:>10.2f} {none:>6.3f} {s.units * 64 / 2 ** 20:>11.1f} {fmt(t[0]):>24} {fmt(t[1]):>24} "
                         f"{QA / (t[1][0] * 1e-3) / 1e6:>10.0f} {per_query:>9.0f} {rate / 1e12:>6.2f} {rate / HBM_PEAK:>10.1%} {tree}")
            print(lines[-1], file=sys.stderr, flush=True)                     # (progress: the table itself is printed at the end)
        del s
    return lines


def sequence_lines():
    """The 3D scores of the raw, the filtered and the fused map of the 30-frame test sequence against its lifted ground-truth depths."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from gpu_util import T
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
    lifted = viz.lift_depth_images(gt, Ks, T(G[ids]))
    reference = lifted['points'][:int(lifted['offsets'][-1])]
    radius, threshold, voxel = 0.1, 0.05, 0.02
    maps = (("raw", world), ("filtered", results.filter_map(world, results.sequence_consistency(world, out))), (f"fused {voxel}", results.fuse_map(world, voxel)))
    lines = ["", f"the 30-frame sequence of tests/test_gpu_sequence_results.py: the map of {len(ids)} keyframes {ids} against the lifted ground-truth depths "
             f"of those keyframes ({reference.shape[0]} points), map_distance at radius {radius}, threshold {threshold}; distances in mm",
             f"{'map':>12} {'points':>8} {'accuracy':>9} {'completion':>10} {'acc. clipped':>12} {'compl. clipped':>14} {'precision':>9} {'recall':>7} {'F-score':>8} "
             f"{'map_distance ms':>24}"]
    for name, w in maps:
        m = {k: float(v) for k, v in results.map_distance(w, reference, radius, threshold=threshold)['metrics'].items()}
        t = timed([lambda: results.map_distance(w, reference, radius, threshold=threshold)], 5, block=5)[0]      # (allocations and metrics included)
        lines.append(f"{name:>12} {int(m['n_a']):>8} {1e3 * m['accuracy']:>9.2f} {1e3 * m['completion']:>10.2f} {1e3 * m['accuracy_clipped']:>12.2f} "
                     f"{1e3 * m['completion_clipped']:>14.2f} {m['precision']:>9.4f} {m['recall']:>7.4f} {m['fscore']:>8.4f} {fmt(t):>24}")
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sequence", action="store_true", help="append the 30-frame test sequence: the 3D scores of its raw, filtered and fused map")
    ap.add_argument("--no-host", action="store_true", help="leave the k-d tree on the host out")
    ap.add_argument("--one", help="Q,neighbours per query: only this shape, --calls times, nothing timed")
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    if args.one:
        Q, neighbours = (int(x) for x in args.one.split(","))
        s = Shape(torch.device("cuda:0"), Q)
        radius = s.radius_for(neighbours)
        for _ in range(args.calls):
            s.build(radius)
            s.query()
        torch.cuda.synchronize()
        print(f"{QA} queries against {Q} points at radius {radius}: mean count {float(s.count.double().mean()):.2f}, {s.units * 64} bytes of scratch")
        return
    lines = lines_of(args.rounds, not args.no_host)
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
