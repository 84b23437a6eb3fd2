#!/usr/bin/env python
"""Developer tool: time of the map neighbourhoods (csrc/sp_knn.hip sp_cloud_grid_knn / sp_cloud_normals) on the GPU, next to
sp_cloud_grid_nearest on the same scratch in the same session.

Scene, radii and clock are those of tools/map_nearest_bench.py (its ``Shape``): a reference cloud of 1 M or 4 M points of the synthetic
multi-keyframe surface, 1 M noisy queries, radii found by bisection for about 1, 4, 16 and 64 neighbours per query; HIP events around
blocks of calls, every shape warmed up first, the median (min - max) over alternating rounds.

Per line: ONE ``sp_cloud_grid_nearest`` call, ONE ``sp_cloud_grid_knn`` call at k = 1, 8, 16 and 32, and ONE ``sp_cloud_normals`` call at
k = 16 (on the lists of the k = 16 query), all on preallocated buffers.  The yardstick for k = 1 is the nearest query: its ratio is
printed; for larger k the time per query.  Before the clock the outputs are checked on the device: k = 1 equals the nearest query bit
for bit, ``count`` is the same at every k, and the first 8 columns at k = 16 and 32 are the lists at k = 8.

``--lib PATH`` (repeatable) names other builds of the library, made with other workgroup sizes of the list kernel
(``make -C super_primitive_amd/csrc KNN_FLAGS="-DSP_KNN_BLOCK_8=64 -DSP_KNN_BLOCK_16=64 -DSP_KNN_BLOCK_32=64"``, the library copied
aside): their ``sp_cloud_grid_knn`` is timed in the same rounds, alternating with the shipped one -- the A/B that decides the shipped
sizes.  Their outputs must equal the shipped library's.

The tool ends with the accuracy of ``sp_cloud_normals`` on the unit sphere of tests/test_gpu_cloud_normals.py: the largest observed
ratio of the angle to its bound.

    python tools/cloud_knn_bench.py [--out profiles/cloud_knn.txt] [--rounds 5] [--lib other/libsp_hip.so ...] [--no-host]

``--no-host`` leaves out the k-d tree on the host (``cKDTree.query(k=16)``, timed once per line and compared with the lists)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_nearest_bench import QA, Shape  # noqa: E402
from tools.map_render_bench import fmt, timed  # noqa: E402

KS = (1, 8, 16, 32)


class KnnShape(Shape):
    def __init__(self, dev, Q, other_libs):
        import torch
        super().__init__(dev, Q)
        self.k_index = torch.empty(QA, 32, dtype=torch.int32, device=dev)
        self.k_dist = torch.empty(QA, 32, dtype=torch.float32, device=dev)
        self.k_count = torch.empty(QA, dtype=torch.int32, device=dev)
        self.normals = torch.empty(QA, 3, dtype=torch.float32, device=dev)
        self.curvature = torch.empty(QA, dtype=torch.float32, device=dev)
        self.used = torch.empty(QA, dtype=torch.int32, device=dev)
        self.others = other_libs

    def knn(self, k, lib=None):
        L = self._lib
        L.check((lib or self.lib).sp_cloud_grid_knn(L.ptr(self.qs), QA, self.Q, L.ptr(self.scratch), 0, k, L.ptr(self.k_index), L.ptr(self.k_dist),
                                                    L.ptr(self.k_count), self.stream), "sp_cloud_grid_knn")

    def lists(self, k, lib=None):
        self.knn(k, lib)
        return self.k_index.view(-1)[:QA * k].view(QA, k).clone(), self.k_dist.view(-1)[:QA * k].view(QA, k).clone(), self.k_count.clone()

    def cloud_normals(self, k):
        L = self._lib
        L.check(self.lib.sp_cloud_normals(L.ptr(self.ref), self.Q, L.ptr(self.qs), L.ptr(self.k_index), QA, k, None, 0, None, L.ptr(self.normals),
                                          L.ptr(self.curvature), L.ptr(self.used), self.stream), "sp_cloud_normals")

    def check(self):
        """The outputs against each other, on the device."""
        import torch
        self.query()
        i8, d8, c8 = self.lists(8)
        i1, d1, c1 = self.lists(1)
        assert torch.equal(i1[:, 0], self.index) and torch.equal(d1[:, 0].view(torch.int32), self.dist.view(torch.int32)) and torch.equal(c1, self.count)
        for k in (8, 16, 32):
            ik, dk, ck = self.lists(k)
            assert torch.equal(ik[:, :8], i8) and torch.equal(dk[:, :8].view(torch.int32), d8.view(torch.int32)) and torch.equal(ck, self.count)
            for lib in self.others:
                io, do, co = self.lists(k, lib)
                assert torch.equal(io, ik) and torch.equal(do.view(torch.int32), dk.view(torch.int32)) and torch.equal(co, ck)

    def host(self, radius, k=16):
        """The k-d tree on the host: seconds of the k = 16 query; its lists must agree where the distances of a list are distinct."""
        from scipy.spatial import cKDTree
        if self.tree is None:
            self.tree = cKDTree(self.ref.cpu().numpy().astype(np.float64))
        q = self.qs.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        d, i = self.tree.query(q, k=k, distance_upper_bound=float(np.float32(radius)), workers=16)
        seconds = time.perf_counter() - t0
        index = self.lists(k)[0].cpu().numpy()
        distinct = ~(np.isfinite(d[:, 1:]) & (d[:, 1:] == d[:, :-1])).any(axis=1)
        want = np.where(np.isfinite(d), i, -1)
        assert np.array_equal(index[distinct], want[distinct]), "the kernel's lists differ from the k-d tree's where the distances are distinct"
        return seconds


def load_other(path):
    from super_primitive_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.sp_cloud_grid_knn.argtypes, lib.sp_cloud_grid_knn.restype = _lib.SIGNATURES["sp_cloud_grid_knn"], ctypes.c_int
    assert lib.sp_abi_version() == _lib.SP_ABI_VERSION, path
    return lib


def lines_of(rounds, host, others):
    import torch
    dev = torch.device("cuda:0")
    names = [os.path.basename(os.path.dirname(os.path.abspath(p))) + "/" + os.path.basename(p) for p in others]
    libs = [load_other(p) for p in others]
    lines = [f"map neighbourhoods, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of 5 calls",
             f"nearest = ONE sp_cloud_grid_nearest of {QA} queries against the reference cloud (Q points), k = .. ONE sp_cloud_grid_knn of the same queries "
             "on the same scratch, normals = ONE sp_cloud_normals at k = 16 on those lists; preallocated buffers; k 1 / nearest = the ratio of the medians; "
             "ns / query = the median over the queries" + ("; cKDTree = scipy.spatial.cKDTree.query(k=16, distance_upper_bound=r, workers=16) on the host "
                                                            "(tree built before the clock), its lists checked against the kernel's" if host else ""),
             f"{'Q':>8} {'radius':>9} {'mean count':>10} {'nearest':>22} " + " ".join(f"{'k = ' + str(k):>22}" for k in KS) + f" {'normals k 16':>22} "
             f"{'k 1 / nearest':>13} " + " ".join(f"{'ns/q k ' + str(k):>9}" for k in KS[1:]) + f" {'ns/q normals':>12}" + (f" {'cKDTree s':>9}" if host else "")]
    ab = []
    for Q in (1_000_000, 4_000_000):
        s = KnnShape(dev, Q, libs)
        for neighbours in (1, 4, 16, 64):
            radius = s.radius_for(neighbours)
            mean = s.mean_count(radius)
            s.check()
            s.knn(16)
            fns = [s.query] + [lambda k=k: s.knn(k) for k in KS]
            t = timed(fns, rounds, block=5)
            s.knn(16)
            tn = timed([lambda: s.cloud_normals(16)], rounds, block=5)[0]
            tree = ""
            if host:
                torch.cuda.synchronize()
                tree = f" {s.host(radius):>9.2f}"
            lines.append(f"{Q:>8} {radius:>9.6f} {mean:>10.2f} {fmt(t[0]):>22} " + " ".join(f"{fmt(x):>22}" for x in t[1:]) + f" {fmt(tn):>22} "
                         f"{t[1][0] / t[0][0]:>13.2f} " + " ".join(f"{x[0] * 1e6 / QA:>9.2f}" for x in t[2:]) + f" {tn[0] * 1e6 / QA:>12.2f}" + tree)
            print(lines[-1], file=sys.stderr, flush=True)                     # (progress: the table itself is printed at the end)
            if libs:
                for k in KS[1:]:
                    tv = timed([lambda k=k: s.knn(k)] + [lambda k=k, lib=lib: s.knn(k, lib) for lib in libs], rounds, block=5)
                    ab.append(f"{Q:>8} {mean:>10.2f} {k:>3} {fmt(tv[0]):>22} " + " ".join(f"{fmt(x):>22} {x[0] / tv[0][0]:>6.3f}" for x in tv[1:]))
                    print(ab[-1], file=sys.stderr, flush=True)
        del s
    if libs:
        lines += ["", "workgroup sizes of the list kernel: the shipped library against other builds, the same scratch, the same rounds (alternating); "
                  "the figure after each time is its ratio to the shipped one",
                  f"{'Q':>8} {'mean count':>10} {'k':>3} {'shipped':>22} " + " ".join(f"{n:>29}" for n in names)] + ab
    return lines


def sphere_lines():
    """The observed-to-bound ratios of the normals on the unit sphere of tests/test_gpu_cloud_normals.py."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cloud_knn_ref as ref
    from super_primitive_amd.tool import viz
    p = ref.sphere()
    lines = ["", "sp_cloud_normals on 4001 points of the unit sphere against numpy.linalg.eigh on the same covariance: the angle between the two normals "
             "over its bound 2^-22 + 64 * 2^-52 * l2 / (l1 - l0), the curvature error over 128 * 2^-52 + 2^-23 * curvature",
             f"{'radius':>7} {'k':>3} {'normals':>8} {'NaN rows':>8} {'largest l2 / (l1 - l0)':>22} {'largest angle / bound':>21} {'largest curvature error / bound':>31} "
             f"{'mean angle to radial':>20}"]
    for radius, k in ((0.15, 16), (0.1, 8)):
        out = viz.cloud_normals(torch.from_numpy(p).cuda(), radius, k=k)
        index = out['knn']['index'].cpu().numpy()
        want = ref.normals(p, p, index)
        n, c = out['normals'].cpu().numpy().astype(np.float64), out['curvature'].cpu().numpy().astype(np.float64)
        ok = ~np.isnan(want['normals']).any(axis=1)
        assert np.array_equal(np.isnan(n).any(axis=1), ~ok) and np.array_equal(out['used'].cpu().numpy(), want['used'])
        ratio = ref.angle(n[ok], want['normals'][ok]) / ref.angle_bound(want['gap'][ok])
        c_ratio = np.abs(c[ok] - want['curvature'][ok]) / ref.curvature_bound(want['curvature'][ok])
        lines.append(f"{radius:>7} {k:>3} {ok.sum():>8} {(~ok).sum():>8} {want['gap'][ok].max():>22.4g} {ratio.max():>21.3f} {c_ratio.max():>31.3f} "
                     f"{ref.angle(n[ok], p[ok].astype(np.float64)).mean():>20.4f}")
    return lines


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", action="append", default=[], help="another build of libsp_hip.so whose sp_cloud_grid_knn is timed beside the shipped one")
    ap.add_argument("--no-host", action="store_true", help="leave the k-d tree on the host out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need a GPU"
    lines = lines_of(args.rounds, not args.no_host, args.lib) + sphere_lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
