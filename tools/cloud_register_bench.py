#!/usr/bin/env python
"""Developer tool: time of one iteration of the map registration (csrc/sp_register.hip ``sp_cloud_register``) on the GPU, beside ONE
``sp_cloud_grid_nearest`` query of the same clouds in the same run -- the registration's pass A is that walk plus the residual, the
Jacobian and a reduction of 36 float64 sums per wave.

Scene: the bumpy height field of tests/cloud_register_ref.py over [-1, 1]^2 at z about 2, sampled on a 1024 x 1024 pixel grid in
row-major order (Q = 2^20 reference points with their analytic normals: neighbouring rows are neighbouring pixels, as in a keyframe's
map); the queries (Qa = 2^20) are the grid's points jittered by half a pixel.  The radius is found by bisection so that the mean number
of neighbours per query is about 16, and ``sp_cloud_grid_nearest`` is timed on these queries.  The registration gets the same queries
moved back by the reference's TRUTH and starts AT TRUTH: its pass A walks from the very positions the timed query walks from (up to the
float32 rounding of the moved-back cloud), iteration after iteration.

Per residual kind ONE ``sp_cloud_register`` call of ``--iters`` iterations with tol = 0 (no iteration is skipped: the status stays
RUNNING until the last), on preallocated buffers; the time per iteration is the call's time over the iterations (the zeroing of the
state and the 2 x iters launches included).  Clock: HIP events around blocks of calls, warm-up of every shape first, then the median
(min - max) over alternating rounds.

    python tools/cloud_register_bench.py [--out profiles/cloud_register.txt] [--rounds 5] [--iters 10]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools.map_render_bench import fmt, timed  # noqa: E402

SIDE = 1024
KINDS = ("point to point", "point to plane", "plane to point")


def make_clouds(dev):
    import torch
    import cloud_register_ref as ref
    rng = np.random.default_rng(31)
    y, x = np.meshgrid(np.linspace(-1.0, 1.0, SIDE), np.linspace(-1.0, 1.0, SIDE), indexing='ij')
    x, y = x.reshape(-1), y.reshape(-1)
    z, n = ref.height(x, y)
    b, bn = np.stack([x, y, z], axis=1).astype(np.float32), n.astype(np.float32)
    pitch = 2.0 / (SIDE - 1)
    xq, yq = x + rng.uniform(-0.5, 0.5, len(x)) * pitch, y + rng.uniform(-0.5, 0.5, len(x)) * pitch
    zq, nq = ref.height(xq, yq)
    p = np.stack([xq, yq, zq], axis=1).astype(np.float32)
    a = ref.inverse_moved(p, ref.TRUTH['R'], ref.TRUTH['t'], ref.TRUTH['s'])
    an = (nq @ ref.TRUTH['R']).astype(np.float32)
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    start = np.concatenate([ref.TRUTH['R'].reshape(9), ref.TRUTH['t'], [ref.TRUTH['s']]])
    return to(p), to(a), to(an), to(b), to(bn), to(start)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import torch
    from super_primitive_amd import _lib
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    p, a, an, b, bn, start = make_clouds(dev)
    Q = Qa = SIDE * SIDE
    scratch = torch.empty(lib.sp_cloud_grid_scratch_units(Q), 8, dtype=torch.int64, device=dev)
    index, count = (torch.empty(Qa, dtype=torch.int32, device=dev) for _ in range(2))
    dist = torch.empty(Qa, dtype=torch.float32, device=dev)
    stream = _lib.stream_ptr()

    def build(radius):
        _lib.check(lib.sp_cloud_grid_build(_lib.ptr(b), Q, radius, 0.0, 0.0, 0.0, _lib.ptr(scratch), stream), "sp_cloud_grid_build")

    def query():
        _lib.check(lib.sp_cloud_grid_nearest(_lib.ptr(p), Qa, Q, _lib.ptr(scratch), 0, _lib.ptr(index), _lib.ptr(dist), _lib.ptr(count), stream),
                   "sp_cloud_grid_nearest")
    lo, hi = 1e-4, 1.0
    for _ in range(24):                                                        # bisection on log(radius)
        mid = float(np.sqrt(lo * hi))
        build(mid)
        query()
        lo, hi = (mid, hi) if float(count.double().mean()) < 16 else (lo, mid)
    radius = float(np.float32(np.sqrt(lo * hi)))
    build(radius)
    query()
    mean, none = float(count.double().mean()), float((index < 0).double().mean())
    state0 = torch.zeros(64, dtype=torch.float64, device=dev)
    state0[:13] = start
    state = state0.clone()
    history = torch.empty(args.iters, 4, dtype=torch.float64, device=dev)
    work = torch.empty(lib.sp_cloud_register_work_doubles(Qa), dtype=torch.float64, device=dev)

    def register(kind):
        def call():
            state.copy_(state0)
            _lib.check(lib.sp_cloud_register(_lib.ptr(a), _lib.ptr((None, bn, an)[kind]), Qa, Q, _lib.ptr(scratch), kind, 1, 0.0, 0.0, 7, args.iters,
                                             _lib.ptr(state), _lib.ptr(history), _lib.ptr(index), _lib.ptr(work), stream), "sp_cloud_register")
        return call
    calls = [query] + [register(k) for k in range(3)]
    t = timed(calls, args.rounds, block=3)
    lines = [f"map registration, Q = Qa = {Q} points of the bumpy surface on a {SIDE} x {SIDE} grid, radius {radius:.6f}: {mean:.2f} neighbours per query, "
             f"{none:.4f} of the queries without one",
             f"ms per call: median (min - max) over {args.rounds} alternating rounds of blocks of 3 calls, HIP events around every block; one "
             f"sp_cloud_register call = {args.iters} iterations from the truth with the scale, tol 0 (none is skipped), the state's copy and zeroing included",
             f"{'call':>40} {'ms per call':>26} {'ms per iteration':>17} {'over one sp_cloud_grid_nearest':>31}",
             f"{'sp_cloud_grid_nearest, one query':>40} {fmt(t[0]):>26} {'':>17} {1.0:>31.2f}"]
    for k in range(3):
        register(k)()
        torch.cuda.synchronize()
        per = t[1 + k][0] / args.iters
        lines.append(f"{'sp_cloud_register, ' + KINDS[k]:>40} {fmt(t[1 + k]):>26} {per:>17.3f} {per / t[0][0]:>31.2f}")
        h = history.cpu().numpy()
        lines.append(f"{'':>40} steps {' '.join(f'{s:.1e}' for s in h[:, 2])}; pairs {int(h[-1, 0])}; status {int(h[-1, 3])}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
