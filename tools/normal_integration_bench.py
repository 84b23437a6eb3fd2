#!/usr/bin/env python
"""Developer tool: time of the normal integration (sp_normal_integration) at the reference's working size -- 240 x 320, about 100 and
about 300 SAM-shaped masks, cg_tol 1e-3 / cap 1000 and 1e-4 / cap 2000 (config/tum/odom_desk.yaml, config/depth_completion/
void_dataset.yaml) -- on a curved analytic surface.  Per case: ms per keyframe (HIP events around the native call, scratch allocated
once; and around the Python call, which sizes the scratch with one read-back), the largest segment run alone (the one-workgroup
tail) and its time per iteration, CG iterations per second, the bytes-per-iteration model next to the achieved rate, and the wall
time of the float32 scipy CG of tests/normal_integration_ref.py on the same input with 16 processes.

    python tools/normal_integration_bench.py [--out profiles/normal_integration.txt] [--reps 10]
"""
import argparse
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import normal_integration_ref as ref  # noqa: E402

H, W = 240, 320
CASES = ((1e-3, 1000), (1e-4, 2000))
# floats moved per box cell and iteration, through the L2 or -- for the vectors a segment keeps there (p, q, r by size) -- through LDS:
# stencil pass reads p, wR, wD and writes q (the neighbours' p, wR, wD hit L1 / LDS); update pass reads u, p, r, q and writes u, r;
# direction pass reads r, p and writes p
MODEL_FLOATS = 13


def scene(nominal, seed):
    from super_primitive_amd import synth
    pair = synth.make_pair(H, W, nominal, seed=seed, shape="sam", blob_coverage=1.1)
    n, K, _, _ = ref.curved_scene(H, W)
    return n.astype(np.float32), K.astype(np.float32), pair.keypoint_regions


def box_cells(mask):
    r, c = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
    return int((r[-1] - r[0] + 1) * ((c[-1] - c[0] + 1 + 15) // 16 * 16))


def _cpu_one(args):
    normals, K, mask, tol, cap = args
    L, b, _ = ref.build_system(normals, K, mask)
    t0 = time.perf_counter()
    _, k, _ = ref.cg(L, b, tol, cap, dtype=np.float32)
    return k, time.perf_counter() - t0


def cpu_baseline(normals, K, masks, tol, cap):
    """(wall seconds of the whole stack with 16 processes -- system assembly included, as a user would pay it --, summed seconds inside
    the CG loops alone, iterations)."""
    order = np.argsort(-masks.reshape(len(masks), -1).sum(1))            # largest first, like the device
    jobs = [(normals, K, masks[k], tol, cap) for k in order]
    t0 = time.perf_counter()
    with Pool(16) as pool:
        res = pool.map(_cpu_one, jobs, chunksize=1)
    wall = time.perf_counter() - t0
    return wall, sum(t for _, t in res), sum(k for k, _ in res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_integration.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    scenes = [("~100 masks", scene(92, 21)), ("~300 masks", scene(280, 22)), ("one full-frame mask", None)]
    n_c, K_c, _ = scenes[0][1]
    scenes[2] = ("one full-frame mask", (n_c, K_c, np.ones((1, H, W), dtype=bool)))
    cpu = {}
    if not a.no_cpu:                                # before the GPU is opened: the pool forks
        for name, (normals, K, masks) in scenes:
            for tol, cap in CASES:
                if len(masks) == 1 and tol < 1e-3:
                    continue
                cpu[name, tol] = cpu_baseline(normals, K, masks, tol, cap)

    import torch
    from super_primitive_amd import _lib
    from super_primitive_amd.frontend.normals import normals_integration as ni
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    lines = [f"normal integration, {H} x {W}, curved analytic surface, {torch.cuda.get_device_name(0)}; {a.reps} timed calls after 3 warm-up calls, "
             "HIP events; median (min)", ""]

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.min(ts))

    def native(normals, K, masks, tol, cap):
        """The native call alone on preallocated buffers -> (callable, info tensor)."""
        N = masks.shape[0]
        m8 = masks.contiguous().view(torch.uint8)
        words = lib.sp_normal_integration_plan_words(N)
        plan = torch.empty(words, dtype=torch.int32, device=dev)
        _lib.check(lib.sp_normal_integration_plan(_lib.ptr(m8), None, N, H, W, _lib.ptr(plan), _lib.stream_ptr()), "plan")
        n_floats = words + int(plan[:2].view(torch.int64).item())
        scratch = torch.empty(n_floats, dtype=torch.float32, device=dev)
        depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        info = torch.empty(N, 2, dtype=torch.float32, device=dev)

        def call():
            _lib.check(lib.sp_normal_integration(_lib.ptr(normals), _lib.ptr(K), _lib.ptr(m8), None, N, H, W, cap, tol, 0, _lib.ptr(scratch),
                                                 n_floats, _lib.ptr(depth), _lib.ptr(info), _lib.stream_ptr()), "sp_normal_integration")
        return call, info, n_floats

    for name, (normals, K, masks) in scenes:
        sizes = masks.reshape(len(masks), -1).sum(1)
        cells = np.array([box_cells(m) for m in masks])
        lines.append(f"== {name}: N = {len(masks)}, mask pixels {sizes.min()} .. {sizes.max()}, coverage {sizes.sum() / (H * W):.2f}; box cells (row stride "
                     f"padded to 16) {cells.sum()}, fill = mask pixels / box cells {sizes.sum() / cells.sum():.2f}")
        n_t, K_t, m_t = T(normals), T(K), T(masks)
        big = int(cells.argmax())
        for tol, cap in CASES:
            if len(masks) == 1 and tol < 1e-3:
                continue
            call, info, n_floats = native(n_t, K_t, m_t, tol, cap)
            med, mn = timed(call)
            it = info[:, 0].cpu().numpy().astype(np.int64)
            py_med, py_mn = timed(lambda: ni.integrate_normals(n_t, K_t, m_t, cg_max_iter=cap, cg_tol=tol))
            one, info1, _ = native(n_t, K_t, m_t[big:big + 1].clone(), tol, cap)
            med1, mn1 = timed(one)
            it1 = int(info1[0, 0])
            moved = float((cells * it).sum()) * MODEL_FLOATS * 4
            lines.append(f"  cg_tol {tol:g} cap {cap}: native call {med:.2f} ms ({mn:.2f}) per keyframe; Python call incl. scratch sizing {py_med:.2f} ms ({py_mn:.2f}); "
                         f"scratch {n_floats * 4 / 2**20:.1f} MiB")
            lines.append(f"      iterations: total {it.sum()}, per segment {it.min()} .. {it.max()}, at the cap {int((it >= cap).sum())}; {it.sum() / med * 1e3:.3g} CG iterations/s; "
                         f"model {MODEL_FLOATS * 4} B per box cell and iteration (L2 + LDS) -> {moved / 2**30:.2f} GiB per keyframe, achieved {moved / med / 1e6:.0f} GB/s")
            lines.append(f"      largest segment alone ({sizes[big]} px, {cells[big]} cells, {it1} iterations): {med1:.2f} ms ({mn1:.2f}) = {med1 / max(it1, 1) * 1e3:.2f} us per iteration, "
                         f"{cells[big] * MODEL_FLOATS * 4 * it1 / med1 / 1e6:.0f} GB/s from one workgroup; it is {100 * med1 / med:.0f} % of the keyframe's time")
            if (name, tol) in cpu:
                wall, inside, k = cpu[name, tol]
                lines.append(f"      float32 scipy CG on the host, 16 processes: {wall * 1e3:.0f} ms wall per keyframe (system assembly included; {inside * 1e3:.0f} ms summed inside the "
                             f"CG loops, {k} iterations) -> the device call is {wall * 1e3 / med:.0f} x faster")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
