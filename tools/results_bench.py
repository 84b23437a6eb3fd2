#!/usr/bin/env python
"""Developer tool: time of the sequence results (csrc/sp_results.hip) on the GPU.

World map: ONE ``sp_map_points`` launch (``odometery.results.keyframe_points``) over 60 keyframes of 224 x 288 x 40 segments at strides 1
and 4, against the composition available without it: per keyframe ``unproject_kf`` (one ``sp_photo_stats`` launch), the down-sampling
slices, the scale, the matmul with the aligned pose, and one ``cat`` over the keyframes -- both in this process, alternating.  The two
give the same points (checked: the composition's float32 matmul against the kernel's fma chain, 1e-4 relative) and colours (the
composition samples bilinearly at the re-projected pixel centre, the kernel loads the pixel: 1e-3).

Alignment: ``sp_traj_align`` (``pose_utils.align_trajectories``) for S = 1 and S = 64 trajectories of 640 poses against the numpy
restatement of the reference (tests/traj_align_ref.py) INCLUDING the device-to-host copy of the poses it needs.

Clock: HIP events around blocks of calls for the device paths (host time between launches counts: it is what a caller waits for),
``time.perf_counter`` around the numpy path (it ends on the host).  Warm-up of every shape, then the median (min - max) over alternating
rounds.

    python tools/results_bench.py [--out profiles/sequence_results.txt] [--rounds 7]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import traj_align_ref as ref  # noqa: E402

N_KF, H, W, N_SEG = 60, 224, 288, 40


def make_keyframes(dev):
    """60 keyframes in distinct device memory: 6 synthetic frames, each copied 10 times (the synthesis is host work)."""
    import torch
    from super_primitive_amd import synth
    from super_primitive_amd.image.keyframe import KeyFrame
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = 0.6 * np.array([0.05, -0.02, 0.015, 0.01, -0.015, 0.008])
    twists = [5 * k * base + np.array([0.0, 0.05 * (k % 3), -0.04 * (k % 2), 0.0, 0.0, 0.0]) for k in range(6)]       # (not on one line)
    seq = synth.make_sequence(H, W, N_SEG, twists, keyframe_ids=list(range(6)), seed=31, overlap=1)
    kfs, klds, poses = [], [], []
    for k in range(N_KF):
        f = seq[k % 6]
        kfs.append(KeyFrame(t(f.image), t(f.K), t(f.logdepth_perseg), t(f.keypoints), t(f.keypoint_regions)))
        klds.append(t(f.kld_gt))
        poses.append(t(f.T_wc.astype(np.float32)))
    return kfs, klds, torch.stack(poses)


def composition(kfs, klds, poses, stride, align):
    """The map from what the package offered before: per keyframe, in the camera frame, Python-bound."""
    import torch
    from super_primitive_amd.core.dense_optim import unproject_kf
    s = align['s'][0].float()
    rot, ts, rr = align['rot'][0].float(), align['trans_scaled'][0].float(), align['rot_reanchor'][0].float()
    pts, rgb = [], []
    for kf, kld, T in zip(kfs, klds, poses):
        u = unproject_kf(kf, kld)
        R, t = rr @ T[:3, :3], s * (rot @ T[:3, 3]) + ts
        pts.append((s * u['src_pts'][::stride]) @ R.t() + t)
        rgb.append(u['src_pixels'][0][:3, ::stride].t())
    return torch.cat(pts), torch.cat(rgb)


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


def bench(rounds):
    import torch
    from super_primitive_amd.odometery.results import keyframe_points
    from super_primitive_amd.tool import pose_utils
    assert torch.cuda.is_available(), "the timings need a GPU"
    dev = torch.device("cuda:0")
    kfs, klds, poses = make_keyframes(dev)
    rng = np.random.default_rng(3)
    gt = poses.clone()
    gt[:, :3, 3] = 1.3 * gt[:, :3, 3] + torch.from_numpy(0.01 * rng.standard_normal((N_KF, 3))).float().to(dev)
    align = pose_utils.align_trajectories(poses[None], gt[None], anchor_rotation=True)
    lines = [f"sequence results, ms per call: median (min - max) over {rounds} alternating rounds, HIP events around blocks of calls (device paths), "
             f"perf_counter (numpy path)", "",
             f"world map of {N_KF} keyframes of {H} x {W} x {N_SEG}, aligned (keyframe_points = ONE sp_map_points launch; composition = per keyframe "
             f"unproject_kf + slices + matmul, then cat)",
             f"{'stride':>6} {'rows':>9} {'MB written':>10} {'sp_map_points':>26} {'composition':>26} {'ratio':>7} {'max rel. diff':>14} {'colour diff':>12}"]
    for stride in (1, 4):
        one = lambda: keyframe_points(kfs, klds, poses, stride=stride, align=align)
        many = lambda: composition(kfs, klds, poses, stride, align)
        a, (p, c) = one(), many()
        diff = float(((a['points'] - p).abs().max(1).values / (p.abs().max(1).values + 1.0)).max())
        # (the composition's colours are unproject_kf's bilinear samples at the RE-PROJECTED pixel centres: up to ~1e-4 px beside the pixel
        #  in float32 at 288 columns, times the image's slope, at most ~1 per pixel -- the kernel loads the pixel itself)
        cdiff = float((a['colours'] - c).abs().max())
        assert diff <= 1e-4 and cdiff <= 1e-3, f"the timed paths disagree: points {diff:.2e} (relative), colours {cdiff:.2e}"
        (t1, tn) = timed([one, many], rounds, block=5)
        rows = int(a['offsets'][-1])
        lines.append(f"{stride:>6} {rows:>9} {rows * 32 / 1e6:>10.1f} {fmt(t1):>26} {fmt(tn):>26} {tn[0] / t1[0]:>6.1f}x {diff:>14.1e} {cdiff:>12.1e}")

    lines += ["", "trajectory alignment, 640 poses per trajectory (align_trajectories = ONE sp_traj_align launch; numpy = the float64 restatement per "
              "trajectory after one device-to-host copy of the poses)",
              f"{'S':>3} {'sp_traj_align':>26} {'numpy + copy':>26} {'ratio':>7}"]
    for S in (1, 64):
        pr = np.stack([ref.make_case('generic', 640, 100 + s)[0] for s in range(S)])
        g = np.stack([ref.make_case('generic', 640, 100 + s)[1] for s in range(S)])
        pd, gd = torch.from_numpy(pr).to(dev), torch.from_numpy(g).to(dev)
        (t1,) = timed([lambda: pose_utils.align_trajectories(pd, gd, anchor_rotation=True)], rounds, block=20)

        def host():
            ph, gh = pd.cpu().numpy(), gd.cpu().numpy()
            return [ref.align_poses(ph[s], gh[s], True) for s in range(S)]
        host()
        th = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            th.append(1e3 * (time.perf_counter() - t0))
        th = (float(np.median(th)), min(th), max(th))
        lines.append(f"{S:>3} {fmt(t1):>26} {fmt(th):>26} {th[0] / t1[0]:>6.1f}x")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    text = "\n".join(bench(args.rounds)) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
