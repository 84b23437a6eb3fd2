#!/usr/bin/env python
"""Developer tool (GPU): one ``infer_masks`` at the reference's size -- 960 x 1280, 300 + 100 keypoints, configuration A
(config/tum) -- on the device path (sp_sam.hip) and on the torch restatement (tests/sam_select_ref.py), on the same GPU.

    python tools/sam_select_bench.py [--out profiles/sam_select.txt] [--runs 12]
        device events around each call, a warm-up of both, the two alternated, median and spread; then the stats pass alone
        against the restatement's two thresholded-sum passes alone, and the host reads of one call; leaves the shapes of the
        run in --shapes (sam_select_shapes.json) for --kernels.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sam -- python tools/sam_select_bench.py --trace-run 5
    python tools/sam_select_bench.py --kernels DIR --trace-run 5 [--out profiles/sam_select.txt]
        per-kernel times of the traced run, each kernel's bytes (computed here from the shapes) over its time as a share of 8 TB/s.

The logits are drawn on the device once (nested noisy blobs in multiples of 1/8) and handed to both paths by a stand-in network
that costs nothing, so the figures are those of the code behind the network.  4.4 GB + 1.5 GB of logits stream past the 256 MB
cache: the rates are HBM rates."""
import argparse
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, N1, N2, EDGE_SHAPE = 960, 1280, 300, 100, (480, 640)
PEAK_BYTES_PER_S = 8e12


def blob_logits(n, seed, dev):
    """(n,3,H,W) float32 logits of n keypoints and their (n,2) normalised positions, drawn on the device in slabs of 20 keypoints."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    kp = torch.rand(n, 2, generator=g, device=dev) * 2 - 1
    out = torch.empty(n, 3, H, W, device=dev)
    rows, cols = torch.arange(H, device=dev)[None, :, None], torch.arange(W, device=dev)[None, None, :]
    for a in range(0, n, 20):
        k = kp[a:a + 20]
        m = k.shape[0]
        rad = (torch.rand(m, 1, generator=g, device=dev) * 60 + 30) * torch.tensor([1.0, 1.7, 2.6], device=dev)
        slope = torch.rand(m, 3, generator=g, device=dev) * 4 + 0.3
        r0, c0 = (k[:, 0] + 1) * 0.5 * (H - 1), (k[:, 1] + 1) * 0.5 * (W - 1)
        d = torch.sqrt((rows - r0[:, None, None]) ** 2 + (cols - c0[:, None, None]) ** 2)
        x = slope[:, :, None, None] * (rad[:, :, None, None] - d[:, None]) + 0.4 * torch.randn(m, 3, H, W, generator=g, device=dev)
        out[a:a + 20] = (x * 8).round().clamp(-127, 127) / 8
    iou = 0.82 + 0.18 * torch.rand(n, 3, generator=g, device=dev)
    return kp, out, iou


class StoredSam:
    """Hands out the stored rounds in turn, whatever the keypoints."""

    def __init__(self, rounds):
        self.rounds, self.at = rounds, 0

    def __call__(self, image, keypoints):
        out = self.rounds[self.at % len(self.rounds)]
        self.at += 1
        return out


def setup():
    import torch
    import sam_select_ref as ref
    from super_primitive_amd.frontend.segment import mask_generation as mg
    dev = torch.device("cuda:0")
    kp, logits1, iou1 = blob_logits(N1, 1, dev)
    _, logits2, iou2 = blob_logits(N2, 2, dev)
    rounds = [{"masks": logits1, "iou_pred": iou1}, {"masks": logits2, "iou_pred": iou2}]
    image = torch.zeros(H, W, 3, device=dev)

    def device_path():
        torch.manual_seed(0)
        return mg.infer_masks(StoredSam(rounds), image, ref.CONFIG_A, keypoints=kp, num_pts=N1, num_pts_active=N2, edge_probs_shape=EDGE_SHAPE)

    def restatement():
        torch.manual_seed(0)
        return ref.infer_masks(StoredSam(rounds), image, ref.CONFIG_A, kp, N2, edge_probs_shape=EDGE_SHAPE)

    return torch, ref, mg, rounds, device_path, restatement


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop), out


def spread(ms):
    return f"median {statistics.median(ms):8.2f} ms  (min {min(ms):.2f}, max {max(ms):.2f}, n = {len(ms)})"


def host_reads(torch, fn):
    """Calls of the tensor methods that make the host wait for the device, during one fn()."""
    counts = {}
    saved = {name: getattr(torch.Tensor, name) for name in ("item", "nonzero", "tolist", "cpu", "__bool__")}

    def counting(name):
        def call(self, *a, **k):
            if self.is_cuda:
                counts[name] = counts.get(name, 0) + 1
            return saved[name](self, *a, **k)
        return call
    for name in saved:
        setattr(torch.Tensor, name, counting(name))
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(torch.Tensor, name, f)
    return counts


def bench(runs, shapes_path):
    torch, ref, mg, rounds, device_path, restatement = setup()
    for _ in range(2):
        got, want = device_path(), restatement()
    for k in ref.RESULT_ARRAYS:
        assert torch.equal(got[k], want[k]), k                                # the timed paths agree
    for k, v in want["masks"].items():
        assert torch.equal(got["masks"][k], v), k
    t_dev, t_ref = [], []
    for _ in range(runs):
        t_dev.append(timed(torch, device_path)[0])
        t_ref.append(timed(torch, restatement)[0])
    x = rounds[0]["masks"].view(-1, H, W)
    t_stats, t_sums = [], []
    for _ in range(runs):
        t_stats.append(timed(torch, lambda: mg.candidate_stats(x))[0])
        t_sums.append(timed(torch, lambda: (ref.threshold_count(x, 1.0), ref.threshold_count(x, -1.0)))[0])
    gb = x.numel() * 4 / 1e9
    reads = host_reads(torch, device_path)
    # the masks built (the survivors of NMS of both rounds) are what the keypoint filter saw: one call without it counts them
    unfiltered = mg.infer_masks(StoredSam(rounds), torch.zeros(H, W, 3, device=x.device), dict(ref.CONFIG_A, filter_edge_points=False),
                                keypoints=torch.zeros(N1, 2, device=x.device), num_pts=N1, num_pts_active=N2, edge_probs_shape=EDGE_SHAPE)
    with open(shapes_path, "w") as f:
        json.dump({"H": H, "W": W, "He": EDGE_SHAPE[0], "We": EDGE_SHAPE[1], "M": [int(r["masks"].shape[0]) * 3 for r in rounds],
                   "K_built": int(unfiltered["masks"]["masks"].shape[0]), "K_final": int(got["masks"]["masks"].shape[0])}, f)
    lines = [f"infer_masks, {H} x {W}, {N1} + {N2} keypoints, configuration A, edges at {EDGE_SHAPE[0]} x {EDGE_SHAPE[1]}; "
             f"{got['masks']['masks'].shape[0]} masks kept; device events, the two paths alternated after a warm-up of both",
             f"  device path (sp_sam.hip)          {spread(t_dev)}",
             f"  torch restatement, same GPU       {spread(t_ref)}",
             f"  ratio of the medians              {statistics.median(t_ref) / statistics.median(t_dev):.2f} x",
             f"the stats pass over round 1 ({x.shape[0]} maps, {gb:.2f} GB, read once) against the restatement's two thresholded sums alone (2 x {gb:.2f} GB)",
             f"  sp_sam_candidate_stats            {spread(t_stats)}   {gb / statistics.median(t_stats):.2f} TB/s = "
             f"{1e9 * gb / statistics.median(t_stats) * 1e3 / PEAK_BYTES_PER_S:.2f} of 8 TB/s",
             f"  two thresholded sums (torch)      {spread(t_sums)}",
             f"  condition (stats <= two sums)     {'met' if statistics.median(t_stats) <= statistics.median(t_sums) else 'NOT met'}",
             f"host reads of one device-path call: {sum(reads.values())} {dict(sorted(reads.items()))}"]
    return lines


def trace_run(n):
    torch, ref, mg, rounds, device_path, _ = setup()
    for _ in range(n):
        device_path()
    torch.cuda.synchronize()


def kernel_bytes(name, s):
    """Bytes one infer_masks moves through the kernel `name`, from the shapes alone (None: not a streaming kernel)."""
    HW, K = s["H"] * s["W"], s["K_built"]
    if "k_candidate_stats" in name:
        return sum(s["M"]) * HW * 4                                           # every logit once
    if "k_build_masks" in name and K:
        return K * HW * 4 + K * HW + HW                                       # K logit maps in, K masks and the coverage out
    if "k_mask_edges" in name and K:
        return K * s["He"] * s["We"] + 8 * s["He"] * s["We"]                  # every mask's coarse pixels once, two float maps out
    if "k_cut_masks" in name and K:
        return K * HW + s["K_final"] * HW + HW                                # K masks in, the kept ones and the coverage out
    return None


OURS = ("k_stats_init", "k_stats_finish", "k_candidate_stats", "k_box_nms", "k_build_masks", "k_mask_edges", "k_cut_keep", "k_cut_masks")


def kernels(directory, shapes_path, calls):
    """From the dispatch list of the traced run, the first dispatch of the first call (k_stats_init) onwards -- what precedes it drew the logits."""
    import csv
    with open(shapes_path) as f:
        s = json.load(f)
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {directory}"
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: next((k for k in OURS if k + "(" in r["Kernel_Name"] or k + "<" in r["Kernel_Name"]), None)
    rows = rows[next(i for i, r in enumerate(rows) if short(r) == "k_stats_init"):]
    total, count = {}, {}
    for r in rows:
        name = short(r) or "every other kernel (torch)"
        total[name] = total.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        count[name] = count.get(name, 0) + 1
    lines = [f"per-kernel times of {calls} device-path calls under rocprofv3 --kernel-trace (a run of its own); "
             f"{len(rows) / calls:.0f} kernel launches per call, torch's included; {s['K_built']} masks built, {s['K_final']} kept",
             f"  {'kernel':<28} {'launches/call':>13} {'us/call':>10} {'MB/call':>10} {'TB/s':>7} {'of 8 TB/s':>10}"]
    for name in sorted(total, key=lambda n: (n not in OURS, -total[n])):
        us = total[name] / calls / 1e3
        b = kernel_bytes(name, s)
        cells = ("", "", "") if b is None else (f"{b / 1e6:.1f}", f"{b / us / 1e6:.2f}", f"{b / (us * 1e-6) / PEAK_BYTES_PER_S:.2f}")
        lines.append(f"  {name:<28} {count[name] / calls:>13.1f} {us:>10.1f} {cells[0]:>10} {cells[1]:>7} {cells[2]:>10}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--trace-run", type=int, default=0)
    ap.add_argument("--kernels")
    ap.add_argument("--shapes", default="sam_select_shapes.json")
    args = ap.parse_args()
    if args.trace_run and not args.kernels:
        return trace_run(args.trace_run)
    lines = kernels(args.kernels, args.shapes, args.trace_run) if args.kernels else bench(args.runs, args.shapes)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
