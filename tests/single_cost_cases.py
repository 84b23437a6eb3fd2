"""The cases of tests/test_gpu_single_cost.py (and of tests/test_single_cost_ref_host.py, which checks on the CPU what they promise): hand-made
point tables -- pix words, src4, kp_L, kld, seg_off, tiles, seg_tile_off -- over a 40 x 56 source frame, B targets with their own pose,
intrinsics and affine pair, packed target levels at 40 x 56 (level 0) or 20 x 28 (level 1, so ax, ay != 1).  The set-up kernels stay out of
the picture (tests/test_gpu_point_table.py pins them); the reference evaluates exactly what is uploaded.

Every table PLANTS points that fail each validity test, far from the threshold: a column / a row outside the frame (the 0.99 band in x / in
y), a depth of 1e-3 in front of a target that has moved forward (qz < 0 <= zmin), exp(-30) (d <= 1e-7), and a depth that puts qz of target
0 within 1e-8 of zero (|qz| <= 1e-6) -- the last with its source bit clear: with it set the point would sit within the float32 noise of
qz > zmin and count as fragile.  What |qz| <= 1e-6 does to a VALID point (the derivative of 1 / z switched off) is the business of the
``micro`` cases: a whole scene at the scale of 1e-6, where 1e-7 < qz <= 1e-6 holds for a third of the points, far from both thresholds in
float32 terms -- valid at zmin = 1e-7, invalid at zmin = 1e-6.  The first point of every segment is kept natural, interior and valid.

Seeds were chosen on the CPU so that the per-segment and per-tile edge cases (NO_FRAGILE) hold no fragile point at all and the others at
most 0.2 % of their valid points (tests/test_single_cost_ref_host.py asserts both)."""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
H, W = 40, 56
LEVEL_HW = {0: (40, 56), 1: (20, 28)}
TRIPS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769)
K_SRC = np.array([[52.0, 0, 27.3], [0, 49.0, 19.6], [0, 0, 1]], f32)

# name -> counts (a tuple, or ("random", N, lo, hi)), tile split {segment: sizes}, B, affine pair, zmin, level, pose kind, seed
SPECS = {
    "trips-a": dict(counts=TRIPS, B=1, aff=False, zmin=1e-7, level=0, seed=1),
    "trips-b": dict(counts=TRIPS, B=3, aff=True, zmin=1e-6, level=1, seed=20),
    "split": dict(counts=(0, 513, 0, 40, 0), split={1: (300, 212, 1)}, B=3, aff=True, zmin=1e-7, level=1, seed=20),
    "tiles-1": dict(counts=("random", 1, 30, 40), B=1, aff=False, zmin=1e-7, level=0, seed=4),
    "tiles-7": dict(counts=("random", 7, 3, 40), B=3, aff=True, zmin=1e-6, level=1, seed=5),
    "tiles-8": dict(counts=("random", 8, 3, 40), B=1, aff=True, zmin=1e-7, level=0, seed=6),
    "tiles-9": dict(counts=("random", 9, 3, 40), B=3, aff=False, zmin=1e-6, level=1, seed=7),
    "tiles-63": dict(counts=("random", 63, 3, 40), B=1, aff=False, zmin=1e-7, level=1, seed=8),
    "tiles-64": dict(counts=("random", 64, 3, 40), B=3, aff=True, zmin=1e-7, level=0, seed=20),
    "tiles-65": dict(counts=("random", 65, 3, 40), B=3, aff=False, zmin=1e-6, level=0, seed=10),
    "tiles-130": dict(counts=("random", 130, 3, 40), B=3, aff=True, zmin=1e-6, level=1, seed=20),
    "n300": dict(counts=("random", 300, 0, 4), B=3, aff=True, zmin=1e-6, level=0, seed=12),
    "behind": dict(counts=(400, 300, 257, 100), B=3, aff=True, zmin=1e-7, level=0, pose="behind", seed=13),
    "nothing": dict(counts=(100, 257), B=3, aff=True, zmin=1e-7, level=1, pose="nothing", seed=14),
    "micro-a": dict(counts=(300, 500), B=1, aff=True, zmin=1e-7, level=0, pose="micro", seed=15),
    "micro-b": dict(counts=(300, 500), B=1, aff=True, zmin=1e-6, level=0, pose="micro", seed=15),
    "big": dict(counts=(4500,), split={0: (2048, 2048, 404)}, B=3, aff=True, zmin=1e-7, level=0, seed=16),
    "stats": dict(counts=(0, 17, 0, 0, 120, 1, 64, 0), B=3, aff=True, zmin=1e-7, level=1, seed=17),
    "stats-1": dict(counts=(97,), B=1, aff=False, zmin=1e-6, level=0, seed=18),
    "fd": dict(counts=(60, 45, 1, 30), B=2, aff=True, zmin=1e-7, level=1, seed=19),
}
COST_CASES = ["trips-a", "trips-b", "split", "tiles-1", "tiles-7", "tiles-8", "tiles-9", "tiles-63", "tiles-64", "tiles-65", "tiles-130", "n300", "behind",
              "nothing", "micro-a", "micro-b", "big"]
NO_FRAGILE = ["trips-a", "trips-b", "split", "tiles-1", "tiles-7", "tiles-8", "tiles-9", "tiles-63", "tiles-64", "tiles-65", "tiles-130", "fd"]
# explicit point lists: (n_points, P_total - n_points, B, affine pair, zmin, level), cut from the ``big`` table
POINT_CASES = [(1, 0, 1, False, 1e-7, 0), (255, 37, 3, True, 1e-7, 1), (256, 0, 1, True, 1e-6, 0), (257, 37, 1, False, 1e-7, 1), (2047, 0, 3, False, 1e-6, 0),
               (2048, 37, 1, True, 1e-7, 0), (2049, 0, 3, True, 1e-7, 1), (4097, 37, 3, True, 1e-6, 0)]
STATS_STRIDES = ("1", "2", "5", "P-1", "P", "P+3")


def _rot(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _targets(rng, B, Hl, Wl):
    """smooth, textured target levels (B,Hl,Wl,3) in about [0.1, 0.9]"""
    y, x = np.mgrid[0:Hl, 0:Wl]
    img = np.zeros((B, Hl, Wl, 3))
    for b in range(B):
        for ch in range(3):
            for _ in range(4):
                fxy = rng.uniform(0.05, 0.45, 2) * (40.0 / Hl)
                img[b, :, :, ch] += rng.uniform(0.05, 0.1) * np.sin(fxy[0] * x + fxy[1] * y + rng.uniform(0, 6.28))
    return (0.5 + img).astype(f32)


def _poses(rng, B, kind):
    poses = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        if kind == "micro":                                          # pure translation at the scene's scale
            poses[b, :3, 3] = 1e-6 * np.array([0.05, -0.03, 0.3]) * (b + 1)
            continue
        deg = {"normal": 2.0 + 1.5 * b, "behind": 9.0 + 2.0 * b, "nothing": 1.0}[kind]
        poses[b, :3, :3] = _rot(rng.normal(size=3) if kind != "behind" else (0.1, 1.0, 0.05), deg)
        poses[b, :3, 3] = [0.12 * rng.uniform(-1, 1), 0.08 * rng.uniform(-1, 1), -0.04 * (b + 1)]
        if kind == "behind":
            poses[b, 2, 3] = -0.5                                    # the near half of the depths ends up behind the camera
        if kind == "nothing":
            poses[b, 2, 3] = -100.0
    return poses.astype(f32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: tables (pix, src4, kp_L, kld, K_src, H, W), seg_off (N+1), tiles (T,4), seg_tile_off (N+1), N, P, B, poses (B,4,4), K_trg (B,3,3),
    trg (B,Hl,Wl,3), aff None or (aff_src (2,), aff_trg (B,2)), zmin, counts, planted {kind: point indices}"""
    sp = SPECS[name]
    rng = np.random.default_rng(1000 + sp["seed"])
    counts = sp["counts"]
    if counts[0] == "random":
        counts = rng.integers(counts[2], counts[3] + 1, counts[1])
    counts = np.asarray(counts, np.int64)
    N, P, B = len(counts), int(counts.sum()), sp["B"]
    kind = sp.get("pose", "normal")
    seg = np.repeat(np.arange(N), counts)
    seg_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    first = seg_off[:-1][counts > 0]
    # pixels: the frame's pixels in a random order, as often as needed; the first point of every segment interior
    order = np.concatenate([rng.permutation(H * W) for _ in range(P // (H * W) + 1)])[:P]
    col, row = order % W, order // W
    col[first], row[first] = rng.integers(20, 35, len(first)), rng.integers(13, 27, len(first))
    bit = rng.random(P) > 0.05
    bit[first] = True
    scale = 1e-6 if kind == "micro" else 1.0
    depth = (1.4 + 0.8 * np.sin(0.11 * col + 0.3) * np.cos(0.13 * row) + 0.5 * rng.random(N)[seg]) * scale
    if kind == "micro":
        depth = depth * np.where(np.arange(P) % 3 == 1, 0.25, 1.0)  # a third of the points: qz in (1e-7, 1e-6]
    kp_L = (np.log(scale) + rng.normal(0.7, 0.1, N)).astype(f32)
    kld = (kp_L + rng.normal(0, 0.05, N)).astype(f32)
    poses = _poses(rng, B, kind)
    K_trg = np.stack([K_SRC.astype(f64) * np.array([[1 + 0.03 * (b + 1), 1, 1 + 0.01 * b], [1, 1 - 0.02 * (b + 1), 1 - 0.015 * b], [1, 1, 1]]) for b in range(B)]).astype(f32)
    # planted points: never the first of a segment, only in segments of three points and more
    room = np.nonzero((counts[seg] >= 3) & ~np.isin(np.arange(P), first))[0]
    planted = {}
    if len(room) >= 10 and kind != "micro":
        pick = rng.choice(room, 10, replace=False)
        planted = dict(band_x=pick[0:2], band_y=pick[2:4], behind=pick[4:6], dead=pick[6:8], guard=pick[8:10])
        col[pick[:4]], row[pick[:4]] = rng.integers(20, 35, 4), rng.integers(13, 27, 4)
        col[planted["band_x"]], row[planted["band_y"]] = W + 10, H + 10
        bit[pick[:8]] = True
        depth[planted["behind"]] = 1e-3
        bit[planted["guard"]] = False
        col[planted["guard"]], row[planted["guard"]] = rng.integers(20, 35, 2), rng.integers(13, 27, 2)
        ray = np.stack(((col[planted["guard"]] - f64(K_SRC[0, 2])) / f64(K_SRC[0, 0]), (row[planted["guard"]] - f64(K_SRC[1, 2])) / f64(K_SRC[1, 1]), np.ones(2)), axis=1)
        depth[planted["guard"]] = -f64(poses[0, 2, 3]) / (ray @ poses[0, 2, :3].astype(f64))
    shift = (kld.astype(f64) - kp_L.astype(f64))[seg]
    w = np.log(depth) - shift
    if planted:
        w[planted["dead"]] = -30.0 - shift[planted["dead"]]
    src4 = np.concatenate((rng.uniform(0.05, 0.95, (P, 3)), w[:, None]), axis=1).astype(f32)
    pix = (col.astype(np.uint32) | (row.astype(np.uint32) << np.uint32(16)) | (bit.astype(np.uint32) << np.uint32(31))).astype(np.uint32)
    # the work list: one tile per non-empty segment, or the hand-chosen split
    tiles, sto = [], [0]
    for n in range(N):
        sizes = sp.get("split", {}).get(n, (int(counts[n]),) if counts[n] else ())
        assert sum(sizes) == counts[n]
        start = int(seg_off[n])
        for s in sizes:
            tiles.append((0, n, start, s))
            start += s
        sto.append(len(tiles))
    Hl, Wl = LEVEL_HW[sp["level"]]
    aff = None
    if sp["aff"]:
        aff = (np.array([0.03, -0.02], f32), np.stack([np.array([-0.05 + 0.045 * b, 0.02 - 0.015 * b], f32) for b in range(B)]))
    tables = dict(pix=pix, src4=src4, kp_L=kp_L, kld=kld, K_src=K_SRC, H=H, W=W)
    return dict(name=name, tables=tables, seg_off=seg_off, tiles=np.asarray(tiles, np.int32).reshape(-1, 4), seg_tile_off=np.asarray(sto, np.int32), N=N, P=P, B=B,
                poses=poses, K_trg=K_trg, trg=_targets(rng, B, Hl, Wl), aff=aff, zmin=sp["zmin"], counts=counts, planted=planted, kind=kind)


def cost_ref(name, **kw):
    import single_cost_ref as ref
    c = case(name)
    return ref.photo_cost_grad_ref(c["tables"], c["tiles"], c["seg_tile_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], c["zmin"], **kw)


@functools.lru_cache(maxsize=None)
def cost_ref_cached(name):
    return cost_ref(name)


def stride_of(tag, P):
    return {"1": 1, "2": 2, "5": 5, "P-1": P - 1, "P": P, "P+3": P + 3}[tag]


@functools.lru_cache(maxsize=None)
def stats_ref_cached(name, stride, source_only=False):
    import single_cost_ref as ref
    c = case(name)
    return ref.photo_stats_ref(c["tables"], c["seg_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], None if source_only else c["trg"], c["aff"], c["zmin"], stride)


@functools.lru_cache(maxsize=None)
def point_list():
    """xyz (n,3), rgb (n,3) float32 of the ``big`` table's points whose source bit is set (those of depth <= 1e-7 stay in), two depths made 0 and
    negative"""
    c = case("big")
    st = stats_ref_cached("big", 1, True)
    keep = (c["tables"]["pix"] >> np.uint32(31)) == 1
    xyz, rgb = st["src_pts"][keep].astype(f32), st["src_rgb"].T[keep].astype(f32)
    xyz[100], xyz[2100] = (0.1, 0.1, 0.0), (0.1, -0.1, -1.5)
    assert len(xyz) >= 4097 and (xyz[:255, 2] <= 1e-7).any()
    return xyz, rgb


def point_case(i):
    """the inputs of POINT_CASES[i]: dict(xyz, rgb, n, P_total, H, W, B, poses, K_trg, trg, aff, zmin)"""
    n, extra, B, with_aff, zmin, level = POINT_CASES[i]
    c = case("big")
    rng = np.random.default_rng(2000 + i)
    xyz, rgb = point_list()
    Hl, Wl = LEVEL_HW[level]
    aff = (c["aff"][0], c["aff"][1][:B]) if with_aff else None
    if n == 1:
        xyz, rgb = xyz[1:], rgb[1:]                                   # (a single point, and a valid one)
    return dict(xyz=np.ascontiguousarray(xyz[:n]), rgb=np.ascontiguousarray(rgb[:n]), n=n, P_total=n + extra, H=H, W=W, B=B, poses=c["poses"][:B], K_trg=c["K_trg"][:B],
                trg=_targets(rng, B, Hl, Wl), aff=aff, zmin=zmin)


@functools.lru_cache(maxsize=None)
def point_ref_cached(i):
    import single_cost_ref as ref
    p = point_case(i)
    return ref.points_cost_grad_ref(p["xyz"], p["rgb"], p["n"], p["P_total"], p["H"], p["W"], p["B"], p["poses"], p["K_trg"], p["trg"], p["aff"], p["zmin"])
