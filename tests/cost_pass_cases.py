"""Inputs of the cost-pass tests, shared by test_cost_pass_ref_host.py (CPU: the reference of tests/cost_pass_ref.py against the
finite-difference oracle, the fragile-point condition, fifteen planted errors) and test_gpu_cost_pass.py (one launch per case and variant
against that reference).  numpy only.  A SCENE is one frame pair as PairBatch takes it -- source keyframe, target image, both cameras, pose,
log-depth seeds, affine pair; a CASE is one or two scenes with the work-list sizes and IRLS epsilons it is run at.  Every case is a few
thousand points, and each exists because of one way the pass can go wrong:

    base        48 x 64, N = 6, the grid and the blobs pair of test_gn_normal_equations_match_oracle_jacobian; levels 0 and 1 (at level 1
                ax, ay != 1 and src4 holds pyramid samples)
    intrinsics  K_trg with fx, fy, cx, cy 3-7 % off K_src: swapping the cameras, or fx with fy, is invisible on synth pairs
    rotation    0.1 rad about each axis and a translation of three different sizes: no row of R, no column of Ahat near zero
    affine      aff = {0.03, -0.02, -0.05, 0.04}: gain and bias enter r and J in mode 1 as well
    validity    a segment behind the camera (wholly invisible: its records are exact zeros), points beyond the 0.99 band on all four sides,
                source pixels of the outermost rows and columns (src_ok clear)
    records     45 x 67, 20 thinned blobs with single-pixel and empty segments and one longer than tile_points, tile_points = 256 and a span
                size that puts a dozen chunks of different segments into one span: every flush, every cost_mark difference
    eps         irls_eps 1e-3 and 5e-2 (most channels on the eps branch of max(|r|, eps))

Run descriptors need every 64-point group of a table to lie in at most two pixel runs, i.e. segments at least 64 pixels wide: the
single-scene cases use full-width row BANDS as segments (ragged heights, overlapping), and base / records have a band twin (base_rd,
records_rd) for the descriptor variants.
"""
import functools
import zlib

import numpy as np

import point_table_ref as ptr

f32, f64 = np.float32, np.float64
WAVE_SPANS, DEPTH_TABLE = 0x100, 0x200

# name -> mode, padding granule, depth tables, run descriptors (every mode-0/1/2 entry of the library's variant table that sp_pairs_cost_opt reaches)
VARIANTS = {
    "1": dict(mode=1, granule=256, dt=False, rd=False),
    "1|DT": dict(mode=1, granule=256, dt=True, rd=False),
    "1|W64": dict(mode=1, granule=64, dt=False, rd=False),
    "1|DT|W64": dict(mode=1, granule=64, dt=True, rd=False),
    "1|DT|W64+RD": dict(mode=1, granule=64, dt=True, rd=True),
    "2": dict(mode=2, granule=256, dt=False, rd=False),
    "0": dict(mode=0, granule=256, dt=False, rd=False),
    "0|DT|W64": dict(mode=0, granule=64, dt=True, rd=False),
    "0|DT|W64+RD": dict(mode=0, granule=64, dt=True, rd=True),
}
GN_VARIANTS = ["1", "1|DT", "1|W64", "1|DT|W64", "1|DT|W64+RD", "2"]
GRAD_VARIANTS = ["0", "0|DT|W64", "0|DT|W64+RD"]


def mode_flags(variant):
    v = VARIANTS[variant]
    return v["mode"] | (WAVE_SPANS if v["granule"] == 64 else 0) | (DEPTH_TABLE if v["dt"] else 0)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def _scene(p, masks=None, kp_rc=None, K_trg=None, pose=None, kld=None, aff=None, key=0):
    """A scene from a synthetic pair; ``masks`` (N,H,W) / ``kp_rc`` (N,2) replace its segments (log-depths = log of the pair's depth map
    minus a per-segment offset, seeds log(2 + 2 rand), as synth lays them out)."""
    rng = _rng("scene", key)
    if masks is None:
        masks, logdepth, keypoints, kld0 = p.keypoint_regions, p.logdepth_perseg, p.keypoints, p.kld_init
    else:
        N = len(masks)
        offs = rng.uniform(-0.7, 0.7, N)
        logdepth = ((np.log(p.depth.astype(f64))[None] - offs[:, None, None]) * masks).astype(f32)
        keypoints = np.stack([2.0 * kp_rc[:, 0] / (p.H - 1) - 1.0, 2.0 * kp_rc[:, 1] / (p.W - 1) - 1.0], 1).astype(f32)
        kld0 = np.log(2.0 + 2.0 * rng.uniform(size=N)).astype(f32)
    return dict(H=p.H, W=p.W, N=len(masks), image=p.src_image, trg_image=p.trg_image, K=p.K.astype(f32), K_trg=(p.K if K_trg is None else K_trg).astype(f32),
                logdepth=logdepth, keypoints=keypoints, masks=np.asarray(masks, bool), kld=(kld0 if kld is None else kld).astype(f32),
                pose=(p.pose_init if pose is None else pose).astype(f32), aff=None if aff is None else np.asarray(aff, f32))


def bands(H, W, rows, singles=(), empties=()):
    """Segments as full-width row bands ``rows`` = [(r0, r1)]; segment n of ``singles`` is cut down to one pixel, of ``empties`` to none.
    Returns (masks, kp_rc): the keypoint is a pixel of the segment (an empty segment keeps the band's)."""
    N = len(rows)
    masks, kp = np.zeros((N, H, W), bool), np.zeros((N, 2), np.int64)
    for n, (r0, r1) in enumerate(rows):
        masks[n, r0:r1] = True
        kp[n] = ((r0 + r1 - 1) // 2, (W // 2 + 5 * n) % W)
        if n in singles or n in empties:
            masks[n] = False
            masks[n, kp[n, 0], kp[n, 1]] = n in singles
    return masks, kp


def _ragged_rows(H, heights, key):
    rng = _rng("rows", key)
    return [(int(r0), int(r0) + h) for h, r0 in ((h, rng.integers(0, H - h + 1)) for h in heights)]


@functools.lru_cache(maxsize=None)
def _pair(H, W, N, seed, shape):
    from super_primitive_amd import synth
    return synth.make_pair(H, W, N, seed=seed, shape=shape, init_sigma=0.01)


BAND_HEIGHTS = (1, 3, 9, 14, 5, 2, 11)
RECORDS_SEED, RECORDS_RD_SEED = 9, 66          # picked so that no point of the two cases is fragile, with a factor 3 to spare on every delta


def _band_scene(seed, key, **kw):
    p = _pair(48, 64, 6, seed, "grid")
    masks, kp = bands(48, 64, _ragged_rows(48, BAND_HEIGHTS, key))
    return _scene(p, masks, kp, key=key, **kw)


def _records_scene():
    p = _pair(45, 67, 20, RECORDS_SEED, "blobs")
    m = p.keypoint_regions.copy()
    big = int(m.reshape(20, -1).sum(1).argmax())
    thin = _rng("records").uniform(size=m.shape) < 0.25
    thin[big] = True
    m &= thin
    kp = p.meta["kp_rc"]
    for n in range(20):
        m[n, kp[n, 0], kp[n, 1]] = True
    for n in (2, 9, 16):
        if n != big:
            m[n] = False
            m[n, kp[n, 0], kp[n, 1]] = True
    for n in (5, 13):
        if n != big:
            m[n] = False
    return _scene(p, m, kp, key="records")


def _records_rd_scene():
    p = _pair(45, 67, 20, RECORDS_RD_SEED, "blobs")
    heights = (1, 2, 5, 1, 3, 1, 2, 4, 1, 1, 6, 2, 1, 3, 1, 2, 1, 4, 2, 1)
    masks, kp = bands(45, 67, _ragged_rows(45, heights, "records_rd"), singles=(3, 8, 14), empties=(5, 15))
    return _scene(p, masks, kp, key="records_rd")


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(scenes, levels (the pyramid levels it is evaluated at), eps (the IRLS epsilons), tile_points, span_points {granule: points})"""
    from super_primitive_amd import synth
    c = dict(name=name, levels=(0,), eps=(1e-3,), tile_points=512, span_points={256: 2048, 64: 512})
    if name == "base":
        c.update(scenes=[_scene(_pair(48, 64, 6, 3, "grid")), _scene(_pair(48, 64, 6, 4, "blobs"))], levels=(0, 1))
    elif name == "base_rd":
        g, b = _pair(48, 64, 6, 3, "grid"), _pair(48, 64, 6, 4, "blobs")
        c.update(scenes=[_scene(g, *bands(48, 64, [(8 * n, 8 * n + 8) for n in range(6)]), key="base_rd grid"),
                         _scene(b, *bands(48, 64, _ragged_rows(48, BAND_HEIGHTS, "base_rd")), key="base_rd blobs")], levels=(0, 1))
    elif name == "intrinsics":
        p = _pair(48, 64, 6, 5, "grid")
        K = p.K.astype(f64).copy()
        K[0, 0] *= 1.05; K[1, 1] *= 0.96; K[0, 2] *= 1.03; K[1, 2] *= 0.94
        c.update(scenes=[_band_scene(5, "intrinsics", K_trg=K)])
    elif name == "rotation":
        pose = synth.se3_exp_np(np.array([0.30, -0.15, 0.08, 0.1, 0.1, 0.1]))
        c.update(scenes=[_band_scene(6, "rotation", pose=pose)])
    elif name == "affine":
        c.update(scenes=[_band_scene(7, "affine", aff=(0.03, -0.02, -0.05, 0.04))])
    elif name == "validity":
        p = _pair(48, 64, 6, 8, "grid")
        masks, kp = bands(48, 64, [(8 * n, 8 * n + 8) for n in range(6)])
        pose = np.eye(4)
        pose[:3, 3] = (0.02, -0.01, -1.0)
        kld = np.log(np.array([0.5, 3.0, 2.8, 3.1, 2.9, 3.0]))
        c.update(scenes=[_scene(p, masks, kp, pose=pose, kld=kld, key="validity")])
    elif name == "eps":
        c.update(scenes=[_band_scene(9, "eps")], eps=(1e-3, 5e-2))
    elif name == "records":
        c.update(scenes=[_records_scene()], tile_points=256, span_points={256: 3072, 64: 1536})
    elif name == "records_rd":
        c.update(scenes=[_records_rd_scene()], tile_points=256, span_points={256: 3072, 64: 1536})
    else:
        raise KeyError(name)
    return c


def case_for(name, variant):
    """base and records have a band twin for the run-descriptor variants"""
    return name + "_rd" if VARIANTS[variant]["rd"] and name in ("base", "records") else name


def runs(variants, cases):
    """[(case, variant, level, eps)] of every evaluation of ``cases`` under ``variants``"""
    out = []
    for v in variants:
        for name in cases:
            c = case(case_for(name, v))
            out += [(c["name"], v, l, e) for l in c["levels"] for e in c["eps"]]
    return out


# base and records on all six Gauss-Newton variants; the other cases on the benchmark's variant and on mode 2
GN_RUNS = runs(GN_VARIANTS, ["base", "records"]) + runs(["1|DT|W64+RD", "2"], ["intrinsics", "rotation", "affine", "validity", "eps"])
GRAD_RUNS = runs(GRAD_VARIANTS, ["base", "intrinsics", "records"])
ALL_CASES = ["base", "base_rd", "intrinsics", "rotation", "affine", "validity", "eps", "records", "records_rd"]
NO_FRAGILE = ("records", "records_rd")                  # per-record cases: no fragile point at all


def scene_aff(sc, variant):
    """the affine pair a variant runs a scene with: the scene's own; mode 2 always has one (zeros: gain 1, bias 0)"""
    if sc["aff"] is not None:
        return sc["aff"]
    return np.zeros(4, f32) if VARIANTS[variant]["mode"] == 2 else None


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch's inputs on the host: tables from the point-table reference, work list from the header's description
# ---------------------------------------------------------------------------------------------------------------------------------
def work_list(counts_per_pair, granule, tile_points, span_points):
    """include/sp_hip.h, "Work list": every segment's padded run cut into pieces of at most tile_points points (granule-aligned, nearly
    equal), spans = greedy runs of consecutive chunks of one pair up to span_points points.  Returns (chunks (C,4), spans (S,4)) int32."""
    chunk_max = max(granule, tile_points // granule * granule)
    chunks, spans = [], []
    for m, counts in enumerate(counts_per_pair):
        first, off = len(chunks), 0
        for n, cnt in enumerate(counts):
            pc = -(-int(cnt) // granule) * granule
            k = -(-pc // chunk_max)
            if k:
                per = -(-(pc // granule) // k) * granule
                done = 0
                while done < pc:
                    c = min(per, pc - done)
                    chunks.append((m, n, off + done, c))
                    done += c
            off += pc
        q = first
        while q < len(chunks):
            q1, pts = q, 0
            while q1 < len(chunks) and (q1 == q or pts + chunks[q1][3] <= span_points):
                pts += chunks[q1][3]
                q1 += 1
            spans.append((q, q1 - q, pts, m))
            q = q1
    return np.asarray(chunks, np.int32).reshape(-1, 4), np.asarray(spans, np.int32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _scene_tables(name, i):
    sc = case(name)["scenes"][i]
    t = ptr.table_ref(sc["masks"], sc["logdepth"], sc["keypoints"])
    s = ptr.source_ref(t, sc["K"], sc["kld"], sc["H"], sc["W"])
    n_levels = max(case(name)["levels"]) + 1
    return t, s, ptr.pyramid_ref(sc["image"], n_levels), ptr.pyramid_ref(sc["trg_image"], n_levels)


def host_launch(name, variant, level, table_dtype=f32, zmin=1e-7):
    """(pairs, chunks, spans, mode | flags) of case ``name`` under ``variant`` at ``level`` without a GPU: the tables of the point-table
    reference (tests/point_table_ref.py) in the batch's padded layout, rounded to ``table_dtype`` (float64: not rounded at all)."""
    import cost_pass_ref as ref
    c, v = case(name), VARIANTS[variant]
    pairs, counts = [], []
    for i, sc in enumerate(c["scenes"]):
        t, s, lv, lv_t = _scene_tables(name, i)
        pos, pad, total = ptr.padded_layout(t["counts"], v["granule"])
        pix = np.zeros(total, np.uint32)
        pix[pos] = t["pix"] | (s["ok"].astype(np.uint32) << np.uint32(31))
        val, _ = ptr.sample_ref(lv[level], s["xn"], s["yn"], (sc["H"], sc["W"]))
        src4 = np.zeros((total, 4), table_dtype)
        src4[pos, :3] = val.T.astype(table_dtype)
        L = t["baseL"].astype(f64)
        src4[pos, 3] = (np.exp(L) if v["dt"] else L).astype(table_dtype)
        trg = ptr.pack_ref(lv_t[level]).astype(table_dtype)
        k4 = lambda K: (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        pairs.append(ref.pair_inputs(pix, src4, t["kp_L"], sc["kld"], trg, k4(sc["K"]), k4(sc["K_trg"]), sc["H"], sc["W"], trg.shape[0], trg.shape[1],
                                     len(t["pix"]), zmin, sc["pose"], scene_aff(sc, variant)))
        counts.append(t["counts"])
    chunks, spans = work_list(counts, v["granule"], c["tile_points"], c["span_points"][v["granule"]])
    return pairs, chunks, spans, mode_flags(variant)
