"""-m gpu: the single-keyframe cost API -- sp_photo_cost_grad, sp_points_cost_grad, sp_photo_stats, through the C ABI -- against the float64
reference of tests/single_cost_ref.py, entry by entry and point by point, on the hand-made tables of tests/single_cost_cases.py: tile
sizes 1 ... 769 (every trip count and tail of the tile loop, both parities of its software pipeline), a segment cut into 300 + 212 + 1,
segments without tiles first / in the middle / last, 1 ... 130 tiles (the 8-way block remap, the finalise's lane loop over tiles), 300
segments (its thread loop over segments), B = 1 and 3 with a pose, intrinsics and affine pair per target, levels with ax, ay = 1 and != 1,
zmin 1e-7 and 1e-6 (with a scene in which they differ in effect), a pose that loses two thirds of the points, one that loses all of
them; explicit lists of 1 ... 4097 points (the 2048-point tiles and their tails), P_total = n and n + 37, dead points in the list, the
workspace exactly as large as sp_points_workspace_floats says; the diagnostics at strides 1, 2, 5, P - 1, P, P + 3 over empty segments
first, in the middle, two in a row and last, N = 1, the source-only form, each output pointer NULL in turn.  Every output and the
workspace is pre-filled with a sentinel, and a tail behind each must survive.

SUMMED OUTPUTS:  |got - want64| <= KAPPA n_e + allowance_e + ulp32(want64) for every entry (KAPPA_MANY for entries that sum 16 valid
points and more), and exactly: g_pose row 3 = 0, g_aff = 0 without an affine pair, g_aff[b,0:2] = -g_aff[b,2:4] bitwise, g_kld = 0 for a
segment without tiles.  tests/test_single_cost_ref_host.py shows on the CPU that this comparison catches every planted error
-- a dropped last trip, first point or final fold, n_points for P_total, target b read with the data of b - 1, ... -- at least 2900 times
over; a kernel with one of them fails here.  KAPPA is measured: worst (err - ulp32) / n_e on gfx950 over all cases of this file,

                                   residual  g_t    g_R    g_aff  g_kld
    sp_photo_cost_grad             0.157     0.568  0.633  0.220  6554.5        entries of 16+ valid points: 0.157  0.568  0.633  0.220  1.510
    sp_points_cost_grad            19.47     2.193  1.890  0.102  --                                         0.278  0.429  0.413  0.102
    photomeric_cost_precomputed    0.000     0.218  0.298  0.000  --            (and photomeric_cost_batch's backward: 0.25 of its bound at most)

times four, rounded up to one digit: KAPPA = 30000 for every entry, KAPPA_MANY = 7 for the entries that sum 16 valid points and more.
KAPPA exceeds the many-pairs pass's 200 because of ONE entry: g_kld of a single-point segment of case n300 (target 2, segment 146),
where n_e is one draw of the float32 twin's rounding error and came out at 1.7e-10 of the entry -- the median over the single-point
entries is 7.4e-7 -- while the device's error there is 1.2e-6 of the entry (its three terms cancel to a twentieth of their size).  The
19.47 is the residual of the one-point list, the next largest g_kld figure 6.8 (five valid points); everything else lies below 4.2.  What
pins the kernels is KAPPA_MANY, four times tighter than the many-pairs pass's 30, and the planted errors above are judged with both.
Nothing in the kernels was found wrong.

PER-POINT OUTPUTS:  seg_ids, src_rgb, src_valid exact; trg_valid exact except at the points the reference flags as fragile; src_pts,
trg_pts, trg_rgb, raw within the bound derived from the operation chain (tests/single_cost_ref.py), in which the kernel's expf and
reciprocal enter with four times their measured distance from the float64 value:

    expf against exp of its own float32 argument: 0.745 ulp at most  ->  EXP_ULPS = 3
    the reciprocal is not observable alone (no output holds 1 / z or the sampling position): RCP_ULPS = 4, four times the 1 ulp of the ISA manual
    worst |err| / bound over the runs below:  src_pts 0.386   trg_pts 0.826   trg_rgb 0.313   raw 0.153

Odd but harmless, pinned as it is: sp_photo_stats' trg_valid ignores the source bit (the reference's trg_valid_mask does too); its
trg_rgb at a point outside the image is the zero-padded bilinear value; sp_photo_cost_grad never reads seg_off.
"""
import functools

import numpy as np
import pytest
import torch

import single_cost_cases as cases
import single_cost_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SENTINEL = 1.0e30
TAIL = 5                                        # elements behind every buffer that no call may touch
WORST, WORST_MANY, WORST_STATS = {}, {}, {}
EXP_DIST = [0.0]


def _buf(n, dtype=torch.float32, fill=SENTINEL):
    return torch.full((n + TAIL,), fill, dtype=dtype, device="cuda:0")


def _tail_ok(t, n, fill=SENTINEL):
    return bool((t[n:] == torch.tensor(fill, dtype=t.dtype)).all())


def _i32(a):
    return T(np.ascontiguousarray(a).view(np.int32) if np.asarray(a).dtype == np.uint32 else np.ascontiguousarray(a, np.int32))


def _aff_ptrs(aff):
    if aff is None:
        return None, None
    return T(np.ascontiguousarray(aff[0], f32)), T(np.ascontiguousarray(aff[1], f32))


@functools.lru_cache(maxsize=None)
def _uploaded(name):
    c = cases.case(name)
    t = c["tables"]
    return dict(pix=_i32(t["pix"]), src4=T(t["src4"]), seg_off=_i32(c["seg_off"]), kp_L=T(t["kp_L"]), kld=T(t["kld"]), K_src=T(np.ascontiguousarray(t["K_src"], f32)),
                tiles=_i32(c["tiles"]), seg_tile_off=_i32(c["seg_tile_off"]), trg=T(c["trg"]), K_trg=T(c["K_trg"]), poses=T(c["poses"]), aff=_aff_ptrs(c["aff"]))


def _photo(name):
    """sp_photo_cost_grad on the case's tables: the outputs as numpy, after the sentinel checks"""
    from super_primitive_amd import _lib
    lib, c, d = _lib.load(), cases.case(name), _uploaded(name)
    B, N, P, nt = c["B"], c["N"], c["P"], len(c["tiles"])
    Hl, Wl = c["trg"].shape[1:3]
    work, res, g_kld, g_pose, g_aff = _buf(B * nt * _lib.SP_GRAD_PARTIAL_FLOATS), _buf(B), _buf(B * N), _buf(B * 16), _buf(B * 4)
    rc = lib.sp_photo_cost_grad(_lib.ptr(d["pix"]), _lib.ptr(d["src4"]), _lib.ptr(d["seg_off"]), _lib.ptr(d["kp_L"]), _lib.ptr(d["tiles"]), _lib.ptr(d["seg_tile_off"]),
                                nt, N, P, c["tables"]["H"], c["tables"]["W"], _lib.ptr(d["K_src"]), _lib.ptr(d["kld"]), _lib.ptr(d["trg"]), Hl, Wl, _lib.ptr(d["K_trg"]),
                                _lib.ptr(d["poses"]), B, _lib.ptr(d["aff"][0]), _lib.ptr(d["aff"][1]), float(c["zmin"]), _lib.ptr(work), _lib.ptr(res), _lib.ptr(g_kld),
                                _lib.ptr(g_pose), _lib.ptr(g_aff), _lib.stream_ptr())
    _lib.check(rc, "sp_photo_cost_grad")
    torch.cuda.synchronize()
    for t, n, what in ((work, B * nt * 16, "workspace"), (res, B, "residual"), (g_kld, B * N, "g_kld"), (g_pose, B * 16, "g_pose"), (g_aff, B * 4, "g_aff")):
        assert _tail_ok(t, n), f"{name}: the tail behind {what} was written"
    assert bool(torch.isfinite(work[: B * nt * 16]).all()) and not bool((work[: B * nt * 16] == SENTINEL).any()), f"{name}: a tile record was not written"
    return dict(residual=npy(res)[:B], g_kld=npy(g_kld)[: B * N].reshape(B, N), g_pose=npy(g_pose)[: B * 16].reshape(B, 4, 4), g_aff=npy(g_aff)[: B * 4].reshape(B, 4))


def _points(p):
    from super_primitive_amd import _lib
    lib = _lib.load()
    B, n = p["B"], p["n"]
    Hl, Wl = p["trg"].shape[1:3]
    nw = lib.sp_points_workspace_floats(n, B)
    assert nw == (n + 2047) // 2048 * B * _lib.SP_GRAD_PARTIAL_FLOATS
    xyz, rgb, trg, K_trg, poses = T(p["xyz"]), T(p["rgb"]), T(p["trg"]), T(p["K_trg"]), T(p["poses"])      # (held until the call has run)
    a_s, a_t = _aff_ptrs(p["aff"])
    work, res, g_pose, g_aff = _buf(nw), _buf(B), _buf(B * 16), _buf(B * 4)
    rc = lib.sp_points_cost_grad(_lib.ptr(xyz), _lib.ptr(rgb), n, p["P_total"], p["H"], p["W"], _lib.ptr(trg), Hl, Wl, _lib.ptr(K_trg), _lib.ptr(poses), B,
                                 _lib.ptr(a_s), _lib.ptr(a_t), float(p["zmin"]), _lib.ptr(work), _lib.ptr(res), _lib.ptr(g_pose), _lib.ptr(g_aff), _lib.stream_ptr())
    _lib.check(rc, "sp_points_cost_grad")
    torch.cuda.synchronize()
    for t, m, what in ((work, nw, "workspace"), (res, B, "residual"), (g_pose, B * 16, "g_pose"), (g_aff, B * 4, "g_aff")):
        assert _tail_ok(t, m), f"points {n}: the tail behind {what} was written"
    assert not bool((work[:nw] == SENTINEL).any())
    return dict(residual=npy(res)[:B], g_pose=npy(g_pose)[: B * 16].reshape(B, 4, 4), g_aff=npy(g_aff)[: B * 4].reshape(B, 4))


def _note(got, r, what, row):
    for store, mp in ((WORST, 0), (WORST_MANY, ref.MANY_POINTS)):
        for k, x in ref.ratios_by_block(got, r, mp).items():
            store.setdefault(row, {})[k] = max(store.get(row, {}).get(k, 0.0), x)
    print(f"{what}: valid {r['valid']} fragile {r['fragile']} (err - ulp32) / n_e " + ", ".join(f"{k} {x:.3f}" for k, x in ref.ratios_by_block(got, r).items()))
    print(f"    worst err / (n_e + allowance + ulp32) at " + ref.excess(got, r, 1.0, 1.0, exact=False)[1])


@pytest.mark.parametrize("name", cases.COST_CASES)
def test_photo_cost_grad_equals_the_float64_reference_entry_by_entry(name):
    c, r = cases.case(name), cases.cost_ref_cached(name)
    got = _photo(name)
    _note(got, r, name, "sp_photo_cost_grad")
    ref.compare_outputs(got, r, what=name)
    if c["kind"] == "nothing":
        assert not any(np.asarray(v).any() for v in got.values()), "nothing is valid: the residual and every gradient are exactly 0"
    again = _photo(name)
    assert all(np.array_equal(got[k], again[k]) for k in got), "the same call twice is bitwise the same"


@pytest.mark.parametrize("i", range(len(cases.POINT_CASES)), ids=[f"n{n}+{e}-B{B}-aff{int(a)}" for n, e, B, a, _, _ in cases.POINT_CASES])
def test_points_cost_grad_equals_the_float64_reference_entry_by_entry(i):
    p, r = cases.point_case(i), cases.point_ref_cached(i)
    got = _points(p)
    _note(got, r, f"points {p['n']} of {p['P_total']}", "sp_points_cost_grad")
    ref.compare_outputs(got, r, what=f"points {p['n']}")


def test_points_cost_grad_equals_photo_cost_grad_on_the_same_points():
    """the list built from the reference's src_pts / src_rgb of a table (points whose source bit is set), P_total = P: both entry points within the
    bounds of the TABLE's reference"""
    name = "trips-b"
    c, r, st = cases.case(name), cases.cost_ref_cached(name), cases.stats_ref_cached(name, 1, True)
    keep = (c["tables"]["pix"] >> np.uint32(31)) == 1
    p = dict(xyz=np.ascontiguousarray(st["src_pts"][keep].astype(f32)), rgb=np.ascontiguousarray(st["src_rgb"].T[keep].astype(f32)), n=int(keep.sum()), P_total=c["P"],
             H=cases.H, W=cases.W, B=c["B"], poses=c["poses"], K_trg=c["K_trg"], trg=c["trg"], aff=c["aff"], zmin=c["zmin"])
    no_kld = dict(r, N=0)
    ref.compare_outputs(_points(p), no_kld, what="the table's points as a list")
    ref.compare_outputs({k: v for k, v in _photo(name).items() if k != "g_kld"}, no_kld, what="the table")


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-point diagnostics
# ---------------------------------------------------------------------------------------------------------------------------------
STATS_OUT = ("src_pts", "trg_pts", "src_rgb", "trg_rgb", "raw", "src_valid", "trg_valid", "seg_ids")
FILL = {"src_valid": 0xAA, "trg_valid": 0xAA, "seg_ids": -7777}


def _stats(name, stride, skip=(), source_only=False):
    """sp_photo_stats: {output: numpy array of its Q-row shape}, the outputs in ``skip`` passed as NULL"""
    from super_primitive_amd import _lib
    lib, c, d = _lib.load(), cases.case(name), _uploaded(name)
    B, N, P = c["B"], c["N"], c["P"]
    Q = (P + stride - 1) // stride
    Hl, Wl = c["trg"].shape[1:3]
    shape = dict(src_pts=(Q, 3), trg_pts=(B, Q, 3), src_rgb=(3, Q), trg_rgb=(B, 3, Q), raw=(B, 3, Q), src_valid=(Q,), trg_valid=(B, Q), seg_ids=(Q,))
    dtype = dict(src_valid=torch.uint8, trg_valid=torch.uint8, seg_ids=torch.int64)
    bufs = {k: _buf(int(np.prod(shape[k])), dtype.get(k, torch.float32), FILL.get(k, SENTINEL)) for k in STATS_OUT}
    arg = lambda k: None if k in skip else _lib.ptr(bufs[k])
    rc = lib.sp_photo_stats(_lib.ptr(d["pix"]), _lib.ptr(d["src4"]), _lib.ptr(d["seg_off"]), _lib.ptr(d["kp_L"]), N, P, c["tables"]["H"], c["tables"]["W"], _lib.ptr(d["K_src"]),
                            _lib.ptr(d["kld"]), None if source_only else _lib.ptr(d["trg"]), Hl, Wl, None if source_only else _lib.ptr(d["K_trg"]),
                            None if source_only else _lib.ptr(d["poses"]), B, _lib.ptr(d["aff"][0]), _lib.ptr(d["aff"][1]), float(c["zmin"]), arg("src_pts"), arg("trg_pts"),
                            arg("src_rgb"), arg("trg_rgb"), arg("raw"), arg("src_valid"), arg("trg_valid"), arg("seg_ids"), stride, _lib.stream_ptr())
    _lib.check(rc, "sp_photo_stats")
    torch.cuda.synchronize()
    out = {}
    for k in STATS_OUT:
        n = int(np.prod(shape[k]))
        assert _tail_ok(bufs[k], n, FILL.get(k, SENTINEL)), f"{name} stride {stride}: the tail behind {k} was written"
        out[k] = npy(bufs[k])[:n].reshape(shape[k])
    return out


def _untouched(a, k):
    return bool((a == (FILL[k] if k in FILL else f32(SENTINEL))).all())


STATS_RUNS = [("stats", s) for s in cases.STATS_STRIDES] + [("stats-1", "1"), ("stats-1", "2"), ("stats-1", "P+3"), ("behind", "1"), ("micro-a", "5"), ("trips-b", "2")]


@pytest.mark.parametrize("name,tag", STATS_RUNS, ids=[f"{n}-stride{t}" for n, t in STATS_RUNS])
def test_photo_stats_equal_the_float64_reference_point_by_point(name, tag):
    c = cases.case(name)
    stride = cases.stride_of(tag, c["P"])
    want = cases.stats_ref_cached(name, stride)
    got = _stats(name, stride)
    assert not any(_untouched(got[k], k) for k in STATS_OUT), "an output was not written"
    n_frag, n_valid = int(want["fragile"].sum()), int((want["trg_valid"] & want["src_valid"][None]).sum())
    planted = len(c["planted"].get("guard", ())) if c["planted"] else 0
    assert n_frag <= max(0.002 * n_valid, planted), f"{n_frag} fragile points of {n_valid}"
    assert (want["checkable"] | ~want["trg_valid"]).all()
    worst, where, per = ref.stats_excess(got, want)
    for k, x in per.items():
        WORST_STATS[k] = max(WORST_STATS.get(k, 0.0), x)
    # the exponential alone: the device's depth against exp of its own float32 argument
    exact = np.exp(want["arg32"].astype(f64))
    EXP_DIST[0] = max(EXP_DIST[0], float((np.abs(got["src_pts"][:, 2].astype(f64) - exact) / ref.ulp32(exact)).max()))
    print(f"{name} stride {stride}: Q {want['Q']} fragile {n_frag}; |err| / bound " + ", ".join(f"{k} {x:.3f}" for k, x in per.items()) + f"; expf off by {EXP_DIST[0]:.3f} ulp at most so far")
    assert worst <= 1.0, f"{name} stride {stride}: |got - want| / bound = {worst:.3g} at {where}"


def test_photo_stats_without_a_target_writes_the_four_source_outputs_only():
    for name, stride in (("stats", 1), ("stats", 5), ("stats-1", 2)):
        got, want = _stats(name, stride, source_only=True), cases.stats_ref_cached(name, stride, True)
        ref.compare_stats({k: got[k] for k in ("src_pts", "src_rgb", "src_valid", "seg_ids")}, want, f"{name} source only")
        full = _stats(name, stride)
        for k in ("src_pts", "src_rgb", "src_valid", "seg_ids"):
            assert np.array_equal(got[k], full[k]), k
        for k in ("trg_pts", "trg_rgb", "raw", "trg_valid"):
            assert _untouched(got[k], k), f"{k} was written without a target"


@pytest.mark.parametrize("skip", STATS_OUT)
def test_photo_stats_with_one_output_null_leaves_the_others_unchanged(skip):
    full, got = _stats("stats", 2), _stats("stats", 2, skip=(skip,))
    for k in STATS_OUT:
        if k == skip:
            assert _untouched(got[k], k)                    # (its buffer was not passed: nothing can have reached it)
        else:
            assert np.array_equal(got[k], full[k]), f"{k} changed when {skip} was NULL"


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python layer, on the device's own table of a small synthetic pair
# ---------------------------------------------------------------------------------------------------------------------------------
def _synth():
    from gpu_util import frames_from_synth
    from super_primitive_amd import synth
    pair = synth.make_pair(40, 56, 5, seed=3, shape="blobs")
    src, trg = frames_from_synth(pair)
    return pair, src, trg


def _table_back(src, kld):
    from super_primitive_amd.segment_table import table_of
    table = table_of(src)
    src4 = table.source_level(src.image, src.K, kld)
    tables = dict(pix=npy(table.pix).view(np.uint32), src4=npy(src4), kp_L=npy(table.kp_L), kld=npy(kld), K_src=npy(src.K), H=table.H, W=table.W)
    return table, tables


def _within(got, want, bound, what):
    got, err = np.asarray(got, f64), np.abs(np.asarray(got, f64) - want)
    assert np.isfinite(got).all() and (err <= bound).all(), f"{what}: worst |err| / bound {(err / np.maximum(bound, 1e-300)).max():.3g}"
    return float((err / np.maximum(bound, 1e-300)).max())


def test_photomeric_cost_batch_backward_is_the_weighted_reference_entry_by_entry():
    from super_primitive_amd.core import dense_optim_batch
    from super_primitive_amd.segment_table import packed_target
    pair, src, trg = _synth()
    B = 3
    rng = np.random.default_rng(5)
    poses_np = np.stack([pair.pose_init.astype(f64) @ np.block([[cases._rot(rng.normal(size=3), 1.0 + b), 0.02 * rng.normal(size=(3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]])
                         for b in range(B)]).astype(f32)
    Ks_np = np.stack([pair.K.astype(f64) * np.array([[1 + 0.02 * b, 1, 1 + 0.01 * b], [1, 1 - 0.02 * b, 1], [1, 1, 1]]) for b in range(B)]).astype(f32)
    imgs = torch.stack([torch.roll(trg.image, (b, -b), (1, 2)) for b in range(B)]).contiguous()
    kld, poses = T(pair.kld_init.astype(f32), True), T(poses_np, True)
    a_s, a_t = T(np.array([0.03, -0.02], f32), True), T(np.array([[-0.05, 0.02], [0.01, -0.01], [0.04, 0.03]], f32), True)
    wts = np.array([0.5, 2.0, -1.25], f32)
    out = dense_optim_batch.photomeric_cost_batch(src, imgs, T(Ks_np), kld, poses, {"mode": "colour", "collect_stats": 0}, affine_comp=(a_s, a_t))
    (out["residual"] * T(wts)).sum().backward()
    table, tables = _table_back(src, kld)
    r = ref.photo_cost_grad_ref(tables, npy(table.tiles), npy(table.seg_tile_off), table.N, table.P, B, poses_np, Ks_np, npy(packed_target(imgs)), (npy(a_s), npy(a_t)), 1e-6)
    assert all(f <= 0.002 * v for f, v in zip(r["fragile"], r["valid"]))
    ref.compare_outputs(dict(residual=npy(out["residual"]), g_kld=r["g_kld"], g_pose=r["g_pose"], g_aff=r["g_aff"]), r, what="batch residual")
    w = wts.astype(f64)
    # a weighted sum of B float32 products: each bound weighted alike, plus the roundings of the products and of the sum
    comb = lambda key: (np.tensordot(w, r[key], 1), np.tensordot(np.abs(w), ref.bound_of(r, key), 1) + (B + 1) * ref.U * 2 * np.tensordot(np.abs(w), np.abs(r[key]), 1))
    worst = [_within(npy(kld.grad), *comb("g_kld"), "kld.grad")]
    gp, bp = w[:, None, None] * r["g_pose"], np.abs(w)[:, None, None] * ref.bound_of(r, "g_pose") + 2 * ref.U * np.abs(w[:, None, None] * r["g_pose"])
    worst.append(_within(npy(poses.grad), gp, bp, "poses.grad"))
    assert (npy(poses.grad)[:, 3] == 0).all()
    ga, ba = comb("g_aff")
    worst.append(_within(npy(a_s.grad), ga[:2], ba[:2], "aff_src.grad (the weighted sum over b)"))
    worst.append(_within(npy(a_t.grad), w[:, None] * r["g_aff"][:, 2:], np.abs(w)[:, None] * ref.bound_of(r, "g_aff")[:, 2:] + 2 * ref.U * np.abs(w[:, None] * r["g_aff"][:, 2:]),
                         "aff_trg.grad"))
    print(f"photomeric_cost_batch backward: worst |err| / bound, kld {worst[0]:.3f} poses {worst[1]:.3f} aff_src {worst[2]:.3f} aff_trg {worst[3]:.3f}")


def test_unproject_kf_then_precomputed_on_every_third_point_equals_the_point_reference():
    from super_primitive_amd.core import dense_optim
    from super_primitive_amd.segment_table import packed_target
    pair, src, trg = _synth()
    kld = T(pair.kld_init.astype(f32))
    with torch.no_grad():
        pre = dense_optim.unproject_kf(src, kld)
    table, tables = _table_back(src, kld)
    want = ref.photo_stats_ref(tables, npy(table.seg_off), table.N, table.P, 1, None, None, None, None, 1e-7)
    ref.compare_stats(dict(src_pts=npy(pre["src_pts"]), src_rgb=npy(pre["src_pixels"])[0], src_valid=npy(pre["src_valid_mask"])[0], seg_ids=npy(pre["segm_ids"])), want, "unproject_kf")
    third = dict(src_pts=pre["src_pts"][::3].contiguous(), src_pixels=pre["src_pixels"][..., ::3].contiguous(), src_valid_mask=pre["src_valid_mask"][..., ::3].contiguous(),
                 segm_ids=pre["segm_ids"][::3].contiguous(), spatial_size=pre["spatial_size"])
    pose = T(pair.pose_init.astype(f32), True)
    a_s, a_t = T(np.array([0.02, -0.01], f32), True), T(np.array([-0.03, 0.02], f32), True)
    out = dense_optim.photomeric_cost_precomputed(third, trg, pose, {"mode": "colour", "collect_stats": 0}, affine_comp=(a_s, a_t))
    out["residual"].sum().backward()
    ok = npy(third["src_valid_mask"]).reshape(-1).astype(bool)
    xyz, rgb = npy(third["src_pts"])[ok], npy(third["src_pixels"])[0].T[ok]
    r = ref.points_cost_grad_ref(xyz, rgb, len(xyz), len(ok), table.H, table.W, 1, npy(pose)[None], npy(trg.K)[None], npy(packed_target(trg.image)), (npy(a_s), npy(a_t)[None]), 1e-7)
    assert r["valid"][0] > 100 and r["fragile"][0] <= 0.002 * r["valid"][0]
    got = dict(residual=npy(out["residual"]), g_pose=npy(pose.grad)[None], g_aff=np.concatenate((npy(a_s.grad), npy(a_t.grad)))[None])
    _note(got, r, "unproject_kf -> every third point -> photomeric_cost_precomputed", "photomeric_cost_precomputed")
    ref.compare_outputs(got, r, what="photomeric_cost_precomputed")


def test_zz_worst_ratios():
    """prints what the docstring's tables hold (run the whole file with -s)"""
    for row in WORST:
        print(f"worst (err - ulp32) / n_e, {row}: " + ", ".join(f"{k} {x:.3f}" for k, x in WORST[row].items()) + f"   [KAPPA {ref.KAPPA:g}]")
        print(f"    ... over entries of {ref.MANY_POINTS}+ valid points: " + ", ".join(f"{k} {x:.3f}" for k, x in WORST_MANY[row].items()) + f"   [KAPPA_MANY {ref.KAPPA_MANY:g}]")
    print("worst |err| / bound of the per-point outputs:      " + ", ".join(f"{k} {x:.3f}" for k, x in WORST_STATS.items()))
    print(f"the kernel's expf against exp of its own argument: {EXP_DIST[0]:.3f} ulp at most   [EXP_ULPS {ref.EXP_ULPS:g}]")
    assert 4 * EXP_DIST[0] <= ref.EXP_ULPS
