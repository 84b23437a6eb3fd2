"""CPU: the single-keyframe reference (tests/single_cost_ref.py) against what it shares no code with -- central finite differences of its own
float64 residual, and the photometric oracle's autograd on a shared synthetic pair -- and what tests/test_gpu_single_cost.py relies on:
a comparison that catches every planted error below with a factor ten to spare at the KAPPA the GPU test uses (the weakest factor is
printed), and cases (tests/single_cost_cases.py) whose fragile points are at most 0.2 % of their valid points -- none in the per-segment
and per-tile edge cases -- with valid points in every non-empty segment and points that fail each validity test.

The planted errors are the ways the kernels of this path can be subtly wrong: points of a tile's last partial trip dropped, the first point
of every tile dropped (the "point -1" slot of the software pipeline), the last folded point dropped, a tile's log-depth column credited to
the next segment, 1 / (3 valid) for 1 / (3 P), n_points for P_total, the other function's zmin, target b evaluated with the intrinsics /
pose / affine pair of b - 1, g_aff halves swapped, g_R transposed, the gain missing from d/da_t, tiles past the 64th or segments past the
256th ignored by the finalise; for the per-point diagnostics: the owner of a point after an empty segment, rows at o stride + 1, and the
channel / batch strides of the (B,3,Q) layout exchanged.  That a kernel with one of them cannot pass the GPU file follows: the GPU test
applies this very comparison to the device's outputs."""

import numpy as np
import pytest
import torch

import cost_pass_cases as pass_cases
import single_cost_cases as cases
import single_cost_ref as ref
from oracle import photometric_oracle as orc

f32, f64 = np.float32, np.float64
ALL_CASES = cases.COST_CASES + ["stats", "stats-1", "fd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference is right
# ---------------------------------------------------------------------------------------------------------------------------------
def _fd_case():
    """the ``fd`` case with every float input widened to float64, so that a step of 1e-6 is not lost in the tables' rounding"""
    c = dict(cases.case("fd"))
    c["tables"] = {k: (v.astype(f64) if isinstance(v, np.ndarray) and v.dtype == f32 else v) for k, v in c["tables"].items()}
    c["poses"], c["K_trg"], c["trg"] = c["poses"].astype(f64), c["K_trg"].astype(f64), c["trg"].astype(f64)
    c["aff"] = (c["aff"][0].astype(f64), c["aff"][1].astype(f64))
    return c


def _residual(c):
    return ref.photo_cost_grad_ref(c["tables"], c["tiles"], c["seg_tile_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], c["zmin"],
                                   yardstick=False)["residual"]


def test_gradients_equal_central_differences_of_the_reference_s_own_residual():
    """Central differences at h and h / 2: the second is off by about a third of their difference (the h^2 term) plus the residual's
    rounding over the step, 2 eps64 |res| / h -- the bound is taken from the step, not from the gradient under test.  The case has no
    fragile point, and the bound itself must stay below 1e-6 of the block's largest entry: no kink of the L1 cost or of the bilinear
    slopes lies within the step."""
    c = _fd_case()
    assert sum(cases.cost_ref_cached("fd")["fragile"]) == 0
    r = ref.photo_cost_grad_ref(c["tables"], c["tiles"], c["seg_tile_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], c["zmin"], yardstick=False)
    res0 = r["residual"]
    h = 1e-6

    def central(set_value, x0, step):
        out = []
        for s in (+step, -step):
            cc = dict(c, tables=dict(c["tables"]))
            set_value(cc, x0 + s)
            out.append(_residual(cc))
        return (out[0] - out[1]) / (2 * step)

    def check(g, set_value, x0, what, b=None):
        d1, d2 = central(set_value, x0, h), central(set_value, x0, h / 2)
        bound = np.abs(d1 - d2) + 2 * np.finfo(f64).eps * np.abs(res0) / (h / 2)
        sel = slice(None) if b is None else b
        err = np.abs(np.atleast_1d(g) - d2[sel])
        assert (err <= bound[sel]).all(), f"{what}: |g - fd| = {err} bound {bound[sel]}"
        return float(np.max(bound[sel])), float(np.max(err / bound[sel]))

    worst_bound, worst = {"g_kld": 0.0, "g_pose": 0.0, "g_aff": 0.0}, 0.0
    for n in range(c["N"]):
        def set_kld(cc, v, n=n):
            k = cc["tables"]["kld"].copy()
            k[n] = v
            cc["tables"]["kld"] = k
        bd, w = check(r["g_kld"][:, n], set_kld, c["tables"]["kld"][n], f"g_kld[{n}]")
        worst_bound["g_kld"], worst = max(worst_bound["g_kld"], bd), max(worst, w)
    for b in range(c["B"]):
        for i in range(3):
            for j in range(4):
                def set_pose(cc, v, b=b, i=i, j=j):
                    p = cc["poses"].copy()
                    p[b, i, j] = v
                    cc["poses"] = p
                bd, w = check(r["g_pose"][b, i, j], set_pose, c["poses"][b, i, j], f"g_pose[{b},{i},{j}]", b)
                worst_bound["g_pose"], worst = max(worst_bound["g_pose"], bd), max(worst, w)
                # the other targets' residuals do not move
                assert (central(set_pose, c["poses"][b, i, j], h)[np.arange(c["B"]) != b] == 0).all()
        for k in range(2):
            def set_aff_trg(cc, v, b=b, k=k):
                a = cc["aff"][1].copy()
                a[b, k] = v
                cc["aff"] = (cc["aff"][0], a)
            bd, w = check(r["g_aff"][b, 2 + k], set_aff_trg, c["aff"][1][b, k], f"g_aff[{b},{2 + k}]", b)
            worst_bound["g_aff"], worst = max(worst_bound["g_aff"], bd), max(worst, w)
    for k in range(2):
        def set_aff_src(cc, v, k=k):
            a = cc["aff"][0].copy()
            a[k] = v
            cc["aff"] = (a, cc["aff"][1])
        bd, w = check(r["g_aff"][:, k], set_aff_src, c["aff"][0][k], f"g_aff[:, {k}]")
        worst_bound["g_aff"], worst = max(worst_bound["g_aff"], bd), max(worst, w)
    assert (r["g_pose"][:, 3] == 0).all()
    for k, bd in worst_bound.items():
        assert bd <= 1e-6 * np.abs(r[k]).max(), f"{k}: a kink within the step (bound {bd:.3g}, largest entry {np.abs(r[k]).max():.3g})"
    print(f"finite differences: worst |g - fd| / bound {worst:.3g}; largest bound per block {worst_bound}")


def test_float64_outputs_equal_the_oracle_s_autograd_on_a_shared_pair():
    """the ``affine`` scene of the cost-pass cases: its padded table with one tile per chunk is a valid (if unusual) single-keyframe table;
    the padding counts in P here, so the outputs scale by P_real / P_padded against the oracle's mean over the real points"""
    pairs, chunks, spans, mf = pass_cases.host_launch("affine", "0", 0, table_dtype=f64)
    sc = pass_cases.case("affine")["scenes"][0]
    pr = pairs[0]
    mine = np.nonzero(chunks[:, 0] == 0)[0]
    tiles = chunks[mine]
    N, P = len(pr["kld"]), len(pr["pix"])
    sto = np.concatenate(([0], np.cumsum(np.bincount(tiles[:, 1], minlength=N))))
    assert (np.diff(tiles[:, 1]) >= 0).all()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    src = orc.OracleFrame(t(sc["image"]), t(sc["K"]), t(sc["logdepth"]), t(sc["keypoints"]), torch.from_numpy(sc["masks"]))
    trg = orc.OracleFrame(t(sc["trg_image"]), t(sc["K_trg"]))
    kld, pose = t(sc["kld"]).requires_grad_(True), t(sc["pose"]).requires_grad_(True)
    a_s, a_t = t(sc["aff"][:2]).requires_grad_(True), t(sc["aff"][2:]).requires_grad_(True)
    res = orc.photometric_cost(src, trg, kld, pose, affine=(a_s, a_t))["residual"]
    res.sum().backward()
    tables = dict(pix=pr["pix"], src4=pr["src4"], kp_L=pr["kp_L"], kld=pr["kld"], K_src=pr["K_src"], H=pr["H"], W=pr["W"])
    r = ref.photo_cost_grad_ref(tables, tiles, sto, N, P, 1, pr["pose"][None], np.asarray(sc["K_trg"], f64)[None], pr["trg"][None], (sc["aff"][:2].astype(f64), sc["aff"][None, 2:].astype(f64)),
                                1e-7, yardstick=False)
    k = P / pr["P"]

    def close(got, want, what):
        got, want = np.asarray(got, f64) * k, np.asarray(want, f64)
        tol = 1e-6 * np.abs(want) + 1e-9 * np.abs(want).max()
        assert (np.abs(got - want) <= tol).all(), f"{what}: worst |err| / tol {(np.abs(got - want) / np.maximum(tol, 1e-300)).max():.3g}"
    np.testing.assert_allclose(r["residual"][0] * k, float(res.detach()), rtol=1e-12)
    close(r["g_kld"][0], kld.grad.numpy(), "g_kld")
    close(r["g_pose"][0], pose.grad.numpy(), "g_pose")
    close(r["g_aff"][0, :2], a_s.grad.numpy(), "g_aff source half")
    close(r["g_aff"][0, 2:], a_t.grad.numpy(), "g_aff target half")


def test_the_float32_twin_passes_the_comparison_it_defines():
    for name in cases.COST_CASES:
        r = cases.cost_ref_cached(name)
        twin = {k: r[f"twin_{k}"] for k in ("residual", "g_kld", "g_pose", "g_aff")}
        assert ref.excess(twin, r, 1.0, 1.0, exact=False)[0] <= 1.0 + 1e-6, name
        assert ref.excess({k: r[k] for k in twin}, r, 1.0, 1.0, exact=False)[0] == 0.0, name
    for i in range(len(cases.POINT_CASES)):
        r = cases.point_ref_cached(i)
        assert ref.excess({k: r[f"twin_{k}"] for k in ("residual", "g_pose", "g_aff")}, r, 1.0, 1.0, exact=False)[0] <= 1.0 + 1e-6, i


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_fragile_points_are_rare_and_absent_from_the_edge_cases(name):
    r = cases.cost_ref_cached(name)
    for b, (valid, fragile) in enumerate(zip(r["valid"], r["fragile"])):
        print(f"{name} target {b}: {fragile} fragile of {valid} valid points ({100.0 * fragile / max(valid, 1):.3f} %)")
        assert fragile <= 0.002 * valid and (fragile == 0 or name not in cases.NO_FRAGILE)
    if name in cases.NO_FRAGILE:
        assert not any(r[f"allow_{k}"].any() for k in ("residual", "g_kld", "g_pose", "g_aff"))
    if name in ("stats", "stats-1", "big"):
        s = cases.stats_ref_cached(name, 1)
        # (the two planted points with qz of target 0 within 1e-8 of zero ARE at float32's mercy against zmin: they are fragile by design)
        fragile = s["fragile"].copy()
        assert fragile[0, cases.case(name)["planted"]["guard"]].all()
        fragile[0, cases.case(name)["planted"]["guard"]] = False
        share = fragile.sum() / max(int((s["trg_valid"] & s["src_valid"][None]).sum()), 1)
        print(f"{name}: {int(fragile.sum())} points whose target validity may flip, beside the planted ones ({100.0 * share:.3f} %)")
        assert share <= 0.002 and (s["checkable"] | ~s["trg_valid"]).all()


@pytest.mark.parametrize("name", ALL_CASES)
def test_cases_have_valid_points_in_every_segment_and_points_that_fail_each_test(name):
    c, r = cases.case(name), cases.cost_ref_cached(name)
    seg = np.repeat(np.arange(c["N"]), c["counts"])
    assert c["P"] <= 20000 and c["tables"]["pix"].shape == (c["P"],) and (np.diff(c["seg_tile_off"]) >= 0).all()
    zmin = float(f32(c["zmin"]))
    for b in range(c["B"]):
        t = r["points"][b]
        per_seg = np.bincount(seg[t["m"]], minlength=c["N"])
        if c["kind"] == "nothing":
            assert not t["m"].any()
            continue
        assert (per_seg[c["counts"] > 0] > 0).all(), f"target {b}: a segment without a valid point"
        assert not per_seg[c["counts"] == 0].any()
    if c["kind"] == "nothing":                                           # (every point fails qz > zmin; what else fails is of no interest)
        return
    if c["kind"] == "behind":
        assert max(r["valid"]) <= 2 * c["P"] // 3
    if c["kind"] == "micro":
        t = r["points"][0]
        window = t["src_ok"] & (t["d"] > 1e-7) & (t["qz"] > 1e-7) & (t["qz"] <= 1e-6) & (np.abs(t["xn"]) <= 0.99) & (np.abs(t["yn"]) <= 0.99)
        assert window.sum() > 200
        a, b_ = cases.cost_ref_cached("micro-a"), cases.cost_ref_cached("micro-b")
        assert a["valid"][0] - b_["valid"][0] == window.sum()          # the single and the batch zmin differ in effect
        return
    t, pl = r["points"][0], c["planted"]
    with np.errstate(all="ignore"):
        inx, iny, front, guard, alive = np.abs(t["xn"]) <= 0.99, np.abs(t["yn"]) <= 0.99, t["qz"] > zmin, np.abs(t["qz"]) > 1e-6, t["d"] > 1e-7
    rest = (front & guard) if c["kind"] == "normal" else np.ones(c["P"], bool)      # (the other tests hold: the band alone rejects the point)
    assert (~inx & iny & rest & alive & t["src_ok"])[pl["band_x"]].all()
    assert (inx & ~iny & rest & alive & t["src_ok"])[pl["band_y"]].all()
    assert (~front & guard & alive & t["src_ok"])[pl["behind"]].all()
    assert (~alive & t["src_ok"])[pl["dead"]].all()
    assert (~guard & alive)[pl["guard"]].all()
    assert (~t["src_ok"]).sum() >= 1


def test_point_lists_hold_dead_points_and_cover_the_tile_sizes():
    xyz, rgb = cases.point_list()
    assert sorted(n for n, *_ in cases.POINT_CASES) == [1, 255, 256, 257, 2047, 2048, 2049, 4097]
    for i, (n, extra, B, aff, zmin, level) in enumerate(cases.POINT_CASES):
        p, r = cases.point_case(i), cases.point_ref_cached(i)
        assert p["xyz"].shape == (n, 3) and p["P_total"] == n + extra and len(ref.point_tiles(n)) == (n + 2047) // 2048
        assert n == 1 or (p["xyz"][:, 2] <= 1e-7).any()
        assert all(f <= 0.002 * v for f, v in zip(r["fragile"], r["valid"])) and min(r["valid"]) >= 1
        print(f"points {n} + {extra}: valid {r['valid']} fragile {r['fragile']}")


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors: each must exceed the bound at least ten times in some entry
# ---------------------------------------------------------------------------------------------------------------------------------
OUT = ("residual", "g_kld", "g_pose", "g_aff")


def _as_got(r):
    return {k: np.asarray(r[k]).astype(f32) for k in OUT if k in r}


def _in_tile(c):
    tix, _ = ref.tile_index(c["tiles"], c["P"])
    return np.arange(c["P"]) - c["tiles"][tix, 2], c["tiles"][tix, 3]


def _drop(name, which):
    c = cases.case(name)
    i, count = _in_tile(c)
    drop = {"last_partial_trip": (count % 256 != 0) & (i >= count // 256 * 256), "first_point": i == 0,
            "last_fold": i >= (np.ceil(count / 256).astype(np.int64) - 1) * 256}[which]
    return _as_got(cases.cost_ref(name, yardstick=False, drop=drop))


def _altered(name, alter):
    return _as_got(cases.cost_ref(name, yardstick=False, _alter=alter))


def _rescaled(name):
    r = cases.cost_ref_cached(name)
    k = cases.case(name)["P"] / np.asarray(r["valid"], f64)
    return _as_got({"residual": r["residual"] * k, "g_kld": r["g_kld"] * k[:, None], "g_pose": r["g_pose"] * k[:, None, None], "g_aff": r["g_aff"] * k[:, None]})


def _other_zmin(name):
    c = cases.case(name)
    return _as_got(ref.photo_cost_grad_ref(c["tables"], c["tiles"], c["seg_tile_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], 1e-6, yardstick=False))


def _previous_target(name, what):
    c = dict(cases.case(name))
    if what == "K_trg":
        c["K_trg"] = np.roll(c["K_trg"], 1, axis=0)
    elif what == "pose":
        c["poses"] = np.roll(c["poses"], 1, axis=0)
    else:
        c["aff"] = (c["aff"][0], np.roll(c["aff"][1], 1, axis=0))
    return _as_got(ref.photo_cost_grad_ref(c["tables"], c["tiles"], c["seg_tile_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], c["zmin"], yardstick=False))


def _output(name, how):
    c, g = cases.case(name), _as_got(cases.cost_ref_cached(name))
    if how == "aff_halves_swapped":
        g["g_aff"] = g["g_aff"][:, [2, 3, 0, 1]]
    elif how == "g_R_transposed":
        g["g_pose"][:, :3, :3] = g["g_pose"][:, :3, :3].transpose(0, 2, 1).copy()
    elif how == "no_gain_in_da_t":
        gain = np.exp(-(c["aff"][1][:, 0].astype(f64) - f64(c["aff"][0][0])))
        g["g_aff"][:, 2] = (g["g_aff"][:, 2] / gain).astype(f32)
        g["g_aff"][:, 0] = -g["g_aff"][:, 2]
    elif how == "segments_past_256_ignored":
        g["g_kld"][:, 256:] = 0
    return g


PLANTED = [
    ("(a) last partial trip dropped", "trips-a", lambda: _drop("trips-a", "last_partial_trip")),
    ("(a) last partial trip dropped", "big", lambda: _drop("big", "last_partial_trip")),
    ("(b) first point of every tile dropped", "trips-b", lambda: _drop("trips-b", "first_point")),
    ("(b) first point of every tile dropped", "big", lambda: _drop("big", "first_point")),
    ("(c) last folded point dropped", "trips-a", lambda: _drop("trips-a", "last_fold")),
    ("(c) last folded point dropped", "big", lambda: _drop("big", "last_fold")),
    ("(d) column 13 to segment n + 1", "split", lambda: _altered("split", "column_13_to_next_segment")),
    ("(e) 1 / (3 valid)", "trips-a", lambda: _rescaled("trips-a")),
    ("(g) zmin 1e-6 for 1e-7", "micro-a", lambda: _other_zmin("micro-a")),
    ("(h) K_trg of b - 1", "trips-b", lambda: _previous_target("trips-b", "K_trg")),
    ("(h) pose of b - 1", "trips-b", lambda: _previous_target("trips-b", "pose")),
    ("(h) affine pair of b - 1", "trips-b", lambda: _previous_target("trips-b", "aff")),
    ("(i) g_aff halves swapped", "trips-b", lambda: _output("trips-b", "aff_halves_swapped")),
    ("(j) g_R transposed", "trips-b", lambda: _output("trips-b", "g_R_transposed")),
    ("(k) gain missing from d/da_t", "trips-b", lambda: _output("trips-b", "no_gain_in_da_t")),
    ("(l) tiles past the 64th ignored", "tiles-65", lambda: _altered("tiles-65", "tiles_past_64_ignored")),
    ("(l) tiles past the 64th ignored", "tiles-130", lambda: _altered("tiles-130", "tiles_past_64_ignored")),
    ("(m) segments past the 256th ignored", "n300", lambda: _output("n300", "segments_past_256_ignored")),
]
FACTORS = {}


@pytest.mark.parametrize("what,name,make", PLANTED, ids=[f"{w}-{n}" for w, n, _ in PLANTED])
def test_planted_errors_exceed_the_bound_ten_times(what, name, make):
    r = cases.cost_ref_cached(name)
    worst, at = ref.excess(make(), r, exact=False)                      # (the bounds alone: the exact checks catch some of them at once)
    FACTORS[f"{what} on {name}"] = worst
    print(f"{what} on {name}: err / bound = {worst:.3g} at {at}")
    assert worst >= 10.0, at
    assert ref.excess(_as_got(r), r)[0] <= 1.0                          # ... and the float64 outputs, rounded once, pass with the exact checks on


def test_planted_error_n_points_for_p_total():
    i = 1                                                               # 255 points of 292
    p, r = cases.point_case(i), cases.point_ref_cached(i)
    k = p["P_total"] / p["n"]
    got = _as_got({"residual": r["residual"] * k, "g_pose": r["g_pose"] * k, "g_aff": r["g_aff"] * k})
    worst, at = ref.excess(got, r)
    FACTORS["(f) n_points for P_total"] = worst
    print(f"(f) n_points for P_total: err / bound = {worst:.3g} at {at}")
    assert worst >= 10.0, at


@pytest.mark.parametrize("alter", ["owner_without_the_skip_over_empty_segments", "rows_at_stride_plus_1", "layout_strides_exchanged"])
def test_planted_errors_in_the_diagnostics_exceed_the_bound_ten_times(alter):
    c = cases.case("stats")
    for stride in (1, 5):
        want = cases.stats_ref_cached("stats", stride)
        if alter == "layout_strides_exchanged":
            wrong = dict(want)
            for k in ("trg_rgb", "raw"):
                wrong[k] = want[k].transpose(1, 0, 2).reshape(want[k].shape)
        else:
            wrong = ref.photo_stats_ref(c["tables"], c["seg_off"], c["N"], c["P"], c["B"], c["poses"], c["K_trg"], c["trg"], c["aff"], c["zmin"], stride, _alter=alter)
        got = {k: (wrong[k].astype(f32) if wrong[k].dtype == f64 else wrong[k]) for k in ref.STATS_EXACT + ref.STATS_BOUNDED + ("trg_valid",)}
        worst, at, per = ref.stats_excess(got, want)
        FACTORS[f"(n) {alter} at stride {stride}"] = worst
        print(f"(n) {alter} at stride {stride}: |err| / bound = {worst:.3g} at {at}; per output {per}")
        assert worst >= 10.0, at
        ok = {k: (want[k].astype(f32) if want[k].dtype == f64 else want[k]) for k in got}
        assert ref.stats_excess(ok, want)[0] <= 1.0


def test_zz_the_weakest_planted_error():
    if FACTORS:
        k = min(FACTORS, key=FACTORS.get)
        print(f"weakest planted error: {k}, {FACTORS[k]:.3g} times the bound (KAPPA {ref.KAPPA:g}, KAPPA_MANY {ref.KAPPA_MANY:g})")
        assert FACTORS[k] >= 10.0
