"""No GPU: the restatements that tests/test_gpu_normal_integration_pin.py holds the device to (plan_ref, weights_and_rhs, cg_step of
tests/normal_integration_ref.py) against what they restate -- build_system, ref.cg and a literal per-segment loop -- and the
preconditions of that file's scenes (tests/normal_integration_cases.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

import normal_integration_cases as cases
import normal_integration_ref as ref


def _ragged_and_rectangle():
    normals, K, names, masks = cases.setup_scene()
    return normals, K, [("ragged", masks[names.index("ragged")]), ("rectangle", masks[names.index("rect 5x33")]),
                        ("whole image", masks[names.index("whole image")])]


def test_weights_and_rhs_scattered_is_build_system():
    """L assembled from wR, wD and b of weights_and_rhs equal build_system's to 1e-15 relative (of the largest entry)."""
    normals, K, masks = _ragged_and_rectangle()
    for name, mask in masks:
        L, b, index = ref.build_system(normals, K, mask)
        w = ref.weights_and_rhs(normals, K, mask)
        P = b.size
        rows, cols, vals = [], [], []
        for img, (dr, dc) in ((w["wR"], (0, 1)), (w["wD"], (1, 0))):
            r, c = np.nonzero(img)
            ip, iq = index[r, c], index[r + dr, c + dc]
            assert (ip >= 0).all() and (iq >= 0).all(), name
            rows += [ip, iq, ip, iq]
            cols += [ip, iq, iq, ip]
            vals += [img[r, c], img[r, c], -img[r, c], -img[r, c]]
        L2 = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(P, P)).tocsr()
        assert abs(L - L2).max() <= 1e-15 * abs(L).max(), name
        assert np.abs(w["b"][mask] - b).max() <= 1e-15 * np.abs(b).max(), name
        for k in ("wR", "wD", "b"):
            assert not w[k][~mask].any() and (w[k + "_mag"] >= np.abs(w[k])).all() and (w[k + "_bound"] == {"b": ref.B_OPS}.get(k, ref.W_OPS) * ref.U32 * w[k + "_mag"]).all()
        # edges only between mask pixels: the weight of a missing edge is 0
        assert not w["wR"][:, -1].any() and not w["wD"][-1].any()
        assert not (w["wR"][:, :-1][~(mask[:, :-1] & mask[:, 1:])]).any() and not (w["wD"][:-1][~(mask[:-1] & mask[1:])]).any()


def test_a_float32_evaluation_of_the_set_up_meets_its_bounds():
    """The device's expressions restated in float32 numpy (no contraction: every rounding the count allows for happens) stay inside
    count * 2^-24 * magnitude, so the bounds are ones a correct kernel meets."""
    f = np.float32
    normals, K, masks = _ragged_and_rectangle()
    H, W = masks[0][1].shape
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    c, r = np.meshgrid(np.arange(W, dtype=f), np.arange(H, dtype=f))
    x, y = c - cx, r - cy
    nx, ny, nz = normals[..., 0], normals[..., 1], normals[..., 2]
    ax = nx * x + ny * y * (fx / fy) + nz * fx
    ay = nx * x * (fy / fx) + ny * y + nz * fy
    assert ax.dtype == f and ay.dtype == f
    for name, mask in masks:
        w = ref.weights_and_rhs(normals, K, mask)
        assert (np.abs(ax - w["ax"]) <= ref.AX_OPS * ref.U32 * w["ax_mag"]).all() and (np.abs(ay - w["ay"]) <= ref.AX_OPS * ref.U32 * w["ay_mag"]).all()
        right = np.zeros_like(mask)
        right[:, :-1] = mask[:, :-1] & mask[:, 1:]
        down = np.zeros_like(mask)
        down[:-1] = mask[:-1] & mask[1:]
        wR, wD, hR, hD = (np.zeros((H, W), dtype=f) for _ in range(4))
        wR[:, :-1] = f(0.5) * (ax[:, :-1] * ax[:, :-1] + ax[:, 1:] * ax[:, 1:])
        hR[:, :-1] = f(0.5) * (ax[:, :-1] * nx[:, :-1] + ax[:, 1:] * nx[:, 1:])
        wD[:-1] = f(0.5) * (ay[:-1] * ay[:-1] + ay[1:] * ay[1:])
        hD[:-1] = f(0.5) * (ay[:-1] * ny[:-1] + ay[1:] * ny[1:])
        wR, hR, wD, hD = wR * right, hR * right, wD * down, hD * down
        b = hR + hD
        b[:, 1:] -= hR[:, :-1]
        b[1:] -= hD[:-1]
        assert b.dtype == f
        for k, got in (("wR", wR), ("wD", wD), ("b", b)):
            ratio = np.abs(got - w[k])[mask] / np.maximum(w[k + "_bound"][mask], 1e-300)
            assert ratio.max() <= 1, (name, k, ratio.max())


def _padded_system(normals, K, mask):
    plan = ref.plan_ref(mask[None])
    seg = ref.segment(plan, 0)
    w = ref.weights_and_rhs(normals, K, mask)
    return seg, ref.box_image(w["wR"], seg), ref.box_image(w["wD"], seg), ref.box_image(w["b"], seg)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_cg_step_iterated_is_the_float64_cg(which):
    """k steps of cg_step on the padded layout == ref.cg(..., dtype=float64) at cap k (to the rounding of a float64 sum in another
    order), also on a rectangle whose width is the stride (32: rows are kept apart by zero weights alone)."""
    normals, K, names, masks = cases.setup_scene()
    mask = masks[names.index(("ragged", "rect 5x32", "whole image")[which])]
    L, b, index = ref.build_system(normals, K, mask)
    seg, wR, wD, bb = _padded_system(normals, K, mask)
    box = np.zeros((seg["bh"], seg["S"]), dtype=bool)
    box[:, :seg["bw"]] = mask[seg["r0"]:seg["r0"] + seg["bh"], seg["c0"]:seg["c0"] + seg["bw"]]
    u, r, p = np.zeros_like(bb), bb.copy(), bb.copy()
    b_norm = float(np.sqrt((bb * bb).sum()))
    for k in range(1, 9):
        st = ref.cg_step(wR, wD, u, r, p, (seg["bh"], seg["S"]), b_norm=b_norm)
        u, r, p = st.u, st.r, st.p
        want, kk, res = ref.cg(L, b, 0.0, k, dtype=np.float64)
        assert kk == k
        assert np.abs(u[box] - want).max() <= 1e-12 * np.abs(want).max(), k
        assert abs(st.res - res) <= 1e-12 * res
        assert not u[~box].any() and not r[~box].any() and not p[~box].any() and not st.q[~box].any()
        assert (st.q_mag >= np.abs(st.q)).all() and st.pq_mag >= abs(st.pq) and st.n == seg["bh"] * seg["S"]


def _literal_plan(masks, boxes):
    N, H, W = masks.shape
    recs = []
    for n in range(N):
        R0, C0, R1, C1 = (0, 0, H, W) if boxes is None else (max(boxes[n][0], 0), max(boxes[n][1], 0), min(boxes[n][2], H), min(boxes[n][3], W))
        rmin, cmin, rmax, cmax = H, W, -1, -1
        for r in range(R0, R1):
            for c in range(C0, C1):
                if masks[n, r, c]:
                    rmin, cmin, rmax, cmax = min(rmin, r), min(cmin, c), max(rmax, r), max(cmax, c)
        if rmax < 0:
            recs.append(dict(r0=0, c0=0, bh=0, bw=0, S=0, len=0))
            continue
        bh, bw = rmax - rmin + 1, cmax - cmin + 1
        S = -(-bw // 16) * 16
        ln = -(-(bh * S + 2 * S) // 16) * 16
        recs.append(dict(r0=rmin, c0=cmin, bh=bh, bw=bw, S=S, len=ln))
    for n in range(N):
        recs[n]["off"] = 6 * sum(recs[j]["len"] for j in range(n))
    order = [0] * N
    for n in range(N):
        rank = sum(1 for j in range(N) if recs[j]["len"] > recs[n]["len"] or (recs[j]["len"] == recs[n]["len"] and j < n))
        order[rank] = n
    return recs, order, 6 * sum(x["len"] for x in recs)


def _assert_plan_is(plan, recs, order, total):
    for n, rec in enumerate(recs):
        assert ref.segment(plan, n) == rec, (n, ref.segment(plan, n), rec)
    assert list(plan["order"]) == order and plan["total"] == total


def test_plan_ref_against_a_literal_loop():
    """An empty mask, one pixel, two segments of equal len (tie by index), hints tight, loose and clipped by the image."""
    H, W = 12, 40
    m = np.zeros((6, H, W), dtype=bool)
    m[1, 7, 33] = True                                   # one pixel
    m[2, 2:6, 3:20] = True                               # 4 x 17 -> S 32, len 192
    m[3, 1:5, 8:38] = True                               # 4 x 30 -> S 32, len 192: ties with 2
    m[4, 0:12, 0:40] = True
    m[5, 3:9:2, 5:30:3] = True                           # ragged, nothing 4-connected
    tight = np.array([[0, 0, 0, 0], [7, 33, 8, 34], [2, 3, 6, 20], [1, 8, 5, 38], [0, 0, 12, 40], [3, 5, 8, 30]])
    loose = tight + np.array([-1, -2, 3, 1])
    clipped = np.tile(np.array([-4, -40, H + 9, W + 100]), (6, 1))
    for boxes in (None, tight, loose, clipped):
        _assert_plan_is(ref.plan_ref(m, boxes), *_literal_plan(m, boxes))
    p = ref.plan_ref(m)
    assert p["len"][2] == p["len"][3] == 192 and list(p["order"]).index(2) + 1 == list(p["order"]).index(3)
    assert ref.segment(p, 0) == dict(r0=0, c0=0, bh=0, bw=0, off=0, S=0, len=0)
    assert ref.segment(p, 1) == dict(r0=7, c0=33, bh=1, bw=1, off=0, S=16, len=48)
    # a hint narrows the scan: pixels outside it do not count
    narrow = tight.copy()
    narrow[4] = [2, 3, 5, 9]
    assert ref.segment(ref.plan_ref(m, narrow), 4)["bh"] == 3 and ref.segment(ref.plan_ref(m, narrow), 4)["bw"] == 6
    # ... and round-trips through the device's words
    words = np.zeros(ref.plan_words(6), dtype=np.int32)
    words[:2] = np.array([p["total"]], dtype=np.int64).view(np.int32)
    rec = words[ref.PLAN_HEAD:ref.PLAN_HEAD + 48].reshape(6, 8)
    for k, f in ((0, "r0"), (1, "c0"), (2, "bh"), (3, "bw"), (6, "S"), (7, "len")):
        rec[:, k] = p[f]
    rec[:, 4:6] = p["off"].astype(np.int64).view(np.int32).reshape(6, 2)
    words[ref.PLAN_HEAD + 48:ref.PLAN_HEAD + 54] = p["order"]
    back = ref.read_plan(words, 6)
    assert all(np.array_equal(back[k], p[k]) for k in ref.SEG_FIELDS + ("order",)) and back["total"] == p["total"]


def test_the_pin_batches_against_the_literal_loop():
    for masks, boxes in (cases.plan_batch_many(), cases.plan_batch_mixed()):
        plan = ref.plan_ref(masks, boxes)
        _assert_plan_is(plan, *_literal_plan(masks, boxes))
    masks, _ = cases.plan_batch_many()
    plan = ref.plan_ref(masks)
    assert len(masks) == 300 and (plan["bh"] == 0).sum() >= 10 and ((plan["bh"] == 1) & (plan["bw"] == 1)).sum() >= 10
    assert len(np.unique(plan["len"])) <= 8                        # many ties
    _, _, masks = cases.tier_scene()
    plan = ref.plan_ref(masks)
    assert list(plan["bh"]) == list(cases.TIER_BH + cases.TRIP_BH) and (plan["bw"] == 64).all() and (plan["S"] == 64).all()
    assert list(plan["len"][:6]) == [12928, 12992, 19456, 19520, 38912, 38976]
    # both sides of every edge of the LDS budget
    assert 3 * 12928 <= ref.NI_LDS_FLOATS < 3 * 12992 and 2 * 19456 == ref.NI_LDS_FLOATS and 38912 == ref.NI_LDS_FLOATS


def test_segment_floats_is_six_vectors_of_len():
    from super_primitive_amd import _lib
    lib = _lib.load()
    for H, W in ((1, 1), (1, 16), (5, 17), (40, 72), (240, 320), (608, 64), (607, 65)):
        assert lib.sp_normal_integration_segment_floats(H, W) == 6 * ref.len_of(H, W), (H, W)
    for N in (1, 2, 3, 300):
        assert lib.sp_normal_integration_plan_words(N) == ref.plan_words(N)


def test_the_clamp_scene_leaves_plus_minus_15_and_float32_cg_stops_by_itself():
    normals, K, mask = ref.clamp_scene()
    w = ref.weights_and_rhs(normals, K, mask)
    assert np.abs(w["ax"][mask] - 0.4).max() < 1e-4
    L, b, _ = ref.build_system(normals, K, mask)
    u = ref.direct_solution(L, b, ref.component_labels(mask))
    assert u.max() > 15.5 and u.min() < -15.5
    for cap in (19, 50, 100):
        u32, k, res = ref.cg(L, b, 1e-6, cap, dtype=np.float32)
        assert k == 19 and res < 1e-6, (cap, k, res)
    assert np.abs(u32 - u32.mean() - u).max() < 1e-4


def test_the_stop_scene_has_strictly_falling_well_separated_residuals():
    """Precondition of the exact stop-rule test: the float32 host CG's |r_k| / |b| falls strictly over k = 1..12 and no neighbouring pair
    is within 1e-3 relative."""
    normals, K, mask = cases.stop_scene()
    plan = ref.plan_ref(mask[None])
    assert (plan["bh"][0], plan["bw"][0]) == (30, 40)
    L, b, _ = ref.build_system(normals, K, mask)
    res = np.array([ref.cg(L, b, 0.0, k, dtype=np.float32)[2] for k in range(1, 13)])
    assert (res[1:] < res[:-1] * (1 - 1e-3)).all(), res


def test_cg_with_wide_dots_is_the_same_iteration():
    normals, K, mask = cases.stop_scene()
    L, b, _ = ref.build_system(normals, K, mask)
    u64, _, _ = ref.cg(L, b, 0.0, 8, dtype=np.float64)
    a, ka, _ = ref.cg(L, b, 0.0, 8, dtype=np.float32)
    c, kc, _ = ref.cg(L, b, 0.0, 8, dtype=np.float32, dots=np.float64)
    assert ka == kc == 8 and a.dtype == c.dtype == np.float32
    for v in (a, c):
        assert np.abs(v - u64).max() <= 1e-5 * np.abs(u64).max()
