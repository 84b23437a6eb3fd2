"""-m gpu: sp_normal_integration (csrc/sp_normals.hip) stage by stage against the float64 restatements of tests/normal_integration_ref.py,
through the raw C ABI: the plan, the set-up (weights and right-hand side), the first step, one CG iteration from the device's own state, the
early iterates, the stop rule, the clamp and exponential, and the scratch contract.  tests/test_normal_integration_ref_host.py holds the
restatements against what they restate and proves the scenes' preconditions; tests/normal_integration_cases.py builds the scenes.

Every call: ``depth`` and ``info`` pre-filled with a sentinel, TAIL sentinel floats behind ``scratch_floats``, the scratch pre-filled with
0x7f bytes unless a test says otherwise.  After every call (``check_contract``): every element of depth and info written, the tail untouched,
the guards of all six vectors of every solved segment exactly 0, off-mask and padding cells of wR, wD, u exactly 0.

Bounds (counted in normal_integration_ref, not tuned; U = 2^-24):
  weights        W_OPS (14) U magnitude, entry by entry;  b: B_OPS (11) U magnitude
  first step     u_1 = alpha_0 b with one rounding: |u_1 - a b64| <= a bound_b + 1 ulp(u_1), a = (u_1 . b64) / (b64 . b64); a against the
                 float64 b.b / b.Lb within the two dot products' (n + 22) U sum|terms|
  one iteration  from the device's own u, r, p, wR, wD after cap k: q within Q_OPS (5) U sum w |p_c - p_x|; u', r', p' with the device's own
                 step lengths (recovered by projection, with the projection's own rounding bound) within alpha bound_q + the two roundings of
                 the update; alpha, beta and the reported residual within the dot products' bounds
  early iterates in the segments that keep vectors in LDS: 8 x the larger deviation of the two float32 host iterations (float32 / float64 dot
                 products) from the float64 iteration at the same cap, at least 4 ulp of max |u_k| -- measured, not derived: those segments do
                 not expose r, p, q
  exp            EXP_OPS (4) U relative: the hardware exp2 at its documented 1 ulp (2 U), 1 + ln2 lo (1), the product (1); the rounding of
                 x log2 e is carried by the compensated low part, what is left is below 2^-40
The shapes of tier_scene stand on both sides of every size at which a segment keeps another set of vectors in LDS; the labels only choose the
shapes, no assertion depends on which path ran -- except where a test reads r, p, q from the scratch, which only the largest segment
(longer than the LDS budget) keeps there.  The worst ratio to each bound is printed at the end of the file.
"""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import normal_integration_cases as cases
import normal_integration_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

f32 = np.float32
U = ref.U32
SENTINEL = -7.0
TAIL = 64
EXP_OPS = 4
EXP_REL = EXP_OPS * U + 2.0 ** -40
WORST = {}
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"\nworst ratio to each bound over the file ({time.perf_counter() - T0:.1f} s): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def ulp(x):
    """One unit in the last place of the float32 x, as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=f32))).astype(np.float64)


def worst_ratio(got, want, bound, what):
    """max |got - want| / bound; where the bound is 0 (an expression without a non-zero term) the entry must be exactly 0."""
    got, want, bound = (np.asarray(a, dtype=np.float64) for a in (got, want, bound))
    zero = bound == 0
    assert not got[zero].any(), f"{what}: a non-zero entry whose expression has no non-zero term"
    return float((np.abs(got - want)[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def call(normals, K, masks, *, boxes=None, cap, tol, fill="7f", short=0):
    """One sp_normal_integration through the raw ABI.  ``short``: floats withheld from the plan's need.  Returns the outputs, the whole
    scratch (float32, plan words included) and the host plan; the buffers' contract is checked by ``check_contract``."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    masks = np.ascontiguousarray(masks, dtype=bool)
    N, H, W = masks.shape
    o = SimpleNamespace(N=N, H=H, W=W, masks=masks)
    o.plan = ref.plan_ref(masks, boxes)
    o.words = ref.plan_words(N)
    assert lib.sp_normal_integration_plan_words(N) == o.words
    o.n_floats = o.words + o.plan["total"] - short
    byte = {"7f": 0x7f, "zero": 0}.get(fill)
    if byte is None:
        buf = torch.full((o.n_floats + TAIL,), float("nan"), dtype=torch.float32, device="cuda:0")
    else:
        buf = torch.full(((o.n_floats + TAIL) * 4,), byte, dtype=torch.uint8, device="cuda:0").view(torch.float32)
    buf[o.n_floats:] = SENTINEL
    depth = torch.full((N, H, W), SENTINEL, dtype=torch.float32, device="cuda:0")
    info = torch.full((N, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
    n_d, K_d, m_d = T(np.ascontiguousarray(normals, dtype=f32)), T(np.ascontiguousarray(K, dtype=f32)), T(masks.view(np.uint8))
    b_d = None if boxes is None else T(np.ascontiguousarray(boxes, dtype=np.int32))
    rc = lib.sp_normal_integration(_lib.ptr(n_d), _lib.ptr(K_d), _lib.ptr(m_d), _lib.ptr(b_d), N, H, W, int(cap), float(tol), 0,
                                   _lib.ptr(buf), o.n_floats, _lib.ptr(depth), _lib.ptr(info), _lib.stream_ptr())
    _lib.check(rc, "sp_normal_integration")
    torch.cuda.synchronize()
    o.depth, o.info, o.buffer = npy(depth), npy(info), npy(buf)
    o.scratch = o.buffer[:o.n_floats]
    capacity = o.n_floats - o.words
    o.fits = (o.plan["off"] + ref.NI_VECS * o.plan["len"]) <= capacity
    o.solved = (o.plan["bh"] > 0) & o.fits
    check_contract(o)
    return o


def views(o, n):
    """(views, guards, box mask (bh, S)) of segment n."""
    seg = ref.segment(o.plan, n)
    v, g = ref.vector_views(o.scratch, o.words, seg)
    return v, g, ref.box_image(o.masks[n], seg).astype(bool)


def check_contract(o):
    assert bits(o.buffer[o.n_floats:]) == bits(np.full(TAIL, SENTINEL, f32)), "a write behind scratch_floats"
    assert (o.depth != SENTINEL).all() and (o.info != SENTINEL).all(), "an element of depth / info was not written"
    assert np.isfinite(o.depth).all() and np.isfinite(o.info).all()
    for n in np.nonzero(o.solved)[0]:
        v, g, box = views(o, n)
        for name in ref.VECTOR_NAMES:
            assert not g[name][0].any() and not g[name][1].any(), f"segment {n}: guard of {name} is not 0"
        for name in ("wR", "wD", "u"):
            assert not v[name][~box].any(), f"segment {n}: {name} is not 0 off the mask"
        assert not o.depth[n][~o.masks[n]].any(), f"segment {n}: depth off the mask"


def assert_plan_is(got, want):
    for f in ref.SEG_FIELDS + ("order",):
        bad = np.nonzero(np.asarray(got[f]) != np.asarray(want[f]))[0]
        assert bad.size == 0, f"{f}: first difference at {bad[0]}: device {got[f][bad[0]]}, reference {want[f][bad[0]]}"
    assert got["total"] == want["total"]


# ---- (a) the plan, exact ----------------------------------------------------------------------------------------------------------------
PLAN_BATCHES = {"300 small masks": cases.plan_batch_many, "mixed hints": cases.plan_batch_mixed}


@pytest.mark.parametrize("batch", list(PLAN_BATCHES))
def test_plan_entry_is_the_reference_plan(batch):
    """sp_normal_integration_plan: every NiSeg field, order and the int64 total."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    masks, boxes = PLAN_BATCHES[batch]()
    N, H, W = masks.shape
    words = ref.plan_words(N)
    plan = T(np.full(words + TAIL, -77, dtype=np.int32))
    m_d = T(np.ascontiguousarray(masks).view(np.uint8))
    b_d = None if boxes is None else T(np.ascontiguousarray(boxes, dtype=np.int32))
    _lib.check(lib.sp_normal_integration_plan(_lib.ptr(m_d), _lib.ptr(b_d), N, H, W, _lib.ptr(plan), _lib.stream_ptr()), "sp_normal_integration_plan")
    torch.cuda.synchronize()
    got = npy(plan)
    assert (got[words:] == -77).all(), "a write behind the plan"
    assert_plan_is(ref.read_plan(got, N), ref.plan_ref(masks, boxes))


@pytest.mark.parametrize("batch", list(PLAN_BATCHES))
def test_full_call_leaves_the_same_plan_in_the_scratch(batch):
    masks, boxes = PLAN_BATCHES[batch]()
    N, H, W = masks.shape
    if batch == "mixed hints":
        normals, K = cases.setup_scene()[:2]
    else:
        rnd = np.random.default_rng(1).standard_normal((H, W, 3))
        normals, K = (rnd / np.linalg.norm(rnd, axis=-1, keepdims=True)).astype(f32), np.array([[12.5, 0, 7.3], [0, 11.0, 3.6], [0, 0, 1]], f32)
    o = call(normals, K, masks, boxes=boxes, cap=3, tol=0.0)
    assert_plan_is(ref.read_plan(o.scratch[:o.words].view(np.int32), N), o.plan)
    empty = o.plan["bh"] == 0
    assert (o.info[empty] == 0).all() and not o.depth[empty].any()
    assert (o.info[:, 0] >= 0).all() and (o.info[:, 0] <= 3).all()


# ---- (b) the set-up, entry by entry -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def setup_run():
    normals, K, names, masks = cases.setup_scene()
    return call(normals, K, masks, cap=0, tol=1e-3)


@functools.lru_cache(maxsize=None)
def setup_truth():
    normals, K, names, masks = cases.setup_scene()
    return [ref.weights_and_rhs(normals, K, m) for m in masks]


def test_set_up_reports_no_iteration_and_unit_depth():
    o = setup_run()
    for n, w in enumerate(setup_truth()):
        assert tuple(o.info[n]) == ((0.0, 1.0) if np.abs(w["b"]).max() > 0 else (0.0, 0.0)), n
        assert (o.depth[n][o.masks[n]] == 1).all() and not o.depth[n][~o.masks[n]].any(), n


def test_set_up_weights_are_within_their_bounds_on_every_entry():
    o = setup_run()
    names = cases.setup_scene()[2]
    for n, w in enumerate(setup_truth()):
        seg = ref.segment(o.plan, n)
        v, _, box = views(o, n)
        for k in ("wR", "wD"):
            r = worst_ratio(v[k], ref.box_image(w[k], seg), ref.box_image(w[k + "_bound"], seg), f"{names[n]} {k}")
            note("weights", r)
            assert r <= 1, f"{names[n]}: {k} is {r:.3g} of its bound"
        assert not v["wD"][-1].any(), f"{names[n]}: a weight towards row bh"
        if seg["bw"] == seg["S"]:
            assert not v["wR"][:, seg["bw"] - 1].any(), f"{names[n]}: bw == S and the last column has a weight into the next row"
        assert not v["u"].any()
    assert sum(1 for n in range(o.N) if o.plan["bw"][n] == o.plan["S"][n]) == 9


@functools.lru_cache(maxsize=None)
def big_alone(cap):
    """The longest segment of tier_scene (bh = 607, longer than the LDS budget: u, r, p, q all live in the scratch) alone, cg_tol 0."""
    normals, K, masks = cases.tier_scene()
    k = cases.TIER_BH.index(607)
    return call(normals, K, masks[k:k + 1], cap=cap, tol=0.0)


@functools.lru_cache(maxsize=None)
def tier_truth(k):
    normals, K, masks = cases.tier_scene()
    return ref.weights_and_rhs(normals, K, masks[k])


def test_set_up_right_hand_side_in_r_and_p():
    """cap 0 on the segment that keeps r and p in the scratch: both are b, within b's bound entry by entry, and bitwise each other."""
    o = big_alone(0)
    assert tuple(o.info[0]) == (0.0, 1.0)
    w = tier_truth(cases.TIER_BH.index(607))
    seg = ref.segment(o.plan, 0)
    v, _, box = views(o, 0)
    assert bits(v["r"]) == bits(v["p"])
    assert not v["r"][~box].any() and not v["u"].any()
    r = worst_ratio(v["r"], ref.box_image(w["b"], seg), ref.box_image(w["b_bound"], seg), "b")
    note("b (r, p at cap 0)", r)
    assert r <= 1, f"b is {r:.3g} of its bound"
    for k in ("wR", "wD"):
        r = worst_ratio(v[k], ref.box_image(w[k], seg), ref.box_image(w[k + "_bound"], seg), k)
        note("weights", r)
        assert r <= 1


# ---- (c) b and the first step, on both sides of every LDS size ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tier_run(cap):
    normals, K, masks = cases.tier_scene()
    return call(normals, K, masks, cap=cap, tol=0.0)


@pytest.mark.parametrize("k", range(8), ids=[f"bh{bh}" for bh in cases.TIER_BH + cases.TRIP_BH])
def test_first_step_is_alpha_times_b(k):
    o = tier_run(1)
    assert o.info[k, 0] == 1
    w = tier_truth(k)
    seg = ref.segment(o.plan, k)
    v, _, box = views(o, k)
    b64, b_bound = ref.box_image(w["b"], seg), ref.box_image(w["b_bound"], seg)
    u1 = v["u"].astype(np.float64)
    a = float((u1 * b64).sum() / (b64 * b64).sum())
    assert a > 0
    r = worst_ratio(u1, a * b64, a * b_bound + ulp(v["u"]) * (b_bound > 0), "u_1")
    note("u_1 = alpha b", r)
    assert r <= 1, f"u_1 is {r:.3g} of its bound"
    for name in ("wR", "wD"):
        r = worst_ratio(v[name], ref.box_image(w[name], seg), ref.box_image(w[name + "_bound"], seg), name)
        note("weights", r)
        assert r <= 1
    st = ref.cg_step(ref.box_image(w["wR"], seg), ref.box_image(w["wD"], seg), np.zeros_like(b64), b64, b64, (seg["bh"], seg["S"]))
    rel = ref.dot_bound(st.n, st.rr_mag) / st.rr + ref.dot_bound(st.n, st.pq_mag) / st.pq
    r = abs(a - st.alpha) / (st.alpha * rel)
    note("alpha_0", r)
    assert r <= 1, f"alpha_0 {a} against {st.alpha}: {r:.3g} of the dot products' bound"


# ---- (d) one CG iteration from the device's own state ------------------------------------------------------------------------------------
def projection(delta, p, terms_bound):
    """The factor a of delta = a p (+ rounding) by least squares, and the bound of its own error from the entries' rounding bound."""
    pp = float((p * p).sum())
    return float((delta * p).sum()) / pp, float((terms_bound * np.abs(p)).sum()) / pp


def test_runs_are_bitwise_repeatable():
    a = big_alone(5)
    big_alone.cache_clear()
    b = big_alone(5)
    assert a is not b and bits(a.scratch[a.words:]) == bits(b.scratch[b.words:]) and bits(a.depth) == bits(b.depth) and bits(a.info) == bits(b.info)


@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_one_iteration_from_the_device_state(k):
    before, after = big_alone(k), big_alone(k + 1)
    assert before.info[0, 0] == k and after.info[0, 0] == k + 1
    seg = ref.segment(after.plan, 0)
    s0 = {n: a.astype(np.float64) for n, a in views(before, 0)[0].items()}
    s1 = {n: a.astype(np.float64) for n, a in views(after, 0)[0].items()}
    raw1 = views(after, 0)[0]
    assert bits(views(before, 0)[0]["wR"]) == bits(raw1["wR"]) and bits(views(before, 0)[0]["wD"]) == bits(raw1["wD"])
    b_dev = views(big_alone(0), 0)[0]["r"].astype(np.float64)
    bb = float((b_dev * b_dev).sum())
    st = ref.cg_step(s0["wR"], s0["wD"], s0["u"], s0["r"], s0["p"], (seg["bh"], seg["S"]), b_norm=np.sqrt(bb))
    q_bound = ref.Q_OPS * U * st.q_mag
    r = worst_ratio(s1["q"], st.q, q_bound, "q")
    note("q = L p", r)
    assert r <= 1, f"q is {r:.3g} of its bound"

    # the device's own alpha, from u' - u = alpha p: each entry carries the product's and the sum's rounding
    p = s0["p"]
    a, a_err = projection(s1["u"] - s0["u"], p, U * (np.abs(s1["u"] - s0["u"]) + np.abs(s1["u"])) * 1.01)
    r = worst_ratio(s1["u"], s0["u"] + a * p, a_err * np.abs(p) + U * (np.abs(a * p) + np.abs(s1["u"])), "u'")
    note("u' = u + alpha p", r)
    assert r <= 1, f"u' is {r:.3g} of its bound"
    r = worst_ratio(s1["r"], s0["r"] - a * st.q, a * q_bound + a_err * np.abs(st.q) + U * (np.abs(a * st.q) + np.abs(s1["r"])), "r'")
    note("r' = r - alpha q", r)
    assert r <= 1, f"r' is {r:.3g} of its bound"
    # alpha = r.r / p.q: two dot products of the device's own float32 terms and one division
    pq = float((p * s1["q"]).sum())
    alpha = st.rr / pq
    rel = ref.dot_bound(st.n, st.rr) / st.rr + ref.dot_bound(st.n, float((np.abs(p) * np.abs(s1["q"])).sum())) / pq + U
    r = abs(a - alpha) / (alpha * rel + a_err)
    note("alpha", r)
    assert r <= 1, f"alpha {a} against {alpha}: {r:.3g} of its bound"

    # beta from p' - r' = beta p
    be, be_err = projection(s1["p"] - s1["r"], p, U * (np.abs(s1["p"] - s1["r"]) + np.abs(s1["p"])) * 1.01)
    r = worst_ratio(s1["p"], s1["r"] + be * p, be_err * np.abs(p) + U * (np.abs(be * p) + np.abs(s1["p"])), "p'")
    note("p' = r' + beta p", r)
    assert r <= 1, f"p' is {r:.3g} of its bound"
    rr1 = float((s1["r"] * s1["r"]).sum())
    beta = rr1 / st.rr
    r = abs(be - beta) / (beta * (2 * ref.dot_bound(st.n, 1.0) + U) + be_err)
    note("beta", r)
    assert r <= 1, f"beta {be} against {beta}: {r:.3g} of its bound"
    # the reported residual: two square roots of dot products and a division
    want = np.sqrt(rr1 / bb)
    r = abs(float(after.info[0, 1]) - want) / (want * (ref.dot_bound(st.n, 1.0) + 3 * U))
    note("reported |r| / |b|", r)
    assert r <= 1, f"info[1] {after.info[0, 1]} against {want}: {r:.3g} of its bound"


# ---- (e) early iterates where vectors live in LDS ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tier_system(k):
    normals, K, masks = cases.tier_scene()
    L, b, _ = ref.build_system(normals, K, masks[k])
    return L, b


def iterate_tolerance(u64, variants):
    """8 x the larger deviation of the float32 host variants from ``u64``, at least 4 ulp of max |u64|; also the yardstick."""
    yard = max(float(np.abs(v.astype(np.float64) - u64).max()) for v in variants)
    return max(8.0 * yard, 4.0 * float(ulp(np.abs(u64).max()))), yard


@pytest.mark.parametrize("cap", [2, 3, 8])
def test_early_iterates_follow_the_float64_cg(cap):
    o = tier_run(cap)
    ratios = []
    for k, bh in enumerate(cases.TIER_BH):
        assert o.info[k, 0] == cap
        L, b = tier_system(k)
        u64, kk, _ = ref.cg(L, b, 0.0, cap, dtype=np.float64)
        assert kk == cap
        tol, yard = iterate_tolerance(u64, [ref.cg(L, b, 0.0, cap, dtype=f32)[0], ref.cg(L, b, 0.0, cap, dtype=f32, dots=np.float64)[0]])
        v, _, box = views(o, k)
        err = float(np.abs(v["u"][box].astype(np.float64) - u64).max())
        ratios.append(err / tol)
        print(f"cap {cap} bh {bh}: |u_dev - u64| {err:.3g}, float32 host {yard:.3g} ({yard / np.abs(u64).max():.2g} of max |u|), ratio to the tolerance {err / tol:.3g}")
    note(f"u_{cap} in the LDS segments", max(ratios))
    assert max(ratios) <= 1, ratios


# ---- (f) the stop rule, exact -------------------------------------------------------------------------------------------------------------
def test_stop_rule_is_exact():
    """|r_k| <= cg_tol |b| stops, nothing else does: with a tolerance between two of the device's own consecutive residuals the count is
    exactly the first k at or below it and the residual reported is that k's, bitwise.  cg_tol = 1 stops before the first iteration
    (|r_0| = |b|, the same float on both sides: the comparison is <=, not <)."""
    normals, K, mask = cases.stop_scene()
    run = lambda cap, tol: call(normals, K, mask[None], cap=cap, tol=tol).info[0]
    res = [f32(1)]
    for cap in range(1, 13):
        it, r = run(cap, 0.0)
        assert it == cap
        res.append(r)
    skipped = 0
    for k in range(2, 13):
        if not res[k] < res[k - 1]:
            skipped += 1
            continue
        tol = float(np.sqrt(float(res[k]) * float(res[k - 1])))
        if min(abs(float(res[k]) - tol), abs(float(res[k - 1]) - tol)) <= 1e-4 * tol:
            skipped += 1
            continue
        want = min(j for j in range(1, 13) if res[j] <= tol)
        it, r = run(100, tol)
        assert it == want and bits(r) == bits(res[want]), (k, it, want, r, res[want])
    note("stop rule: skipped of 11", skipped)
    assert skipped <= 2, res
    assert tuple(run(100, 1.0)) == (0.0, 1.0)


# ---- (g) clamp and exponential ------------------------------------------------------------------------------------------------------------
def exp_ratio(o, n):
    v, _, box = views(o, n)
    seg = ref.segment(o.plan, n)
    u = v["u"][box]
    d = o.depth[n][seg["r0"]:seg["r0"] + seg["bh"], seg["c0"]:seg["c0"] + seg["bw"]][box[:, :seg["bw"]]].astype(np.float64)
    want = np.exp(np.clip(u.astype(np.float64), -15.0, 15.0))
    return float((np.abs(d - want) / want).max()) / EXP_REL


def test_clamp_and_exponential_on_the_chain():
    normals, K, mask = ref.clamp_scene()
    o = call(normals, K, mask[None], cap=100, tol=1e-6)
    assert 0 < o.info[0, 0] < 100 and o.info[0, 1] <= 1e-6
    L, b, _ = ref.build_system(normals, K, mask)
    lab = ref.component_labels(mask)
    want = ref.direct_solution(L, b, lab)
    centred = [ref.remove_component_means(ref.cg(L, b, 1e-6, 100, dtype=f32, dots=d)[0], lab) for d in (None, np.float64)]
    tol, yard = iterate_tolerance(want, centred)
    v, _, box = views(o, 0)
    u = v["u"][box]
    err = float(np.abs(ref.remove_component_means(u, lab) - want).max())
    print(f"chain: |u_dev - direct| {err:.3g}, float32 host {yard:.3g}, tolerance {tol:.3g}; u {u.min():.2f} .. {u.max():.2f}")
    note("chain u against the direct solution", err / tol)
    assert err <= tol
    d = o.depth[0][mask]
    hi, lo = u > 15, u < -15
    assert hi.sum() >= 3 and lo.sum() >= 3
    assert len(set(d[hi].tolist())) == 1 and len(set(d[lo].tolist())) == 1 and d[lo][0] > 1e-7
    r = exp_ratio(o, 0)
    note("fast_exp", r)
    assert r <= 1, f"exp is {r:.3g} of its bound ({r * EXP_REL / U:.2f} U)"


def test_exponential_on_the_converged_set_up_scenes():
    normals, K, names, masks = cases.setup_scene()
    o = call(normals, K, masks, cap=2000, tol=1e-4)
    assert (o.info[:, 0] < 2000).all() and (o.info[:, 1] <= 1e-4).all()
    for n in range(o.N):
        r = exp_ratio(o, n)
        note("fast_exp", r)
        assert r <= 1, f"{names[n]}: exp is {r:.3g} of its bound ({r * EXP_REL / U:.2f} U)"


# ---- (h) a scratch one float short, and a dirty scratch ------------------------------------------------------------------------------------
def test_scratch_one_float_short():
    normals, K = cases.setup_scene()[:2]
    masks, boxes = cases.plan_batch_mixed()
    full = call(normals, K, masks, boxes=boxes, cap=50, tol=1e-3)
    short = call(normals, K, masks, boxes=boxes, cap=50, tol=1e-3, short=1)
    cut = (full.plan["bh"] > 0) & ~short.fits
    assert full.fits.all() and cut.sum() == 1 and not cut[full.plan["bh"] == 0].any()
    for n in range(full.N):
        if cut[n]:
            assert tuple(short.info[n]) == (-1.0, 0.0) and not short.depth[n].any()
        else:
            assert bits(short.info[n]) == bits(full.info[n]) and bits(short.depth[n]) == bits(full.depth[n]), n


def test_a_dirty_scratch_changes_nothing():
    from super_primitive_amd.frontend.normals import normals_integration as ni
    normals, K = cases.setup_scene()[:2]
    masks, boxes = cases.plan_batch_mixed()
    runs = [call(normals, K, masks, boxes=boxes, cap=50, tol=1e-3, fill=f) for f in ("7f", "nan", "zero")]
    for o in runs[1:]:
        assert bits(o.depth) == bits(runs[0].depth) and bits(o.info) == bits(runs[0].info)
        assert bits(o.scratch[o.words:]) == bits(runs[0].scratch[o.words:]), "the vectors depend on what the scratch held"
    depth, info = ni.integrate_normals(T(normals), T(K), T(masks), boxes=T(boxes), cg_max_iter=50, cg_tol=1e-3, return_info=True)
    assert bits(npy(depth)) == bits(runs[0].depth) and bits(npy(info)) == bits(runs[0].info)
