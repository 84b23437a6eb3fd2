"""CPU: the cost-pass reference (tests/cost_pass_ref.py) against what it shares no code with -- the finite-difference Gauss-Newton oracle
and the photometric oracle's autograd -- and what tests/test_gpu_cost_pass.py relies on about its cases (tests/cost_pass_cases.py): every
real point in exactly one span record and one segment record, fragile points at most 0.2 % of a pair's valid points and none in the
per-record cases, and a comparison that catches fifteen planted errors with a factor ten to spare at the KAPPA the GPU test uses.

The tables here come from the point-table reference (tests/point_table_ref.py); the GPU test reads the device's own."""
import functools

import numpy as np
import pytest
import torch

import cost_pass_cases as cases
import cost_pass_ref as ref
from oracle import gn_oracle, photometric_oracle as orc

f64 = np.float64


@functools.lru_cache(maxsize=None)
def host_ref(name, variant, level, eps, table_dtype=np.float32):
    pairs, chunks, spans, mf = cases.host_launch(name, variant, level, table_dtype=table_dtype)
    return ref.launch_ref(pairs, chunks, spans, mf, eps, yardstick=table_dtype is np.float32), pairs, chunks, spans, mf


def _oracle_frames(sc):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    src = orc.OracleFrame(t(sc["image"]), t(sc["K"]), t(sc["logdepth"]), t(sc["keypoints"]), torch.from_numpy(sc["masks"]))
    return src, orc.OracleFrame(t(sc["trg_image"]), t(sc["K_trg"]))


def _close(got, want, what):
    """within 1e-6 of each entry's own magnitude plus 1e-9 of the block's largest"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    tol = 1e-6 * np.abs(want) + 1e-9 * np.abs(want).max()
    bad = np.abs(got - want) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} entries, worst |err| / tol = {(np.abs(got - want) / np.maximum(tol, 1e-300)).max():.3g}"


@pytest.mark.parametrize("name", ["base", "affine"])
@pytest.mark.parametrize("mode", [1, 2])
def test_float64_reference_equals_the_finite_difference_oracle_entry_by_entry(name, mode):
    variant = str(mode)
    r, pairs, chunks, spans, mf = host_ref(name, variant, 0, 1e-3, np.float64)
    got = ref.assemble(r, chunks, spans, [len(p["kld"]) for p in pairs], False, mode)
    for m, sc in enumerate(cases.case(name)["scenes"]):
        src, trg = _oracle_frames(sc)
        aff = cases.scene_aff(sc, variant)
        affine = None if aff is None else (torch.from_numpy(aff[:2].astype(f64)), torch.from_numpy(aff[2:].astype(f64)))
        want = gn_oracle.normal_equations(src, trg, torch.from_numpy(sc["kld"]), torch.from_numpy(sc["pose"]), eps=float(np.float32(1e-3)), affine=affine, with_affine=mode == 2)
        H, b, N = want["H"].numpy(), want["b"].numpy(), sc["N"]
        g = got[m]
        assert g["n_valid"] == want["n_valid"] == r["valid"][m]
        np.testing.assert_allclose(g["abs_sum"] / (3.0 * pairs[m]["P"]), want["cost"], rtol=1e-12)
        blocks = [(np.s_[:6, :6], "H_pp"), (np.s_[:6, 6:6 + N], "H_pd"), (np.s_[6:6 + N, 6:6 + N], "H_dd")]
        if mode == 2:
            blocks += [(np.s_[6 + N:, 6 + N:], "H_aa"), (np.s_[6 + N:, :6], "H_ap"), (np.s_[6 + N:, 6:6 + N], "H_ad")]
        for sl, what in blocks:
            _close(g["H"][sl], H[sl], f"{name} pair {m} mode {mode} {what}")
        for sl, what in [(np.s_[:6], "b_p"), (np.s_[6:6 + N], "b_d")] + ([(np.s_[6 + N:], "b_a")] if mode == 2 else []):
            _close(g["b"][sl], b[sl], f"{name} pair {m} mode {mode} {what}")
    if name == "base":
        assert r["valid"] == [2774, 2317]


@pytest.mark.parametrize("name", ["base", "affine", "intrinsics"])
def test_float64_gradient_sums_equal_the_oracle_s_autograd(name):
    r, pairs, chunks, spans, mf = host_ref(name, "0", 0, 1e-3, np.float64)
    got = ref.assemble(r, chunks, spans, [len(p["kld"]) for p in pairs], False, 0)
    for m, sc in enumerate(cases.case(name)["scenes"]):
        src, trg = _oracle_frames(sc)
        kld = torch.from_numpy(sc["kld"]).double().requires_grad_(True)
        pose = torch.from_numpy(sc["pose"]).double().requires_grad_(True)
        affine = None
        if sc["aff"] is not None:
            affine = (torch.from_numpy(sc["aff"][:2].astype(f64)), torch.from_numpy(sc["aff"][2:].astype(f64)).requires_grad_(True))
        res = orc.photometric_cost(src, trg, kld, pose, affine=affine)["residual"]
        res.sum().backward()
        scale = 1.0 / (3.0 * pairs[m]["P"])
        g = got[m]
        np.testing.assert_allclose(g["abs_sum"] * scale, float(res), rtol=1e-12)
        _close(g["g_t"] * scale, pose.grad[:3, 3].numpy(), f"{name} pair {m} g_t")
        _close(g["g_R"] * scale, pose.grad[:3, :3].numpy(), f"{name} pair {m} g_R")
        _close(g["g_kld"] * scale, kld.grad.numpy(), f"{name} pair {m} g_kld")
        if affine is not None:
            _close(g["g_aff"] * scale, affine[1].grad.numpy(), f"{name} pair {m} g_aff")


@pytest.mark.parametrize("name,variant,level,eps", cases.GN_RUNS + cases.GRAD_RUNS)
def test_every_real_point_lands_in_one_span_record_and_one_segment_record(name, variant, level, eps):
    r, pairs, chunks, spans, mf = host_ref(name, variant, level, eps)
    mode, wave = mf & 0xff, bool(mf & ref.WAVE_SPANS)
    S, Rn = ref.n_records(chunks, spans, wave)
    for m, (pr, pt) in enumerate(zip(pairs, r["points"])):
        at, real = pt["att"], pr["pix"] != 0
        assert (at["cover"][real] == 1).all() and (at["cover"] <= 1).all()
        assert (at["span"][real] >= 0).all() and (at["span"][real] < S).all() and (at["rec"][real] >= 0).all() and (at["rec"][real] < Rn).all()
        assert (chunks[at["rec"][real] // (1 if wave else 4), 1] == at["seg"][real]).all()        # a record belongs to the point's segment
        # the pair's records sum to the sums over its points
        mine = np.asarray(spans)[:, 3] == m
        np.testing.assert_allclose(r["span"][mine].sum(0), pt["t64"]["span"].sum(0), rtol=1e-12, atol=1e-300)
        assert r["span"][mine][:, 0].sum() > 0
    # padding adds zero: every column of a record is the sum over real, valid points only
    assert all(not pt["t64"]["m"][pr["pix"] == 0].any() for pr, pt in zip(pairs, r["points"]))


@pytest.mark.parametrize("name,variant,level,eps", cases.GN_RUNS + cases.GRAD_RUNS)
def test_fragile_points_are_rare_and_absent_from_the_per_record_cases(name, variant, level, eps):
    r = host_ref(name, variant, level, eps)[0]
    for valid, fragile in zip(r["valid"], r["fragile"]):
        assert fragile <= 0.002 * valid, (name, variant, fragile, valid)
        assert fragile == 0 or name not in cases.NO_FRAGILE
    if name in cases.NO_FRAGILE:
        assert not r["allow_span"].any() and not r["allow_seg"].any() and not r["tol_span"].any() and not r["tol_seg"].any()
    assert (r["n_span"][:, ref.SPAN_DEFINED[r["mode"]]] >= 0).all()


def test_validity_case_has_every_kind_of_invisible_point_and_a_segment_of_exact_zeros():
    r, pairs, chunks, spans, mf = host_ref("validity", "1|DT|W64+RD", 0, 1e-3)
    t, pr = r["points"][0]["t64"], pairs[0]
    real = pr["pix"] != 0
    with np.errstate(all="ignore"):
        front = real & t["src_ok"] & (t["qz"] > pr["zmin"])
        assert (real & t["src_ok"] & (t["qz"] < 0)).sum() > 100                                    # behind the camera
        for beyond in (t["xn"] > 0.99, t["xn"] < -0.99, t["yn"] > 0.99, t["yn"] < -0.99):        # each side of the band
            assert (front & beyond).sum() > 20
    col, row = pr["pix"] & 0xffff, (pr["pix"] >> 16) & 0x7fff
    for edge in (col == 0, col == 63, row == 0, row == 47):                                       # the outermost source pixels
        assert (real & edge).any() and not t["src_ok"][real & edge].any()
    assert 500 < r["valid"][0] < 2000
    seg0 = np.asarray(chunks)[:, 1] == 0
    assert seg0.any() and not r["seg"][seg0].any() and not r["n_seg"][seg0].any() and r["seg"][~seg0][:, 9].all()
    assert not r["span"][np.asarray(spans)[:, 0] == 0].any()                                      # ... and so is the span of its chunks


def test_records_cases_exercise_every_flush():
    for name, variant in (("records", "1"), ("records", "1|W64"), ("records_rd", "1|DT|W64+RD")):
        r, pairs, chunks, spans, mf = host_ref(name, variant, 0, 1e-3)
        counts = cases.case(name)["scenes"][0]["masks"].reshape(20, -1).sum(1)
        assert (counts == 1).sum() >= 2 and (counts == 0).sum() >= 2 and counts.max() > cases.case(name)["tile_points"]
        per_seg = np.bincount(chunks[:, 1], minlength=20)
        assert per_seg.max() >= 2 and (per_seg[counts == 0] == 0).all()                           # a segment over two chunks; empty ones have none
        assert spans[:, 1].max() >= 8 and len(spans) >= 2                                         # about a dozen chunks in one span


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors: each must exceed KAPPA n_e + allowance_e by at least ten times in some entry
# ---------------------------------------------------------------------------------------------------------------------------------
def _hpp15_negated(span, seg):
    span[:, 11] = -span[:, 11]                  # upper triangle, row-major: (1,5) is column 1 + 6 + 4


def _doubles_kept(span, seg):
    span[:, 16], span[:, 21] = span[:, 13], span[:, 20]        # (3,2) next to (3,3) and (5,4) next to (5,5) of H_pp: the wrong half written back


def _seg_cost_to_neighbour(span, seg):
    seg[:, 8:10] = np.roll(seg[:, 8:10], 1, axis=0)


MUTATIONS = [
    # (planted error, where it acts, case, variant, level, eps)
    ("A03_sign", "formula", "base", "1", 0, 1e-3),
    ("A01_halves", "formula", "base", "1", 0, 1e-3),
    (_hpp15_negated, "output", "base", "1", 0, 1e-3),
    (_doubles_kept, "output", "base", "1|DT|W64", 0, 1e-3),
    ("fx_fy_swapped", "formula", "intrinsics", "1|DT|W64+RD", 0, 1e-3),
    ("K_src_projects", "formula", "intrinsics", "1|DT|W64+RD", 0, 1e-3),
    ("ax_1", "formula", "base", "1", 1, 1e-3),
    ("e_is_q", "formula", "base", "1", 0, 1e-3),
    ("e_is_q", "formula", "rotation", "1|DT|W64+RD", 0, 1e-3),
    ("no_gain_in_J", "formula", "affine", "1|DT|W64+RD", 0, 1e-3),
    ("jb_plus", "formula", "base", "2", 0, 1e-3),
    ("jb_plus", "formula", "affine", "2", 0, 1e-3),
    ("last_point_to_next_chunk", "attribution", "records", "1", 0, 1e-3),
    ("last_point_to_next_chunk", "attribution", "records", "1|W64", 0, 1e-3),
    ("last_point_to_next_chunk", "attribution", "records_rd", "1|DT|W64+RD", 0, 1e-3),
    ("wave_xor_1", "attribution", "records", "1", 0, 1e-3),
    ("wave_xor_1", "attribution", "records", "2", 0, 1e-3),
    (_seg_cost_to_neighbour, "output", "records", "1", 0, 1e-3),
    (_seg_cost_to_neighbour, "output", "records_rd", "1|DT|W64+RD", 0, 1e-3),
    ("w_sum", "formula", "eps", "1|DT|W64+RD", 0, 1e-3),
    ("w_sum", "formula", "eps", "2", 0, 5e-2),
    ("band_1", "formula", "validity", "1|DT|W64+RD", 0, 1e-3),
    ("band_1", "formula", "validity", "2", 0, 1e-3),
]


def mutation_excess(mut, where, name, variant, level, eps, kappa):
    r, pairs, chunks, spans, mf = host_ref(name, variant, level, eps)
    if where == "output":
        span, seg = r["span"].copy(), r["seg"].copy()
        mut(span, seg)
    else:
        kw = dict(_alter=mut) if where == "formula" else dict(_alter_attr=mut)
        wrong = ref.launch_ref(pairs, chunks, spans, mf, eps, yardstick=False, **kw)
        span, seg = wrong["span"], wrong["seg"]
    return ref.excess(span, seg, r, kappa)


@pytest.mark.parametrize("mut,where,name,variant,level,eps", MUTATIONS, ids=[f"{m if isinstance(m, str) else m.__name__}-{n}-{v}" for m, _, n, v, _, _ in MUTATIONS])
def test_planted_errors_exceed_the_bound_ten_times(mut, where, name, variant, level, eps):
    worst, at = mutation_excess(mut, where, name, variant, level, eps, ref.KAPPA)
    print(f"{mut if isinstance(mut, str) else mut.__name__} on {name} {variant}: err / (KAPPA n_e + allowance) = {worst:.3g} at {at}")
    assert worst >= 10.0, at


def test_the_float32_twin_passes_the_comparison_it_defines():
    """the twin's records lie within its own yardstick (at most 1 n_e by construction) -- and the float64 records within zero"""
    for name, variant, level, eps in cases.GN_RUNS + cases.GRAD_RUNS:
        r = host_ref(name, variant, level, eps)[0]
        assert ref.excess(r["twin_span"], r["twin_seg"], r, 1.0)[0] <= 1.0 + 1e-6              # (float64 summation order)
        assert ref.excess(r["span"], r["seg"], r, 1.0)[0] == 0.0
