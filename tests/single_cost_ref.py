"""Independent reference of the single-keyframe cost API (include/sp_hip.h: sp_photo_cost_grad, sp_points_cost_grad, sp_photo_stats): numpy,
written from the header's contract, no GPU and no autograd.  The per-point terms are those of tests/cost_pass_ref.py (``point_terms`` in
mode 0 restates the 16 columns a tile accumulates, with the float32-twin yardstick and the fragile-point allowances); what is added here is
the assembly around them for this path -- tiles, the per-segment column, the scatter into g_pose / g_aff, the 1 / (3 P) scale -- and the
per-point diagnostics.

    photo_cost_grad_ref    residual[B], g_kld[B,N], g_pose[B,4,4], g_aff[B,4] in float64, and per output entry the yardstick n_e, the
                           fragile points' allowance and the number of valid points it sums
    points_cost_grad_ref   the same for an explicit point list: no g_kld, denominator 3 P_total, tiles of 2048 points
    photo_stats_ref        every output array of sp_photo_stats in float64 at a stride, a first-order error bound for every value, and
                           the points whose validity a float32 evaluation may flip
    compare_outputs        |got - want64| <= kappa n_e + allowance_e + ulp32(want64), entry by entry; the entries the contract fixes, exactly
    compare_stats          the exact arrays exactly, every other value within its bound

ATTRIBUTION FOLLOWS THE WORK LIST.  A point belongs to the tile that covers it; its depth is shifted by the kld / kp_L of the segment the
TILE names, and g_kld[n] sums column 13 of the tiles seg_tile_off[n] .. seg_tile_off[n + 1]: a work list that disagrees with the table shows.

THE BOUND OF A SUMMED ENTRY.  n_e = (sum over the entry's points of |c64 - c32 twin|) / (3 P) is what float32 arithmetic does to the entry
when nothing cancels (tests/cost_pass_ref.py); the device may lie KAPPA n_e off (KAPPA_MANY for entries that sum at least MANY_POINTS valid
points), plus what the fragile points may add, plus one float32 ulp of the value: the device sums the tile records in float64 and casts
once.  Nothing is scaled by the largest entry of a block.  KAPPA / KAPPA_MANY are four times the worst (err - ulp32) / n_e measured on
gfx950 over the cases of tests/single_cost_cases.py, rounded up to one digit (tests/test_gpu_single_cost.py lists the figures).

THE BOUND OF A PER-POINT VALUE (``photo_stats_ref``) is derived from the operation chain of the kernel, u = 2^-24 per correctly rounded
operation, propagated to first order through the float64 values and slopes:

    a   = w + (kld - kp_L)              2 roundings                         e_a  = u (|kld - kp_L| + |a|)
    d   = exp(a)                        EXP_ULPS                            e_d  = d (e_a + EXP_ULPS 2u)
    x   = ((col - cx) d) (1 / fx)       4 roundings (1 / fx is one)         e_x  = |x| (e_d / d + 4u)            (y alike; z = d)
    q_i = fma(R0, x, fma(R1, y, R2 z)) + t_i                                e_q  = sum_j |R_ij| e_pj + 3u sum_j |R_ij p_j| + u |q_i|
    1/z = rcp(q_z)                      RCP_ULPS                            rel  = e_qz / |q_z| + RCP_ULPS 2u    (exact on the guarded branch)
    u   = (q_x fx) (1/z) + cx           3 roundings                         e_u  = |fx / z| e_qx + |q_x fx / z| (rel + 2u) + u |u|
    xn  = 2 u (1 / (W - 1)) - 1         3 roundings                         e_xn = 2 e_u / (W - 1) + 2u |xn + 1| + u |xn|
    ix  = (xn + 1) (Wl - 1) / 2         2 roundings                         e_ix = (Wl - 1) / 2 (e_xn + u |xn + 1|) + u |ix|
    I   = bilinear(ix, iy)              3 fma levels over the taps          e_I  = |I_x| e_ix + |I_y| e_iy + 6u max|tap|
    I'  = fma(gain, I, bias)            gain = exp(.): EXP_ULPS             e_I' = gain e_I + |I| e_gain + u |bias| + u |I'|
    raw = (s - I') mask                 2 roundings                         e_r  = e_I' + 2u |s - I'|

The kernel's exponential and reciprocal have no stated error bound in this tree: EXP_ULPS and RCP_ULPS are four times the worst distance
from the float64 value measured on gfx950 over the cases (tests/test_gpu_single_cost.py), in units of 2u.  Bilinear interpolation is
continuous across cell borders (zero padding outside the image included), so a float32 position that falls into the neighbouring cell
changes a VALUE by no more than the slopes say; only a validity test that flips changes it by a jump.  Such points -- within ``delta`` of
the 0.99 band or of zmin, delta four times the largest float64 / float32 difference of that quantity as in tests/cost_pass_ref.py -- are
flagged ``fragile``: their trg_valid may differ, their raw may be 0 or the residual.
"""
import numpy as np

import cost_pass_ref as cpr

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
POINT_TILE = 2048                               # SP_POINT_TILE: points per tile of sp_points_cost_grad
# Measured on gfx950 (tests/test_gpu_single_cost.py lists the figures): four times the worst (err - ulp32) / n_e, rounded up to one digit.
# KAPPA holds for EVERY entry; its measurement, 6554.5, is g_kld of ONE single-point segment (case n300), where n_e is one draw of the
# float32 twin's rounding error and came out at 1.7e-10 of the entry -- 4000 times below the median of the single-point entries, 7.4e-7 --
# while the device's error there, 1.2e-6 of the entry, is 1.6 times that median (the entry's three terms cancel to a twentieth).  The next
# largest figure is 19.5.  Over the entries that sum at least MANY_POINTS valid points -- where n_e is a sum, not a draw -- the worst is
# 1.51: KAPPA_MANY holds there in addition, and is what pins the kernels; it is four times tighter than the many-pairs pass's 30.
KAPPA = 30000.0
KAPPA_MANY, MANY_POINTS = 7.0, 16
# The kernel's expf lies at most 0.745 ulp from exp of its own float32 argument over the cases: four times that, rounded up to one digit.
EXP_ULPS = 3.0
# Its reciprocal (v_rcp_f32) cannot be observed alone -- no output holds 1 / z or the position; its share is four times the 1 ulp the ISA
# manual states, and trg_rgb / raw, the only outputs it reaches, come out at 0.32 of their bound at most.
RCP_ULPS = 4.0


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def K4(K):
    """(fx, fy, cx, cy) of a 3x3 / 9-float / 4-float intrinsics"""
    K = np.asarray(K, f64).reshape(-1)
    return K if K.size == 4 else np.array([K[0], K[4], K[2], K[5]])


# ---------------------------------------------------------------------------------------------------------------------------------
# the summed outputs
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_index(tiles, P):
    """(P,) the tile that covers every point (-1: none) and the segment that tile names"""
    tiles = np.asarray(tiles, np.int64).reshape(-1, 4)
    tix, seg = np.full(P, -1, np.int64), np.full(P, -1, np.int64)
    for t, (_, n, start, count) in enumerate(tiles):
        assert count >= 0 and 0 <= start and start + count <= P and (tix[start: start + count] == -1).all(), "tiles overlap or leave the table"
        tix[start: start + count], seg[start: start + count] = t, n
    return tix, seg


def _columns(t):
    """the 16 columns of one tile record per point: the span columns of mode 0 with the segment column as column 13"""
    c = t["span"].copy()
    c[:, 13] = t["seg"][:, 0]
    return c


def _assemble(cols, tix, n_tiles, seg_tile_off, N, scale, has_aff, signed=True, _alter=None):
    """k_finalise_single on per-point columns: (residual, g_kld (N), g_pose (4,4), g_aff (4)).  ``signed`` False: for the yardstick,
    the allowance and the counts (nothing is negated)."""
    part = np.zeros((n_tiles, 16))
    use = tix >= 0
    np.add.at(part, tix[use], cols[use])
    tot = (part[:64] if _alter == "tiles_past_64_ignored" else part).sum(0)
    g_pose = np.zeros((4, 4))
    g_pose[:3, 3], g_pose[:3, :3] = tot[1:4], tot[4:13].reshape(3, 3)
    neg = -1.0 if signed else 1.0
    g_aff = np.array([neg * tot[14], neg * tot[15], tot[14], tot[15]]) if has_aff else np.zeros(4)
    g_kld = np.zeros(N)
    if N:
        sto = np.asarray(seg_tile_off, np.int64)
        owner = np.repeat(np.arange(N), np.diff(sto[:N + 1]))        # the segment every tile is credited to
        if _alter == "column_13_to_next_segment":                   # the last tile of the first segment with two tiles or more
            n = int(np.nonzero((np.diff(sto[:N + 1]) >= 2) & (np.arange(N) < N - 1))[0][0])
            owner[sto[n + 1] - 1] = n + 1
        np.add.at(g_kld, owner, part[: len(owner), 13])
    return tot[0] * scale, g_kld * scale, g_pose * scale, g_aff * scale


def _cost_ref(prs, tix, seg, n_tiles, seg_tile_off, N, denom, has_aff, yardstick, drop=None, _alter=None):
    B = len(prs)
    scale = 1.0 / (3.0 * denom)
    names = ("residual", "g_kld", "g_pose", "g_aff")
    out = {k: [] for k in names}
    out.update({f"{p}_{k}": [] for p in ("n", "allow", "cnt", "twin") for k in names})
    out.update(valid=[], fragile=[], deltas=[], points=[], has_aff=has_aff, N=N, B=B)
    for pr in prs:
        t64 = cpr.point_terms(pr, seg, 0, False, 0.0, f64)
        c64 = _columns(t64)
        keep = (tix >= 0) if drop is None else (tix >= 0) & ~drop
        tx = np.where(keep, tix, -1)
        asm = lambda cols, scale=scale, signed=True, alter=_alter: _assemble(cols, tx, n_tiles, seg_tile_off, N, scale, has_aff, signed, alter)
        for k, v in zip(names, asm(c64)):
            out[k].append(v)
        m = (t64["m"] & keep).astype(f64)
        for k, v in zip(names, asm(np.repeat(m[:, None], 16, axis=1), 1.0, False, None)):
            out[f"cnt_{k}"].append(v)
        out["valid"].append(int(m.sum()))
        out["points"].append(t64)
        if not yardstick:
            continue
        free = cpr.point_terms(pr, seg, 0, False, 0.0, f32)
        t32 = cpr.point_terms(pr, seg, 0, False, 0.0, f32, force=(t64["x0"], t64["y0"], t64["m"], t64["sign"]))
        c32 = _columns(t32)
        for k, v in zip(names, asm(c32)):
            out[f"twin_{k}"].append(v)
        for k, v in zip(names, asm(np.abs(c64 - c32), signed=False)):
            out[f"n_{k}"].append(v)
        fr = cpr.fragility(pr, t64, free, 0)
        out["fragile"].append(int((fr["any"] & keep).sum()))
        out["deltas"].append(fr["deltas"])
        a = np.zeros_like(c64)
        if fr["any"].any():
            a_span, a_seg = cpr._allowance(pr, seg, 0, False, 0.0, t64, fr)
            a = a_span.copy()
            a[:, 13] = a_seg[:, 0]
        for k, v in zip(names, asm(a, signed=False)):
            out[f"allow_{k}"].append(v)
    for k in list(out):
        if isinstance(out[k], list) and out[k] and isinstance(out[k][0], (np.ndarray, float, f64)):
            out[k] = np.stack([np.asarray(v, f64) for v in out[k]])
    return out


def photo_cost_grad_ref(tables, tiles, seg_tile_off, N, P, B, poses, K_trg, trg, aff, zmin, yardstick=True, drop=None, _alter=None):
    """sp_photo_cost_grad.  tables: dict(pix (P,), src4 (P,4), kp_L (N,), kld (N,), K_src, H, W) -- what was uploaded; tiles (T,4) {pair,
    segment, start, count}; poses (B,4,4); K_trg (B,3,3); trg (B,Hl,Wl,3) packed; aff None or (aff_src (2,), aff_trg (B,2)).  Returns a
    dict: residual (B,), g_kld (B,N), g_pose (B,4,4), g_aff (B,4) float64; n_* the yardstick, allow_* the fragile points' allowance, cnt_* the
    valid points every entry sums (all in the outputs' shapes); twin_* the float32 twin's outputs; valid / fragile points per target.
    ``drop`` (P,) bool: points left out (planted errors)."""
    tiles = np.asarray(tiles, np.int64).reshape(-1, 4)
    tix, seg = tile_index(tiles, P)
    trg = np.asarray(trg)
    poses, K_trg = np.asarray(poses).reshape(B, 4, 4), np.asarray(K_trg).reshape(B, -1)
    Hl, Wl = trg.shape[1:3]
    prs = []
    for b in range(B):
        a4 = None if aff is None else np.concatenate((np.asarray(aff[0]).reshape(2), np.asarray(aff[1]).reshape(B, 2)[b]))
        prs.append(cpr.pair_inputs(tables["pix"], tables["src4"], tables["kp_L"], tables["kld"], trg[b], K4(tables["K_src"]), K4(K_trg[b]), tables["H"], tables["W"],
                                   Hl, Wl, P, zmin, poses[b], a4))
    return _cost_ref(prs, tix, seg, len(tiles), seg_tile_off, N, P, aff is not None, yardstick, drop, _alter)


def point_tiles(n_points):
    n_t = (n_points + POINT_TILE - 1) // POINT_TILE
    return np.array([[0, 0, t * POINT_TILE, min(POINT_TILE, n_points - t * POINT_TILE)] for t in range(n_t)], np.int64).reshape(-1, 4)


def points_cost_grad_ref(xyz, rgb, n_points, P_total, H, W, B, poses, K_trg, trg, aff, zmin, yardstick=True, drop=None, _alter=None):
    """sp_points_cost_grad over xyz (n,3), rgb (n,3): as photo_cost_grad_ref, without g_kld (shape (B,0)); the denominator is 3 P_total."""
    xyz, rgb, trg = np.asarray(xyz).reshape(-1, 3)[:n_points], np.asarray(rgb).reshape(-1, 3)[:n_points], np.asarray(trg)
    poses, K_trg = np.asarray(poses).reshape(B, 4, 4), np.asarray(K_trg).reshape(B, -1)
    Hl, Wl = trg.shape[1:3]
    tiles = point_tiles(n_points)
    tix, _ = tile_index(tiles, n_points)
    prs = []
    for b in range(B):
        a4 = None if aff is None else np.concatenate((np.asarray(aff[0]).reshape(2), np.asarray(aff[1]).reshape(B, 2)[b]))
        prs.append(cpr.point_inputs(xyz, rgb, trg[b], K4(K_trg[b]), H, W, Hl, Wl, P_total, zmin, poses[b], a4))
    return _cost_ref(prs, tix, np.zeros(n_points, np.int64), len(tiles), None, 0, P_total, aff is not None, yardstick, drop, _alter)


def _entries(got, ref):
    """(block, got, want, n_e, allowance, valid points) per block of output entries, each flattened alike"""
    g = {k: np.asarray(got[k], f64) for k in ("residual", "g_pose", "g_aff")}
    sel = {"residual": ("residual", np.s_[:]), "g_t": ("g_pose", np.s_[:, :3, 3]), "g_R": ("g_pose", np.s_[:, :3, :3]), "g_aff": ("g_aff", np.s_[:, 2:])}
    if ref["N"]:
        g["g_kld"] = np.asarray(got["g_kld"], f64).reshape(ref["B"], ref["N"])
        sel["g_kld"] = ("g_kld", np.s_[:])
    for block, (k, sl) in sel.items():
        yield block, g[k][sl].ravel(), ref[k][sl].ravel(), ref[f"n_{k}"][sl].ravel(), ref[f"allow_{k}"][sl].ravel(), ref[f"cnt_{k}"][sl].ravel()


def exact_violations(got, ref):
    """what the contract fixes: a list of descriptions, empty when all hold"""
    bad = []
    g_pose, g_aff = np.asarray(got["g_pose"], f32).reshape(-1, 4, 4), np.asarray(got["g_aff"], f32).reshape(-1, 4)
    bits = lambda a: np.ascontiguousarray(a, f32).view(np.uint32)
    if not (bits(g_pose[:, 3]) == 0).all():
        bad.append("g_pose row 3 is not +0")
    if not ref["has_aff"] and not (bits(g_aff) == 0).all():
        bad.append("g_aff is not 0 without an affine pair")
    if not (bits(g_aff[:, 0]) == bits(-g_aff[:, 2])).all() and ref["has_aff"]:
        bad.append("g_aff[b,0] != -g_aff[b,2] bitwise")
    if not (bits(g_aff[:, 1]) == bits(-g_aff[:, 3])).all() and ref["has_aff"]:
        bad.append("g_aff[b,1] != -g_aff[b,3] bitwise")
    if ref["N"]:
        g_kld = np.asarray(got["g_kld"], f32).reshape(ref["B"], ref["N"])
        if g_kld[ref["cnt_g_kld"] == 0].any():
            bad.append("g_kld of a segment without tiles (or without a valid point) is not 0")
    for k in ("residual", "g_pose", "g_aff") + (("g_kld",) if ref["N"] else ()):
        if not np.isfinite(np.asarray(got[k], f64)).all():
            bad.append(f"{k}: non-finite (or not written)")
    return bad


def excess(got, ref, kappa=None, kappa_many=None, exact=True):
    """The worst |got - want| / (kappa n_e + allowance_e + ulp32(want)) over all entries -- for the entries that sum at least MANY_POINTS
    valid points also with kappa_many -- and where: (ratio, description); inf when something the contract fixes is violated (``exact`` False:
    the bounds alone)."""
    kappa = KAPPA if kappa is None else kappa
    kappa_many = KAPPA_MANY if kappa_many is None else kappa_many
    bad = exact_violations(got, ref) if exact else []
    if bad:
        return np.inf, "; ".join(bad)
    worst, where = 0.0, ""
    for block, g, want, n, allow, cnt in _entries(got, ref):
        err = np.abs(g - want)
        for kap, use, tag in ((kappa, np.ones(len(g), bool), "KAPPA"), (kappa_many, cnt >= MANY_POINTS, "KAPPA_MANY")):
            if not use.any():
                continue
            ratio = np.where(use, err / (kap * n + allow + ulp32(want)), 0.0)
            i = int(np.argmax(ratio))
            if ratio[i] > worst:
                worst, where = float(ratio[i]), f"{block}[{i}] ({tag}, {int(cnt[i])} valid points): got {g[i]!r} want {want[i]!r} n_e {n[i]:.3g} allowance {allow[i]:.3g}"
    return worst, where


def bound_of(ref, key, kappa=None, kappa_many=None):
    """the bound of every entry of ref[key], in its shape: both assertions of ``excess`` at once (the smaller kappa where MANY_POINTS are summed)"""
    kappa = KAPPA if kappa is None else kappa
    kappa_many = KAPPA_MANY if kappa_many is None else kappa_many
    kap = np.where(ref[f"cnt_{key}"] >= MANY_POINTS, min(kappa, kappa_many), kappa)
    return kap * ref[f"n_{key}"] + ref[f"allow_{key}"] + ulp32(ref[key])


def ratios_by_block(got, ref, min_points=0):
    """{block: worst max(|got - want| - ulp32(want), 0) / n_e over the block's entries whose allowance is zero} -- the figure KAPPA is derived from"""
    out = {}
    for block, g, want, n, allow, cnt in _entries(got, ref):
        use = (allow == 0) & (n > 0) & (cnt >= min_points)
        out[block] = float((np.maximum(np.abs(g - want) - ulp32(want), 0.0)[use] / n[use]).max()) if use.any() else 0.0
    return out


def compare_outputs(got, ref, kappa=None, kappa_many=None, what=""):
    """The assertion of tests/test_gpu_single_cost.py on one call's outputs (dict residual, g_kld, g_pose, g_aff).  Returns ratios_by_block."""
    worst, where = excess(got, ref, kappa, kappa_many)
    assert worst <= 1.0, f"{what}: err / (kappa n_e + allowance + ulp32) = {worst:.3g} at {where}"
    return ratios_by_block(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-point diagnostics
# ---------------------------------------------------------------------------------------------------------------------------------
def _bilinear_zero_padded(img, ix, iy):
    """value and slopes (per level pixel) of the zero-padded bilinear interpolation of img (Hl,Wl,3) at (ix, iy): (Q,3) each, and max |tap|"""
    Hl, Wl = img.shape[:2]
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    wx, wy = (ix - x0)[:, None], (iy - y0)[:, None]

    def tap(y, x):
        inside = (x >= 0) & (x < Wl) & (y >= 0) & (y < Hl)
        return np.where(inside[:, None], img[np.clip(y, 0, Hl - 1), np.clip(x, 0, Wl - 1)].astype(f64), 0.0)
    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top, bot = a + wx * (b - a), c + wx * (d - c)
    Ix = (1 - wy) * (b - a) + wy * (d - c)
    Iy = bot - top
    return top + wy * Iy, Ix, Iy, np.max(np.abs(np.stack((a, b, c, d))), axis=(0, 2))


def photo_stats_ref(tables, seg_off, N, P, B, poses, K_trg, trg, aff, zmin, stride=1, exp_ulps=None, rcp_ulps=None, _alter=None):
    """sp_photo_stats at ``stride``: Q = ceil(P / stride) rows.  Returns float64 src_pts (Q,3), src_rgb (3,Q), trg_pts (B,Q,3), trg_rgb (B,3,Q),
    raw (B,3,Q); src_valid (Q), trg_valid (B,Q) bool; seg_ids (Q) int64; e_<name>: the error bound of every value (module docstring);
    ``fragile`` (B,Q): a float32 evaluation may flip the point's target validity; ``checkable`` (B,Q): the position bound is below a
    hundredth of a level pixel, so the first-order bound of trg_rgb / raw holds (every valid point must be); ``arg32`` (Q,): the
    exponential's float32 argument, for the measurement of EXP_ULPS.  trg None: the source outputs only."""
    exp_ulps = EXP_ULPS if exp_ulps is None else exp_ulps
    rcp_ulps = RCP_ULPS if rcp_ulps is None else rcp_ulps
    rows = np.arange(0, P, stride, dtype=np.int64)
    if _alter == "rows_at_stride_plus_1":
        rows = np.minimum(rows + 1, P - 1)
    Q = len(rows)
    assert Q == (P + stride - 1) // stride
    so = np.asarray(seg_off, np.int64)[:N]
    owner = np.searchsorted(so, rows, side="right") - 1             # the last n with seg_off[n] <= i
    if _alter == "owner_without_the_skip_over_empty_segments":      # ... the first of the segments that share the offset
        owner = np.searchsorted(so, so[owner], side="left")
    assert (owner >= 0).all()
    pix = np.asarray(tables["pix"]).view(np.uint32).reshape(-1)[rows]
    src4 = np.asarray(tables["src4"]).reshape(-1, 4)[rows]
    col, row, bit = (pix & np.uint32(0xffff)).astype(f64), ((pix >> np.uint32(16)) & np.uint32(0x7fff)).astype(f64), (pix >> np.uint32(31)) == 1
    kld, kp_L = np.asarray(tables["kld"]), np.asarray(tables["kp_L"])
    fx, fy, cx, cy = K4(tables["K_src"])
    H, W = tables["H"], tables["W"]
    with np.errstate(all="ignore"):
        arg32 = src4[:, 3] + (kld - kp_L)[owner]                    # in the tables' own type
        sh = (kld.astype(f64) - kp_L.astype(f64))[owner]
        a = src4[:, 3].astype(f64) + sh
        d = np.exp(a)
        e_d = d * (U * (np.abs(sh) + np.abs(a)) + exp_ulps * 2 * U)
        x, y = (col - cx) * d / fx, (row - cy) * d / fy
        e_x, e_y = np.abs(x) * (e_d / d + 4 * U), np.abs(y) * (e_d / d + 4 * U)
        p, e_p = np.stack((x, y, d), axis=1), np.stack((e_x, e_y, e_d), axis=1)
        src_valid = bit & (d > 1e-7)
        out = dict(src_pts=p, e_src_pts=e_p, src_rgb=src4[:, :3].astype(f64).T.copy(), src_valid=src_valid, seg_ids=owner.astype(np.int64), arg32=arg32, rows=rows,
                   d=d, Q=Q, B=B)
        if trg is None:
            return out
        trg = np.asarray(trg)
        Hl, Wl = trg.shape[1:3]
        poses, K_trg = np.asarray(poses, f64).reshape(B, 4, 4), np.asarray(K_trg).reshape(B, -1)
        zmin = float(f32(zmin))
        for k in ("trg_pts", "e_trg_pts", "trg_rgb", "e_trg_rgb", "raw", "e_raw", "trg_valid", "fragile", "checkable", "e_pos"):
            out[k] = []
        # the deltas of the validity tests: four times the float64 / float32 difference over the valid points of the WHOLE table
        seg_all = np.searchsorted(so, np.arange(P), side="right") - 1
        for b in range(B):
            R, t = poses[b, :3, :3], poses[b, :3, 3]
            fxt, fyt, cxt, cyt = K4(K_trg[b])
            gain, bias, e_gain, e_bias = 1.0, 0.0, 0.0, 0.0
            a4 = None
            if aff is not None:
                a_s, a_t = np.asarray(aff[0], f64).reshape(2), np.asarray(aff[1], f64).reshape(B, 2)[b]
                a4 = np.concatenate((np.asarray(aff[0]).reshape(2), np.asarray(aff[1]).reshape(B, 2)[b]))
                gain, bias = np.exp(-(a_t[0] - a_s[0])), a_t[1] - a_s[1]
                e_gain, e_bias = gain * (U * abs(a_t[0] - a_s[0]) + exp_ulps * 2 * U), U * abs(bias)
            q = p @ R.T + t
            e_q = e_p @ np.abs(R).T + 3 * U * (np.abs(p) @ np.abs(R).T) + U * np.abs(q)
            qx, qy, qz = q.T
            guard = np.abs(qz) > 1e-6
            zi = np.where(guard, 1.0 / np.where(guard, qz, 1.0), 1e-6)
            rel = np.where(guard, e_q[:, 2] / np.abs(qz) + rcp_ulps * 2 * U, 0.0)
            u_, v_ = fxt * qx * zi + cxt, fyt * qy * zi + cyt
            e_u = np.abs(fxt * zi) * e_q[:, 0] + np.abs(fxt * qx * zi) * (rel + 2 * U) + U * np.abs(u_)
            e_v = np.abs(fyt * zi) * e_q[:, 1] + np.abs(fyt * qy * zi) * (rel + 2 * U) + U * np.abs(v_)
            xn, yn = 2 * u_ / (W - 1) - 1, 2 * v_ / (H - 1) - 1
            e_xn = 2 * e_u / (W - 1) + 2 * U * np.abs(xn + 1) + U * np.abs(xn)
            e_yn = 2 * e_v / (H - 1) + 2 * U * np.abs(yn + 1) + U * np.abs(yn)
            sx, sy = 0.5 * (Wl - 1), 0.5 * (Hl - 1)
            ix, iy = (xn + 1) * sx, (yn + 1) * sy
            e_ix, e_iy = sx * (e_xn + U * np.abs(xn + 1)) + U * np.abs(ix), sy * (e_yn + U * np.abs(yn + 1)) + U * np.abs(iy)
            trg_valid = (np.abs(xn) <= cpr.BAND) & (np.abs(yn) <= cpr.BAND) & (qz > zmin)
            finite = np.isfinite(ix) & np.isfinite(iy) & (np.abs(ix) < 1e6) & (np.abs(iy) < 1e6)
            checkable = finite & (e_ix < 0.01) & (e_iy < 0.01)
            I, Ix, Iy, tapmax = _bilinear_zero_padded(trg[b], np.where(finite, ix, 0.0), np.where(finite, iy, 0.0))
            e_I = np.abs(Ix) * e_ix[:, None] + np.abs(Iy) * e_iy[:, None] + 6 * U * tapmax[:, None]
            it = gain * I + bias
            e_it = gain * e_I + np.abs(I) * e_gain + e_bias + U * np.abs(it)
            s = src4[:, :3].astype(f64)
            mask = (trg_valid & src_valid)[:, None]
            raw = (s - it) * mask
            e_raw = (e_it + 2 * U * np.abs(s - it)) * mask
            # fragile: a validity test within its delta of flipping (deltas as tests/cost_pass_ref.py takes them, over the whole table)
            pr = cpr.pair_inputs(tables["pix"], tables["src4"], kp_L, kld, trg[b], (fx, fy, cx, cy), (fxt, fyt, cxt, cyt), H, W, Hl, Wl, P, zmin, poses[b], a4)
            t64, t32 = cpr.point_terms(pr, seg_all, 0, False, 0.0, f64), cpr.point_terms(pr, seg_all, 0, False, 0.0, f32)
            dl = cpr.fragility(pr, t64, t32, 0)["deltas"]
            near = (np.abs(np.abs(xn) - cpr.BAND) < dl["n"]) | (np.abs(np.abs(yn) - cpr.BAND) < dl["n"]) | (np.abs(qz - zmin) < dl["qz"])
            for k, v in (("trg_pts", q), ("e_trg_pts", e_q), ("trg_rgb", it.T), ("e_trg_rgb", e_it.T), ("raw", raw.T), ("e_raw", e_raw.T), ("trg_valid", trg_valid),
                         ("fragile", near), ("checkable", checkable), ("e_pos", np.maximum(e_ix, e_iy))):
                out[k].append(v)
        for k in ("trg_pts", "e_trg_pts", "trg_rgb", "e_trg_rgb", "raw", "e_raw", "trg_valid", "fragile", "checkable", "e_pos"):
            out[k] = np.stack(out[k])
    return out


STATS_EXACT = ("seg_ids", "src_rgb", "src_valid")
STATS_BOUNDED = ("src_pts", "trg_pts", "trg_rgb", "raw")


def stats_excess(got, ref):
    """The worst |got - want| / bound over the per-point values present in ``got`` (inf: an exact array differs, a trg_valid differs at a
    point that is not fragile, or a value is not finite), where, and {name: worst ratio}."""
    worst, where, per = 0.0, "", {}

    def note(r, w, name):
        nonlocal worst, where
        per[name] = max(per.get(name, 0.0), r)
        if r > worst:
            worst, where = r, w
    for k in STATS_EXACT:
        if got.get(k) is not None:
            want = ref[k].astype(f32) if k == "src_rgb" else ref[k]
            g = np.asarray(got[k]).reshape(want.shape)
            same = g.astype(bool) == want if k == "src_valid" else g == want
            note(0.0 if same.all() else np.inf, f"{k}: {int((~same).sum())} entries differ", k)
    if "trg_valid" not in ref:
        return worst, where, per
    B, Q = ref["B"], ref["Q"]
    frag = ref["fragile"]
    if got.get("trg_valid") is not None:
        differ = (np.asarray(got["trg_valid"]).reshape(B, Q).astype(bool) != ref["trg_valid"]) & ~frag
        note(np.inf if differ.any() else 0.0, f"trg_valid: {int(differ.sum())} points differ that are not fragile", "trg_valid")
    for k in STATS_BOUNDED:
        if got.get(k) is None:
            continue
        want, bound = ref[k], ref[f"e_{k}"]
        g = np.asarray(got[k], f64).reshape(want.shape)
        err = np.abs(g - want)
        if k == "src_pts":
            use = np.ones(want.shape, bool)
        elif k == "trg_pts":
            use = np.ones(want.shape, bool)
        else:
            use = np.broadcast_to(ref["checkable"][:, None, :], want.shape)
            if k == "raw":                                           # a fragile point's raw is 0 or the residual: either passes
                full = (ref["src_rgb"][None] - ref["trg_rgb"]) * ref["src_valid"][None, None, :]
                err = np.where(frag[:, None, :], np.minimum(np.abs(g - full), np.abs(g)), err)
                bound = np.where(frag[:, None, :], ref["e_trg_rgb"] + 2 * U * np.abs(full), bound)
        if not np.isfinite(g[use]).all():
            note(np.inf, f"{k}: non-finite (or not written)", k)
            continue
        with np.errstate(all="ignore"):
            ratio = np.where(use & (err > 0), err / bound, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        note(float(ratio[i]), f"{k}{list(map(int, i))}: got {g[i]!r} want {want[i]!r} bound {bound[i]:.3g}", k)
    return worst, where, per


def compare_stats(got, ref, what=""):
    worst, where, per = stats_excess(got, ref)
    assert worst <= 1.0, f"{what}: |got - want| / bound = {worst:.3g} at {where}"
    return per
