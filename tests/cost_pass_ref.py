"""Independent reference of ONE launch of the many-pairs cost pass (include/sp_hip.h, sp_pairs_cost / sp_pairs_cost_opt): numpy, written
from the header's contract, no GPU and no autograd.  It restates every span record and every segment record of the launch, column by
column, in float64 -- and says how far a float32 implementation may lie from that, per entry.

Inputs are what the launch reads (``pair_inputs``): the padded tables pix / src4 / kp_L (the set-up in front of the pass is pinned on its
own, tests/test_gpu_point_table.py), the packed target level, intrinsics, sizes, pose, log-depths, affine pair, and the work list.

    point_terms   what ONE table point adds to its span record and to its segment record (every column), in a chosen float type
    attribution   which span record and which segment record every table position feeds
    launch_ref    records (float64), the yardstick n_e, the allowance of the fragile points and the tolerance of the valid counts
    compare       the assertion of tests/test_gpu_cost_pass.py: |got - want| <= kappa n_e + allowance_e, entry by entry

THE YARDSTICK.  ``point_terms`` runs twice: in float64 and in float32 (per-point quantities in that type, the float32 twin forced onto
the float64 run's bilinear cells, validity and signs, so that it differs by ROUNDING only).  For record entry e

    n_e = sum over the record's points of |c64[p, e] - c32[p, e]|

is what float32 arithmetic does to that entry when nothing cancels.  It scales with the entry's own terms, not with the largest entry of a
block: an entry a thousand times smaller than its neighbours is resolved a thousand times finer.  The device may lie KAPPA n_e off (KAPPA,
and the tighter KAPPA_MANY for records of MANY_POINTS valid points and more: measured, see below and tests/test_gpu_cost_pass.py; the
kernel's v_rcp_f32 and exponential are not the twin's division and exp).  The launch's float arguments (irls_eps, zmin) are rounded to
float32 before either run: at a large epsilon most weights ARE 1 / eps.

FRAGILE POINTS.  A float32 position can fall into another bilinear cell, or on the other side of a validity test, than the float64 one;
the slopes (and the mask) jump there.  A point is fragile when ix or iy lies within ``delta`` of an integer, when one of its validity
tests (the 0.99 band, qz > zmin, |qz| > 1e-6, d > 1e-7) lies within that test's delta of flipping while the others hold, or -- mode 0 --
when a channel's |r| lies within delta_r of zero (the sign).  No delta is chosen by hand: each is four times the largest float64 / float32
difference of that quantity over the pair's valid points.  A fragile point adds |c(alternative) - c64| to the allowance of the entries it
feeds (alternative = the neighbouring cell, the flipped mask, the flipped sign) and one to the tolerance of its records' valid counts.
The cases of tests/cost_pass_cases.py keep fragile points below 0.2 % of a pair's valid points; the per-record cases have none.
"""
import numpy as np

f32, f64 = np.float32, np.float64
WAVE_SPANS, DEPTH_TABLE = 0x100, 0x200          # SP_COST_WAVE_SPANS, SP_COST_DEPTH_TABLE
BAND = 0.99
# How far the device may lie from the float64 records, in units of the yardstick.  Both are four times the worst err / n_e measured on
# gfx950 (tests/test_gpu_cost_pass.py lists the figures), rounded up to one digit.  KAPPA holds for EVERY entry; its measurement, 25.25, comes
# from the record of a single-pixel segment, where n_e is ONE sample of the twin's rounding error and happened to be a hundredth of its
# neighbours' (the device's own error there, 1.9e-6 of the entry, is smaller than the 1e-5 the same point's other columns carry).  Over the
# records that sum at least MANY_POINTS valid points -- where n_e is a sum, not a draw -- the worst is 5.13: KAPPA_MANY holds there in addition.
KAPPA = 200.0
KAPPA_MANY, MANY_POINTS = 30.0, 16
DELTA_FACTOR = 4.0                              # a delta = this times the largest float64 / float32 difference of its quantity
IU6 = np.triu_indices(6)

# record layouts (include/sp_hip.h): floats per record, the columns with a meaning, the columns written as zero / never written
SPAN_FLOATS = {0: 16, 1: 32, 2: 48}
SEG_FLOATS = {0: 1, 1: 12, 2: 12}
SPAN_DEFINED = {0: [c for c in range(16) if c != 13], 1: list(range(29)), 2: list(range(46))}
SPAN_ZERO = {0: [13], 1: [29, 30, 31], 2: [46, 47]}                 # the whole span record is written: these as 0
SEG_DEFINED = {0: [0], 1: list(range(10)), 2: list(range(10))}
SEG_UNTOUCHED = {0: [], 1: [10, 11], 2: [10, 11]}                   # never written: they keep what the buffer held
SPAN_COUNT_COL = {0: None, 1: 28, 2: 28}
SEG_COUNT_COL = {0: None, 1: 9, 2: None}
BLOCKS = {                                                          # named groups of columns, for the reports
    0: dict(span={"sum|r|": [0], "g_t": [1, 2, 3], "g_R": list(range(4, 13)), "g_aff": [14, 15]}, seg={"g_kld": [0]}),
    1: dict(span={"sum|r|": [0], "H_pp": list(range(1, 22)), "b_p": list(range(22, 28))},
            seg={"H_pd": list(range(6)), "D": [6], "b_d": [7], "seg sum|r|": [8]}),
    2: dict(span={"sum|r|": [0], "H_pp": list(range(1, 22)), "b_p": list(range(22, 28)), "H_aa": [29, 30, 31], "b_a": [32, 33],
                  "H_ap": list(range(34, 46))},
            seg={"H_pd": list(range(6)), "D": [6], "b_d": [7], "H_ad": [8, 9]}),
}


def pair_inputs(pix, src4, kp_L, kld, trg, K_src, K_trg, H, W, Hl, Wl, P, zmin, pose, aff=None):
    """One pair as the launch sees it.  pix (Ppad,) uint32, src4 (Ppad,4), kp_L / kld (N,), trg (Hl,Wl,3) packed, K_* = (fx, fy, cx, cy),
    pose (4,4) target <- source, aff = (a_s, b_s, a_t, b_t) or None.  Arrays keep the float type they come in (float32 from a device
    batch; float64 tables for the comparison with the finite-difference oracle)."""
    return dict(pix=np.asarray(pix).view(np.uint32).reshape(-1), src4=np.asarray(src4).reshape(-1, 4), kp_L=np.asarray(kp_L), kld=np.asarray(kld),
                trg=np.asarray(trg).reshape(Hl, Wl, 3), K_src=np.asarray(K_src, f64), K_trg=np.asarray(K_trg, f64), H=int(H), W=int(W), Hl=int(Hl),
                Wl=int(Wl), P=int(P), zmin=float(f32(zmin)), pose=np.asarray(pose).reshape(4, 4), aff=None if aff is None else np.asarray(aff).reshape(4))


def point_inputs(xyz, rgb, trg, K_trg, H, W, Hl, Wl, P, zmin, pose, aff=None):
    """One explicit point list as sp_points_cost_grad sees it (tests/single_cost_ref.py): xyz (n,3) source-camera points and rgb (n,3)
    given directly -- no source camera, no pixel words, no shift; a point is source-valid when its depth xyz[:, 2] > 1e-7."""
    xyz, rgb = np.asarray(xyz).reshape(-1, 3), np.asarray(rgb).reshape(-1, 3)
    n = len(xyz)
    pr = pair_inputs(np.zeros(n, np.uint32), np.concatenate((rgb, np.zeros((n, 1), rgb.dtype)), axis=1), np.zeros(0, xyz.dtype), np.zeros(0, xyz.dtype),
                     trg, (1.0, 1.0, 0.0, 0.0), K_trg, H, W, Hl, Wl, P, zmin, pose, aff)
    pr["xyz"] = xyz
    return pr


# ---------------------------------------------------------------------------------------------------------------------------------
# attribution
# ---------------------------------------------------------------------------------------------------------------------------------
def attribution(chunks, spans, n_pairs, ppads, wave_spans, _alter=None):
    """chunks (C,4) {pair, segment, start, count}, spans (S,4) {first chunk, chunks, points, pair}.  Per pair m: dict(seg, span, rec), each
    (ppads[m],) int64 -- the segment, the span record and the segment record of every table position, -1 where no chunk covers it -- and
    ``cover``, how many chunks cover each position.  Segment record: 4 chunk + wave for the points chunk.start + 256 j + 64 wave + lane;
    under wave spans: chunk."""
    chunks, spans = np.asarray(chunks, np.int64).reshape(-1, 4), np.asarray(spans, np.int64).reshape(-1, 4)
    span_of_chunk = np.full(len(chunks), -1, np.int64)
    for s, (q0, n, pts, m) in enumerate(spans):
        assert (span_of_chunk[q0: q0 + n] == -1).all() and (chunks[q0: q0 + n, 0] == m).all() and chunks[q0: q0 + n, 3].sum() == pts
        span_of_chunk[q0: q0 + n] = s
    assert (span_of_chunk >= 0).all(), "a chunk outside every span"
    out = [dict(seg=np.full(ppads[m], -1, np.int64), span=np.full(ppads[m], -1, np.int64), rec=np.full(ppads[m], -1, np.int64),
                cover=np.zeros(ppads[m], np.int64)) for m in range(n_pairs)]
    trip = 64 if wave_spans else 256
    for q, (m, seg, start, count) in enumerate(chunks):
        assert count > 0 and count % trip == 0 and start % trip == 0
        o, sl = out[m], slice(start, start + count)
        i = np.arange(count)
        o["seg"][sl], o["span"][sl] = seg, span_of_chunk[q]
        o["cover"][sl] += 1
        if wave_spans:
            rec = np.full(count, q)
        else:
            wave = (i % 256) // 64
            if _alter == "wave_xor_1":
                wave = wave ^ 1
            rec = 4 * q + wave
        if _alter == "last_point_to_next_chunk":                    # the flush one point late
            last = i >= count - trip
            nxt = q + 1 if q + 1 < len(chunks) and span_of_chunk[q + 1] == span_of_chunk[q] else q
            rec = np.where(last, (nxt if wave_spans else 4 * nxt + (i % 256) // 64), rec)
        o["rec"][sl] = rec
    return out


def n_records(chunks, spans, wave_spans):
    return len(np.asarray(spans).reshape(-1, 4)), len(np.asarray(chunks).reshape(-1, 4)) * (1 if wave_spans else 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# one table point
# ---------------------------------------------------------------------------------------------------------------------------------
def point_terms(pr, seg, mode, depth_table, irls_eps, dtype, force=None, alt=None, _alter=None):
    """What every table position of pair ``pr`` adds to its records, all per-point arithmetic in ``dtype``; ``seg`` (Ppad,) = the segment
    of every position.  Returns dict(span (Ppad, SPAN_FLOATS) float64, seg (Ppad, SEG_FLOATS) float64 -- zero where the mask is clear --,
    and the quantities the fragility analysis looks at: m, ix, iy, xn, yn, qz, d, r, x0, y0, src_ok).
    ``force`` = (x0, y0, m, sign): cells, mask and mode-0 signs taken from another run (the float32 twin).
    ``alt`` = dict(dx (Ppad,), dy (Ppad,), flip (Ppad,) bool, flip_sign (Ppad,3) bool): the alternative of a fragile point.
    ``_alter``: a planted error (tests/test_cost_pass_ref_host.py)."""
    T = dtype
    c = lambda v: np.asarray(v).astype(T)
    pix = pr["pix"]
    n = len(pix)
    segc = np.clip(seg, 0, None)
    col, row, src_ok = c(pix & np.uint32(0xffff)), c((pix >> np.uint32(16)) & np.uint32(0x7fff)), (pix >> np.uint32(31)) == 1
    fx_s, fy_s, cx_s, cy_s = (T(v) for v in pr["K_src"])
    fx_t, fy_t, cx_t, cy_t = (T(v) for v in (pr["K_src"] if _alter == "K_src_projects" else pr["K_trg"]))
    if _alter == "fx_fy_swapped":
        fx_t, fy_t = fy_t, fx_t
    H, W, Hl, Wl = pr["H"], pr["W"], pr["Hl"], pr["Wl"]
    R, t = c(pr["pose"][:3, :3]), c(pr["pose"][:3, 3])
    band = T(1.0 if _alter == "band_1" else BAND)
    with np.errstate(all="ignore"):
        if pr.get("xyz") is not None:                               # the explicit-point front (point_inputs): x, y, d as given
            p = c(pr["xyz"])
            d, src_ok = p[:, 2], np.ones(n, bool)
        else:
            shift = (c(pr["kld"]) - c(pr["kp_L"]))[segc] if len(pr["kld"]) else np.zeros(n, T)
            w4 = c(pr["src4"][:, 3])
            d = w4 * np.exp(shift) if depth_table else np.exp(w4 + shift)
            p = np.stack(((col - cx_s) * d / fx_s, (row - cy_s) * d / fy_s, d), axis=1)
        q = p @ R.T + t
        qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
        guard = np.abs(qz) > T(1e-6)
        zi = np.where(guard, T(1) / np.where(guard, qz, T(1)), T(1e-6))
        u, v = fx_t * qx * zi + cx_t, fy_t * qy * zi + cy_t
        xn, yn = T(2) * u / T(W - 1) - T(1), T(2) * v / T(H - 1) - T(1)
        ix, iy = (xn + T(1)) * T(Wl - 1) / T(2), (yn + T(1)) * T(Hl - 1) / T(2)
        m = src_ok & (d > T(1e-7)) & (np.abs(xn) <= band) & (np.abs(yn) <= band) & (qz > T(pr["zmin"]))
        if force is not None:
            x0, y0, m = force[0], force[1], force[2]
        else:
            x0 = np.clip(np.floor(np.nan_to_num(ix, nan=0.0, posinf=0.0, neginf=0.0)), 0, max(Wl - 2, 0)).astype(np.int64)
            y0 = np.clip(np.floor(np.nan_to_num(iy, nan=0.0, posinf=0.0, neginf=0.0)), 0, max(Hl - 2, 0)).astype(np.int64)
        if alt is not None:
            x0 = np.clip(x0 + alt["dx"], 0, max(Wl - 2, 0))
            y0 = np.clip(y0 + alt["dy"], 0, max(Hl - 2, 0))
            m = m ^ alt["flip"]
        wx, wy = (ix - c(x0))[:, None], (iy - c(y0))[:, None]
        trg = pr["trg"]
        x1, y1 = np.minimum(x0 + 1, Wl - 1), np.minimum(y0 + 1, Hl - 1)
        a, b, cc, dd = c(trg[y0, x0]), c(trg[y0, x1]), c(trg[y1, x0]), c(trg[y1, x1])
        e1, e2 = b - a, cc - a
        e3 = (dd - cc) - e1
        Ix, Iy = e1 + wy * e3, e2 + wx * e3                          # slopes in level pixels, (Ppad,3)
        I = a + wx * e1 + wy * Iy
        gain, bias = T(1), T(0)
        if pr["aff"] is not None:
            aff = c(pr["aff"])
            gain, bias = np.exp(-(aff[2] - aff[0])), aff[3] - aff[1]
        r = c(pr["src4"][:, :3]) - (gain * I + bias)
        absr = np.abs(r)
        ax, ay = T(Wl - 1) / T(W - 1), T(Hl - 1) / T(H - 1)
        if _alter == "ax_1":
            ax = ay = T(1)
        ga, gb = (gain * ax * fx_t) * zi, (gain * ay * fy_t) * zi
        zd = np.where(guard, zi, T(0))                               # d(1/z) = 0 on the guarded branch
        ux, vy = qx * zd, qy * zd
        span = np.zeros((n, SPAN_FLOATS[mode]), f64)
        segr = np.zeros((n, SEG_FLOATS[mode]), f64)
        if mode == 0:
            s = np.sign(r)
            if force is not None:
                s = c(force[3])
            if alt is not None:
                s = np.where(alt["flip_sign"], -s, s)
            gxs, gys = (s * Ix).sum(1), (s * Iy).sum(1)
            ga0, gb0 = -ga * gxs, -gb * gys
            gq = np.stack((ga0, gb0, -(ga0 * qx + gb0 * qy) * zd), axis=1)
            span[:, 0] = absr.sum(1)
            span[:, 1:4] = gq
            span[:, 4:13] = (gq[:, :, None] * p[:, None, :]).reshape(n, 9)
            span[:, 14] = gain * (s * I).sum(1)
            span[:, 15] = -s.sum(1)
            segr[:, 0] = (gq * (q - t)).sum(1)
            sign = s
        else:
            sign = np.sign(r)
            one, zero = np.ones(n, T), np.zeros(n, T)
            e = q if _alter == "e_is_q" else q - t
            A0 = [one, zero, -ux, -ux * qy, qz + ux * qx, -qy, e[:, 0] - ux * e[:, 2]]
            A1 = [zero, one, -vy, -(qz + vy * qy), vy * qx, qx, e[:, 1] - vy * e[:, 2]]
            if _alter == "A03_sign":
                A0[3] = -A0[3]
            if _alter == "A01_halves":
                A0[4], A0[5] = A0[5], A0[4]
            A0, A1 = np.stack(A0, axis=1), np.stack(A1, axis=1)     # (Ppad,7)
            if _alter == "no_gain_in_J":
                ga, gb = (ax * fx_t) * zi, (ay * fy_t) * zi
            J = -((Ix * ga[:, None])[:, :, None] * A0[:, None, :] + (Iy * gb[:, None])[:, :, None] * A1[:, None, :])      # (Ppad,3,7)
            wgt = T(1) / (absr + T(irls_eps) if _alter == "w_sum" else np.maximum(absr, T(irls_eps)))
            Hm = np.einsum("pc,pci,pcj->pij", wgt, J, J)
            bv = np.einsum("pc,pci->pi", wgt * r, J)
            span[:, 0] = absr.sum(1)
            span[:, 1:22] = Hm[:, IU6[0], IU6[1]]
            span[:, 22:28] = bv[:, :6]
            span[:, 28] = 1.0
            segr[:, 0:6] = Hm[:, :6, 6]
            segr[:, 6], segr[:, 7] = Hm[:, 6, 6], bv[:, 6]
            if mode == 1:
                segr[:, 8], segr[:, 9] = absr.sum(1), 1.0
            else:
                ja = gain * I
                jb = T(1.0 if _alter == "jb_plus" else -1.0)
                span[:, 29], span[:, 30], span[:, 31] = (wgt * ja * ja).sum(1), (wgt * ja * jb).sum(1), (wgt * jb * jb).sum(1)
                span[:, 32], span[:, 33] = (wgt * r * ja).sum(1), (wgt * r * jb).sum(1)
                span[:, 34:40] = np.einsum("pc,pci->pi", wgt * ja, J[:, :, :6])
                span[:, 40:46] = np.einsum("pc,pci->pi", wgt * jb, J[:, :, :6])
                segr[:, 8] = np.einsum("pc,pc->p", wgt * ja, J[:, :, 6])
                segr[:, 9] = np.einsum("pc,pc->p", wgt * jb, J[:, :, 6])
        span, segr = np.where(m[:, None], span, 0.0), np.where(m[:, None], segr, 0.0)
    assert np.isfinite(span).all() and np.isfinite(segr).all()
    return dict(span=span, seg=segr, m=m, ix=ix, iy=iy, xn=xn, yn=yn, qz=qz, d=d, r=r, x0=x0, y0=y0, src_ok=src_ok, sign=sign)


# ---------------------------------------------------------------------------------------------------------------------------------
# fragile points
# ---------------------------------------------------------------------------------------------------------------------------------
def fragility(pr, t64, t32, mode):
    """The fragile points of one pair from its float64 run and its UNFORCED float32 run: dict(deltas, cell_x, cell_y (signed: which
    neighbour), validity, sign (Ppad,3), any (Ppad,))."""
    v = t64["m"]
    worst = lambda a, b: DELTA_FACTOR * float(np.abs(a.astype(f64)[v] - b.astype(f64)[v]).max()) if v.any() else 0.0
    dl = dict(pos=max(worst(t64["ix"], t32["ix"]), worst(t64["iy"], t32["iy"])), n=max(worst(t64["xn"], t32["xn"]), worst(t64["yn"], t32["yn"])),
              qz=worst(t64["qz"], t32["qz"]), d=worst(t64["d"], t32["d"]),
              r=DELTA_FACTOR * float(np.abs(t64["r"] - t32["r"].astype(f64))[v].max()) if v.any() else 0.0)
    with np.errstate(all="ignore"):
        fx, fy = t64["ix"] - np.rint(t64["ix"]), t64["iy"] - np.rint(t64["iy"])
        # the neighbouring cell: a position just above an integer may fall below it (cell - 1), one just below may rise (cell + 1)
        cell_x = np.where(v & (np.abs(fx) < dl["pos"]), np.where(fx >= 0, -1, 1), 0)
        cell_y = np.where(v & (np.abs(fy) < dl["pos"]), np.where(fy >= 0, -1, 1), 0)
        xn, yn, qz, d = t64["xn"], t64["yn"], t64["qz"], t64["d"]
        tests = [(np.abs(xn) <= BAND, np.abs(np.abs(xn) - BAND) < dl["n"]), (np.abs(yn) <= BAND, np.abs(np.abs(yn) - BAND) < dl["n"]),
                 (qz > pr["zmin"], np.abs(qz - pr["zmin"]) < dl["qz"]), (np.abs(qz) > 1e-6, np.abs(np.abs(qz) - 1e-6) < dl["qz"]),
                 (d > 1e-7, np.abs(d - 1e-7) < dl["d"])]
        near = np.zeros(len(v), bool)
        rest = t64["src_ok"].copy()
        for ok, close in tests:
            near |= close
            rest &= ok | close
        validity = near & rest
        sign = (v[:, None] & (np.abs(t64["r"]) < dl["r"])) if mode == 0 else np.zeros(t64["r"].shape, bool)
    return dict(deltas=dl, cell_x=cell_x, cell_y=cell_y, validity=validity, sign=sign,
                any=(cell_x != 0) | (cell_y != 0) | validity | sign.any(axis=1))


def _allowance(pr, seg, mode, depth_table, irls_eps, t64, fr):
    """sum over a fragile point's alternatives of |c(alternative) - c64|: (span, seg) arrays, zero on every other point"""
    n = len(seg)
    zero_i, zero_b, zero_s = np.zeros(n, np.int64), np.zeros(n, bool), np.zeros((n, 3), bool)
    a_span, a_seg = np.zeros_like(t64["span"]), np.zeros_like(t64["seg"])
    alts = []
    if (fr["cell_x"] != 0).any():
        alts.append(dict(dx=fr["cell_x"], dy=zero_i, flip=zero_b, flip_sign=zero_s))
    if (fr["cell_y"] != 0).any():
        alts.append(dict(dx=zero_i, dy=fr["cell_y"], flip=zero_b, flip_sign=zero_s))
    if ((fr["cell_x"] != 0) & (fr["cell_y"] != 0)).any():
        alts.append(dict(dx=fr["cell_x"], dy=fr["cell_y"], flip=zero_b, flip_sign=zero_s))
    if fr["validity"].any():
        alts.append(dict(dx=zero_i, dy=zero_i, flip=fr["validity"], flip_sign=zero_s))
    for ch in range(3):
        if fr["sign"][:, ch].any():
            fs = zero_s.copy()
            fs[:, ch] = fr["sign"][:, ch]
            alts.append(dict(dx=zero_i, dy=zero_i, flip=zero_b, flip_sign=fs))
    for alt in alts:
        ta = point_terms(pr, seg, mode, depth_table, irls_eps, f64, alt=alt)
        a_span += np.abs(ta["span"] - t64["span"])
        a_seg += np.abs(ta["seg"] - t64["seg"])
    return a_span, a_seg


# ---------------------------------------------------------------------------------------------------------------------------------
# one launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _scatter(idx, vals, n_rec):
    out = np.zeros((n_rec, vals.shape[1]), f64)
    use = idx >= 0
    np.add.at(out, idx[use], vals[use])
    return out


def launch_ref(pairs, chunks, spans, mode_flags, irls_eps, _alter=None, _alter_attr=None, yardstick=True):
    """The records of sp_pairs_cost(pairs, chunks, spans, mode | flags, irls_eps).  Returns dict(span (S, SPAN_FLOATS), seg (R, SEG_FLOATS)
    float64; n_span / n_seg the yardstick; allow_span / allow_seg the fragile points' allowance; tol_span / tol_seg (S,) / (R,) the
    tolerance of the valid-point columns; twin_span / twin_seg the float32 twin's records; per pair: valid points, fragile points, deltas;
    ``points``: per pair the float64 per-point terms and the attribution)."""
    mode = mode_flags & 0xff
    wave_spans, depth_table = bool(mode_flags & WAVE_SPANS), bool(mode_flags & DEPTH_TABLE)
    irls_eps = float(f32(irls_eps))                 # the launch takes a float: 1 / eps is the weight of most channels at a large epsilon
    assert mode in (0, 1, 2) and not (mode == 2 and (wave_spans or depth_table))
    S, Rn = n_records(chunks, spans, wave_spans)
    att = attribution(chunks, spans, len(pairs), [len(p["pix"]) for p in pairs], wave_spans, _alter=_alter_attr)
    out = dict(mode=mode, span=np.zeros((S, SPAN_FLOATS[mode])), seg=np.zeros((Rn, SEG_FLOATS[mode])), valid=[], fragile=[], deltas=[], points=[])
    for k in ("n_span", "allow_span", "twin_span"):
        out[k] = np.zeros_like(out["span"])
    for k in ("n_seg", "allow_seg", "twin_seg"):
        out[k] = np.zeros_like(out["seg"])
    out["tol_span"], out["tol_seg"] = np.zeros(S), np.zeros(Rn)
    out["cnt_span"], out["cnt_seg"] = np.zeros(S), np.zeros(Rn)            # valid points of every record
    for pr, at in zip(pairs, att):
        t64 = point_terms(pr, at["seg"], mode, depth_table, irls_eps, f64, _alter=_alter)
        covered = at["cover"] > 0
        assert not t64["m"][~covered].any(), "a valid point outside every chunk"
        out["span"] += _scatter(at["span"], t64["span"], S)
        out["seg"] += _scatter(at["rec"], t64["seg"], Rn)
        out["valid"].append(int(t64["m"].sum()))
        out["cnt_span"] += _scatter(at["span"], t64["m"].astype(f64)[:, None], S)[:, 0]
        out["cnt_seg"] += _scatter(at["rec"], t64["m"].astype(f64)[:, None], Rn)[:, 0]
        out["points"].append(dict(t64=t64, att=at))
        if not yardstick:
            continue
        free = point_terms(pr, at["seg"], mode, depth_table, irls_eps, f32)
        t32 = point_terms(pr, at["seg"], mode, depth_table, irls_eps, f32, force=(t64["x0"], t64["y0"], t64["m"], t64["sign"]))
        out["twin_span"] += _scatter(at["span"], t32["span"], S)
        out["twin_seg"] += _scatter(at["rec"], t32["seg"], Rn)
        out["n_span"] += _scatter(at["span"], np.abs(t64["span"] - t32["span"]), S)
        out["n_seg"] += _scatter(at["rec"], np.abs(t64["seg"] - t32["seg"]), Rn)
        fr = fragility(pr, t64, free, mode)
        out["fragile"].append(int(fr["any"].sum()))
        out["deltas"].append(fr["deltas"])
        if fr["any"].any():
            a_span, a_seg = _allowance(pr, at["seg"], mode, depth_table, irls_eps, t64, fr)
            out["allow_span"] += _scatter(at["span"], a_span, S)
            out["allow_seg"] += _scatter(at["rec"], a_seg, Rn)
            flips = fr["validity"].astype(f64)[:, None]
            out["tol_span"] += _scatter(at["span"], flips, S)[:, 0]
            out["tol_seg"] += _scatter(at["rec"], flips, Rn)[:, 0]
    return out


def assemble(ref_or_got, chunks, spans, pairs_N, wave_spans, mode, span=None, seg=None):
    """Per pair the dense system of the records, summed in float64: dict(H (6+N [+2], 6+N [+2]), b, abs_sum, n_valid) -- unknowns
    [xi(6), log-depths (N), and in mode 2 a_t, b_t]; mode 0: dict(abs_sum, g_t (3), g_R (3,3), g_kld (N), g_aff (2))."""
    span = ref_or_got["span"] if span is None else span
    seg = ref_or_got["seg"] if seg is None else seg
    chunks, spans = np.asarray(chunks, np.int64).reshape(-1, 4), np.asarray(spans, np.int64).reshape(-1, 4)
    per = 1 if wave_spans else 4
    out = []
    for m, N in enumerate(pairs_N):
        sp = span[spans[:, 3] == m].sum(0)
        g = np.zeros((N, seg.shape[1]))
        for q in np.nonzero(chunks[:, 0] == m)[0]:
            g[chunks[q, 1]] += seg[per * q: per * q + per].sum(0)
        if mode == 0:
            out.append(dict(abs_sum=sp[0], g_t=sp[1:4], g_R=sp[4:13].reshape(3, 3), g_kld=g[:, 0], g_aff=sp[14:16]))
            continue
        n = 6 + N + (2 if mode == 2 else 0)
        Hm, b = np.zeros((n, n)), np.zeros(n)
        Hpp = np.zeros((6, 6))
        Hpp[IU6] = sp[1:22]
        Hm[:6, :6] = Hpp + np.triu(Hpp, 1).T
        b[:6] = sp[22:28]
        Hm[:6, 6:6 + N] = g[:, :6].T
        Hm[6:6 + N, :6] = g[:, :6]
        Hm[np.arange(6, 6 + N), np.arange(6, 6 + N)] = g[:, 6]
        b[6:6 + N] = g[:, 7]
        if mode == 2:
            ia, ib = 6 + N, 7 + N
            Hm[ia, ia], Hm[ia, ib], Hm[ib, ia], Hm[ib, ib] = sp[29], sp[30], sp[30], sp[31]
            b[ia], b[ib] = sp[32], sp[33]
            Hm[ia, :6], Hm[:6, ia], Hm[ib, :6], Hm[:6, ib] = sp[34:40], sp[34:40], sp[40:46], sp[40:46]
            Hm[ia, 6:6 + N], Hm[6:6 + N, ia], Hm[ib, 6:6 + N], Hm[6:6 + N, ib] = g[:, 8], g[:, 8], g[:, 9], g[:, 9]
        out.append(dict(H=Hm, b=b, abs_sum=sp[0], n_valid=sp[28]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def excess(got_span, got_seg, ref, kappa, min_points=0):
    """The worst  |got - want| / (kappa n_e + allowance_e)  over the defined columns other than the valid counts (inf where the bound is
    zero and the entry is not exact), and where it is: (ratio, description).  ``min_points``: only the records that sum at least that
    many valid points."""
    mode = ref["mode"]
    worst, where = 0.0, ""
    for name, got, want, n, allow, cols, skip, cnt in (
            ("span", got_span, ref["span"], ref["n_span"], ref["allow_span"], SPAN_DEFINED[mode], SPAN_COUNT_COL[mode], ref["cnt_span"]),
            ("segment", got_seg, ref["seg"], ref["n_seg"], ref["allow_seg"], SEG_DEFINED[mode], SEG_COUNT_COL[mode], ref["cnt_seg"])):
        cols = [c for c in cols if c != skip]
        if got.shape[0] == 0 or not (cnt >= min_points).any():
            continue
        err = np.abs(np.asarray(got, f64)[:, cols] - want[:, cols])
        bound = kappa * n[:, cols] + allow[:, cols]
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        ratio = np.where((cnt >= min_points)[:, None], ratio, 0.0)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        if ratio[i] > worst:
            worst, where = float(ratio[i]), f"{name} record {i[0]} column {cols[i[1]]}: got {np.asarray(got)[i[0], cols[i[1]]]!r} want {want[i[0], cols[i[1]]]!r} bound {bound[i]:.3g}"
    return worst, where


def ratios_by_block(got_span, got_seg, ref, min_points=0):
    """{block: worst |got - want| / n_e over the block's entries whose allowance is zero} -- the figure KAPPA is derived from;
    ``min_points`` as in ``excess`` (KAPPA_MANY)"""
    mode = ref["mode"]
    out = {}
    for kind, got, want, n, allow, cnt in (("span", got_span, ref["span"], ref["n_span"], ref["allow_span"], ref["cnt_span"]),
                                           ("seg", got_seg, ref["seg"], ref["n_seg"], ref["allow_seg"], ref["cnt_seg"])):
        for name, cols in BLOCKS[mode][kind].items():
            err = np.abs(np.asarray(got, f64)[:, cols] - want[:, cols])
            use = (allow[:, cols] == 0) & (n[:, cols] > 0) & (cnt >= min_points)[:, None]
            out[name] = float((err[use] / n[:, cols][use]).max()) if use.any() else 0.0
    return out


def compare(got_span, got_seg, ref, kappa, sentinel_bits, what=""):
    """The assertions on one launch's record buffers (float32, (S + extra, SPAN_FLOATS) and (R + extra, SEG_FLOATS), pre-filled with the
    sentinel): every defined column within kappa n_e + allowance_e of the float64 records; valid counts exact up to the records' fragile
    points; the unused span columns zero; the unused segment columns and every record past the work list untouched.  Returns
    ``ratios_by_block``."""
    mode = ref["mode"]
    S, Rn = ref["span"].shape[0], ref["seg"].shape[0]
    got_span, got_seg = np.asarray(got_span, f32), np.asarray(got_seg, f32)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (bits(got_span[S:]) == sentinel_bits).all(), f"{what}: a span record past the work list was written"
    assert (bits(got_seg[Rn:]) == sentinel_bits).all(), f"{what}: a segment record past the work list was written"
    gs, gg = got_span[:S], got_seg[:Rn]
    assert np.isfinite(gs).all(), f"{what}: non-finite span record (or one not written)"
    assert (gs[:, SPAN_ZERO[mode]] == 0).all(), f"{what}: unused span columns are written as zero"
    if SEG_UNTOUCHED[mode]:
        assert (bits(gg[:, SEG_UNTOUCHED[mode]]) == sentinel_bits).all(), f"{what}: unused segment columns are never written"
    assert np.isfinite(gg[:, SEG_DEFINED[mode]]).all(), f"{what}: non-finite segment record (or one not written)"
    worst, where = excess(gs, gg, ref, kappa)
    assert worst <= 1.0, f"{what}: err / (kappa n_e + allowance) = {worst:.3g} at {where}"
    worst, where = excess(gs, gg, ref, KAPPA_MANY, MANY_POINTS)
    assert worst <= 1.0, f"{what}: records of {MANY_POINTS}+ points: err / (KAPPA_MANY n_e + allowance) = {worst:.3g} at {where}"
    for name, got, col, want, tol in (("span", gs, SPAN_COUNT_COL[mode], ref["span"], ref["tol_span"]), ("segment", gg, SEG_COUNT_COL[mode], ref["seg"], ref["tol_seg"])):
        if col is not None and got.shape[0]:
            off = np.abs(got[:, col].astype(f64) - want[:, col])
            assert (off <= tol).all(), f"{what}: valid points of {name} record {int(np.argmax(off - tol))}: off by {off.max():g}"
    return ratios_by_block(gs, gg, ref)
