"""CPU-only: the float64 statements of tests/map_surfel_ref.py against what they must reduce to (the analytic normal of a linear
log-depth, the neighbour rules, the footprint render for zero normals, the point render for zero radii), the inputs of every device case
of tests/test_gpu_map_surfel.py against the conditions the comparison there relies on (how many pixels the masks exclude in every posed
view; how far another float64 summation order moves an edge of a rectangle), and what every constructed case is there for."""
import functools

import numpy as np
import pytest

import map_render_ref as base
import map_splat_ref as splat
import map_surfel_ref as ref

TAINT_CAP = 0.02          # the project's cap on excluded pixels (tests/test_gpu_segment_depth.py)
EYE = np.eye(4, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    return ref.CASES[name]()


@functools.lru_cache(maxsize=None)
def _tables():
    return [ref.table_from_masks(m, L, K) for m, L, K in ref.normal_scene()]


def _rows_of(tab, n):
    """(table index, row, column) of every point of segment n."""
    lo, hi = int(tab['seg_off'][n]), int(tab['seg_off'][n + 1])
    return [(i, int(tab['pix'][i]) >> 16, int(tab['pix'][i]) & 0xffff) for i in range(lo, hi)]


def _eye_rotation():
    return ref.rotation(EYE)


# ---- the normal -----------------------------------------------------------------------------------------------------------------------
def test_linear_log_depth_pins_the_formula():
    """L = alpha c + beta r + gamma over the full 24 x 32 mask, stored as float32: every difference -- central or one-sided -- is alpha
    (beta) up to the rounding of L, so the normal must be -(-fx alpha, -fy beta, 1 + (c - cx) alpha + (r - cy) beta), normalised.
    The bound.  A stored L is off by at most d = 2^-24 max|L| (half an ulp); a central difference by (d + d) / 2 = d, a one-sided one
    by 2 d.  So |dm| <= 2 d (fx, fy, |c - cx| + |r - cy|) per component, |dm|_2 <= 2 d sqrt(fx^2 + fy^2 + e^2), e the largest
    |c - cx| + |r - cy|.  For n = -m / |m|, |dn|_2 <= 2 |dm|_2 / |m| (the projection of dm, first order, with a factor 2 for the
    rest); m . ray = 1 gives |m| >= 1 / |ray|.  1e-12 covers the float64 arithmetic of both sides."""
    tab = _tables()[0]
    K = tab['K'].astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    al, be = ref.LINEAR['alpha'], ref.LINEAR['beta']
    rows = _rows_of(tab, 0)
    assert len(rows) == 24 * 32
    d = 2.0 ** -24 * float(np.abs(tab['baseL'][:len(rows)]).max())
    e = max(abs(c - cx) + abs(r - cy) for _, r, c in rows)
    ray = max(np.sqrt(((c - cx) / fx) ** 2 + ((r - cy) / fy) ** 2 + 1.0) for _, r, c in rows)
    bound = 2.0 * (2.0 * d * np.sqrt(fx * fx + fy * fy + e * e)) * ray + 1e-12
    worst = 0.0
    for i, r, c in rows:
        m = np.array([-fx * al, -fy * be, 1.0 + (c - cx) * al + (r - cy) * be])
        want = -m / np.linalg.norm(m)
        got = np.array(ref.table_normal(tab, i, _eye_rotation()))
        worst = max(worst, float(np.abs(got - want).max()))
        assert got @ np.array([(c - cx) / fx, (r - cy) / fy, 1.0]) < 0          # it faces the camera
    print(f"\nlinear log-depth: worst component error {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound and bound < 1e-5


def test_neighbour_rules():
    tab = _tables()[0]
    Rm = _eye_rotation()
    K = tab['K'].astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    L = tab['baseL'].astype(np.float64)
    # a one-pixel segment: no neighbour, m = (0, 0, 1)
    (i, r, c), = _rows_of(tab, 1)
    assert ref.neighbours(tab['pix'], i, i + 1, i) == (None, None, None, None)
    assert ref.table_normal(tab, i, Rm) == (0.0, 0.0, -1.0)
    # a one-row segment: Lv = 0, so the y component of m -- and of the camera-frame normal -- is exactly 0
    for i, r, c in _rows_of(tab, 2):
        lo, hi = int(tab['seg_off'][2]), int(tab['seg_off'][3])
        left, right, up, down = ref.neighbours(tab['pix'], lo, hi, i)
        assert up is None and down is None and (left is None) == (c == 4) and (right is None) == (c == 19)
        n = ref.table_normal(tab, i, Rm)
        assert n[1] == 0.0 and n[0] != 0.0
    # a hole at (5, 15): its four neighbours difference one-sidedly, away from it
    seg3 = {(r, c): i for i, r, c in _rows_of(tab, 3)}
    lo, hi = int(tab['seg_off'][3]), int(tab['seg_off'][4])
    assert (5, 15) not in seg3
    for (r, c), missing in (((5, 14), 1), ((5, 16), 0), ((4, 15), 3), ((6, 15), 2)):
        i = seg3[(r, c)]
        nb = ref.neighbours(tab['pix'], lo, hi, i)
        assert nb[missing] is None and all(nb[k] is not None for k in range(4) if k != missing)
        if missing == 1:
            Lu, Lv = L[i] - L[seg3[(5, 13)]], (L[seg3[(6, 14)]] - L[seg3[(4, 14)]]) / 2
        elif missing == 0:
            Lu, Lv = L[seg3[(5, 17)]] - L[i], (L[seg3[(6, 16)]] - L[seg3[(4, 16)]]) / 2
        elif missing == 3:
            Lu, Lv = (L[seg3[(4, 16)]] - L[seg3[(4, 14)]]) / 2, L[i] - L[seg3[(3, 15)]]
        else:
            Lu, Lv = (L[seg3[(6, 16)]] - L[seg3[(6, 14)]]) / 2, L[seg3[(7, 15)]] - L[i]
        m = np.array([-(fx * Lu), -(fy * Lv), (1.0 + (c - cx) * Lu) + (r - cy) * Lv])
        want = -m / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        assert np.array_equal(np.array(ref.table_normal(tab, i, Rm)), want), (r, c)
    # the table neighbour of a row's end is the next row's start: adjacent in the table, not a neighbour
    i = seg3[(3, 18)]
    assert tab['pix'][i + 1] == (4 << 16 | 12) and ref.neighbours(tab['pix'], lo, hi, i)[1] is None


def test_overlapping_segments_never_read_each_other():
    tab = _tables()[0]
    Rm = _eye_rotation()
    rows4, rows5 = _rows_of(tab, 4), _rows_of(tab, 5)
    assert len({(r, c) for _, r, c in rows4} & {(r, c) for _, r, c in rows5}) == 25
    before = [ref.table_normal(tab, i, Rm) for i, _, _ in rows4]
    other = dict(tab, baseL=tab['baseL'].copy())
    lo5, hi5 = int(tab['seg_off'][5]), int(tab['seg_off'][6])
    other['baseL'][lo5:hi5] += np.float32(0.37) * np.arange(hi5 - lo5, dtype=np.float32)
    assert _same_with_nan(before, [ref.table_normal(other, i, Rm) for i, _, _ in rows4])
    assert [ref.table_normal(tab, i, Rm) for i, _, _ in rows5] != [ref.table_normal(other, i, Rm) for i, _, _ in rows5]
    # the last point of segment 4 and the first of segment 5 are adjacent in the table and not neighbours
    last = rows4[-1][0]
    assert ref.neighbours(tab['pix'], int(tab['seg_off'][4]), int(tab['seg_off'][5]), last)[1] is None


def _same_with_nan(a, b):
    return np.array_equal(np.array(a), np.array(b), equal_nan=True)


def test_a_nan_log_depth_zeroes_exactly_the_rows_that_read_it():
    """(14, 8) of segment 4 holds NaN.  Its four neighbours read it in a difference and get (0, 0, 0); (14, 8) itself is interior, its
    central differences read only its neighbours, and it keeps a normal."""
    tab = _tables()[0]
    seg4 = {(r, c): i for i, r, c in _rows_of(tab, 4)}
    assert np.isnan(tab['baseL'][seg4[(14, 8)]]) and np.isnan(tab['baseL']).sum() == 1
    zero = {rc for rc, i in seg4.items() if ref.table_normal(tab, i, _eye_rotation()) == (0.0, 0.0, 0.0)}
    assert zero == {(14, 7), (14, 9), (13, 8), (15, 8)}
    for n in (0, 1, 2, 3, 5):
        assert not any(ref.table_normal(tab, i, _eye_rotation()) == (0.0, 0.0, 0.0) for i, _, _ in _rows_of(tab, n)[::7])


def test_rotation_with_and_without_an_alignment_record():
    rng = np.random.default_rng(5)
    pose = base.pose_of(rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3))
    rec = dict(rot_reanchor=base.pose_of(rng.uniform(-1, 1, 3), [0, 0, 0])[:3, :3].astype(np.float64))
    R = np.array(ref.rotation(pose))
    assert np.array_equal(R, pose[:3, :3].astype(np.float64))
    np.testing.assert_allclose(np.array(ref.rotation(pose, rec)), rec['rot_reanchor'] @ R, rtol=0, atol=4e-16)
    tab = _tables()[1]
    n_cam = np.array(ref.table_normal(tab, 5, _eye_rotation()))
    np.testing.assert_allclose(np.array(ref.table_normal(tab, 5, ref.rotation(pose, rec))), rec['rot_reanchor'] @ R @ n_cam, rtol=0, atol=1e-15)
    assert abs(np.linalg.norm(n_cam) - 1.0) < 1e-15


def test_the_ragged_keyframe_is_ragged():
    masks, _, _ = ref.normal_scene()[1]
    extents = {(int(np.argmax(row)), int(row.sum())) for row in masks[0] if row.any()}
    assert masks.shape == (1, 17, 21) and len(extents) >= 8
    tab = _tables()[1]
    kinds = set()
    for i in range(tab['P']):
        kinds.add(tuple(x is None for x in ref.neighbours(tab['pix'], 0, tab['P'], i)))
    assert len(kinds) >= 8                                         # most combinations of missing neighbours occur
    assert _tables()[0]['seg_off'][1] > 256                        # and segment 0 of A spans more than one workgroup


# ---- the render -------------------------------------------------------------------------------------------------------------------------
def _views(c):
    return list(c['poses']) if 'poses' in c else [None]


@pytest.mark.parametrize("name", ["surfel_posed", "surfel_edges"])
def test_zero_normals_are_the_footprint_render(name):
    c = _case(name)
    zero = np.zeros_like(c['normals'])
    for pose in _views(c):
        want = splat.render(c['points'], c['colours'], c['radii'], c['K'], pose, c['H'], c['W'], c['max_px'])
        for cull in (0, 1):
            got = ref.render(c['points'], c['colours'], zero, c['radii'], c['K'], pose, c['H'], c['W'], c['max_px'], cull)
            for g, w in zip(got, want):
                np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("make", [base.case_posed, lambda: base.case_duplicates()[0]], ids=["posed", "duplicates"])
def test_radius_zero_is_the_point_render_in_mode_1(make):
    c = make()
    zero = np.zeros(len(c['points']), np.float32)
    normals = ref.unit_normals(len(c['points']), 9)
    for pose in c['poses']:
        want = base.render(c['points'], c['colours'], c['K'], pose, c['H'], c['W'], 1)
        got = ref.render(c['points'], c['colours'], normals, zero, c['K'], pose, c['H'], c['W'], max_px=3, cull=0)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


POSED = [(name, k, cull) for name in ref.CASES for k, pose in enumerate(_views(ref.CASES[name]())) if not ref.is_identity(pose)
         for cull in ref.CULLS[name]]


@pytest.mark.parametrize("name,k,cull", POSED, ids=[f"{n}-{k}-cull{q}" for n, k, q in POSED])
def test_masks_exclude_few_pixels(name, k, cull):
    """A condition on the INPUTS, asserted on every posed view of every case the device test compares, under every cull it uses."""
    _, mask = ref.view_of(_case(name), k, cull)
    print(f"\n{name} view {k} cull {cull}: {int((~mask).sum())} of {mask.size} pixels excluded ({100 * (~mask).mean():.3f} %)")
    assert (~mask).mean() <= TAINT_CAP


@pytest.mark.parametrize("name", [n for n in ref.CASES if 'poses' in ref.CASES[n]()])
def test_summation_order_moves_no_edge_by_a_sixteenth_of_delta(name):
    c = _case(name)
    H, W = c['H'], c['W']
    worst = 0.0
    for pose in c['poses']:
        if ref.is_identity(pose):
            continue
        u0, v0, z0, ru0, rv0 = splat.footprints(c['points'], c['radii'], c['K'], pose, c['max_px'], order=0)
        for order in (1, 2):
            u, v, z, ru, rv = splat.footprints(c['points'], c['radii'], c['K'], pose, c['max_px'], order=order)
            with np.errstate(invalid='ignore'):
                near = ((np.minimum(z0, z) > 0) & (np.minimum(u0 + ru0, u + ru) > -1) & (np.maximum(u0 - ru0, u - ru) < W + 1)
                        & (np.minimum(v0 + rv0, v + rv) > -1) & (np.maximum(v0 - rv0, v - rv) < H + 1))
            for e0, e in ((u0 - ru0, u - ru), (u0 + ru0, u + ru), (v0 - rv0, v - rv), (v0 + rv0, v + rv)):
                if near.any():
                    worst = max(worst, float(np.abs(e - e0)[near].max()))
    print(f"\n{name}: another summation order moves an edge by at most {worst:.2e} px (DELTA / 16 = {ref.DELTA / 16:.2e})")
    assert worst <= ref.DELTA / 16 == 6.25e-8


def test_surfel_posed_holds_what_it_is_there_for():
    c = _case("surfel_posed")
    assert len(c['points']) == 3001 and c['max_px'] == 3 and len(c['poses']) == 3
    assert (np.abs(np.linalg.norm(c['normals'], axis=1) - 1) < 1e-6).sum() > 2700 and not c['normals'][::11].any()
    _, _, z1 = base.project(c['points'], c['K'], c['poses'][1])
    assert 0.4 < (z1 < 0).mean() < 0.6                                          # half the cloud behind view 1
    both, front = ref.view_of(c, 0, 0)[0], ref.view_of(c, 0, 1)[0]
    flat = splat.render(c['points'], c['colours'], c['radii'], c['K'], c['poses'][0], c['H'], c['W'], c['max_px'])
    assert (front[2] >= 0).sum() < (both[2] >= 0).sum() <= (flat[2] >= 0).sum()  # culling removes surfels; coverage is the footprints'
    assert (both[1] != flat[1]).mean() > 0.3                                    # and the depths are not the flat ones


def test_surfel_edges_each_point_does_what_it_is_there_for():
    c = _case("surfel_edges")
    R = ref.EDGE_ROWS
    assert len(c['points']) == len(R) == 16
    out = {cull: ref.render(c['points'], c['colours'], c['normals'], c['radii'], c['K'], None, c['H'], c['W'], c['max_px'], cull) for cull in (0, 1)}

    def pixels(name, cull=0):
        return sorted(map(tuple, np.argwhere(out[cull][2] == R[name]).tolist()))

    def block(r0, r1, c0, c1):
        return [(r, col) for r in range(r0, r1 + 1) for col in range(c0, c1 + 1)]

    def depth(r, col, cull=0):
        return float(out[cull][1][r, col])
    made = {(i, r, col): t for i, r, col, t, flat in ref.offers(c['points'], c['normals'], c['radii'], c['K'], None, c['H'], c['W'], c['max_px'], 0)}
    # den = 0 exactly at column 3 (t = -inf before the clamp), front-facing
    K = c['K'].astype(np.float64)
    n0 = c['normals'][R['den_zero']].astype(np.float64)
    assert (n0[0] * ((3 + 0.5) - K[0, 2]) / K[0, 0] + n0[1] * ((4 + 0.5) - K[1, 2]) / K[1, 1]) + n0[2] == 0.0
    assert pixels("den_zero") == pixels("den_zero", 1) == block(3, 5, 3, 5)
    assert depth(4, 3) == 1.75 and depth(4, 4) == 2.0 and depth(4, 5) == 1.75
    # the grazing normal hits both clamps
    assert pixels("grazing") == pixels("grazing", 1) == block(2, 6, 10, 14)
    assert depth(4, 12) == 2.5 and depth(4, 13) == 1.5 and depth(4, 11) == 1.5
    for name, cols in (("zero_normal", (19, 21)), ("nan_normal", (27, 29)), ("inf_normal", (35, 37))):
        assert pixels(name) == pixels(name, 1) == block(3, 5, *cols) and all(depth(r, col) == 2.0 for r, col in pixels(name))
    # s = 0 exactly: t = 0 / den, clamped to z - h with cull = 0; dropped with cull = 1
    p, n = c['points'][R['s_zero']].astype(np.float64), c['normals'][R['s_zero']].astype(np.float64)
    assert (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2] == 0.0
    assert len(pixels("s_zero")) == 9 and pixels("s_zero", 1) == [] and all(depth(r, col) == 1.75 for r, col in pixels("s_zero"))
    assert len(pixels("back")) == 9 and pixels("back", 1) == []
    assert len({depth(r, col) for r, col in pixels("back")}) == 9               # two-sided: a tilted depth per pixel
    for name, col in (("nan_radius", 12), ("negative_radius", 20), ("zero_radius", 28)):
        assert pixels(name) == pixels(name, 1) == [(20, col)] and depth(20, col) == 2.0
    assert pixels("inf_radius") == block(17, 23, 33, 39) and pixels("huge_radius") == block(27, 33, 1, 7)
    for name in ("inf_radius", "huge_radius"):                                  # no clamp in reach: the plane's own depth, never a bound
        seen = {depth(r, col) for r, col in pixels(name)}
        assert len(seen) >= 25 and min(seen) < 1.8 and max(seen) > 2.3
    # z > z_min, and the tilt takes most of the rectangle to t <= z_min: only column 14 is drawn
    i = R['near_plane']
    assert c['points'][i, 2] > ref.Z_MIN and pixels("near_plane") == block(27, 33, 14, 14)
    assert sum(1 for (j, r, col), t in made.items() if j == i) == 49 and sum(1 for (j, r, col), t in made.items() if j == i and t <= ref.Z_MIN) == 42
    assert pixels("reaches") == block(35, 37, 0, 0) and pixels("misses") == [] and pixels("corner") == block(35, 39, 43, 47)
    # no two rectangles overlap: every point's pixels are its whole clipped rectangle
    assert sum(len(pixels(name)) for name in R) == (out[0][2] >= 0).sum()


@pytest.mark.parametrize("footprint", [2.0, 3.0])
def test_oriented_beats_flat_on_the_slanted_surfaces(footprint):
    """The reason for the feature, on the statements: the linear-depth surface the flat render is pinned on (0.025 / 0.035), and a
    plane in space, both half-sampled at 48 x 64."""
    for make in (ref.case_plane, ref.case_true_plane):
        c = make(footprint)
        H, W = c['H'], c['W']
        _, flat, idx_flat = splat.render(c['points'], c['colours'], c['radii'], c['K_mid'], None, H, W, c['max_px'])
        _, tilt, idx = ref.render(c['points'], c['colours'], c['normals'], c['radii'], c['K_mid'], None, H, W, c['max_px'], 1)
        e_flat = np.abs(flat.astype(np.float64) - c['gt'].astype(np.float64)).max()
        e_tilt = np.abs(tilt.astype(np.float64) - c['gt'].astype(np.float64)).max()
        print(f"\n{make.__name__}, footprint {footprint}: worst error flat {e_flat:.7f}, oriented {e_tilt:.3e}")
        assert (idx >= 0).all() and (idx_flat >= 0).all() and e_tilt < e_flat
        assert e_tilt <= (c['curvature'] + 2e-6 if 'curvature' in c else 2e-6)
