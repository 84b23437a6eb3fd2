"""-m gpu: map normals and oriented surfels (csrc/sp_surfel.hip: sp_map_normals; csrc/sp_views.hip: sp_render_surfels; through ``tool/viz.py`` and
``odometery/results.py``) against the float64 statements of tests/map_surfel_ref.py.

What is compared how.  Normals: every component within 1 float32 ulp of the statement rounded once (the statement reads the device's own
table, which is asserted to be the table of the masks first); observed: 0 components differ at all.  Surfels: with the identity pose the
kernel's float64 arithmetic is the statement's, operation for operation: image, depth and index are compared BITWISE on every pixel.  For
posed views the pixels of the masks (tests/map_surfel_ref.py; at most 2 % of a view, asserted on every posed view and cull by
tests/test_map_surfel_ref_host.py) are left out and the rest is compared bitwise too.  Zero normals against the footprint render and zero
radii against the point render: bitwise on every pixel, no reference involved.

Excluded pixels per posed view (of the statement's inputs; the device agreed on every other pixel): surfel_posed 0, 0, 0 under both
culls; surfel_collide view 1: 4 of 768; surfel_views17: 0 in all 17 under both culls."""
import functools

import numpy as np
import pytest
import torch

import map_render_ref as base
import map_splat_ref as splat
import map_surfel_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)[None]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    """Two device tensors bit for bit (the scene holds a NaN log-depth, so some points are NaN)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    """The two keyframes of ref.normal_scene() on the device, their log-depths, and the tables the DEVICE built, read back."""
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.segment_table import table_of
    rng = np.random.default_rng(402)
    kfs, klds, tables = [], [], []
    for masks, L, K in ref.normal_scene():
        N, H, W = masks.shape
        image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
        keypoints = np.zeros((N, 2), np.float32)
        for n in range(N):
            rc = np.argwhere(masks[n])
            r, c = rc[len(rc) // 2]
            keypoints[n] = (2.0 * r / (H - 1) - 1.0, 2.0 * c / (W - 1) - 1.0)
        kfs.append(KeyFrame(T(image), T(K), T(L), T(keypoints), T(masks)))
        klds.append(T((0.2 * rng.standard_normal(N) + 0.5).astype(np.float32)))
        tab = table_of(kfs[-1])
        tables.append(dict(pix=npy(tab.pix).view(np.uint32), baseL=npy(tab.baseL), seg_off=npy(tab.seg_off), N=tab.N, P=tab.P, K=K))
        want = ref.table_from_masks(masks, L, K)
        assert tab.P == want['P'] and np.array_equal(tables[-1]['pix'] & 0x7fffffff, want['pix'])           # row-major within a segment
        assert np.array_equal(tables[-1]['seg_off'][:N], want['seg_off'][:N]) and np.array_equal(_bits(tables[-1]['baseL']), _bits(want['baseL']))
    return kfs, klds, tables


def _records(rng, n):
    record = np.zeros((n, 32))
    recs = []
    for r in range(n):
        rec = dict(rot=base.pose_of(rng.uniform(-1, 1, 3), [0, 0, 0])[:3, :3].astype(np.float64), trans_scaled=rng.uniform(-3, 3, 3), s=(0.37, 2.6)[r % 2],
                   rot_reanchor=base.pose_of(rng.uniform(-1, 1, 3), [0, 0, 0])[:3, :3].astype(np.float64))
        record[r, 0:9], record[r, 9:12], record[r, 15], record[r, 16:25] = rec['rot'].reshape(-1), rec['trans_scaled'], rec['s'], rec['rot_reanchor'].reshape(-1)
        recs.append(rec)
    return record, recs


def _ulps(got, want):
    """|got - want| in units of want's float32 spacing (+0 and -0 are one value)."""
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -126))).astype(np.float64)


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("with_align", [False, True], ids=["plain", "aligned"])
def test_normals_against_the_statement(stride, with_align):
    """Two keyframes of different sizes (24 x 32 with six segments: a 768-point one across three workgroups, one pixel, one row, a hole,
    two overlapping, a NaN; 17 x 21 with one ragged segment), stride 1 and 3 (a row's neighbours are then not rows), with and without
    alignment records: every component within 1 float32 ulp of the statement rounded once."""
    from super_primitive_amd.odometery.results import keyframe_points
    kfs, klds, tables = _scene()
    rng = np.random.default_rng(403)
    poses = np.stack([base.pose_of(rng.uniform(-1.2, 1.2, 3), rng.uniform(-2, 2, 3)) for _ in kfs])
    align, recs = None, None
    if with_align:
        record, two = _records(rng, 2)
        align, recs = T(record), [two[1], two[0]]
    out = keyframe_points(kfs, klds, T(poses), stride=stride, align=align, align_index=[1, 0] if with_align else None, normals=True)
    plain = keyframe_points(kfs, klds, T(poses), stride=stride, align=align, align_index=[1, 0] if with_align else None)
    got = npy(out['normals'])
    assert 'normals' not in plain and all(_same(out[k], plain[k]) for k in ('points', 'colours', 'kf_index', 'seg_ids'))
    assert got.dtype == np.float32 and got.shape == tuple(out['points'].shape)
    want = ref.map_normals(tables, stride, poses, recs).astype(np.float32)
    assert want.shape == got.shape
    ulps = _ulps(got, want)
    differ = int((ulps > 0).sum())
    print(f"\nnormals stride {stride} {'aligned' if with_align else 'plain'}: {got.shape[0]} rows, {differ} of {got.size} components differ, worst {ulps.max():.2f} ulp")
    assert ulps.max() <= 1.0
    zero = ~want.any(axis=1)
    assert np.array_equal(~got.any(axis=1), zero) and zero.sum() == (4 if stride == 1 else zero.sum())
    length = np.linalg.norm(got[~zero].astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6                                     # (a float32 rotation is orthonormal to about 1e-7)
    again = npy(keyframe_points(kfs, klds, T(poses), stride=stride, align=align, align_index=[1, 0] if with_align else None, normals=True)['normals'])
    assert np.array_equal(_bits(got), _bits(again))


def test_normals_do_not_depend_on_the_keypoint_log_depths():
    from super_primitive_amd.odometery.results import keyframe_points
    kfs, klds, _ = _scene()
    eye = T(np.repeat(EYE, 2, axis=0))
    a = keyframe_points(kfs, klds, eye, normals=True)
    b = keyframe_points(kfs, [k + 0.75 for k in klds], eye, normals=True)
    assert _same(a['normals'], b['normals']) and not _same(a['points'], b['points'])


def test_normal_rows_are_the_rows_of_the_points():
    """The linear-log-depth segment (segment 0 of the first keyframe, identity pose: world = camera frame): the chord from row j to its
    right and its lower table neighbour lies in the tangent plane of row j up to second order.
    The bound.  p(u) = e^L(u) ray(u) with L linear of slope g along the axis and ray linear of slope 1 / f: p'' = e^L (g^2 ray + 2 g ray'),
    so the chord to the next pixel leaves the tangent plane by at most 1/2 d_max (g^2 |ray|_max + 2 |g| / f).  Added: the error of the
    normal (within 1e-5 of the analytic one: tests/test_map_surfel_ref_host.py derives 7e-6) times the chord's length, and 16 float32
    roundings of the largest coordinate for the two points (float32 fma arithmetic)."""
    from super_primitive_amd.odometery.results import keyframe_points
    kfs, klds, tables = _scene()
    out = keyframe_points(kfs, klds, T(np.repeat(EYE, 2, axis=0)), normals=True)
    tab = tables[0]
    n_rows = int(tab['seg_off'][1])
    p, n = npy(out['points'])[:n_rows].astype(np.float64), npy(out['normals'])[:n_rows].astype(np.float64)
    K = tab['K'].astype(np.float64)
    rows, cols = (tab['pix'][:n_rows] & 0x7fffffff) >> 16, tab['pix'][:n_rows] & 0xffff
    assert n_rows == 768 and np.array_equal(rows * 32 + cols, np.arange(768))
    ray = np.sqrt(((cols - K[0, 2]) / K[0, 0]) ** 2 + ((rows - K[1, 2]) / K[1, 1]) ** 2 + 1.0).max()
    d_max, p_max = p[:, 2].max(), np.abs(p).max()
    assert (np.einsum('ij,ij->i', n, p) < 0).all()                                  # every normal faces the camera
    worst = 0.0
    for step, g, f in ((1, ref.LINEAR['alpha'], K[0, 0]), (32, ref.LINEAR['beta'], K[1, 1])):
        j = np.arange(n_rows - step)
        j = j[(cols[j] < 31)] if step == 1 else j
        chord = p[j + step] - p[j]
        off = np.abs(np.einsum('ij,ij->i', n[j], chord))
        bound = 0.5 * d_max * (g * g * ray + 2.0 * abs(g) / f) + 1e-5 * np.linalg.norm(chord, axis=1).max() + 16 * 2.0 ** -24 * p_max
        worst = max(worst, float(off.max() / bound))
        assert off.max() <= bound, (step, off.max(), bound)
    print(f"\nnormals . chords to the right / lower neighbour: worst {worst:.3f} of the bound")


# ---- surfels ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    return ref.CASES[name]()


@functools.lru_cache(maxsize=None)
def _want(name, k, cull):
    return ref.view_of(_case(name), k, cull)


def _render(c, cull=0, radii="own", normals="own", **kw):
    from super_primitive_amd.tool import viz
    rad = c['radii'] if isinstance(radii, str) else radii
    nrm = c['normals'] if isinstance(normals, str) else normals
    extra = {} if rad is None else dict(radii=T(rad), max_px=c.get('max_px', 8))
    if nrm is not None:
        extra.update(normals=T(nrm), cull=bool(cull))
    out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', EYE)), c['H'], c['W'], depth_buffer=True, **extra, **kw)
    return {k: npy(v) for k, v in out.items()}


def _compare(name, out, cull):
    c = _case(name)
    excluded = []
    for k in range(len(c.get('poses', EYE))):
        (image, depth, index), mask = _want(name, k, cull)
        excluded.append(int((~mask).sum()))
        assert mask.mean() >= 0.98
        np.testing.assert_array_equal(out['index'][k][mask], index[mask], err_msg=f"{name} view {k} cull {cull}: index")
        np.testing.assert_array_equal(out['image'][k][mask], image[mask], err_msg=f"{name} view {k} cull {cull}: image")
        np.testing.assert_array_equal(_bits(out['depth'][k])[mask], _bits(depth)[mask], err_msg=f"{name} view {k} cull {cull}: depth")
    print(f"\n{name} cull {cull}: pixels excluded per view {excluded}; coverage {[round(float((out['index'][k] >= 0).mean()), 3) for k in range(len(excluded))]}")


def _raw_surfels(name, cull, image=True, depth=True, index=True):
    """sp_render_surfels on keys and outputs pre-filled with junk: every pixel of every requested output has to be written."""
    from super_primitive_amd import _lib
    c = _case(name)
    poses = c.get('poses', EYE)
    V, H, W = len(poses), c['H'], c['W']
    views = T(np.concatenate([np.tile(c['K'].reshape(1, 9), (V, 1)), poses.reshape(V, 16)], axis=1).astype(np.float32))
    pts, cols, rad, nrm = T(c['points']), T(c['colours']), T(c['radii']), T(c['normals'])
    keys = torch.full((V * H * W,), -1, dtype=torch.int64, device=pts.device)
    out = dict(image=torch.full((V, H, W, 3), 0xAB, dtype=torch.uint8, device=pts.device) if image else None,
               depth=torch.full((V, H, W), 777.0, dtype=torch.float32, device=pts.device) if depth else None,
               index=torch.full((V, H, W), 12345, dtype=torch.int32, device=pts.device) if index else None)
    lib = _lib.load()
    _lib.check(lib.sp_render_surfels(_lib.ptr(pts), _lib.ptr(cols), _lib.ptr(nrm), len(c['points']), _lib.ptr(views), V, H, W, 1e-6, _lib.ptr(rad),
                                     c['max_px'], cull, _lib.ptr(keys), _lib.ptr(out['image']), _lib.ptr(out['depth']), _lib.ptr(out['index']),
                                     _lib.stream_ptr()), "sp_render_surfels")
    torch.cuda.synchronize()
    return {k: None if v is None else npy(v) for k, v in out.items()}


@pytest.mark.parametrize("cull", [0, 1])
def test_surfel_posed(cull):
    """3001 points with random unit normals (every 11th zero: flat), three posed views in one call, half the cloud behind one camera, an
    empty view; outputs pre-filled with junk, each left out in turn; two runs give the same bits; the Python surface gives the raw call."""
    out = _raw_surfels("surfel_posed", cull)
    _compare("surfel_posed", out, cull)
    assert not out['image'][2].any() and not out['depth'][2].any() and (out['index'][2] == -1).all()
    again = _raw_surfels("surfel_posed", cull)
    for key in out:
        assert np.array_equal(_bits(out[key]), _bits(again[key])), key
    for left_out in ('image', 'depth', 'index'):
        part = _raw_surfels("surfel_posed", cull, **{left_out: False})
        assert part[left_out] is None
        for key in out:
            if key != left_out:
                assert np.array_equal(_bits(part[key]), _bits(out[key])), (left_out, key)
    through_viz = _render(_case("surfel_posed"), cull)
    for key in out:
        assert np.array_equal(_bits(through_viz[key]), _bits(out[key])), key
    flat = _render(_case("surfel_posed"), normals=None)
    covered, flat_covered = out['index'] >= 0, flat['index'] >= 0
    # coverage is the footprints', less the culled surfels and the pixels whose t leaves (z_min, inf)
    assert (flat_covered | ~covered).all() and (covered.sum() > 0.9 * flat_covered.sum() if cull == 0 else covered.sum() < flat_covered.sum())
    assert (out['depth'][0] != flat['depth'][0]).mean() > 0.3


@pytest.mark.parametrize("cull", [0, 1])
def test_surfel_views17(cull):
    """17 views, one more than a staging chunk."""
    out = _render(_case("surfel_views17"), cull)
    assert out['index'].shape == (17, 30, 40)
    _compare("surfel_views17", out, cull)
    assert (out['index'][16] >= 0).mean() > 0.1


def test_surfel_collide():
    """70 001 points into 24 x 32, ids beyond 65 535, from the identity pose (bitwise everywhere) and from a posed view."""
    out = _render(_case("surfel_collide"))
    _compare("surfel_collide", out, 0)
    assert _want("surfel_collide", 0, 0)[1].all()
    assert out['index'][0].max() > 65535 and (out['index'] > 65535).sum() >= 10


@pytest.mark.parametrize("cull", [0, 1])
def test_surfel_edges(cull):
    """Identity pose, bitwise on every pixel: den = 0, both clamps, zero / NaN / infinite normals, s = 0, back-facing, NaN / negative /
    zero / infinite / 1e9 radii, pixels with t <= z_min under a z > z_min, squares reaching and missing the borders
    (tests/test_map_surfel_ref_host.py asserts what each row does in the statement)."""
    c = _case("surfel_edges")
    out = _render(c, cull)
    _compare("surfel_edges", out, cull)
    assert _want("surfel_edges", 0, cull)[1].all()
    idx, R = out['index'][0], ref.EDGE_ROWS
    gone = {R['misses']} | ({R['s_zero'], R['back']} if cull else set())
    assert set(idx[idx >= 0].tolist()) == set(range(16)) - gone
    assert out['depth'][0, 4, 12] == 2.5 and out['depth'][0, 4, 13] == 1.5 and out['depth'][0, 4, 3] == 1.75
    for q in (R['reaches'], R['misses']):                                      # Q = 1: a kept and a dropped single surfel
        one = _render(dict(c, points=c['points'][q:q + 1], colours=c['colours'][q:q + 1], radii=c['radii'][q:q + 1], normals=c['normals'][q:q + 1]), cull)
        assert int((one['index'] >= 0).sum()) == (3 if q == R['reaches'] else 0)


@pytest.mark.parametrize("name", ["surfel_posed", "surfel_edges", "surfel_collide"])
def test_zero_normals_are_the_footprint_render_on_every_pixel(name):
    """All normals zero (and, in a second run, NaN): sp_render_splats, bit for bit; no reference is involved."""
    c = _case(name)
    want = _render(c, normals=None)
    for fill in (0.0, np.nan):
        for cull in (0, 1):
            got = _render(c, cull, normals=np.full_like(c['normals'], fill))
            for key in ('image', 'depth', 'index'):
                assert np.array_equal(_bits(got[key]), _bits(want[key])), (fill, cull, key)
    assert (want['index'] >= 0).sum() > 100


@pytest.mark.parametrize("make", [base.case_posed, lambda: base.case_duplicates()[0]], ids=["posed", "duplicates"])
def test_radius0_is_the_point_render_on_every_pixel(make):
    """All radii 0 -- sp_render_views in mode 1, bit for bit, whatever the normals; no reference is involved."""
    c = make()
    want = _render(c, radii=None, normals=None)
    normals = ref.unit_normals(len(c['points']), 9)
    for max_px in (0, 3, 16):
        got = _render(dict(c, max_px=max_px), radii=np.zeros(len(c['points']), np.float32), normals=normals)
        for key in ('image', 'depth', 'index'):
            assert np.array_equal(_bits(got[key]), _bits(want[key])), (max_px, key)
    assert (want['index'] >= 0).sum() > 100


# ---- the reason for the feature ---------------------------------------------------------------------------------------------------------
def _rounding_bound(c):
    """What float32 inputs and a float32 output can cost the depth of a surfel's pixel, and whether the clamp can act.
    Exact: the pixel's ray meets the tangent plane of sample p at t = (n . p) / (n . ray).  The kernel has float32(p) and float32(n), each
    component off by at most e = 2^-24 relative, so its s is off by at most (2 e + e^2) S_np, S_np = sum_k |n_k p_k|, and its den by
    e S_nr, S_nr = sum_k |n_k ray_k|; t = s / den then moves by at most ((2 e + e^2) S_np + e t S_nr) / (|den| - e S_nr).  The float64
    operations themselves (1e-12) do not show.  float32(t) costs e t, and the ground truth is stored as float32: e t again.  The
    maxima are taken over every (sample, pixel of its rectangle) the statement's rectangles give.  Returns (bound, every |t - z| < h)."""
    e = 2.0 ** -24
    Kd = c['K_mid'].astype(np.float64)
    fx, fy, cx, cy = Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]
    gt = c['gt'].astype(np.float64)
    S_np = S_nr = 0.0
    den_min, slack = np.inf, np.inf
    for i, (r0, r1, c0, c1), z, nc, s, h in ref.surfels(c['points'], c['normals'], c['radii'], c['K_mid'], None, c['H'], c['W'], c['max_px']):
        p = c['points'][i].astype(np.float64)
        S_np = max(S_np, float(np.abs(np.array(nc) * p).sum()))
        for r in range(r0, r1 + 1):
            for col in range(c0, c1 + 1):
                ray = np.array([((col + 0.5) - cx) / fx, ((r + 0.5) - cy) / fy, 1.0])
                S_nr = max(S_nr, float(np.abs(np.array(nc) * ray).sum()))
                den_min = min(den_min, abs(float(np.array(nc) @ ray)))
                slack = min(slack, h - abs(gt[r, col] - z))
    t = float(gt.max())
    return ((2 * e + e * e) * S_np + e * t * S_nr) / (den_min - e * S_nr) + 2 * e * t + 1e-12, slack


@pytest.mark.parametrize("footprint", [2.0, 3.0])
@pytest.mark.parametrize("surface", ["linear_depth", "plane"])
def test_slanted_surface_renders_at_true_depth(surface, footprint):
    """The half-sampled slanted 48 x 64 surfaces through ``render_map`` / ``score_map`` with the exact normals in the world dict and the
    ground truth at pixel-centre rays: ``linear_depth`` is the very input the flat render is pinned on (0.0250001 / 0.0350001), whose
    depth is linear in the pixel coordinates and therefore not a plane in space -- its bound adds the curvature term derived in
    map_surfel_ref.case_plane --; ``plane`` is a plane in space, where only float32 rounding is left (``_rounding_bound``).  The clamp
    z -+ 2 rad is shown not to be in reach first.  Observed worst errors, flat -> oriented: linear_depth 0.0250001 -> 2.24e-4 (footprint 2)
    and 0.0350001 -> 2.24e-4 (3); plane 0.0321403 -> 2.4e-7 and 0.0440104 -> 2.4e-7."""
    from super_primitive_amd.odometery.results import render_map, score_map
    c = ref.case_plane(footprint) if surface == "linear_depth" else ref.case_true_plane(footprint)
    H, W = c['H'], c['W']
    world = dict(points=T(c['points']), colours=T(c['colours']), normals=T(c['normals']))
    K_mid, eye, rad = T(c['K_mid']), T(EYE), T(c['radii'])
    rounding, slack = _rounding_bound(c)
    bound = rounding + c.get('curvature', 0.0)
    assert slack > 0 and rounding < 2e-6
    flat = render_map(world, K_mid, eye, (H, W), radii=rad, max_px=c['max_px'])
    gt = c['gt'].astype(np.float64)
    e_flat = np.abs(npy(flat['depth'][0]).astype(np.float64) - gt).max()
    for cull in (False, True):
        out = render_map(world, K_mid, eye, (H, W), radii=rad, max_px=c['max_px'], normals=True, cull=cull)
        assert float((out['index'] >= 0).float().mean()) == 1.0
        err = np.abs(npy(out['depth'][0]).astype(np.float64) - gt)
        print(f"\n{surface}, footprint {footprint}, cull {cull}: worst error oriented {err.max():.3e} (bound {bound:.3e}), flat {e_flat:.7f}")
        assert err.max() <= bound and err.max() < e_flat
        want = ref.render(c['points'], c['colours'], c['normals'], c['radii'], c['K_mid'], None, H, W, c['max_px'], int(cull))
        for key, w in zip(('image', 'depth', 'index'), want):
            np.testing.assert_array_equal(_bits(npy(out[key][0])), _bits(w))
    tilt = score_map(world, T(c['gt'][None]), K_mid, eye, radii=rad, max_px=c['max_px'], normals=True)
    level = score_map(world, T(c['gt'][None]), K_mid, eye, radii=rad, max_px=c['max_px'])
    col = {name: k for k, name in enumerate(tilt['columns'])}
    assert float(tilt['coverage'][0]) == 1.0 == float(level['coverage'][0])
    assert float(tilt['metrics'][0, col['rmse']]) < float(level['metrics'][0, col['rmse']])


def test_sequence_map_scored_flat_and_oriented():
    """The 30-frame sequence of tests/test_gpu_sequence_results.py, its map at that test's stride 4 with ``sequence_map(normals=True)``
    normals, scored against the ground-truth depth from the ground-truth keyframe cameras with flat and with oriented footprints of 4
    source pixels (stride counts along a table row).  Recorded, not judged: nobody has measured it before; finite, coverage unchanged."""
    from test_gpu_sequence import make_sequence_inputs
    from super_primitive_amd.odometery.results import point_radii, score_map, sequence_map
    from super_primitive_amd.odometery.sequence import run_sequence
    seq, frames, to_kf = make_sequence_inputs()
    out = run_sequence(frames, to_kf, T(seq[0].T_wc), T(seq[0].kld_gt), engine="gn", keep_keyframes=True, window_size=2, translation_thresh=0.1)
    G = np.stack([f.T_wc for f in seq]).astype(np.float32)
    world = sequence_map(out, 4, T(G), normals=True)
    plain = sequence_map(out, 4, T(G))
    assert torch.equal(world['points'], plain['points']) and tuple(world['normals'].shape) == tuple(world['points'].shape)
    length = world['normals'].double().norm(dim=1)
    assert bool(((length - 1).abs() < 1e-5).logical_or(length == 0).all())         # (the archive poses are float32 products)
    ids = world['ids']
    Ks = T(np.stack([seq[i].K for i in ids]).astype(np.float32))
    gt = T(np.stack([seq[i].depth for i in ids]).astype(np.float32))
    radii = point_radii(world, out, footprint=4.0)
    flat = score_map(world, gt, Ks, T(G[ids]), radii=radii)
    tilt = score_map(world, gt, Ks, T(G[ids]), radii=radii, normals=True)
    col = {name: k for k, name in enumerate(flat['columns'])}
    a, b = npy(flat['metrics'])[:, col['rmse']], npy(tilt['metrics'])[:, col['rmse']]
    print(f"\nsequence map, stride 4, footprint 4, {world['points'].shape[0]} points: rmse per view flat {np.round(a, 2).tolist()} mm, oriented "
          f"{np.round(b, 2).tolist()} mm; coverage {np.round(npy(flat['coverage']), 4).tolist()}")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert torch.equal(flat['coverage'], tilt['coverage'])


# ---- fusion and filtering ---------------------------------------------------------------------------------------------------------------
def test_filter_fuse_and_export_carry_normals(tmp_path):
    from super_primitive_amd.odometery.results import filter_map, fuse_map, fused_normals, keyframe_points, write_ply
    kfs, klds, _ = _scene()
    rng = np.random.default_rng(404)
    poses = np.stack([base.pose_of(0.05 * rng.standard_normal(3), 0.05 * rng.standard_normal(3)) for _ in kfs])
    world = keyframe_points(kfs, klds, T(poses), normals=True)
    Q = int(world['points'].shape[0])
    counts = torch.zeros(Q, 3, dtype=torch.int32, device=world['points'].device)
    counts[::3, 0] = 1
    kept = filter_map(world, dict(counts=counts))
    assert _same(kept['normals'], world['normals'][::3]) and _same(kept['points'], world['points'][::3])
    clean = filter_map(world, dict(counts=(torch.isfinite(world['points']).all(dim=1, keepdim=True)).int().expand(Q, 3).contiguous()))
    fused, again = fuse_map(clean, 0.08), fuse_map(clean, 0.08)
    M = int(fused['points'].shape[0])
    assert 0 < M < int(clean['points'].shape[0]) and tuple(fused['normals'].shape) == (M, 3) and fused['normals'].dtype == torch.float32
    assert torch.equal(fused['normals'].view(torch.int32), again['normals'].view(torch.int32))
    length = fused['normals'].double().norm(dim=1)
    assert bool(((length - 1).abs() < 2e-7).logical_or(length == 0).all()) and float((length > 0).float().mean()) > 0.9
    on_host = fused_normals(clean['normals'].cpu(), fused['label'].cpu(), M)
    assert torch.equal(on_host.view(torch.int32), fused['normals'].cpu().view(torch.int32))       # the helper's CPU path, bit for bit
    bare = fuse_map({k: v for k, v in clean.items() if k != 'normals'}, 0.08)
    assert 'normals' not in bare and torch.equal(bare['points'], fused['points'])
    raw = open(write_ply(tmp_path / "fused.ply", fused), 'rb').read()
    head, body = raw.split(b"end_header\n", 1)
    rows = np.frombuffer(body, dtype=np.dtype([('p', '<f4', 3), ('n', '<f4', 3), ('c', 'u1', 3)]))
    assert f"element vertex {M}\n".encode() in head and b"property float nx" in head and len(rows) == M
    assert np.array_equal(rows['p'], npy(fused['points'])) and np.array_equal(_bits(rows['n'].copy()), _bits(npy(fused['normals'])))
