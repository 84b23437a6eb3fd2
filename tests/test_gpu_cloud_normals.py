"""-m gpu: normals from neighbour lists (csrc/sp_knn.hip sp_cloud_normals through the C ABI, ``tool/viz.py`` ``cloud_normals``,
``odometery/results.py`` ``estimate_normals`` / ``statistical_outliers`` / ``select_map``) against the float64 reference of
tests/cloud_knn_ref.py, whose solver is ``numpy.linalg.eigh``.

``used`` is exact.  The angle between the device normal and the reference eigenvector is held to ``2^-22 + 64 * 2^-52 * l2 / (l1 - l0)``
(float32 rounding of three components; Davis-Kahan with a constant of 64 over float64's unit roundoff, for two different backward-stable
3 x 3 solvers), the curvature to ``128 * 2^-52 + 2^-23 * curvature``.  Outputs are pre-filled with 0x7f bytes and every entry must have
been written."""
import numpy as np
import pytest
import torch

import cloud_knn_ref as ref
import cloud_register_ref as reg
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK32 = 0x7f7f7f7f
ORIGIN = (0.0, 0.0, 0.0)


def _raw(points, queries, index, toward=None, owner=None):
    """sp_cloud_normals through the C ABI on junk-filled outputs; returns the host arrays."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    pts = T(np.asarray(points, np.float32))
    qs = pts if queries is points else T(np.asarray(queries, np.float32))
    idx = T(np.ascontiguousarray(index, dtype=np.int32))
    Qa, k = idx.shape
    view = None if toward is None else T(np.asarray(toward, np.float32).reshape(-1, 3))
    own = None if owner is None else T(np.asarray(owner, np.int32))
    junk = lambda *shape: torch.full(shape, JUNK32, dtype=torch.int32, device=pts.device)
    normals, curvature, used = junk(Qa, 3), junk(Qa), junk(Qa)
    _lib.check(lib.sp_cloud_normals(_lib.ptr(pts), len(points), _lib.ptr(qs), _lib.ptr(idx), Qa, k, _lib.ptr(view), 0 if view is None else len(view),
                                    _lib.ptr(own), _lib.ptr(normals), _lib.ptr(curvature), _lib.ptr(used), _lib.stream_ptr()), "sp_cloud_normals")
    torch.cuda.synchronize()
    out = dict(normals=npy(normals), curvature=npy(curvature), used=npy(used))
    for key, v in out.items():
        assert not (v.view(np.uint32) == JUNK32).any(), f"{key} has entries that were not written"
    out['normals'], out['curvature'] = out['normals'].view(np.float32), out['curvature'].view(np.float32)
    return out


def _check(got, want, what):
    """``used`` exact, NaN rows where the reference has them, the angle and the curvature within their bounds; returns the largest
    observed ratio of the angle to its bound."""
    np.testing.assert_array_equal(got['used'], want['used'], err_msg=f"{what}: used")
    nan = np.isnan(want['normals']).any(axis=1)
    assert np.array_equal(np.isnan(got['normals']).all(axis=1), nan) and np.array_equal(np.isnan(got['normals']).any(axis=1), nan), f"{what}: NaN rows"
    assert np.array_equal(np.isnan(got['curvature']), nan), f"{what}: NaN curvature"
    ok = ~nan
    n = got['normals'][ok].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 2.0 ** -22, f"{what}: not unit"
    ratio = ref.angle(n, want['normals'][ok]) / ref.angle_bound(want['gap'][ok])
    c_err = np.abs(got['curvature'][ok].astype(np.float64) - want['curvature'][ok]) / ref.curvature_bound(want['curvature'][ok])
    print(f"\n{what}: {ok.sum()} normals, {nan.sum()} NaN rows, largest l2 / (l1 - l0) {want['gap'][ok].max():.3g}, angle / bound at most {ratio.max():.3f}, "
          f"curvature error / bound at most {c_err.max():.3f}")
    assert ratio.max() <= 1.0, f"{what}: angle beyond the bound"
    assert c_err.max() <= 1.0 and (got['curvature'][ok] >= 0).all() and (got['curvature'][ok] <= np.float32(1 / 3)).all(), f"{what}: curvature"
    return float(ratio.max())


def _dot3(n, e):
    return (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]


def test_unit_sphere():
    """4001 points of the unit sphere, r = 0.15, k = 16: the reference's own lists; used, angle, curvature, the three orientations, and
    the analytic surface."""
    p = ref.sphere()
    lists = ref.sphere_lists(0.15, 16)
    want = ref.normals(p, p, lists['index'])
    assert (want['used'] >= 3).all() and (want['used'] == 16).mean() > 0.9 and not np.isnan(want['normals']).any()
    got = _raw(p, p, lists['index'])
    _check(got, want, "sphere, r 0.15, k 16")
    n = got['normals'].astype(np.float64)
    assert (n[np.arange(len(n)), np.abs(n).argmax(axis=1)] > 0).all()         # without a viewpoint: the largest component is positive
    radial = p.astype(np.float64)
    to_radial = ref.angle(n, radial)
    print(f"angle to the radial direction: mean {to_radial.mean():.4f}, max {to_radial.max():.4f} (reference {ref.angle(want['normals'], radial).mean():.4f})")
    assert to_radial.mean() < 0.15                                             # the angular size of the neighbourhood, r / R
    inward = _raw(p, p, lists['index'], toward=np.zeros(3, np.float32))
    _check(inward, ref.normals(p, p, lists['index'], toward=np.zeros(3, np.float32)), "sphere, towards the centre")
    assert (_dot3(inward['normals'].astype(np.float64), radial) < 0).all()     # every normal points at the origin
    assert np.array_equal(np.abs(inward['normals']), np.abs(got['normals']))   # (the orientation changes signs only)
    view = np.array([0.0, 0.0, 10.0], np.float32)
    seen = _raw(p, p, lists['index'], toward=view)
    want_seen = ref.normals(p, p, lists['index'], toward=view)
    e = view.astype(np.float64)[None] - radial
    dot, want_dot = _dot3(seen['normals'].astype(np.float64), e), _dot3(want_seen['normals'], e)
    sure = np.abs(want_dot) > 1e-5                                             # (the float32 rounding of n moves the product by < 2^-22 |e|)
    assert sure.mean() > 0.99 and np.array_equal(dot[sure] > 0, want_dot[sure] > 0) and (want_dot >= 0).all() and (dot > -1e-5).all()
    assert 0.2 < (dot * _dot3(n, e) < 0).mean() < 0.5                          # about a third of the rows were turned over
    # two viewpoints by owner; an owner outside them keeps the rule without a viewpoint
    owner = (np.arange(len(p)) % 4 - 1).astype(np.int32)                       # -1, 0, 1, 2: two of the four have no viewpoint
    views = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 10.0]], np.float32)
    mixed = _raw(p, p, lists['index'], toward=views, owner=owner)
    for o, other in ((-1, got), (0, inward), (1, seen), (2, got)):
        assert np.array_equal(mixed['normals'][owner == o], other['normals'][owner == o]), o


def test_sphere_with_short_and_nearly_round_neighbourhoods():
    """r = 0.1, k = 8: l2 / (l1 - l0) reaches thousands -- the bound scales with it -- and a few rows have fewer than three members:
    those come back NaN with the right ``used``."""
    p = ref.sphere()
    lists = ref.sphere_lists(0.1, 8)
    want = ref.normals(p, p, lists['index'])
    few = want['used'] < 3
    assert 0 < few.sum() < 40 and np.isnan(want['normals'][few]).all() and want['gap'][~few].max() > 100
    got = _raw(p, p, lists['index'])
    _check(got, want, "sphere, r 0.1, k 8")
    assert np.isnan(got['normals'][few]).all() and np.array_equal(got['used'][few], want['used'][few])


def test_degenerate_neighbourhoods():
    """An exactly collinear lattice line and coincident points give NaN; a flat lattice plane gives +-z and no curvature."""
    line = np.stack([np.arange(40) * 0.25 + 5.0, np.full(40, -3.0), np.full(40, 1.5)], axis=1).astype(np.float32)
    lists = ref.knn(line, line, 0.6, ORIGIN, 5)
    got = _raw(line, line, lists['index'])
    assert (got['used'] >= 3).all() and np.array_equal(got['used'], ref.normals(line, line, lists['index'])['used'])
    assert np.isnan(got['normals']).all() and np.isnan(got['curvature']).all()
    twins = np.full((300, 3), 0.7, np.float32)
    got = _raw(twins, twins, ref.knn(twins, twins, 0.1, ORIGIN, 8)['index'])
    assert (got['used'] == 8).all() and np.isnan(got['normals']).all() and np.isnan(got['curvature']).all()
    k2 = np.stack(np.meshgrid(np.arange(17), np.arange(17), indexing='ij'), axis=-1).reshape(-1, 2)
    plane = np.concatenate([k2 * 0.25 - 2.0, np.full((289, 1), 3.0)], axis=1).astype(np.float32)
    lists = ref.knn(plane, plane, 0.4, ORIGIN, 9)
    want = ref.normals(plane, plane, lists['index'])
    got = _raw(plane, plane, lists['index'])
    _check(got, want, "lattice plane")
    assert np.array_equal(got['normals'], np.tile(np.float32([0, 0, 1]), (289, 1))) and not got['curvature'].any()
    down = _raw(plane, plane, lists['index'], toward=np.zeros(3, np.float32))
    assert np.array_equal(down['normals'], np.tile(np.float32([0, 0, -1]), (289, 1)))


def test_lists_handed_in_by_the_caller():
    """Lists with -1, Q, 2^31 - 1 and a point with a NaN coordinate, queries that are not points of the cloud: the entries are skipped,
    nothing faults, and the result is the reference's."""
    rng = np.random.default_rng(41)
    p = ref.sphere(1000, 9).copy()
    Q, Qa, k = len(p), 513, 12
    p[17, 1], p[400, 0] = np.nan, np.inf
    q = (p[rng.integers(0, Q, Qa)] + rng.normal(scale=0.01, size=(Qa, 3))).astype(np.float32)
    q[np.isnan(q) | np.isinf(q)] = 0.5
    index = rng.integers(0, Q, (Qa, k)).astype(np.int64)
    index[rng.uniform(size=(Qa, k)) < 0.2] = -1
    index[rng.uniform(size=(Qa, k)) < 0.1] = Q
    index[rng.uniform(size=(Qa, k)) < 0.1] = 2 ** 31 - 1
    index[rng.uniform(size=(Qa, k)) < 0.05] = -2 ** 31
    index[::7, 3], index[::11, 5] = 17, 400
    index[5], index[6, 2:] = -1, Q                                             # nothing at all; two points
    want = ref.normals(p, q, index)
    got = _raw(p, q, index)
    _check(got, want, "caller's lists")
    assert got['used'][5] == 0 and got['used'][6] <= 2 and np.isnan(got['normals'][[5, 6]]).all() and 3 < got['used'].mean() < k


def test_cloud_normals_is_the_three_calls():
    """``viz.cloud_normals``: its lists are the reference's, its normals what the raw call gives on them, to the bit; a grid handed in
    is used; ``estimate_normals`` returns a new dict with the three entries."""
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    p = ref.sphere()
    lists = ref.sphere_lists(0.15, 16)
    view = np.array([0.0, 0.0, 10.0], np.float32)
    raw = _raw(p, p, lists['index'], toward=view)
    out = viz.cloud_normals(T(p), 0.15, k=16, toward=T(view))
    assert set(out) == {'normals', 'curvature', 'used', 'knn'} and out['normals'].dtype == torch.float32 and out['used'].dtype == torch.int32
    assert np.array_equal(npy(out['knn']['index']), lists['index']) and np.array_equal(npy(out['knn']['count']), lists['count'])
    for key in ('normals', 'curvature', 'used'):
        assert npy(out[key]).tobytes() == raw[key].tobytes(), key
    grid = viz.cloud_grid(T(p), 0.15)
    again = viz.cloud_normals(T(p), 99.0, k=16, toward=T(view[None]), owner=torch.zeros(len(p), dtype=torch.int32, device="cuda"), grid=grid)
    assert torch.equal(again['normals'], out['normals']) and torch.equal(again['knn']['dist'], out['knn']['dist'])
    cloud = dict(points=T(p), colours=T(np.full_like(p, 0.5)), note="kept")
    est = results.estimate_normals(cloud, 0.15, k=16, view_centres=T(view))
    assert set(est) == set(cloud) | {'normals', 'curvature', 'normals_used'} and est['note'] == "kept" and 'normals' not in cloud
    assert torch.equal(est['normals'], out['normals']) and torch.equal(est['normals_used'], out['used']) and est['points'] is cloud['points']
    bare = results.estimate_normals(T(p), 0.15)
    assert set(bare) == {'points', 'normals', 'curvature', 'normals_used'} and np.array_equal(np.abs(npy(bare['normals'])), np.abs(raw['normals']))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _scene():
    """The last scene of tests/test_gpu_cloud_register.py, from its helpers: a 48 x 64 keyframe over a non-flat log-depth table -- here
    WITHOUT normals -- and the lift of its own depth image from a pose 0.03 / 1 degree away."""
    from test_gpu_cloud_register import _bumpy_keyframe
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    H, W = 48, 64
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], dtype=np.float32)
    kf, kld = _bumpy_keyframe(H, W, K, 3)
    world = results.keyframe_points([kf], [kld], T(np.eye(4, dtype=np.float32)[None]), stride=1)
    world['ids'] = [0]
    depth = viz.keyframe_depths([kf], [kld])['depth'][0]
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = reg.rodrigues(np.deg2rad(1.0) * np.array([0.6, -0.64, 0.48])), (0.02, -0.01, 0.02)
    reference = viz.depth_image_lift(depth, T(K), T=T(pose.astype(np.float32)))
    assert world['points'].shape[0] == H * W == reference['points'].shape[0] and world.get('normals') is None
    return world, reference, np.float32(pose).astype(np.float64)


def test_a_lifted_cloud_gets_normals_and_register_map_reaches_its_plane_residual(tmp_path):
    """The lifted cloud has no normals and the map is made without: ``estimate_normals`` gives the reference its own, ``register_map``
    then picks ``'plane'``, ends CONVERGED at the true pose, and in fewer iterations than ``residual='point'`` (measured: 4 against 6,
    and point to point ends 48 mm off -- both clouds are the same lattice of samples and it locks onto neighbouring ones)."""
    from super_primitive_amd.odometery import results
    world, reference, truth = _scene()
    radius = 0.1
    with_normals = results.estimate_normals(reference, radius, k=16, view_centres=T(truth[:3, 3].astype(np.float32)))
    assert 'normals' not in reference and float(torch.isfinite(with_normals['normals']).all(dim=1).float().mean()) > 0.99
    kw = dict(tol=1e-9, max_iters=60)
    out = results.register_map(world, with_normals, radius, **kw)
    named = results.register_map(world, with_normals, radius, residual='plane', **kw)
    by_point = results.register_map(world, with_normals, radius, residual='point', **kw)
    for key in ('rot', 'trans', 's', 'history'):                               # the default is the plane residual
        assert torch.equal(out['transform'][key], named['transform'][key]), key
    assert not torch.equal(out['transform']['history'], by_point['transform']['history'])
    got = dict(R=npy(out['transform']['rot']), t=npy(out['transform']['trans']), s=float(out['transform']['s']))
    n_plane, n_point = int(out['transform']['iterations']), int(by_point['transform']['iterations'])
    print(f"\nlifted cloud with estimated normals: 'plane' {n_plane} iterations (status {int(out['transform']['status'])}), 'point' {n_point} iterations "
          f"(status {int(by_point['transform']['status'])}, |t - truth| {np.abs(npy(by_point['transform']['trans']) - truth[:3, 3]).max():.2e}); "
          f"'plane' |t - truth| {np.abs(got['t'] - truth[:3, 3]).max():.2e}, angle to truth {reg.rotation_angle(got['R'], truth[:3, :3]):.2e}")
    assert int(out['transform']['status']) == reg.CONVERGED
    assert np.abs(got['t'] - truth[:3, 3]).max() < 1e-5 and reg.rotation_angle(got['R'], truth[:3, :3]) < 1e-5 and got['s'] == 1.0
    assert n_plane < n_point
    moved = results.transform_map(with_normals, out['transform']['rot'], out['transform']['trans'])         # transform_map takes the result
    assert tuple(moved['normals'].shape) == tuple(with_normals['normals'].shape)
    coloured = dict(with_normals, colours=torch.full_like(with_normals['points'], 0.5))
    path = results.write_ply(tmp_path / "lifted.ply", coloured)                                                # and write_ply exports nx ny nz
    assert b"property float nx" in open(path, 'rb').read(400)


def test_statistical_outliers_drop_displaced_points():
    """2 % of the map's rows displaced by ten spacings: at least 90 % of them go, and less of the rest than Cantelli's inequality allows
    at two deviations, 1 / (1 + 2^2)."""
    from super_primitive_amd.odometery import results
    world = _scene()[0]
    Q = world['points'].shape[0]
    rng = np.random.default_rng(51)
    moved = np.zeros(Q, bool)
    moved[rng.permutation(Q)[:Q // 50]] = True
    spacing = 2.0 / 60.0                                                        # a pixel at depth 2
    pts = npy(world['points']).copy()
    pts[moved, 2] -= np.float32(10 * spacing)
    dirty = dict(world, points=T(pts))
    out = results.statistical_outliers(dirty, 0.5, k=16, std_ratio=2.0)
    assert set(out) == {'mean_dist', 'keep', 'mu', 'sigma', 'threshold', 'knn'} and tuple(out['knn']['dist'].shape) == (Q, 16)
    keep = npy(out['keep'])
    dropped_moved, dropped_rest = float((~keep[moved]).mean()), float((~keep[~moved]).mean())
    print(f"\nstatistical_outliers: mu {float(out['mu']):.4f}, sigma {float(out['sigma']):.4f}, threshold {float(out['threshold']):.4f}; dropped "
          f"{dropped_moved:.3f} of the {moved.sum()} displaced rows and {dropped_rest:.4f} of the rest")
    assert dropped_moved >= 0.9 and dropped_rest < 0.2
    # the lists are the reference's, and the figures follow from them
    want = ref.knn_candidates(pts, pts, 0.5, ORIGIN, 16, skip_self=True)
    assert np.array_equal(npy(out['knn']['index']), want['index']) and npy(out['knn']['dist']).tobytes() == want['dist'].tobytes()
    mean = want['dist'].astype(np.float64).mean(axis=1)
    assert np.isfinite(mean).all() and np.allclose(npy(out['mean_dist']), mean, rtol=1e-14, atol=0)
    clean = results.select_map(dirty, out['keep'])
    assert clean['points'].shape[0] == keep.sum() == clean['offsets'][-1] and torch.equal(clean['points'], dirty['points'][out['keep']])
    assert clean['ids'] == [0] and torch.equal(clean['kept'], torch.nonzero(out['keep'])[:, 0])
