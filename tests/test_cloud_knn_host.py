"""CPU-only: the ABI of the map neighbourhoods (include/sp_hip.h: sp_cloud_grid_knn, sp_cloud_normals), their argument checks -- made
before any device work, so they answer without a GPU --, the argument checks of the Python surface (``tool/viz.py`` ``nearest_k`` /
``cloud_normals``, ``odometery/results.py`` ``estimate_normals`` / ``statistical_outliers`` / ``select_map``), the arithmetic of
``statistical_outliers`` on CPU tensors against a loop, ``select_map`` against ``filter_map``, and the reference of
tests/cloud_knn_ref.py against itself: its two forms agree."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cloud_knn_ref as ref
import map_nearest_ref as base


def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    for name in ("sp_cloud_grid_knn", "sp_cloud_normals"):
        assert name in _lib.SIGNATURES, name
    assert _lib.SP_CLOUD_KNN_MAX == ref.KNN_MAX == 32


def test_knn_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(queries=p, Qa=10, Q=10, scratch=p, skip_self=0, k=4, index=p, dist=p, count=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_cloud_grid_knn(a['queries'], a['Qa'], a['Q'], a['scratch'], a['skip_self'], a['k'], a['index'], a['dist'], a['count'], None)
    for bad in (dict(queries=None), dict(scratch=None), dict(scratch=ctypes.c_void_p(0x2004)), dict(index=None), dict(dist=None), dict(count=None),
                dict(Qa=0), dict(Qa=-3), dict(Q=0), dict(Q=-1), dict(k=0), dict(k=-1), dict(skip_self=2), dict(skip_self=-1), dict(skip_self=1, Qa=11),
                dict(skip_self=1, Q=9)):
        assert call(**bad) == -1, bad
    for big in (dict(k=33), dict(k=1 << 20), dict(Q=(1 << 28) + 1), dict(Qa=2 ** 31 - 1), dict(Qa=1 << 40), dict(Qa=2 ** 31 - 2, k=2),
                dict(Qa=(2 ** 31 - 2) // 32 + 1, k=32), dict(Qa=1 << 27, k=16)):
        assert call(**big) == -2, big
    assert call(Qa=1 << 40, k=0) == -1 and call(k=33, index=None) == -1 and call(Qa=1 << 40, skip_self=1) == -1    # invalid beats too large


def test_normals_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(points=p, Q=10, queries=p, index=p, Qa=10, k=4, toward=None, V=0, owner=None, normals=p, curvature=p, used=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_cloud_normals(a['points'], a['Q'], a['queries'], a['index'], a['Qa'], a['k'], a['toward'], a['V'], a['owner'], a['normals'],
                                    a['curvature'], a['used'], None)
    for bad in (dict(points=None), dict(queries=None), dict(index=None), dict(normals=None), dict(curvature=None), dict(used=None), dict(Q=0),
                dict(Q=-2), dict(Qa=0), dict(Qa=-1), dict(k=0), dict(k=-7), dict(toward=p, V=0), dict(toward=p, V=-1), dict(toward=p, V=2),
                dict(toward=p, V=0, owner=p)):
        assert call(**bad) == -1, bad
    for big in (dict(k=33), dict(Q=(1 << 28) + 1), dict(Qa=2 ** 31 - 1), dict(Qa=1 << 27, k=16), dict(Qa=2 ** 31 - 2, k=2)):
        assert call(**big) == -2, big
    assert call(k=33, points=None) == -1 and call(Qa=1 << 40, toward=p, V=3) == -1                                 # invalid beats too large


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    pts_cpu = torch.zeros(5, 3)
    grid_cpu = dict(scratch=torch.zeros(8, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0, 0, 0), points=pts_cpu)
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.nearest_k(pts_cpu, grid_cpu, 4)
    with pytest.raises(ValueError, match="HIP-only"):
        viz.cloud_normals(pts_cpu, 0.1)
    with pytest.raises(ValueError, match="HIP-only"):
        results.estimate_normals(dict(points=pts_cpu), 0.1)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts = _meta(5, 3)
    grid = dict(scratch=_meta(5, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0.0, 0.0, 0.0), points=pts)
    for k in (0, -1, 33, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="k "):
            viz.nearest_k(_meta(4, 3), grid, k)
        with pytest.raises(ValueError, match="k "):
            viz.cloud_normals(pts, 0.1, k=k)
        with pytest.raises(ValueError, match="k "):
            results.estimate_normals(pts, 0.1, k=k)
    for bad in (_meta(4, 2), _meta(4), _meta(4, 3, dtype=torch.float16), _meta(0, 3), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            viz.nearest_k(bad, grid, 4)
        with pytest.raises(ValueError):
            viz.cloud_normals(bad, 0.1)
    with pytest.raises(ValueError, match="skip_self"):
        viz.nearest_k(_meta(4, 3), grid, 4, skip_self=True)                    # not the grid's cloud
    for handle in (None, {}, dict(grid, Q=6), dict(grid, Q=0), dict(grid, points=_meta(7, 3)), dict(grid, scratch=None),
                   {k: v for k, v in grid.items() if k != 'radius'}):
        with pytest.raises(ValueError, match="grid"):                          # a handle of the wrong size, or no handle
            viz.nearest_k(_meta(4, 3), handle, 4)
    with pytest.raises(ValueError, match="grid"):
        viz.cloud_normals(_meta(6, 3), 0.1, grid=grid)                         # a handle over another cloud
    for toward in (_meta(2), _meta(3, dtype=torch.float64), _meta(4, 2), _meta(0, 3), _meta(2, 3, 1)):
        with pytest.raises(ValueError, match="toward"):
            viz.cloud_normals(pts, 0.1, toward=toward)
    with pytest.raises(ValueError, match="owner"):
        viz.cloud_normals(pts, 0.1, toward=_meta(2, 3))                        # two viewpoints and nobody says whose
    with pytest.raises(ValueError, match="owner"):
        viz.cloud_normals(pts, 0.1, owner=_meta(5, dtype=torch.int32))         # owners of nothing
    for owner in (_meta(4, dtype=torch.int32), _meta(5, dtype=torch.int64), _meta(5, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="owner"):
            viz.cloud_normals(pts, 0.1, toward=_meta(2, 3), owner=owner)
    for radius in (0.0, -1.0, float("inf"), float("nan"), "wide", None):
        with pytest.raises(ValueError, match="radius"):
            results.estimate_normals(pts, radius)
    with pytest.raises(ValueError, match="cloud"):
        results.estimate_normals(dict(colours=pts), 0.1)
    world = dict(points=pts, colours=_meta(5, 3), kf_index=_meta(5, dtype=torch.int32), seg_ids=_meta(5, dtype=torch.int32), offsets=np.array([0, 5]))
    with pytest.raises(ValueError, match="world"):
        results.statistical_outliers(dict(points=pts), 0.1)
    with pytest.raises(ValueError, match="radius"):
        results.statistical_outliers(world, -0.1)
    with pytest.raises(ValueError, match="k "):
        results.statistical_outliers(world, 0.1, k=40)
    for ratio in (-1.0, float("nan"), float("inf"), "two"):
        with pytest.raises(ValueError, match="std_ratio"):
            results.statistical_outliers(world, 0.1, std_ratio=ratio)
    for knn in ({}, dict(dist=_meta(4, 8)), dict(dist=_meta(5, 8, dtype=torch.float64)), dict(dist=_meta(5)), 3):
        with pytest.raises(ValueError, match="knn"):
            results.statistical_outliers(world, 0.1, knn=knn)
    for keep in (_meta(4, dtype=torch.bool), _meta(5, dtype=torch.int32), _meta(5, 1, dtype=torch.bool), [True] * 5):
        with pytest.raises(ValueError, match="keep"):
            results.select_map(world, keep)
    with pytest.raises(ValueError, match="world"):
        results.select_map(dict(points=pts), _meta(5, dtype=torch.bool))


# ---- statistical_outliers and select_map on CPU tensors -------------------------------------------------------------------------------------
def _world(Q, seed, normals=False):
    rng = np.random.default_rng(seed)
    offsets = np.array([0, Q // 3, Q // 3, Q])                                 # three keyframes, the middle one empty
    kf = np.repeat(np.arange(3), np.diff(offsets)).astype(np.int32)
    w = dict(points=torch.from_numpy(rng.normal(size=(Q, 3)).astype(np.float32)), colours=torch.from_numpy(rng.uniform(size=(Q, 3)).astype(np.float32)),
             kf_index=torch.from_numpy(kf), seg_ids=torch.from_numpy(rng.integers(0, 9, Q).astype(np.int32)), offsets=offsets, ids=[0, 4, 9])
    if normals:
        w['normals'] = torch.from_numpy(rng.normal(size=(Q, 3)).astype(np.float32))
    return w


@pytest.mark.parametrize("std_ratio", [2.0, 0.5])
def test_statistical_outliers_against_a_loop(std_ratio):
    """A hand-made ``knn``: lists of 1 .. 6 finite distances padded with +inf, rows with none; Python floats row by row."""
    from super_primitive_amd.odometery.results import statistical_outliers
    Q, k = 701, 6
    rng = np.random.default_rng(21)
    dist = np.sort(rng.uniform(0.0, 0.1, (Q, k)).astype(np.float32), axis=1)
    dist[np.arange(k)[None, :] >= rng.integers(0, k + 1, Q)[:, None]] = np.inf # (some rows keep nothing)
    dist[:20, 0] = np.float32(0.5)                                              # the outliers
    dist[:20, 1:] = np.inf
    world = _world(Q, 22)
    knn = dict(dist=torch.from_numpy(dist), index=None, count=None)
    got = statistical_outliers(world, 0.5, k=k, std_ratio=std_ratio, knn=knn)
    assert set(got) == {'mean_dist', 'keep', 'mu', 'sigma', 'threshold', 'knn'} and got['knn'] is knn
    assert got['mean_dist'].dtype == torch.float64 and got['keep'].dtype == torch.bool and all(got[x].dim() == 0 for x in ('mu', 'sigma', 'threshold'))
    means = []
    for row in dist.tolist():
        finite = [x for x in row if x < float("inf")]
        means.append(sum(finite) / len(finite) if finite else float("inf"))
    rows = [m for m in means if m < float("inf")]
    mu = sum(rows) / len(rows)
    sigma = math.sqrt(sum((m - mu) ** 2 for m in rows) / len(rows))
    assert 0 < len(rows) < Q
    tol = 4 * Q * 2.0 ** -52                                                   # reordered float64 sums of Q non-negative terms
    assert abs(float(got['mu']) - mu) <= tol * mu and abs(float(got['sigma']) - sigma) <= 4 * tol * sigma
    assert float(got['threshold']) == float(got['mu']) + std_ratio * float(got['sigma'])
    m = got['mean_dist'].numpy()
    assert np.array_equal(np.isposinf(m), np.isposinf(means)) and np.allclose(m[np.isfinite(m)], np.array(means)[np.isfinite(m)], rtol=8 * 2.0 ** -52, atol=0)
    keep = got['keep'].numpy()
    assert np.array_equal(keep, m <= float(got['threshold'])) and not keep[:20].any() and not keep[np.isposinf(m)].any() and keep.mean() > 0.5
    # nothing finite anywhere: nothing is kept, and nothing raises
    none = statistical_outliers(world, 0.5, knn=dict(dist=torch.full((Q, k), float("inf"))))
    assert not bool(none['keep'].any()) and bool(torch.isnan(none['mu']))


@pytest.mark.parametrize("normals", [False, True])
def test_select_map_is_filter_maps_selection(normals):
    from super_primitive_amd.odometery.results import filter_map, select_map
    Q = 333
    world = _world(Q, 31, normals)
    counts = torch.from_numpy(np.random.default_rng(32).integers(0, 3, (Q, 3)).astype(np.int32))
    want = filter_map(world, dict(counts=counts), min_agree=1, max_in_front=1)
    got = select_map(world, (counts[:, 0] >= 1) & (counts[:, 1] <= 1))
    assert set(got) == set(want) and ('normals' in got) == normals and 0 < got['points'].shape[0] < Q
    for key, v in want.items():
        assert torch.equal(got[key], v) if torch.is_tensor(v) else np.array_equal(np.asarray(got[key]), np.asarray(v)), key
    assert got['offsets'][1] == got['offsets'][2] and got['offsets'][-1] == got['points'].shape[0] and got['ids'] == [0, 4, 9]
    assert torch.equal(got['points'], world['points'][got['kept']])
    everything, nothing = select_map(world, torch.ones(Q, dtype=torch.bool)), select_map(world, torch.zeros(Q, dtype=torch.bool))
    assert torch.equal(everything['points'], world['points']) and nothing['points'].shape[0] == 0 and not nothing['offsets'].any()


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,k", ref.RANDOM_CASES)
def test_the_two_forms_agree_on_the_random_clouds(setting, k):
    a, b = base.case_random()
    radius, origin = base.SETTINGS[setting]
    want = ref.reference_random(setting, k)
    got = ref.knn_candidates(a, b, radius, origin, k)
    assert ref.same(got, want) and np.array_equal(got['d2'], want['d2'])
    one = base.reference_random(setting)                                       # the first column is the 1-nearest answer, count is its count
    assert np.array_equal(want['index'][:, 0], one['index']) and np.array_equal(want['count'], one['count'])
    assert np.array_equal(want['dist'][:, 0].view(np.uint32), one['dist'].view(np.uint32))
    full = float((want['count'] > k).mean())
    assert 0.002 < full < 0.99
    filled = (want['index'] >= 0).sum(axis=1)
    assert np.array_equal(filled, np.minimum(want['count'], k)) and np.array_equal(want['index'] < 0, np.isposinf(want['dist']))
    d2 = want['d2']
    assert (d2[:, 1:] >= d2[:, :-1]).all()                                     # ascending, the +inf padding last


def test_the_two_forms_agree_on_the_lattice_and_on_the_cloud_against_itself():
    a, b = base.case_lattice()
    for o in base.LATTICE_ORIGINS:
        want = ref.knn(a, b, base.LATTICE_R, o, 4)
        assert ref.same(ref.knn_candidates(a, b, base.LATTICE_R, o, 4), want)
    cut = (want['count'] > 4) & (want['d2'][:, 3] == base.LATTICE_R ** 2)      # the cut falls inside a tie at exactly r: the row decides
    assert cut.sum() > 100
    p = base.case_random()[1]
    own = ref.reference_self()
    assert ref.same(ref.knn_candidates(p, p, ref.SELF_RADIUS, (0.0, 0.0, 0.0), ref.SELF_K, skip_self=True), own)
    assert own['count'].max() >= 20 and (own['count'] > 5).mean() > 0.9 and not (own['index'] == np.arange(len(p))[:, None]).any()


def test_the_normals_reference_on_a_plane_and_a_line():
    """A flat lattice plane gives +-z and curvature 0; a lattice line and coincident points give NaN; fewer than three points give NaN."""
    k = np.stack(np.meshgrid(np.arange(9), np.arange(9), indexing='ij'), axis=-1).reshape(-1, 2)
    plane = np.concatenate([k * 0.25, np.full((81, 1), 3.0)], axis=1).astype(np.float32)
    lists = ref.knn(plane, plane, 0.4, (0.0, 0.0, 0.0), 9)
    out = ref.normals(plane, plane, lists['index'])
    assert (out['used'] >= 4).all() and np.array_equal(out['normals'], np.tile([0.0, 0.0, 1.0], (81, 1))) and not out['curvature'].any()
    down = ref.normals(plane, plane, lists['index'], toward=np.zeros(3, np.float32))
    assert np.array_equal(down['normals'], np.tile([0.0, 0.0, -1.0], (81, 1)))
    line = np.stack([np.arange(20) * 0.25, np.zeros(20), np.zeros(20)], axis=1).astype(np.float32)
    out = ref.normals(line, line, ref.knn(line, line, 0.6, (0.0, 0.0, 0.0), 5)['index'])
    assert (out['used'] >= 3).all() and np.isnan(out['normals']).all() and np.isnan(out['curvature']).all()
    same = np.full((10, 3), 0.7, np.float32)
    out = ref.normals(same, same, ref.knn(same, same, 0.1, (0.0, 0.0, 0.0), 8)['index'])
    assert (out['used'] == 8).all() and np.isnan(out['normals']).all()
    out = ref.normals(plane, plane, np.array([[0, 1, -1, 81, 2 ** 31 - 1]] * 81))
    assert (out['used'] == 2).all() and np.isnan(out['normals']).all()
