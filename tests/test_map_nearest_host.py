"""CPU-only: the ABI of the map distances (include/sp_hip.h: sp_cloud_grid_scratch_units, sp_cloud_grid_build, sp_cloud_grid_nearest),
their argument checks -- made before any device work, so they answer without a GPU --, the argument checks of the Python surface
(``tool/viz.py`` ``cloud_grid`` / ``nearest_points``, ``odometery/results.py`` ``map_distance`` / ``map_neighbours``), ``cloud_metrics``
on CPU tensors against a float64 loop, and the reference of tests/map_nearest_ref.py against itself: its three forms agree."""
import ctypes
import os

import numpy as np
import pytest
import torch

import map_nearest_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for name in ("sp_cloud_grid_scratch_units", "sp_cloud_grid_build", "sp_cloud_grid_nearest"):
        assert name in _lib.SIGNATURES, name
    assert "1.0009765625" in header and "lowest row wins" in header and "Why the search is local" in header
    assert _lib.SP_CLOUD_GRID_MAX_POINTS == 1 << 28


def test_scratch_units_and_build_refuse_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    assert lib.sp_cloud_grid_scratch_units(0) == -1 and lib.sp_cloud_grid_scratch_units(-5) == -1
    assert lib.sp_cloud_grid_scratch_units((1 << 28) + 1) == -2
    # header | S slots of 16 bytes | Q records of 16 bytes | Q int32 | ceil(S / 256) int32, each a whole number of 64-byte units
    assert lib.sp_cloud_grid_scratch_units(1) == 1 + 1 + 1 + 1 + 1
    assert lib.sp_cloud_grid_scratch_units(3001) == 1 + 8192 // 4 + 751 + 188 + 2
    assert 0 < lib.sp_cloud_grid_scratch_units(1 << 28) < 2 ** 31
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(points=p, Q=10, radius=0.25, ox=0.0, oy=0.0, oz=0.0, scratch=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_cloud_grid_build(a['points'], a['Q'], a['radius'], a['ox'], a['oy'], a['oz'], a['scratch'], None)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(points=None), dict(scratch=None), dict(scratch=ctypes.c_void_p(0x2008)), dict(Q=0), dict(Q=-1), dict(radius=0.0), dict(radius=-1.0),
                dict(radius=inf), dict(radius=nan), dict(radius=1e39), dict(ox=inf), dict(oy=nan), dict(oz=-inf)):
        assert call(**bad) == -1, bad
    assert call(Q=(1 << 28) + 1) == -2
    assert call(Q=1 << 40, radius=0.0) == -1 and call(Q=1 << 40, points=None) == -1  # invalid beats too large


def test_nearest_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(queries=p, Qa=10, Q=10, scratch=p, skip_self=0, index=p, dist=p, count=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_cloud_grid_nearest(a['queries'], a['Qa'], a['Q'], a['scratch'], a['skip_self'], a['index'], a['dist'], a['count'], None)
    for bad in (dict(queries=None), dict(scratch=None), dict(scratch=ctypes.c_void_p(0x2004)), dict(index=None), dict(dist=None), dict(count=None),
                dict(Qa=0), dict(Qa=-3), dict(Q=0), dict(Q=-1), dict(skip_self=2), dict(skip_self=-1), dict(skip_self=1, Qa=11), dict(skip_self=1, Q=9)):
        assert call(**bad) == -1, bad
    for big in (dict(Q=(1 << 28) + 1), dict(Qa=2 ** 31 - 1), dict(Qa=1 << 40)):
        assert call(**big) == -2, big
    assert call(Qa=1 << 40, skip_self=1) == -1 and call(Q=1 << 40, index=None) == -1 and call(Qa=1 << 40, skip_self=3) == -1   # invalid beats too large


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.cloud_grid(torch.zeros(5, 3), 0.1)
    with pytest.raises(ValueError, match="HIP-only"):
        viz.nearest_points(torch.zeros(5, 3), dict(scratch=torch.zeros(8, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0, 0, 0), points=torch.zeros(5, 3)))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts = _meta(5, 3)
    for bad in (_meta(5, 2), _meta(5), _meta(5, 3, dtype=torch.float64), _meta(0, 3), [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            viz.cloud_grid(bad, 0.1)
    with pytest.raises(ValueError, match="no points"):
        viz.cloud_grid(_meta(0, 3), 0.1)
    for radius in (0.0, -1.0, float("inf"), float("nan"), 1e39, "wide", None):
        with pytest.raises(ValueError, match="radius"):
            viz.cloud_grid(pts, radius)
    for origin in ((0.0, 0.0), (0.0, 0.0, float("inf")), (float("nan"), 0.0, 0.0), "here", (0.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="origin"):
            viz.cloud_grid(pts, 0.1, origin)
    grid = dict(scratch=_meta(5, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0.0, 0.0, 0.0), points=pts)
    for bad in (_meta(4, 2), _meta(4, 3, dtype=torch.float16), _meta(0, 3)):
        with pytest.raises(ValueError):
            viz.nearest_points(bad, grid)
    with pytest.raises(ValueError, match="skip_self"):
        viz.nearest_points(_meta(4, 3), grid, skip_self=True)                  # not the grid's cloud
    for handle in (None, {}, dict(grid, Q=6), dict(grid, Q=0), dict(grid, points=_meta(7, 3)), dict(grid, scratch=None),
                   {k: v for k, v in grid.items() if k != 'radius'}):
        with pytest.raises(ValueError, match="grid"):                          # a handle of the wrong size, or no handle
            viz.nearest_points(_meta(4, 3), handle)
    world = dict(points=pts, colours=_meta(5, 3), kf_index=_meta(5, dtype=torch.int32), seg_ids=_meta(5, dtype=torch.int32), offsets=np.array([0, 5]))
    with pytest.raises(ValueError, match="threshold"):
        results.map_distance(world, _meta(9, 3), 0.1, threshold=0.2)           # the search would not have seen such neighbours
    with pytest.raises(ValueError, match="radius"):
        results.map_distance(world, _meta(9, 3), 0.0)
    with pytest.raises(ValueError, match="reference"):
        results.map_distance(world, dict(colours=pts), 0.1)
    with pytest.raises(ValueError, match="no points"):
        results.map_distance(world, dict(points=_meta(0, 3)), 0.1)
    with pytest.raises(ValueError):
        results.map_distance(world, _meta(9, 3, dtype=torch.float64), 0.1)
    with pytest.raises(ValueError, match="world"):
        results.map_distance({k: v for k, v in world.items() if k != 'seg_ids'}, _meta(9, 3), 0.1)
    with pytest.raises(ValueError, match="world"):
        results.map_neighbours(dict(points=pts), 0.1)
    with pytest.raises(ValueError, match="radius"):
        results.map_neighbours(world, -0.1)


# ---- cloud_metrics ------------------------------------------------------------------------------------------------------------------------
def _distances(n, seed, radius, none_share):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.0, radius, n).astype(np.float32)
    d[rng.uniform(size=n) < none_share] = np.inf
    d[:3] = (0.0, np.float32(radius), np.float32(0.05))                        # on the radius, and on the threshold
    return d


@pytest.mark.parametrize("none_share", [0.0, 0.2])
def test_cloud_metrics_against_a_float64_loop(none_share):
    from super_primitive_amd.odometery.results import cloud_metrics
    radius, threshold = 0.1, float(np.float32(0.05))
    a, b = _distances(4001, 11, radius, none_share), _distances(1777, 12, radius, none_share / 2)
    got = cloud_metrics(torch.from_numpy(a), torch.from_numpy(b), radius, threshold)
    want = ref.metrics(a, b, radius, threshold)
    assert set(got) == set(want) and all(torch.is_tensor(v) and v.dim() == 0 for v in got.values())
    for key in ('n_a', 'n_b', 'found_a', 'found_b', 'within_a', 'within_b'):
        assert got[key].dtype == torch.int64 and int(got[key]) == want[key], key
    assert want['within_a'] >= 2 and (none_share == 0) == (want['found_a'] == want['n_a'])
    for key, n in (('accuracy', len(a)), ('completion', len(b)), ('accuracy_clipped', len(a)), ('completion_clipped', len(b)), ('chamfer', len(a) + len(b))):
        assert got[key].dtype == torch.float64
        assert abs(float(got[key]) - want[key]) <= n * 2.0 ** -52 * want[key], key   # a reordered float64 sum of n non-negative terms
    for key in ('precision', 'recall', 'fscore'):
        assert got[key].dtype == torch.float64 and abs(float(got[key]) - want[key]) <= 4 * 2.0 ** -52 * want[key], key
    assert float(got['completion_clipped']) >= float(got['completion']) * (1 - 1e-12) or none_share == 0


def test_cloud_metrics_edges():
    from super_primitive_amd.odometery.results import cloud_metrics
    d = torch.tensor([0.01, 0.02, float("inf")])
    with pytest.raises(ValueError, match="threshold"):
        cloud_metrics(d, d, 0.1, 0.2)
    for bad in (d.double(), d[:0], d[None], [0.1]):
        with pytest.raises(ValueError):
            cloud_metrics(bad, d, 0.1, 0.05)
    nothing = torch.full((4,), float("inf"))
    out = cloud_metrics(nothing, d, 0.5, 0.5)
    assert int(out['found_a']) == 0 and bool(torch.isnan(out['accuracy'])) and float(out['accuracy_clipped']) == 0.5
    assert float(out['precision']) == 0.0 and float(out['recall']) == 2 / 3 and float(out['fscore']) == 0.0
    out = cloud_metrics(nothing, nothing, 0.5, 0.5)
    assert float(out['fscore']) == 0.0 and int(out['within_b']) == 0


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", range(len(ref.SETTINGS)))
def test_the_forms_of_the_reference_agree_on_the_random_clouds(setting):
    a, b = ref.case_random()
    radius, origin = ref.SETTINGS[setting]
    want = ref.reference_random(setting)
    none = float((want['index'] < 0).mean())
    assert 0.01 < none < 0.9 and want['count'].max() >= 3
    for form in (ref.nearest_candidates, ref.nearest_cells):
        got = form(a, b, radius, origin)
        assert ref.same(got, want) and np.array_equal(got['d2'], want['d2']), form.__name__
    for bad in ref.BAD_ROWS:                                                   # never found, and as queries "none"
        assert want['index'][bad] == -1 and want['count'][bad] == 0 and np.isposinf(want['dist'][bad]) and not (want['index'] == bad).any()


@pytest.mark.parametrize("origin", range(len(ref.LATTICE_ORIGINS)))
def test_the_cell_walk_equals_all_pairs_on_the_lattice(origin):
    """Distances of exactly r, duplicated rows: the 27 cells hold every neighbour, whatever the origin."""
    a, b = ref.case_lattice()
    o = ref.LATTICE_ORIGINS[origin]
    want = ref.nearest(a, b, ref.LATTICE_R, o)
    for form in (ref.nearest_cells, ref.nearest_candidates):
        got = form(a, b, ref.LATTICE_R, o)
        assert ref.same(got, want) and np.array_equal(got['d2'], want['d2']), form.__name__
    assert (want['count'] > 1).sum() > 1000 and 0 < (want['index'] < 0).sum() < 150
    assert (want['d2'] == ref.LATTICE_R ** 2).sum() > 10                       # winners at exactly r
    twins = want['index'][want['index'] >= 0]
    assert (twins < 12 ** 3).all()                                             # a repeated row loses the tie to its original


def test_skip_self_in_the_reference():
    p = ref.case_self()
    radius, origin = ref.SETTINGS[0]
    plain, other = ref.nearest(p, p, radius, origin), ref.nearest(p, p, radius, origin, skip_self=True)
    assert other['index'][50] == 100 and other['index'][100] == 50 and other['dist'][50] == 0.0
    assert not (other['index'] == np.arange(len(p))).any()
    ok = plain['count'] > 0
    assert np.array_equal(other['count'][ok], plain['count'][ok] - 1) and not other['count'][~ok].any()
    assert ref.same(ref.nearest_candidates(p, p, radius, origin, skip_self=True), other)
