"""CPU-only: the float64 reference of the map registration (tests/cloud_register_ref.py) against transforms it must recover, the ABI of
``sp_cloud_register`` (include/sp_hip.h) -- symbols, the size of ``SpCloudReg``, the ABI version --, every argument check of the
entry points (made before any device work, so they answer without a GPU), the argument checks of the Python surface (``tool/viz.py``
``register_clouds``, ``odometery/results.py`` ``register_map``) and ``transform_map`` on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_register_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_the_reference_recovers_a_known_similarity_from_identical_points(kind):
    """2003 rows of the 3001 reference samples, moved back by TRUTH (|omega| about 0.04, |t| about 0.05, s = 1.02) and rounded to
    float32, from the identity.  A query row is off its twin by at most e = 2^-24 max|coordinate| per coordinate, and the estimate
    averages the rows: t and s within e, the rotation within e over the cloud's RMS radius.  Measured: point to point 22 iterations, rotation
    7e-10, translation 2e-9; the plane kinds 5 iterations, rotation 1e-8, translation 4e-8, scale 2e-8."""
    a, an, b, bn = ref.case_identical()
    out = ref.check_gap(ref.run(a, an, b, bn, kind, True, tol=1e-10, max_iters=40))
    e = 2.0 ** -24 * float(np.abs(b).max())
    radius = float(np.sqrt((b.astype(np.float64) ** 2).sum(axis=1).mean()))
    rot, trans, scale = ref.rotation_angle(out['R'], ref.TRUTH['R']), float(np.abs(out['t'] - ref.TRUTH['t']).max()), abs(out['s'] - ref.TRUTH['s'])
    print(f"\nkind {kind}: {out['iterations']} iterations, rotation {rot:.2e} (bound {e / radius:.2e}), translation {trans:.2e}, scale {scale:.2e} (bound {e:.2e}), "
          f"smallest margin of a correspondence {out['gap']:.2e}, cond(H) {out['cond']:.0f}")
    assert out['status'] == ref.CONVERGED and out['n'] == len(a) and out['iterations'] <= (25 if kind == 0 else 6)
    assert np.array_equal(out['index'], np.arange(len(a)))                     # every row ends on its twin
    assert rot <= e / radius and trans <= e and scale <= e
    hist = out['history']
    assert (hist[:out['iterations'] - 1, 3] == ref.RUNNING).all() and (hist[out['iterations'] - 1:, 3] == ref.CONVERGED).all()
    assert not hist[out['iterations']:, :3].any() and hist[out['iterations'] - 1, 2] <= 1e-10


@pytest.mark.parametrize("kind", [1, 2])
def test_the_reference_on_independent_samples(kind):
    """Independent samples of one surface: the plane kinds reach a step below 1e-9 within 6 iterations, H is well conditioned, and the
    same sums taken in reversed row order move the result by a few ulps only."""
    a, an, b, bn = ref.case_independent()
    out = ref.check_gap(ref.run(a, an, b, bn, kind, True, tol=1e-9, max_iters=40))
    back = ref.run(a, an, b, bn, kind, True, tol=1e-9, max_iters=40, reverse=True)
    print(f"\nkind {kind}: {out['iterations']} iterations, cond(H) {out['cond']:.0f}, reversed sums move the result by {ref.difference(out, back):.2e}")
    assert out['status'] == ref.CONVERGED and out['iterations'] <= 6 and out['cond'] <= 1e4
    assert ref.difference(out, back) <= 1e-12 and back['iterations'] == out['iterations']
    assert float(np.abs(out['t'] - ref.TRUTH['t']).max()) < 2e-3 and abs(out['s'] - ref.TRUTH['s']) < 2e-3       # (the sampling's own error)


def test_the_reference_stops():
    a, an, b, bn = ref.case_lattice()
    flat = ref.run(a, an, b, bn, 1, False, max_iters=5)
    assert flat['status'] == ref.DEGENERATE and flat['iterations'] == 1 and np.array_equal(flat['R'], np.eye(3)) and not flat['t'].any()
    H = flat['first']['H']
    assert not H[2].any() and not H[3].any() and not H[4].any() and H[0, 0] > 0 and H[5, 5] > 0          # exact zero columns
    assert ref.run(a, an, b, bn, 0, True, max_iters=30, tol=1e-9)['status'] == ref.CONVERGED             # point to point pins the lattice
    far = ref.run(a + np.float32(1.0), an, b, bn, 0, False, max_iters=3)
    assert far['status'] == ref.FEW and far['n'] == 0 and (far['index'] == -1).all() and (far['history'][:, 3] == ref.FEW).all()


@pytest.mark.parametrize("kind", [1, 2])
def test_huber_in_the_reference_ends_closer_to_the_truth(kind):
    """Every 20th query displaced by 0.2 along z, a rigid fit: measured translation error 1.0e-2 without and 1.1e-3 with huber = 0.02."""
    a, an, b, bn = ref.case_outliers()
    plain = ref.run(a, an, b, bn, kind, False, tol=1e-9, max_iters=40)
    robust = ref.check_gap(ref.run(a, an, b, bn, kind, False, huber=0.02, tol=1e-9, max_iters=40))
    err = lambda o: float(np.abs(o['t'] - ref.TRUTH['t']).max())
    print(f"\nkind {kind}: translation error without huber {err(plain):.2e}, with huber 0.02 {err(robust):.2e}")
    assert robust['status'] == ref.CONVERGED and err(robust) < 0.2 * err(plain)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_size_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for name in ("sp_cloud_register_work_doubles", "sp_cloud_register"):
        assert name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.SpCloudReg) % 64 == 0
    assert "sizeof(SpCloudReg) % 64 == 0" in header and "TWO RUNS GIVE THE SAME BITS" in header
    for k, name in enumerate(("RUNNING", "CONVERGED", "MAX_ITERS", "FEW", "DEGENERATE")):
        assert getattr(_lib, "SP_CLOUD_REG_" + name) == k == getattr(ref, name)
    assert _lib.SP_CLOUD_REG_WORK_DOUBLES == 40
    assert float(re.search(r"#define\s+SP_CLOUD_REG_SMALL_ANGLE2\s+(\S+)", header).group(1)) == ref.SMALL_ANGLE2


def test_every_argument_check_answers_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    assert lib.sp_cloud_register_work_doubles(0) == -1 and lib.sp_cloud_register_work_doubles(-7) == -1
    assert lib.sp_cloud_register_work_doubles(2 ** 31 - 1) == -2
    assert lib.sp_cloud_register_work_doubles(1) == 40 and lib.sp_cloud_register_work_doubles(256) == 40 and lib.sp_cloud_register_work_doubles(257) == 80
    assert lib.sp_cloud_register_work_doubles(70001) == 40 * 274 and 0 < lib.sp_cloud_register_work_doubles(2 ** 31 - 2) < 2 ** 31
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(queries=p, normals=p, Qa=100, Q=100, scratch=p, residual=1, with_scale=1, huber=0.0, tol=1e-6, min_pairs=7, max_iters=3, state=p,
              history=p, index=p, work=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_cloud_register(a['queries'], a['normals'], a['Qa'], a['Q'], a['scratch'], a['residual'], a['with_scale'], a['huber'], a['tol'],
                                     a['min_pairs'], a['max_iters'], a['state'], a['history'], a['index'], a['work'], None)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(queries=None), dict(scratch=None), dict(state=None), dict(history=None), dict(index=None), dict(work=None),
                dict(residual=-1), dict(residual=3), dict(normals=None), dict(normals=None, residual=2), dict(with_scale=2), dict(with_scale=-1),
                dict(huber=-1.0), dict(huber=inf), dict(huber=nan), dict(tol=-1e-9), dict(tol=inf), dict(tol=nan),
                dict(min_pairs=6), dict(min_pairs=5, with_scale=0), dict(min_pairs=0), dict(min_pairs=-3), dict(max_iters=0), dict(max_iters=-2),
                dict(Q=0), dict(Q=-1), dict(Qa=0), dict(Qa=-5), dict(scratch=ctypes.c_void_p(0x2008)), dict(state=ctypes.c_void_p(0x2004)),
                dict(history=ctypes.c_void_p(0x2004)), dict(work=ctypes.c_void_p(0x2008))):
        assert call(**bad) == -1, bad
    for big in (dict(Q=(1 << 28) + 1), dict(Qa=2 ** 31 - 1), dict(Qa=1 << 40), dict(max_iters=4097)):
        assert call(**big) == -2, big
    for both in (dict(Q=1 << 40, residual=3), dict(Qa=1 << 40, index=None), dict(max_iters=10 ** 6, tol=nan), dict(Q=1 << 40, min_pairs=6)):
        assert call(**both) == -1, both                            # invalid beats too large


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    cpu_grid = dict(scratch=torch.zeros(8, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0, 0, 0), points=torch.zeros(5, 3))
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.register_clouds(torch.zeros(4, 3), cpu_grid)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts = _meta(5, 3)
    grid = dict(scratch=_meta(5, 8, dtype=torch.int64), Q=5, radius=0.1, origin=(0.0, 0.0, 0.0), points=pts)
    for handle in (None, {}, dict(grid, Q=6), dict(grid, Q=0), dict(grid, points=_meta(7, 3)), dict(grid, scratch=None),
                   {k: v for k, v in grid.items() if k != 'radius'}):
        with pytest.raises(ValueError, match="grid"):                          # a handle of the wrong size, or no handle
            viz.register_clouds(_meta(4, 3), handle)
    for bad in (_meta(4, 2), _meta(4, 3, dtype=torch.float16), _meta(0, 3)):
        with pytest.raises(ValueError):
            viz.register_clouds(bad, grid)
    with pytest.raises(ValueError, match="residual"):
        viz.register_clouds(_meta(4, 3), grid, residual='planes')
    for residual in ('plane', 'query_plane'):
        with pytest.raises(ValueError, match="needs normals"):
            viz.register_clouds(_meta(4, 3), grid, residual=residual)
    with pytest.raises(ValueError, match="grid point"):
        viz.register_clouds(_meta(4, 3), grid, normals=_meta(4, 3), residual='plane')          # one row per GRID point
    with pytest.raises(ValueError, match="query"):
        viz.register_clouds(_meta(4, 3), grid, normals=_meta(5, 3), residual='query_plane')    # one row per QUERY
    for kw in (dict(huber=-1.0), dict(huber=float("nan")), dict(tol=float("inf")), dict(tol=-1.0), dict(s0=0.0), dict(s0=float("nan")), dict(min_pairs=5),
               dict(min_pairs=6, scale=True), dict(max_iters=0), dict(max_iters=4097), dict(tol="tight"), dict(T0=torch.eye(3))):
        with pytest.raises(ValueError):
            viz.register_clouds(_meta(4, 3), grid, **kw)
    world = dict(points=pts, colours=_meta(5, 3), kf_index=_meta(5, dtype=torch.int32), seg_ids=_meta(5, dtype=torch.int32), offsets=np.array([0, 5]))
    with pytest.raises(ValueError, match="world"):
        results.register_map({k: v for k, v in world.items() if k != 'seg_ids'}, _meta(9, 3), 0.1)
    with pytest.raises(ValueError, match="reference"):
        results.register_map(world, dict(colours=pts), 0.1)
    with pytest.raises(ValueError, match="normals of the reference"):
        results.register_map(world, _meta(9, 3), 0.1, residual='plane')
    with pytest.raises(ValueError, match="normals of the map"):
        results.register_map(world, dict(points=_meta(9, 3), normals=_meta(9, 3)), 0.1, residual='query_plane')
    with pytest.raises(ValueError, match="radius"):
        results.register_map(world, _meta(9, 3), 0.0)


def test_transform_map_on_cpu_tensors():
    from super_primitive_amd.odometery.results import transform_map
    p, n = ref.samples(301, 9)
    world = dict(points=torch.from_numpy(p.copy()), normals=torch.from_numpy(n.copy()), colours=torch.zeros(301, 3), ids=[3], offsets=np.array([0, 301]))
    R, t, s = ref.TRUTH['R'], ref.TRUTH['t'], ref.TRUTH['s']
    out = transform_map(world, torch.from_numpy(R), torch.from_numpy(t), torch.tensor(s, dtype=torch.float64))
    assert out is not world and set(out) == set(world) and out['colours'] is world['colours'] and out['ids'] is world['ids']
    assert np.array_equal(out['points'].numpy().view(np.uint32), ref.move(p, R, t, s).astype(np.float32).view(np.uint32))     # float64, rounded once
    assert np.array_equal(out['normals'].numpy().view(np.uint32), ref.move(n, R, np.zeros(3), 1.0).astype(np.float32).view(np.uint32))
    assert np.array_equal(world['points'].numpy(), p) and np.array_equal(world['normals'].numpy(), n)                         # the input is untouched
    plain = transform_map(dict(points=world['points']), R.tolist(), t.tolist())                # numbers, no normals, s = 1
    assert set(plain) == {'points'} and np.array_equal(plain['points'].numpy(), ref.move(p, R, t, 1.0).astype(np.float32))
    for bad in (dict(points=world['points'].double()), dict(points=world['points'][:, :2]), dict(), None, dict(points=world['points'], normals=world['normals'][:5])):
        with pytest.raises(ValueError):
            transform_map(bad, R, t)
    for rot, trans, sc in ((np.eye(4), t, 1.0), (R, np.zeros(2), 1.0), (R, t, [1.0, 2.0])):
        with pytest.raises(ValueError):
            transform_map(world, rot, trans, sc)
