"""CPU-only: the ABI of the surface views (include/sp_hip.h: sp_tsdf_raycast), its argument checks -- made before any device work, so they
answer without a GPU --, the reference of tests/tsdf_raycast_ref.py against the properties the rule promises (a fronto-parallel plane at its
depth with normals (0, 0, -1); the seeded views; a hole with a rim of NaN normals; no hit from behind), and the argument checks of the
Python surface on ``meta`` tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tsdf_raycast_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")


# ---- ABI and arguments ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_matches_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    assert "sp_tsdf_raycast" in _lib.SIGNATURES
    assert "sp_tsdf_raycast" not in _lib.RESTYPES and _lib.load().sp_tsdf_raycast.restype is ctypes.c_int
    assert _lib.SP_TSDF_RAYCAST_MAX_STEPS == 1 << 20
    assert header.index("int sp_tsdf_mesh(") < header.index("int sp_tsdf_raycast(")


def test_raycast_refuses_bad_arguments_without_a_device():
    """Every case is refused before the launch: a set of arguments that passes is never sent (there may be no device, and 0x2000 is no
    buffer).  An upper limit's edge is therefore its first refused value."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(tsdf=p, weight=p, colour=p, nx=14, ny=12, nz=10, voxel=0.125, ox=0.0, oy=0.0, oz=0.0, min_weight=1.0, views=p, V=3, H=24, W=32,
              z_start=0.0, step=0.125, n_steps=25, depth=p, normals=p, image=p, index=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_tsdf_raycast(a['tsdf'], a['weight'], a['colour'], a['nx'], a['ny'], a['nz'], a['voxel'], a['ox'], a['oy'], a['oz'], a['min_weight'],
                                   a['views'], a['V'], a['H'], a['W'], a['z_start'], a['step'], a['n_steps'], a['depth'], a['normals'], a['image'],
                                   a['index'], None)
    none = dict(depth=None, normals=None, image=None, index=None)
    for bad in (dict(tsdf=None), dict(weight=None), dict(views=None), none, dict(colour=None), dict(none, colour=None, image=p),
                dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(nz=-4), dict(V=0), dict(V=-1), dict(H=0), dict(W=0), dict(W=-5),
                dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=INF), dict(voxel=NAN), dict(step=0.0), dict(step=-1.0), dict(step=INF), dict(step=NAN),
                dict(ox=INF), dict(oy=-INF), dict(oz=NAN), dict(min_weight=NAN), dict(z_start=-1e-9), dict(z_start=INF), dict(z_start=NAN),
                dict(n_steps=1), dict(n_steps=0), dict(n_steps=-3)):
        assert call(**bad) == -1, bad
    for big in (dict(V=65536), dict(V=32768, H=256, W=256), dict(V=1, H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15),
                dict(nx=1025, ny=1024, nz=1024), dict(nx=2, ny=2, nz=(1 << 28) + 1), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
                dict(nx=1 << 16, ny=1 << 16, nz=2), dict(n_steps=(1 << 20) + 1), dict(n_steps=2 ** 31 - 1)):
        assert call(**big) == -2, big
    # invalid beats too large
    assert call(V=65536, tsdf=None) == -1 and call(nx=1025, ny=1024, nz=1024, step=0.0) == -1 and call(V=1 << 20, nz=1) == -1
    assert call(n_steps=(1 << 20) + 1, **none) == -1 and call(n_steps=(1 << 20) + 1, colour=None) == -1 and call(V=65536, n_steps=1) == -1
    assert call(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=1) == -1 and call(n_steps=2 ** 31 - 1, z_start=NAN) == -1


# ---- the reference on its own ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_value, hits", [(1.7, 560), (2.05, 440)])
def test_a_fronto_parallel_plane_is_seen_at_its_depth_with_normals_towards_the_camera(depth_value, hits):
    """One identity-pose camera fuses a constant depth image; the field is then linear in z and independent of x and y.  Every node value
    carries one float32 rounding (<= 2^-24 of a value <= 1) and the slope along z is 1 / trunc; the interpolation of a linear field is exact
    up to float64 rounding, so the crossing lies within about trunc 2^-23 of the plane (the two values that bracket it, each off by 2^-24,
    over a slope of 1 / trunc), and the bound takes a factor 8 over that: trunc 2^-20.  The gradient of such a field is (0, 0, -2 voxel /
    trunc) up to the same roundings: the tsdf FALLS with z, so the normal is (0, 0, -1) -- towards the camera -- within the same bound,
    relative (the components of a unit vector)."""
    case = ref.plane_case(depth_value)
    depth, normals, image, index, counts = ref.raycast_view(case['volume'], case['K'][0], case['pose'][0], case['H'], case['W'], **ref.MAIN_STEPS)
    hit = index >= 0
    bound = case['trunc'] * 2.0 ** -20
    err = np.abs(depth[hit].astype(np.float64) - float(np.float32(depth_value)))
    print(f"\nplane at {depth_value}: {counts}; largest |depth - plane| {err.max():.3e} (bound {bound:.3e})")
    assert counts['hits'] == hits == int(hit.sum()) and hits < case['H'] * case['W']               # what a prototype of the rule gave
    assert err.max() <= bound
    assert (depth[~hit] == 0).all() and np.isnan(normals[~hit]).all() and (image[~hit] == 0).all() and (index[~hit] == -1).all()
    whole = hit & ~np.isnan(normals).any(axis=-1)
    assert int(whole.sum()) == hits - counts['nan_normals'] > 300
    n_err = np.abs(normals[whole].astype(np.float64) - np.array([0.0, 0.0, -1.0]))
    print(f"normals of {int(whole.sum())} hits with six valid samples: largest deviation from (0, 0, -1) {n_err.max():.3e}")
    assert (normals[whole][:, 2] < 0).all()                                                         # the sign: towards the camera at the origin
    assert n_err.max() <= 2.0 ** -20
    assert np.isnan(normals[hit & ~whole]).all() and (depth[hit & ~whole] > 0).all()                # a NaN normal leaves the depth alone
    # the cell behind the surface: the last sample before the plane and the first behind it lie in consecutive layers of cells
    iz = index[hit] // (14 * 12)
    assert set(np.unique(iz).tolist()) == {int(np.floor((np.ceil(depth_value / 0.125) * 0.125 - 1.0) / 0.125 - 0.5))}
    assert image[hit].std() > 10                                                                    # colours are the camera's own image, interpolated


def test_the_seeded_views_of_the_main_volume():
    case, vol = ref.main_volume()
    out = ref.raycast(vol, case['Ks'], case['poses'], case['H'], case['W'], **ref.MAIN_STEPS)
    pixels = case['H'] * case['W']
    print(f"\nmain volume: {out['counts']}")
    # the counts of this reference, as constants (a prototype of the rule gave the same hits: 451 and 279 of 768)
    assert out['counts'] == [dict(hits=451, ended_without_hit=204, nan_normals=277), dict(hits=279, ended_without_hit=300, nan_normals=227),
                             dict(hits=0, ended_without_hit=0, nan_normals=0)]
    assert all(c['hits'] + c['ended_without_hit'] <= pixels for c in out['counts'])
    away = 2                                                                                        # the view that looks away: all defaults
    assert (out['depth'][away] == 0).all() and (out['index'][away] == -1).all() and (out['image'][away] == 0).all() and np.isnan(out['normals'][away]).all()
    for v in (0, 1):
        hit = out['index'][v] >= 0
        assert (out['depth'][v][hit] > 0).all() and (out['depth'][v][~hit] == 0).all() and np.isfinite(out['depth'][v]).all()
        nrm = out['normals'][v][hit & ~np.isnan(out['normals'][v]).any(axis=-1)].astype(np.float64)
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-6
        # the plane 0.25 x + 0.125 y + z = 1.75 was seen from z < 1.75: the normals face that side
        assert (nrm @ np.array([0.25, 0.125, 1.0]) < 0).all()
        # a hit lies near the plane: its world point, from the ray, within a voxel (a sanity check, not a bound of the rule: a node takes
        # the depth of its nearest pixel, the views see the slanted plane under different angles, and their sdfs are averaged)
        r, c = np.nonzero(hit)
        p = np.stack(ref.world_points(case['Ks'][v], case['poses'][v], r, c, out['depth'][v][hit].astype(np.float64)), axis=-1)
        assert np.abs(p @ np.array([0.25, 0.125, 1.0]) - 1.75).max() < case['voxel']
    # a volume without colour: no image, everything else bit for bit
    plain = ref.raycast(ref.main_volume(colour=False)[1], case['Ks'], case['poses'], case['H'], case['W'], **ref.MAIN_STEPS)
    assert plain['image'] is None and np.array_equal(plain['depth'].view(np.uint32), out['depth'].view(np.uint32))
    assert np.array_equal(plain['index'], out['index'])


def test_every_camera_of_the_device_cases_does_what_its_name_says():
    case, vol = ref.main_volume()
    counts = {name: ref.raycast_view(vol, K, pose, case['H'], case['W'], **steps)[4] for name, (K, pose, steps) in ref.cameras().items()}
    print(f"\ncameras: {counts}")
    assert counts['away'] == dict(hits=0, ended_without_hit=0, nan_normals=0)
    assert counts['behind']['hits'] == 0 and counts['behind']['ended_without_hit'] > 700           # (d): the surface from behind is no hit
    for name in ('front', 'inside', 'oblique', 'grazing', 'far'):
        assert counts[name]['hits'] > 0 and counts[name]['ended_without_hit'] > 0, name
    assert counts['oblique']['hits'] + counts['oblique']['ended_without_hit'] < 200                 # most of its rays miss the box


def _cells_of_hits(vol, case, hit, index):
    """The eight nodes (linear indices, (hits, 8)) of the two cells a hit of the plane at 1.7 interpolates in: every such ray ends at k = 14
    (z = 1.75) after the sample at k = 13 (z = 1.625).  The first must be the cell ``index`` names."""
    nz, ny, nx = vol.tsdf.shape
    r, c = np.nonzero(hit)
    offsets = np.array([(dz * ny + dy) * nx + dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])
    out = []
    for k in (14, 13):
        ok, F, node = ref.sample(vol, ref.world_points(case['K'][0], case['pose'][0], r, c, np.float64(k) * 0.125))
        assert ok.all() and ((F < 0) if k == 14 else (F >= 0)).all()
        out.append(node[:, None] + offsets)
    assert np.array_equal(out[0][:, 0], index[hit])
    return out


def test_a_hole_has_a_rim_of_nan_normals_and_no_hit_touches_an_invalid_node():
    case, vol = ref.holed_volume()
    whole = ref.plane_case(1.7)['volume']
    assert int((vol.weight < 1.0).sum()) - int((whole.weight < 1.0).sum()) == 27
    args = (case['K'][0], case['pose'][0], case['H'], case['W'])
    depth, normals, image, index, counts = ref.raycast_view(vol, *args, **ref.MAIN_STEPS)
    d0, n0, _, i0, c0 = ref.raycast_view(whole, *args, **ref.MAIN_STEPS)
    lost = (i0 >= 0) & (index < 0)
    print(f"\nholed: {counts} (whole: {c0}); {int(lost.sum())} hits lost")
    assert 0 < int(lost.sum()) < 150 and not ((index >= 0) & (i0 < 0)).any()                        # a hole, and nothing new
    assert (depth[lost] == 0).all() and np.isnan(normals[lost]).all() and (image[lost] == 0).all()
    # no hit touches an invalid node: neither the cell of sample k (index) nor that of sample k-1
    hit = index >= 0
    for corners in _cells_of_hits(vol, case, hit, index):
        assert vol.node_ok.reshape(-1)[corners].all()
    kept = hit & (i0 >= 0)
    assert np.array_equal(depth[kept].view(np.uint32), d0[kept].view(np.uint32))                    # the depth of a surviving hit stands
    rim = kept & np.isnan(normals).any(axis=-1) & ~np.isnan(n0).any(axis=-1)
    assert int(rim.sum()) >= 8 and (depth[rim] > 0).all()                                           # the rim: a depth, but no normal


def test_nan_inf_and_light_nodes_are_holes_and_an_exact_zero_is_positive():
    case, vol = ref.odd_volume()
    whole = ref.plane_case(1.7)['volume']
    args = (case['K'][0], case['pose'][0], case['H'], case['W'])
    index = ref.raycast_view(vol, *args, **ref.MAIN_STEPS)[3]
    nz, ny, nx = vol.tsdf.shape
    for name, (iz, iy, ix) in ref.ODD.items():
        # the same volume with the node's weight set to 0 instead: the same image of holes
        weight = vol.weight.copy()
        weight[iz, iy, ix] = 0.0
        tsdf = vol.tsdf.copy()
        tsdf[iz, iy, ix] = whole.tsdf[iz, iy, ix]
        as_hole = ref.raycast_view(ref.Volume(tsdf, weight, vol.colour, vol.voxel, vol.origin), *args, **ref.MAIN_STEPS)[3]
        assert np.array_equal(as_hole >= 0, index >= 0), name
        bad = (iz * ny + iy) * nx + ix
        for corners in _cells_of_hits(vol, case, index >= 0, index):
            assert not (corners == bad).any(), name
    assert int((index >= 0).sum()) < 560
    # sampled in the planes of the nodes, the patch of exact zeros gives F = 0 exactly at z = 1.6875: positive, so the ray goes on, ends at the
    # next sample and t = 0: the depth is that plane's z, exactly
    depth, _, _, index, counts = ref.raycast_view(vol, *args, **ref.ON_NODES)
    exact = (depth == np.float32(1.6875)) & (index >= 0)
    print(f"\nodd volume sampled on its nodes: {counts}; {int(exact.sum())} hits at exactly 1.6875")
    assert int(exact.sum()) >= 4
    assert (index[exact] // (nx * ny) == 6).all()                                                   # ended by the sample in the next plane: g_z = 6 exactly


def test_the_smallest_volume_and_partial_tiles():
    vol, K, pose = ref.minimum_volume()
    depth, normals, image, index, counts = ref.raycast_view(vol, K, pose, 9, 11, 0.0, 0.0625, 30)
    assert counts['hits'] > 20 and (index[index >= 0] == 0).all() and np.isnan(normals).all()       # one cell: node 0, and no room for a gradient
    assert counts['nan_normals'] == counts['hits']


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    cpu = results.tsdf_volume((0, 0, 0), (0.5, 0.5, 0.5), 0.1, device="cpu")
    Ks, poses = torch.eye(3), torch.eye(4)[None].repeat(2, 1, 1)
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.tsdf_raycast(cpu, Ks, poses, 6, 8, 2.0)
    with pytest.raises(ValueError, match="HIP-only"):
        results.render_surface(cpu, Ks, poses, (6, 8), 2.0)
    with pytest.raises(ValueError, match="HIP-only"):
        results.score_surface(cpu, torch.ones(2, 6, 8), Ks, poses)
    with pytest.raises(ValueError, match="HIP-only"):
        results.score_surface_images(cpu, torch.ones(2, 3, 6, 8), Ks, poses, 2.0)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    vol = results.tsdf_volume((0, 0, 0), (0.5, 0.4, 0.3), 0.1, device="meta")
    plain = dict(vol, colour=None)
    K, T, d, img = _meta(2, 3, 3), _meta(2, 4, 4), _meta(2, 6, 8), _meta(2, 3, 6, 8)
    for handle in (None, {}, 3, dict(vol, dims=(5, 4)), dict(vol, tsdf=_meta(3, 4, 5, dtype=torch.float64)), dict(vol, weight=None),
                   dict(vol, colour=_meta(3, 4, 5, 3, dtype=torch.float16)), dict(vol, voxel=0.0), dict(vol, origin=(0, INF, 0))):
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            viz.tsdf_raycast(handle, K, T, 6, 8, 2.0)
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            results.render_surface(handle, K, T, (6, 8), 2.0)
        with pytest.raises(ValueError, match="volume|voxel|origin|step"):
            results.score_surface(handle, d, K, T)
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            results.score_surface_images(handle, img, K, T, 2.0)
    with pytest.raises(ValueError, match="no cell"):
        viz.tsdf_raycast(results.tsdf_volume((0, 0, 0), (0.5, 0.5, 0.05), 0.1, device="meta"), K, T, 6, 8, 2.0)
    # wrong dtypes and shapes of the views and the targets
    for bad_T in (_meta(4, 4), _meta(2, 3, 4), _meta(2, 4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses"):
            viz.tsdf_raycast(vol, K, bad_T, 6, 8, 2.0)
        with pytest.raises(ValueError, match="poses"):
            results.render_surface(vol, K, bad_T, (6, 8), 2.0)
    for bad_K in (_meta(3, 3, 3), _meta(2, 9), _meta(2, 3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="Ks"):
            viz.tsdf_raycast(vol, bad_K, T, 6, 8, 2.0)
    for depths in (_meta(2, 6, 8, dtype=torch.float64), _meta(3, 6, 8), _meta(2, 6), [[1.0]]):
        with pytest.raises(ValueError, match="gt_depths"):
            results.score_surface(vol, depths, K, T)
    for images in (_meta(2, 3, 6, 8, dtype=torch.float16), _meta(2, 4, 6, 8), _meta(3, 3, 6, 8), _meta(2, 6, 8)):
        with pytest.raises(ValueError, match="images"):
            results.score_surface_images(vol, images, K, T, 2.0)
    # V = 0
    for call in (lambda: viz.tsdf_raycast(vol, K, _meta(0, 4, 4), 6, 8, 2.0), lambda: results.render_surface(vol, K, _meta(0, 4, 4), (6, 8), 2.0),
                 lambda: results.score_surface(vol, _meta(0, 6, 8), K, _meta(0, 4, 4)),
                 lambda: results.score_surface_images(vol, _meta(0, 3, 6, 8), K, _meta(0, 4, 4), 2.0)):
        with pytest.raises(ValueError, match="poses"):
            call()
    for H, W in ((0, 8), (6, -1)):
        with pytest.raises(ValueError, match="image size"):
            viz.tsdf_raycast(vol, K, T, H, W, 2.0)
    # an image of a volume without colour: silently off by default, an error when asked for
    with pytest.raises(ValueError, match="colour"):
        viz.tsdf_raycast(plain, K, T, 6, 8, 2.0, image=True)
    with pytest.raises(ValueError, match="colour"):
        results.score_surface_images(plain, img, K, T, 2.0)
    # the depth range and the steps
    for z_min, z_max in ((1e-6, 1e-6), (0.5, 0.25), (0.0, 0.0), (0.0, INF), (0.0, NAN), (0.0, "far")):
        with pytest.raises(ValueError, match="z_max"):
            viz.tsdf_raycast(vol, K, T, 6, 8, z_max, z_min=z_min)
    for z_min in (-1.0, NAN):
        with pytest.raises(ValueError, match="z_min"):
            viz.tsdf_raycast(vol, K, T, 6, 8, 2.0, z_min=z_min)
    for step in (0.0, -0.1, INF, NAN, "fine"):
        with pytest.raises(ValueError, match="step"):
            viz.tsdf_raycast(vol, K, T, 6, 8, 2.0, step=step)
        with pytest.raises(ValueError, match="step"):
            results.score_surface(vol, d, K, T, step=step)
    with pytest.raises(ValueError, match="2\\^20"):                            # n_steps beyond the limit: 2^20 steps and one more sample
        viz.tsdf_raycast(vol, K, T, 6, 8, float(1 << 20), z_min=0.0, step=1.0)
    with pytest.raises(ValueError, match="2\\^20"):
        viz.tsdf_raycast(vol, K, T, 6, 8, 2.0, step=1e-7)
    with pytest.raises(ValueError, match="2\\^20"):
        results.score_surface(vol, d, K, T, max_depth=5.0, step=1e-6)
    for min_weight in (NAN, "heavy", None):
        with pytest.raises(ValueError, match="min_weight"):
            viz.tsdf_raycast(vol, K, T, 6, 8, 2.0, min_weight=min_weight)
    with pytest.raises(ValueError, match="no output"):
        viz.tsdf_raycast(vol, K, T, 6, 8, 2.0, depth=False, normals=False, image=False, index=False)
    with pytest.raises(ValueError, match="no output"):
        viz.tsdf_raycast(plain, K, T, 6, 8, 2.0, depth=False, normals=False, index=False)
    with pytest.raises(ValueError, match="limits"):
        viz.tsdf_raycast(vol, K, T, 1 << 15, 1 << 15, 2.0)
    with pytest.raises(ValueError, match="depth range"):
        results.score_surface(vol, d, K, T, min_depth=3.0, max_depth=2.0)


def test_the_largest_allowed_march_reaches_the_library(monkeypatch):
    """n_steps = 2^20 is allowed: ceil((z_max - z_min) / step) = 2^20 - 1."""
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    seen = {}

    class Lib:
        def sp_tsdf_raycast(self, *args):
            seen['n_steps'], seen['outputs'] = args[17], [a is not None for a in args[18:22]]
            return 0
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else 1)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    vol = results.tsdf_volume((0, 0, 0), (0.5, 0.4, 0.3), 0.1, device="meta")
    K, T = _meta(3, 3), _meta(2, 4, 4)
    out = viz.tsdf_raycast(vol, K, T, 6, 8, float((1 << 20) - 1), z_min=0.0, step=1.0)
    assert seen == dict(n_steps=1 << 20, outputs=[True] * 4) and set(out) == {'depth', 'normals', 'image', 'index'}
    assert tuple(out['normals'].shape) == (2, 6, 8, 3) and out['image'].dtype == torch.uint8 and out['index'].dtype == torch.int32
    out = viz.tsdf_raycast(dict(vol, colour=None), K, T, 6, 8, 1.0, z_min=0.5, step=0.25, normals=False)        # the image: silently off
    assert seen == dict(n_steps=3, outputs=[True, False, False, True]) and set(out) == {'depth', 'index'}
    viz.tsdf_raycast(vol, K, T, 6, 8, 0.95, z_min=0.5)                                                         # the step defaults to the voxel
    assert seen['n_steps'] == int(np.ceil((0.95 - 0.5) / float(np.float32(0.1)))) + 1 == 6
    surface = results.render_surface(dict(vol, colour=None), K, T, (6, 8), 1.0)
    assert set(surface) == {'depth', 'normals', 'image', 'index'} and tuple(surface['image'].shape) == (2, 6, 8, 3)
