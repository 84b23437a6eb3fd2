"""-m gpu: the map surfaces on the device (csrc/sp_tsdf.hip) against the NumPy restatements of tests/tsdf_ref.py and
tests/tsdf_mesh_ref.py, bit for bit: the integrate over the seeded views (whole, twice, in two calls, without colour, a partial block),
the mesh of the sphere, the holed sphere and the odd volumes (counts, capacities, every row), then ``fuse_tsdf`` / ``extract_mesh`` on a
plane seen by three cameras and ``sequence_tsdf`` on a short synthetic sequence."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_ref as ref
from gpu_util import T, dev, npy

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(got, want, what):
    got = npy(got) if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == want.dtype, what
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ, first at {np.argwhere(diff)[0].tolist()}"


# ---- integrate --------------------------------------------------------------------------------------------------------------------------------
def _fresh(case, colour=True):
    nx, ny, nz = case['dims']
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev())
    return dict(tsdf=z(nz, ny, nx), weight=z(nz, ny, nx), colour=z(nz, ny, nx, 3) if colour else None, origin=case['origin'], voxel=case['voxel'],
                trunc=case['trunc'], dims=case['dims'])


def _integrate(case, vol, views=slice(None), images=True):
    from super_primitive_amd.tool import viz
    return viz.tsdf_integrate(vol, T(case['depth'][views]), T(case['Ks'][views]), T(case['poses'][views]),
                              images=T(case['images'][views]) if images else None, z_min=case['z_min'], depth_max=case['depth_max'])


@pytest.fixture(scope="module")
def main():
    case = ref.case_main()
    return case, ref.reference(case)


def test_integrate_equals_the_reference_bit_for_bit(main):
    case, want = main
    got = _integrate(case, _fresh(case))
    for key in ('tsdf', 'weight', 'colour'):
        _same_bits(got[key], want[key], key)
    assert float(got['weight'].max()) == 2.0 and int((got['weight'] > 0).sum()) > 500
    again = _integrate(case, _fresh(case))                                     # two runs: the same bits
    for key in ('tsdf', 'weight', 'colour'):
        assert torch.equal(again[key].view(torch.int32), got[key].view(torch.int32)), key


def test_two_calls_continue_one_volume(main):
    case, want = main
    vol = _integrate(case, _fresh(case), slice(0, 1))
    first = {k: vol[k].clone() for k in ('tsdf', 'weight', 'colour')}
    for key, w in ref.reference(case, views=slice(0, 1)).items():
        _same_bits(first[key], w, f"views 0..0: {key}")
    vol = _integrate(case, vol, slice(1, 3))
    for key in ('tsdf', 'weight', 'colour'):
        _same_bits(vol[key], want[key], f"views 0..0 then 1..2: {key}")


def test_without_images_the_colour_is_left_alone(main):
    case, want = main
    vol = _fresh(case)
    vol['colour'].fill_(0.25)
    got = _integrate(case, vol, images=False)
    assert got['colour'] is vol['colour'] and bool((vol['colour'] == 0.25).all())
    _same_bits(got['tsdf'], want['tsdf'], 'tsdf')
    _same_bits(got['weight'], want['weight'], 'weight')
    plain = _integrate(case, _fresh(case, colour=False), images=False)         # a volume without colour: NULL all the way
    assert plain['colour'] is None
    _same_bits(plain['tsdf'], want['tsdf'], 'tsdf without colour')


def test_a_partial_block():
    case = ref.case_small()
    want = ref.reference(case)
    got = _integrate(case, _fresh(case))
    for key in ('tsdf', 'weight', 'colour'):
        _same_bits(got[key], want[key], key)
    assert int((got['weight'] > 0).sum()) >= 15


# ---- mesh -------------------------------------------------------------------------------------------------------------------------------------
def _device_volume(vol):
    nz, ny, nx = vol['tsdf'].shape
    return dict(tsdf=T(vol['tsdf']), weight=T(vol['weight']), colour=None if vol['colour'] is None else T(vol['colour']), origin=vol['origin'],
                voxel=vol['voxel'], trunc=4 * vol['voxel'], dims=(nx, ny, nz))


def _raw_mesh(vol, max_vertices, max_faces, rows_v, rows_f, min_weight=1.0, sentinel=-7.0):
    """One sp_tsdf_mesh call with buffers of rows_v / rows_f rows pre-filled with a sentinel and the capacities max_vertices / max_faces."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    d = _device_volume(vol)
    nx, ny, nz = d['dims']
    scratch = torch.empty(lib.sp_tsdf_mesh_scratch_bytes(nx, ny, nz) // 4, dtype=torch.int32, device=dev())
    n_out = torch.full((2,), -1, dtype=torch.int64, device=dev())
    vertices = torch.full((rows_v, 3), sentinel, dtype=torch.float32, device=dev()) if max_vertices else None
    colours = torch.full((rows_v, 3), sentinel, dtype=torch.float32, device=dev()) if max_vertices and d['colour'] is not None else None
    faces = torch.full((rows_f, 3), int(sentinel), dtype=torch.int32, device=dev()) if max_faces else None
    o = [float(np.float32(a)) for a in d['origin']]
    _lib.check(lib.sp_tsdf_mesh(_lib.ptr(d['tsdf']), _lib.ptr(d['weight']), _lib.ptr(d['colour']), nx, ny, nz, float(np.float32(d['voxel'])), o[0], o[1], o[2],
                                min_weight, _lib.ptr(scratch), max_vertices, max_faces, _lib.ptr(vertices), _lib.ptr(colours), _lib.ptr(faces),
                                _lib.ptr(n_out), _lib.stream_ptr()), "sp_tsdf_mesh")
    return dict(vertices=vertices, colours=colours, faces=faces, n_out=n_out.tolist())


@pytest.mark.parametrize("name", ["sphere", "holed", "odd", "minimum"])
def test_mesh_equals_the_reference_bit_for_bit(name):
    from super_primitive_amd.tool import viz
    vol, want = mref.reference(name)
    nv, nf = len(want['vertices']), len(want['faces'])
    assert nv > 0 and nf > 0
    counted = _raw_mesh(vol, 0, 0, 0, 0)
    assert counted['n_out'] == [nv, nf]                                        # the counting call
    got = viz.tsdf_mesh(_device_volume(vol))
    _same_bits(got['vertices'], want['vertices'], f"{name}: vertices")
    np.testing.assert_array_equal(npy(got['faces']), want['faces'])
    if want['colours'] is None:
        assert got['colours'] is None
    else:
        _same_bits(got['colours'], want['colours'], f"{name}: colours")
    # capacities one short: the last row keeps its sentinel, the rows before it are the mesh, the counts are the true ones
    short = _raw_mesh(vol, nv - 1, nf - 1, nv, nf)
    assert short['n_out'] == [nv, nf]
    _same_bits(short['vertices'][:nv - 1], want['vertices'][:nv - 1], f"{name}: vertices below the capacity")
    np.testing.assert_array_equal(npy(short['faces'][:nf - 1]), want['faces'][:nf - 1])
    assert bool((short['vertices'][nv - 1] == -7.0).all()) and bool((short['faces'][nf - 1] == -7).all())
    if want['colours'] is not None:
        assert bool((short['colours'][nv - 1] == -7.0).all())
        _same_bits(short['colours'][:nv - 1], want['colours'][:nv - 1], f"{name}: colours below the capacity")
    # vertices only
    only = _raw_mesh(vol, nv, 0, nv, 0)
    assert only['n_out'] == [nv, nf] and only['faces'] is None
    _same_bits(only['vertices'], want['vertices'], f"{name}: vertices alone")


def test_a_higher_weight_bound_and_an_empty_level_set():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    vol = mref.sphere_volume()
    vol['weight'][:, :, :6] = 1.0                                              # half the volume below the bound of 2
    want = mref.mesh(vol['tsdf'], vol['weight'], vol['colour'], vol['voxel'], vol['origin'], min_weight=2.0)
    got = viz.tsdf_mesh(_device_volume(vol), min_weight=2.0)
    assert 0 < len(want['faces']) < len(mref.reference('sphere')[1]['faces'])
    _same_bits(got['vertices'], want['vertices'], "vertices")
    np.testing.assert_array_equal(npy(got['faces']), want['faces'])
    # all positive: no vertex, no face, and the wrappers return empty tensors
    vol['tsdf'] = np.abs(vol['tsdf']) + np.float32(0.01)
    assert _raw_mesh(vol, 0, 0, 0, 0)['n_out'] == [0, 0]
    none = results.extract_mesh(_device_volume(vol))
    assert tuple(none['points'].shape) == (0, 3) and tuple(none['faces'].shape) == (0, 3) and tuple(none['colours'].shape) == (0, 3)
    assert none['offsets'].tolist() == [0, 0]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_three_cameras_fuse_a_plane_into_a_mesh_without_a_hole():
    from super_primitive_amd.odometery import results
    H, W, voxel = 48, 64, 0.05
    K = T(np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], np.float32))
    poses = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    poses[:, :3, 3] = [(-0.1, 0.0, 0.0), (0.1, 0.05, 0.0), (0.0, -0.05, 0.0)]     # fronto-parallel, looking down +z
    depths = torch.full((3, H, W), 2.0, dtype=torch.float32, device=dev())
    images = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(3)).to(dev())
    lo, hi = (-0.4, -0.3, 1.7), (0.4, 0.3, 2.3)                                    # every node of this box is inside all three images
    vol = results.fuse_tsdf(depths, K, T(poses), voxel, bounds=(lo, hi), images=images)
    nx, ny, nz = vol['dims']
    assert (nx, ny) == (16, 12) and nz in (12, 13) and vol['trunc'] == 4 * voxel
    w = npy(vol['weight'])
    pz = ref.node_centres(nz, voxel, lo[2])
    assert (w[pz <= 2.0 + vol['trunc']] == 3.0).all() and (w[pz > 2.0 + np.float64(np.float32(vol['trunc']))] == 0.0).all()
    mesh = results.extract_mesh(vol)
    v, f = npy(mesh['points']).astype(np.float64), npy(mesh['faces'])
    assert len(v) > 300 and len(f) > 500 and mesh['faces'].dtype == torch.int32
    err = np.abs(v[:, 2] - 2.0).max()
    print(f"\nplane: {len(v)} vertices, {len(f)} faces; largest |z - 2| {err:.3e}")
    assert err <= 1e-5
    # no hole: every edge has two faces with opposite directions, but for the rim, which lies in the lattice's outer faces
    px, py = ref.node_centres(nx, voxel, lo[0]), ref.node_centres(ny, voxel, lo[1])
    uses = mref.edge_uses(f)
    assert all(len(u) == 1 or sorted(u) == [-1, 1] for u in uses.values())
    rim = [e for e, u in uses.items() if len(u) == 1]
    for a, b in rim:
        on = [abs(v[a][0] - px[0]) < 1e-6 and abs(v[b][0] - px[0]) < 1e-6, abs(v[a][0] - px[-1]) < 1e-6 and abs(v[b][0] - px[-1]) < 1e-6,
              abs(v[a][1] - py[0]) < 1e-6 and abs(v[b][1] - py[0]) < 1e-6, abs(v[a][1] - py[-1]) < 1e-6 and abs(v[b][1] - py[-1]) < 1e-6]
        assert any(on), (v[a], v[b])
    assert len(v) - len(uses) + len(f) == 1                                        # a disc
    assert v[:, 0].min() == pytest.approx(px[0], abs=1e-6) and v[:, 0].max() == pytest.approx(px[-1], abs=1e-6)
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (normal[:, 2] < 0).all()                                                # towards the cameras
    c = npy(mesh['colours'])
    assert c.shape == v.shape and c.min() >= 0.0 and c.max() <= 1.0 and c.std() > 0.01
    # the mesh is a cloud: the 3D scores take it as it is
    gx, gy = np.meshgrid(np.arange(-0.375, 0.376, 0.0125), np.arange(-0.275, 0.276, 0.0125))
    plane = T(np.stack([gx.reshape(-1), gy.reshape(-1), np.full(gx.size, 2.0)], axis=1).astype(np.float32))
    scores = results.map_distance(mesh, dict(points=plane), radius=voxel)
    assert float(scores['to_reference']['dist'].max()) <= 0.0125 and int((scores['to_map']['index'] < 0).sum()) == 0
    # default bounds: the lifted depths' extent padded by trunc; the same surface comes out
    auto = results.fuse_tsdf(depths, K, T(poses), voxel, images=images)
    assert auto['origin'][2] == pytest.approx(2.0 - 4 * voxel, abs=1e-6) and auto['dims'][2] in (8, 9)
    auto_mesh = results.extract_mesh(auto)
    assert auto_mesh['points'].shape[0] > 300 and float((auto_mesh['points'][:, 2] - 2.0).abs().max()) <= 1e-5
    more = results.fuse_tsdf(depths[:1], K, T(poses[:1]), voxel, volume=auto, images=images[:1])              # continuing a volume
    assert more is auto and float(auto['weight'].max()) == 4.0


# ---- a sequence -----------------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_fuses_its_own_keyframes():
    """A 12-frame run of tests/test_gpu_sequence.py's synthetic sequence with a window of two keyframes, as
    tests/test_gpu_sequence_results.py makes its results.  The condition: the occupied nodes (weight > 0) include the voxel of at least 95 % of
    the map points inside the volume -- asked of the NumPy reference on the same depths, Ks and poses, and of the device."""
    from test_gpu_sequence import make_sequence_inputs
    from super_primitive_amd.odometery import results
    from super_primitive_amd.odometery.sequence import run_sequence
    seq, frames, to_kf = make_sequence_inputs(n=12)
    out = run_sequence(frames, to_kf, T(seq[0].T_wc), T(seq[0].kld_gt), engine="gn", keep_keyframes=True, window_size=2, translation_thresh=0.1)
    world = results.sequence_map(out, 2)
    n_kf = len(world['ids'])
    assert n_kf >= 2
    pts = npy(world['points']).astype(np.float64)
    finite = np.isfinite(pts).all(axis=1)
    voxel = float((pts[finite].max(axis=0) - pts[finite].min(axis=0)).max()) / 48.0
    vol = results.sequence_tsdf(world, out, voxel)
    nx, ny, nz = vol['dims']
    H, W = seq[0].depth.shape
    assert tuple(vol['depths'].shape) == (n_kf, H, W) and vol['trunc'] == 4 * voxel and nx * ny * nz < 400000
    # the rule alone, on the same views
    views = results._sequence_views(world, out, "test")
    images = np.stack([npy(out['kf_archive'][i]['kf'].image[:3].float()) for i in world['ids']])
    want = ref.integrate(ref.empty_volume(vol['dims']), npy(views['depths']), images, npy(views['Ks'].float()), npy(views['poses'].float()), vol['voxel'],
                         vol['origin'], vol['trunc'], 1e-6, np.inf)
    for key in ('tsdf', 'weight', 'colour'):
        _same_bits(vol[key], want[key], key)
    idx = np.floor((pts[finite] - np.array(vol['origin'])) / voxel).astype(np.int64)
    inside = ((idx >= 0) & (idx < np.array([nx, ny, nz]))).all(axis=1)
    idx = idx[inside]
    share_ref = float((want['weight'][idx[:, 2], idx[:, 1], idx[:, 0]] > 0).mean())
    share = float((npy(vol['weight'])[idx[:, 2], idx[:, 1], idx[:, 0]] > 0).mean())
    print(f"\nsequence: {n_kf} keyframes, {int(finite.sum())} map points, {int(inside.sum())} inside {nx}x{ny}x{nz} nodes of {voxel:.4f}; "
          f"their voxel is occupied for {share:.4f} (reference {share_ref:.4f}); occupied nodes {int((want['weight'] > 0).sum())}")
    assert inside.mean() > 0.99
    assert share_ref >= 0.95 and share >= 0.95
    mesh = results.extract_mesh(vol)
    assert mesh['points'].shape[0] > 1000 and mesh['faces'].shape[0] > 1000 and int(mesh['faces'].max()) < mesh['points'].shape[0]
    assert bool(torch.isfinite(mesh['points']).all())
