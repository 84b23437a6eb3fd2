"""CPU-only: the ABI of the map surfaces (include/sp_hip.h: sp_tsdf_integrate, sp_tsdf_mesh, sp_tsdf_mesh_scratch_bytes), their argument
checks -- made before any device work, so they answer without a GPU --, the two references of tests/tsdf_ref.py and tests/tsdf_mesh_ref.py
against the properties the rule promises (a closed, outward-facing sphere; a hole with a clean rim; chunked views), ``write_ply`` with
faces, and the argument checks of the Python surface on ``meta`` tensors."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as mref
import tsdf_ref as ref

INF = float("inf")
NAN = float("nan")


# ---- ABI and arguments ----------------------------------------------------------------------------------------------------------------------
def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    for name in ("sp_tsdf_integrate", "sp_tsdf_mesh", "sp_tsdf_mesh_scratch_bytes"):
        assert name in _lib.SIGNATURES, name
    assert _lib.RESTYPES["sp_tsdf_mesh_scratch_bytes"] is ctypes.c_longlong       # the one 64-bit return: 4.1 GiB at the node limit
    assert _lib.load().sp_tsdf_mesh_scratch_bytes.restype is ctypes.c_longlong and _lib.load().sp_tsdf_mesh.restype is ctypes.c_int
    assert _lib.SP_TSDF_MAX_NODES == 1 << 30


def test_scratch_bytes_answers_every_size_on_the_host():
    from super_primitive_amd import _lib
    size = _lib.load().sp_tsdf_mesh_scratch_bytes
    assert size(2, 2, 2) == 3 * 64                                             # 8 words, one block of nodes, one of cells: a unit each
    assert size(12, 11, 10) == 64 * (-(-1320 // 16) + 1 + 1)
    for bad in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (0, 5, 5), (-3, 5, 5), (5, 5, -1)):
        assert size(*bad) == -1, bad
    at_limit = size(1024, 1024, 1024)                                          # 2^30 nodes: allowed, and beyond 32 bits
    blocks = (1 << 30) // 256
    cell_blocks = -(-(1023 ** 3) // 256)
    assert at_limit == 64 * ((1 << 30) // 16 + blocks // 16 + -(-cell_blocks // 16)) and at_limit > 2 ** 32
    assert at_limit <= 4 * (1 << 30) * (1 + 2 / 256) + 256                     # the bound include/sp_hip.h states
    assert size(2, 2, 1 << 28) > 0
    for big in ((1025, 1024, 1024), (2, 2, (1 << 28) + 1), (1 << 16, 1 << 16, 2), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert size(*big) == -2, big
    assert size(1, 1 << 20, 1 << 20) == -1 and size(2 ** 31 - 1, 2 ** 31 - 1, 0) == -1                            # invalid beats too large


def test_integrate_refuses_bad_arguments_without_a_device():
    """Every case is refused before the launch: a set of arguments that passes is never sent (there may be no device, and 0x2000 is no
    buffer).  An upper limit's edge is therefore its first refused value."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(depth=p, images=None, views=p, V=3, H=24, W=32, nx=14, ny=12, nz=10, voxel=0.125, ox=0.0, oy=0.0, oz=0.0, trunc=0.5, z_min=0.0,
              depth_max=INF, tsdf=p, weight=p, colour=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_tsdf_integrate(a['depth'], a['images'], a['views'], a['V'], a['H'], a['W'], a['nx'], a['ny'], a['nz'], a['voxel'], a['ox'], a['oy'],
                                     a['oz'], a['trunc'], a['z_min'], a['depth_max'], a['tsdf'], a['weight'], a['colour'], None)
    for bad in (dict(depth=None), dict(views=None), dict(tsdf=None), dict(weight=None), dict(images=p), dict(colour=p),
                dict(V=0), dict(V=-1), dict(H=0), dict(W=0), dict(W=-5), dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=-2),
                dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=INF), dict(voxel=NAN), dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=INF), dict(trunc=NAN),
                dict(z_min=-1e-9), dict(z_min=NAN), dict(depth_max=0.0), dict(depth_max=-1.0), dict(depth_max=NAN),
                dict(ox=INF), dict(oy=-INF), dict(oz=NAN)):
        assert call(**bad) == -1, bad
    for big in (dict(V=65536), dict(V=32768, H=256, W=256), dict(V=1, H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15),
                dict(nx=(1 << 30) + 1, ny=1, nz=1), dict(nx=1025, ny=1024, nz=1024), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
                dict(nx=1 << 16, ny=1 << 16, nz=1)):
        assert call(**big) == -2, big
    # invalid beats too large
    assert call(V=65536, tsdf=None) == -1 and call(nx=1025, ny=1024, nz=1024, trunc=0.0) == -1 and call(V=1 << 20, nz=0) == -1
    assert call(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=0) == -1 and call(V=65536, images=p) == -1


def test_mesh_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(tsdf=p, weight=p, colour=p, nx=12, ny=11, nz=10, voxel=0.05, ox=0.0, oy=0.0, oz=0.0, min_weight=1.0, scratch=p, max_vertices=100,
              max_faces=200, vertices=p, vertex_colours=p, faces=p, n_out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_tsdf_mesh(a['tsdf'], a['weight'], a['colour'], a['nx'], a['ny'], a['nz'], a['voxel'], a['ox'], a['oy'], a['oz'], a['min_weight'],
                                a['scratch'], a['max_vertices'], a['max_faces'], a['vertices'], a['vertex_colours'], a['faces'], a['n_out'], None)
    counting = dict(max_vertices=0, max_faces=0, vertices=None, vertex_colours=None, faces=None)
    for bad in (dict(tsdf=None), dict(weight=None), dict(scratch=None), dict(n_out=None), dict(scratch=ctypes.c_void_p(0x2002)),
                dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(nz=-4), dict(max_vertices=-1), dict(max_faces=-1),
                dict(vertices=None), dict(faces=None), dict(vertex_colours=None),                           # NULL with a capacity > 0
                dict(max_vertices=0), dict(max_faces=0),                                                    # a buffer with capacity 0
                dict(max_vertices=0, vertices=None), dict(counting, vertices=p), dict(counting, faces=p), dict(counting, vertex_colours=p),
                dict(colour=None), dict(colour=None, vertex_colours=p, max_vertices=0, vertices=None),      # colours of a volume without colour
                dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=INF), dict(voxel=NAN), dict(ox=INF), dict(oy=NAN), dict(oz=-INF), dict(min_weight=NAN),
                dict(counting, nx=1), dict(counting, tsdf=None), dict(counting, n_out=None)):
        assert call(**bad) == -1, bad
    for big in (dict(nx=1025, ny=1024, nz=1024), dict(nx=2, ny=2, nz=(1 << 28) + 1), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1),
                dict(max_vertices=2 ** 31), dict(max_faces=2 ** 31), dict(max_faces=1 << 40), dict(counting, nx=1 << 16, ny=1 << 16, nz=2)):
        assert call(**big) == -2, big
    # invalid beats too large
    assert call(nx=1025, ny=1024, nz=1024, n_out=None) == -1 and call(max_vertices=2 ** 31, vertices=None) == -1
    assert call(nx=1, ny=1 << 20, nz=1 << 20) == -1 and call(max_faces=1 << 40, voxel=0.0) == -1


# ---- the mesh reference on its own ----------------------------------------------------------------------------------------------------------
def test_the_orientation_table_mirrors_under_a_swap_of_all_signs():
    table = mref.orientation_table()
    assert table == mref.orientation_table(12, 11) == mref.orientation_table(3, 200)        # it depends on (tetrahedron, case) only
    sizes = set()
    for t in range(6):
        for case in range(16):
            a, b = table[t][case], table[t][case ^ 15]
            sizes.add(len(a))
            assert len(a) == {0: 0, 1: 3, 2: 4, 3: 3, 4: 0}[bin(case).count("1")]
            assert b == (a[:1] + a[:0:-1]), (t, case)                          # the same start, the cycle reversed
            assert all(lo < hi and lo & hi == lo for lo, hi in a) and len(set(a)) == len(a)
    assert sizes == {0, 3, 4}


def test_a_sphere_comes_out_closed_and_faces_outward():
    vol, mesh = mref.reference('sphere')
    v, f = mesh['vertices'].astype(np.float64), mesh['faces']
    assert len(v) > 300 and len(f) > 600 and f.min() == 0 and f.max() == len(v) - 1
    assert np.all(np.diff(mesh['edge_ids']) > 0)
    uses = mref.edge_uses(f)
    assert all(sorted(u) == [-1, 1] for u in uses.values())                    # every edge: two faces, opposite directions
    assert len(v) - len(uses) + len(f) == 2
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    outward = (v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) / 3.0 - vol['centre']
    assert ((normal * outward).sum(axis=1) > 0).all()
    radial = np.abs(np.linalg.norm(v - vol['centre'], axis=1) - vol['radius'])
    print(f"\nsphere: {len(v)} vertices, {len(f)} faces; largest radial error {radial.max():.6e} = {radial.max() / vol['voxel']:.4f} voxels")
    # measured here: 5.557697e-03 (0.111 voxels: linear interpolation of a distance that is not linear along a lattice edge); twice that
    assert radial.max() <= 2 * 5.557697e-03
    c = mesh['colours']
    assert c.dtype == np.float32 and c.shape == v.shape and c.min() >= 0.0 and c.max() <= 1.0


def test_a_hole_has_a_clean_rim():
    vol, mesh = mref.reference('holed')
    whole = mref.reference('sphere')[1]
    f = mesh['faces']
    uses = mref.edge_uses(f)
    rim = [e for e, u in uses.items() if len(u) == 1]
    assert len(rim) >= 8 and all(len(u) == 1 or sorted(u) == [-1, 1] for u in uses.values())
    assert 0 < len(whole['faces']) - len(f) < 300
    # no vertex lies on a lattice edge with an invalid end
    nz, ny, nx = vol['weight'].shape
    invalid = (vol['weight'] < 1.0).reshape(-1)
    assert invalid.sum() == 27
    node, e = mesh['edge_ids'] // 7, mesh['edge_ids'] % 7 + 1
    other = node + ((e >> 2) * ny + ((e >> 1) & 1)) * nx + (e & 1)
    assert not invalid[node].any() and not invalid[other].any()
    # the rim is one closed loop around the hole: every rim vertex has two rim edges
    ends = np.array(rim).reshape(-1)
    assert (np.bincount(ends)[np.unique(ends)] == 2).all()


def test_small_volumes_of_the_reference():
    vol, mesh = mref.reference('minimum')                                      # corner 0 negative: all six tetrahedra cut one triangle off
    assert mesh['vertices'].shape == (7, 3) and mesh['faces'].shape == (6, 3) and mesh['colours'] is None
    np.testing.assert_array_equal(mesh['edge_ids'], np.arange(7))
    np.testing.assert_array_equal(mesh['vertices'][0], np.array([0.5 + 0.25 / 0.75, 0.5, 0.5], np.float32))
    vol, mesh = mref.reference('odd')
    node = mesh['edge_ids'] // 7
    nan_node, inf_node, light = (1 * 4 + 1) * 5 + 3, (2 * 4 + 3) * 5 + 1, (0 * 4 + 2) * 5 + 4
    e = mesh['edge_ids'] % 7 + 1
    other = node + ((e >> 2) * 4 + ((e >> 1) & 1)) * 5 + (e & 1)
    for gone in (nan_node, inf_node, light):
        assert gone not in node and gone not in other
    zero = (1 * 4 + 2) * 5 + 2                                                 # the exact 0 is positive: its vertices sit on the node itself
    on_zero = (node == zero) | (other == zero)
    assert on_zero.any()
    p0 = np.array([0.5 + 2.5 * 0.25, -1.0 + 2.5 * 0.25, 2.0 + 1.5 * 0.25], np.float32)
    assert all(np.array_equal(v, p0) for v in mesh['vertices'][on_zero])
    assert np.isfinite(mesh['vertices']).all() and np.isfinite(mesh['colours']).all()


# ---- the integrate reference on its own -----------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view(np.uint32)


def test_chunked_views_equal_whole_views_bitwise_and_every_seeded_case_occurs():
    case = ref.case_main()
    stats = []
    whole = ref.reference(case, stats=stats)
    for k in (1, 2):
        part = ref.reference(case, views=slice(0, k))
        part = ref.reference(case, views=slice(k, 3), vol=part)
        for key in ('tsdf', 'weight', 'colour'):
            assert np.array_equal(_bits(whole[key]), _bits(part[key])), (k, key)
    s0, s1, s2 = stats
    for s in (s0, s1):
        assert min(s['nan'], s['zero'], s['negative'], s['inf'], s['beyond'], s['outside'], s['hidden'], s['updated'], s['clipped']) > 0, s
    assert s0['at_minus_trunc'] >= 1 and s0['at_trunc'] >= 1
    assert s0['behind'] == 0 and 0 < s1['behind'] < 14 * 12 * 10 and s1['updated'] > 100            # the volume partly behind view 1
    assert s2['behind'] + s2['outside'] == 14 * 12 * 10 and s2['updated'] == 0                      # view 2 sees none of it
    w = whole['weight']
    assert set(np.unique(w).tolist()) == {0.0, 1.0, 2.0} and np.all((whole['tsdf'] >= -1.0) & (whole['tsdf'] <= 1.0))
    assert whole['tsdf'].min() == -1.0 and whole['tsdf'].max() == 1.0
    plain = ref.reference(case, colour=False)
    assert plain['colour'] is None and np.array_equal(_bits(plain['tsdf']), _bits(whole['tsdf']))
    small = ref.reference(ref.case_small())
    assert small['tsdf'].shape == (2, 3, 5) and (small['weight'] > 0).sum() >= 15


# ---- write_ply --------------------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    """A small reader of what write_ply writes: the header's elements and properties, then the binary rows."""
    data = open(path, 'rb').read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode('ascii').split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = []
    for line in lines[2:]:
        words = line.split()
        if words[:1] == ["element"]:
            elements.append((words[1], int(words[2]), []))
        elif words[:1] == ["property"]:
            elements[-1][2].append(tuple(words[1:]))
    out, at = {}, 0
    for name, n, props in elements:
        if props == [("list", "uchar", "int", "vertex_indices")]:
            rows = np.frombuffer(body, dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]), count=n, offset=at)
            at += 13 * n
            assert (rows['n'] == 3).all()
            out[name] = rows['v'].copy()
        else:
            dt = np.dtype([(p[1], {'float': '<f4', 'uchar': 'u1'}[p[0]]) for p in props])
            out[name] = np.frombuffer(body, dtype=dt, count=n, offset=at)
            at += dt.itemsize * n
    assert at == len(body)
    return out


def test_write_ply_with_faces_round_trips_and_without_them_is_what_it_was(tmp_path):
    from super_primitive_amd.odometery.results import write_ply
    vol, mesh = mref.reference('sphere')
    world = dict(points=torch.from_numpy(mesh['vertices']), colours=torch.from_numpy(mesh['colours']), faces=torch.from_numpy(mesh['faces']))
    got = _read_ply(write_ply(tmp_path / "mesh.ply", world))
    assert set(got) == {"vertex", "face"} and got['vertex'].dtype.names == ('x', 'y', 'z', 'red', 'green', 'blue')
    np.testing.assert_array_equal(np.stack([got['vertex'][k] for k in 'xyz'], axis=1), mesh['vertices'])
    np.testing.assert_array_equal(got['face'], mesh['faces'])
    rgb = np.clip(np.trunc(mesh['colours'].astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    np.testing.assert_array_equal(np.stack([got['vertex'][k] for k in ('red', 'green', 'blue')], axis=1), rgb)
    none = _read_ply(write_ply(tmp_path / "none.ply", dict(world, faces=torch.zeros(0, 3, dtype=torch.int32))))
    assert none['face'].shape == (0, 3)
    for bad in (torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 4, dtype=torch.int32), torch.zeros(12, dtype=torch.int32), [[0, 1, 2]]):
        with pytest.raises(ValueError, match="faces"):
            write_ply(tmp_path / "bad.ply", dict(world, faces=bad))
    # a fixed cloud without faces: the bytes written before there were faces, put together by hand
    pts = np.array([[0.0, 1.0, -2.5], [3.25, 1e-3, 7.0]], np.float32)
    cols = np.array([[0.0, 0.5, 1.0], [1.5, -0.25, float("nan")]], np.float32)
    path = write_ply(tmp_path / "cloud.ply", dict(points=torch.from_numpy(pts), colours=torch.from_numpy(cols)))
    want = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            + struct.pack("<3f3B", 0.0, 1.0, -2.5, 0, 127, 255) + struct.pack("<3f3B", 3.25, float(np.float32(1e-3)), 7.0, 255, 0, 0))
    assert open(path, 'rb').read() == want
    nrm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], np.float32)
    with_normals = open(write_ply(tmp_path / "normals.ply", dict(points=torch.from_numpy(pts), colours=torch.from_numpy(cols), normals=torch.from_numpy(nrm))), 'rb').read()
    assert b"element face" not in with_normals and len(with_normals) - with_normals.index(b"end_header\n") - 11 == 2 * 27


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_tsdf_volume_lays_the_box_out_and_refuses_what_is_too_large():
    from super_primitive_amd.odometery import results
    vol = results.tsdf_volume((-0.3, 0.2, 1.0), (0.3, 0.75, 1.5), 0.05, device="meta")
    assert set(vol) == {'tsdf', 'weight', 'colour', 'origin', 'voxel', 'trunc', 'dims'}
    assert vol['dims'] == (12, 11, 10) and tuple(vol['tsdf'].shape) == tuple(vol['weight'].shape) == (10, 11, 12) and tuple(vol['colour'].shape) == (10, 11, 12, 3)
    assert vol['origin'] == (-0.3, 0.2, 1.0) and vol['voxel'] == 0.05 and vol['trunc'] == 4 * 0.05
    flat = results.tsdf_volume((0, 0, 0), (1.0, 0.0, 0.01), 0.25, trunc=0.3, colour=False, device="meta")
    assert flat['dims'] == (4, 1, 1) and flat['colour'] is None and flat['trunc'] == 0.3
    assert results.tsdf_volume((0, 0, 0), (1024, 1024, 1024), 1.0, device="meta")['dims'] == (1024, 1024, 1024)       # 2^30: the limit itself
    with pytest.raises(ValueError, match="2\\^30"):
        results.tsdf_volume((0, 0, 0), (1025, 1024, 1024), 1.0, device="meta")
    with pytest.raises(ValueError, match="2\\^30"):
        results.tsdf_volume((0, 0, 0), (10.0, 10.0, 10.0), 1e-4)                                                      # (raises before it allocates)
    for voxel in (0.0, -0.1, INF, NAN, "fine", None):
        with pytest.raises(ValueError, match="voxel"):
            results.tsdf_volume((0, 0, 0), (1, 1, 1), voxel, device="meta")
    for trunc in (0.0, -1.0, INF, NAN, "wide"):
        with pytest.raises(ValueError, match="trunc"):
            results.tsdf_volume((0, 0, 0), (1, 1, 1), 0.1, trunc=trunc, device="meta")
    for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, INF)), ((0, NAN, 0), (1, 1, 1)), ((0, 0, 0), (1, -1, 1)), ("abc", (1, 1, 1)), (None, (1, 1, 1))):
        with pytest.raises(ValueError, match="tsdf_volume"):
            results.tsdf_volume(lo, hi, 0.1, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    cpu = results.tsdf_volume((0, 0, 0), (0.5, 0.5, 0.5), 0.1, device="cpu")
    Ks, poses = torch.eye(3), torch.eye(4)[None].repeat(2, 1, 1)
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.tsdf_integrate(cpu, torch.ones(2, 6, 8), Ks, poses)
    with pytest.raises(ValueError, match="HIP-only"):
        viz.tsdf_mesh(cpu)
    with pytest.raises(ValueError, match="HIP-only"):
        results.extract_mesh(cpu)
    with pytest.raises(ValueError, match="HIP-only"):
        results.fuse_tsdf(torch.ones(2, 6, 8), Ks, poses, 0.1, bounds=((0, 0, 0), (1, 1, 1)))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    vol = results.tsdf_volume((0, 0, 0), (0.5, 0.4, 0.3), 0.1, device="meta")
    assert vol['dims'] == (5, 4, 3)
    d, K, T, img = _meta(2, 6, 8), _meta(2, 3, 3), _meta(2, 4, 4), _meta(2, 3, 6, 8)
    for handle in (None, {}, 3, {k: v for k, v in vol.items() if k != 'trunc'}, dict(vol, dims=(5, 4)), dict(vol, dims=(4, 4, 3)), dict(vol, dims=(5, 4, 0)),
                   dict(vol, tsdf=_meta(3, 4, 5, dtype=torch.float64)), dict(vol, weight=_meta(3, 4)), dict(vol, weight=None), dict(vol, colour=_meta(3, 4, 5)),
                   dict(vol, tsdf=_meta(5, 4, 3).permute(2, 1, 0)), dict(vol, voxel=0.0), dict(vol, voxel=NAN), dict(vol, voxel="x"), dict(vol, trunc=-1.0),
                   dict(vol, trunc=INF), dict(vol, origin=(0, 0)), dict(vol, origin=(0, INF, 0)), dict(vol, origin=None), dict(vol, tsdf=[0.0])):
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            viz.tsdf_integrate(handle, d, K, T)
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            viz.tsdf_mesh(handle)
        with pytest.raises(ValueError, match="volume|voxel|origin"):
            results.extract_mesh(handle)
        if handle is not None:                                                 # (None: a new volume)
            with pytest.raises(ValueError, match="volume|voxel|origin"):
                results.fuse_tsdf(d, K, T, 0.1, volume=handle)
    for depths in (_meta(2, 6, 8, dtype=torch.float64), _meta(3, 6, 8), _meta(2, 6), _meta(2, 0, 8), [[1.0]]):
        with pytest.raises(ValueError):
            viz.tsdf_integrate(vol, depths, K, T)
        with pytest.raises(ValueError):
            results.fuse_tsdf(depths, K, T, 0.1, bounds=((0, 0, 0), (1, 1, 1)))
    for bad_T in (_meta(4, 4), _meta(2, 3, 4), _meta(0, 4, 4), _meta(2, 4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="poses"):
            viz.tsdf_integrate(vol, d, K, bad_T)
    for bad_K in (_meta(3, 3, 3), _meta(2, 9), _meta(2, 3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="Ks"):
            viz.tsdf_integrate(vol, d, bad_K, T)
    for images in (_meta(2, 3, 6, 9), _meta(2, 4, 6, 8), _meta(2, 3, 6, 8, dtype=torch.float16), _meta(3, 6, 8)):
        with pytest.raises(ValueError, match="images"):
            viz.tsdf_integrate(vol, d, K, T, images=images)
    with pytest.raises(ValueError, match="without colour"):
        viz.tsdf_integrate(dict(vol, colour=None), d, K, T, images=img)
    for z_min in (-1.0, NAN):
        with pytest.raises(ValueError, match="z_min"):
            viz.tsdf_integrate(vol, d, K, T, z_min=z_min)
    for depth_max in (0.0, -2.0, NAN):
        with pytest.raises(ValueError, match="depth_max"):
            viz.tsdf_integrate(vol, d, K, T, depth_max=depth_max)
        with pytest.raises(ValueError, match="depth_max"):
            results.fuse_tsdf(d, K, T, 0.1, bounds=((0, 0, 0), (1, 1, 1)), depth_max=depth_max)
    with pytest.raises(ValueError, match="limits"):
        viz.tsdf_integrate(vol, _meta(2, 1 << 15, 1 << 15), K, T)
    for min_weight in (NAN, "heavy", None):
        with pytest.raises(ValueError, match="min_weight"):
            viz.tsdf_mesh(vol, min_weight=min_weight)
        with pytest.raises(ValueError, match="min_weight"):
            results.extract_mesh(vol, min_weight=min_weight)
    with pytest.raises(ValueError, match="no cell"):
        viz.tsdf_mesh(results.tsdf_volume((0, 0, 0), (0.5, 0.5, 0.05), 0.1, device="meta"))
    for voxel, trunc in ((0.0, None), (NAN, None), (0.1, -1.0), ("x", None), (0.1, INF)):
        with pytest.raises(ValueError, match="voxel"):
            results.fuse_tsdf(d, K, T, voxel, bounds=((0, 0, 0), (1, 1, 1)), trunc=trunc)
        with pytest.raises(ValueError, match="voxel"):
            results.sequence_tsdf(dict(points=_meta(5, 3)), dict(kf_archive={}), voxel, trunc=trunc)
    for bounds in (3, ((0, 0, 0),), ((0, 0, 0), (1, 1)), ((0, 0, 0), (1, NAN, 1)), ((2, 0, 0), (1, 1, 1))):
        with pytest.raises(ValueError, match="bounds|tsdf_volume"):
            results.fuse_tsdf(d, K, T, 0.1, bounds=bounds)
    with pytest.raises(ValueError, match="2\\^30"):
        results.fuse_tsdf(d, K, T, 1e-4, bounds=((0, 0, 0), (10, 10, 10)))
    with pytest.raises(ValueError, match="keep_keyframes"):
        results.sequence_tsdf(dict(points=_meta(5, 3), ids=[0, 4]), dict(kf_archive={0: dict(kf=None), 4: dict(kf=None)}), 0.05)
