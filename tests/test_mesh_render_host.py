"""CPU-only: the ABI of the mesh views (include/sp_hip.h: sp_mesh_render), its argument checks -- made before any device work, so they answer
without a GPU --, the refusals of the Python surface on ``meta`` tensors, and the reference of tests/mesh_render_ref.py against the
properties the rule promises: a watertight sphere from inside, the silhouette and the depth bound from outside, exact rows and depths on
a plane that crosses the camera plane, no crack along a shared edge, exact negation of shared edge planes, the highest index on equal
depths, and ``visible_faces`` / ``cull_mesh`` on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_render_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
H, W = ref.H, ref.W


# ---- ABI and arguments ----------------------------------------------------------------------------------------------------------------------
def test_the_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype and constant against the ctypes mirror: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    lib = _lib.load()
    for name in ("sp_mesh_render", "sp_mesh_render_scratch_units"):
        assert name in _lib.SIGNATURES and name not in _lib.RESTYPES and getattr(lib, name).restype is ctypes.c_int
        assert f"int {name}(" in header
    assert _lib.SP_ABI_VERSION == 20 and "#define SP_ABI_VERSION 20" in header
    assert _lib.SP_MESH_RENDER_VIEW_CHUNK == 16
    assert header.index("int sp_mesh_sample(") < header.index("int sp_mesh_render(")
    assert len(_lib.SIGNATURES["sp_mesh_render"]) == 19


def test_scratch_units():
    from super_primitive_amd import _lib
    lib = _lib.load()
    assert lib.sp_mesh_render_scratch_units(0) == -1 and lib.sp_mesh_render_scratch_units(-5) == -1
    assert lib.sp_mesh_render_scratch_units((1 << 28) + 1) == -2
    chunk = _lib.SP_MESH_RENDER_VIEW_CHUNK
    for F in (1, 256, 257, 1196, 1 << 28):
        blocks = -(-F // 256)
        assert lib.sp_mesh_render_scratch_units(F) == 1 + -(-blocks * chunk // 8) + blocks * chunk * 32, F
    assert 0 < lib.sp_mesh_render_scratch_units(1 << 28) < 2 ** 31


def test_render_refuses_bad_arguments_without_a_device():
    """Every case is refused before the launch: a set of arguments that passes is never sent (there may be no device, and 0x2000 is no
    buffer).  An upper limit's edge is therefore its first refused value."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    p, odd4, odd8 = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x2002), ctypes.c_void_p(0x2004)
    ok = dict(vertices=p, colours=p, M=600, faces=p, F=1196, face_normals=p, views=p, V=3, H=24, W=32, z_min=1e-6, cull=0, scratch=p, keys=p,
              depth=p, normals=p, image=p, index=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_mesh_render(a['vertices'], a['colours'], a['M'], a['faces'], a['F'], a['face_normals'], a['views'], a['V'], a['H'], a['W'],
                                  a['z_min'], a['cull'], a['scratch'], a['keys'], a['depth'], a['normals'], a['image'], a['index'], None)
    none = dict(depth=None, normals=None, image=None, index=None)
    for bad in (dict(vertices=None), dict(faces=None), dict(views=None), dict(scratch=None), dict(keys=None), none, dict(colours=None),
                dict(face_normals=None), dict(none, colours=None, image=p), dict(none, face_normals=None, normals=p),
                dict(scratch=odd8), dict(keys=odd8), dict(vertices=odd4), dict(faces=odd4), dict(views=odd4), dict(colours=odd4),
                dict(face_normals=odd4), dict(depth=odd4), dict(normals=odd4), dict(index=odd4),
                dict(F=0), dict(F=-1), dict(M=0), dict(M=-7), dict(V=0), dict(V=-1), dict(H=0), dict(W=0), dict(W=-5),
                dict(z_min=-1e-9), dict(z_min=NAN), dict(cull=2), dict(cull=-1)):
        assert call(**bad) == -1, bad
    for big in (dict(F=(1 << 28) + 1), dict(M=(1 << 28) + 1), dict(F=1 << 40), dict(V=65536), dict(V=32768, H=256, W=256),
                dict(V=1, H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15)):
        assert call(**big) == -2, big
    # invalid beats too large
    assert call(V=65536, vertices=None) == -1 and call(F=(1 << 28) + 1, cull=3) == -1 and call(M=1 << 40, z_min=NAN) == -1
    assert call(V=1 << 20, **none) == -1 and call(F=1 << 40, colours=None) == -1 and call(V=2, H=1 << 15, W=1 << 15, M=0) == -1
    assert call(F=(1 << 28) + 1, keys=odd8) == -1


# ---- the reference on its own ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball():
    return ref.sphere(), ref.sphere_views()


@pytest.mark.parametrize("fx", [20.0, 6.0])
def test_the_sphere_is_watertight_from_its_centre_and_culled_away_entirely(ball, fx):
    mesh, views = ball
    args = (mesh['vertices'], mesh['faces'], ref.camera(fx), views['centre'], H, W)
    depth, _, _, index, counts = ref.render_view(*args)
    print(f"\nfrom the centre, fx = {fx}: {counts}")
    assert counts['hits'] == 768 == H * W and (index >= 0).all() and (depth > 0).all()
    assert counts['whole'] > 0                                                      # faces with vertices on both sides of the camera plane
    r = float(mesh['radius'])
    assert depth.max() <= r * (1 + 1e-3)                                           # z <= the distance <= the radius, up to the mesh's vertices
    assert ref.render_view(*args, cull=1)[4] == dict(hits=0, faces=0, whole=0)     # the faces look outwards


def test_the_sphere_from_outside_stays_inside_the_analytic_silhouette(ball):
    mesh, views = ball
    K, T = ref.camera(20.0), views['outside']
    depth, _, _, index, counts = ref.render_view(mesh['vertices'], mesh['faces'], K, T, H, W)
    culled = ref.render_view(mesh['vertices'], mesh['faces'], K, T, H, W, cull=1)
    print(f"\nfrom 4 r: {counts}")
    assert counts == dict(hits=80, faces=77, whole=0) == culled[4]
    assert np.array_equal(depth.view(np.uint32), culled[0].view(np.uint32)) and np.array_equal(index, culled[3])
    # the analytic sphere through the same pixels: the ray (a, b, 1) s from the camera (identity rotation) at o
    c, r = np.asarray(mesh['centre'], np.float64), float(mesh['radius'])
    o = T[:3, 3].astype(np.float64)
    rows, cols = np.mgrid[0:H, 0:W]
    d = np.stack([(cols - 15.5) / 20.0, (rows - 11.5) / 20.0, np.ones((H, W))], axis=-1)
    oc = o - c
    A, B, C = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - r * r
    disc = B * B - 4.0 * A * C
    hit = index >= 0
    assert (disc[hit] > 0).all(), "a pixel outside the sphere's silhouette is hit"
    z_sphere = (-B - np.sqrt(np.where(disc > 0, disc, 0.0))) / (2.0 * A)
    slack = (depth.astype(np.float64) - z_sphere)[hit]
    print(f"mesh depth - sphere depth on the {int(hit.sum())} hits: {slack.min():.3e} .. {slack.max():.3e}")
    assert (slack >= 0).all()                                                       # the chordal mesh lies inside the sphere


def test_shared_edges_negate_exactly(ball):
    """For every edge shared by two faces of the sphere the edge plane of one is the exact negation of the other's, component by
    component, in a view with a general pose: what makes the inclusive comparison crack-free."""
    mesh, views = ball
    planes = {}
    for face in mesh['faces']:
        s = ref.face_setup(mesh['vertices'], face, ref.camera(20.0), views['grazing'], H, W, 0.0, 0)
        i = [int(k) for k in face]
        q = [ref.camera_point(views['grazing'], mesh['vertices'][k]) for k in i]
        n = [ref.cross(q[1], q[2]), ref.cross(q[2], q[0]), ref.cross(q[0], q[1])]
        assert s is None or s['n'] == n
        for k in range(3):
            planes[(i[(k + 1) % 3], i[(k + 2) % 3])] = n[k]
    shared = [(e, (e[1], e[0])) for e in planes if e[0] < e[1] and (e[1], e[0]) in planes]
    assert len(shared) > 1700 and len(planes) == 3 * len(mesh['faces'])             # a closed surface: (nearly) every edge has its twin
    for e, twin in shared:
        assert all(x == -y for x, y in zip(planes[e], planes[twin])), e


def test_a_floor_that_crosses_the_camera_plane_is_hit_on_exactly_the_rows_in_range():
    """The plane y = 1 from z = -10 to z = 60 under an identity camera: the ray of row r meets it at z = 1 / b, b = (r - cy) / fy."""
    for h, w, last in ((21, 30, 20), (H, W, 23)):
        m = ref.floor()
        depth, _, _, index, counts = ref.render_view(m['vertices'], m['faces'], ref.camera(20.0), ref.identity(), h, w)
        b = (np.arange(h) - 11.5) / 20.0
        with np.errstate(divide='ignore'):
            want = (b > 0) & (1.0 / b < 60.0)
        rows = (index >= 0).any(axis=1)
        assert np.array_equal(rows, want) and np.nonzero(rows)[0].tolist() == list(range(12, last + 1))
        assert counts['whole'] == 1 and counts['faces'] == 1                        # tested on the whole image, no clipping
        z = np.broadcast_to((1.0 / b[rows])[:, None], (int(rows.sum()), w))
        hit = index[rows] >= 0
        err = np.abs(depth[rows].astype(np.float64) - z)[hit] / z[hit]
        print(f"\nfloor {h}x{w}: {counts}; largest relative depth error {err.max():.3e}")
        assert err.max() <= 2.0 ** -22
        # seen from above it is a front face; flipped it is culled
        assert ref.render_view(m['vertices'], m['faces'], ref.camera(20.0), ref.identity(), h, w, cull=1)[4] == counts
        flipped = ref.floor(flipped=True)
        assert ref.render_view(flipped['vertices'], flipped['faces'], ref.camera(20.0), ref.identity(), h, w)[4] == counts
        assert ref.render_view(flipped['vertices'], flipped['faces'], ref.camera(20.0), ref.identity(), h, w, cull=1)[4]['hits'] == 0


def _inside_outline(corners, h, w):
    """Pixels strictly inside the convex outline of the projected ``corners`` (k,2), by a margin far above any rounding."""
    rows, cols = np.mgrid[0:h, 0:w]
    inside = np.ones((h, w), bool)
    n = len(corners)
    orient = np.sign(sum(corners[k][0] * corners[(k + 1) % n][1] - corners[(k + 1) % n][0] * corners[k][1] for k in range(n)))
    for k in range(n):
        (x0, y0), (x1, y1) = corners[k], corners[(k + 1) % n]
        inside &= orient * ((x1 - x0) * (rows - y0) - (y1 - y0) * (cols - x0)) > 1e-9
    return inside


@pytest.mark.parametrize("posed", [False, True])
def test_the_slanted_quad_has_the_planes_depth_and_no_crack_along_its_diagonal(posed):
    m = ref.quad()
    K = ref.camera(20.0)
    T = ref.pose((0.2, -0.3, 0.1), (0.3, -0.2, -1.0)) if posed else ref.identity()
    depth, _, _, index, counts = ref.render_view(m['vertices'], m['faces'], K, T, H, W)
    q = np.array([ref.camera_point(T, p) for p in m['vertices']])
    corners = [ref.pixel_of(K, p) for p in q]
    inside = _inside_outline(corners, H, W)
    hit = index >= 0
    print(f"\nquad, posed = {posed}: {counts}; {int(inside.sum())} pixels strictly inside the outline")
    assert inside.sum() > 100 and hit[inside].all()                                 # the diagonal is crossed by rows of them
    assert counts['faces'] == 2
    # the ray-plane depth in float64: the plane through the camera-frame corners 0, 1, 2 (exactly coplanar with 3 for the identity)
    nrm = np.cross(q[1] - q[0], q[2] - q[0])
    rows, cols = np.nonzero(hit)
    rays = np.stack([(cols - 15.5) / 20.0, (rows - 11.5) / 20.0, np.ones(len(rows))], axis=-1)
    z = (nrm @ q[0]) / (rays @ nrm)
    err = np.abs(depth[hit].astype(np.float64) - z) / z
    print(f"largest relative depth error against the plane: {err.max():.3e}")
    assert err.max() <= 2.0 ** -22                                                  # one rounding to float32 is 2^-24; the float64 noise is far below


def test_a_duplicated_face_goes_to_the_higher_index_and_a_face_behind_the_camera_hits_nothing():
    m = ref.duplicate()
    index, counts = ref.render_view(m['vertices'], m['faces'], ref.camera(20.0), ref.identity(), H, W)[3:]
    assert counts['hits'] > 100 and set(np.unique(index).tolist()) <= {-1, 1, 2} and (index == 1).sum() > 100
    one = ref.single()
    alone = ref.render_view(one['vertices'], one['faces'], ref.camera(20.0), ref.identity(), H, W)[3]
    assert np.array_equal(index[alone >= 0], np.ones(int((alone >= 0).sum()), np.int32))      # every pixel of the pair: face 1
    b = ref.behind()
    assert ref.render_view(b['vertices'], b['faces'], ref.camera(20.0), ref.identity(), H, W)[4] == dict(hits=0, faces=0, whole=0)
    u = ref.unusable()
    assert ref.render_view(u['vertices'], u['faces'], ref.camera(20.0), ref.identity(), H, W)[4] == dict(hits=0, faces=0, whole=0)


def test_a_triangle_larger_than_the_image_hits_every_pixel_from_its_own_rectangle():
    m = ref.oversized()
    depth, _, image, index, counts = ref.render_view(m['vertices'], m['faces'], ref.camera(20.0), ref.identity(), 40, 56, colours=m['colours'])
    assert counts == dict(hits=2240, faces=1, whole=0) and (index == 0).all() and (depth > 2).all() and (depth < 4).all()
    total = image.astype(np.int64).sum(axis=-1)
    assert total.min() >= 253 and total.max() <= 255                               # the weights sum to one


def test_every_device_case_shows_what_its_name_says():
    counts = {}
    for name, (mesh, Ks, poses, h, w) in ref.cases().items():
        out, rec = ref.rendered(name, mesh, Ks, poses, h, w)
        counts[name] = out['counts'][0]
        hit = out['index'] >= 0
        assert (out['depth'][~hit] == 0).all() and np.isnan(out['normals'][~hit]).all() and (out['depth'][hit] > 0).all()
        if out['image'] is not None:
            assert (out['image'][~hit] == 0).all()
    print(f"\n{counts}")
    mixed_index = ref.rendered('mixed', *ref.cases()['mixed'])[0]['index']
    assert set(np.unique(mixed_index).tolist()) == {-1, 0, 3}                       # both valid faces, and none of the others
    assert counts['skewed']['whole'] >= 3 and counts['skewed']['faces'] >= 10       # whole-image faces beside tiny ones
    skewed_index = ref.rendered('skewed from afar', *ref.cases()['skewed from afar'])[0]['index']
    assert (skewed_index == 137).sum() > 200 and counts['skewed from afar']['faces'] >= 2
    strip_index = ref.rendered('strip', *ref.cases()['strip'])[0]['index']
    assert strip_index.max() >= 100 and counts['strip']['faces'] > 20
    assert counts['floor']['whole'] == 1 and counts['oversized'] == dict(hits=2240, faces=1, whole=0)
    assert counts['unusable']['hits'] == 0 and counts['sphere from its centre']['hits'] == 768
    assert 0 < counts['sphere grazing']['hits'] < 21 * 30


# ---- visible_faces and cull_mesh on CPU tensors ---------------------------------------------------------------------------------------------
def _mesh_dict(mesh):
    out = dict(points=torch.from_numpy(mesh['vertices']), faces=torch.from_numpy(mesh['faces']))
    if mesh.get('colours') is not None:
        out['colours'] = torch.from_numpy(mesh['colours'])
    return out


def test_visible_faces_and_cull_mesh_on_cpu_tensors(ball):
    from super_primitive_amd.odometery import results
    mesh, views = ball
    Ks, poses = np.stack([ref.camera(20.0)] * 2), np.stack([views['outside'], views['grazing']])
    out = ref.render(mesh['vertices'], mesh['faces'], Ks, poses, H, W)
    index = torch.from_numpy(out['index'])
    m = _mesh_dict(mesh)
    seen = results.visible_faces(m, None, None, None, index=index)
    F = len(mesh['faces'])
    assert seen['pixels'].dtype == torch.int64 and seen['views'].dtype == torch.int32 and tuple(seen['pixels'].shape) == tuple(seen['views'].shape) == (F,)
    assert int(seen['pixels'].sum()) == sum(c['hits'] for c in out['counts'])
    per_view = [np.bincount(out['index'][v][out['index'][v] >= 0], minlength=F) for v in range(2)]
    assert np.array_equal(seen['pixels'].numpy(), per_view[0] + per_view[1])
    assert np.array_equal(seen['views'].numpy(), (per_view[0] > 0).astype(np.int32) + (per_view[1] > 0))
    assert int(seen['views'].max()) == 2
    # from outside alone: the cull keeps exactly the faces seen, in order, and the vertices they use
    first = results.visible_faces(m, None, None, None, index=index[:1])
    kept = results.cull_mesh(m, None, None, None, visible=first)
    faces_seen = np.unique(out['index'][0][out['index'][0] >= 0])
    assert len(faces_seen) == 77 and np.array_equal(kept['kept_faces'].numpy(), faces_seen)
    assert np.array_equal(kept['kept_vertices'].numpy(), np.unique(mesh['faces'][faces_seen]))
    assert np.array_equal(kept['points'].numpy()[kept['faces'].numpy()], mesh['vertices'][mesh['faces'][faces_seen]])
    assert np.array_equal(kept['colours'].numpy(), mesh['colours'][kept['kept_vertices'].numpy()])
    assert kept['faces'].dtype == torch.int32 and kept['offsets'].tolist() == [0, len(kept['points'])]
    # a second cull is the identity: the kept faces hide nothing of each other that the whole sphere did not hide
    again_index = ref.render(kept['points'].numpy(), kept['faces'].numpy(), Ks[:1], poses[:1], H, W)['index']
    assert np.array_equal(again_index >= 0, out['index'][:1] >= 0)
    again = results.cull_mesh(kept, None, None, None, visible=results.visible_faces(kept, None, None, None, index=torch.from_numpy(again_index)))
    assert torch.equal(again['faces'], kept['faces']) and torch.equal(again['points'], kept['points'])
    assert again['kept_faces'].tolist() == list(range(77))
    # min_pixels
    two = results.cull_mesh(m, None, None, None, min_pixels=2, visible=first)
    assert np.array_equal(two['kept_faces'].numpy(), np.nonzero(per_view[0] >= 2)[0]) and 0 < len(two['kept_faces']) < 77
    for bad in (0, -1, 1.5, "many", None):
        with pytest.raises(ValueError, match="min_pixels"):
            results.cull_mesh(m, None, None, None, min_pixels=bad, visible=first)
    with pytest.raises(ValueError, match="visible"):
        results.cull_mesh(m, None, None, None, visible=dict(pixels=torch.zeros(5, dtype=torch.int64)))
    with pytest.raises(ValueError, match="index"):
        results.visible_faces(m, None, None, None, index=index.long())


def test_clean_mesh_still_selects_as_before():
    """``clean_mesh`` and ``cull_mesh`` share one selection: the degenerate faces of ``mixed`` go, the order stays."""
    from super_primitive_amd.odometery import results
    mesh, rec = ref.records_of('mixed')
    records = dict(state=torch.from_numpy(rec['state']), area=torch.from_numpy(rec['area']), normals=torch.from_numpy(rec['normals']),
                   area_max=torch.tensor(rec['area_max'], dtype=torch.float64))
    out = results.clean_mesh(_mesh_dict(mesh), records=records)
    assert out['kept_faces'].tolist() == [0, 3] and out['kept_vertices'].tolist() == [0, 1, 2, 3]
    assert out['faces'].tolist() == [[0, 1, 2], [1, 3, 2]] and out['offsets'].tolist() == [0, 4]


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------
def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    cpu = _mesh_dict(ref.single())
    Ks, poses = torch.eye(3), torch.eye(4)[None].repeat(2, 1, 1)
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.mesh_render(cpu['points'], cpu['faces'], Ks, poses, 6, 8)
    with pytest.raises(ValueError, match="HIP-only"):
        results.render_mesh(cpu, Ks, poses, (6, 8))
    with pytest.raises(ValueError, match="HIP-only"):
        results.score_mesh(cpu, torch.ones(2, 6, 8), Ks, poses)
    with pytest.raises(ValueError, match="HIP-only"):
        results.score_mesh_images(cpu, torch.ones(2, 3, 6, 8), Ks, poses)
    with pytest.raises(ValueError, match="HIP-only"):
        results.visible_faces(cpu, Ks, poses, (6, 8))
    with pytest.raises(ValueError, match="HIP-only"):
        results.cull_mesh(cpu, Ks, poses, (6, 8))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    v, f, c, n = _meta(5, 3), _meta(7, 3, dtype=torch.int32), _meta(5, 3), _meta(7, 3)
    K, T, d, img = _meta(2, 3, 3), _meta(2, 4, 4), _meta(2, 6, 8), _meta(2, 3, 6, 8)
    mesh = dict(points=v, faces=f, colours=c)
    for bad_v, bad_f in ((_meta(5, 3, dtype=torch.float64), f), (_meta(5, 4), f), (v, _meta(7, 3, dtype=torch.int64)), (v, _meta(7, 4, dtype=torch.int32)),
                         (_meta(0, 3), f), (v, _meta(0, 3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="vertices|faces|mesh"):
            viz.mesh_render(bad_v, bad_f, K, T, 6, 8)
        for call in (lambda m: results.render_mesh(m, K, T, (6, 8)), lambda m: results.score_mesh(m, d, K, T),
                     lambda m: results.score_mesh_images(m, img, K, T), lambda m: results.visible_faces(m, K, T, (6, 8)),
                     lambda m: results.cull_mesh(m, K, T, (6, 8))):
            with pytest.raises(ValueError, match="points|faces|mesh"):
                call(dict(points=bad_v, faces=bad_f, colours=c))
    for handle in (None, {}, 3, dict(points=v)):
        with pytest.raises(ValueError, match="mesh"):
            results.render_mesh(handle, K, T, (6, 8))
        with pytest.raises(ValueError, match="mesh"):
            results.visible_faces(handle, K, T, (6, 8))
    for bad_T in (_meta(4, 4), _meta(2, 3, 4), _meta(2, 4, 4, dtype=torch.int32), _meta(0, 4, 4)):
        with pytest.raises(ValueError, match="poses"):
            viz.mesh_render(v, f, K, bad_T, 6, 8)
        with pytest.raises(ValueError, match="poses"):
            results.score_mesh(mesh, _meta(int(bad_T.shape[0]), 6, 8), K, bad_T)
    for bad_K in (_meta(3, 3, 3), _meta(2, 9), _meta(2, 3, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="Ks"):
            viz.mesh_render(v, f, bad_K, T, 6, 8)
    for size in ((0, 8), (6, -1)):
        with pytest.raises(ValueError, match="image size"):
            viz.mesh_render(v, f, K, T, *size)
    for z_min in (-1.0, NAN, "near"):
        with pytest.raises(ValueError, match="z_min"):
            viz.mesh_render(v, f, K, T, 6, 8, z_min=z_min)
    for colours in (_meta(4, 3), _meta(5, 3, dtype=torch.float64), _meta(5, 4)):
        with pytest.raises(ValueError, match="colours"):
            viz.mesh_render(v, f, K, T, 6, 8, colours=colours)
        with pytest.raises(ValueError, match="colours"):
            results.render_mesh(dict(mesh, colours=colours), K, T, (6, 8), records=dict(state=1))
    for normals in (_meta(5, 3), _meta(7, 3, dtype=torch.float64), _meta(7, 4)):
        with pytest.raises(ValueError, match="face_normals"):
            viz.mesh_render(v, f, K, T, 6, 8, face_normals=normals)
    with pytest.raises(ValueError, match="colours"):
        viz.mesh_render(v, f, K, T, 6, 8, image=True)
    with pytest.raises(ValueError, match="colours"):
        results.score_mesh_images(dict(points=v, faces=f), img, K, T)
    with pytest.raises(ValueError, match="face_normals"):
        viz.mesh_render(v, f, K, T, 6, 8, normals=True)
    with pytest.raises(ValueError, match="no output"):
        viz.mesh_render(v, f, K, T, 6, 8, depth=False, index=False)
    with pytest.raises(ValueError, match="no output"):
        viz.mesh_render(v, f, K, T, 6, 8, colours=c, face_normals=n, depth=False, normals=False, image=False, index=False)
    with pytest.raises(ValueError, match="limits"):
        viz.mesh_render(v, f, K, T, 1 << 15, 1 << 15)
    with pytest.raises(ValueError, match="records"):
        results.render_mesh(mesh, K, T, (6, 8), records=dict(state=1))
    for depths in (_meta(2, 6, 8, dtype=torch.float64), _meta(3, 6, 8), _meta(2, 6), [[1.0]]):
        with pytest.raises(ValueError, match="gt_depths"):
            results.score_mesh(mesh, depths, K, T)
    with pytest.raises(ValueError, match="depth range"):
        results.score_mesh(mesh, d, K, T, min_depth=3.0, max_depth=2.0)
    for images in (_meta(2, 3, 6, 8, dtype=torch.float16), _meta(2, 4, 6, 8), _meta(3, 3, 6, 8), _meta(2, 6, 8)):
        with pytest.raises(ValueError, match="images"):
            results.score_mesh_images(mesh, images, K, T)


def test_the_wrapper_hands_the_library_what_the_header_says(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    seen = {}

    class Lib:
        def sp_mesh_render_scratch_units(self, F):
            seen['F'] = F
            return 3

        def sp_mesh_render(self, *args):
            seen.update(M=args[2], F=args[4], V=args[7], H=args[8], W=args[9], z_min=args[10], cull=args[11],
                        given=[a is not None for a in (args[1], args[5])], outputs=[a is not None for a in args[14:18]])
            return 0
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else 1)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    v, f, c, n = _meta(5, 3), _meta(7, 3, dtype=torch.int32), _meta(5, 3), _meta(7, 3)
    K, T = _meta(3, 3), _meta(2, 4, 4)
    out = viz.mesh_render(v, f, K, T, 6, 8)
    assert seen == dict(M=5, F=7, V=2, H=6, W=8, z_min=viz.Z_MIN, cull=0, given=[False, False], outputs=[True, False, False, True])
    assert set(out) == {'depth', 'index'} and tuple(out['depth'].shape) == (2, 6, 8) and out['index'].dtype == torch.int32
    out = viz.mesh_render(v, f, K, T, 6, 8, colours=c, face_normals=n, cull=True, z_min=0.0)
    assert seen['cull'] == 1 and seen['z_min'] == 0.0 and seen['given'] == [True, True] and seen['outputs'] == [True] * 4
    assert tuple(out['normals'].shape) == (2, 6, 8, 3) and out['image'].dtype == torch.uint8 and tuple(out['image'].shape) == (2, 6, 8, 3)
    out = viz.mesh_render(v, f, K, T, 6, 8, colours=c, face_normals=n, depth=False, image=False)
    assert seen['outputs'] == [False, True, False, True] and set(out) == {'normals', 'index'}
    records = dict(area=_meta(7, dtype=torch.float64), normals=n, state=_meta(7, dtype=torch.uint8), area_max=_meta(1, dtype=torch.float64))
    surface = results.render_mesh(dict(points=v, faces=f), K, T, (6, 8), cull=True, records=records)
    assert set(surface) == {'depth', 'normals', 'image', 'index'} and tuple(surface['image'].shape) == (2, 6, 8, 3)
    assert seen['cull'] == 1 and seen['outputs'] == [True, True, False, True]
