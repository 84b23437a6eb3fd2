"""-m gpu: the mesh views on the device (csrc/sp_mesh_render.hip) against the NumPy restatement of tests/mesh_render_ref.py, word for word,
through raw calls whose outputs are pre-filled with a sentinel: the sphere from inside, outside and a grazing pose, meshes with bad faces,
a large face beside tiny ones across two 256-face blocks, whole-image faces, partial tiles (21 x 30), an image smaller than its triangle,
equal depths, cull 0 and 1, every subset of the outputs, several views and a chunk boundary, repeatability, interpolated colours; then the
Python layers: ``render_mesh`` / ``score_mesh`` / ``score_mesh_images`` / ``visible_faces`` / ``cull_mesh``."""
import itertools

import numpy as np
import pytest
import torch

import mesh_render_ref as ref
from gpu_util import T, dev, npy

pytestmark = pytest.mark.gpu

OUTPUTS = ('depth', 'normals', 'image', 'index')
SENTINEL = -7


def _raw(mesh, normals, Ks, poses, h, w, cull=0, z_min=ref.Z_MIN, outputs=None):
    """One sp_mesh_render call; the outputs asked for are pre-filled with a sentinel, the others are NULL."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    outputs = outputs or tuple(k for k in OUTPUTS if k != 'image' or mesh.get('colours') is not None)
    v, f = T(mesh['vertices']), T(mesh['faces'])
    c = None if mesh.get('colours') is None else T(mesh['colours'])
    n = T(normals)
    V, M, F = len(poses), len(mesh['vertices']), len(mesh['faces'])
    views = torch.cat((T(np.asarray(Ks, np.float32).reshape(V, 9)), T(np.asarray(poses, np.float32).reshape(V, 16))), dim=1).contiguous()
    shapes = dict(depth=((V, h, w), torch.float32), normals=((V, h, w, 3), torch.float32), image=((V, h, w, 3), torch.uint8), index=((V, h, w), torch.int32))
    out = {k: torch.full(shapes[k][0], SENTINEL % 256 if k == 'image' else SENTINEL, dtype=shapes[k][1], device=dev()) for k in outputs}
    scratch = torch.full((8 * lib.sp_mesh_render_scratch_units(F),), SENTINEL, dtype=torch.int64, device=dev())
    keys = torch.full((V * h * w,), SENTINEL, dtype=torch.int64, device=dev())
    _lib.check(lib.sp_mesh_render(_lib.ptr(v), _lib.ptr(c), M, _lib.ptr(f), F, _lib.ptr(n), _lib.ptr(views), V, h, w, z_min, cull, _lib.ptr(scratch),
                                  _lib.ptr(keys), *(_lib.ptr(out.get(k)) for k in OUTPUTS), _lib.stream_ptr()), "sp_mesh_render")
    return out


def _same_words(got, want, what):
    """All outputs as 32-bit words (8-bit for the image): the NaNs of the normals by isnan agreement, everything else by bits."""
    for key in got:
        g, w = npy(got[key]), want[key]
        assert w is not None and g.shape == w.shape and g.dtype == w.dtype, f"{what}: {key}"
        if key == 'normals':
            assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: the NaN normals differ at {np.argwhere(np.isnan(g) != np.isnan(w))[:4].tolist()}"
            g, w = np.where(np.isnan(g), np.float32(0), g), np.where(np.isnan(w), np.float32(0), w)
        if g.dtype == np.float32:
            g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        diff = g != w
        assert not diff.any(), f"{what}: {key}: {int(diff.sum())} of {diff.size} words differ, first at {np.argwhere(diff)[0].tolist()}"


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", ['sphere from its centre', 'sphere from outside', 'sphere grazing', 'mixed', 'skewed', 'skewed from afar', 'strip',
                                  'single', 'floor', 'oversized', 'duplicate', 'quad', 'unusable'])
def test_a_case_equals_the_reference_word_for_word(cases, name, cull):
    mesh, Ks, poses, h, w = cases[name]
    want, rec = ref.rendered(name, mesh, Ks, poses, h, w, cull)
    got = _raw(mesh, rec['normals'], Ks, poses, h, w, cull=cull)
    assert set(got) == {k for k in OUTPUTS if want[k] is not None}
    _same_words(got, want, f"{name}, cull {cull}")
    print(f"\n{name}, cull {cull}: {want['counts'][0]}")
    assert int((got['index'] >= 0).sum()) == want['counts'][0]['hits']
    if name == 'unusable':
        assert bool((got['depth'] == 0).all()) and bool((got['index'] == -1).all()) and bool(torch.isnan(got['normals']).all()) and bool((got['image'] == 0).all())
    if name == 'mixed' and cull == 0:
        assert set(np.unique(npy(got['index'])).tolist()) == {-1, 0, 3}
    if name == 'duplicate' and cull == 0:
        assert int((got['index'] == 0).sum()) == 0 and int((got['index'] == 1).sum()) > 100
    if name == 'floor':
        assert want['counts'][0]['whole'] == 1


def test_every_subset_of_the_outputs_leaves_the_given_ones_unchanged(cases):
    mesh, Ks, poses, h, w = cases['sphere grazing']
    want, rec = ref.rendered('sphere grazing', mesh, Ks, poses, h, w)
    for n in range(1, 5):
        for subset in itertools.combinations(OUTPUTS, n):
            got = _raw(mesh, rec['normals'], Ks, poses, h, w, outputs=subset)
            assert set(got) == set(subset)
            _same_words(got, want, f"outputs {subset}")                        # (equal to the reference everywhere: every sentinel was overwritten)
    assert not (want['depth'] == SENTINEL).any() and not (want['index'] == SENTINEL).any()


def _views_around_the_sphere(n):
    """n cameras on a circle around the sphere, all looking at it, every third with another focal length."""
    mesh = ref.sphere()
    c, r = np.asarray(mesh['centre'], np.float64), float(mesh['radius'])
    Ks, poses = [], []
    for k in range(n):
        angle = 2.0 * np.pi * k / n
        T_k = ref.pose((0.0, angle, 0.0), c - 3.0 * r * np.array([np.sin(angle), 0.0, np.cos(angle)]))
        Ks.append(ref.camera(14.0 if k % 3 else 20.0))
        poses.append(T_k)
    return mesh, np.stack(Ks), np.stack(poses)


def test_three_views_in_one_call_and_two_runs_give_the_same_bits():
    mesh, Ks, poses = _views_around_the_sphere(3)
    want, rec = ref.rendered('three views', mesh, Ks, poses, 21, 30)
    got = _raw(mesh, rec['normals'], Ks, poses, 21, 30)
    _same_words(got, want, "three views")
    assert all(c['hits'] > 50 for c in want['counts'])
    again = _raw(mesh, rec['normals'], Ks, poses, 21, 30)
    for key in OUTPUTS:
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (got[key], again[key]))
        assert torch.equal(a, b), key


def test_a_chunk_boundary_and_the_order_of_the_views():
    """V = chunk + 1 views: the last goes through a second round of count, scan and raster.  The same views in another order give every
    view the same words: what a view holds depends on that view alone."""
    from super_primitive_amd import _lib
    V = _lib.SP_MESH_RENDER_VIEW_CHUNK + 1
    mesh, Ks, poses = _views_around_the_sphere(V)
    want, rec = ref.rendered('a chunk and one', mesh, Ks, poses, 21, 30)
    got = _raw(mesh, rec['normals'], Ks, poses, 21, 30)
    _same_words(got, want, "chunk + 1 views")
    assert all(c['hits'] > 50 for c in want['counts'])
    order = np.roll(np.arange(V)[::-1], 5)
    moved = _raw(mesh, rec['normals'], Ks[order], poses[order], 21, 30)
    _same_words(moved, {k: v[order] for k, v in want.items() if k != 'counts'}, "chunk + 1 views, reordered")


def test_interpolated_colours_of_one_triangle(cases):
    mesh, Ks, poses, h, w = cases['single']
    want, rec = ref.rendered('single', mesh, Ks, poses, h, w)
    got = _raw(mesh, rec['normals'], Ks, poses, h, w, outputs=('image', 'index'))
    _same_words(got, want, "single: image")
    hit = got['index'] >= 0
    total = got['image'][hit].long().sum(dim=1)
    print(f"\nsingle: {int(hit.sum())} hits, channel sums {int(total.min())} .. {int(total.max())}")
    assert int(hit.sum()) == 137 and int(total.min()) >= 253 and int(total.max()) <= 255      # red, green, blue corners: the weights sum to one
    assert bool((got['image'][hit].max(dim=0).values > 150).all())                           # and every corner's colour shows


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------
def _device_mesh(mesh):
    out = dict(points=T(mesh['vertices']), faces=T(mesh['faces']))
    if mesh.get('colours') is not None:
        out['colours'] = T(mesh['colours'])
    return out


def test_the_layers_equal_their_parts_put_together_by_hand():
    from super_primitive_amd.depth_completion import void
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    mesh, Ks, poses = _views_around_the_sphere(3)
    want, rec = ref.rendered('three views', mesh, Ks, poses, 21, 30)
    m = _device_mesh(mesh)
    K, P = T(Ks), T(poses)
    out = results.render_mesh(m, K, P, (21, 30))
    assert set(out) == set(OUTPUTS)
    _same_words(out, want, "render_mesh")
    records = results.mesh_faces(m)
    _same_words(results.render_mesh(m, K, P, (21, 30), records=records), want, "render_mesh with records")
    plain = results.render_mesh(dict(points=m['points'], faces=m['faces']), K, P, (21, 30), cull=True)
    assert bool((plain['image'] == 0).all()) and torch.equal(plain['index'], out['index'])   # the sphere from outside: nothing to cull
    raw = viz.mesh_render(m['points'], m['faces'], K, P, 21, 30)
    assert set(raw) == {'depth', 'index'} and torch.equal(raw['depth'].view(torch.int32), out['depth'].view(torch.int32))
    # score_mesh against a perturbed copy of its own depth: the tail by hand
    gt = out['depth'] * 1.01 + 0.001 * (out['index'] % 3 == 0)
    score = results.score_mesh(m, gt, K, P, min_depth=0.1, max_depth=5.0)
    in_range = (gt >= 0.1) & (gt <= 5.0)
    scored = in_range & (out['index'] >= 0)
    assert torch.equal(score['metrics'], void.depth_metrics(out['depth'], gt, scored))
    assert torch.equal(score['coverage'], scored.sum(dim=(1, 2)).double() / in_range.sum(dim=(1, 2)).double())
    # against its own depth: no error, on every pixel a face won
    own = results.score_mesh(m, out['depth'], K, P, min_depth=0.1, max_depth=5.0)
    col = {name: k for k, name in enumerate(own['columns'])}
    hits = torch.tensor([c['hits'] for c in want['counts']], dtype=torch.float64, device=dev())
    assert torch.equal(own['metrics'][:, col['n']], hits) and bool((own['metrics'][:, col['rmse']] == 0).all()) and bool((own['metrics'][:, col['mae']] == 0).all())
    assert bool((own['coverage'] == 1.0).all())
    # score_mesh_images
    images = torch.rand(3, 3, 21, 30, generator=torch.Generator().manual_seed(3)).to(dev())
    scored_images = results.score_mesh_images(m, images, K, P)
    sums = viz.image_metrics(out['image'], images, out['index'])
    assert torch.equal(scored_images['sums'], sums) and sums[:, 0].tolist() == [c['hits'] for c in want['counts']]
    assert bool(torch.isfinite(scored_images['psnr']).all())
    # visible_faces: the bincounts of the reference's index
    seen = results.visible_faces(m, K, P, (21, 30))
    F = len(mesh['faces'])
    per_view = np.stack([np.bincount(want['index'][v][want['index'][v] >= 0], minlength=F) for v in range(3)])
    assert np.array_equal(npy(seen['pixels']), per_view.sum(axis=0)) and np.array_equal(npy(seen['views']), (per_view > 0).sum(axis=0))
    assert seen['pixels'].dtype == torch.int64 and seen['views'].dtype == torch.int32


def test_cull_mesh_of_the_sphere_from_outside_lies_on_the_sphere(cases):
    from super_primitive_amd.odometery import results
    mesh, Ks, poses, h, w = cases['sphere from outside']
    want, _ = ref.rendered('sphere from outside', mesh, Ks, poses, h, w)
    m = _device_mesh(mesh)
    culled = results.cull_mesh(m, T(Ks), T(poses), (h, w))
    faces_seen = np.unique(want['index'][want['index'] >= 0])
    assert len(faces_seen) == 77 and np.array_equal(npy(culled['kept_faces']), faces_seen)
    assert np.array_equal(npy(culled['points'])[npy(culled['faces'])], mesh['vertices'][mesh['faces'][faces_seen]])
    again = results.cull_mesh(culled, T(Ks), T(poses), (h, w))                               # a second cull is the identity
    assert torch.equal(again['faces'], culled['faces']) and torch.equal(again['points'], culled['points'])
    # every sample of the culled mesh lies on a face of the sphere: its nearest sample of the whole sphere is within the sampling radius
    radius = 0.05
    met = results.mesh_distance(culled, m, radius, density=3000.0, seed=5)['metrics']
    print(f"\nculled sphere against the sphere: accuracy {float(met['accuracy']):.4e} over {int(met['n_a'])} samples, completion ratio {float(met['recall']):.3f}")
    assert int(met['within_a']) == int(met['n_a']) > 20 and float(met['accuracy']) < radius   # no sample of it is farther than the radius
    assert float(met['recall']) < 0.5                                                         # and it is a part of the sphere only


def test_a_mesh_extracted_from_a_fused_plane_is_seen_where_the_ray_cast_sees_the_volume():
    """``fuse_tsdf`` of a fronto-parallel synthetic depth, ``extract_mesh``, then ``render_mesh`` and ``render_surface`` from the same
    camera: both surfaces are the zero crossing of the same cells -- linear along an edge for the mesh, trilinear inside the cell for the
    ray -- so where both hit, away from the border, their depths differ by at most one voxel."""
    import tsdf_raycast_ref as rref
    from super_primitive_amd.odometery import results
    case = rref.plane_case(1.7)
    lo = case['origin']
    hi = tuple(o + n * case['voxel'] for o, n in zip(lo, case['dims']))
    depth, K, pose, images = T(case['depth']), T(case['K']), T(case['pose']), T(case['images'])
    vol = results.fuse_tsdf(depth, K, pose, case['voxel'], bounds=(lo, hi), images=images, trunc=case['trunc'])
    mesh = results.extract_mesh(vol)
    size = (case['H'], case['W'])
    by_mesh = results.render_mesh(mesh, K, pose, size)
    by_ray = results.render_surface(vol, K, pose, size, 3.0)
    both = (by_mesh['index'] >= 0) & (by_ray['index'] >= 0)
    inner = torch.zeros_like(both)
    inner[:, 1:-1, 1:-1] = both[:, 1:-1, 1:-1] & both[:, :-2, 1:-1] & both[:, 2:, 1:-1] & both[:, 1:-1, :-2] & both[:, 1:-1, 2:]
    diff = (by_mesh['depth'].double() - by_ray['depth'].double()).abs()[inner]
    print(f"\nmesh against ray-cast on a fused plane: {int((by_mesh['index'] >= 0).sum())} and {int((by_ray['index'] >= 0).sum())} hits, "
          f"{int(inner.sum())} compared; largest |difference| {float(diff.max()):.3e} (voxel {case['voxel']})")
    assert int(inner.sum()) > 300 and float(diff.max()) <= case['voxel']
    assert float((by_mesh['depth'][inner].double() - 1.7).abs().max()) <= case['voxel']
    nrm = by_mesh['normals'][inner]
    assert bool((nrm[:, 2] < -0.99).all())                                                    # the faces look into free space: at the camera
    assert int(by_mesh['image'][inner].long().sum()) > 0                                      # the volume's colours, carried by the vertices
