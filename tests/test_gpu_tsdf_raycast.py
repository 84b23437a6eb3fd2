"""-m gpu: the surface views on the device (csrc/sp_raycast.hip) against the NumPy restatement of tests/tsdf_raycast_ref.py, word for word:
the volumes are made by the NumPy references on the host and uploaded, so nothing here depends on sp_tsdf_integrate; cameras in front of,
inside, beside and far from the volume (the reference marches every k, the kernel clips the ray against the box: a wrong clip shows here),
holes and odd nodes, the smallest volume, partial tiles, other steps, every subset of the outputs; then ``render_surface`` /
``score_surface`` / ``score_surface_images`` on a fused plane, and ``score_map`` / ``score_map_images`` against what they computed before
their tails were shared."""
import itertools

import numpy as np
import pytest
import torch

import tsdf_raycast_ref as ref
from gpu_util import T, dev, npy

pytestmark = pytest.mark.gpu

H, W = 24, 32
OUTPUTS = ('depth', 'normals', 'image', 'index')
SENTINEL = -7


def _device_volume(vol):
    return dict(tsdf=T(vol.tsdf), weight=T(vol.weight), colour=None if vol.colour is None else T(vol.colour), origin=vol.origin, voxel=vol.voxel,
                trunc=4 * vol.voxel, dims=vol.dims)


def _raw(vol, Ks, poses, h, w, z_start, step, n_steps, outputs=OUTPUTS):
    """One sp_tsdf_raycast call; the outputs asked for are pre-filled with a sentinel, the others are NULL."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    d = _device_volume(vol)
    nx, ny, nz = d['dims']
    V = len(poses)
    views = torch.cat((T(np.asarray(Ks, np.float32).reshape(V, 9)), T(np.asarray(poses, np.float32).reshape(V, 16))), dim=1).contiguous()
    shapes = dict(depth=((V, h, w), torch.float32), normals=((V, h, w, 3), torch.float32), image=((V, h, w, 3), torch.uint8), index=((V, h, w), torch.int32))
    out = {k: torch.full(shapes[k][0], SENTINEL % 256 if k == 'image' else SENTINEL, dtype=shapes[k][1], device=dev()) for k in outputs}
    _lib.check(lib.sp_tsdf_raycast(_lib.ptr(d['tsdf']), _lib.ptr(d['weight']), _lib.ptr(d['colour']), nx, ny, nz, vol.voxel, *vol.origin, vol.min_weight,
                                   _lib.ptr(views), V, h, w, z_start, step, n_steps, *(_lib.ptr(out.get(k)) for k in OUTPUTS), _lib.stream_ptr()),
               "sp_tsdf_raycast")
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


def _check(vol, Ks, poses, h, w, steps, what, outputs=None):
    outputs = outputs or tuple(k for k in OUTPUTS if k != 'image' or vol.colour is not None)
    want = ref.raycast(vol, Ks, poses, h, w, **steps)
    got = _raw(vol, Ks, poses, h, w, outputs=outputs, **steps)
    _same_words(got, want, what)
    return got, want


@pytest.fixture(scope="module")
def main():
    return ref.main_volume()


@pytest.mark.parametrize("name", ["front", "inside", "away", "oblique", "grazing", "far", "behind"])
def test_a_camera_on_the_main_volume_equals_the_reference_bit_for_bit(main, name):
    case, vol = main
    K, pose, steps = ref.cameras()[name]
    got, want = _check(vol, K[None], pose[None], H, W, steps, name)
    counts = want['counts'][0]
    print(f"\n{name}: {counts}")
    assert int((got['index'] >= 0).sum()) == counts['hits']
    if name in ('away', 'behind'):
        assert counts['hits'] == 0 and bool((got['depth'] == 0).all()) and bool(torch.isnan(got['normals']).all()) and bool((got['image'] == 0).all())
    else:
        assert counts['hits'] > 0 and counts['ended_without_hit'] > 0


def test_three_views_in_one_call_and_two_runs_give_the_same_bits(main):
    case, vol = main
    got, want = _check(vol, case['Ks'], case['poses'], H, W, ref.MAIN_STEPS, "three views")
    assert [int((got['index'][v] >= 0).sum()) for v in range(3)] == [451, 279, 0]
    again = _raw(vol, case['Ks'], case['poses'], H, W, **ref.MAIN_STEPS)
    for key in OUTPUTS:
        a, b = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (got[key], again[key]))
        assert torch.equal(a, b), key


def test_every_subset_of_the_outputs_leaves_the_given_ones_unchanged(main):
    case, vol = main
    want = ref.raycast(vol, case['Ks'][:2], case['poses'][:2], H, W, **ref.MAIN_STEPS)
    for n in range(1, 5):
        for subset in itertools.combinations(OUTPUTS, n):
            got = _raw(vol, case['Ks'][:2], case['poses'][:2], H, W, outputs=subset, **ref.MAIN_STEPS)
            assert set(got) == set(subset)
            _same_words(got, want, f"outputs {subset}")                        # (equal to the reference everywhere: every sentinel was overwritten)
    assert not (want['depth'] == SENTINEL).any() and not (want['index'] == SENTINEL).any()


@pytest.mark.parametrize("which", ["holed", "odd", "odd on its nodes"])
def test_holes_and_odd_nodes(which):
    case, vol = ref.holed_volume() if which == "holed" else ref.odd_volume()
    steps = ref.ON_NODES if which == "odd on its nodes" else ref.MAIN_STEPS
    got, want = _check(vol, case['K'], case['pose'], H, W, steps, which)
    hits = int((got['index'] >= 0).sum())
    assert 0 < hits < 560 and want['counts'][0]['nan_normals'] > 176           # fewer hits and more NaN normals than the whole plane has
    if which == "odd on its nodes":
        assert int(((got['depth'] == 1.6875) & (got['index'] >= 0)).sum()) >= 4    # F = 0 exactly is positive: t = 0 at the next sample


def test_the_smallest_volume_in_a_view_of_partial_tiles():
    vol, K, pose = ref.minimum_volume()
    got, want = _check(vol, K[None], pose[None], 9, 11, dict(z_start=0.0, step=0.0625, n_steps=30), "2 x 2 x 2 nodes, 9 x 11 pixels")
    assert want['counts'][0]['hits'] > 20 and bool(torch.isnan(got['normals']).all())
    # the main volume in the same small view: partial tiles on both axes, hits with normals
    case, main_vol = ref.main_volume()
    K = np.array([[10.0, 0, 5.0], [0, 10.0, 4.0], [0, 0, 1]], np.float32)
    got, want = _check(main_vol, K[None], case['poses'][:1], 9, 11, ref.MAIN_STEPS, "14 x 12 x 10 nodes, 9 x 11 pixels")
    assert want['counts'][0]['hits'] > 20 and want['counts'][0]['nan_normals'] < want['counts'][0]['hits']


@pytest.mark.parametrize("step, n_steps", [(0.0625, 50), (0.1875, 17)])
def test_other_steps(main, step, n_steps):
    case, vol = main
    got, want = _check(vol, case['Ks'][:2], case['poses'][:2], H, W, dict(z_start=0.03125, step=step, n_steps=n_steps), f"step {step}")
    assert all(c['hits'] > 100 for c in want['counts'])


def test_a_volume_without_colour(main):
    case, coloured = main
    vol = ref.main_volume(colour=False)[1]
    got, want = _check(vol, case['Ks'], case['poses'], H, W, ref.MAIN_STEPS, "no colour")
    assert set(got) == {'depth', 'normals', 'index'} and want['image'] is None
    from super_primitive_amd.tool import viz
    out = viz.tsdf_raycast(_device_volume(vol), T(case['Ks']), T(case['poses']), H, W, 3.0, z_min=0.0)       # the image: silently off
    assert set(out) == {'depth', 'normals', 'index'}
    _same_words(out, want, "viz.tsdf_raycast without colour")
    with pytest.raises(ValueError, match="colour"):
        viz.tsdf_raycast(_device_volume(vol), T(case['Ks']), T(case['poses']), H, W, 3.0, image=True)
    full = viz.tsdf_raycast(_device_volume(coloured), T(case['Ks']), T(case['poses']), H, W, 3.0, z_min=0.0)
    _same_words(full, ref.raycast(coloured, case['Ks'], case['poses'], H, W, **ref.MAIN_STEPS), "viz.tsdf_raycast")


# ---- the Python level -------------------------------------------------------------------------------------------------------------------------
def test_a_fused_plane_is_rendered_and_scored_at_its_depth():
    """``fuse_tsdf`` of the fronto-parallel plane of tests/test_tsdf_raycast_host.py, then the surface functions from the same camera.  The
    bound is that test's: trunc 2^-20 (in the metric's unit, 1000 trunc 2^-20 mm)."""
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    case = ref.plane_case(1.7)
    lo = case['origin']
    hi = tuple(o + n * case['voxel'] for o, n in zip(lo, case['dims']))
    depth, K, pose, images = T(case['depth']), T(case['K']), T(case['pose']), T(case['images'])
    vol = results.fuse_tsdf(depth, K, pose, case['voxel'], bounds=(lo, hi), images=images, trunc=case['trunc'])
    assert vol['dims'] == case['dims']
    for key in ('tsdf', 'weight', 'colour'):                                   # (the volume the reference made: the rest compares like with like)
        assert np.array_equal(npy(vol[key]).view(np.uint32), getattr(case['volume'], key).view(np.uint32)), key
    size, z_max = (case['H'], case['W']), 3.0
    out = results.render_surface(vol, K, pose, size, z_max)
    assert set(out) == set(OUTPUTS)
    hit = out['index'] >= 0
    bound = case['trunc'] * 2.0 ** -20
    err = float((out['depth'][hit].double() - float(np.float32(1.7))).abs().max())
    print(f"\nfused plane: {int(hit.sum())} hits; largest |depth - 1.7| {err:.3e} (bound {bound:.3e})")
    assert int(hit.sum()) == 560 and err <= bound
    nrm = out['normals'][hit]
    whole = ~torch.isnan(nrm).any(dim=1)
    assert int(whole.sum()) > 300 and float((nrm[whole].double() - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64, device=dev())).abs().max()) <= 2.0 ** -20
    # the same call by the rule: z_start is the float32 of viz.Z_MIN, n_steps = ceil((z_max - z_min) / step) + 1
    n_steps = int(np.ceil((z_max - viz.Z_MIN) / case['voxel'])) + 1
    want = ref.raycast(case['volume'], case['K'], case['pose'], *size, z_start=viz.Z_MIN, step=case['voxel'], n_steps=n_steps)
    _same_words(out, want, "render_surface")
    score = results.score_surface(vol, depth, K, pose)
    col = {name: k for k, name in enumerate(score['columns'])}
    m = npy(score['metrics'])[0]
    print(f"score_surface: coverage {float(score['coverage'][0]):.4f}, n {m[col['n']]:.0f}, rmse {m[col['rmse']]:.3e} mm")
    assert float(score['coverage'][0]) == 560 / (case['H'] * case['W']) and m[col['n']] == 560
    assert m[col['rmse']] <= 1000.0 * bound
    # the image that coloured the volume, from the same single camera
    scored = results.score_surface_images(vol, images, K, pose, z_max)
    sums = viz.image_metrics(T(want['image']), images, T(want['index']))
    print(f"score_surface_images: sums {scored['sums'].tolist()}, psnr {float(scored['psnr'][0]):.2f} dB, l1 {float(scored['l1'][0]):.2f}")
    assert torch.equal(scored['sums'], sums) and int(sums[0, 0]) == 560
    assert bool(torch.isfinite(scored['psnr']).all()) and float(scored['coverage'][0]) == 560 / (case['H'] * case['W'])


def test_score_map_and_score_map_images_give_the_bits_they_gave_before_their_tails_were_shared():
    from super_primitive_amd.depth_completion import void
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    rng = np.random.default_rng(21)
    Q, V, h, w = 4000, 2, 30, 40
    pts = np.stack([rng.uniform(-1.0, 1.0, Q), rng.uniform(-0.8, 0.8, Q), rng.uniform(1.0, 3.0, Q)], axis=1).astype(np.float32)
    world = dict(points=T(pts), colours=T(rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)))
    K = T(np.array([[30.0, 0, 19.5], [0, 30.0, 14.5], [0, 0, 1]], np.float32))
    poses = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    poses[1, :3, 3] = (0.1, -0.05, 0.2)
    poses = T(poses)
    gt = rng.uniform(0.1, 6.0, (V, h, w)).astype(np.float32)                   # some below min_depth, some beyond max_depth
    gt[0, 3, 4:9] = np.nan
    gt, images = T(gt), T(rng.uniform(0.0, 1.0, (V, 3, h, w)).astype(np.float32))
    radii = torch.full((Q,), 0.02, dtype=torch.float32, device=dev())
    bits = lambda t: t.contiguous().view(torch.int64)
    for kw in (dict(), dict(radii=radii, max_px=4)):
        got = results.score_map(world, gt, K, poses, min_depth=0.2, max_depth=5.0, **kw)
        # the expressions of score_map as they stood
        depth = viz.render_views(world['points'], None, K, poses, h, w, depth_buffer=True, image=False, index=False, radii=kw.get('radii'),
                                 max_px=kw.get('max_px', 8), normals=None, cull=False)['depth']
        in_range = (gt >= 0.2) & (gt <= 5.0)
        scored = in_range & (depth > 0)
        metrics = void.depth_metrics(depth, gt, scored)
        coverage = scored.sum(dim=(1, 2)).double() / in_range.sum(dim=(1, 2)).double()
        assert set(got) == {'metrics', 'columns', 'coverage'} and got['columns'] == void._COLUMNS
        assert torch.equal(bits(got['metrics']), bits(metrics)) and torch.equal(bits(got['coverage']), bits(coverage))
        assert float(metrics[0, 0]) > 50
        got = results.score_map_images(world, images, K, poses, **kw)
        # the expressions of score_map_images as they stood
        out = viz.render_views(world['points'], world['colours'], K, poses, h, w, depth_buffer=True, depth=False, radii=kw.get('radii'),
                               max_px=kw.get('max_px', 8), normals=None, cull=False)
        sums = viz.image_metrics(out['image'], images, out['index'])
        n3, s1, s2 = 3.0 * sums[:, 0].double(), sums[:, 1].double(), sums[:, 2].double()
        want = dict(sums=sums, psnr=10.0 * torch.log10(255.0 ** 2 * n3 / s2), l1=s1 / n3, coverage=sums[:, 0].double() / float(h * w))
        assert set(got) == set(want)
        for key in want:
            assert torch.equal(bits(got[key]), bits(want[key])), key
