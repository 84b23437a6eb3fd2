"""-m gpu: footprints through the depth buffer and the image score (csrc/sp_views.hip: sp_render_splats, sp_image_metrics, through
``tool/viz.py`` and ``odometery/results.py``) against the float64 statements of tests/map_splat_ref.py.

What is compared how.  With the identity pose the kernel's float64 arithmetic is NumPy's, operation for operation: image, depth and
index are compared BITWISE on every pixel.  For posed views the pixels of the two ambiguity masks (position taint, depth-tie taint:
tests/map_splat_ref.py; at most 2 % of a view, asserted on every posed view by tests/test_map_splat_ref_host.py) are left out and the
rest is compared bitwise too.  The image score is integers: exact.

Excluded pixels per posed view (of the statement's inputs; the device agreed on every other pixel): splat_posed 0, 0, 0;
splat_collide view 1: 4 of 768; splat_views17: 0 in all 17."""
import functools

import numpy as np
import pytest
import torch

import map_render_ref as base
import map_splat_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)[None]


@functools.lru_cache(maxsize=None)
def _case(name):
    return ref.CASES[name]()


@functools.lru_cache(maxsize=None)
def _want(name, k):
    """The statement's (image, depth, index) of view k and the mask of the pixels to compare; made once per (case, view)."""
    c = _case(name)
    pose = None if 'poses' not in c else c['poses'][k]
    want = ref.render(c['points'], c['colours'], c['radii'], c['K'], pose, c['H'], c['W'], c['max_px'])
    mask = np.ones((c['H'], c['W']), bool)
    if not ref.is_identity(pose):
        args = (c['points'], c['radii'], c['K'], pose, c['H'], c['W'], c['max_px'])
        mask &= ~(ref.position_taint(*args) | ref.depth_tie_taint(*args))
    return want, mask


def _render(c, radii="own", **kw):
    from super_primitive_amd.tool import viz
    rad = c['radii'] if isinstance(radii, str) else radii
    extra = {} if rad is None else dict(radii=T(rad), max_px=c.get('max_px', 8))
    out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', EYE)), c['H'], c['W'], depth_buffer=True, **extra, **kw)
    return {k: npy(v) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _compare(name, out):
    c = _case(name)
    excluded = []
    for k in range(len(c.get('poses', EYE))):
        (image, depth, index), mask = _want(name, k)
        excluded.append(int((~mask).sum()))
        assert mask.mean() >= 0.98
        np.testing.assert_array_equal(out['index'][k][mask], index[mask], err_msg=f"{name} view {k}: index")
        np.testing.assert_array_equal(out['image'][k][mask], image[mask], err_msg=f"{name} view {k}: image")
        np.testing.assert_array_equal(_bits(out['depth'][k])[mask], _bits(depth)[mask], err_msg=f"{name} view {k}: depth")
    print(f"\n{name}: pixels excluded per view {excluded}; coverage {[round(float((out['index'][k] >= 0).mean()), 3) for k in range(len(excluded))]}")


@pytest.mark.parametrize("make", [base.case_posed, lambda: base.case_duplicates()[0]], ids=["posed", "duplicates"])
def test_radius0_is_the_point_render_on_every_pixel(make):
    """Case 1: all radii 0 -- sp_render_views in mode 1, bit for bit; no reference is involved."""
    c = make()
    want = _render(c, radii=None)
    for max_px in (0, 3, 16):
        got = _render(dict(c, max_px=max_px), radii=np.zeros(len(c['points']), np.float32))
        for key in ('image', 'depth', 'index'):
            assert np.array_equal(_bits(got[key]), _bits(want[key])), (max_px, key)
    assert (want['index'] >= 0).sum() > 100


def _raw_splats(name, image=True, depth=True, index=True):
    """sp_render_splats on keys and outputs pre-filled with junk: every pixel of every requested output has to be written."""
    from super_primitive_amd import _lib
    c = _case(name)
    poses = c.get('poses', EYE)
    V, H, W = len(poses), c['H'], c['W']
    views = T(np.concatenate([np.tile(c['K'].reshape(1, 9), (V, 1)), poses.reshape(V, 16)], axis=1).astype(np.float32))
    pts, cols, rad = T(c['points']), T(c['colours']), T(c['radii'])
    keys = torch.full((V * H * W,), -1, dtype=torch.int64, device=pts.device)
    out = dict(image=torch.full((V, H, W, 3), 0xAB, dtype=torch.uint8, device=pts.device) if image else None,
               depth=torch.full((V, H, W), 777.0, dtype=torch.float32, device=pts.device) if depth else None,
               index=torch.full((V, H, W), 12345, dtype=torch.int32, device=pts.device) if index else None)
    lib = _lib.load()
    _lib.check(lib.sp_render_splats(_lib.ptr(pts), _lib.ptr(cols), len(c['points']), _lib.ptr(views), V, H, W, 1e-6, _lib.ptr(rad), c['max_px'],
                                    _lib.ptr(keys), _lib.ptr(out['image']), _lib.ptr(out['depth']), _lib.ptr(out['index']), _lib.stream_ptr()),
               "sp_render_splats")
    torch.cuda.synchronize()
    return {k: None if v is None else npy(v) for k, v in out.items()}


def test_splat_posed():
    """Case 2: three posed views in one call, outputs pre-filled with junk; splats at the cap, half the cloud behind one camera, an
    empty view; each output left out in turn; two runs give the same bits."""
    c = _case("splat_posed")
    out = _raw_splats("splat_posed")
    _compare("splat_posed", out)
    points_only = _render(c, radii=None)
    for k in (0, 1):
        assert (out['index'][k] >= 0).mean() > (points_only['index'][k] >= 0).mean()
    assert (out['index'][1] >= 0).mean() > 0.99
    _, _, z1 = ref.project(c['points'], c['K'], c['poses'][1])
    assert (z1[out['index'][1][out['index'][1] >= 0]] > 0).all()
    assert not out['image'][2].any() and not out['depth'][2].any() and (out['index'][2] == -1).all()
    again = _raw_splats("splat_posed")
    for key in out:
        assert np.array_equal(_bits(out[key]), _bits(again[key])), key
    for left_out in ('image', 'depth', 'index'):
        part = _raw_splats("splat_posed", **{left_out: False})
        assert part[left_out] is None
        for key in out:
            if key != left_out:
                assert np.array_equal(_bits(part[key]), _bits(out[key])), (left_out, key)
    through_viz = _render(c)
    for key in out:
        assert np.array_equal(_bits(through_viz[key]), _bits(out[key])), key


def test_splat_collide():
    """Case 3: 70 001 points into 24 x 32, indices beyond 65 535, from the identity pose (bitwise everywhere) and from a posed view."""
    out = _render(_case("splat_collide"))
    _compare("splat_collide", out)
    assert _want("splat_collide", 0)[1].all()
    assert out['index'][0].max() > 65535 and (out['index'] > 65535).sum() >= 10


def test_splat_views17():
    """Case 4: 17 views, one more than a staging chunk."""
    out = _render(_case("splat_views17"))
    assert out['index'].shape == (17, 30, 40)
    _compare("splat_views17", out)
    assert (out['index'][16] >= 0).mean() > 0.2


def test_splat_edges():
    """Case 5: identity pose, bitwise: squares clipped by the border, missing it, at the cap; NaN, negative, infinite and zero radii;
    z = inf, z below z_min, NaN coordinates."""
    c = _case("splat_edges")
    out = _render(c)
    _compare("splat_edges", out)
    idx, R = out['index'][0], ref.EDGE_ROWS
    assert set(idx[idx >= 0].tolist()) == set(range(11)) - {R['misses'], R['below_z_min'], R['nan_point']}
    assert (idx == R['inf_radius']).sum() == 49 and (idx == R['corner']).sum() == 25 and (idx == R['reaches']).sum() == 3
    assert idx[7, 8] == R['z_inf'] and np.isinf(out['depth'][0, 7, 8])
    for q in (R['reaches'], R['misses']):                                      # Q = 1: a kept and a dropped single splat
        one = _render(dict(c, points=c['points'][q:q + 1], colours=c['colours'][q:q + 1], radii=c['radii'][q:q + 1]))
        assert int((one['index'] >= 0).sum()) == (3 if q == R['reaches'] else 0)


@pytest.mark.parametrize("footprint", [2.0, 3.0])
def test_plane_end_to_end(footprint):
    """Case 6: a plane sampled at every second pixel in both directions: the point render covers a quarter of the view, footprints of
    two source pixels all of it, every pixel within the bound of the ground truth; score_map reports it."""
    from super_primitive_amd.odometery.results import render_map, score_map
    c = ref.case_plane(footprint)
    H, W = c['H'], c['W']
    world = dict(points=T(c['points']), colours=T(c['colours']))
    K_mid, eye = T(c['K_mid']), T(EYE)
    plain = render_map(world, K_mid, eye, (H, W))
    assert float((plain['index'] >= 0).float().mean()) == 0.25
    out = render_map(world, K_mid, eye, (H, W), radii=T(c['radii']), max_px=c['max_px'])
    assert float((out['index'] >= 0).float().mean()) == 1.0
    err = np.abs(npy(out['depth'][0]).astype(np.float64) - c['gt'].astype(np.float64))
    print(f"\nplane, footprint {footprint}: worst error {err.max():.7f} (bound {c['bound']:.6f})")
    assert err.max() <= c['bound']
    want = ref.render(c['points'], c['colours'], c['radii'], c['K_mid'], None, H, W, c['max_px'])
    for key, w in zip(('image', 'depth', 'index'), want):
        np.testing.assert_array_equal(_bits(npy(out[key][0])), _bits(w))
    score = score_map(world, T(c['gt'][None]), K_mid, eye, radii=T(c['radii']), max_px=c['max_px'])
    assert float(score['coverage'][0]) == 1.0
    assert float(score_map(world, T(c['gt'][None]), K_mid, eye)['coverage'][0]) == 0.25


def _aligned(pose, rec):
    """apply_scale in float64: R' = rot_reanchor R, t' = s rot t + trans_scaled."""
    P = pose.astype(np.float64)
    if rec is not None:
        P = P.copy()
        P[:3, 3] = rec['s'] * (rec['rot'] @ pose[:3, 3].astype(np.float64)) + rec['trans_scaled']
        P[:3, :3] = rec['rot_reanchor'] @ pose[:3, :3].astype(np.float64)
    return P


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("with_align", [False, True], ids=["plain", "aligned"])
def test_point_radii(stride, with_align):
    """Case 7: two keyframes (12 x 20 and 24 x 40) with poses, with and without an alignment record: the radii against the float64
    formula at 8 * 2^-24 * footprint / (2 fx) * (|p|_1 + |c|_1); splats of those radii seen from the keyframe's own camera cover at least
    what the points cover."""
    from test_gpu_map_points import _pose, _scene
    from super_primitive_amd.odometery.results import keyframe_points, point_radii, render_map
    from super_primitive_amd.tool.pose_utils import record_views
    kfs, klds, _ = _scene()
    kfs, klds = [kfs[0], kfs[2]], [klds[0], klds[2]]
    rng = np.random.default_rng(8)
    poses = np.stack([_pose(rng) for _ in kfs])
    rec, align = None, None
    if with_align:
        rec = dict(rot=_pose(rng)[:3, :3].astype(np.float64), trans_scaled=rng.uniform(-3, 3, 3), s=0.37, rot_reanchor=_pose(rng)[:3, :3].astype(np.float64))
        record = np.zeros((1, 32))
        record[0, 0:9], record[0, 9:12], record[0, 15], record[0, 16:25] = rec['rot'].reshape(-1), rec['trans_scaled'], rec['s'], rec['rot_reanchor'].reshape(-1)
        record_d = T(record)
        align = dict(record=record_d, **record_views(record_d))
    world = keyframe_points(kfs, klds, T(poses), stride=stride, align=align)
    world['ids'] = [4, 9]
    if with_align:
        world['align'] = align
    result = dict(kf_archive={i: dict(kf=kf, kld=kld, pose=T(poses[k])) for k, (i, kf, kld) in enumerate(zip(world['ids'], kfs, klds))})
    footprint = 1.5
    radii = point_radii(world, result, footprint=footprint)
    assert radii.dtype == torch.float32 and tuple(radii.shape) == (world['points'].shape[0],)
    p = npy(world['points']).astype(np.float64)
    worst = 0.0
    for k, kf in enumerate(kfs):
        a0, a1 = int(world['offsets'][k]), int(world['offsets'][k + 1])
        P = _aligned(poses[k], rec)
        fx = float(npy(kf.K).reshape(-1)[0])
        want = footprint / (2.0 * fx) * ((p[a0:a1] - P[:3, 3]) @ P[:3, 2])
        bound = 8.0 * 2.0 ** -24 * footprint / (2.0 * fx) * (np.abs(p[a0:a1]).sum(1) + np.abs(P[:3, 3]).sum())
        err = np.abs(npy(radii[a0:a1]).astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (k, float((err / bound).max()))
        assert (want > 0).all()
        H, W = kf.image.shape[1:]
        cam = dict(Ks=kf.K, poses=T(P.astype(np.float32)[None]), size=(H, W))
        dots = npy(render_map(world, **cam)['index'][0]) >= 0
        splats = npy(render_map(world, radii=radii, **cam)['index'][0]) >= 0
        assert dots.sum() > 0 and (splats | ~dots).all() and splats.sum() >= dots.sum()
    print(f"\npoint_radii stride {stride} {'aligned' if with_align else 'plain'}: worst error {worst:.3f} of the bound")
    assert torch.equal(point_radii(world, result, footprint=3.0), 2.0 * radii)       # (a power of two: the radius is linear in the footprint)


@pytest.mark.parametrize("shape", [(3, 19, 23), (1, 64, 80)], ids=["3x19x23", "1x64x80"])
def test_image_metrics(shape):
    """Case 8: random views, an index with -1 in about a third of the pixels (one view all -1), targets beyond 0..1 and NaN: the sums
    are the NumPy integers exactly."""
    from super_primitive_amd.tool import viz
    V, H, W = shape
    rendered, target, index = ref.metrics_inputs(V, H, W, 204 + V)
    if V == 3:
        index[1] = -1
    want = ref.image_metrics(rendered, target, index)
    got = viz.image_metrics(T(rendered), T(target), T(index))
    assert got.dtype == torch.int64 and tuple(got.shape) == (V, 3)
    np.testing.assert_array_equal(npy(got), want)
    from super_primitive_amd import _lib
    a, b, i = T(rendered), T(target), T(index)
    out = torch.full((V, 3), -7, dtype=torch.int64, device=a.device)            # the call zeroes its output
    _lib.check(_lib.load().sp_image_metrics(_lib.ptr(a), _lib.ptr(b), _lib.ptr(i), V, H, W, _lib.ptr(out), _lib.stream_ptr()), "sp_image_metrics")
    np.testing.assert_array_equal(npy(out), want)
    assert want[0, 0] > 0 and np.isnan(target).any() and (V == 1 or not want[1].any())
    if V == 1:
        assert H * W > 4 * 1024                                                 # more than one workgroup per view


def test_score_map_images():
    """Case 8, through ``score_map_images``: a view against its own image has sum d^2 = 0 and psnr = inf; an empty view NaN; a shifted
    target the NumPy figures."""
    from super_primitive_amd.odometery.results import render_map, score_map_images
    c = _case("splat_posed")
    world = dict(points=T(c['points']), colours=T(c['colours']))
    K, poses, rad = T(c['K']), T(c['poses']), T(c['radii'])
    views = render_map(world, K, poses, (c['H'], c['W']), radii=rad, max_px=c['max_px'])
    own = ((npy(views['image']).astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).transpose(0, 3, 1, 2)     # trunc(c * 255) gives the byte back
    score = score_map_images(world, T(own), K, poses, radii=rad, max_px=c['max_px'])
    sums, psnr = npy(score['sums']), npy(score['psnr'])
    n = (npy(views['index']) >= 0).reshape(3, -1).sum(1)
    np.testing.assert_array_equal(sums[:, 0], n)
    assert not sums[:, 1:].any() and n[2] == 0
    assert np.isinf(psnr[0]) and np.isinf(psnr[1]) and np.isnan(psnr[2]) and np.isnan(npy(score['l1'])[2])
    np.testing.assert_allclose(npy(score['coverage']), n / float(c['H'] * c['W']), rtol=2.0 ** -51, atol=0)      # (one float64 division)
    rng = np.random.default_rng(205)
    other = rng.uniform(0, 1, own.shape).astype(np.float32)
    score = score_map_images(world, T(other), K, poses, radii=rad, max_px=c['max_px'])
    want = ref.image_metrics(npy(views['image']), other, npy(views['index']))
    np.testing.assert_array_equal(npy(score['sums']), want)
    for k in (0, 1):
        np.testing.assert_allclose(npy(score['psnr'])[k], 10 * np.log10(255.0 ** 2 * 3 * want[k, 0] / want[k, 2]), rtol=1e-12)
        np.testing.assert_allclose(npy(score['l1'])[k], want[k, 1] / (3.0 * want[k, 0]), rtol=1e-12)
    # without radii: the point render's pixels only
    dots = score_map_images(world, T(other), K, poses)
    assert float(dots['coverage'][0]) < float(score['coverage'][0])
