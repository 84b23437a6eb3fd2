"""-m gpu: the map views (csrc/sp_views.hip through ``tool/viz.py`` and ``odometery/results.py`` ``render_map`` / ``score_map``) against
the float64 statements of tests/map_render_ref.py and, for the reference's own mode, the image the real ``render_pcd`` returned (golden
g_render_pcd).

What is compared how.  With the identity pose the kernel's float64 arithmetic is NumPy's, operation for operation: image, depth and
index are compared BITWISE on every pixel.  For posed views the pixels of the two ambiguity masks (position taint, depth-tie taint:
tests/map_render_ref.py; at most 2 % of a view, tests/test_map_render_ref_host.py) are left out and the rest is compared bitwise too --
depth included: z is a sum of float64 products formed in the statement's order, so float32(z) agrees bit for bit, which is stricter
than the rtol 2e-6 tests/test_gpu_segment_depth.py uses for the same quantity.
The lift: counts, offsets, pixel and colours exactly; points within 2^-23 relative of the float64 statement (the kernel forms the
statement's float64 operations in the statement's order and rounds to float32 once: half an ulp, 2^-24)."""
import functools

import numpy as np
import pytest
import torch

import map_render_ref as ref
from conftest import load_golden
from map_splat_ref import case_splat_views17
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)[None]
LIFT_RTOL = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "duplicates":
        return ref.case_duplicates()[0]
    return dict(golden0=ref.case_golden0, collide=ref.case_collide, posed=ref.case_posed, edges=ref.case_edges, views17=case_splat_views17)[name]()


@functools.lru_cache(maxsize=None)
def _want(name, k, mode):
    """The statement's (image, depth, index) of view k and the mask of the pixels to compare; made once per (case, view, mode)."""
    c = _case(name)
    pose = None if 'poses' not in c else c['poses'][k]
    want = ref.render(c['points'], c['colours'], c['K'], pose, c['H'], c['W'], mode)
    mask = np.ones((c['H'], c['W']), bool)
    if not ref.is_identity(pose):
        mask &= ~ref.position_taint(c['points'], c['K'], pose, c['H'], c['W'])
        if mode == 1:
            mask &= ~ref.depth_tie_taint(c['points'], c['K'], pose, c['H'], c['W'])
    return want, mask


def _render(name, mode, **kw):
    from super_primitive_amd.tool import viz
    c = _case(name)
    out = viz.render_views(T(c['points']), T(c['colours']), T(c['K']), T(c.get('poses', EYE)), c['H'], c['W'], depth_buffer=bool(mode), **kw)
    return {k: npy(v) for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _compare(name, mode, out):
    c = _case(name)
    for k in range(len(c.get('poses', EYE))):
        (image, depth, index), mask = _want(name, k, mode)
        assert mask.mean() >= 0.98
        np.testing.assert_array_equal(out['index'][k][mask], index[mask], err_msg=f"{name} view {k} mode {mode}: index")
        np.testing.assert_array_equal(out['image'][k][mask], image[mask], err_msg=f"{name} view {k} mode {mode}: image")
        np.testing.assert_array_equal(_bits(out['depth'][k])[mask], _bits(depth)[mask], err_msg=f"{name} view {k} mode {mode}: depth")


def test_mode0_is_the_reference_render_pcd_bitwise():
    """Case 1: 5003 points (20 workgroups, the last one partial) into 37 x 53, z over [-0.5, 4]."""
    from super_primitive_amd.tool import viz
    c, g = _case("golden0"), load_golden("g_render_pcd")
    image = viz.render_pcd(T(c['points']), T(c['colours']), T(c['K']), c['H'], c['W'])
    assert image.dtype == torch.uint8 and tuple(image.shape) == (37, 53, 3)
    np.testing.assert_array_equal(npy(image), g["golden0_image"])
    image2, depth, index = viz.render_pcd(T(c['points']), T(c['colours']), T(c['K']), c['H'], c['W'], return_maps=True)
    assert depth.dtype == torch.float32 and index.dtype == torch.int32 and torch.equal(image, image2)
    _compare("golden0", 0, dict(image=npy(image2)[None], depth=npy(depth)[None], index=npy(index)[None]))
    idx = npy(index)
    assert (c['points'][idx[idx >= 0], 2] < 0).sum() >= 2                     # points behind the camera won pixels, as in the reference
    # the depth buffer on the same input drops them
    _, depth1, index1 = viz.render_pcd(T(c['points']), T(c['colours']), T(c['K']), c['H'], c['W'], depth_buffer=True, return_maps=True)
    _compare("golden0", 1, dict(image=npy(viz.render_pcd(T(c['points']), T(c['colours']), T(c['K']), c['H'], c['W'], depth_buffer=True))[None],
                                depth=npy(depth1)[None], index=npy(index1)[None]))
    assert float(depth1[index1 >= 0].min()) > 1e-6


@pytest.mark.parametrize("mode", [0, 1])
def test_heavy_collisions(mode):
    """Case 2: 70 001 points into 24 x 32, about 90 per pixel, indices beyond 65 535."""
    out = _render("collide", mode)
    _compare("collide", mode, out)
    if mode == 0:
        np.testing.assert_array_equal(out['image'][0], load_golden("g_render_pcd")["collide_image"])
        assert out['index'].max() > 65535
    else:
        assert (out['index'] > 65535).sum() >= 10                            # the index half of the key is in use beyond 16 bits


def test_depth_buffer_with_exact_duplicates_and_one_float32_z():
    """Case 3: duplicates at low and high indices, and two float64 z behind one float32(z): the index decides."""
    _, (r, c) = ref.case_duplicates()
    out = _render("duplicates", 1)
    _compare("duplicates", 1, out)
    assert out['index'][0, r, c] == 551 and out['depth'][0, r, c] == np.float32(9.0)
    _compare("duplicates", 0, _render("duplicates", 0))


def _raw_render(name, mode, image=True, depth=True, index=True):
    """sp_render_views on outputs pre-filled with junk: every pixel of every requested output has to be written."""
    from super_primitive_amd import _lib
    c = _case(name)
    poses = c.get('poses', EYE)
    V, H, W = len(poses), c['H'], c['W']
    views = T(np.concatenate([np.tile(c['K'].reshape(1, 9), (V, 1)), poses.reshape(V, 16)], axis=1).astype(np.float32))
    pts, cols = T(c['points']), T(c['colours'])
    keys = torch.full((V * H * W,), -1, dtype=torch.int64, device=pts.device)
    out = dict(image=torch.full((V, H, W, 3), 0xAB, dtype=torch.uint8, device=pts.device) if image else None,
               depth=torch.full((V, H, W), 777.0, dtype=torch.float32, device=pts.device) if depth else None,
               index=torch.full((V, H, W), 12345, dtype=torch.int32, device=pts.device) if index else None)
    lib = _lib.load()
    _lib.check(lib.sp_render_views(_lib.ptr(pts), _lib.ptr(cols), len(c['points']), _lib.ptr(views), V, H, W, mode, 1e-6, _lib.ptr(keys),
                                   _lib.ptr(out['image']), _lib.ptr(out['depth']), _lib.ptr(out['index']), _lib.stream_ptr()), "sp_render_views")
    torch.cuda.synchronize()
    return {k: None if v is None else npy(v) for k, v in out.items()}


@pytest.mark.parametrize("name,mode", [("posed", 0), ("posed", 1), ("views17", 0), ("views17", 1)], ids=["0", "1", "views17-0", "views17-1"])
def test_three_posed_views_in_one_call(name, mode):
    """Case 4: one view looks at the cloud, one has half of it behind, one sees nothing; outputs pre-filled with junk.  views17: the 17
    views and 300 points of map_splat_ref.case_splat_views17 as points (radii ignored): one view more than the key pass stages at a time."""
    c = _case(name)
    out = _raw_render(name, mode)
    _compare(name, mode, out)
    if name == "views17":
        assert out['index'].shape == (17, 30, 40) and (_want(name, 16, mode)[0][2] >= 0).any()      # the view of the second chunk sees points
        return
    _, _, z1 = ref.project(c['points'], c['K'], c['poses'][1])
    won = out['index'][1][out['index'][1] >= 0]
    if mode == 0:
        assert (z1[won] < 0).sum() >= 20                                     # the reference's mode keeps points behind the camera
    else:
        assert len(won) > 50 and (z1[won] > 0).all()
    assert not out['image'][2].any() and not out['depth'][2].any() and (out['index'][2] == -1).all()
    assert (out['index'][0] >= 0).mean() > 0.3


@pytest.mark.parametrize("mode", [0, 1])
def test_smallest_and_non_finite_inputs(mode):
    """Case 5: the border (u = 0 kept, u = W dropped), NaN and inf coordinates, a NaN colour, z = inf; and Q = 1."""
    from super_primitive_amd.tool import viz
    c = _case("edges")
    out = _render("edges", mode)
    _compare("edges", mode, out)
    idx = out['index'][0]
    assert set(idx[idx >= 0].tolist()) == ({0, 7, 8, 9, 10} if mode == 0 else {0, 7, 8, 9})
    assert idx[8, 0] == 0 and 1 not in idx and idx[7, 8] == 7 and np.isinf(out['depth'][0, 7, 8])
    r8, c8 = np.argwhere(idx == 8)[0]
    assert out['image'][0, r8, c8].tolist() == [0, 127, 0]                   # NaN channels give 0
    for q in (0, 1):                                                         # a kept and a dropped single point
        one = viz.render_views(T(c['points'][q:q + 1]), T(c['colours'][q:q + 1]), T(c['K']), T(EYE), c['H'], c['W'], depth_buffer=bool(mode))
        want = ref.render(c['points'][q:q + 1], c['colours'][q:q + 1], c['K'], None, c['H'], c['W'], mode)
        for key, w in zip(('image', 'depth', 'index'), want):
            np.testing.assert_array_equal(npy(one[key][0]), w)
        assert int((one['index'] >= 0).sum()) == 1 - q


def test_nullable_outputs_and_determinism():
    """Case 6: each output left out in turn; two runs give the same bits."""
    for mode in (0, 1):
        full = _raw_render("posed", mode)
        again = _raw_render("posed", mode)
        for key in full:
            assert np.array_equal(_bits(full[key]), _bits(again[key])), (mode, key)
        for left_out in ('image', 'depth', 'index'):
            part = _raw_render("posed", mode, **{left_out: False})
            assert part[left_out] is None
            for key in full:
                if key != left_out:
                    assert np.array_equal(_bits(part[key]), _bits(full[key])), (mode, left_out, key)
    a, b = _render("collide", 1), _render("collide", 1)
    assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)
    from super_primitive_amd.tool import viz
    c = _case("posed")
    only = viz.render_views(T(c['points']), None, T(c['K']), T(c['poses']), c['H'], c['W'], depth_buffer=True, image=False, index=False)
    assert set(only) == {'depth'} and np.array_equal(_bits(npy(only['depth'])), _bits(_raw_render("posed", 1)['depth']))


def _check_lift(got, want, cap):
    n = int(want['offsets'][-1])
    np.testing.assert_array_equal(npy(got['counts']), want['counts'])
    np.testing.assert_array_equal(npy(got['offsets']), want['offsets'])
    assert got['counts'].dtype == torch.int32 and got['offsets'].dtype == torch.int64 and got['pixel'].dtype == torch.int32
    assert tuple(got['points'].shape) == (cap, 3) and tuple(got['colours'].shape) == (cap, 3) and tuple(got['pixel'].shape) == (cap,)
    np.testing.assert_array_equal(npy(got['pixel'])[:n], want['pixel'])
    np.testing.assert_array_equal(npy(got['colours'])[:n], want['colours'])
    p = npy(got['points'])[:n].astype(np.float64)
    err = np.abs(p - want['points'])
    print(f"\nlift: {n} of {cap} pixels valid; max relative error of a coordinate {float((err / np.maximum(np.abs(want['points']), 1e-300)).max()):.2e} (bound {LIFT_RTOL:.2e})")
    assert np.all(err <= LIFT_RTOL * np.abs(want['points']))
    np.testing.assert_array_equal(p.astype(np.float32), want['points'].astype(np.float32))     # in fact the statement, rounded once


def _raw_lift(depth, K, poses, image):
    """sp_depth_lift on capacity buffers pre-filled with junk."""
    from super_primitive_amd import _lib
    B, H, W = depth.shape
    lib = _lib.load()
    d, Kd, Td, img = T(depth), T(K.reshape(B, 9)), T(poses.reshape(B, 16)), T(image)
    dev, cap = d.device, B * H * W
    scratch = torch.full((lib.sp_depth_lift_blocks(B, H, W),), -7, dtype=torch.int32, device=dev)
    out = dict(points=torch.full((cap, 3), -7.0, device=dev), colours=torch.full((cap, 3), -7.0, device=dev),
               pixel=torch.full((cap,), -7, dtype=torch.int32, device=dev), counts=torch.full((B,), -7, dtype=torch.int32, device=dev),
               offsets=torch.full((B + 1,), -7, dtype=torch.int64, device=dev))
    _lib.check(lib.sp_depth_lift(_lib.ptr(d), _lib.ptr(Kd), _lib.ptr(Td), _lib.ptr(img), B, H, W, 100.0, _lib.ptr(scratch), _lib.ptr(out['points']),
                                 _lib.ptr(out['colours']), _lib.ptr(out['pixel']), _lib.ptr(out['counts']), _lib.ptr(out['offsets']),
                                 _lib.stream_ptr()), "sp_depth_lift")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("make", [ref.lift_case_small, ref.lift_case_single, ref.lift_case_blocks, ref.lift_case_blocks_odd],
                         ids=["3x19x23", "1x64x80", "3x150x150", "3x149x149"])
def test_depth_lift(make):
    """Case 7: 0, negative, NaN, inf and > depth_trunc depths, an all-invalid and an all-valid image; the capacity buffers keep their
    junk beyond offsets[B]."""
    from super_primitive_amd.tool import viz
    depth, K, poses, image = make()
    B, H, W = depth.shape
    want = ref.lift(depth, K, poses, image)
    n, cap = int(want['offsets'][-1]), B * H * W
    assert 0 < n < cap
    raw = _raw_lift(depth, K, poses, image)
    _check_lift(raw, want, cap)
    for key in ('points', 'colours', 'pixel'):
        assert bool((raw[key][n:] == -7).all()), key                         # rows at or beyond offsets[B] are never written
    got = viz.lift_depth_images(T(depth), T(K), T(poses), T(image))
    for key in ('counts', 'offsets'):
        assert torch.equal(got[key], raw[key]), key
    for key in ('points', 'colours', 'pixel'):
        assert got[key].shape == raw[key].shape and torch.equal(got[key][:n], raw[key][:n]), key
    # without poses and colours: the camera-frame cloud
    plain = viz.lift_depth_images(T(depth), T(K))
    assert 'colours' not in plain and torch.equal(plain['offsets'], got['offsets']) and torch.equal(plain['pixel'][:n], got['pixel'][:n])
    cam = ref.lift(depth, K)
    np.testing.assert_array_equal(npy(plain['points'])[:n], cam['points'].astype(np.float32))
    # the trimmed single-image form and the reference's mask over the compacted rows
    b = B - 1
    a0, a1 = int(want['offsets'][b]), int(want['offsets'][b + 1])
    one = viz.depth_image_lift(T(depth[b]), T(K[b]), image=T(image[b]), T=T(poses[b]))
    assert tuple(one['points'].shape) == (a1 - a0, 3)
    np.testing.assert_array_equal(npy(one['points']), npy(got['points'])[a0:a1])
    np.testing.assert_array_equal(npy(one['colours']), want['colours'][a0:a1])
    np.testing.assert_array_equal(npy(one['pixel']), want['pixel'][a0:a1])
    mask = np.arange(a1 - a0) % 3 == 1
    masked = viz.depth_image_lift(T(depth[b]), T(K[b]), image=T(image[b]), mask=T(mask), T=T(poses[b]))
    for key in ('points', 'colours', 'pixel'):
        np.testing.assert_array_equal(npy(masked[key]), npy(one[key])[mask])
    with pytest.raises(ValueError, match="mask"):
        viz.depth_image_lift(T(depth[b]), T(K[b]), mask=T(mask[:-1]))
    assert viz.depth_image_lift(T(depth[b]), T(K[b]))['colours'] is None


def test_lift_render_round_trip_and_score():
    """Case 8: a posed 48 x 64 depth image lifted and rendered back.  The lift puts a pixel's point at its corner coordinate (c, r), as
    Open3D does, and the renderer truncates, so the rendering camera's principal point is moved by half a pixel: every point lands in
    the middle of its own pixel."""
    from super_primitive_amd.odometery.results import render_map, score_map
    from super_primitive_amd.tool import viz
    H, W = 48, 64
    rng = np.random.default_rng(107)
    rr, cc = np.mgrid[0:H, 0:W]
    depth = (2.0 + 0.5 * np.sin(rr / 7.0) * np.cos(cc / 9.0) + 0.05 * rng.uniform(-1, 1, (H, W))).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.1] = 0.0                               # holes
    K = ref.camera(50.0, 52.0, 31.3, 24.6)
    pose = ref.pose_of([0.2, -0.3, 0.1], [0.5, -0.2, 0.3])
    image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    cloud = viz.depth_image_lift(T(depth), T(K), image=T(image), T=T(pose))
    valid = depth > 0
    assert cloud['points'].shape[0] == valid.sum()
    K_mid = K.copy()
    K_mid[0, 2] += 0.5
    K_mid[1, 2] += 0.5
    world = dict(points=cloud['points'], colours=cloud['colours'])
    out = render_map(world, T(K_mid), T(pose[None]), (H, W))
    index, got = npy(out['index'][0]), npy(out['depth'][0])
    np.testing.assert_array_equal(index >= 0, valid)                          # every valid pixel is hit, and no other
    np.testing.assert_array_equal(npy(cloud['pixel'])[index[valid]], (rr * W + cc)[valid])      # ... by its own point
    np.testing.assert_allclose(got[valid], depth[valid], rtol=2e-6, atol=0)
    np.testing.assert_array_equal(npy(out['image'][0])[valid], ref.colour_u8(image.transpose(1, 2, 0))[valid])
    score = score_map(world, T(depth[None]), T(K_mid), T(pose[None]), min_depth=0.2, max_depth=5.0)
    col = {name: k for k, name in enumerate(score['columns'])}
    m = npy(score['metrics'])[0]
    print(f"\nround trip: coverage {float(score['coverage'][0])}, n {m[col['n']]:.0f}, rmse {m[col['rmse']]:.3e} mm, delta105 {m[col['delta105']]}")
    assert float(score['coverage'][0]) == 1.0 and m[col['n']] == valid.sum()
    assert m[col['rmse']] < 1e-2 and m[col['delta105']] == 1.0
    # 10 % of the ground truth scaled by 1.2: the mean absolute error against NumPy's figure
    gt = depth.copy()
    pick = valid & (rng.uniform(size=(H, W)) < 0.1)
    gt[pick] *= np.float32(1.2)
    score = score_map(world, T(gt[None]), T(K_mid), T(pose[None]))
    mae = np.abs(1000.0 * got[valid].astype(np.float64) - 1000.0 * gt[valid].astype(np.float64)).mean()
    np.testing.assert_allclose(npy(score['metrics'])[0, col['mae']], mae, rtol=1e-5)
    assert float(score['coverage'][0]) == 1.0 and pick.sum() > 100
    # a ground truth with nothing in range: no coverage figure, no crash
    far = score_map(world, T(np.full((1, H, W), 9.0, np.float32)), T(K_mid), T(pose[None]))
    assert np.isnan(float(far['coverage'][0]))


def test_sequence_map_rendered_into_the_ground_truth_keyframe_cameras():
    """Case 9: the 30-frame 224 x 288 x 40 sequence of tests/test_gpu_sequence.py with a window of two keyframes (the run of
    tests/test_gpu_sequence_results.py); its map, aligned against the ground truth, seen from the ground-truth keyframe cameras."""
    from test_gpu_sequence import make_sequence_inputs
    from super_primitive_amd.odometery.results import render_map, score_map, sequence_map
    from super_primitive_amd.odometery.sequence import run_sequence
    seq, frames, to_kf = make_sequence_inputs()
    out = run_sequence(frames, to_kf, T(seq[0].T_wc), T(seq[0].kld_gt), engine="gn", keep_keyframes=True, window_size=2, translation_thresh=0.1)
    G = np.stack([f.T_wc for f in seq]).astype(np.float32)
    world = sequence_map(out, 1, T(G))
    ids = world['ids']
    n_kf = len(ids)
    assert n_kf >= 3
    Ks = np.stack([seq[i].K for i in ids]).astype(np.float32)
    H, W = seq[0].depth.shape
    views = render_map(world, T(Ks), T(G[ids]), (H, W))
    index = views['index']
    assert tuple(views['image'].shape) == (n_kf, H, W, 3) and tuple(index.shape) == (n_kf, H, W)
    coverage = npy((index >= 0).float().mean(dim=(1, 2)))
    hit = index >= 0
    kf_map = torch.where(hit, world['kf_index'][index.clamp(min=0).long()], torch.full_like(index, -1))
    seg_map = torch.where(hit, world['seg_ids'][index.clamp(min=0).long()], torch.full_like(index, -1))
    named = sorted(set(npy(kf_map[hit]).tolist()))
    score = score_map(world, T(np.stack([seq[i].depth for i in ids]).astype(np.float32)), T(Ks), T(G[ids]), size=(H, W))
    col = {name: k for k, name in enumerate(score['columns'])}
    m = npy(score['metrics'])
    print(f"\nsequence map: {world['points'].shape[0]} points of {n_kf} keyframes {ids}; coverage per view {np.round(coverage, 3).tolist()}; keyframes named {named}; "
          f"score: coverage {np.round(npy(score['coverage']), 3).tolist()}, rmse {np.round(m[:, col['rmse']], 1).tolist()} mm, "
          f"delta125 {np.round(m[:, col['delta1']], 3).tolist()}; ATE {float(world['ate_scaled']):.2e}")
    assert (coverage > 0.5).all()
    assert named[0] >= 0 and named[-1] < n_kf and int(seg_map.max()) < 40 and int(seg_map[hit].min()) >= 0
    own = torch.stack([(kf_map[k] == k).float().mean() for k in range(n_kf)])
    assert bool((own > 0).all())                                              # every keyframe is seen from its own camera
