"""-m gpu: the map consistency test and the keyframes' own depth images (csrc/sp_views.hip sp_map_consistency, csrc/sp_results.hip
sp_keyframe_depths, through the C ABI, ``tool/viz.py`` and ``odometery/results.py``) against the float64 statements of
tests/map_consistency_ref.py.

What is compared how.  The counts are integers: every point that is not ambiguous (tests/map_consistency_ref.py; at most 0.5 % of a
case, tests/test_map_consistency_ref_host.py) is compared EXACTLY, an ambiguous one may differ by one view per ambiguous pair moving
between two classes.  With the identity pose nothing is ambiguous.  The keyframes' depth images and segment maps are compared bitwise.
Every call writes into counts pre-filled with 0x7f bytes."""
import numpy as np
import pytest
import torch

import map_consistency_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK = 0x7f7f7f7f


def _views(K, poses):
    V = len(poses)
    Ks = np.broadcast_to(np.asarray(K, np.float32), (V, 3, 3)) if np.ndim(K) == 2 else np.asarray(K, np.float32)
    return np.concatenate([Ks.reshape(V, 9), np.asarray(poses, np.float32).reshape(V, 16)], axis=1).astype(np.float32)


def _raw(points, K, poses, depth, owner=None, view_owner=None, tol=0.05, window=1, z_min=1e-6):
    """sp_map_consistency through the C ABI on counts pre-filled with junk: every row has to be written."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    pts, views, d = T(points), T(_views(K, poses)), T(np.asarray(depth, np.float32))
    own = None if owner is None else T(np.asarray(owner, np.int32))
    vown = None if view_owner is None else T(np.asarray(view_owner, np.int32))
    V, H, W = d.shape
    counts = torch.full((len(points), 3), JUNK, dtype=torch.int32, device=pts.device)
    _lib.check(lib.sp_map_consistency(_lib.ptr(pts), _lib.ptr(own), len(points), _lib.ptr(views), _lib.ptr(vown), V, _lib.ptr(d), H, W, tol, window,
                                      z_min, _lib.ptr(counts), _lib.stream_ptr()), "sp_map_consistency")
    torch.cuda.synchronize()
    return npy(counts)


def _raw_case(c, window, **kw):
    args = dict(owner=c.get('owner'), view_owner=c.get('view_owner'), tol=c['tol'], window=window)
    args.update(kw)
    return _raw(c['points'], c['K'], c['poses'], c['depth'], **args)


@pytest.mark.parametrize("window", [0, 1, 2])
def test_posed_random_views(window):
    """Case 1: Q = 5003 (20 workgroups, the last one partial) against three posed views of 30 x 40, one of which sees nothing; depth
    images with zeros, NaN, negative and +inf pixels; owners -1 .. 2."""
    c, cls, amb = ref.reference("posed", window)
    got = _raw_case(c, window)
    n_amb = ref.check_counts(got, cls, amb, f"posed, window {window}")
    print(f"\nposed, window {window}: {n_amb} ambiguous points; agree / in front / behind pairs {got.sum(axis=0).tolist()}")
    assert (got.sum(axis=0) >= 20).all() and got.max() <= 2
    aside = _raw(c['points'], c['K'], c['poses'][2:], c['depth'][2:], tol=c['tol'], window=window)
    assert not aside.any()                                                   # the view that stands aside: every pair unseen


def test_thresholds_borders_and_windows():
    """Case 2: the identity pose, D = 2, tol = 0.25 -- the arithmetic is exact: 2.5 agrees and the next float is behind, 1.5 agrees and
    the float below is in front; u = 0 is seen, u = W is not; z = z_min is not seen; NaN / inf coordinates are unseen; the corner pixel
    reads its clipped 3 x 3 at window 2; a window whose only valid pixel is a neighbour; a point between a nearer and a farther
    surface is behind."""
    c, expect = ref.case_thresholds()
    one_hot = {ref.AGREE: [1, 0, 0], ref.IN_FRONT: [0, 1, 0], ref.BEHIND: [0, 0, 1], ref.UNSEEN: [0, 0, 0]}
    for (view, window), table in expect.items():
        depth = c['depth'][view][None]
        got = _raw(c['points'], c['K'], c['poses'], depth, tol=c['tol'], window=window)
        cls = ref.classes(c['points'], c['K'], c['poses'], depth, tol=c['tol'], window=window)
        np.testing.assert_array_equal(got, ref.counts_of(cls), err_msg=f"view {view}, window {window}")
        for k, kind in table.items():
            assert got[k].tolist() == one_hot[kind], (view, window, k, ref.CLASS_NAMES[kind])
    # the three images as three views of one call
    stack = np.stack([c['depth'][v] for v in 'ABC'])
    eye3 = np.repeat(c['poses'], 3, axis=0)
    got = _raw(c['points'], c['K'], eye3, stack, tol=c['tol'], window=1)
    np.testing.assert_array_equal(got, ref.counts_of(ref.classes(c['points'], c['K'], eye3, stack, tol=c['tol'], window=1)))
    assert got[14].tolist() == [2, 0, 0] and got[15].tolist() == [1, 0, 1]


def test_owners_skip_exactly_their_own_views():
    """Case 3: V = 4, owners -1 .. 3: a point is skipped in exactly its own view, -1 never; without either owner array nothing is
    skipped; two views of one owner are both skipped."""
    c = ref.case_owners()
    owner = c['owner']
    free = ref.classes(c['points'], c['K'], c['poses'], c['depth'], tol=c['tol'], window=0)
    amb = ref.ambiguous(c['points'], c['K'], c['poses'], c['depth'], tol=c['tol'], window=0)
    assert amb.any(axis=1).mean() <= 0.005
    in_view = free != ref.UNSEEN
    assert in_view.all(axis=1).mean() > 0.5                                   # (the depth images are valid everywhere)
    for view_owner in (np.arange(4), np.array([0, 1, 1, 3]), np.array([-1, -1, 2, -1])):
        view_owner = view_owner.astype(np.int32)
        got = _raw_case(c, 0, view_owner=view_owner)
        cls = ref.classes(c['points'], c['K'], c['poses'], c['depth'], owner, view_owner, c['tol'], 0)
        ref.check_counts(got, cls, amb, f"view owners {view_owner.tolist()}")
        own_views = (owner[:, None] == view_owner[None]) & (owner[:, None] >= 0)
        assert ((cls == ref.SKIPPED) == own_views).all() and own_views[owner == 1].sum(axis=1).tolist() == [int((view_owner == 1).sum())] * int((owner == 1).sum())
        clean = ~amb.any(axis=1)
        np.testing.assert_array_equal(got.sum(axis=1)[clean], (in_view & ~own_views).sum(axis=1)[clean])
    for kw in (dict(owner=None, view_owner=np.arange(4)), dict(view_owner=None), dict(owner=None, view_owner=None)):
        ref.check_counts(_raw_case(c, 0, **kw), free, amb, f"nothing skipped: {sorted(kw)}")


def test_more_views_than_one_workgroup_takes():
    """Case 4: V = 70 views of 8 x 10, Q = 300.  A workgroup takes 32 views (CONS_CHUNK in csrc/sp_views.hip), so this call runs three
    chunks -- 32, 32 and 6 views -- that add their counts by integer atomics; V = 32 and V = 1 run the single-chunk kernel, which stores;
    V = 33 is the smallest call with two chunks."""
    c, cls, amb = ref.reference("many_views", 1)
    got = _raw_case(c, 1)
    ref.check_counts(got, cls, amb, "70 views")
    assert got.sum(axis=1).max() > 32
    for V in (33, 32, 1):
        part = _raw(c['points'], c['K'], c['poses'][:V], c['depth'][:V], c['owner'], c['view_owner'][:V], c['tol'], 1)
        ref.check_counts(part, cls[:, :V], amb[:, :V], f"{V} views")


def test_large_indices_and_heavy_reuse():
    """Case 5: 70 001 points (indices beyond 65 535, 274 workgroups) into two views of 24 x 32: about 90 points read every pixel."""
    c, cls, amb = ref.reference("collide", 1)
    got = _raw_case(c, 1)
    ref.check_counts(got, cls, amb, "collide")
    assert got[65536:].any() and (got.sum(axis=0) > 1000).all()


def test_counts_are_overwritten_and_two_runs_give_the_same_bits():
    """Case 6: counts pre-filled with 0x7f bytes are fully overwritten, on the single-chunk (V = 3) and the multi-chunk (V = 70) path;
    two runs give the same bits; the Python wrapper returns the same."""
    from super_primitive_amd.tool import viz
    for name, window in (("posed", 2), ("many_views", 1)):
        c = ref.reference(name, window)[0]
        a, b = _raw_case(c, window), _raw_case(c, window)
        assert a.tobytes() == b.tobytes(), name
        assert a.min() >= 0 and a.max() <= len(c['poses']) and a.sum(axis=1).max() <= len(c['poses']), name
        out = viz.map_consistency(T(c['points']), T(c['K']), T(c['poses']), T(c['depth']), owner=T(c['owner']), view_owner=T(c['view_owner']),
                                  tol=c['tol'], window=window)
        assert out.dtype == torch.int32 and tuple(out.shape) == a.shape and np.array_equal(npy(out), a), name


def _keyframes():
    from super_primitive_amd.image.keyframe import KeyFrame
    cases = ref.case_keyframes()
    kfs = [KeyFrame(T(k['image']), T(k['K']), T(k['L']), T(k['keypoints']), T(k['masks'])) for k in cases]
    return cases, kfs, [T(k['kld']) for k in cases]


def _raw_keyframe_depths(kfs, klds, with_seg=True):
    """sp_keyframe_depths through the C ABI on outputs (and scratch) pre-filled with junk."""
    from super_primitive_amd import _lib
    from super_primitive_amd.segment_table import table_of
    lib = _lib.load()
    n = len(kfs)
    recs = (_lib.SpMapKeyframe * n)()
    tabs, block = [table_of(kf) for kf in kfs], 0
    for r, tab, kld in zip(recs, tabs, klds):
        r.pix, r.baseL, r.seg_off, r.kp_L, r.kld = tab.pix.data_ptr(), tab.baseL.data_ptr(), tab.seg_off.data_ptr(), tab.kp_L.data_ptr(), kld.data_ptr()
        r.N, r.P, r.H, r.W, r.first_block = tab.N, tab.P, tab.H, tab.W, block
        block += (tab.P + 255) // 256
    H, W = tabs[0].H, tabs[0].W
    dev = klds[0].device
    recs_d = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
    keys = torch.full((n * H * W,), -1, dtype=torch.int64, device=dev)
    depth = torch.full((n, H, W), 777.0, dtype=torch.float32, device=dev)
    seg = torch.full((n, H, W), 12345, dtype=torch.int32, device=dev) if with_seg else None
    _lib.check(lib.sp_keyframe_depths(_lib.ptr(recs_d), n, block, H, W, _lib.ptr(keys), _lib.ptr(depth), _lib.ptr(seg), _lib.stream_ptr()),
               "sp_keyframe_depths")
    torch.cuda.synchronize()
    return npy(depth), None if seg is None else npy(seg)


def test_keyframe_depths_bitwise_from_the_tables():
    """Case 7: two 37 x 53 keyframes (5 and 3 segments): nested and overlapping masks, an empty segment each, a NaN log-depth (skipped),
    a huge one (z = inf, skipped), and a segment that duplicates another's z bit for bit (the higher table index wins).  z per table
    point comes from ``keyframe_points`` at the identity pose (pinned by tests/test_gpu_map_points.py), the pixels from the table."""
    from super_primitive_amd.odometery.results import keyframe_points
    from super_primitive_amd.segment_table import table_of
    from super_primitive_amd.tool import viz
    cases, kfs, klds = _keyframes()
    pts = keyframe_points(kfs, klds, torch.eye(4, device="cuda").repeat(2, 1, 1), stride=1)
    out = viz.keyframe_depths(kfs, klds)
    torch.cuda.synchronize()
    assert out['depth'].dtype == torch.float32 and out['seg'].dtype == torch.int32 and tuple(out['depth'].shape) == tuple(out['seg'].shape) == (2, 37, 53)
    raw_depth, raw_seg = _raw_keyframe_depths(kfs, klds)
    only_depth, none = _raw_keyframe_depths(kfs, klds, with_seg=False)      # seg = NULL is accepted
    assert none is None
    for k, case in enumerate(cases):
        a, b = int(pts['offsets'][k]), int(pts['offsets'][k + 1])
        z, seg_of_point = npy(pts['points'])[a:b, 2], npy(pts['seg_ids'])[a:b]
        rows, cols = ref.decode_pix(npy(table_of(kfs[k]).pix))
        assert len(rows) == b - a == case['masks'].sum()
        depth, seg = ref.keyframe_depth(rows, cols, z, seg_of_point, 37, 53)
        for name, got_depth, got_seg in (("wrapper", npy(out['depth'][k]), npy(out['seg'][k])), ("raw", raw_depth[k], raw_seg[k]),
                                         ("raw, seg NULL", only_depth[k], None)):
            np.testing.assert_array_equal(got_depth.view(np.uint32), depth.view(np.uint32), err_msg=f"keyframe {k}, {name}: depth")
            if got_seg is not None:
                np.testing.assert_array_equal(got_seg, seg, err_msg=f"keyframe {k}, {name}: seg")
        covered = case['masks'].any(axis=0)
        assert not depth[~covered].any() and (seg[~covered] == -1).all() and (~covered).sum() > 0
        skipped = 1 if k == 0 else 0                                         # the NaN / the inf segment: its points are in the table, never in the map
        assert (seg_of_point == skipped).sum() > 50 and not np.isfinite(z[seg_of_point == skipped]).any() and not (seg == skipped).any()
        if k == 0:
            # segment 3 repeats segment 0's z on its pixels, bit for bit: the tie goes to the higher table index
            z0 = {(r, c): v for r, c, v, s in zip(rows, cols, z, seg_of_point) if s == 0}
            ties = [(r, c) for r, c, v, s in zip(rows, cols, z, seg_of_point) if s == 3 and z0[(r, c)].tobytes() == v.tobytes()]
            won = [(r, c) for r, c in ties if depth[r, c].tobytes() == z0[(r, c)].tobytes()]
            assert len(ties) == case['masks'][3].sum() and len(won) > 50 and all(seg[r, c] == 3 for r, c in won)


def _two_plane_depth(K, pose, H, W):
    """The depth image (rays through the pixel CORNERS (c, r), as the lift places its points) and the surface labels of a plate
    |x| < 0.3, |y| < 0.25 at world z = 2 in front of the plane z = 3."""
    K, T4 = K.astype(np.float64), pose.astype(np.float64)
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(cc - K[0, 2]) / K[0, 0], (rr - K[1, 2]) / K[1, 1], np.ones_like(rr)], axis=-1) @ T4[:3, :3].T
    s_plate, s_back = (2.0 - T4[2, 3]) / ray[..., 2], (3.0 - T4[2, 3]) / ray[..., 2]
    hit = T4[:3, 3] + s_plate[..., None] * ray
    plate = (np.abs(hit[..., 0]) < 0.3) & (np.abs(hit[..., 1]) < 0.25)
    return np.where(plate, s_plate, s_back).astype(np.float32), plate


def test_two_views_of_one_surface_end_to_end():
    """Case 8: two posed 48 x 64 depth images of one analytic surface (a plate in front of a plane; B stands a unit to the side and is turned back towards it).  Cloud A, lifted from image A,
    against image B through a principal point moved by half a pixel (tests/test_gpu_map_render.py, case 8): every point of A whose
    neighbourhood in B shows its own surface agrees; a background point wholly hidden by the plate is behind; near the plate's outline
    (a window that shows both surfaces, i.e. within `window` pixels of it) nothing is claimed.  A rectangle of A's depth scaled by 1.3 is behind in B, by 0.7 in front."""
    from super_primitive_amd.odometery.results import filter_map, map_consistency
    from super_primitive_amd.tool import viz
    H, W, window = 48, 64, 1
    K = ref.camera(50.0, 52.0, 31.3, 24.6)
    K_mid = K.copy()
    K_mid[0, 2] += 0.5
    K_mid[1, 2] += 0.5
    pose_a, pose_b = ref.pose_of([0.02, -0.03, 0.01], [0.1, -0.05, 0.0]), ref.pose_of([-0.03, 0.3, 0.0], [-0.9, 0.05, 0.05])
    depth_a, plate_a = _two_plane_depth(K, pose_a, H, W)
    depth_b, plate_b = _two_plane_depth(K, pose_b, H, W)
    assert 100 < plate_a.sum() < H * W / 4 and 100 < plate_b.sum() < H * W / 4

    def run(depth):
        cloud = viz.depth_image_lift(T(depth), T(K), T=T(pose_a))
        Q = cloud['points'].shape[0]
        assert Q == H * W
        world = dict(points=cloud['points'], colours=cloud['points'].clone(), kf_index=torch.zeros(Q, dtype=torch.int32, device="cuda"),
                     seg_ids=T(plate_a.reshape(-1).astype(np.int32)), offsets=np.array([0, Q]))
        cons = map_consistency(world, T(depth_b[None]), T(K_mid), T(pose_b[None]), tol=0.05, window=window)
        # where each point lands in B, and which surfaces B shows in the window the kernel reads around it
        u, v, z = ref.project(npy(cloud['points']), K_mid, pose_b)
        inside = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > 0)
        r, c = np.where(inside, v, 0).astype(int), np.where(inside, u, 0).astype(int)
        m = window
        pad = np.pad(plate_b.astype(np.int64), m, mode='edge')
        near = sum(pad[r + dr, c + dc] for dr in range(2 * m + 1) for dc in range(2 * m + 1))
        return world, cons, inside, near == (2 * m + 1) ** 2, near == 0

    world, cons, inside, all_plate, all_back = run(depth_a)
    counts = npy(cons['counts'])
    assert set(cons) == {'counts', 'agree', 'in_front', 'behind', 'seen'} and counts.dtype == np.int32
    np.testing.assert_array_equal(npy(cons['seen']), counts.sum(axis=1))
    assert not counts[~inside].any()
    on_plate = plate_a.reshape(-1)
    same = inside & np.where(on_plate, all_plate, all_back)
    hidden = inside & ~on_plate & all_plate
    print(f"\ntwo views: {inside.sum()} of {H * W} points of A land in B; {same.sum()} see their own surface, {hidden.sum()} are hidden by the plate, "
          f"{(inside & ~same & ~hidden).sum()} lie near its outline; counts {counts.sum(axis=0).tolist()}")
    assert same.sum() > 0.6 * H * W and hidden.sum() >= 10
    np.testing.assert_array_equal(counts[same], np.tile([1, 0, 0], (same.sum(), 1)))
    np.testing.assert_array_equal(counts[hidden], np.tile([0, 0, 1], (hidden.sum(), 1)))
    # the exported map: exactly the rows the counts confirm
    kept_rows = np.nonzero(counts[:, 0] >= 1)[0]
    out = filter_map(world, cons, min_agree=1)
    np.testing.assert_array_equal(npy(out['kept']), kept_rows)
    np.testing.assert_array_equal(out['offsets'], [0, len(kept_rows)])
    for key in ('points', 'colours', 'kf_index', 'seg_ids'):
        np.testing.assert_array_equal(npy(out[key]), npy(world[key])[kept_rows], err_msg=key)
    assert 0 < len(kept_rows) < H * W
    strict = filter_map(world, cons, min_agree=1, max_in_front=0)
    np.testing.assert_array_equal(npy(strict['kept']), np.nonzero((counts[:, 0] >= 1) & (counts[:, 1] <= 0))[0])
    # a rectangle of the background pushed away / pulled nearer
    rect = np.zeros((H, W), bool)
    rect[4:14, 6:22] = True
    assert not plate_a[rect].any()
    for factor, column in ((1.3, 2), (0.7, 1)):
        moved = depth_a.copy()
        moved[rect] *= np.float32(factor)
        _, cons_m, inside_m, _, all_back_m = run(moved)
        counts_m = npy(cons_m['counts'])
        sure = rect.reshape(-1) & inside_m & all_back_m                      # (seen against the background alone: 3.9 or 2.1 against 3)
        want = np.zeros((sure.sum(), 3), np.int32)
        want[:, column] = 1
        assert sure.sum() > 50, (factor, int(sure.sum()))
        np.testing.assert_array_equal(counts_m[sure], want, err_msg=f"depth x {factor}")
        untouched = ~rect.reshape(-1)
        np.testing.assert_array_equal(counts_m[untouched], counts[untouched])


def test_a_sequence_checks_its_own_map():
    """Case 9: the 30-frame run of tests/test_gpu_map_render.py's case 9 (window of two keyframes, aligned map).  The shares printed
    here are measurements (DESIGN.md section 4 quotes them), not thresholds.  Then one mid-sized segment of the second keyframe gets
    log 1.5 added to its archived log-depth: by ``segment_consistency`` it now has the lowest agree-per-seen ratio of all (keyframe,
    segment) pairs with at least 50 seen points (a rank: no threshold), and no count of another keyframe's point against another
    view changes by a bit."""
    from test_gpu_sequence import make_sequence_inputs
    from super_primitive_amd.odometery import results
    from super_primitive_amd.odometery.sequence import run_sequence
    from super_primitive_amd.tool import pose_utils
    seq, frames, to_kf = make_sequence_inputs()
    out = run_sequence(frames, to_kf, T(seq[0].T_wc), T(seq[0].kld_gt), engine="gn", keep_keyframes=True, window_size=2, translation_thresh=0.1)
    G = np.stack([f.T_wc for f in seq]).astype(np.float32)
    world = results.sequence_map(out, 1, T(G))
    ids = world['ids']
    n_kf = len(ids)
    assert n_kf >= 3
    Q = world['points'].shape[0]
    cons = results.sequence_consistency(world, out)
    H, W = seq[0].depth.shape
    assert tuple(cons['depths'].shape) == tuple(cons['seg_maps'].shape) == (n_kf, H, W) and tuple(cons['counts'].shape) == (Q, 3)
    counts = npy(cons['counts']).astype(np.int64)
    seen = npy(cons['seen'])
    np.testing.assert_array_equal(seen, counts.sum(axis=1))
    assert seen.max() <= n_kf - 1                                            # never against its own keyframe
    Ks = np.stack([seq[i].K for i in ids]).astype(np.float32)
    gt = results.map_consistency(world, T(np.stack([seq[i].depth for i in ids]).astype(np.float32)), T(Ks), T(G[ids]))
    gt_counts = npy(gt['counts']).astype(np.int64)
    share = counts[:, 0].sum() / counts.sum()
    gt_share = gt_counts[:, 0].sum() / gt_counts.sum()
    print(f"\nsequence: {Q} points of {n_kf} keyframes {ids}; seen by another keyframe {np.mean(seen > 0):.3f}; of the seen pairs: agree {share:.4f}, "
          f"in front {counts[:, 1].sum() / counts.sum():.4f}, behind {counts[:, 2].sum() / counts.sum():.4f}; against the ground-truth depths "
          f"(own view included): agree {gt_share:.4f}, in front {gt_counts[:, 1].sum() / gt_counts.sum():.4f}, behind {gt_counts[:, 2].sum() / gt_counts.sum():.4f}; "
          f"points with agree >= 1: {np.mean(counts[:, 0] >= 1):.4f}")
    assert np.mean(seen > 0) > 0.5
    # ---- one segment of the second keyframe pushed away by a factor 1.5
    table0 = npy(results.segment_consistency(world, cons, n_segments=40))
    assert table0.shape == (n_kf, 40, 5) and table0[:, :, 0].sum() == Q
    np.testing.assert_array_equal(table0, npy(results.segment_consistency(world, cons))[:, :40])
    eligible = np.nonzero(table0[1, :, 1] >= 100)[0]                         # (the rank below is among segments other keyframes see)
    assert len(eligible) >= 3
    victim = int(eligible[np.argsort(table0[1, eligible, 0])[len(eligible) // 2]])      # the median size among them
    entry = dict(out['kf_archive'][ids[1]])
    entry['kld'] = entry['kld'].clone()
    entry['kld'][victim] += float(np.log(1.5))
    out2 = dict(out, kf_archive={**out['kf_archive'], ids[1]: entry})
    world2 = results.sequence_map(out2, 1, T(G))
    cons2 = results.sequence_consistency(world2, out2)
    table = npy(results.segment_consistency(world2, cons2, n_segments=40)).astype(np.float64)
    enough = table[:, :, 1] >= 50
    ratio = np.where(enough, table[:, :, 2] / np.maximum(table[:, :, 1], 1), np.inf)
    worst = np.unravel_index(np.argmin(ratio), ratio.shape)
    order = np.sort(ratio[enough])
    print(f"corrupted segment {victim} of keyframe 1 ({int(table[1, victim, 0])} points, {int(table[1, victim, 1])} seen): agree-per-seen "
          f"{ratio[1, victim]:.4f} (before: {table0[1, victim, 2] / max(table0[1, victim, 1], 1):.4f}); the lowest three of {int(enough.sum())} segments: {np.round(order[:3], 4).tolist()}")
    assert enough[1, victim] and worst == (1, victim)
    # ---- every other keyframe's points against every other view: not a bit changes
    a = world.get('align')
    poses = torch.stack([pose_utils.apply_scale(out['kf_archive'][i]['pose'].detach(), dict(s=a['s'][0], rot=a['rot'][0], trans_scaled=a['trans_scaled'][0],
                                                                                            rot_reanchor=a['rot_reanchor'][0])) for i in ids])
    others = [k for k in range(n_kf) if k != 1]
    view_kf = torch.tensor(others, dtype=torch.int32)
    kw = dict(Ks=T(Ks[others]), poses=poses[others], view_kf=view_kf)
    before = results.map_consistency(world, cons['depths'][others].contiguous(), **kw)['counts']
    after = results.map_consistency(world2, cons2['depths'][others].contiguous(), **kw)['counts']
    rest = world['kf_index'] != 1
    assert torch.equal(world['kf_index'], world2['kf_index']) and torch.equal(world['points'][rest], world2['points'][rest])
    assert torch.equal(before[rest], after[rest]) and int(before[rest].sum()) > 0
    # (and the sequence's own call is that call plus the corrupted view)
    assert bool((cons['counts'][rest] >= before[rest]).all())
