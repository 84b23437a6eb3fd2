"""-m gpu: map distances (csrc/sp_nearest.hip sp_cloud_grid_build / sp_cloud_grid_nearest through the C ABI, ``tool/viz.py``
``cloud_grid`` / ``nearest_points`` and ``odometery/results.py`` ``map_distance`` / ``map_neighbours`` / ``cloud_metrics``) against the
float64 reference of tests/map_nearest_ref.py.

Everything is compared EXACTLY: ``index`` and ``count`` equal, ``dist`` equal as uint32 bit patterns.  Every call writes into outputs
and a scratch pre-filled with 0x7f bytes, and every output row must have been overwritten."""
import numpy as np
import pytest
import torch

import map_nearest_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK32 = 0x7f7f7f7f


def _raw(queries, points, radius, origin, skip_self=0, builds=1):
    """Build and query through the C ABI on a junk-filled scratch and junk-filled outputs; returns the host arrays."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    Q, Qa = len(points), len(queries)
    pts = T(np.asarray(points, np.float32))
    qs = pts if queries is points else T(np.asarray(queries, np.float32))
    units = lib.sp_cloud_grid_scratch_units(Q)
    assert units > 0
    dev = pts.device
    junk = lambda *shape: torch.full(shape, JUNK32, dtype=torch.int32, device=dev)
    scratch = junk(units * 16)
    for _ in range(builds):                                                    # (a second build on the used scratch must give the same)
        _lib.check(lib.sp_cloud_grid_build(_lib.ptr(pts), Q, float(radius), float(origin[0]), float(origin[1]), float(origin[2]), _lib.ptr(scratch),
                                           _lib.stream_ptr()), "sp_cloud_grid_build")
    index, dist, count = junk(Qa), junk(Qa), junk(Qa)
    _lib.check(lib.sp_cloud_grid_nearest(_lib.ptr(qs), Qa, Q, _lib.ptr(scratch), int(skip_self), _lib.ptr(index), _lib.ptr(dist), _lib.ptr(count),
                                         _lib.stream_ptr()), "sp_cloud_grid_nearest")
    torch.cuda.synchronize()
    return dict(index=npy(index), dist=npy(dist).view(np.float32), count=npy(count))


def _check(got, want, what):
    """Bit for bit against the reference; no row left as it was."""
    np.testing.assert_array_equal(got['count'], want['count'], err_msg=f"{what}: count")
    np.testing.assert_array_equal(got['index'], want['index'], err_msg=f"{what}: index")
    np.testing.assert_array_equal(got['dist'].view(np.uint32), want['dist'].view(np.uint32), err_msg=f"{what}: dist")
    for key in ('index', 'dist', 'count'):
        assert not (got[key].view(np.uint32) == JUNK32).any(), f"{what}: {key} has rows that were not written"


@pytest.mark.parametrize("setting", range(len(ref.SETTINGS)))
def test_random_clouds(setting):
    """Qa = 5003 (20 workgroups, the last one partial) against Q = 3001, coordinates in +-2, at r 0.25 through zero, r 0.3 through
    (0.1, -0.7, 3.3) and r 0.1: each cloud with a NaN row, a +inf row, a row out of range and a -0.0."""
    a, b = ref.case_random()
    radius, origin = ref.SETTINGS[setting]
    want = ref.reference_random(setting)
    got = _raw(a, b, radius, origin)
    none = float((got['index'] < 0).mean())
    print(f"\nr {radius}, origin {origin}: {none:.3f} of the queries have no neighbour, largest count {got['count'].max()}")
    _check(got, want, f"r {radius}, origin {origin}")
    assert 0.01 < none < 0.9                                                   # (cannot pass on all-none output)
    for bad in ref.BAD_ROWS:
        assert got['index'][bad] == -1 and got['count'][bad] == 0 and np.isposinf(got['dist'][bad]) and not (got['index'] == bad).any()


@pytest.mark.parametrize("origin", range(len(ref.LATTICE_ORIGINS)))
def test_lattice(origin):
    """Reference rows on a 12^3 lattice of pitch r with every 7th row repeated, queries at exactly r, r / 2, r (1 + 1e-7) and (0.3, 0.3,
    0.3) from lattice points: distances of exactly r are neighbours, a repeated row loses the tie to its original."""
    a, b = ref.case_lattice()
    o = ref.LATTICE_ORIGINS[origin]
    want = ref.nearest(a, b, ref.LATTICE_R, o)
    got = _raw(a, b, ref.LATTICE_R, o)
    _check(got, want, f"lattice, origin {o}")
    assert (got['count'] > 1).sum() > 1000 and 0 < (got['index'] < 0).sum() < 150 and got['index'].max() < 12 ** 3


def test_one_long_cell():
    """3000 reference rows in ONE cell, 256 queries within r of all of them: every walk is 3000 records long."""
    a, b, radius, origin = ref.case_one_cell()
    got = _raw(a, b, radius, origin)
    _check(got, ref.nearest(a, b, radius, origin), "one cell")
    assert (got['count'] == 3000).all()


def test_the_table_at_its_highest_load():
    """4096 reference rows, each alone in its cell, in shuffled order: S = 8192 slots, load exactly 0.5, long probe chains."""
    a, b, radius, origin = ref.case_full_load()
    got = _raw(a, b, radius, origin)
    _check(got, ref.nearest_candidates(a, b, radius, origin), "full load")
    assert (got['index'] >= 0).mean() > 0.9
    own = _raw(b, b, radius, origin)                                           # every row finds at least itself, at distance 0
    assert (own['count'] >= 1).all() and not own['dist'][own['index'] == np.arange(4096)].any()


@pytest.mark.parametrize("Q", [1, 256, 257, 70001])
@pytest.mark.parametrize("Qa", [1, 256, 257, 70001])
def test_sizes(Qa, Q):
    """One row; exactly one workgroup; one row into the second; 70 001 rows (rows beyond 65 535, a scan with more than one block sum per
    thread: S = 262 144 slots are 1024 blocks)."""
    a, b = ref.case_sizes(Qa, Q)
    radius, origin = ref.SIZES_SETTING
    want = ref.nearest_candidates(a, b, radius, origin)
    got = _raw(a, b, radius, origin)
    _check(got, want, f"Qa = {Qa}, Q = {Q}")
    if Q == 70001 and Qa >= 256:
        assert got['index'].max() > 65535 and got['count'].max() >= 10


def test_skip_self():
    """The random cloud against itself: no row finds itself, a duplicated row finds its twin at distance 0, count is the plain count
    minus one; Qa != Q is refused."""
    from super_primitive_amd import _lib
    p = ref.case_self()
    radius, origin = ref.SETTINGS[0]
    want = ref.nearest(p, p, radius, origin, skip_self=True)
    got, plain = _raw(p, p, radius, origin, skip_self=1), _raw(p, p, radius, origin)
    _check(got, want, "skip_self")
    _check(plain, ref.nearest(p, p, radius, origin), "the cloud against itself")
    assert not (got['index'] == np.arange(len(p))).any()
    assert got['index'][50] == 100 and got['index'][100] == 50 and got['dist'][50] == 0.0 and got['dist'][100] == 0.0
    ok = plain['count'] > 0
    assert ok.sum() == len(p) - 3 and np.array_equal(got['count'][ok], plain['count'][ok] - 1) and not got['count'][~ok].any()
    lib, some = _lib.load(), T(np.zeros((8, 3), np.float32))
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.sp_cloud_grid_nearest(_lib.ptr(some), 7, 8, _lib.ptr(some), 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), _lib.stream_ptr()) == -1


def test_two_runs_give_the_same_bits_and_a_permutation_renames_the_rows():
    """Two runs (and a second build on the used scratch) give the same bits.  The random case has no tie in its winning distances, so
    with the reference rows permuted ``dist`` and ``count`` are bitwise unchanged and ``perm[index]`` is the unpermuted index."""
    a, b = ref.case_random()
    radius, origin = ref.SETTINGS[1]
    first, again, rebuilt = _raw(a, b, radius, origin), _raw(a, b, radius, origin), _raw(a, b, radius, origin, builds=2)
    for key in ('index', 'dist', 'count'):
        assert first[key].tobytes() == again[key].tobytes() == rebuilt[key].tobytes(), key
    perm = np.random.default_rng(77).permutation(len(b))
    moved = _raw(a, b[perm], radius, origin)
    _check(moved, ref.nearest(a, b[perm], radius, origin), "permuted")
    assert moved['dist'].tobytes() == first['dist'].tobytes() and moved['count'].tobytes() == first['count'].tobytes()
    found = first['index'] >= 0
    assert np.array_equal(moved['index'] >= 0, found) and np.array_equal(perm[moved['index'][found]], first['index'][found])
    assert not np.array_equal(moved['index'], first['index'])


def test_the_python_surface_gives_the_same_and_checks_its_handle():
    from super_primitive_amd.tool import viz
    a, b = ref.case_random()
    radius, origin = ref.SETTINGS[1]
    want = ref.reference_random(1)
    grid = viz.cloud_grid(T(b), radius, origin)
    assert set(grid) == {'scratch', 'Q', 'radius', 'origin', 'points'} and grid['Q'] == len(b) and grid['radius'] == float(np.float32(radius))
    out = viz.nearest_points(T(a), grid)
    assert out['index'].dtype == torch.int32 and out['dist'].dtype == torch.float32 and out['count'].dtype == torch.int32
    _check({k: npy(v) for k, v in out.items()}, want, "nearest_points")
    again = viz.nearest_points(T(a[:100]), grid)                               # one build answers any number of query clouds
    assert npy(again['dist']).tobytes() == want['dist'][:100].tobytes()
    default = viz.nearest_points(T(a), viz.cloud_grid(T(b), 0.25))             # the default origin is 0, 0, 0
    _check({k: npy(v) for k, v in default.items()}, ref.reference_random(0), "default origin")
    with pytest.raises(ValueError, match="scratch"):
        viz.nearest_points(T(a), dict(grid, scratch=grid['scratch'][:-1]))
    with pytest.raises(ValueError, match="skip_self"):
        viz.nearest_points(T(a), grid, skip_self=True)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _plane_keyframe(H, W, K, seed):
    """A keyframe whose every pixel lies at depth 2.02 (four segments, the quadrants), with a random image."""
    from super_primitive_amd.image.keyframe import KeyFrame
    rng = np.random.default_rng(seed)
    masks = np.zeros((4, H, W), dtype=bool)
    masks[0, :H // 2, :W // 2] = masks[1, :H // 2, W // 2:] = masks[2, H // 2:, :W // 2] = masks[3, H // 2:, W // 2:] = True
    L = np.full((4, H, W), np.log(2.02), dtype=np.float32) * masks
    keypoints = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, -0.5], [0.5, 0.5]], dtype=np.float32)
    image = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    return KeyFrame(T(image), T(K), T(L), T(keypoints), T(masks)), T(np.full(4, np.log(2.02), dtype=np.float32))


def _check_metrics(got, dist_a, dist_b, radius, threshold):
    want = ref.metrics(dist_a, dist_b, radius, threshold)
    assert set(got) == set(want)
    for key in ('n_a', 'n_b', 'found_a', 'found_b', 'within_a', 'within_b'):
        assert got[key].dtype == torch.int64 and got[key].dim() == 0 and int(got[key]) == want[key], key
    for key, n in (('accuracy', len(dist_a)), ('completion', len(dist_b)), ('accuracy_clipped', len(dist_a)), ('completion_clipped', len(dist_b)),
                   ('chamfer', len(dist_a) + len(dist_b)), ('precision', 4), ('recall', 4), ('fscore', 4)):
        assert got[key].dtype == torch.float64 and abs(float(got[key]) - want[key]) <= n * 2.0 ** -52 * want[key], key
    return want


def test_two_keyframes_of_one_plane_against_a_lifted_depth_image():
    """Two 48 x 64 keyframes that look at the plane z = 2.02 from 0.1 apart, against the lift of a depth image of the plane z = 2.05 seen
    from the first pose: the gap is 0.03 and the reference's sample pitch 2.05 / 60, so the accuracy lies in 0.03 .. 0.0385."""
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    H, W = 48, 64
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], dtype=np.float32)
    (kf_a, kld_a), (kf_b, kld_b) = _plane_keyframe(H, W, K, 1), _plane_keyframe(H, W, K, 2)
    poses = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    poses[1, 0, 3] = 0.1
    world = results.keyframe_points([kf_a, kf_b], [kld_a, kld_b], T(poses), stride=1)
    world['ids'] = [0, 7]
    Q = world['points'].shape[0]
    assert Q == 2 * H * W
    reference = viz.depth_image_lift(T(np.full((H, W), 2.05, dtype=np.float32)), T(K), T=T(poses[0]))
    R = reference['points'].shape[0]
    assert R == H * W
    before = {k: (v.clone() if torch.is_tensor(v) else np.array(v)) for k, v in world.items()}
    radius, threshold = 0.1, 0.035
    out = results.map_distance(world, reference, radius, threshold=threshold)
    assert set(out) == {'to_reference', 'to_map', 'metrics'}
    p, q = npy(world['points']), npy(reference['points'])
    to_reference, to_map = {k: npy(v) for k, v in out['to_reference'].items()}, {k: npy(v) for k, v in out['to_map'].items()}
    _check(to_reference, ref.nearest(p, q, radius, (0.0, 0.0, 0.0)), "map to reference")
    _check(to_map, ref.nearest(q, p, radius, (0.0, 0.0, 0.0)), "reference to map")
    m = out['metrics']
    want = _check_metrics(m, to_reference['dist'], to_map['dist'], radius, threshold)
    print(f"\ntwo plane keyframes against the lifted plane: {Q} map points, {R} reference points; " +
          ", ".join(f"{k} {want[k]:.5f}" if isinstance(want[k], float) else f"{k} {want[k]}" for k in want))
    assert 0.03 <= float(m['accuracy']) <= 0.0385
    assert 0 < int(m['within_a']) < Q and 0 < int(m['within_b']) <= R
    for side in ('a', 'b'):                                                    # a row without a neighbour counts at the radius
        mean, clipped = ('accuracy', 'accuracy_clipped') if side == 'a' else ('completion', 'completion_clipped')
        if int(m['found_' + side]) < int(m['n_' + side]):
            assert float(m[clipped]) > float(m[mean])
        else:
            assert float(m[clipped]) == float(m[mean])
    # at half the radius the far end of the second keyframe's extra strip has no reference point: the clipped accuracy sees it
    near = results.map_distance(world, reference['points'], 0.05)
    _check({k: npy(v) for k, v in near['to_reference'].items()}, ref.nearest(p, q, 0.05, (0.0, 0.0, 0.0)), "map to reference at 0.05")
    _check_metrics(near['metrics'], npy(near['to_reference']['dist']), npy(near['to_map']['dist']), 0.05, 0.05)
    assert int(near['metrics']['found_a']) < Q and float(near['metrics']['accuracy_clipped']) > float(near['metrics']['accuracy'])
    assert int(near['metrics']['within_a']) == int(near['metrics']['found_a'])             # the threshold defaults to the radius
    with pytest.raises(ValueError, match="threshold"):
        results.map_distance(world, reference, 0.05, threshold=0.1)
    # the input is left as it was
    assert set(world) == set(before)
    for k, v in before.items():
        assert torch.equal(world[k], v) if torch.is_tensor(v) else np.array_equal(np.asarray(world[k]), v), k
    # a fused and a filtered map go through the same call
    fused = results.fuse_map(world, 0.05)
    M = fused['points'].shape[0]
    d = results.map_distance(fused, reference, radius, threshold=threshold)
    assert tuple(d['to_reference']['dist'].shape) == (M,) and tuple(d['to_map']['index'].shape) == (R,) and int(d['metrics']['n_a']) == M
    assert int(d['to_map']['index'].max()) < M
    Ks, Ts = T(np.stack([K, K])), T(poses)
    own = viz.keyframe_depths([kf_a, kf_b], [kld_a, kld_b])
    kept = results.filter_map(world, results.map_consistency(world, own['depth'], Ks, Ts, view_kf=[0, 1]))
    n_kept = kept['points'].shape[0]
    d = results.map_distance(kept, reference, radius, threshold=threshold, origin=(0.01, 0.02, 0.03))
    assert 0 < n_kept <= Q and tuple(d['to_reference']['count'].shape) == (n_kept,) and tuple(d['to_map']['dist'].shape) == (R,)
    assert float(d['metrics']['precision']) > 0
    # the map against itself: every interior point has another point within 0.05 (the pitch is 2.02 / 60)
    nb = results.map_neighbours(world, 0.05)
    _check({k: npy(v) for k, v in nb.items()}, ref.nearest_candidates(p, p, 0.05, (0.0, 0.0, 0.0), skip_self=True), "map_neighbours")
    count = npy(nb['count'])
    inner = (np.abs(p[:, 0] - 0.05) < 0.9) & (np.abs(p[:, 1]) < 0.7)          # away from the rim of both keyframes: four pixel neighbours
    assert (count >= 1).all() and (count[inner] >= 4).all() and inner.sum() > Q // 2 and (npy(nb['index']) != np.arange(Q)).all()
