"""-m gpu: map fusion (csrc/sp_fuse.hip sp_map_fuse through the C ABI, ``tool/viz.py`` ``fuse_points`` and ``odometery/results.py``
``fuse_map`` / ``pool_map``) against the float64 loop of tests/map_fuse_ref.py.

Everything is compared EXACTLY: the float32 bit patterns of positions and colours, ``count``, ``first``, ``label`` and ``n_fused``.
Every call writes into outputs (and scratch) pre-filled with 0x7f bytes; rows at or beyond ``n_fused`` must still hold them."""
import numpy as np
import pytest
import torch

import map_fuse_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK32 = 0x7f7f7f7f


def _raw(points, colours, voxel, origin):
    """sp_map_fuse through the C ABI on junk-filled outputs and scratch; returns the host arrays (whole capacity buffers)."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    Q = len(points)
    pts = T(np.asarray(points, np.float32))
    cols = None if colours is None else T(np.asarray(colours, np.float32))
    units = lib.sp_map_fuse_scratch_units(Q)
    assert units > 0
    dev = pts.device
    junk = lambda *shape: torch.full(shape, JUNK32, dtype=torch.int32, device=dev)
    scratch = junk(units * 16)
    out_p, out_c, count, first, label = junk(Q, 3), (None if cols is None else junk(Q, 3)), junk(Q), junk(Q), junk(Q)
    n = torch.full((1,), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device=dev)
    _lib.check(lib.sp_map_fuse(_lib.ptr(pts), _lib.ptr(cols), Q, float(voxel), float(origin[0]), float(origin[1]), float(origin[2]),
                               _lib.ptr(scratch), _lib.ptr(out_p), _lib.ptr(out_c), _lib.ptr(count), _lib.ptr(first), _lib.ptr(label), _lib.ptr(n),
                               _lib.stream_ptr()), "sp_map_fuse")
    torch.cuda.synchronize()
    return dict(points=npy(out_p), colours=None if out_c is None else npy(out_c), count=npy(count), first=npy(first), label=npy(label),
                n=int(n[0]))


def _check(got, want, what):
    """Bit for bit against the reference; the capacity rows beyond M untouched."""
    M = want['n']
    assert got['n'] == M, f"{what}: n_fused {got['n']} against {M}"
    np.testing.assert_array_equal(got['label'], want['label'], err_msg=f"{what}: label")
    np.testing.assert_array_equal(got['first'][:M], want['first'], err_msg=f"{what}: first")
    np.testing.assert_array_equal(got['count'][:M], want['count'], err_msg=f"{what}: count")
    np.testing.assert_array_equal(got['points'][:M].view(np.uint32), want['points'].view(np.uint32), err_msg=f"{what}: positions")
    if want['colours'] is not None:
        np.testing.assert_array_equal(got['colours'][:M].view(np.uint32), want['colours'].view(np.uint32), err_msg=f"{what}: colours")
    for key in ('points', 'colours', 'count', 'first'):
        if got[key] is not None:
            assert (got[key][M:] == JUNK32).all(), f"{what}: {key} written at or beyond row {M}"


@pytest.mark.parametrize("setting", range(len(ref.SETTINGS)))
def test_random_points(setting):
    """Q = 5003 (20 workgroups, the last one partial), coordinates in +-2, at voxel 0.25 through zero, voxel 0.3 (q is inexact) and
    voxel 0.25 through (0.1, -0.7, 3.3): points on voxel faces, negative coordinates, -0.0, a NaN row, a +inf row and a row out of range
    (all three dropped), colours beyond 0 .. 1 and a NaN colour."""
    p, c = ref.case_random()
    voxel, origin = ref.SETTINGS[setting]
    want = ref.reference_random(setting)
    got = _raw(p, c, voxel, origin)
    _check(got, want, f"voxel {voxel}, origin {origin}")
    assert np.nonzero(got['label'] < 0)[0].tolist() == list(ref.BAD_ROWS) and got['count'][:got['n']].sum() == len(p) - 3
    if setting == 0:
        coarse = ref.fuse(p, c, 1.0, origin)                                 # about 75 points per voxel: long chains of adds into one slot
        _check(_raw(p, c, 1.0, origin), coarse, "voxel 1.0")
        assert coarse['count'].max() >= 50


def test_the_table_at_its_highest_load():
    """Q = 4096 points, each alone in its voxel, in shuffled order: S = 8192 slots, load exactly 0.5, long probe chains.  M = Q, every
    count is 1, first and label are the identity."""
    p, c, voxel, origin = ref.case_full_load()
    got = _raw(p, c, voxel, origin)
    _check(got, ref.fuse(p, c, voxel, origin), "full load")
    assert got['n'] == 4096 and (got['count'] == 1).all()
    np.testing.assert_array_equal(got['first'], np.arange(4096))
    np.testing.assert_array_equal(got['label'], np.arange(4096))


@pytest.mark.parametrize("n_voxels", [1, 2])
def test_the_highest_contention(n_voxels):
    """Q = 3000 points in ONE voxel -- every atomic of the call lands on one slot --, and in two voxels alternating row by row."""
    p, c, voxel, origin = ref.case_contention(n_voxels)
    want = ref.fuse(p, c, voxel, origin)
    got = _raw(p, c, voxel, origin)
    _check(got, want, f"{n_voxels} voxel(s)")
    assert got['n'] == n_voxels and got['count'][:n_voxels].tolist() == [3000 // n_voxels] * n_voxels
    np.testing.assert_array_equal(got['label'], np.arange(3000) % n_voxels)


def test_a_row_permutation_reorders_the_output_and_keeps_the_voxels():
    """The random case under a row permutation: the fused rows are the reference's for the permuted input (order of first rows), and
    the multiset of voxels -- position, colour and count per voxel -- is that of the unpermuted call."""
    p, c = ref.case_random()
    voxel, origin = ref.SETTINGS[0]
    perm = np.random.default_rng(77).permutation(len(p))
    want = ref.fuse(p[perm], c[perm], voxel, origin)
    got = _raw(p[perm], c[perm], voxel, origin)
    _check(got, want, "permuted")
    plain = _raw(p, c, voxel, origin)
    M = want['n']
    assert plain['n'] == M and not np.array_equal(plain['first'][:M], got['first'][:M])

    def bag(r):                                                              # (position and colour are functions of key, n, S and C)
        rows = np.concatenate([r['points'][:M].view(np.uint32), r['colours'][:M].view(np.uint32), r['count'][:M, None].astype(np.uint32)], axis=1)
        return rows[np.lexsort(rows.T[::-1])]
    np.testing.assert_array_equal(bag(got), bag(plain))
    ref_plain = ref.reference_random(0)
    key_bag = lambda r: sorted(zip(map(int, r['keys']), map(int, r['count']), map(tuple, r['sums'].tolist()), map(tuple, r['colour_sums'].tolist())))
    assert key_bag(want) == key_bag(ref_plain)
    # the members of every voxel are the same rows: labels agree through the permutation, up to the renumbering of the voxels
    same = {}
    for a, b in zip(got['label'].tolist(), plain['label'][perm].tolist()):
        assert same.setdefault(a, b) == b


@pytest.mark.parametrize("Q", [1, 256, 257, 70001])
def test_sizes(Q):
    """One point; exactly one workgroup; one row into the second; 70 001 rows (274 workgroups, rows beyond 65 535, a scan with more than
    one block count per thread)."""
    p, c = ref.case_random(Q)
    voxel, origin = ref.SETTINGS[2]
    want = ref.fuse(p, c, voxel, origin)
    got = _raw(p, c, voxel, origin)
    _check(got, want, f"Q = {Q}")
    assert got['n'] >= 1 and (Q < 70001 or (got['count'][:got['n']].max() >= 10 and got['label'][65536:].min() >= 0))


def test_without_colours_and_two_runs_give_the_same_bits():
    """colours = out_colours = NULL: positions, counts and labels as with colours; two runs of either call give the same bits; the
    Python wrapper returns the same, with ``first`` pre-filled so that rows beyond n sort last."""
    from super_primitive_amd.tool import viz
    p, c = ref.case_random()
    voxel, origin = ref.SETTINGS[1]
    a, b = _raw(p, None, voxel, origin), _raw(p, None, voxel, origin)
    assert a['colours'] is None
    _check(a, ref.reference_random(1, with_colours=False), "no colours")
    for key in ('points', 'count', 'first', 'label'):
        assert a[key].tobytes() == b[key].tobytes(), key
    with_c, again = _raw(p, c, voxel, origin), _raw(p, c, voxel, origin)
    for key in ('points', 'colours', 'count', 'first', 'label'):
        assert with_c[key].tobytes() == again[key].tobytes(), key
    for key in ('points', 'count', 'first', 'label'):
        assert with_c[key].tobytes() == a[key].tobytes(), key
    M = a['n']
    for cols in (None, T(c)):
        out = viz.fuse_points(T(p), cols, voxel=voxel, origin=origin)
        assert out['n'].dtype == torch.int64 and out['n'].dim() == 0 and int(out['n']) == M
        assert (out['colours'] is None) == (cols is None)
        for key in ('points', 'count', 'first'):
            assert npy(out[key][:M]).tobytes() == with_c[key][:M].tobytes(), key
        assert npy(out['label']).tobytes() == with_c['label'].tobytes()
        if cols is not None:
            assert npy(out['colours'][:M]).tobytes() == with_c['colours'][:M].tobytes()
        first = npy(out['first'])
        assert (first[M:] == 2 ** 31 - 1).all() and (np.diff(first.astype(np.int64)) >= 0).all()
    out = viz.fuse_points(T(p), None, voxel=0.25)                             # the default origin is 0, 0, 0
    want = ref.reference_random(0, with_colours=False)
    assert int(out['n']) == want['n'] and np.array_equal(npy(out['label']), want['label'])
    assert npy(out['points'][:want['n']]).tobytes() == want['points'].tobytes()


def _plane_keyframe(H, W, K, seed):
    """A keyframe whose every pixel lies at depth 2.02 -- inside the voxel layer 2 .. 2.05 -- (four segments, the quadrants), with a
    random image."""
    from super_primitive_amd.image.keyframe import KeyFrame
    rng = np.random.default_rng(seed)
    masks = np.zeros((4, H, W), dtype=bool)
    masks[0, :H // 2, :W // 2] = masks[1, :H // 2, W // 2:] = masks[2, H // 2:, :W // 2] = masks[3, H // 2:, W // 2:] = True
    L = np.full((4, H, W), np.log(2.02), dtype=np.float32) * masks
    keypoints = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, -0.5], [0.5, 0.5]], dtype=np.float32)
    image = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    return KeyFrame(T(image), T(K), T(L), T(keypoints), T(masks)), T(np.full(4, np.log(2.02), dtype=np.float32))


def test_two_keyframes_of_one_plane_end_to_end():
    """Two 48 x 64 keyframes (built as in tests/test_gpu_map_points.py) that look at the plane z = 2.02 from 0.1 apart: ``fuse_map`` stores
    the shared part of the plane once.  One point of the map is made NaN: it is dropped, and nothing else notices."""
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    H, W, voxel = 48, 64, 0.05
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], dtype=np.float32)
    (kf_a, kld_a), (kf_b, kld_b) = _plane_keyframe(H, W, K, 1), _plane_keyframe(H, W, K, 2)
    poses = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    poses[1, 0, 3] = 0.1
    world = results.keyframe_points([kf_a, kf_b], [kld_a, kld_b], T(poses), stride=1)
    world['ids'] = [0, 7]
    Q = world['points'].shape[0]
    assert Q == 2 * H * W and world['offsets'].tolist() == [0, H * W, Q]
    world['points'][100, 1] = float("nan")
    before = {k: (v.clone() if torch.is_tensor(v) else np.array(v)) for k, v in world.items()}
    fused = results.fuse_map(world, voxel)
    M = fused['points'].shape[0]
    count, first, label = npy(fused['count']), npy(fused['first']), npy(fused['label'])
    print(f"\ntwo keyframes of one plane: Q = {Q} -> M = {M} at voxel {voxel}; largest count {count.max()}; offsets {fused['offsets'].tolist()}")
    assert 0 < M < Q and count.sum() == Q - 1 and (label < 0).sum() == 1 and label[100] == -1
    for key in ('points', 'colours'):
        assert tuple(fused[key].shape) == (M, 3) and fused[key].dtype == torch.float32
    for key in ('kf_index', 'seg_ids', 'count', 'first'):
        assert tuple(fused[key].shape) == (M,) and fused[key].dtype == torch.int32
    assert tuple(fused['label'].shape) == (Q,) and fused['ids'] == [0, 7]
    # the whole result against the reference loop
    want = ref.fuse(npy(world['points']), npy(world['colours']), voxel, (0.0, 0.0, 0.0))
    _check(dict(points=npy(fused['points']), colours=npy(fused['colours']), count=count, first=first, label=label, n=M), want, "fuse_map")
    # bookkeeping: first rows ascend, the per-point entries are the first member's, offsets are the bincount of kf_index
    kf = npy(fused['kf_index'])
    np.testing.assert_array_equal(kf, npy(world['kf_index'])[first])
    np.testing.assert_array_equal(npy(fused['seg_ids']), npy(world['seg_ids'])[first])
    assert isinstance(fused['offsets'], np.ndarray) and fused['offsets'].dtype == np.int64
    np.testing.assert_array_equal(fused['offsets'], np.concatenate(([0], np.cumsum(np.bincount(kf, minlength=2)))))
    assert (np.diff(kf) >= 0).all() and 0 < fused['offsets'][1] < M          # the second keyframe adds the strip only it sees
    assert fused['offsets'][2] - fused['offsets'][1] < fused['offsets'][1]
    # the input is left as it was
    assert set(world) == set(before)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t    # (the NaN compares as its bits)
    for k, v in before.items():
        assert torch.equal(bits(world[k]), bits(v)) if torch.is_tensor(v) else np.array_equal(np.asarray(world[k]), v), k
    # the fused map goes through the map functions as it is
    Ks, Ts = T(np.stack([K, K])), T(poses)
    views = results.render_map(fused, Ks, Ts, (H, W), radii=torch.full((M,), voxel / 2, device="cuda"))
    assert tuple(views['image'].shape) == (2, H, W, 3) and float((views['index'] >= 0).float().mean()) > 0.9
    own = viz.keyframe_depths([kf_a, kf_b], [kld_a, kld_b])
    cons_fused = results.map_consistency(fused, own['depth'], Ks, Ts, view_kf=[0, 1])
    assert tuple(cons_fused['counts'].shape) == (M, 3) and int(cons_fused['agree'].sum()) > 0
    kept = results.filter_map(fused, cons_fused)
    assert 0 < kept['points'].shape[0] <= M
    # the input map's own consistency counts, pooled per fused point: nothing is lost but the dropped row
    cons = results.map_consistency(world, own['depth'], Ks, Ts, view_kf=[0, 1])
    pooled = results.pool_map(fused, cons['counts'])
    assert pooled.dtype == torch.int64 and tuple(pooled.shape) == (M, 3)
    counts = npy(cons['counts']).astype(np.int64)
    np.testing.assert_array_equal(npy(pooled).sum(axis=0), counts.sum(axis=0) - counts[100])
    want_pooled = np.zeros((M, 3), np.int64)
    np.add.at(want_pooled, label[label >= 0], counts[label >= 0])
    np.testing.assert_array_equal(npy(pooled), want_pooled)
    np.testing.assert_array_equal(npy(results.pool_map(fused, torch.ones(Q, dtype=torch.int32, device="cuda"))), count)
