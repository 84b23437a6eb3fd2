"""CPU-only: the float64 statements of tests/map_consistency_ref.py checked against differently written ones, and the preconditions of
the device cases made there (tests/test_gpu_map_consistency.py): few ambiguous points, and every class of pair occurring."""
import numpy as np
import pytest

import map_consistency_ref as ref

RANDOM = [("posed", 0), ("posed", 1), ("posed", 2), ("owners", 0), ("many_views", 1), ("collide", 1)]
AMBIGUOUS_CAP = 0.005          # a condition on the cases, not a measurement: DELTA is 1e-6 px, so the expected share is about 1e-5


@pytest.mark.parametrize("name,window", RANDOM)
def test_the_random_cases_have_few_ambiguous_points(name, window):
    c, cls, amb = ref.reference(name, window)
    share = amb.any(axis=1).mean()
    print(f"\n{name} window {window}: ambiguous share {share:.2e}; pairs per class {dict(zip(ref.CLASS_NAMES, np.bincount(cls.ravel(), minlength=5).tolist()))}")
    assert share <= AMBIGUOUS_CAP
    assert cls.shape == (len(c['points']), len(c['poses'])) and cls.dtype == np.int8


def test_every_class_occurs_in_the_random_cases():
    total = np.zeros(5, np.int64)
    for name, window in RANDOM:
        per_case = np.bincount(ref.reference(name, window)[1].ravel(), minlength=5)
        total += per_case
        if name in ("posed", "many_views"):                                  # these two carry owners: every class, in one call
            assert (per_case >= 20).all(), (name, window, per_case.tolist())
    assert (total >= 20).all(), total.tolist()
    third = ref.reference("posed", 1)[1][:, 2]                               # the view that stands aside sees nothing
    assert set(np.unique(third).tolist()) <= {ref.UNSEEN, ref.SKIPPED}


def _brute(points, K, pose, img, tol, window, z_min=ref.Z_MIN):
    """The same rule written the other way round: a padded image, whole-array masks over the (2 window + 1)^2 shifts."""
    H, W = img.shape
    u, v, z = ref.project(points, K, pose)
    with np.errstate(invalid='ignore', over='ignore'):
        seen = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > np.float64(np.float32(z_min)))
        zf = z.astype(np.float32).astype(np.float64)
    r = np.where(seen, np.nan_to_num(np.trunc(v), nan=0, posinf=0, neginf=0), 0).astype(int)
    c = np.where(seen, np.nan_to_num(np.trunc(u), nan=0, posinf=0, neginf=0), 0).astype(int)
    pad = np.zeros((H + 2 * window, W + 2 * window))
    pad[window:window + H, window:window + W] = img
    t = np.float64(np.float32(tol))
    n_valid = np.zeros(len(zf), int)
    n_agree = np.zeros(len(zf), int)
    n_front = np.zeros(len(zf), int)
    for dr in range(2 * window + 1):
        for dc in range(2 * window + 1):
            D = pad[r + dr, c + dc]
            with np.errstate(invalid='ignore'):
                ok = np.isfinite(D) & (D > 0)
                n_valid += ok
                n_agree += ok & (np.abs(zf - D) <= t * D)
                n_front += ok & (zf < D - t * D)
    out = np.where(n_agree > 0, ref.AGREE, np.where(n_front == n_valid, ref.IN_FRONT, ref.BEHIND))
    return np.where(seen & (n_valid > 0), out, ref.UNSEEN).astype(np.int8)


@pytest.mark.parametrize("window", [0, 1, 2])
def test_the_window_loop_agrees_with_a_second_brute_force(window):
    rng = np.random.default_rng(301)
    H, W, Q = 6, 7, 4000
    K = ref.camera(5.0, 4.5, 3.4, 2.9)
    z = rng.uniform(0.5, 3.0, Q)
    pts = np.stack([rng.uniform(-0.9, 0.9, Q) * z, rng.uniform(-0.9, 0.9, Q) * z, z * rng.choice([1, 1, 1, -1], Q)], axis=1).astype(np.float32)
    img = ref._spoil(rng.uniform(0.5, 3.0, (1, H, W)).astype(np.float32), rng, zeros=0.3)[0]
    for pose in (np.eye(4, dtype=np.float32), ref.pose_of([0.1, -0.2, 0.05], [0.1, 0.05, -0.2])):
        for tol in (0.05, 0.25):
            want = _brute(pts, K, pose, img, tol, window)
            got = ref.classes(pts, K, pose[None], img[None], tol=tol, window=window)[:, 0]
            np.testing.assert_array_equal(got, want)
            # (a 5 x 5 window covers most of this image: being in front of ALL of it is rare)
            assert all((got == k).sum() >= 20 for k in (ref.AGREE, ref.BEHIND, ref.UNSEEN) + ((ref.IN_FRONT,) if window < 2 else ()))


def test_the_hand_written_threshold_table_is_the_statement():
    c, expect = ref.case_thresholds()
    assert set(expect) >= {('A', 1), ('B', 2), ('B', 1), ('B', 0), ('C', 1)}
    for (view, window), table in expect.items():
        cls = ref.classes(c['points'], c['K'], c['poses'], c['depth'][view][None], tol=c['tol'], window=window)[:, 0]
        assert {k: int(cls[k]) for k in table} == table, (view, window)
    # the identity pose is never ambiguous; a posed point exactly on a pixel edge is
    assert not ref.ambiguous(c['points'], c['K'], c['poses'], c['depth']['A'][None], tol=c['tol']).any()
    shifted = ref.pose_of([0, 0, 0], [0, 0, -1.0])                            # z_c = z + 1
    pts = np.array([[0.0, 0.0, 1.0], [0.03125, 0.0, 1.0], [0.01, 0.013, 1.0], [0.01, 0.013, 1.5]], np.float32)
    K = ref.camera(16.0, 16.0, 8.0, 7.5)
    A = np.full((1, 20, 24), 2.0, np.float32)
    amb = ref.ambiguous(pts, K, shifted[None], A, tol=0.25)[:, 0]           # u = 8 (an edge); u = 8.25; clear; zf = 2.5 = D + b (a border)
    assert amb.tolist() == [True, False, False, True]


def test_the_keyframe_depth_loop_agrees_with_minimum_at_on_bit_patterns():
    rng = np.random.default_rng(302)
    H, W, P = 9, 11, 3000
    rows, cols = rng.integers(0, H, P), rng.integers(0, W, P)
    cols[rows == 4] = np.minimum(cols[rows == 4], 5)                         # a stretch of empty pixels
    z = rng.uniform(0.5, 4.0, P).astype(np.float32)
    z[rng.integers(0, P, 400)] = z[rng.integers(0, P, 400)]                   # repeated values
    z[:200:7], z[1:200:7], z[2:200:7], z[3:200:7] = np.nan, np.inf, 0.0, -1.0
    z[2000:2100] = np.float32(0.25)                                          # many exact ties at the front
    seg_of_point = np.sort(rng.integers(0, 6, P)).astype(np.int32)
    depth, seg = ref.keyframe_depth(rows, cols, z, seg_of_point, H, W)
    with np.errstate(invalid='ignore'):
        ok = (z > 0) & (z < np.inf)
    flat = rows * W + cols
    bits = np.full(H * W, 0xffffffff, np.uint32)
    np.minimum.at(bits, flat[ok], z[ok].view(np.uint32))                      # positive floats order as their bit patterns
    winner = np.full(H * W, -1, np.int64)
    at_min = ok & (z.view(np.uint32) == bits[flat])
    np.maximum.at(winner, flat[at_min], np.nonzero(at_min)[0])                # equal z: the highest index
    hit = winner >= 0
    assert 0 < hit.sum() < H * W
    np.testing.assert_array_equal(depth.view(np.uint32).ravel()[hit], bits[hit])
    assert not depth.ravel()[~hit].any() and (seg.ravel()[~hit] == -1).all()
    np.testing.assert_array_equal(seg.ravel()[hit], seg_of_point[winner[hit]])
    assert len(set(seg.ravel()[depth.ravel() == np.float32(0.25)].tolist())) >= 1 and (depth == np.float32(0.25)).sum() >= 20


def test_decode_pix_and_the_keyframe_case():
    r, c = ref.decode_pix(np.array([(1 << 31) | (36 << 16) | 52, (5 << 16) | 7], np.uint32).view(np.int32))
    assert r.tolist() == [36, 5] and c.tolist() == [52, 7]
    kfs = ref.case_keyframes()
    assert [k['masks'].shape for k in kfs] == [(5, 37, 53), (3, 37, 53)]
    a, b = kfs
    assert a['masks'][4].sum() == 0 and b['masks'][1].sum() == 0             # one empty segment each
    assert (a['masks'][1] & ~a['masks'][0]).sum() == 0                       # nested
    assert (a['masks'][0] & a['masks'][2]).sum() > 0 and (a['masks'][2] & ~a['masks'][0]).sum() > 0      # overlapping
    dup = a['masks'][3]
    assert (dup & ~a['masks'][0]).sum() == 0 and np.array_equal(a['L'][3][dup], a['L'][0][dup]) and a['kld'][3] == a['kld'][0]
    assert np.isnan(a['kld'][1]) and b['kld'][0] == 200.0
    assert (~a['masks'].any(0)).sum() > 0 and (~b['masks'].any(0)).sum() > 0  # pixels no segment covers
