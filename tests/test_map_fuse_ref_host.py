"""CPU-only: the explicit loop of tests/map_fuse_ref.py held to a second formulation (whole-array NumPy float64, ``np.unique`` on the
keys, ``np.add.at`` on int64), the derived bound of the fused position against the float64 mean of the members, and the preconditions
of the device cases (tests/test_gpu_map_fuse.py): each case is what it claims to be."""
import numpy as np
import pytest

import map_fuse_ref as ref


def _vectorised(points, colours, voxel, origin):
    """The same rule, whole arrays at a time: returns per fused row (in ascending order of the first member row) key, n, S, C, i0, and
    per input row the label."""
    p = np.asarray(points, np.float32).astype(np.float64)
    v, o = np.float64(np.float32(voxel)), np.asarray(origin, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        q = (p - o) / v
        g = np.floor(q)
        kept = np.isfinite(q).all(axis=1) & ((g >= -ref.HALF) & (g <= ref.HALF - 1)).all(axis=1)
    rows = np.nonzero(kept)[0]
    q, g = q[rows], g[rows]
    cell = g.astype(np.int64) + ref.HALF
    key = cell[:, 0] << 42 | cell[:, 1] << 21 | cell[:, 2]
    s = np.minimum(np.trunc((q - g) * 65536.0).astype(np.int64), 65535)
    with np.errstate(invalid='ignore'):
        c255 = np.asarray(colours, np.float32).astype(np.float64)[rows] * 255.0
        c8 = np.where(c255 > 0, np.minimum(np.nan_to_num(np.trunc(c255), nan=0.0), 255.0), 0.0).astype(np.int64)
    uniq, inverse = np.unique(key, return_inverse=True)
    n = np.zeros(len(uniq), np.int64)
    S, C = np.zeros((len(uniq), 3), np.int64), np.zeros((len(uniq), 3), np.int64)
    i0 = np.full(len(uniq), len(p), np.int64)
    np.add.at(n, inverse, 1)
    np.add.at(S, inverse, s)
    np.add.at(C, inverse, c8)
    np.minimum.at(i0, inverse, rows)
    order = np.argsort(i0)
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    label = np.full(len(p), -1, np.int64)
    label[rows] = rank[inverse]
    return uniq[order], n[order], S[order], C[order], i0[order], label, g, rows


def _cases():
    p, c = ref.case_random()
    for k, (voxel, origin) in enumerate(ref.SETTINGS):
        yield f"random {k}", p, c, voxel, origin, ref.reference_random(k)
    yield ("random at voxel 1",) + (p, c, 1.0, (0.0, 0.0, 0.0), ref.fuse(p, c, 1.0, (0.0, 0.0, 0.0)))
    for name, case in (("full load", ref.case_full_load()), ("one voxel", ref.case_contention(1)), ("two voxels", ref.case_contention(2))):
        yield (name,) + case + (ref.fuse(*case),)


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_the_loop_against_the_whole_array_formulation_and_the_bound(case):
    name, p, c, voxel, origin, got = case
    key, n, S, C, i0, label, g, rows = _vectorised(p, c, voxel, origin)
    M = len(key)
    assert got['n'] == M and got['points'].shape == (M, 3) and got['points'].dtype == np.float32
    np.testing.assert_array_equal(got['keys'].astype(np.int64), key)
    np.testing.assert_array_equal(got['count'], n)
    np.testing.assert_array_equal(got['first'], i0)
    np.testing.assert_array_equal(got['sums'].astype(np.int64), S)
    np.testing.assert_array_equal(got['colour_sums'].astype(np.int64), C)
    np.testing.assert_array_equal(got['label'], label)
    assert (np.diff(got['first']) > 0).all() and n.sum() == len(rows)
    # positions and colours from the sums, whole arrays at a time
    v, o = np.float64(np.float32(voxel)), np.asarray(origin, np.float32).astype(np.float64)
    cell = np.stack([(key >> 42) & 0x1fffff, (key >> 21) & 0x1fffff, key & 0x1fffff], axis=1) - ref.HALF
    m = S.astype(np.float64) / n[:, None].astype(np.float64)
    want = ((cell.astype(np.float64) + (m + 0.5) / 65536.0) * v + o).astype(np.float32)
    np.testing.assert_array_equal(got['points'].view(np.uint32), want.view(np.uint32))
    want_c = (C.astype(np.float64) / (255.0 * n[:, None].astype(np.float64))).astype(np.float32)
    np.testing.assert_array_equal(got['colours'].view(np.uint32), want_c.view(np.uint32))
    # the derived bound: per coordinate less than voxel 2^-16 from the float64 mean of the members (the quantisation with its half-step
    # offset contributes voxel 2^-17; the float64 roundings and the one float32 rounding of the result are far below the rest)
    mean = np.zeros((M, 3))
    np.add.at(mean, label[rows], p[rows].astype(np.float64))
    mean /= n[:, None]
    err = np.abs(got['points'].astype(np.float64) - mean)
    print(f"\n{name}: M = {M}, max n = {n.max()}, dropped {len(p) - len(rows)}; largest |fused - mean| = {err.max():.3e} = "
          f"{err.max() / (v * 2.0 ** -16):.3f} x voxel 2^-16")
    assert (err < v * 2.0 ** -16).all()
    # no fused point left its own voxel after the float32 rounding
    assert (np.floor((got['points'].astype(np.float64) - o) / v) == cell).all()


def test_the_random_case_is_what_it_claims():
    p, c = ref.case_random()
    assert p.shape == (5003, 3) and p.dtype == np.float32 and -(-5003 // 256) == 20
    got = ref.reference_random(0)
    assert (got['count'] >= 4).sum() >= 20
    q = p.astype(np.float64) / 0.25
    with np.errstate(invalid='ignore'):
        on_face = np.isfinite(q).all(axis=1) & (q == np.floor(q)).any(axis=1)
    assert on_face.sum() >= 20 and on_face[::ref.FACE_EVERY].sum() >= 20
    assert (p < 0).any() and np.signbit(p[ref.NEG_ZERO_ROW]).all() and (p[ref.NEG_ZERO_ROW] == 0).all()
    assert np.isnan(p[ref.BAD_ROWS[0]]).sum() == 1 and np.isposinf(p[ref.BAD_ROWS[1]]).sum() == 1 and (p[ref.BAD_ROWS[2]] == 1e7).all()
    assert np.nanmin(c) < 0 and np.nanmax(c) > 1 and np.isnan(c).sum() == 1
    for k in range(len(ref.SETTINGS)):
        label = ref.reference_random(k)['label']
        assert np.nonzero(label < 0)[0].tolist() == list(ref.BAD_ROWS), k             # exactly the constructed bad rows are dropped
    assert ref.reference_random(0)['label'][ref.NEG_ZERO_ROW] >= 0
    coarse = ref.fuse(p, c, 1.0, (0.0, 0.0, 0.0))
    print(f"\nrandom case: voxel 0.25: M = {got['n']}, max n = {got['count'].max()}; voxel 1.0: M = {coarse['n']}, max n = {coarse['count'].max()}")
    assert coarse['n'] < 100 and coarse['count'].max() >= 50


def test_the_other_cases_are_what_they_claim():
    p, c, voxel, origin = ref.case_full_load()
    got = ref.fuse(p, c, voxel, origin)
    assert len(p) == 4096 and got['n'] == 4096 and (got['count'] == 1).all()
    np.testing.assert_array_equal(got['first'], np.arange(4096))
    np.testing.assert_array_equal(got['label'], np.arange(4096))
    assert (np.diff(got['keys'].astype(np.int64)) < 0).any()                          # shuffled: the keys do not arrive in order
    one = ref.fuse(*ref.case_contention(1))
    assert one['n'] == 1 and one['count'].tolist() == [3000] and one['first'].tolist() == [0] and not one['label'].any()
    two = ref.fuse(*ref.case_contention(2))
    assert two['n'] == 2 and two['count'].tolist() == [1500, 1500] and two['first'].tolist() == [0, 1]
    np.testing.assert_array_equal(two['label'], np.arange(3000) % 2)


def test_a_permutation_reorders_the_rows_and_keeps_the_voxels():
    p, c = ref.case_random()
    perm = np.random.default_rng(77).permutation(len(p))
    a, b = ref.reference_random(0), ref.fuse(p[perm], c[perm], *ref.SETTINGS[0])
    assert a['n'] == b['n'] and not np.array_equal(a['keys'], b['keys'])
    def bag(r):
        return sorted((int(k), int(n), tuple(map(int, S)), tuple(map(int, C))) for k, n, S, C in zip(r['keys'], r['count'], r['sums'], r['colour_sums']))
    assert bag(a) == bag(b)


def test_a_point_just_below_a_face_stays_inside_its_voxel():
    """q in (-2^-54, 0): g = -1 and q - g rounds to 1; the sub-voxel position is held at 65535, not 65536."""
    p = np.array([[-1e-30, 0.5, 0.5]], np.float32)
    got = ref.fuse(p, None, 1.0, (0.0, 0.0, 0.0))
    assert got['sums'][0].tolist() == [65535, 32768, 32768] and got['keys'][0] >> 42 == ref.HALF - 1
    assert -1.0 < got['points'][0, 0] < 0.0
