"""-m gpu: the k nearest neighbours of the map neighbourhoods (csrc/sp_knn.hip sp_cloud_grid_knn through the C ABI, ``tool/viz.py``
``nearest_k``) against the float64 reference of tests/cloud_knn_ref.py.

Everything is compared EXACTLY: ``index`` and ``count`` equal, ``dist`` equal as uint32 bit patterns.  Every call writes into outputs
and a scratch pre-filled with 0x7f bytes, and no entry of any output may be left as it was."""
import numpy as np
import pytest
import torch

import cloud_knn_ref as ref
import map_nearest_ref as base
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK32 = 0x7f7f7f7f


def _raw(queries, points, radius, origin, k, skip_self=0, builds=1, nearest=False):
    """Build and query through the C ABI on a junk-filled scratch and junk-filled outputs; returns the host arrays (with ``nearest``
    also what sp_cloud_grid_nearest answers from the same scratch, under 'one')."""
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
    index, dist, count = junk(Qa, k), junk(Qa, k), junk(Qa)
    _lib.check(lib.sp_cloud_grid_knn(_lib.ptr(qs), Qa, Q, _lib.ptr(scratch), int(skip_self), k, _lib.ptr(index), _lib.ptr(dist), _lib.ptr(count),
                                     _lib.stream_ptr()), "sp_cloud_grid_knn")
    out = dict(index=npy(index), dist=npy(dist).view(np.float32), count=npy(count))
    if nearest:
        i1, d1, c1 = junk(Qa), junk(Qa), junk(Qa)
        _lib.check(lib.sp_cloud_grid_nearest(_lib.ptr(qs), Qa, Q, _lib.ptr(scratch), int(skip_self), _lib.ptr(i1), _lib.ptr(d1), _lib.ptr(c1),
                                             _lib.stream_ptr()), "sp_cloud_grid_nearest")
        out['one'] = dict(index=npy(i1), dist=npy(d1).view(np.float32), count=npy(c1))
    torch.cuda.synchronize()
    return out


def _check(got, want, what):
    """Bit for bit against the reference; no entry left as it was; the padding is -1 and +inf."""
    np.testing.assert_array_equal(got['count'], want['count'], err_msg=f"{what}: count")
    np.testing.assert_array_equal(got['index'], want['index'], err_msg=f"{what}: index")
    np.testing.assert_array_equal(got['dist'].view(np.uint32), want['dist'].view(np.uint32), err_msg=f"{what}: dist")
    for key in ('index', 'dist', 'count'):
        assert not (got[key].view(np.uint32) == JUNK32).any(), f"{what}: {key} has entries that were not written"
    assert np.array_equal(got['index'] < 0, np.isposinf(got['dist']))


@pytest.mark.parametrize("setting,k", ref.RANDOM_CASES)
def test_random_clouds(setting, k):
    """Qa = 5003 against Q = 3001 with a NaN row, a +inf row, a row out of range and a -0.0: lists that are cut (count > k) and lists that
    are padded (count < k) in one call."""
    a, b = base.case_random()
    radius, origin = base.SETTINGS[setting]
    want = ref.reference_random(setting, k)
    got = _raw(a, b, radius, origin, k)
    cut = float((got['count'] > k).mean())
    print(f"\nr {radius}, origin {origin}, k {k}: {cut:.3f} of the rows have more than k neighbours, largest count {got['count'].max()}")
    _check(got, want, f"r {radius}, origin {origin}, k {k}")
    assert 0.002 < cut < 0.99                                                  # (cannot pass on all-padding or all-full output)
    for bad in base.BAD_ROWS:
        assert (got['index'][bad] == -1).all() and got['count'][bad] == 0 and np.isposinf(got['dist'][bad]).all() and not (got['index'] == bad).any()


def test_the_cloud_against_itself_with_skip_self():
    """The 3001 points against themselves at r = 0.4, k = 8: counts up to 28, nearly every list full, no row lists itself."""
    p = base.case_random()[1]
    got = _raw(p, p, ref.SELF_RADIUS, (0.0, 0.0, 0.0), ref.SELF_K, skip_self=1)
    _check(got, ref.reference_self(), "skip_self")
    assert got['count'].max() >= 20 and (got['count'] > 5).mean() > 0.9 and not (got['index'] == np.arange(len(p))[:, None]).any()


@pytest.mark.parametrize("skip_self", [0, 1])
def test_k_1_is_the_nearest_query_to_the_bit(skip_self):
    a, b = base.case_random()
    radius, origin = base.SETTINGS[1]
    got = _raw(b if skip_self else a, b, radius, origin, 1, skip_self=skip_self, nearest=True)
    one = got['one']
    assert got['index'][:, 0].tobytes() == one['index'].tobytes() and got['dist'][:, 0].tobytes() == one['dist'].tobytes()
    assert got['count'].tobytes() == one['count'].tobytes() and (one['index'] >= 0).mean() > 0.5


@pytest.mark.parametrize("origin", range(len(base.LATTICE_ORIGINS)))
def test_lattice(origin):
    """Interior lattice points have six neighbours at exactly r: with k = 4 the cut falls inside a tie, and the row order decides it."""
    a, b = base.case_lattice()
    o = base.LATTICE_ORIGINS[origin]
    want = ref.knn(a, b, base.LATTICE_R, o, 4)
    got = _raw(a, b, base.LATTICE_R, o, 4)
    _check(got, want, f"lattice, origin {o}")
    assert ((want['count'] > 4) & (want['d2'][:, 3] == base.LATTICE_R ** 2)).sum() > 100


def test_one_long_cell():
    """3000 reference rows in ONE cell, 256 queries within r of all of them, k = 32: every lane inserts many times into a full list."""
    a, b, radius, origin = base.case_one_cell()
    got = _raw(a, b, radius, origin, 32)
    _check(got, ref.knn(a, b, radius, origin, 32), "one cell")
    assert (got['count'] == 3000).all() and (got['index'] >= 0).all()


def test_the_table_at_its_highest_load():
    a, b, radius, origin = base.case_full_load()
    got = _raw(a, b, radius, origin, 2)
    _check(got, ref.knn_candidates(a, b, radius, origin, 2), "full load")
    assert (got['index'][:, 0] >= 0).mean() > 0.9 and 0 < (got['index'][:, 1] >= 0).mean() < 1


@pytest.mark.parametrize("Q", [1, 255, 256, 257])
@pytest.mark.parametrize("Qa", [1, 255, 256, 257])
def test_sizes(Qa, Q):
    """Around one workgroup of every shipped size, with k = 5."""
    a, b = base.case_sizes(Qa, Q)
    radius, origin = 0.9, base.SIZES_SETTING[1]
    got = _raw(a, b, radius, origin, 5)
    _check(got, ref.knn_candidates(a, b, radius, origin, 5), f"Qa = {Qa}, Q = {Q}")
    if Q >= 255 and Qa >= 255:
        assert (got['count'] > 5).any() and (got['count'] < 5).any()


def test_more_than_65536_rows_with_k_32():
    """70 001 queries against 70 001 points with k = 32: entries beyond 2^21 of the (Qa, k) outputs, rows beyond 65 535."""
    a, b = base.case_sizes(70001, 70001)
    radius, origin = base.SIZES_SETTING
    got = _raw(a, b, radius, origin, 32)
    _check(got, ref.knn_candidates(a, b, radius, origin, 32), "70 001 x 70 001, k = 32")
    assert got['index'].max() > 65535 and (got['count'] > 32).any() and (got['count'] < 32).any()


@pytest.mark.parametrize("k", [1, 7, 8, 9, 16, 17, 32])
def test_every_capacity_boundary(k):
    """One small cloud against itself at r = 0.9 (counts from 0 to over 40): the list kernels of capacity 8, 16 and 32 at their edges."""
    p = ref.small_cloud()
    got = _raw(p, p, 0.9, (0.0, 0.0, 0.0), k)
    want = ref.knn(p, p, 0.9, (0.0, 0.0, 0.0), k)
    _check(got, want, f"k = {k}")
    assert want['count'].max() > 32 and (want['count'] < k).any()
    again = _raw(p, p, 0.9, (0.0, 0.0, 0.0), k, skip_self=1)
    _check(again, ref.knn(p, p, 0.9, (0.0, 0.0, 0.0), k, skip_self=True), f"k = {k}, skip_self")


def test_two_runs_give_the_same_bits_and_a_permutation_renames_the_rows():
    """Two runs (and a second build on the used scratch) give the same bits.  With the reference rows permuted ``count`` and ``dist`` keep
    their bits, and ``index`` maps back through the permutation on every row whose listed d2 are pairwise distinct."""
    a, b = base.case_random()
    radius, origin = base.SETTINGS[1]
    k = 8
    first, again, rebuilt = _raw(a, b, radius, origin, k), _raw(a, b, radius, origin, k), _raw(a, b, radius, origin, k, builds=2)
    for key in ('index', 'dist', 'count'):
        assert first[key].tobytes() == again[key].tobytes() == rebuilt[key].tobytes(), key
    perm = np.random.default_rng(77).permutation(len(b))
    moved = _raw(a, b[perm], radius, origin, k)
    _check(moved, ref.knn(a, b[perm], radius, origin, k), "permuted")
    assert moved['dist'].tobytes() == first['dist'].tobytes() and moved['count'].tobytes() == first['count'].tobytes()
    d2 = ref.reference_random(1, k)['d2']
    distinct = ~((d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])).any(axis=1)
    assert distinct.mean() > 0.9
    back = np.where(moved['index'] >= 0, perm[np.maximum(moved['index'], 0)], -1)
    assert np.array_equal(back[distinct], first['index'][distinct]) and not np.array_equal(moved['index'], first['index'])


def test_the_python_surface_gives_the_same_and_checks_its_handle():
    from super_primitive_amd.tool import viz
    a, b = base.case_random()
    radius, origin = base.SETTINGS[1]
    grid = viz.cloud_grid(T(b), radius, origin)
    out = viz.nearest_k(T(a), grid, 8)
    assert out['index'].dtype == torch.int32 and out['dist'].dtype == torch.float32 and out['count'].dtype == torch.int32
    assert tuple(out['index'].shape) == (len(a), 8) == tuple(out['dist'].shape) and tuple(out['count'].shape) == (len(a),)
    _check({k: npy(v) for k, v in out.items()}, ref.reference_random(1, 8), "nearest_k")
    one, first = viz.nearest_points(T(a), grid), viz.nearest_k(T(a), grid, 1)
    assert torch.equal(first['index'][:, 0], one['index']) and torch.equal(first['count'], one['count'])
    assert npy(first['dist'][:, 0]).tobytes() == npy(one['dist']).tobytes()
    with pytest.raises(ValueError, match="scratch"):
        viz.nearest_k(T(a), dict(grid, scratch=grid['scratch'][:-1]), 4)
    with pytest.raises(ValueError, match="skip_self"):
        viz.nearest_k(T(a), grid, 4, skip_self=True)
    with pytest.raises(ValueError, match="k "):
        viz.nearest_k(T(a), grid, 33)
