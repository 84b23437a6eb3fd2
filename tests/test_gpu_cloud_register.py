"""-m gpu: map registration (csrc/sp_register.hip ``sp_cloud_register`` through the C ABI, ``tool/viz.py`` ``register_clouds`` and
``odometery/results.py`` ``register_map`` / ``transform_map``) against the float64 reference of tests/cloud_register_ref.py.

Every raw call writes into a state, a history, an index and a work buffer pre-filled with 0x7f bytes (only rot, trans and s of the
state are the caller's).  The moved points, residuals and Jacobians of the device are the reference's to the bit, so ``index`` and ``n``
are compared exactly; the sums differ by their order only and are held to (n + 8) 2^-52 sum|term| per entry; the solve is held to the
backward-error bound of LDL^T on the device's OWN stored system, and the new transform to the retraction of the device's OWN delta."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import cloud_register_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

JUNK32 = 0x7f7f7f7f
U = 2.0 ** -53
IDENTITY = dict(R=np.eye(3), t=np.zeros(3), s=1.0)


def _raw(a, normals, b, kind, scale, start=IDENTITY, huber=0.0, tol=1e-6, min_pairs=None, max_iters=1, radius=ref.RADIUS, origin=ref.ORIGIN):
    """Build the grid over ``b`` and register ``a`` onto it through the C ABI on junk-filled buffers; returns the host arrays."""
    from super_primitive_amd import _lib
    lib = _lib.load()
    Q, Qa = len(b), len(a)
    pts, qs = T(np.asarray(b, np.float32)), T(np.asarray(a, np.float32))
    nrm = None if normals is None else T(np.asarray(normals, np.float32))
    dev = pts.device
    junk = lambda n: torch.full((n,), JUNK32, dtype=torch.int32, device=dev)
    scratch = junk(lib.sp_cloud_grid_scratch_units(Q) * 16)
    _lib.check(lib.sp_cloud_grid_build(_lib.ptr(pts), Q, float(radius), float(origin[0]), float(origin[1]), float(origin[2]), _lib.ptr(scratch),
                                       _lib.stream_ptr()), "sp_cloud_grid_build")
    host = np.full(128, JUNK32, np.int32).view(np.float64)
    host[:9], host[9:12], host[12] = np.asarray(start['R'], np.float64).reshape(9), start['t'], start['s']
    state = T(host.copy())
    assert lib.sp_cloud_register_work_doubles(Qa) == 40 * ((Qa + 255) // 256)
    history, index, work = junk(8 * max_iters), junk(Qa), junk(2 * lib.sp_cloud_register_work_doubles(Qa))
    _lib.check(lib.sp_cloud_register(_lib.ptr(qs), _lib.ptr(nrm), Qa, Q, _lib.ptr(scratch), kind, int(scale), float(huber), float(tol),
                                     (7 if scale else 6) if min_pairs is None else min_pairs, max_iters, _lib.ptr(state), _lib.ptr(history), _lib.ptr(index),
                                     _lib.ptr(work), _lib.stream_ptr()), "sp_cloud_register")
    torch.cuda.synchronize()
    st = npy(state)
    return dict(R=st[:9].reshape(3, 3).copy(), t=st[9:12].copy(), s=float(st[12]), H=st[13:41].copy(), g=st[41:48].copy(), delta=st[48:55].copy(),
                cost=float(st[55]), step=float(st[56]), n=int(st.view(np.int64)[57]), status=int(st.view(np.int32)[116]),
                iterations=int(st.view(np.int32)[117]), history=npy(history).view(np.float64).reshape(max_iters, 4), index=npy(index), state=st)


def _bits(out):
    return out['state'][:59].tobytes() + out['history'].tobytes() + out['index'].tobytes()


def _check_sums(got, first, what):
    """H, g and the cost of the device's state against the reference's first iteration: index and n exact, every entry within
    (n + 8) 2^-52 sum|term| -- a sum of n terms in ANY order is within (n - 1) u sum|term| of the exact one, u = 2^-53, and so is the
    reference's; the terms themselves differ by nothing (the same operations on the same bits)."""
    np.testing.assert_array_equal(got['index'], first['index'], err_msg=f"{what}: index")
    assert not (got['index'].view(np.uint32) == JUNK32).any(), f"{what}: index has rows that were not written"
    assert got['n'] == first['n'], what
    sums = np.concatenate([got['H'], got['g'], [got['cost']]])
    bound = (first['n'] + 8) * 2.0 ** -52 * first['abs']
    err = np.abs(sums - first['sums'])
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"\n{what}: n {got['n']}, worst |sum - reference| / bound {worst:.3f}")
    assert (err <= bound).all(), f"{what}: entries {np.nonzero(err > bound)[0]} of (H, g, cost) are off by {err[err > bound]} (bound {bound[err > bound]})"
    return worst


def _check_solve(got, m, what):
    """|| H delta + g ||_2 over the device's own stored H, g and delta, evaluated exactly (rationals), against the backward error of the
    solve.  LDL^T of a symmetric positive definite H is Cholesky's R^T R with R = D^(1/2) L^T computed without the square roots: the
    same products and sums.  Higham, Accuracy and Stability of Numerical Algorithms, Theorems 10.3 / 10.4: the computed solution satisfies
    (H + dH) x = -g with |dH| <= gamma_(3m+1) |R^T| |R|, gamma_k = k u / (1 - k u), u = 2^-53, and (10.7) || |R^T| |R| ||_2 <=
    m (1 - m gamma_(m+1))^-1 ||H||_2.  The kernel multiplies by 1 / d_j where Cholesky divides -- one more rounding in every entry of L
    and of D^-1 y: gamma_(3m+3).  So || H x + g ||_2 = || dH x ||_2 <= gamma_(3m+3) m (1 - m gamma_(m+1))^-1 ||H||_2 ||x||_2; fused
    multiply-adds in the solve only remove roundings."""
    H, g, x = ref.full(got['H'], m), got['g'][:m], got['delta'][:m]
    res = [sum(Fraction(float(H[i, j])) * Fraction(float(x[j])) for j in range(m)) + Fraction(float(g[i])) for i in range(m)]
    norm = float(sum(r * r for r in res)) ** 0.5
    gamma = lambda k: k * U / (1 - k * U)
    bound = gamma(3 * m + 3) * m / (1 - m * gamma(m + 1)) * float(np.linalg.norm(H, 2)) * float(np.linalg.norm(x))
    print(f"{what}: || H delta + g || = {norm:.3e}, bound {bound:.3e}")
    assert norm <= bound, what
    assert not got['delta'][m:].any()


def _check_retraction(got, start, m, what):
    """The stored transform against the retraction of the stored delta recomputed in NumPy: the formulas of the contract, sin / cos / exp
    each within an ulp or two of NumPy's -- 4 ulps of the largest magnitude that enters the entry."""
    R, t, s = ref.retract(np.asarray(start['R'], np.float64), np.asarray(start['t'], np.float64), float(start['s']), got['delta'])
    ulp = 2.0 ** -52
    assert np.abs(got['R'] - R).max() <= 4 * ulp, what
    assert np.abs(got['t'] - t).max() <= 4 * ulp * max(np.abs(start['t']).max(), np.abs(got['delta'][3:6]).max(), np.abs(t).max()), what
    assert abs(got['s'] - s) <= 4 * ulp * abs(s), what
    assert abs(got['step'] - ref.step_length(got['delta'], m)) <= 2 * ulp * got['step'], what


def _one_iteration(a, an, b, bn, kind, scale, what, order=None):
    """One enqueued iteration from START with huber = 0.03 (weights on both sides of 1) against the reference; ``order``: the query rows
    the device gets (a permutation) -- the reference keeps its own order."""
    m = 7 if scale else 6
    want = ref.check_gap(ref.run(a, an, b, bn, kind, scale, huber=0.03, tol=0.0, max_iters=1, **ref.START))
    normals = {0: None, 1: bn, 2: an}[kind]
    if order is not None:
        a, normals = a[order], (normals[order] if kind == 2 else normals)
    got = _raw(a, normals, b, kind, scale, start=ref.START, huber=0.03, tol=0.0, max_iters=1)
    first = dict(want['first'], index=want['first']['index'] if order is None else want['first']['index'][order])
    _check_sums(got, first, what)
    assert got['status'] == ref.MAX_ITERS and got['iterations'] == 1 and want['status'] == ref.MAX_ITERS
    _check_solve(got, m, what)
    _check_retraction(got, ref.START, m, what)
    np.testing.assert_array_equal(got['history'][0], [got['n'], got['cost'], got['step'], ref.MAX_ITERS])
    assert np.abs(got['delta'] - want['first']['delta']).max() <= 1e-9                     # (the same step as the reference's, loosely)
    return got, want


# ---- one iteration ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_one_iteration(kind, scale):
    """Qa = 5003 (20 workgroups, the last one partial) against Q = 3001, both clouds with a NaN row, a +inf row and a row out of range, and
    a good row with a NaN normal (never a pair: as a query's own normal for kind 2, as the neighbour's normal for kind 1)."""
    a, an, b, bn = ref.case_one_iteration()
    got, want = _one_iteration(a, an, b, bn, kind, scale, f"kind {kind}, scale {scale}")
    assert 4000 < got['n'] <= len(a) - 3
    for bad in ref.BAD_ROWS:
        assert got['index'][bad] == -1 and not (got['index'] == bad).any()
    if kind == 1:
        assert not (got['index'] == ref.BAD_NORMAL_ROW).any()
        plain = _raw(a, None, b, 0, scale, start=ref.START, tol=0.0)
        assert (plain['index'] == ref.BAD_NORMAL_ROW).sum() == plain['n'] - got['n'] > 0    # those queries do have that neighbour
    if kind == 2:
        assert got['index'][ref.BAD_NORMAL_ROW] == -1
    if not scale:
        assert not got['H'][[6, 12, 17, 21, 24, 26, 27]].any() and got['g'][6] == 0.0 and got['delta'][6] == 0.0 and got['s'] == ref.START['s']


@pytest.mark.parametrize("Qa", [255, 256, 257, 70001])
def test_block_edges(Qa):
    """One workgroup short of a row, exactly one, one row into the second, and 70 001 rows: 274 partial records, more than one per thread
    of the solve pass's strided sums."""
    a, an = ref.samples(Qa, 701, bad=True)
    b, bn = ref.samples(ref.Q_REF, 702, bad=True)
    _one_iteration(a, an, b, bn, 1, 1, f"Qa = {Qa}")
    _one_iteration(a, an, b, bn, 0, 0, f"Qa = {Qa}, point to point")


def test_one_query_is_too_few():
    a, an = ref.samples(1, 701)
    b, bn = ref.samples(ref.Q_REF, 702, bad=True)
    got = _raw(a, an, b, 2, 1, start=ref.START, max_iters=3)
    assert got['status'] == ref.FEW and got['n'] == 1 and got['index'][0] >= 0 and got['iterations'] == 1
    assert got['state'][:13].tobytes() == np.concatenate([ref.START['R'].reshape(9), ref.START['t'], [ref.START['s']]]).tobytes()
    np.testing.assert_array_equal(got['history'][:, 3], [ref.FEW] * 3)
    assert got['history'][0, 0] == 1 and not got['history'][1:, :3].any() and not got['delta'].any() and got['step'] == 0.0


# ---- whole runs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference_identical(kind):
    a, an, b, bn = ref.case_identical()
    return ref.check_gap(ref.run(a, an, b, bn, kind, True, tol=1e-10, max_iters=40))


def _errors(out):
    return (ref.rotation_angle(out['R'], ref.TRUTH['R']), float(np.abs(out['t'] - ref.TRUTH['t']).max()), abs(out['s'] - ref.TRUTH['s']))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_recovery_of_a_known_similarity(kind):
    """Identical points under TRUTH, from the identity, with the scale: CONVERGED, t and s within e = 2^-24 max|coordinate| of the truth
    and the rotation within e over the cloud's RMS radius -- each query row is off its twin by at most e per coordinate (its float32
    rounding) and the estimate averages the rows.  The reference meets the same bound."""
    a, an, b, bn = ref.case_identical()
    want = _reference_identical(kind)
    got = _raw(a, {0: None, 1: bn, 2: an}[kind], b, kind, 1, tol=1e-10, max_iters=40)
    e = 2.0 ** -24 * float(np.abs(b).max())
    radius = float(np.sqrt((b.astype(np.float64) ** 2).sum(axis=1).mean()))
    for name, out in (("device", got), ("reference", want)):
        rot, trans, scale = _errors(out)
        print(f"\nkind {kind}, {name}: {out['iterations']} iterations, rotation {rot:.2e} (bound {e / radius:.2e}), translation {trans:.2e}, scale {scale:.2e} "
              f"(bound {e:.2e})")
        assert out['status'] == ref.CONVERGED and rot <= e / radius and trans <= e and scale <= e, name
    assert got['iterations'] == want['iterations'] and got['n'] == len(a) and np.array_equal(got['index'], np.arange(len(a)))
    it = got['iterations']
    assert (got['history'][:it - 1, 3] == ref.RUNNING).all() and (got['history'][it - 1:, 3] == ref.CONVERGED).all() and not got['history'][it:, :3].any()
    assert got['history'][it - 1, 2] == got['step'] <= 1e-10 and (got['history'][:it - 1, 2] > 1e-10).all()


def _tolerance(want, back):
    """How far the device's final transform may lie from the reference's: 64 x the spread of the reference against itself with its sums
    in reversed row order, floored at cond(H) (n + 8) 2^-52 -- a relative perturbation (n + 8) 2^-52 of the sums moves the solution of
    H delta = -g by cond(H) times as much, and the iteration's fixed point with it; the factor 64 covers 1 / (1 - rho) for the
    contraction rho of the last steps (read off the reference's history: the steps shrink by more than 10 x per iteration, rho < 0.1)."""
    steps = want['history'][:want['iterations'], 2]
    assert (steps[1:] < 0.5 * steps[:-1]).all(), steps
    spread = ref.difference(want, back)
    return max(64 * spread, want['cond'] * (want['n'] + 8) * 2.0 ** -52), spread


@pytest.mark.parametrize("kind", [1, 2])
def test_independent_samples_end_where_the_reference_ends(kind):
    """Independent samples of one surface, the plane kinds with the scale: the final transform against the reference's, within
    ``_tolerance``.  Measured on the MI355X (profiles/cloud_register.txt has the lines this test prints): device - reference 6.5e-16
    (kind 1) and 1.4e-15 (kind 2), the reference against its own reversed sums 6.1e-16 and 8.5e-16, tolerance 3.2e-9 and 3.3e-9 (the
    floor cond(H) (n + 8) 2^-52 with cond(H) 7272 / 7329, n = 2003); 5 iterations on both sides."""
    a, an, b, bn = ref.case_independent()
    want = ref.check_gap(ref.run(a, an, b, bn, kind, True, tol=1e-9, max_iters=40))
    back = ref.run(a, an, b, bn, kind, True, tol=1e-9, max_iters=40, reverse=True)
    tolerance, spread = _tolerance(want, back)
    got = _raw(a, bn if kind == 1 else an, b, kind, 1, tol=1e-9, max_iters=40)
    diff = ref.difference(got, want)
    print(f"\nindependent samples, kind {kind}: device - reference {diff:.3e}; reference against its reversed sums {spread:.3e}; tolerance {tolerance:.3e} "
          f"(cond(H) {want['cond']:.0f}, n {want['n']}); {got['iterations']} iterations")
    assert got['status'] == ref.CONVERGED == want['status'] and got['iterations'] == want['iterations'] and got['n'] == want['n']
    assert np.array_equal(got['index'], want['index']) and diff <= tolerance


@pytest.mark.parametrize("kind", [1, 2])
def test_huber(kind):
    """Every 20th query displaced by 0.2 along z, a rigid fit.  First on the CPU: the reference with huber = 0.02 ends closer to the truth
    than without; then the device ends where the reference ends."""
    a, an, b, bn = ref.case_outliers()
    plain = ref.run(a, an, b, bn, kind, False, tol=1e-9, max_iters=40)
    want = ref.check_gap(ref.run(a, an, b, bn, kind, False, huber=0.02, tol=1e-9, max_iters=40))
    err = lambda o: float(np.abs(o['t'] - ref.TRUTH['t']).max())
    assert want['status'] == ref.CONVERGED and err(want) < 0.2 * err(plain)
    back = ref.run(a, an, b, bn, kind, False, huber=0.02, tol=1e-9, max_iters=40, reverse=True)
    tolerance, spread = _tolerance(want, back)
    got = _raw(a, bn if kind == 1 else an, b, kind, 0, huber=0.02, tol=1e-9, max_iters=40)
    diff = ref.difference(got, want)
    print(f"\nhuber 0.02, kind {kind}: translation error {err(plain):.2e} without, {err(want):.2e} with (reference), {err(got):.2e} (device); "
          f"device - reference {diff:.3e}, spread {spread:.3e}, tolerance {tolerance:.3e}")
    assert got['status'] == ref.CONVERGED and got['iterations'] == want['iterations'] and np.array_equal(got['index'], want['index']) and diff <= tolerance
    unweighted = _raw(a, bn if kind == 1 else an, b, kind, 0, tol=1e-9, max_iters=40)
    assert err(got) < 0.2 * err(unweighted)


# ---- stops --------------------------------------------------------------------------------------------------------------------------------
def test_a_flat_lattice_is_degenerate_for_point_to_plane():
    """Normals (0, 0, 1) on every row: the columns of the rotation about z and of the translations along x and y are exact zeros, the
    third pivot is exactly 0.  DEGENERATE, and the transform is bitwise the start."""
    a, an, b, bn = ref.case_lattice()
    got = _raw(a, bn, b, 1, 0, start=ref.START, max_iters=4)
    start = np.concatenate([ref.START['R'].reshape(9), ref.START['t'], [ref.START['s']]])
    assert got['status'] == ref.DEGENERATE and got['iterations'] == 1 and got['n'] == len(a) and got['state'][:13].tobytes() == start.tobytes()
    H = ref.full(got['H'])
    assert not H[2].any() and not H[3].any() and not H[4].any() and H[0, 0] > 0 and H[1, 1] > 0 and H[5, 5] > 0
    assert not got['delta'].any() and got['step'] == 0.0 and got['cost'] > 0
    np.testing.assert_array_equal(got['history'][:, 3], [ref.DEGENERATE] * 4)
    assert got['history'][0, 0] == len(a) and got['history'][0, 1] == got['cost'] and not got['history'][1:, :3].any()
    assert ref.run(a, an, b, bn, 1, False, max_iters=4, **ref.START)['status'] == ref.DEGENERATE
    pinned = _raw(a, None, b, 0, 0, tol=1e-9, max_iters=30)                                # point to point pins the lattice
    assert pinned['status'] == ref.CONVERGED and np.abs(pinned['t'] + np.array([0.013, 0.007, 0.01])).max() < 1e-6


def test_queries_beyond_the_radius_are_too_few():
    a, an, b, bn = ref.case_identical()
    got = _raw(a + np.float32(1.0), None, b, 0, 1, start=ref.START, max_iters=3)
    assert got['status'] == ref.FEW and got['n'] == 0 and (got['index'] == -1).all() and got['iterations'] == 1
    assert got['state'][:13].tobytes() == np.concatenate([ref.START['R'].reshape(9), ref.START['t'], [ref.START['s']]]).tobytes()
    assert not got['H'].any() and not got['g'].any() and got['cost'] == 0.0
    np.testing.assert_array_equal(got['history'], [[0, 0, 0, ref.FEW]] * 3)


def test_iterations_after_the_stop_change_nothing():
    """max_iters 40 and 60: the same bits in rot, trans and s; the rows of the history past the stop are {0, 0, 0, status}; a run that
    is cut short says MAX_ITERS."""
    a, an, b, bn = ref.case_identical()
    short, long = (_raw(a, bn, b, 1, 1, tol=1e-10, max_iters=k) for k in (40, 60))
    it = short['iterations']
    assert short['status'] == long['status'] == ref.CONVERGED and it == long['iterations'] < 10
    assert short['state'][:59].tobytes() == long['state'][:59].tobytes() and short['index'].tobytes() == long['index'].tobytes()
    assert short['history'].tobytes() == long['history'][:40].tobytes()
    np.testing.assert_array_equal(long['history'][it:], [[0, 0, 0, ref.CONVERGED]] * (60 - it))
    cut = _raw(a, bn, b, 1, 1, tol=1e-10, max_iters=it - 1)
    assert cut['status'] == ref.MAX_ITERS and cut['iterations'] == it - 1
    np.testing.assert_array_equal(cut['history'][:, :3], short['history'][:it - 1, :3])
    np.testing.assert_array_equal(cut['history'][:, 3], [ref.RUNNING] * (it - 2) + [ref.MAX_ITERS])


# ---- repeatability ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_permutations():
    """Two runs: the same bits in state, history and index.  The reference rows permuted (their normals with them): the state bitwise
    the same, index renamed through the permutation.  The query rows permuted: the sums within the summation bound only."""
    a, an, b, bn = ref.case_one_iteration()
    first, again = (_raw(a, bn, b, 1, 1, start=ref.START, tol=1e-9, max_iters=12) for _ in range(2))
    assert first['status'] == ref.CONVERGED and _bits(first) == _bits(again)
    perm = np.random.default_rng(77).permutation(len(b))
    moved = _raw(a, bn[perm], b[perm], 1, 1, start=ref.START, tol=1e-9, max_iters=12)
    assert moved['state'][:59].tobytes() == first['state'][:59].tobytes() and moved['history'].tobytes() == first['history'].tobytes()
    found = first['index'] >= 0
    assert np.array_equal(moved['index'] >= 0, found) and np.array_equal(perm[moved['index'][found]], first['index'][found])
    assert not np.array_equal(moved['index'], first['index'])
    order = np.random.default_rng(78).permutation(len(a))
    _one_iteration(a, an, b, bn, 2, 1, "queries permuted", order=order)


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------
def test_register_clouds_equals_the_raw_call():
    from super_primitive_amd import _lib
    from super_primitive_amd.tool import viz
    a, an, b, bn = ref.case_independent()
    grid = viz.cloud_grid(T(b), ref.RADIUS)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = ref.START['R'], ref.START['t']
    for residual, kind, normals in (('point', 0, None), ('plane', 1, bn), ('query_plane', 2, an)):
        raw = _raw(a, normals, b, kind, 1, start=ref.START, huber=0.05, tol=1e-8, max_iters=9)
        out = viz.register_clouds(T(a), grid, normals=None if normals is None else T(normals), residual=residual, T0=T0, s0=ref.START['s'], scale=True,
                                  huber=0.05, tol=1e-8, max_iters=9)
        assert set(out) == {'rot', 'trans', 's', 'T', 'status', 'iterations', 'n', 'cost', 'history', 'index'}
        assert all(torch.is_tensor(v) and v.is_cuda for v in out.values())
        assert out['rot'].dtype == out['T'].dtype == out['history'].dtype == torch.float64 and tuple(out['T'].shape) == (4, 4)
        assert out['status'].dtype == out['iterations'].dtype == out['index'].dtype == torch.int32 and out['n'].dtype == torch.int64
        assert npy(out['rot']).tobytes() == raw['R'].tobytes() and npy(out['trans']).tobytes() == raw['t'].tobytes() and float(out['s']) == raw['s']
        assert npy(out['history']).tobytes() == raw['history'].tobytes() and npy(out['index']).tobytes() == raw['index'].tobytes()
        assert (int(out['status']), int(out['iterations']), int(out['n']), float(out['cost'])) == (raw['status'], raw['iterations'], raw['n'], raw['cost'])
        want_T = np.eye(4)
        want_T[:3, :3], want_T[:3, 3] = raw['s'] * raw['R'], raw['t']
        np.testing.assert_array_equal(npy(out['T']), want_T)
    default = viz.register_clouds(T(a), grid, max_iters=3)                                 # the identity, rigid, point to point
    plain = _raw(a, None, b, 0, 0, tol=1e-6, max_iters=3)
    assert npy(default['rot']).tobytes() == plain['R'].tobytes() and int(default['status']) == plain['status'] == _lib.SP_CLOUD_REG_MAX_ITERS
    with pytest.raises(ValueError, match="scratch"):
        viz.register_clouds(T(a), dict(grid, scratch=grid['scratch'][:-1]))
    with pytest.raises(ValueError, match="grid"):
        viz.register_clouds(T(a), dict(grid, Q=len(b) - 1))
    with pytest.raises(ValueError, match="needs normals"):
        viz.register_clouds(T(a), grid, residual='plane')
    with pytest.raises(ValueError, match="grid point"):
        viz.register_clouds(T(a), grid, normals=T(an), residual='plane')


def _bumpy_keyframe(H, W, K, seed):
    """A keyframe over a non-flat log-depth table (four segments, the quadrants), with a random image."""
    from super_primitive_amd.image.keyframe import KeyFrame
    rng = np.random.default_rng(seed)
    masks = np.zeros((4, H, W), dtype=bool)
    masks[0, :H // 2, :W // 2] = masks[1, :H // 2, W // 2:] = masks[2, H // 2:, :W // 2] = masks[3, H // 2:, W // 2:] = True
    rr, cc = np.mgrid[0:H, 0:W]
    z = ref.height(2.0 * cc / (W - 1) - 1.0, 2.0 * rr / (H - 1) - 1.0)[0]
    L = (np.log(z)[None] * masks).astype(np.float32)
    keypoints = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, -0.5], [0.5, 0.5]], dtype=np.float32)
    image = rng.uniform(0.0, 1.0, (3, H, W)).astype(np.float32)
    return KeyFrame(T(image), T(K), T(L), T(keypoints), T(masks)), T(np.full(4, np.log(2.0), dtype=np.float32))


def test_register_map_end_to_end():
    """A 48 x 64 keyframe over a non-flat log-depth table through ``keyframe_points(..., normals=True)``, against ``depth_image_lift`` of
    the keyframe's own depth image from a pose 0.03 / 1 degree away: the same surface, moved.  ``register_map`` (plane to point: the map
    has the normals, the lifted cloud has none) recovers that pose to the reference's value, the accuracy of ``map_distance`` falls, and
    ``world`` is left untouched."""
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    H, W = 48, 64
    K = np.array([[60.0, 0, 31.5], [0, 60.0, 23.5], [0, 0, 1]], dtype=np.float32)
    kf, kld = _bumpy_keyframe(H, W, K, 3)
    world = results.keyframe_points([kf], [kld], T(np.eye(4, dtype=np.float32)[None]), stride=1, normals=True)
    world['ids'] = [0]
    depth = viz.keyframe_depths([kf], [kld])['depth'][0]
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = ref.rodrigues(np.deg2rad(1.0) * np.array([0.6, -0.64, 0.48])), (0.02, -0.01, 0.02)
    reference = viz.depth_image_lift(depth, T(K), T=T(pose.astype(np.float32)))
    assert world['points'].shape[0] == H * W == reference['points'].shape[0] and float(world['normals'].abs().sum(dim=1).gt(0).float().mean()) > 0.5
    before = {k: (v.clone() if torch.is_tensor(v) else np.array(v)) for k, v in world.items()}
    radius = 0.1
    score0 = results.map_distance(world, reference, radius)['metrics']
    out = results.register_map(world, reference, radius, tol=1e-9, max_iters=30)
    assert set(out) == {'transform', 'world'} and int(out['transform']['status']) == ref.CONVERGED
    score1 = results.map_distance(out['world'], reference, radius)['metrics']
    p, n, q = npy(world['points']), npy(world['normals']), npy(reference['points'])
    want = ref.check_gap(ref.run(p, n, q, None, 2, False, tol=1e-9, max_iters=30, radius=radius))
    back = ref.run(p, n, q, None, 2, False, tol=1e-9, max_iters=30, radius=radius, reverse=True)
    tolerance, spread = _tolerance(want, back)
    got = dict(R=npy(out['transform']['rot']), t=npy(out['transform']['trans']), s=float(out['transform']['s']))
    diff = ref.difference(got, want)
    truth = np.float32(pose).astype(np.float64)
    print(f"\nend to end: accuracy {float(score0['accuracy']):.5f} -> {float(score1['accuracy']):.2e}; device - reference {diff:.3e} (tolerance {tolerance:.3e}, "
          f"spread {spread:.3e}); |t - truth| {np.abs(got['t'] - truth[:3, 3]).max():.2e}, {int(out['transform']['iterations'])} iterations")
    assert want['status'] == ref.CONVERGED and diff <= tolerance and got['s'] == 1.0
    assert np.abs(got['t'] - truth[:3, 3]).max() < 1e-5 and ref.rotation_angle(got['R'], truth[:3, :3]) < 1e-5
    assert float(score1['accuracy']) < float(score0['accuracy']) and float(score1['accuracy']) < 1e-5
    moved = results.transform_map(world, out['transform']['rot'], out['transform']['trans'], out['transform']['s'])
    assert torch.equal(moved['points'], out['world']['points']) and torch.equal(moved['normals'], out['world']['normals'])
    assert npy(out['world']['points']).tobytes() == ref.move(p, got['R'], got['t'], got['s']).astype(np.float32).tobytes()
    assert set(world) == set(before)                                           # the input is left as it was
    for k, v in before.items():
        assert torch.equal(world[k], v) if torch.is_tensor(v) else np.array_equal(np.asarray(world[k]), v), k
    # a bare tensor as the reference and a residual by name: the call that register_clouds makes on a grid of its own, to the bit
    by_point = results.register_map(world, reference['points'], radius, residual='point', tol=1e-9, max_iters=20)
    direct = viz.register_clouds(world['points'], viz.cloud_grid(reference['points'], radius), residual='point', tol=1e-9, max_iters=20)
    for key in ('rot', 'trans', 's', 'history', 'index'):
        assert torch.equal(by_point['transform'][key], direct[key]), key
    assert torch.equal(by_point['world']['normals'], results.transform_map(world, direct['rot'], direct['trans'])['normals'])
    with pytest.raises(ValueError, match="normals of the reference"):
        results.register_map(world, reference, radius, residual='plane')
    with pytest.raises(ValueError, match="grid"):
        viz.register_clouds(world['points'], dict(scratch=reference['points'], Q=3), normals=world['normals'], residual='query_plane')
