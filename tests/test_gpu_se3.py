"""-m gpu: se3_exp_times and renormalise_rotation (csrc/sp_solve_device.h) on every branch, through sp_se3_retract (k_se3_retract, forward
on Dual<1>, backward on Dual<6>) and sp_renormalise_se3 (k_renormalise), against tests/se3_ref.py.

The truth (scipy's expm, its derivative by the complex step), the magnitude companion, the counts OPS_* and the edge tables are se3_ref's;
tests/test_se3_ref_host.py holds them against mpmath and proves that a correct float32 evaluation meets every bound used here and that each
error planted there leaves one.  Bounds (counted in se3_ref's docstring, not tuned):

  forward    |T - Exp(a) X| <= OPS_ROT | OPS_TRANS (12 | 13) * 2^-24 * magnitude, entry by entry; a = 0 returns X bit for bit; the last row
             is 0 0 0 1 bit for bit
  backward   G one-hot on each of the 12 entries (one Jacobian column alone) and one random G: |ga - truth| <= sum over the entries of
             (OPS_D_ROT | OPS_D_TRANS (14 | 16) + non-zero G entries) * 2^-24 * magnitude * |G|
  batches    n = 1, 63, 64, 65, 130 (blocks of 64: a partial one, a full one, a second one), sentinels behind the n-th output, the other
             mode's buffer NULL, element b of 130 bitwise the batch of 1 on the same input
  renormalise  every rotation of se3_ref.rotation_table() (each quaternion candidate clean and noisy, two exact ties) cycled over the same n:
             rotation within RENORM_OPS ulp at max(|entry|, 1) of window_gn_step_ref.renormalise_rotation, translation column and last row
             untouched, sentinels, and a second application moves nothing beyond the same bound
The worst ratio to each bound is printed at the end of the file.
"""
import time

import numpy as np
import pytest
import torch

import se3_ref as s
from se3_ref import f32
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

SENTINEL = -5.0
TAIL = 7
BATCHES = [1, 63, 64, 65, 130]
WORST = {}
T0 = time.perf_counter()
NAMES, TWISTS = s.edge_twists()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"\nworst ratio to each bound over the file ({time.perf_counter() - T0:.1f} s): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


@pytest.fixture(scope="module")
def truth():
    """Per pose of se3_ref.POSES: (want (n, 4, 4), Jacobian (n, 6, 4, 4), mag, dmag) on the edge twists -- computed once, never written."""
    out = []
    for _, X in s.POSES:
        mag, dmag = s.magnitudes(TWISTS, X)
        out.append((s.retract(TWISTS, X), s.retract_jacobian(TWISTS, X), mag, dmag))
    return out


def retract(a, X, G=None):
    """One sp_se3_retract launch on a (n, 6), X (n, 4, 4) [, G (n, 4, 4)]: forward T (n, 4, 4) or backward ga (n, 6); the buffer of the other
    mode is NULL and the output's sentinel tail is checked."""
    from super_primitive_amd import _lib
    lib, n = _lib.load(), len(a)
    a_d, X_d = T(np.array(a, f32)), T(np.array(np.broadcast_to(X, (n, 4, 4)), f32))
    width = 16 if G is None else 6
    out = T(np.full(n * width + TAIL, SENTINEL, f32))
    if G is None:
        rc = lib.sp_se3_retract(_lib.ptr(a_d), _lib.ptr(X_d), n, _lib.ptr(out), None, None, _lib.stream_ptr())
    else:
        G_d = T(np.array(np.broadcast_to(G, (n, 4, 4)), f32))
        rc = lib.sp_se3_retract(_lib.ptr(a_d), _lib.ptr(X_d), n, None, _lib.ptr(G_d), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "sp_se3_retract")
    torch.cuda.synchronize()
    got = npy(out)
    assert (got[n * width:] == SENTINEL).all(), "a write behind the n-th output"
    assert bits(npy(a_d)) == bits(np.ascontiguousarray(a, f32)), "the twists were written"
    return got[:n * width].reshape((n, 4, 4) if G is None else (n, 6))


def worst_case(r):
    return NAMES[int(r.reshape(len(r), -1).max(1).argmax())]


@pytest.mark.parametrize("pose", [0, 1], ids=[p[0] for p in s.POSES])
def test_forward_on_every_edge_twist(pose, truth):
    X = s.POSES[pose][1]
    want, _, mag, _ = truth[pose]
    got = retract(TWISTS, X)
    assert bits(got[:, 3]) == bits(np.tile(np.array([0, 0, 0, 1], f32), (len(got), 1))), "last row"
    r = np.abs(got[:, :3].astype(np.float64) - want[:, :3]) / s.value_bound(mag)
    note(f"forward, X {s.POSES[pose][0]}", r.max())
    assert r.max() <= 1, f"T is {r.max():.3g} of its bound at {worst_case(r)}"
    zero = ~TWISTS.any(1)
    assert zero.sum() == 3 and all(bits(g) == bits(X) for g in got[zero]), "a = 0 must return X bit for bit"
    assert not got[:, :3][mag == 0].any(), "an entry whose expression has no non-zero term"


@pytest.mark.parametrize("pose", [0, 1], ids=[p[0] for p in s.POSES])
def test_backward_on_every_edge_twist(pose, truth):
    X = s.POSES[pose][1]
    _, J, _, dmag = truth[pose]
    for i in range(3):
        for j in range(4):          # one column of the Jacobian alone
            G = np.zeros((4, 4), f32)
            G[i, j] = 1
            r = np.abs(retract(TWISTS, X, G).astype(np.float64) - J[:, :, i, j]) / s.grad_bound(dmag, G)
            note(f"backward one-hot, X {s.POSES[pose][0]}", r.max())
            assert r.max() <= 1, f"d T[{i},{j}] / d a is {r.max():.3g} of its bound at {worst_case(r)}, component {int(r.max(0).argmax())}"
    G = np.random.default_rng(8).standard_normal((4, 4)).astype(f32)          # the last row must not be read into the result
    r = np.abs(retract(TWISTS, X, G).astype(np.float64) - s.retract_grad(TWISTS, X, G)) / s.grad_bound(dmag, G)
    note(f"backward random G, X {s.POSES[pose][0]}", r.max())
    assert r.max() <= 1, f"ga is {r.max():.3g} of its bound at {worst_case(r)}"


def batch_inputs(n):
    """n twists cycled through the table from an offset that depends on n, the two poses by turns, a G per element."""
    idx = (np.arange(n) * 7 + n) % len(TWISTS)
    X = np.stack([s.POSES[k % 2][1] for k in range(n)])
    G = np.random.default_rng(n).standard_normal((n, 4, 4)).astype(f32)
    return TWISTS[idx], X, G


@pytest.mark.parametrize("n", BATCHES)
def test_batches(n):
    a, X, G = batch_inputs(n)
    fwd, bwd = retract(a, X), retract(a, X, G)
    mag, dmag = s.magnitudes(a, X)
    rv = np.abs(fwd[:, :3].astype(np.float64) - s.retract(a, X)[:, :3]) / s.value_bound(mag)
    rg = np.abs(bwd.astype(np.float64) - s.retract_grad(a, X, G)) / s.grad_bound(dmag, G)
    note("batches forward", rv.max())
    note("batches backward", rg.max())
    assert rv.max() <= 1 and rg.max() <= 1, (rv.max(), rg.max())
    assert bits(fwd[:, 3]) == bits(np.tile(np.array([0, 0, 0, 1], f32), (n, 1)))
    for b in sorted({0, n // 2, n - 1}):          # every element is computed alone: the batch of 1 on the same input, bit for bit
        assert bits(retract(a[b:b + 1], X[b:b + 1])[0]) == bits(fwd[b]), f"forward element {b} of {n}"
        assert bits(retract(a[b:b + 1], X[b:b + 1], G[b:b + 1])[0]) == bits(bwd[b]), f"backward element {b} of {n}"


def renormalise(M):
    from super_primitive_amd import _lib
    lib, n = _lib.load(), len(M)
    buf = T(np.concatenate([np.array(M, f32).ravel(), np.full(TAIL, SENTINEL, f32)]))
    _lib.check(lib.sp_renormalise_se3(_lib.ptr(buf), n, _lib.stream_ptr()), "sp_renormalise_se3")
    torch.cuda.synchronize()
    got = npy(buf)
    assert (got[16 * n:] == SENTINEL).all(), "a write behind matrix n"
    return got[:16 * n].reshape(n, 4, 4)


@pytest.mark.parametrize("n", BATCHES)
def test_renormalise(n):
    table = s.rotation_table()
    M = np.stack([table[(k + n) % len(table)][1] for k in range(n)])
    want = np.stack([s.renormalise_rotation(m.ravel()).reshape(4, 4) for m in M])
    got = renormalise(M)
    assert bits(got[:, :, 3]) == bits(M[:, :, 3]) and bits(got[:, 3]) == bits(M[:, 3]), "translation column or last row touched"
    u = s.renorm_ulps(got, want).reshape(n, -1).max(1)
    note("renormalise (of RENORM_OPS ulp)", u.max() / s.RENORM_OPS)
    assert u.max() <= s.RENORM_OPS, f"{table[(int(u.argmax()) + n) % len(table)][0]}: {u.max():.3g} ulp"
    again = renormalise(got)
    u2 = s.renorm_ulps(again, got).max()
    note("renormalise twice (of RENORM_OPS ulp)", u2 / s.RENORM_OPS)
    assert u2 <= s.RENORM_OPS and bits(again[:, :, 3]) == bits(M[:, :, 3]) and bits(again[:, 3]) == bits(M[:, 3])
