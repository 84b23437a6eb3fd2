"""-m gpu: ``sp_traj_align`` (csrc/sp_results.hip) -- S trajectories per launch, float64 -- against the float64 restatement of the
reference's ``align`` / ``transfer_scale`` (tests/traj_align_ref.py, itself pinned to the real reference by golden g26), and the
reference-named wrappers of ``tool/pose_utils.py``.

Tolerance (not a number fixed in advance): per case and field, 64 x the largest deviation of the restatement between 8 random orders of
the poses and the given order, at least 1e-13 -- the kernel decomposes by Jacobi rotations and sums in another order; both are
backward stable and scale with the condition number the permutation spread exposes.  Measured (MI355X): DESIGN.md section 4."""
import functools

import numpy as np
import pytest
import torch

import traj_align_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

LAUNCHES = {"generic": ["generic3", "generic65", "generic257", "generic1000"], "planar_mirrored": ["planar65", "mirrored65"]}
N_MAX = {"generic": 1000, "planar_mirrored": 80}


@functools.lru_cache(maxsize=None)
def _case(name):
    _, kind, n, seed = next(c for c in ref.CASES if c[0] == name)
    return ref.make_case(kind, n, seed)


@functools.lru_cache(maxsize=None)
def _reference(name, anchor):
    """(restatement, tolerance per field, spread per field) of a case; computed once and shared."""
    base, spread = ref.permutation_spread(*_case(name), anchor_rotation=anchor)
    return base, ref.tolerance(spread), spread


def _padded(names, n_max):
    pred = np.full((len(names), n_max, 4, 4), np.nan, dtype=np.float32)
    gt = np.full_like(pred, np.nan)
    lengths = []
    for k, name in enumerate(names):
        p, g = _case(name)
        pred[k, :len(p)], gt[k, :len(g)] = p, g
        lengths.append(len(p))
    return T(pred), T(gt), lengths


@pytest.mark.parametrize("anchor", [False, True], ids=["plain", "anchor_rotation"])
@pytest.mark.parametrize("launch", list(LAUNCHES))
def test_one_launch_aligns_trajectories_of_different_lengths(launch, anchor):
    from super_primitive_amd.tool import pose_utils
    names, n_max = LAUNCHES[launch], N_MAX[launch]
    pred, gt, lengths = _padded(names, n_max)
    out = pose_utils.align_trajectories(pred, gt, lengths, anchor_rotation=anchor)
    torch.cuda.synchronize()
    assert out['record'].shape == (len(names), 32) and out['record'].dtype == torch.float64
    assert bool(torch.isfinite(out['record']).all()), "NaN padding reached the record"
    for key in ('trans_scaled_error', 'trans_error'):
        assert bool(torch.isfinite(out[key]).all()), "NaN padding reached the per-pose errors"
    for k, name in enumerate(names):
        want, tol, spread = _reference(name, anchor)
        n, worst = lengths[k], {}
        for field in ref.FIELDS:
            got = npy(out[field][k])
            if field in ('trans_scaled_error', 'trans_error'):
                assert np.all(got[n:] == 0.0), (name, field)
                got = got[:n]
            dev = float(np.abs(got - want[field]).max())
            worst[field] = dev
        print(f"\n{name} ({'anchored' if anchor else 'plain'}): condition {ref.condition(*_case(name)):.3f}; per field (spread of the restatement over 8 orders / "
              f"kernel's deviation): " + ", ".join(f"{f} {spread[f]:.1e}/{worst[f]:.1e}" for f in ref.FIELDS))
        for field in ref.FIELDS:
            assert worst[field] <= tol[field], (name, field, worst[field], tol[field])
        if not anchor:
            np.testing.assert_array_equal(npy(out['rot_reanchor'][k]), np.eye(3))


def test_reference_named_functions():
    """``align``, ``transfer_scale`` and ``apply_scale`` with the reference's keys, as float64 device tensors."""
    from super_primitive_amd.tool import pose_utils
    name = "generic65"
    pred, gt = _case(name)
    want, tol, _ = _reference(name, True)
    a = pose_utils.align(T(pred[:, :3, 3].T.copy()), T(gt[:, :3, 3].T.copy()))
    ra = ref.align(pred[:, :3, 3].T, gt[:, :3, 3].T)
    composed = 16 * (tol['rot'] + tol['s'] + tol['trans_scaled'])
    assert np.abs(pred[:, :3, 3]).sum(1).max() <= 6 and ra['s'] <= 1.8
    assert set(a) == {'rot', 'trans_scaled', 'trans_scaled_error', 'trans', 'trans_error', 's', 'model_aligned_scaled', 'model_aligned'}
    for key in a:
        assert a[key].is_cuda and a[key].dtype == torch.float64 and tuple(a[key].shape) == np.shape(ra[key]), key
        # (the aligned models are s rot m + trans of fields each within its tolerance; |m|_1 <= 6 and s <= 1.8 in these cases, so
        #  their error is at most 11 tol_rot + 6 tol_s + tol_trans: `composed` below)
        bar = tol.get(key, composed)
        assert float(np.abs(npy(a[key]) - ra[key]).max()) <= bar, key
    for anchor in (False, True):
        est, pa = pose_utils.transfer_scale(T(gt), [T(p) for p in pred], anchor_rotation=anchor)
        rest, rpa = ref.transfer_scale(gt, pred, anchor_rotation=anchor)
        assert ('rot_reanchor' in pa) == anchor
        np.testing.assert_allclose(npy(est), np.stack(rest), rtol=0, atol=composed)
        got = pose_utils.apply_scale(T(pred[1]), pa)
        np.testing.assert_allclose(npy(got), ref.apply_scale(pred[1], rpa), rtol=0, atol=composed)
        if anchor:
            np.testing.assert_allclose(npy(pa['rot_reanchor']), want['rot_reanchor'], rtol=0, atol=tol['rot_reanchor'])


def test_short_trajectories_are_refused_on_the_host():
    from super_primitive_amd.tool import pose_utils
    pred, gt, _ = _padded(["generic3", "generic65"], 80)
    for lengths in ([2, 65], [3, 81], [3]):
        with pytest.raises(ValueError):
            pose_utils.align_trajectories(pred, gt, lengths)
    with pytest.raises(ValueError):
        pose_utils.align_trajectories(pred[:, :2], gt[:, :2])
