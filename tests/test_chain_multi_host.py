"""CPU-only: the lockstep form of the odometry chain (``sp_chain_step_multi``, ``odometery.sequence_batch``) -- the symbol, the ABI, and
the argument checks that refuse a call before anything reaches a device."""
import ctypes

import pytest

SP_EINVAL = -1                                      # (include/sp_hip.h)


def _lib():
    from super_primitive_amd import _lib as L
    return L, L.load()


def _records(n, stages):
    L, _ = _lib()
    arr = (L.SpChainStep * n)()
    for k in range(n):
        st = arr[k]
        st.stages, st.H, st.W, st.n_levels = stages, 64, 96, 2
        for w in (st.track, st.supp):
            w.gn[0].pairs = 0x1000               # (never dereferenced: the checks fail first)
            w.n_phases, w.check_every = 1, 4
            w.phase[0].level, w.phase[0].max_iters, w.phase[0].irls_eps, w.phase[0].conv_tol = 0, 8, 1e-3, 1e-3
            w.lam0, w.lm_up, w.lm_down, w.lm_min = 1e-4, 8.0, 0.5, 1e-7
    return arr


def _call(arr, n):
    _, lib = _lib()
    fake = ctypes.c_void_p(0x2000)
    return lib.sp_chain_step_multi(arr, n, fake, fake, fake, None)


def test_multi_symbol_and_abi():
    L, lib = _lib()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "sp_chain_step_multi")
    assert not hasattr(ctypes.CDLL(L.LIB_PATH), "sp_chain_step")             # (since ABI 17: one sequence is the multi call at n_steps = 1)
    assert lib.sp_chain_multi_bytes() > 0


def test_multi_refuses_empty_and_null():
    L, lib = _lib()
    arr = _records(2, L.SP_CHAIN_TRACK)
    assert _call(arr, 0) == SP_EINVAL
    assert _call(arr, 65536) == SP_EINVAL
    assert lib.sp_chain_step_multi(None, 1, ctypes.c_void_p(0x2000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x2000), None) == SP_EINVAL
    assert lib.sp_chain_step_multi(arr, 2, None, ctypes.c_void_p(0x2000), ctypes.c_void_p(0x2000), None) == SP_EINVAL


def test_multi_refuses_mixed_stages_and_sizes():
    L, _ = _lib()
    arr = _records(3, L.SP_CHAIN_TRACK | L.SP_CHAIN_SUPP)
    arr[2].stages = L.SP_CHAIN_TRACK
    assert _call(arr, 3) == SP_EINVAL
    arr = _records(2, L.SP_CHAIN_TRACK)
    arr[1].W = 95
    assert _call(arr, 2) == SP_EINVAL
    arr = _records(2, L.SP_CHAIN_TRACK)
    arr[1].n_levels = 3
    assert _call(arr, 2) == SP_EINVAL


@pytest.mark.parametrize("field", ["level", "max_iters", "irls_eps", "conv_tol", "n_phases", "check_every", "check_first", "flags", "lm_up"])
def test_multi_refuses_mismatched_schedules(field):
    L, _ = _lib()
    for stage, win in ((L.SP_CHAIN_TRACK, "track"), (L.SP_CHAIN_SUPP, "supp")):
        arr = _records(2, stage)
        w = getattr(arr[1], win)
        if field in ("level", "max_iters", "irls_eps", "conv_tol"):
            setattr(w.phase[0], field, {"level": 1, "max_iters": 9, "irls_eps": 2e-3, "conv_tol": 2e-3}[field])
        else:
            setattr(w, field, {"n_phases": 2, "check_every": 5, "check_first": 1, "flags": 2, "lm_up": 4.0}[field])
        assert _call(arr, 2) == SP_EINVAL, (field, win)


def test_run_sequences_refuses_other_engines():
    from super_primitive_amd.odometery.sequence_batch import run_sequences
    with pytest.raises(ValueError):
        run_sequences([dict(frames=[], to_keyframe=None, pose0=None, kld0=None)], engine="adam")
    with pytest.raises(ValueError):
        run_sequences([dict(frames=[], to_keyframe=None, pose0=None, kld0=None)], native_step=False)
    with pytest.raises(ValueError):
        run_sequences([dict(frames=[], to_keyframe=None, pose0=None, kld0=None)], motion_prior=True)
