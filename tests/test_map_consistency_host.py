"""CPU-only: the ABI of the map consistency entry points (include/sp_hip.h: sp_keyframe_depths, sp_map_consistency), their argument
checks -- made before any device work, so they answer without a GPU --, the argument checks of the Python surface (``tool/viz.py``
``keyframe_depths`` / ``map_consistency``, ``odometery/results.py`` ``map_consistency``) and the two torch-only helpers
``segment_consistency`` / ``filter_map`` on CPU tensors against NumPy."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for name in ("sp_keyframe_depths", "sp_map_consistency"):
        assert name in _lib.SIGNATURES, name
    for phrase in ("behind every surface, or between surfaces", "HIGHEST table index", "WRITTEN FOR EVERY ROW"):
        assert phrase in header, phrase                                      # the rules are part of the contract


def test_keyframe_depths_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(kfs=p, n_kf=2, total_blocks=3, H=4, W=4, keys=p, depth=p, seg=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_keyframe_depths(a['kfs'], a['n_kf'], a['total_blocks'], a['H'], a['W'], a['keys'], a['depth'], a['seg'], None)
    for bad in (dict(kfs=None), dict(keys=None), dict(depth=None), dict(n_kf=0), dict(n_kf=-1), dict(n_kf=65536), dict(total_blocks=0),
                dict(H=0), dict(W=0), dict(H=-2), dict(W=-1)):
        assert call(**bad) == -1, bad
    for big in (dict(H=1 << 16, W=1 << 15), dict(n_kf=2, H=1 << 15, W=1 << 15), dict(n_kf=65535, H=1 << 10, W=1 << 10)):
        assert call(**big) == -2, big
        assert call(seg=None, **big) == -2, big                    # (a null seg is allowed: it does not turn into SP_EINVAL)
    assert call(n_kf=2, H=1 << 15, W=1 << 15, keys=None) == -1     # invalid beats too large


def test_map_consistency_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(points=p, owner=p, Q=10, views=p, view_owner=p, V=1, depth=p, H=4, W=4, tol=0.05, window=1, z_min=1e-6, counts=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_map_consistency(a['points'], a['owner'], a['Q'], a['views'], a['view_owner'], a['V'], a['depth'], a['H'], a['W'], a['tol'],
                                      a['window'], a['z_min'], a['counts'], None)
    nan = float("nan")
    for bad in (dict(points=None), dict(views=None), dict(depth=None), dict(counts=None), dict(Q=0), dict(Q=-1), dict(V=0), dict(V=-5),
                dict(H=0), dict(W=-3), dict(tol=-0.01), dict(tol=nan), dict(tol=1.0), dict(tol=7.5), dict(window=-1), dict(window=3),
                dict(window=1 << 20), dict(z_min=-1.0), dict(z_min=nan)):
        assert call(**bad) == -1, bad
    for big in (dict(Q=2 ** 31 - 1), dict(Q=2 ** 40), dict(V=65536), dict(H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15),
                dict(V=65535, H=1 << 10, W=1 << 10)):
        assert call(**big) == -2, big
        assert call(owner=None, view_owner=None, **big) == -2, big  # (null owners are allowed)
    for both in (dict(Q=2 ** 40, counts=None), dict(V=65536, tol=1.0), dict(Q=2 ** 31 - 1, window=3), dict(V=2, H=1 << 15, W=1 << 15, z_min=nan)):
        assert call(**both) == -1, both                            # invalid beats too large: nothing is launched either way


def test_the_defaults_of_the_python_surface():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    sig = inspect.signature(viz.map_consistency).parameters
    assert list(sig) == ['points', 'Ks', 'poses', 'depths', 'owner', 'view_owner', 'tol', 'window', 'z_min']
    assert (sig['owner'].default, sig['view_owner'].default, sig['tol'].default, sig['window'].default, sig['z_min'].default) == (None, None, 0.05, 1, 1e-6)
    assert list(inspect.signature(viz.keyframe_depths).parameters) == ['kfs', 'klds']
    sig = inspect.signature(results.map_consistency).parameters
    assert list(sig) == ['world', 'depths', 'Ks', 'poses', 'view_kf', 'tol', 'window'] and sig['view_kf'].default is None
    for fn in (results.map_consistency, results.sequence_consistency):
        sig = inspect.signature(fn).parameters
        assert sig['tol'].default == 0.05 and sig['window'].default == 1, fn.__name__
    assert list(inspect.signature(results.sequence_consistency).parameters) == ['world', 'result', 'tol', 'window']
    assert inspect.signature(results.segment_consistency).parameters['n_segments'].default is None
    sig = inspect.signature(results.filter_map).parameters
    assert sig['min_agree'].default == 1 and sig['max_in_front'].default is None


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


class _Kf:
    """What ``table_of`` would see; the fake below hands the table out directly."""
    def __init__(self, H, W, N=3, P=10):
        self.tab = type("Tab", (), dict(H=H, W=W, N=N, P=P))()


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib, segment_table
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.map_consistency(torch.zeros(5, 3), torch.eye(3), torch.eye(4)[None], torch.ones(1, 4, 6))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts, K, eye, d = _meta(5, 3), _meta(3, 3), _meta(2, 4, 4), _meta(2, 4, 6)
    ok = dict(points=pts, Ks=K, poses=eye, depths=d, owner=_meta(5, dtype=torch.int32), view_owner=_meta(2, dtype=torch.int32))
    for kw in (dict(points=_meta(5, 4)), dict(points=_meta(5, 3, dtype=torch.float64)), dict(points=_meta(0, 3)), dict(poses=_meta(4, 4)),
               dict(poses=_meta(3, 4, 4)), dict(Ks=_meta(3, 3, 3)), dict(depths=_meta(3, 4, 6)), dict(depths=_meta(2, 4)),
               dict(depths=_meta(2, 4, 6, dtype=torch.float64)), dict(depths=_meta(2, 0, 6)), dict(owner=_meta(4, dtype=torch.int32)),
               dict(owner=_meta(5, dtype=torch.int64)), dict(view_owner=_meta(3, dtype=torch.int32)), dict(view_owner=_meta(2)),
               dict(owner=[0] * 5), dict(tol=-0.1), dict(tol=1.0), dict(tol=float("nan")), dict(window=-1), dict(window=3), dict(window=1.5),
               dict(z_min=-1.0), dict(z_min=float("nan"))):
        with pytest.raises(ValueError):
            viz.map_consistency(**dict(ok, **kw))
    with pytest.raises(ValueError, match="limits"):
        viz.map_consistency(pts, K, eye, _meta(2, 1 << 15, 1 << 15))
    world = dict(points=pts, kf_index=_meta(5, dtype=torch.int32))
    for depths in (_meta(3, 4, 6), _meta(2, 4, 6, dtype=torch.float16), _meta(4, 6), [[1.0]]):
        with pytest.raises(ValueError, match="depths"):
            results.map_consistency(world, depths, K, eye)
    for view_kf in ([0], [0, 1, 2], torch.zeros(2), [[0, 1]]):
        with pytest.raises(ValueError, match="view_kf"):
            results.map_consistency(world, d, K, eye, view_kf=view_kf)
    with pytest.raises(ValueError):
        results.map_consistency(world, d, K, _meta(4, 4))
    with pytest.raises(ValueError):
        results.map_consistency(world, d, K, eye, tol=2.0)
    with pytest.raises(ValueError, match="keep_keyframes"):
        results.sequence_consistency(dict(world, ids=[0, 4]), dict(kf_archive={0: dict(kf=None), 4: dict(kf=None)}))
    # keyframe_depths: keyframes of differing sizes, counts that do not match, a keyframe without segment pixels
    monkeypatch.setattr(segment_table, "table_of", lambda kf: kf.tab)
    kld = _meta(3)
    with pytest.raises(ValueError, match="differing|is 5x8"):
        viz.keyframe_depths([_Kf(6, 8), _Kf(5, 8)], [kld, kld])
    with pytest.raises(ValueError, match="log-depths"):
        viz.keyframe_depths([_Kf(6, 8), _Kf(6, 8)], [kld, _meta(4)])
    with pytest.raises(ValueError):
        viz.keyframe_depths([_Kf(6, 8)], [kld, kld])
    with pytest.raises(ValueError):
        viz.keyframe_depths([], [])

    def no_pixels(kf):
        raise ValueError("keyframe has no segment pixels")
    monkeypatch.setattr(segment_table, "table_of", no_pixels)
    with pytest.raises(ValueError, match="no segment pixels"):
        viz.keyframe_depths([_Kf(6, 8)], [kld])


def _world(rng, sizes, n_seg):
    Q = int(sum(sizes))
    kf = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    seg = np.concatenate([np.sort(rng.integers(0, n_seg, s)) for s in sizes]).astype(np.int32)
    counts = rng.integers(0, 3, (Q, 3)).astype(np.int32)
    counts[rng.uniform(size=Q) < 0.3] = 0
    world = dict(points=torch.from_numpy(rng.standard_normal((Q, 3)).astype(np.float32)), colours=torch.from_numpy(rng.uniform(size=(Q, 3)).astype(np.float32)),
                 kf_index=torch.from_numpy(kf), seg_ids=torch.from_numpy(seg), offsets=np.concatenate(([0], np.cumsum(sizes))).astype(np.int64),
                 ids=[3 * k for k in range(len(sizes))], align=dict(s=torch.tensor([1.5])), ate=torch.tensor(0.25))
    return world, kf, seg, counts


def test_segment_consistency_on_cpu_tensors_against_numpy():
    from super_primitive_amd.odometery.results import segment_consistency
    rng = np.random.default_rng(401)
    world, kf, seg, counts = _world(rng, [700, 1, 350, 0, 64], 7)
    want = np.zeros((5, 9, 5), np.int64)
    for i in range(len(kf)):                                                 # an explicit loop over the points
        a, f, b = counts[i]
        want[kf[i], seg[i]] += (1, a + f + b > 0, a >= 1, f >= 1 and a == 0, a)
    cons = dict(counts=torch.from_numpy(counts))
    got = segment_consistency(world, cons, n_segments=9)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, 9, 5)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(segment_consistency(world, cons).numpy(), want[:, :int(seg.max()) + 1])     # N_max read from the ids
    assert want[:, :, 3].sum() > 20 and want[3].sum() == 0 and want[:, 7:].sum() == 0
    few = segment_consistency(world, cons, n_segments=4).numpy()            # ids beyond N_max are counted nowhere
    np.testing.assert_array_equal(few, want[:, :4])
    with pytest.raises(ValueError):
        segment_consistency(world, dict(counts=torch.from_numpy(counts[:-1])))
    with pytest.raises(ValueError):
        segment_consistency(world, cons, n_segments=0)


@pytest.mark.parametrize("min_agree,max_in_front", [(1, None), (2, None), (1, 0), (0, 1), (3, None)])
def test_filter_map_on_cpu_tensors_against_numpy(min_agree, max_in_front):
    from super_primitive_amd.odometery.results import filter_map
    rng = np.random.default_rng(402)
    sizes = [300, 0, 5, 411]
    world, kf, seg, counts = _world(rng, sizes, 5)
    keep = counts[:, 0] >= min_agree
    if max_in_front is not None:
        keep &= counts[:, 1] <= max_in_front
    rows = np.nonzero(keep)[0]
    out = filter_map(world, dict(counts=torch.from_numpy(counts)), min_agree=min_agree, max_in_front=max_in_front)
    assert out['kept'].dtype == torch.int64
    np.testing.assert_array_equal(out['kept'].numpy(), rows)
    for key in ('points', 'colours', 'kf_index', 'seg_ids'):
        np.testing.assert_array_equal(out[key].numpy(), world[key].numpy()[rows], err_msg=key)
        assert out[key].dtype == world[key].dtype
    want_offsets = np.concatenate(([0], np.cumsum(np.bincount(kf[rows], minlength=len(sizes)))))
    assert isinstance(out['offsets'], np.ndarray) and out['offsets'].dtype == np.int64
    np.testing.assert_array_equal(out['offsets'], want_offsets)
    assert out['ids'] == world['ids'] and out['align'] is world['align'] and out['ate'] is world['ate']
    assert world['points'].shape[0] == sum(sizes) and 'kept' not in world      # the input is left as it was
    if min_agree == 3:                                                       # an incomplete world is an argument error
        cons = dict(counts=torch.from_numpy(counts))
        for broken in ({k: v for k, v in world.items() if k != 'colours'}, dict(world, seg_ids=None), dict(world, kf_index=kf.tolist()),
                       dict(world, colours=world['colours'][:-1]), dict(world, offsets=world['offsets'][:-1]), {k: v for k, v in world.items() if k != 'offsets'}):
            with pytest.raises(ValueError, match='filter_map'):
                filter_map(broken, cons)

        assert len(rows) == 0 and out['points'].shape == (0, 3)
    else:
        assert 0 < len(rows) < len(keep)
