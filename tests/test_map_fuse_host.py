"""CPU-only: the ABI of the map fusion entry points (include/sp_hip.h: sp_map_fuse_scratch_units, sp_map_fuse), their argument checks
-- made before any device work, so they answer without a GPU --, the argument checks of the Python surface (``tool/viz.py``
``fuse_points``, ``odometery/results.py`` ``fuse_map``) and the torch-only helpers ``pool_map`` / ``write_ply`` on CPU tensors."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_Q = 1 << 28


def test_symbols_match_the_header_and_the_abi_version_stays():
    """(the types of every prototype, record and constant against the ctypes mirror, and the ABI number: tests/test_abi_mirror.py)"""
    from super_primitive_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp_hip.h")).read()
    for name in ("sp_map_fuse_scratch_units", "sp_map_fuse"):
        assert name in _lib.SIGNATURES, name
    for phrase in ("ascending order of i0", "WRITTEN FOR EVERY ROW", "before any conversion to an integer", "Invalid beats too large"):
        assert phrase in header, phrase                                      # the rules are part of the contract
    assert _lib.SP_MAP_FUSE_MAX_POINTS == MAX_Q == 1 << 28                    # the limit the header states


def test_scratch_units_and_their_error_codes():
    from super_primitive_amd import _lib
    lib = _lib.load()
    for bad in (0, -1, -2 ** 40):
        assert lib.sp_map_fuse_scratch_units(bad) == -1, bad
    for big in (MAX_Q + 1, 2 ** 31, 2 ** 40):
        assert lib.sp_map_fuse_scratch_units(big) == -2, big

    def want(Q):
        S = 2
        while S < 2 * Q:
            S *= 2
        return S + -(-Q // 16) + -(-(-(-Q // 256)) // 16)                    # slots of 64 bytes, Q int32, ceil(Q / 256) int32
    for Q in (1, 2, 3, 255, 256, 257, 4096, 4097, 5003, 70001, 1 << 26, MAX_Q):
        assert lib.sp_map_fuse_scratch_units(Q) == want(Q) > 2 * Q, Q


def test_map_fuse_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(points=p, colours=p, Q=10, voxel=0.25, ox=0.0, oy=0.0, oz=0.0, scratch=p, out_points=p, out_colours=p, count=p, first=p,
              label=p, n_fused=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_map_fuse(a['points'], a['colours'], a['Q'], a['voxel'], a['ox'], a['oy'], a['oz'], a['scratch'], a['out_points'],
                               a['out_colours'], a['count'], a['first'], a['label'], a['n_fused'], None)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(points=None), dict(scratch=None), dict(out_points=None), dict(count=None), dict(first=None), dict(label=None),
                dict(n_fused=None), dict(colours=None), dict(out_colours=None), dict(Q=0), dict(Q=-1), dict(voxel=0.0), dict(voxel=-0.25),
                dict(voxel=nan), dict(voxel=inf), dict(voxel=1e39), dict(ox=nan), dict(oy=inf), dict(oz=-inf), dict(ox=1e39)):
        assert call(**bad) == -1, bad                              # (1e39 is inf as a float32)
    for big in (dict(Q=MAX_Q + 1), dict(Q=2 ** 31), dict(Q=2 ** 40)):
        assert call(**big) == -2, big
        assert call(colours=None, out_colours=None, **big) == -2, big          # (both colour pointers null is allowed)
    for both in (dict(Q=2 ** 40, label=None), dict(Q=MAX_Q + 1, voxel=0.0), dict(Q=2 ** 31, colours=None), dict(Q=2 ** 40, oz=nan)):
        assert call(**both) == -1, both                            # invalid beats too large: nothing is launched either way


def test_the_defaults_of_the_python_surface():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    sig = inspect.signature(viz.fuse_points).parameters
    assert list(sig) == ['points', 'colours', 'voxel', 'origin'] and sig['colours'].default is None and sig['origin'].default is None
    sig = inspect.signature(results.fuse_map).parameters
    assert list(sig) == ['world', 'voxel', 'origin'] and sig['origin'].default is None
    assert list(inspect.signature(results.pool_map).parameters) == ['fused', 'values']
    assert list(inspect.signature(results.write_ply).parameters) == ['path', 'world']


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.fuse_points(torch.zeros(5, 3), voxel=0.1)
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and values only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts, cols = _meta(5, 3), _meta(5, 3)
    ok = dict(points=pts, colours=cols, voxel=0.25, origin=None)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(points=_meta(5, 4)), dict(points=_meta(5, 3, dtype=torch.float64)), dict(points=_meta(0, 3)), dict(points=_meta(15)),
               dict(points=[[0.0, 0.0, 0.0]]), dict(colours=_meta(4, 3)), dict(colours=_meta(5, 3, dtype=torch.float16)), dict(colours=_meta(5)),
               dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(voxel=1e39), dict(voxel=1e-50), dict(voxel=None),
               dict(voxel="wide"), dict(origin=(0.0, 0.0)), dict(origin=(0.0, 0.0, 0.0, 0.0)), dict(origin=(0.0, nan, 0.0)),
               dict(origin=(inf, 0.0, 0.0)), dict(origin=(0.0, 0.0, 1e39)), dict(origin="here")):
        with pytest.raises(ValueError):
            viz.fuse_points(**dict(ok, **kw))
    with pytest.raises(ValueError, match="limit"):
        viz.fuse_points(_meta(MAX_Q + 1, 3), voxel=0.25)
    # fuse_map validates its world the way filter_map does
    world = dict(points=pts, colours=cols, kf_index=_meta(5, dtype=torch.int32), seg_ids=_meta(5, dtype=torch.int32), offsets=np.array([0, 2, 5]))
    for broken in ({k: v for k, v in world.items() if k != 'colours'}, dict(world, seg_ids=None), dict(world, kf_index=[0] * 5),
                   dict(world, colours=_meta(4, 3)), dict(world, offsets=np.array([0, 2])), {k: v for k, v in world.items() if k != 'offsets'}):
        with pytest.raises(ValueError, match='fuse_map'):
            results.fuse_map(broken, 0.25)
    for voxel in (0.0, nan, -2.0):
        with pytest.raises(ValueError, match='voxel'):
            results.fuse_map(world, voxel)
    with pytest.raises(ValueError, match='origin'):
        results.fuse_map(world, 0.25, origin=(0.0, 1.0))


def test_pool_map_on_cpu_tensors_against_an_explicit_loop():
    from super_primitive_amd.odometery.results import pool_map
    rng = np.random.default_rng(601)
    Q, M = 900, 37
    label = rng.integers(-1, M, Q).astype(np.int32)
    label[label == 5] = 6                                                     # a fused row without a member left
    counts = rng.integers(0, 4, (Q, 3)).astype(np.int32)
    fused = dict(points=torch.zeros(M, 3), label=torch.from_numpy(label))
    want = np.zeros((M, 3), np.int64)
    for i in range(Q):                                                       # an explicit loop over the input rows
        if label[i] >= 0:
            want[label[i]] += counts[i]
    got = pool_map(fused, torch.from_numpy(counts))
    assert got.dtype == torch.int64 and tuple(got.shape) == (M, 3)
    np.testing.assert_array_equal(got.numpy(), want)
    assert (label < 0).sum() > 5 and not want[5].any() and want.sum() == counts[label >= 0].sum() < counts.sum()
    one = pool_map(fused, torch.from_numpy(counts[:, 1].astype(np.int64)))    # (Q,) values, another integer type
    assert tuple(one.shape) == (M,)
    np.testing.assert_array_equal(one.numpy(), want[:, 1])
    members = pool_map(fused, torch.ones(Q, dtype=torch.uint8))
    np.testing.assert_array_equal(members.numpy(), np.bincount(label[label >= 0], minlength=M))
    for bad in (torch.from_numpy(counts[:-1]), torch.zeros(Q, 3), torch.zeros(Q, 3, 2, dtype=torch.int32), counts):
        with pytest.raises(ValueError, match='pool_map'):
            pool_map(fused, bad)


def test_write_ply_on_cpu_tensors_read_back_from_its_own_header(tmp_path):
    from super_primitive_amd.odometery.results import write_ply
    rng = np.random.default_rng(602)
    M = 301
    points = rng.standard_normal((M, 3)).astype(np.float32)
    points[3] = (np.inf, -0.0, np.nan)                                       # (written as they are)
    colours = rng.uniform(-0.1, 1.1, (M, 3)).astype(np.float32)
    colours[0] = (0.0, 1.0, np.nan)
    colours[1] = (np.float32(1.0 / 255.0), np.float32(254.999 / 255.0), 0.5)
    world = dict(points=torch.from_numpy(points), colours=torch.from_numpy(colours), ids=[0, 3])
    path = tmp_path / "map.ply"
    assert write_ply(path, world) == path
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[2] == f"element vertex {M}"
    types = {"float": "<f4", "uchar": "u1"}
    fields = [(name, types[kind]) for _, kind, name in (line.split() for line in lines if line.startswith("property "))]
    assert [name for name, _ in fields] == ["x", "y", "z", "red", "green", "blue"]
    body = np.frombuffer(raw[end:], dtype=np.dtype(fields))
    assert body.shape == (M,) and len(raw) == end + 15 * M
    xyz = np.stack([body["x"], body["y"], body["z"]], axis=1)
    assert xyz.tobytes() == points.tobytes()                                 # bytes compared: the NaN and the -0.0 included
    want = np.zeros((M, 3), np.uint8)
    for i in range(M):                                                       # the renderer's 8-bit rule, channel by channel
        for ch in range(3):
            p = float(colours[i, ch]) * 255.0
            want[i, ch] = 0 if not p > 0.0 else (255 if p >= 255.0 else int(p))
    np.testing.assert_array_equal(np.stack([body["red"], body["green"], body["blue"]], axis=1), want)
    assert want[0].tolist() == [0, 255, 0] and want.min() == 0 and want.max() == 255 and want[1, 0] in (0, 1)
    empty = write_ply(tmp_path / "empty.ply", dict(points=torch.zeros(0, 3), colours=torch.zeros(0, 3)))
    assert empty.read_bytes().endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                                       b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    for broken in (dict(points=world['points']), dict(world, colours=world['colours'][:-1]), dict(world, points=world['points'].double()),
                   dict(world, colours=None), dict(world, points=points)):
        with pytest.raises(ValueError, match='write_ply'):
            write_ply(tmp_path / "bad.ply", broken)
