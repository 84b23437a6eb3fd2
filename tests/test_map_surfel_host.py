"""CPU-only: the ABI of the map normals and the surfel render (include/sp_hip.h: sp_map_normals, sp_render_surfels), their argument
checks -- made before any device work, so they answer without a GPU --, the argument checks of the Python surface (``tool/viz.py``
``render_views(normals=...)``, ``odometery/results.py`` ``render_map`` / ``score_map`` / ``score_map_images``), and the parts of the
feature that are host arithmetic: ``write_ply`` with normals, ``filter_map`` and the fused normal (``fused_normals``) on CPU tensors."""
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
    for name in ("sp_map_normals", "sp_render_surfels"):
        assert name in _lib.SIGNATURES, name
    assert "strictly increasing" in header and "PRECONDITION" in header          # the table order the neighbour search relies on
    assert "sp_render_splats, bit for bit on every pixel" in header and "sp_render_views in mode 1, bit for bit on every pixel" in header


def test_render_surfels_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)                                    # (never dereferenced: the checks fail first)
    ok = dict(points=p, colours=p, normals=p, Q=10, views=p, V=1, H=4, W=4, z_min=1e-6, radii=p, max_px=3, cull=0, keys=p, image=p, depth=p,
              index=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_render_surfels(a['points'], a['colours'], a['normals'], a['Q'], a['views'], a['V'], a['H'], a['W'], a['z_min'], a['radii'],
                                     a['max_px'], a['cull'], a['keys'], a['image'], a['depth'], a['index'], None)
    for bad in (dict(normals=None), dict(cull=2), dict(cull=-1), dict(max_px=17), dict(max_px=-1), dict(z_min=-1.0), dict(z_min=float("nan")),
                dict(points=None), dict(views=None), dict(keys=None), dict(radii=None), dict(colours=None), dict(Q=0), dict(V=0), dict(H=0),
                dict(W=-3)):
        assert call(**bad) == -1, bad
    for big in (dict(Q=2 ** 31 - 1), dict(V=65536), dict(H=1 << 16, W=1 << 15), dict(V=2, H=1 << 15, W=1 << 15)):
        assert call(**big) == -2, big
    assert call(Q=2 ** 40, normals=None) == -1 and call(V=65536, cull=2) == -1       # invalid beats too large


def test_map_normals_refuses_bad_arguments_without_a_device():
    from super_primitive_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(0x2000)
    ok = dict(kfs=p, n_kf=2, total_blocks=3, stride=1, align=None, n_align=0, normals=p, total_rows=600)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sp_map_normals(a['kfs'], a['n_kf'], a['total_blocks'], a['stride'], a['align'], a['n_align'], a['normals'], a['total_rows'], None)
    for bad in (dict(stride=0), dict(stride=-2), dict(kfs=None), dict(normals=None), dict(n_kf=0), dict(n_kf=65536), dict(total_blocks=0),
                dict(n_align=1), dict(align=p), dict(n_align=-1), dict(total_rows=0), dict(total_rows=3 * 256 + 1)):
        assert call(**bad) == -1, bad


def test_the_new_keywords_default_to_the_existing_call():
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    sig = inspect.signature(viz.render_views).parameters
    assert sig['normals'].default is None and sig['cull'].default is False
    for fn in (results.render_map, results.score_map, results.score_map_images):
        sig = inspect.signature(fn).parameters
        assert sig['normals'].default is False and sig['cull'].default is False, fn.__name__
    for fn in (results.keyframe_points, results.sequence_map):
        assert inspect.signature(fn).parameters['normals'].default is False, fn.__name__
    assert callable(viz.keyframe_normals) and callable(results.fused_normals)


def _meta(*shape, dtype=torch.float32):
    """A tensor without storage: every case must raise before a pointer is taken."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_python_surface_raises_value_error_before_any_launch(monkeypatch):
    from super_primitive_amd import _lib
    from super_primitive_amd.odometery import results
    from super_primitive_amd.tool import viz
    with pytest.raises(ValueError, match="HIP-only"):                          # CPU tensors
        viz.render_views(torch.zeros(5, 3), torch.zeros(5, 3), torch.eye(3), torch.eye(4)[None], 4, 4, depth_buffer=True, radii=torch.zeros(5),
                         normals=torch.zeros(5, 3))
    monkeypatch.setattr(_lib, "require_device", lambda *t: None)              # shapes and dtypes only: nothing below reaches a launch
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error reached the library"))
    pts, cols, K, eye, rad, nrm = _meta(5, 3), _meta(5, 3), _meta(3, 3), _meta(1, 4, 4), _meta(5), _meta(5, 3)
    ok = dict(points=pts, colours=cols, Ks=K, poses=eye, H=4, W=6, depth_buffer=True, radii=rad, max_px=3, normals=nrm)
    with pytest.raises(ValueError, match="radii"):
        viz.render_views(**dict(ok, radii=None))
    with pytest.raises(ValueError, match="depth_buffer"):
        viz.render_views(**dict(ok, depth_buffer=False))
    with pytest.raises(ValueError, match="cull"):
        viz.render_views(**dict(ok, normals=None, cull=True))
    for kw in (dict(normals=_meta(4, 3)), dict(normals=_meta(5)), dict(normals=_meta(5, 3, dtype=torch.float64)), dict(normals=[[0.0, 0.0, 1.0]] * 5),
               dict(max_px=17)):
        with pytest.raises(ValueError):
            viz.render_views(**dict(ok, **kw))
    bare, world = dict(points=pts, colours=cols), dict(points=pts, colours=cols, normals=nrm)
    with pytest.raises(ValueError, match="normals"):
        results.render_map(bare, K, eye, (4, 6), radii=rad, normals=True)      # the world has none
    with pytest.raises(ValueError, match="radii"):
        results.render_map(world, K, eye, (4, 6), normals=True)                # radii are missing
    with pytest.raises(ValueError, match="normals"):
        results.score_map(bare, _meta(1, 4, 6), K, eye, radii=rad, normals=True)
    with pytest.raises(ValueError, match="radii"):
        results.score_map(world, _meta(1, 4, 6), K, eye, normals=True)
    with pytest.raises(ValueError, match="normals"):
        results.score_map_images(bare, _meta(1, 3, 4, 6), K, eye, radii=rad, normals=True)
    with pytest.raises(ValueError):
        results.render_map(dict(world, normals=_meta(4, 3)), K, eye, (4, 6), radii=rad, normals=True)


# ---- write_ply ------------------------------------------------------------------------------------------------------------------------
def _world(M, seed, normals=True):
    rng = np.random.default_rng(seed)
    w = dict(points=torch.from_numpy(rng.uniform(-2, 2, (M, 3)).astype(np.float32)),
             colours=torch.from_numpy(rng.uniform(-0.1, 1.1, (M, 3)).astype(np.float32)))
    if normals:
        n = rng.standard_normal((M, 3))
        w['normals'] = torch.from_numpy((n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
        w['normals'][0] = 0.0
    w['colours'][1, 0] = float("nan")
    return w


def _u8(colours):
    p = colours.numpy().astype(np.float64) * 255.0
    with np.errstate(invalid='ignore'):
        return np.trunc(np.where(p > 0, np.minimum(p, 255.0), 0.0)).astype(np.uint8)


def test_write_ply_with_normals_reads_back(tmp_path):
    from super_primitive_amd.odometery.results import write_ply
    w = _world(37, 1)
    path = write_ply(tmp_path / "map.ply", w)
    raw = open(path, 'rb').read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode('ascii') == ("ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\nproperty float y\nproperty float z\n"
                                    "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                                    "property uchar blue\n")
    vertex = np.dtype([('p', '<f4', 3), ('n', '<f4', 3), ('c', 'u1', 3)])
    assert vertex.itemsize == 27 and len(body) == 37 * 27
    rows = np.frombuffer(body, dtype=vertex)
    assert np.array_equal(rows['p'], w['points'].numpy()) and np.array_equal(rows['n'], w['normals'].numpy())
    assert np.array_equal(rows['c'], _u8(w['colours']))
    for bad in (w['normals'][:5], w['normals'].double(), w['normals'].numpy()):
        with pytest.raises(ValueError, match="normals"):
            write_ply(tmp_path / "bad.ply", dict(w, normals=bad))


def test_write_ply_without_normals_is_the_file_it_always_was(tmp_path):
    """Byte for byte the parent's file: its header and its 15-byte rows, assembled here as the parent's code assembled them."""
    from super_primitive_amd.odometery.results import write_ply
    w = _world(21, 2, normals=False)
    raw = open(write_ply(tmp_path / "map.ply", w), 'rb').read()
    points, colours = w['points'], w['colours']
    M = 21
    rgb = torch.nan_to_num(colours.detach().double() * 255.0, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)
    rows = torch.cat((points.detach().contiguous().view(torch.uint8).reshape(M, 12), rgb), dim=1).cpu().numpy()
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {M}\n" + "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert raw == header.encode('ascii') + rows.tobytes()
    assert raw == open(write_ply(tmp_path / "none.ply", dict(w, normals=None)), 'rb').read()


# ---- fusion and filtering on CPU tensors ---------------------------------------------------------------------------------------------------
def test_fused_normals_match_a_float64_loop_and_repeat_bit_for_bit():
    from super_primitive_amd.odometery.results import fused_normals
    rng = np.random.default_rng(3)
    Q, M = 500, 23
    n = rng.standard_normal((Q, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    label = rng.integers(-1, M - 3, Q).astype(np.int32)                        # -1: dropped rows; the last three fused points have no member
    n[10] = (np.nan, 0.5, np.inf)                                              # non-finite components count as 0
    # fused point 0: two opposite members and nothing else -> zero
    label[label == 0] = 1
    label[[3, 4]] = 0
    n[3] = (0.6, -0.8, 0.0)
    n[4] = (-0.6, 0.8, 0.0)
    got = fused_normals(torch.from_numpy(n), torch.from_numpy(label), M)
    again = fused_normals(torch.from_numpy(n), torch.from_numpy(label), M)
    assert got.dtype == torch.float32 and tuple(got.shape) == (M, 3)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    want = np.zeros((M, 3))
    sums = np.zeros((M, 3), np.int64)
    for i in range(Q):
        if label[i] >= 0:
            for a in range(3):
                x = float(n[i, a])
                sums[label[i], a] += int(np.rint(x * 2.0 ** 20)) if np.isfinite(x) else 0
    for j in range(M):
        S = sums[j].astype(np.float64)
        length = np.sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2])
        want[j] = S / length if length > 0 else 0.0
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert not got[0].any() and not got[M - 3:].any() and not sums[0].any()
    length = np.linalg.norm(got.numpy().astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1.0) < 2e-7) | (length == 0))
    with pytest.raises(ValueError):
        fused_normals(torch.from_numpy(n).double(), torch.from_numpy(label), M)
    with pytest.raises(ValueError):
        fused_normals(torch.from_numpy(n), torch.from_numpy(label[:-1]), M)


def test_pool_map_is_unchanged_by_the_shared_sum():
    from super_primitive_amd.odometery.results import pool_map
    label = torch.tensor([0, 2, -1, 2, 1, 0], dtype=torch.int32)
    fused = dict(label=label, points=torch.zeros(3, 3))
    values = torch.tensor([[1, 2], [3, 4], [100, 100], [5, 6], [7, 8], [9, 10]], dtype=torch.int32)
    assert pool_map(fused, values).tolist() == [[10, 12], [7, 8], [8, 10]] and pool_map(fused, values[:, 0]).tolist() == [10, 7, 8]


def test_filter_map_keeps_the_normals_of_the_rows_it_keeps():
    from super_primitive_amd.odometery.results import filter_map
    w = _world(12, 4)
    w.update(kf_index=torch.tensor([0] * 5 + [1] * 7, dtype=torch.int32), seg_ids=torch.arange(12, dtype=torch.int32), offsets=np.array([0, 5, 12]),
             ids=[3, 8])
    counts = torch.zeros(12, 3, dtype=torch.int32)
    counts[[1, 4, 5, 9, 11], 0] = 1
    out = filter_map(w, dict(counts=counts))
    assert out['kept'].tolist() == [1, 4, 5, 9, 11] and out['offsets'].tolist() == [0, 2, 5]
    assert torch.equal(out['normals'], w['normals'][out['kept']]) and torch.equal(out['points'], w['points'][out['kept']])
    bare = {k: v for k, v in w.items() if k != 'normals'}
    assert 'normals' not in filter_map(bare, dict(counts=counts))
    with pytest.raises(ValueError, match="normals"):
        filter_map(dict(w, normals=w['normals'][:7]), dict(counts=counts))
