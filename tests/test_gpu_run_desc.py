"""Run descriptors (include/sp_hip.h SpRunDesc): the cost passes of a wave-span depth table rebuild every point's pixel word from
one 32-byte record per 64-point group instead of reading pix.

* CPU: the host reference builder / decoder below on hand-made groups (one run, two runs, padding, more runs);
* GPU: sp_run_desc_build against that reference on grid, blobs, SAM-like and odd-size tables; the decoded words against pix on
  every point of every group of at most two runs; mode-0 and mode-1 partials and 20 Gauss-Newton steps (also with conv_tol) bitwise
  equal with and without descriptors.
"""
import numpy as np
import pytest
import torch

LANE = np.arange(64)


def ref_build(pix):
    """(64 G,) uint32 pixel words -> ((G + 1, 8) uint32 records, (G,) runs): what sp_run_desc_build writes."""
    w = np.asarray(pix, dtype=np.uint32).reshape(-1, 64)
    w = np.concatenate((w, np.zeros((1, 64), np.uint32)))
    G = w.shape[0]
    v = (w & 0x7fffffff).astype(np.int64)
    nz = w != 0
    last = np.where(nz.any(1), 63 - np.argmax(nz[:, ::-1], axis=1), 0)
    prev = np.concatenate((v[:, :1], v[:, :-1]), axis=1)
    starts = (LANE == 0)[None, :] | ((LANE[None, :] <= last[:, None]) & (v != prev + 1))
    runs = starts.sum(1)
    rest = starts.copy()
    rest[:, 0] = False
    s1 = np.where(rest.any(1), np.argmax(rest, axis=1), 64)
    v0, v1 = v[:, 0], v[np.arange(G), s1 & 63]
    c0, r0 = v0 & 0xffff, v0 >> 16
    c1 = np.where(s1 < 64, v1 & 0xffff, c0 + s1)
    r1 = np.where(s1 < 64, v1 >> 16, r0)
    bits = (w >> 31).astype(np.uint64) << LANE.astype(np.uint64)[None, :]
    valid = np.bitwise_or.reduce(bits, axis=1)
    f = lambda a: np.asarray(a, np.float32).view(np.uint32)
    rec = np.stack(((valid & 0xffffffff).astype(np.uint32), (valid >> np.uint64(32)).astype(np.uint32), f(c1 - s1 - c0), f(r1 - r0),
                    f(c0), f(r0), f(1 - s1), runs.astype(np.uint32)), axis=1)
    return rec, runs[:-1]


def ref_decode(rec):
    """(G, 8) uint32 records -> (64 G,) uint32 words by the formula of include/sp_hip.h (float arithmetic, as the cost pass does it)."""
    rec = np.asarray(rec, np.uint32)
    fl = rec.view(np.float32)
    lane = LANE.astype(np.float32)[None, :]
    step = np.clip(lane + fl[:, 6:7], np.float32(0), np.float32(1))
    col = (step * fl[:, 2:3] + lane) + fl[:, 4:5]
    row = (step * fl[:, 3:4] + np.float32(0)) + fl[:, 5:6]
    valid = ((rec[:, 0:1].astype(np.uint64) | (rec[:, 1:2].astype(np.uint64) << np.uint64(32))) >> LANE.astype(np.uint64)[None, :]) & np.uint64(1)
    return ((row.astype(np.uint32) << 16) | col.astype(np.uint32) | (valid.astype(np.uint32) << 31)).reshape(-1)


def real_lanes(pix):
    """Lanes up to each group's last nonzero word (the rest is padding; lane 0 always counts)."""
    nz = np.asarray(pix, np.uint32).reshape(-1, 64) != 0
    last = np.where(nz.any(1), 63 - np.argmax(nz[:, ::-1], axis=1), 0)
    return (LANE[None, :] <= last[:, None]).reshape(-1)


def word(r, c, ok=True):
    return (r << 16) | c | (0x80000000 if ok else 0)


def test_reference_format_round_trip():
    g_one = [word(7, 10 + l, ok=l % 3 != 0) for l in range(64)]                                   # one run
    g_two = [word(3, 60 + l) for l in range(20)] + [word(4, 2 + l, ok=l != 5) for l in range(44)]   # a row break at lane 20
    g_pad = [word(9, 100 + l) for l in range(37)] + [0] * 27                                      # the tail of a segment
    g_zero = [0, word(0, 1)] + [word(1, l) for l in range(30)] + [0] * 32                          # pixel (0, 0), invalid
    g_three = [word(5, l) for l in range(10)] + [word(6, l) for l in range(10)] + [word(7, l) for l in range(44)]
    pix = np.array(g_one + g_two + g_pad + g_zero + g_three, dtype=np.uint32)
    rec, runs = ref_build(pix)
    assert runs.tolist() == [1, 2, 1, 2, 3]
    assert rec.shape == (6, 8) and rec[-1, 0] == rec[-1, 1] == 0 and rec[-1, 7] == 1
    got = ref_decode(rec[:-1])
    ok = np.repeat(runs <= 2, 64) & real_lanes(pix)
    np.testing.assert_array_equal(got[ok], pix[ok])
    assert not np.array_equal(got[4 * 64: 5 * 64], pix[4 * 64:])          # three runs: the formula does not hold
    # padding lanes continue the last run, invalid
    assert (got[2 * 64 + 37: 3 * 64] >> 31 == 0).all()
    assert (got[2 * 64 + 37: 3 * 64] & 0xffff).tolist() == list(range(137, 164))


def _batch(shape, H=480, W=640, N=64, n=2, seed=300, **kw):
    from super_primitive_amd import synth
    from super_primitive_amd.optim.pair_batch import PairBatch
    shape_kw = dict(overlap=4) if shape == "grid" else dict(shape=shape, blob_coverage=1.2)
    pairs = [synth.make_pair(H, W, N, seed=seed + k, init_sigma=0.004, **shape_kw) for k in range(n)]
    return PairBatch.from_synth(pairs, levels=(0, 2), device="cuda:0", granule=64, **kw)


def _device_records(batch):
    from super_primitive_amd import _lib
    n_groups = batch.pix.numel() // 64
    rd = torch.empty((n_groups + 1) * 8, dtype=torch.int32, device="cuda:0")
    n_general = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    _lib.check(batch.lib.sp_run_desc_build(_lib.ptr(batch.pix), n_groups, _lib.ptr(rd), _lib.ptr(n_general), _lib.stream_ptr()), "sp_run_desc_build")
    torch.cuda.synchronize()
    return rd.cpu().numpy().view(np.uint32).reshape(-1, 8), int(n_general.item())


CASES = [("grid", 480, 640, 64), ("grid", 121, 203, 4), ("blobs", 120, 160, 40), ("sam", 120, 160, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,H,W,N", CASES)
def test_device_records_match_reference_and_decode_to_pix(shape, H, W, N):
    batch = _batch(shape, H, W, N)
    pix = batch.pix.cpu().numpy().view(np.uint32)
    got, n_general = _device_records(batch)
    want, runs = ref_build(pix)
    np.testing.assert_array_equal(got, want)
    assert n_general == int((runs > 2).sum())
    assert (batch.run_desc is not None) == (n_general == 0)
    ok = np.repeat(runs <= 2, 64) & real_lanes(pix)
    np.testing.assert_array_equal(ref_decode(got[:-1])[ok], pix[ok])
    if shape == "grid":
        assert n_general == 0 and batch.run_desc is not None


def _partials(batch, mode):
    from super_primitive_amd import _lib
    batch.cost_pass(0, mode)
    torch.cuda.synchronize()
    NV = _lib.SP_GN_PARTIAL_FLOATS if mode == 1 else _lib.SP_GRAD_PARTIAL_FLOATS
    NS = _lib.SP_GN_SEG_FLOATS if mode == 1 else _lib.SP_GRAD_SEG_FLOATS
    return batch.partials[: batch.n_spans * NV].clone(), batch.seg_partials[: batch.n_seg_records * NS].clone()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,N", [(480, 640, 64), (121, 203, 4)])
def test_partials_bitwise_with_and_without_descriptors(H, W, N):
    batch = _batch("grid", H, W, N)
    rd = batch.run_desc
    assert rd is not None
    for mode in (0, 1):
        with_rd = _partials(batch, mode)
        batch.run_desc = None
        without = _partials(batch, mode)
        batch.run_desc = rd
        assert torch.equal(with_rd[0], without[0]) and torch.equal(with_rd[1], without[1]), mode


@pytest.mark.gpu
@pytest.mark.parametrize("conv_tol", [0.0, 1e-4])
def test_gn_steps_bitwise_with_and_without_descriptors(conv_tol):
    a = _batch("grid", n=3, seed=320)
    b = _batch("grid", n=3, seed=320, run_desc=False)
    assert a.run_desc is not None and b.run_desc is None
    for _ in range(20):
        ca = a.gn_step(0, conv_tol=conv_tol).clone()
        cb = b.gn_step(0, conv_tol=conv_tol).clone()
        assert torch.equal(ca, cb)
    torch.cuda.synchronize()
    assert torch.equal(a.pose, b.pose) and torch.equal(a.kld, b.kld) and torch.equal(a.costs(), b.costs())
    for _ in range(5):
        assert torch.equal(a.adam_step(0).clone(), b.adam_step(0).clone())
    assert torch.equal(a.pose, b.pose) and torch.equal(a.kld, b.kld)
