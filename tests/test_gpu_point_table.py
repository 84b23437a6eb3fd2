"""-m gpu: the point-table set-up against the independent reference of tests/point_table_ref.py, on every point.

Per-keyframe path (SegmentTable: sp_mask_count, sp_table_fill, sp_table_sample_source; sp_blur_decimate; sp_pack_rgb) and batched path
(PairBatch: sp_prepare_count / _count_boxed / _fill / _sample / _sample_pairs / _blur_pack / _gather) on the cases of
tests/point_table_cases.py: counts, pixel words in torch.where order, log-depths, kp_L, the padded layout with its zero padding, the
decimated lattices, pyramids and packed targets are EXACT; bit 31 of every pixel word equals the reference's validity; every colour lies
within the reference's per-point bound.  tests/test_point_table_ref_host.py proves on the CPU that these comparisons notice a swapped
weight pair, a reflect index off by one, half-up keypoint rounding, column-major order, a band of 1.0, a shifted lattice and a replicated
border tap.

Measured on gfx950, worst err / bound per pyramid level (0, 1, 2): per-keyframe path 0.321, 0.218, 0.103; batched path 0.321, 0.218,
0.103 (the two paths compute bitwise the same samples)."""
import numpy as np
import pytest
import torch

import point_table_cases as cases
import point_table_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu
LEVELS = tuple(range(cases.N_LEVELS))
FAST_PATH = ["33x16", "64x1024", "300x64", "1104x16", "pp_outside"]          # W a multiple of 16 up to 1024: the count pass's fast path
WORST = {"per-keyframe": [0.0] * cases.N_LEVELS, "batched": [0.0] * cases.N_LEVELS}


def _note(path, level, ratio):
    WORST[path][level] = max(WORST[path][level], ratio)


def _report(path, what):
    print(f"{what}: worst err / bound per level so far ({path} path): " + ", ".join(f"{w:.3f}" for w in WORST[path]))


def _check_samples(src4, r, stride, level, path, what):
    """src4 (P,4) of a table's real points against the reference: w bitwise the log-depth, colours within the bound"""
    t = r.table(stride)
    assert np.array_equal(np.ascontiguousarray(src4[:, 3]).view(np.uint32), t["baseL"].view(np.uint32)), f"{what}: src4.w"
    _note(path, level, ref.check_rgb(src4[:, :3], *r.sample(stride, level), what=what))


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_per_keyframe_tables_pyramid_and_samples_equal_the_reference(name):
    from super_primitive_amd.image import gaussian_pyramid
    from super_primitive_amd.segment_table import SegmentTable, packed_target
    r = ref.case_ref(name)
    c, t = r.c, r.table(1)
    tab = SegmentTable(T(c["masks"]), T(c["logdepth"]), T(c["keypoints"]))
    ref.check_table(tab.counts, npy(tab.pix), npy(tab.baseL), npy(tab.kp_L), t, name)
    assert not (npy(tab.pix).view(np.uint32) >> 31).any() and tab.P == len(t["pix"])
    assert np.array_equal(npy(tab.seg_off), np.concatenate(([0], np.cumsum(t["counts"]))))
    lv_s, lv_t = [T(c["image"])], [T(c["trg_image"])]
    for l in LEVELS[1:]:
        lv_s.append(gaussian_pyramid.blur_decimate(lv_s[-1][None])[0])
        lv_t.append(gaussian_pyramid.blur_decimate(lv_t[-1][None])[0])
    for l in LEVELS:
        ref.check_bitwise(npy(lv_s[l]), r.levels[l], f"{name}: source level {l}")
        ref.check_bitwise(npy(lv_t[l]), r.trg_levels[l], f"{name}: target level {l}")
        ref.check_bitwise(npy(packed_target(lv_t[l]))[0], ref.pack_ref(r.trg_levels[l]), f"{name}: packed target level {l}")
    K, kld = T(c["K"]), T(r.kld)
    for l in LEVELS:
        src4 = npy(tab.source_level(lv_s[l], K, kld, cache=False))
        ref.check_table(tab.counts, npy(tab.pix), npy(tab.baseL), npy(tab.kp_L), t, name)
        ref.check_validity(npy(tab.pix), r.source(1)["ok"], f"{name}: after level {l}")
        _check_samples(src4, r, 1, l, "per-keyframe", f"{name}: level {l}")
    _report("per-keyframe", name)


# ---------------------------------------------------------------------------------------------------------------------------------
# batched path
# ---------------------------------------------------------------------------------------------------------------------------------
def _boxes(name):
    """tight boxes of a case's masks, except: the whole-frame segment's box reaches past the image, empty segments get inverted boxes"""
    from super_primitive_amd.optim.batch_prepare import segment_boxes_of
    c = cases.case(name)
    b = segment_boxes_of(T(c["masks"])).cpu()
    full = 0 if c["N"] == 2 else cases.SEG_FULL
    b[full] = torch.tensor([-3, -5, c["H"] + 4, c["W"] + 9], dtype=torch.int32)
    if c["N"] > 2:
        for n in cases.SEG_EMPTY:
            b[n] = torch.tensor([5, 7, 2, 3], dtype=torch.int32)
    return b


def _build(names, granule, point_stride, extra_tables=(), boxes=False):
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.pair_batch import PairBatch
    frames, trg, trg_K, klds = [], [], [], []
    for name in names:
        r = ref.case_ref(name)
        c = r.c
        kf = KeyFrame(T(c["image"]), T(c["K"]), T(c["logdepth"]), T(c["keypoints"]), T(c["masks"]))
        if boxes:
            kf.segment_boxes = _boxes(name).to(kf.image.device)
        frames.append(kf)
        trg.append(T(c["trg_image"]))
        trg_K.append(T(c["K_trg"]))
        klds.append(T(r.kld))
    poses = torch.eye(4, device=frames[0].image.device)[None].repeat(len(names), 1, 1)
    return PairBatch(frames, trg, trg_K, poses, klds, levels=(0, cases.N_LEVELS), point_stride=point_stride, extra_tables=extra_tables,
                     granule=granule, depth_table=False, lazy_levels=False, tile_points=1024)


def _check_batch(batch, names, granule, coarse_keys, what):
    from super_primitive_amd import _lib
    refs = [ref.case_ref(n) for n in names]
    M = len(names)
    assert batch.M == M and sorted(batch.coarse) == sorted(coarse_keys)
    # per-pair scalars, gathered inputs, level sizes, packed targets
    assert batch.Ns == [r.c["N"] for r in refs] and batch.Ps == [len(r.table(1)["pix"]) for r in refs]
    assert np.array_equal(npy(batch.kld).view(np.uint32), np.concatenate([r.kld for r in refs]).view(np.uint32)), f"{what}: gathered log-depth seeds"
    k4 = lambda K: np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
    for l in LEVELS:
        d = np.frombuffer(npy(batch.desc[l]).tobytes(), dtype=np.dtype(_lib.SpPair))
        off = 0
        for m, r in enumerate(refs):
            Hl, Wl = r.trg_levels[l].shape[1:]
            assert batch.level_hw[l][m] == (Hl, Wl)
            assert np.array_equal(d["K_src"][m], k4(r.c["K"])) and np.array_equal(d["K_trg"][m], k4(r.c["K_trg"])), f"{what}: gathered intrinsics"
            assert (d["N"][m], d["P"][m], d["H"][m], d["W"][m], d["Hl"][m], d["Wl"][m]) == (r.c["N"], batch.Ps[m], r.c["H"], r.c["W"], Hl, Wl)
            ref.check_bitwise(npy(batch.trg4[l][off: off + 3 * Hl * Wl]).reshape(Hl, Wl, 3), ref.pack_ref(r.trg_levels[l]), f"{what}: {names[m]} packed target {l}")
            off += 3 * Hl * Wl
        assert batch.trg4[l].numel() == off
    n_off = np.concatenate(([0], np.cumsum(batch.Ns)))
    kp_L = npy(batch.kp_L)
    # the all-points table at every level, then every decimated table at its own level: reference -> padded layout -> flat arrays
    tables = [(1, list(LEVELS), npy(batch.pix), {l: npy(batch.src4[l]).reshape(-1, 4) for l in LEVELS})]
    for stride in sorted({s for _, s in coarse_keys}):
        lays = {l: lay for (l, s), lay in batch.coarse.items() if s == stride}
        first = next(iter(lays.values()))
        assert all(lay.pix is first.pix or torch.equal(lay.pix, first.pix) for lay in lays.values())
        tables.append((stride, sorted(lays), npy(first.pix), {l: npy(lay.src4).reshape(-1, 4) for l, lay in lays.items()}))
        assert first.points == [len(r.table(stride)["pix"]) for r in refs]
    for stride, levels, pix_flat, src4_flat in tables:
        lo = 0
        for m, r in enumerate(refs):
            w = f"{what}: {names[m]} stride {stride}"
            t = r.table(stride)
            pos, pad, total = ref.padded_layout(t["counts"], granule)
            assert lo + total <= len(pix_flat), w
            if stride == 1:
                assert (batch.p_off[m], batch.p_off[m + 1]) == (lo, lo + total), w
            pix = pix_flat[lo: lo + total]
            ref.check_table(t["counts"], pix[pos], None, kp_L[n_off[m]: n_off[m + 1]], t, w)
            ref.check_validity(pix[pos], r.source(stride)["ok"], w)
            assert not pix[pad].any(), f"{w}: padding pixel words"
            for l in levels:
                src4 = src4_flat[l][lo: lo + total]
                assert not src4[pad].view(np.uint32).any(), f"{w}: padding samples, level {l}"
                _check_samples(src4[pos], r, stride, l, "batched", f"{w} level {l}")
            lo += total
        assert len(pix_flat) == max(lo, 1) and all(len(s) == max(lo, 1) for s in src4_flat.values()), f"{what}: stride {stride} table size"
    _report("batched", what)


@pytest.mark.parametrize("granule", [256, 64])
@pytest.mark.parametrize("strides,extra", [((1, 2, 4), ()), ((1, 8, 16), ()), ((1, 2, 4), ((1, 3),))], ids=["s124", "s1816", "s124+3"])
def test_batched_tables_of_one_ragged_batch_equal_the_reference(granule, strides, extra):
    """(1, 2, 4) and (1, 8, 16): fast-path keyframes go through the 16-byte count pass and the bit-word fill; the extra stride-3 table
    (no divisor of 16) forces the general count and fill for the whole batch."""
    batch = _build(cases.CASE_NAMES, granule, strides, extra)
    keys = [(l, s) for l, s in zip(LEVELS, strides) if s > 1] + [tuple(e) for e in extra]
    _check_batch(batch, cases.CASE_NAMES, granule, keys, f"granule {granule} strides {strides} {extra}")


def test_batched_tables_with_segment_boxes_equal_the_reference():
    """Tight boxes from segment_boxes_of, one reaching past the image, inverted ones on the empty segments.  The fast-path keyframes as
    one batch (all boxed: sp_prepare_count_boxed); the others, which ignore their boxes, with one boxed fast-path keyframe as a second
    (sp_prepare_count with boxes)."""
    c0 = int(_boxes("33x16")[cases.SEG_BLOBS, 1])
    assert c0 % 16 != 0                                      # a box that starts inside a 16-pixel piece
    others = [n for n in cases.CASE_NAMES if n not in FAST_PATH] + ["33x16"]
    for names in (FAST_PATH, others):
        batch = _build(names, 256, (1, 2, 4), boxes=True)
        _check_batch(batch, names, 256, [(1, 2), (2, 4)], f"boxed {names[0]}..")


def test_nan_log_depths_clear_the_validity_bit():
    """A segment whose log-depths are NaN: bit 31 is clear on all its points, on both paths (its colours are left open)."""
    from super_primitive_amd.segment_table import SegmentTable
    r = ref.case_ref("nan")
    c, t, src = r.c, r.table(1), r.source(1)
    nan_seg = t["seg"] == 1
    assert nan_seg.any() and not src["ok"][nan_seg].any() and src["ok"][~nan_seg].any()
    tab = SegmentTable(T(c["masks"]), T(c["logdepth"]), T(c["keypoints"]))
    src4 = npy(tab.source_level(T(c["image"]), T(c["K"]), T(r.kld), cache=False))
    ref.check_table(tab.counts, npy(tab.pix), npy(tab.baseL), npy(tab.kp_L), t, "nan")
    ref.check_validity(npy(tab.pix), src["ok"], "nan, per keyframe")
    val, bound = r.sample(1, 0)
    ref.check_rgb(src4[~nan_seg, :3], val[:, ~nan_seg], bound[:, ~nan_seg], "nan, per keyframe")
    for granule in (256, 64):
        batch = _build(["nan"], granule, (1, 1, 1))
        pos, pad, total = ref.padded_layout(t["counts"], granule)
        pix = npy(batch.pix)
        assert len(pix) == total and not pix[pad].any()
        ref.check_table(t["counts"], pix[pos], None, npy(batch.kp_L), t, "nan, batched")
        ref.check_validity(pix[pos], src["ok"], "nan, batched")
        got = npy(batch.src4[0]).reshape(-1, 4)[pos]
        ref.check_rgb(got[~nan_seg, :3], val[:, ~nan_seg], bound[:, ~nan_seg], "nan, batched")
