"""CPU: the point-table reference (tests/point_table_ref.py) against things it shares no code with -- torch.where, F.grid_sample,
F.pad + conv2d, the photometric oracle -- and what tests/test_gpu_point_table.py relies on about its cases (tests/point_table_cases.py):
validity margins, exact pyramids, the float32 position error behind C_POS, and comparisons that notice seven planted errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import point_table_cases as cases
import point_table_ref as ref
from oracle import photometric_oracle as orc

f32 = np.float32
STRIDES = (1, 2, 3, 4, 8, 16)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_table_ref_lists_the_points_in_torch_where_order(name):
    c = cases.case(name)
    masks, L = torch.from_numpy(c["masks"]), torch.from_numpy(c["logdepth"])
    for s in STRIDES:
        t = ref.table_ref(c["masks"], c["logdepth"], c["keypoints"], s)
        lat = torch.zeros_like(masks)
        lat[:, ::s, ::s] = masks[:, ::s, ::s]
        seg, row, col = torch.where(lat)
        assert np.array_equal(t["seg"], seg.numpy()) and np.array_equal(t["pix"], ((row << 16) | col).numpy().astype(np.uint32))
        assert np.array_equal(t["baseL"], L[seg, row, col].numpy()) and np.array_equal(t["counts"], lat.sum(dim=(1, 2)).numpy())
    # kp_L: the oracle's rounding (torch.round, half to even) and torch's own index wrapping where the index is legal; clamped otherwise
    rc = orc.to_pixel_index(torch.from_numpy(c["keypoints"]), (c["H"], c["W"]))
    legal = ((rc >= torch.tensor([-c["H"], -c["W"]])) & (rc < torch.tensor([c["H"], c["W"]]))).all(dim=1)
    n = torch.arange(c["N"])[legal]
    assert np.array_equal(ref.table_ref(c["masks"], c["logdepth"], c["keypoints"])["kp_L"][legal.numpy()], L[n, rc[legal, 0], rc[legal, 1]].numpy())
    if c["N"] > 2:
        assert bool(legal[cases.SEG_CHECKER]) and int(rc[cases.SEG_CHECKER, 0]) == -1 and int(rc[cases.SEG_SINGLES, 1]) == -1       # the wrapping keypoints
        assert not bool(legal[cases.SEG_ROWS])
        t = ref.table_ref(c["masks"], c["logdepth"], c["keypoints"])
        assert t["kp_L"][cases.SEG_ROWS] == c["logdepth"][cases.SEG_ROWS, 0, c["W"] - 1]                                              # ... and the clamped one


def test_keypoint_ties_round_to_even_on_65x33():
    c = cases.case("65x33")
    for n, (kr, kc) in cases.TIE_SEGMENTS.items():
        v = (0.5 * 64 * (float(c["keypoints"][n, 0]) + 1), 0.5 * 32 * (float(c["keypoints"][n, 1]) + 1))
        assert v == (kr + 0.5, kc + 0.5)
        want = (kr + kr % 2, kc + kc % 2)
        assert (int(ref.keypoint_pixel(c["keypoints"][n, 0], 65)), int(ref.keypoint_pixel(c["keypoints"][n, 1], 33))) == want
    ks = np.array(list(cases.TIE_SEGMENTS.values()))
    assert (ks % 2 == 0).any() and (ks % 2 == 1).any()


def test_padded_layout():
    counts = np.array([0, 5, 256, 257, 0, 64, 1])
    for g in (64, 256):
        pos, pad, total = ref.padded_layout(counts, g)
        starts = [int(pos[counts[:n].sum()]) for n in range(len(counts)) if counts[n]]
        assert all(s % g == 0 for s in starts) and total % g == 0 and len(pos) == counts.sum() and (~pad).sum() == counts.sum()
        assert np.array_equal(np.sort(pos), pos) and total == sum(-(-int(c) // g) * g for c in counts)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_every_case_keeps_its_distance_from_the_validity_band_and_has_the_depths_it_names(name):
    r = ref.case_ref(name)
    for s in STRIDES:
        src = r.source(s)
        assert src["margin"].size == 0 or src["margin"].min() >= 1e-4, (name, s)
    t, src = r.table(1), r.source(1)
    if r.c["N"] > 2:
        below, zinv, ordinary = t["seg"] == cases.SEG_BELOW_FLOOR, t["seg"] == cases.SEG_ZINV, t["seg"] == cases.SEG_BLOBS
        assert below.any() and zinv.any() and ordinary.any()
        assert (src["d"][below] < 0.6e-7).all() and not src["ok"][below].any()
        assert (src["d"][zinv] > 2e-7).all() and (src["d"][zinv] < 0.5e-6).all()
        assert (src["d"][ordinary] > 0.1).all()
        if name == "pp_outside":            # the principal point lies beyond the last column: these points sample across the border
            assert not src["ok"][zinv].any() and (ref.level_position(src["xn"][zinv], r.c["W"]) > r.c["W"] - 1 + 0.3).all()
        else:                               # they land on the principal point, inside the band: valid
            assert src["ok"][zinv].all()
            K = r.c["K"].astype(np.float64)
            assert np.abs(ref.level_position(src["xn"][zinv], r.c["W"]) - K[0, 2]).max() < 1e-9
        # every structure the masks promise
        counts = t["counts"]
        assert all(counts[n] == 0 for n in cases.SEG_EMPTY) and counts[cases.SEG_FULL] == r.c["H"] * r.c["W"]
        assert all(r.table(s)["counts"][cases.SEG_ODD_ROWS] == 0 for s in (2, 4, 8, 16)) and counts[cases.SEG_ODD_ROWS] > 0
        assert (r.c["masks"][cases.SEG_ROWS].sum(axis=1) == 1).any()
    assert src["ok"].any() or name == "2x2"
    assert (~src["ok"]).any()


def test_validity_equals_the_oracle_s_mask_on_an_ordinary_case():
    r = ref.case_ref("50x84")
    t, src = r.table(1), r.source(1)
    K = torch.from_numpy(r.c["K"]).double()
    col_row = torch.from_numpy(np.stack((t["pix"] & 0xffff, t["pix"] >> 16), axis=1).astype(np.int64))
    pts = orc.backproject(col_row.double(), torch.from_numpy(src["d"]), K)
    vals, ok = orc.sample_single(torch.from_numpy(r.levels[0]), pts, K, (r.c["H"], r.c["W"]))
    assert np.array_equal(ok[0].numpy(), src["ok"]) and src["ok"].any() and not src["ok"].all()


@pytest.mark.parametrize("name", ["97x131", "5x3", "2x2", "pp_outside", "33x16"])
def test_sample_ref_equals_float64_grid_sample(name):
    r = ref.case_ref(name)
    src = r.source(1)
    grid = torch.from_numpy(np.stack((src["xn"], src["yn"]), axis=1))[None, None]
    for l in range(cases.N_LEVELS):
        want = F.grid_sample(torch.from_numpy(r.levels[l])[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0].numpy()
        val, bound = r.sample(1, l)
        np.testing.assert_allclose(val, want, rtol=0, atol=1e-12)
        assert (bound > 0).all() and bound.max() < 2e-3


def test_blur_decimate_ref_equals_pad_and_conv_and_the_oracle():
    rng = np.random.default_rng(5)
    k = torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64)
    k = (k[:, None] * k[None, :] / 16.0)[None, None].repeat(3, 1, 1, 1)
    for H, W in [(2, 2), (3, 2), (2, 5), (9, 16), (17, 8), (97, 131)]:
        img = rng.uniform(size=(3, H, W))
        want = F.conv2d(F.pad(torch.from_numpy(img)[None], (1, 1, 1, 1), mode="reflect"), k, groups=3)[0, :, ::2, ::2].numpy()
        got = ref.blur_decimate_ref(img)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got, orc.blur_decimate(torch.from_numpy(img)[None])[0].numpy(), rtol=0, atol=1e-15)
    # a 1-pixel dimension (torch's reflect padding refuses it) pads with the pixel itself
    one = rng.uniform(size=(3, 1, 1))
    np.testing.assert_allclose(ref.blur_decimate_ref(one), one, rtol=0, atol=1e-15)
    col = rng.uniform(size=(1, 5, 1))
    want = F.conv2d(F.pad(torch.from_numpy(col)[None], (0, 0, 1, 1), mode="reflect"), torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64).view(1, 1, 3, 1))
    np.testing.assert_allclose(ref.blur_decimate_ref(col), want[0, :, ::2].numpy(), rtol=0, atol=1e-15)
    assert np.array_equal(ref.pack_ref(np.arange(24).reshape(3, 2, 4))[1, 2], [6, 14, 22])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_four_pyramid_levels_of_the_case_images_are_exact_in_float32(name):
    c = cases.case(name)
    for img in (c["image"], c["trg_image"]):
        assert np.array_equal(np.rint(img.astype(np.float64) * 256), img.astype(np.float64) * 256) and img.min() >= 1 / 16 and img.max() <= 1
        if min(img.shape[1:]) < 2:
            continue
        for l, lv in enumerate(ref.pyramid_ref(img, 4)):
            assert np.array_equal(lv.astype(f32).astype(np.float64), lv), (name, l)
            assert np.array_equal(np.rint(lv * 2.0 ** (8 + 4 * l)), lv * 2.0 ** (8 + 4 * l))          # at most 8 + 4 l bits below the point


def test_float32_replay_of_the_position_stays_within_half_of_c_pos():
    """Fixes C_POS: the contract's float32 operation order against the float64 position, every point of every case at every level, with
    exp moved by -2, 0, +2 ulp, in units of 2^-24 dim.  (Ordinary points: the exact position is col (Wl - 1) / (W - 1).)"""
    worst = 0.0
    for name in cases.CASE_NAMES:
        r = ref.case_ref(name)
        t, src = r.table(1), r.source(1)
        H, W = r.c["H"], r.c["W"]
        ordinary = src["d"] > 1e-6
        col = (t["pix"] & 0xffff).astype(np.float64)
        for l in range(cases.N_LEVELS):
            Hl, Wl = r.levels[l].shape[1:]
            ex_x, ex_y = ref.level_position(src["xn"], Wl), ref.level_position(src["yn"], Hl)
            assert np.abs(ex_x - col * (Wl - 1) / (W - 1))[ordinary].max() < 1e-9
            for e in (-2, 0, 2):
                ix, iy = ref.position_replay_f32(t, r.c["K"], r.kld, H, W, Hl, Wl, e)
                worst = max(worst, float(np.abs(ix - ex_x).max()) / (ref.U24 * W), float(np.abs(iy - ex_y).max()) / (ref.U24 * H))
    print(f"float32 position replay: worst {worst:.3f} x 2^-24 dim; C_POS = {ref.C_POS}")
    assert 2.0 * worst <= ref.C_POS <= 2.0 * worst + 0.1


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the GPU test's comparisons must notice each of these planted errors on the chosen cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _as_device(val):
    """a float64 reference value as the device would hand it over: (P,3) float32"""
    return np.ascontiguousarray(val.T).astype(f32)


def test_the_comparisons_pass_the_reference_itself():
    r = ref.case_ref("65x33")
    t = r.table(2)
    ref.check_table(t["counts"], t["pix"] | np.uint32(0x80000000), t["baseL"], t["kp_L"], t)
    ref.check_validity(t["pix"] | (r.source(2)["ok"].astype(np.uint32) << np.uint32(31)), r.source(2)["ok"])
    for l in range(3):
        assert ref.check_rgb(_as_device(r.sample(1, l)[0]), *r.sample(1, l)) <= 1.0
    ref.check_bitwise(r.levels[2].astype(f32), r.levels[2])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_swapped_ne_sw_weights_are_caught(name):
    r = ref.case_ref(name)
    src = r.source(1)
    caught = 0
    for l in (1, 2):
        if min(r.levels[l].shape[1:]) < 2:
            continue
        bad, _ = ref.sample_ref(r.levels[l], src["xn"], src["yn"], (r.c["H"], r.c["W"]), _alter="swap_ne_sw")
        with pytest.raises(AssertionError):
            ref.check_rgb(_as_device(bad), *r.sample(1, l))
        caught += 1
    assert caught or name == "2x2"


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_reflect_index_off_by_one_is_caught(name):
    r = ref.case_ref(name)
    for l in range(cases.N_LEVELS - 1):
        if r.levels[l].shape[1:] == (1, 1):
            continue
        with pytest.raises(AssertionError):
            ref.check_bitwise(ref.blur_decimate_ref(r.levels[l], _alter="reflect_off_by_one").astype(f32), r.levels[l + 1])


def test_keypoint_rounding_half_up_is_caught():
    r = ref.case_ref("65x33")
    t = r.table(1)
    bad = ref.table_ref(r.c["masks"], r.c["logdepth"], r.c["keypoints"], _alter="half_up")
    with pytest.raises(AssertionError, match="kp_L"):
        ref.check_table(bad["counts"], bad["pix"], bad["baseL"], bad["kp_L"], t)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_column_major_order_and_a_shifted_lattice_are_caught(name):
    r = ref.case_ref(name)
    bad = ref.table_ref(r.c["masks"], r.c["logdepth"], r.c["keypoints"], _alter="column_major")
    with pytest.raises(AssertionError, match="pixel words"):
        ref.check_table(bad["counts"], bad["pix"], bad["baseL"], bad["kp_L"], r.table(1))
    for s in (2, 3, 4, 8, 16):
        bad = ref.table_ref(r.c["masks"], r.c["logdepth"], r.c["keypoints"], s, _alter="lattice_1")
        with pytest.raises(AssertionError):
            ref.check_table(bad["counts"], bad["pix"], bad["baseL"], bad["kp_L"], r.table(s))


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_band_of_one_is_caught(name):
    r = ref.case_ref(name)
    t = r.table(1)
    bad = ref.source_ref(t, r.c["K"], r.kld, r.c["H"], r.c["W"], _band=1.0)
    with pytest.raises(AssertionError, match="validity"):
        ref.check_validity(t["pix"] | (bad["ok"].astype(np.uint32) << np.uint32(31)), r.source(1)["ok"])


def test_replicated_border_tap_is_caught():
    """Needs a position beyond the border (on the border itself the outside tap has weight 0): the case whose principal point lies outside."""
    r = ref.case_ref("pp_outside")
    src = r.source(1)
    for l in range(cases.N_LEVELS):
        bad, _ = ref.sample_ref(r.levels[l], src["xn"], src["yn"], (r.c["H"], r.c["W"]), _alter="replicate")
        with pytest.raises(AssertionError):
            ref.check_rgb(_as_device(bad), *r.sample(1, l))
