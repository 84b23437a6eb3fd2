"""-m gpu: ONE launch of the many-pairs cost pass (sp_pairs_cost_opt through the C ABI) against the float64 per-point reference of
tests/cost_pass_ref.py -- every span record and every segment record, column by column.

For each case of tests/cost_pass_cases.py and each variant of the kernel (modes 1 and 2: 1, 1|DT, 1|W64, 1|DT|W64, 1|DT|W64 with run
descriptors, 2; mode 0: 0, 0|DT|W64, 0|DT|W64 with run descriptors) the records are written into buffers pre-filled with a sentinel, the
reference is evaluated on the tables, target level, poses and work list READ BACK FROM THE BATCH, and then

    |got - want64| <= KAPPA n_e + allowance_e       for every defined column of every record (nothing is scaled by a block maximum),
    |got - want64| <= KAPPA_MANY n_e + allowance_e  in addition, for the records that sum at least MANY_POINTS (16) valid points,
    valid points (span [28], segment [9]) exact, up to the record's fragile points,
    the unused span columns are zero, the unused segment columns and the records past the work list keep the sentinel.

n_e is the reference's float32 yardstick of that very entry, allowance_e what the record's fragile points may add (both in
tests/cost_pass_ref.py; tests/test_cost_pass_ref_host.py shows on the CPU that this comparison catches fifteen planted errors with a factor
ten to spare: the weakest of them, a negated H_pp(1,5), exceeds KAPPA n_e 134 times).  KAPPA cannot be derived -- the kernel's v_rcp_f32
and exponential are not the twin's division and exp -- so it is four times the worst err / n_e measured on gfx950 over all cases, rounded
up to one digit.  Measured, worst err / n_e per variant over all its cases (span blocks, then segment blocks):

    variant        sum|r|  H_pp   b_p   | H_pd    D      b_d    seg sum|r|      (mode 2: H_aa 1.000, b_a 1.667, H_ap 0.931, H_ad 3.870)
    1              1.204   1.642  1.294 | 25.250  3.902  3.285  2.315
    1|DT           1.229   1.740  1.179 |  9.935  2.507  2.864  3.724
    1|W64          2.102   2.433  3.020 | 25.250  3.902  3.172  2.102
    1|DT|W64       2.187   2.285  2.851 |  9.935  1.893  2.791  3.724
    1|DT|W64 + RD  1.700   2.212  2.023 |  4.669  2.488  1.482  2.349
    2              1.204   1.642  1.345 | 25.250  3.959  3.285  --
                   sum|r|  g_t    g_R    g_aff | g_kld
    0              1.151   0.967  0.704  0.819 | 1.602
    0|DT|W64       1.779   1.436  2.105  2.244 | 2.706
    0|DT|W64 + RD  1.406   1.933  2.105  1.312 | 3.442

The 25.25 (and 9.9, 4.7, 3.4) are entries of SINGLE-PIXEL segments' records: there n_e is one draw of the float32 twin's rounding error,
and in H_pd[5] of one of them it came out a hundredth of what the same point's other columns carry, while the device's error, 1.9e-6 of
the entry, is smaller than theirs.  KAPPA = 4 x 25.25 -> 200 therefore says little about the kernel; over the records of 16 and more valid
points (2 and more give the same figures) the worst is 5.128 (mode 2, H_pd; 3.3 elsewhere), KAPPA_MANY = 4 x 5.128 -> 30, and today's
kernel meets that bound with a factor 5.8 to spare, the all-entry bound with 7.9.  Nothing in the kernel was found wrong.
"""
import functools

import numpy as np
import pytest
import torch

import cost_pass_cases as cases
import cost_pass_ref as ref
from gpu_util import T, npy

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(1.0e30)
SENTINEL_BITS = SENTINEL.view(np.uint32)
EXTRA = 3                                     # records past the work list, which no launch may touch
WORST = {}                                    # variant -> block -> worst err / n_e so far


@functools.lru_cache(maxsize=None)
def _batch(name, granule, depth_table, run_desc, with_aff):
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.optim.pair_batch import PairBatch
    c = cases.case(name)
    frames = [KeyFrame(T(s["image"]), T(s["K"]), T(s["logdepth"]), T(s["keypoints"]), T(s["masks"])) for s in c["scenes"]]
    poses = torch.stack([T(s["pose"]) for s in c["scenes"]])
    batch = PairBatch(frames, [T(s["trg_image"]) for s in c["scenes"]], [T(s["K_trg"]) for s in c["scenes"]], poses, [T(s["kld"]) for s in c["scenes"]],
                      levels=(0, max(c["levels"]) + 1), use_affine=with_aff, tile_points=c["tile_points"], span_points=c["span_points"][granule],
                      granule=granule, depth_table=depth_table, run_desc=run_desc, lazy_levels=False)
    assert (batch.run_desc is not None) == run_desc, "the case's segments do not decode from run descriptors"
    return batch


def _launch_inputs(batch, level, affs):
    """what the launch reads, copied to the host: (pairs, chunks, spans)"""
    from super_primitive_amd import _lib
    d = np.frombuffer(npy(batch.desc[level]).tobytes(), dtype=np.dtype(_lib.SpPair))
    pix, src4 = npy(batch.pix).view(np.uint32), npy(batch.src4[level]).reshape(-1, 4)
    kp_L, kld, pose, trg = npy(batch.kp_L), npy(batch.kld), npy(batch.pose).reshape(-1, 4, 4), npy(batch.trg4[level])
    pairs, t0 = [], 0
    for m in range(batch.M):
        Hl, Wl = batch.level_hw[level][m]
        assert (int(d["Hl"][m]), int(d["Wl"][m]), int(d["N"][m]), int(d["P"][m])) == (Hl, Wl, batch.Ns[m], batch.Ps[m])
        p0, p1, n0, n1 = batch.p_off[m], batch.p_off[m + 1], batch.n_off[m], batch.n_off[m + 1]
        pairs.append(ref.pair_inputs(pix[p0:p1], src4[p0:p1], kp_L[n0:n1], kld[n0:n1], trg[t0: t0 + 3 * Hl * Wl], d["K_src"][m], d["K_trg"][m], d["H"][m], d["W"][m],
                                     Hl, Wl, d["P"][m], d["zmin"][m], pose[m], None if affs is None else affs[m]))
        t0 += 3 * Hl * Wl
    return pairs, npy(batch.chunks).reshape(-1, 4), npy(batch.spans).reshape(-1, 4)


def _run(name, variant, level, eps):
    from super_primitive_amd import _lib
    v, c = cases.VARIANTS[variant], cases.case(name)
    affs = [cases.scene_aff(s, variant) for s in c["scenes"]]
    with_aff = affs[0] is not None
    batch = _batch(name, v["granule"], v["dt"], v["rd"], with_aff)
    if with_aff:
        batch.aff.copy_(T(np.stack(affs)))
    pairs, chunks, spans = _launch_inputs(batch, level, affs if with_aff else None)
    mf = cases.mode_flags(variant)
    mode = mf & 0xff
    S, Rn = ref.n_records(chunks, spans, v["granule"] == 64)
    assert S == batch.n_spans and Rn == batch.n_seg_records
    NV, NS = ref.SPAN_FLOATS[mode], ref.SEG_FLOATS[mode]
    span_buf = torch.full(((S + EXTRA) * NV,), float(SENTINEL), dtype=torch.float32, device=batch.device)
    seg_buf = torch.full(((Rn + EXTRA) * NS,), float(SENTINEL), dtype=torch.float32, device=batch.device)
    rd = v["rd"]
    _lib.check(batch.lib.sp_pairs_cost_opt(_lib.ptr(batch.desc[level]), _lib.ptr(batch.chunks), _lib.ptr(batch.spans), batch.n_spans, mf, float(eps), _lib.ptr(span_buf),
                                           _lib.ptr(seg_buf), _lib.ptr(None), _lib.ptr(batch.pix if rd else None), _lib.ptr(batch.run_desc if rd else None),
                                           _lib.stream_ptr()), "sp_pairs_cost_opt")
    torch.cuda.synchronize()
    r = ref.launch_ref(pairs, chunks, spans, mf, eps)
    what = f"{name} {variant} level {level} eps {eps:g}"
    for valid, fragile in zip(r["valid"], r["fragile"]):
        assert fragile <= 0.002 * valid and (fragile == 0 or name not in cases.NO_FRAGILE), f"{what}: {fragile} fragile points of {valid}"
    ratios = ref.ratios_by_block(npy(span_buf).reshape(-1, NV)[:S], npy(seg_buf).reshape(-1, NS)[:Rn], r)
    w = WORST.setdefault(variant, {})
    for k, x in ratios.items():
        w[k] = max(w.get(k, 0.0), x)
    print(f"{what}: valid {r['valid']} fragile {r['fragile']} err / n_e " + ", ".join(f"{k} {x:.3f}" for k, x in ratios.items()))
    print(f"worst err / n_e so far ({variant}): " + ", ".join(f"{k} {x:.3f}" for k, x in w.items()) + f"   [KAPPA {ref.KAPPA:g}]")
    many = ref.ratios_by_block(npy(span_buf).reshape(-1, NV)[:S], npy(seg_buf).reshape(-1, NS)[:Rn], r, min_points=ref.MANY_POINTS)
    wm = WORST.setdefault((variant, "many"), {})
    for k, x in many.items():
        wm[k] = max(wm.get(k, 0.0), x)
    print(f"  ... over records of {ref.MANY_POINTS}+ valid points: " + ", ".join(f"{k} {x:.3f}" for k, x in wm.items()) + f"   [KAPPA_MANY {ref.KAPPA_MANY:g}]")
    ref.compare(npy(span_buf).reshape(-1, NV), npy(seg_buf).reshape(-1, NS), r, ref.KAPPA, SENTINEL_BITS, what)
    return r, npy(span_buf).reshape(-1, NV)[:S], npy(seg_buf).reshape(-1, NS)[:Rn], chunks, spans


@pytest.mark.parametrize("name,variant,level,eps", cases.GN_RUNS, ids=[f"{n}-{v}-l{l}-eps{e:g}" for n, v, l, e in cases.GN_RUNS])
def test_gauss_newton_records_equal_the_float64_reference_entry_by_entry(name, variant, level, eps):
    r, span, seg, chunks, spans = _run(name, variant, level, eps)
    if name == "validity":
        # the segment behind the camera: every record of its chunks, and the span that holds nothing else, are exact zeros
        per = 1 if cases.VARIANTS[variant]["granule"] == 64 else 4
        for q in np.nonzero(chunks[:, 1] == 0)[0]:
            assert not seg[per * q: per * q + per, ref.SEG_DEFINED[r["mode"]]].any()
        assert r["valid"][0] > 0 and not r["seg"][np.repeat(chunks[:, 1] == 0, per)].any()


@pytest.mark.parametrize("name,variant,level,eps", cases.GRAD_RUNS, ids=[f"{n}-{v}-l{l}-eps{e:g}" for n, v, l, e in cases.GRAD_RUNS])
def test_gradient_records_equal_the_float64_reference_entry_by_entry(name, variant, level, eps):
    _run(name, variant, level, eps)
