"""-m gpu: ONE call of the odometry chain (sp_chain_step_multi, csrc/sp_chain.hip, with k_chain_pyramid_multi of sp_table.hip,
k_window_compose_multi of sp_window.hip and the k_chain_crit_* / k_chain_splat_* / k_chain_select_pass kernels of sp_aux.hip) pinned stage
by stage to tests/chain_step_ref.py, and sp_kf_criterion_ws at its own granule of 4096 pixels per workgroup.

A. Glue-only calls.  A stage whose schedule has no phase (n_phases = 0) or only phases with max_iters <= 0 runs everything of the call
except the Gauss-Newton rounds, so the records are hand-made: windows of node / edge / SpPair arrays with pose and aff slots as in
test_gpu_window_gn_step.py, no image table, no cost pass; the keyframe the criterion renders is a ``chain_step_ref.scene``.  Rig: every
buffer a record names is a live allocation with a sentinel tail (one sentinel node behind n_nodes), the buffers a stage must not touch
hold sentinels or seeded contents, level[0] ("unused") is a live sentinel buffer too, keys and crit_ws start dirty; after the call EVERY
buffer of EVERY record is compared with its expectation, bit for bit -- where a quantity has a tolerance it is judged first and the
device's own value becomes the expectation, and each stage is judged from the device's own inputs to it, so no bound compounds.

Bounds (derived, not tuned):
  packed level 0        the planar image permuted: bitwise
  level l >= 1          float64 [1 2 1; 2 4 2; 1 2 1] / 16 of the DEVICE's level l - 1: nine fused multiply-adds from a zero start -- the
                        first an exact product (the weights are powers of two times 1, 2, 4), eight roundings of half an ulp at partial sums
                        no larger than the window's largest magnitude: 4 ulp there; packed = planar bitwise; bitwise sp_blur_decimate +
                        sp_pack_rgb on the same input
  target nodes          T, aff bitwise the buffers; a, m, v, aff_m, aff_v zero; aff untouched for a NULL pair; every other node bitwise
  pose / aff slots      window_gn_step_ref.compose_edge of the device's nodes: 1 ulp at max(|entry|, 1) / max(|t|, 1) (a float64 product
                        rounded once), 20 ulp for a kind-1 target with a tangent; aff slots bitwise; bitwise sp_window_compose on a copy
  LM state              [lam0, -1, 0 x 14] exactly, on the device and in state_host; track_iters = supp_iters = 0
  out_pose              window_gn_step_ref.renormalise_rotation of the device's node: 20 ulp at 1 on the rotation (19 operations on the
                        longest path + 1); translation and last row bitwise; out_aff bitwise
  slots, kld_dst        bitwise
  rel_pose              float64 inv(A) B of the device's out_pose, rigid form: inv[3] = three products and two adds (5 half-ulps at
                        sum |R t|), an entry a four-term dot (7 half-ulps at sum |inv| |B|) + inv[3]'s error through B's last row
                        (chain_step_ref.rel_pose_bound); last row exactly 0 0 0 1
  depth_out             segment_depth_ref.splat under the DEVICE's rel_pose: touched set, winner and value at RTOL on every untainted pixel;
                        bitwise sp_depth_splat under the same rel_pose
  crit                  from the device's depth_out: [0] = float32(count) / float32(HW) exactly, [1] the lower median bitwise, [2] 6 ulp
                        (three differences, squares, two adds under a root: 2.5 u + root + sum + division = 5.5 u), [3] a float64 atan2
                        rounded once: 1 ulp; crit_host = crit; bitwise sp_kf_criterion_ws on the same depth and poses
Every "bitwise the stand-alone entry point" assertion holds: the header's "their arithmetic" is kept by every instantiation met here.
Pinned as it is, and questionable: nothing.  Held although the header only implies it: level[0] is neither read nor written; a float32
denormal above valid_thresh = 0 counts as valid (the comparison does not flush it).

B. The phases (test_phases_*, test_phase_*): a real ``GnTracker`` / ``GnSuppMapper`` of the 48x64 sequence of test_gpu_sequence.py bound to
the call through ``ChainStep``, against the same schedule on a TWIN built from the same inputs: the node overwrite through
``PoseWindow.set_nodes``, then ``chain_step_ref.run_stepped`` -- fresh state, per phase the re-phase edit and up to max_iters times
sp_pairs_cost (mode 2, the phase's irls_eps) + sp_window_gn_step (the chain's flags, predicted exit included, its LM constants, the phase's
conv_tol), a phase ending at the first frozen state.  Demanded BITWISE, for TRACK and SUPP, at S = 1 and S = 3: nodes, log-depths, both
backups, state[0..15] and its pinned copy, losses, out_pose / out_aff (the twin's through ``renormalise_se3``), the depths copied into the
tracker's block, the iteration counts.  In the S = 3 calls one record starts at the optimum of its first phase and freezes after one round
while the others run on; each record is bitwise its stepped reference and its own S = 1 call.  check_first 1 / 0 and check_every 1 / 4 give
the same bits (the poll cadence shows nowhere), and a phase list with max_iters = 0 and -1 phases in the middle gives those of the list
without them (a skipped phase applies no re-phase edit).  No package change was needed: the twin calls the two entry points itself.

C. sp_kf_criterion_ws on flat arrays of n in {1, 2, 4095, 4096, 4097, 8193} floats whose contents steer the radix passes; [0], [1] exact
against numpy, [2], [3] as above, a second call on the dirty workspace bitwise.

Case -> branch
  test_glue_frames            18x22 x 3 levels (odd sizes at every level, both borders reflect), 16x24 (multiple of 4), 2x2 x 2 levels (a 1x1
                              level: reflect1_or_self), n_levels = 1, a tracker with levels {1, 2} only (packed[0] NULL); target node 0 and
                              n_nodes - 1, src_node = -1 edges, a kind-1 target, a kind-1 bystander with a tangent; phases all skipped
  test_glue_stage_masks       TRACK; SUPP; CRITERION alone (the judged pose comes through out_pose); TRACK|CRITERION; all three, the supp
                              target's pose aliasing the tracker's out_pose as in the package
  test_slot_moves             supp_images 0, 1, 2, 3
  test_criterion_scenes       nothing lands; identical poses; 180 degrees about the optical axis; an even and an odd count
  test_three_records          S = 3, records differing in P, N, kld_n (one 0), supp_images, poses, aff NULL / set, window shapes: each judged
                              as above and bitwise its own S = 1 call
  test_phases_*               see B; rounds per phase as printed: TRACK [4, 4, 5] (every phase to its max_iters), the frozen record [1, 3, 5];
                              SUPP [7] of 10, the frozen record [1]
  test_criterion_at_its_granule  see C
  test_stride_loops           130x128 (k_chain_crit_zero: HW > 64 * 256), 66x64 (the criterion's second workgroup), 150x148 with kld_n = 16388
                              (k_chain_slots_multi: 3 HW > 256 * 256; k_chain_copy_multi: > 64 * 256)
"""

import numpy as np
import pytest
import torch

import chain_step_ref as cr
import segment_depth_ref as sd
import window_gn_step_ref as wg
from gpu_util import T, npy
from test_gpu_window_gn_step import KIND1_ULPS, pose_ulps

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = -5.0
TAIL = 3
TRACK, SUPP, CRITERION = 1, 2, 4
LEVELS = 4
DIRTY_KEY = (5 << 32) | 0x40400000          # what keys hold before the call: a pixel nobody zeroes would decode to 3.0
DIRTY_WS = 0x5A5A5A5A
LM = dict(lam0=0.375, lm_up=8.0, lm_down=0.5, lm_min=1e-7)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst distance from the reference over the file: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def lib_of():
    from super_primitive_amd import _lib
    return _lib, _lib.load()


def tailed(a, tail=TAIL, fill=SENT):
    """Device float32 buffer: a's values, then ``tail`` sentinels."""
    a = np.asarray(a, f32).ravel()
    return T(np.concatenate([a, np.full(tail, fill, f32)]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------------------------------
def window_shape(rng, shape):
    """(nodes, edges (src, trg, block, weight), target nodes).  A: the package's tracker (keyframe, tracked frame; target = n_nodes - 1).
    B: a kind-1 target at index 0 with a tangent, a src_node = -1 edge.  C: four nodes, a renormalising node, a kind-1 BYSTANDER with a
    tangent (its slot is Exp(a) X), targets 3 and 1."""
    mk = lambda **kw: wg.make_node(T=wg.random_pose(rng), aff=rng.integers(-4, 5, 2) / 64.0, **kw)
    if shape == "A":
        return [mk(lr_pose=0.0, lr_aff=0.0), mk()], [(0, 1, 0, 1.0)], (1, 0)
    if shape == "B":
        return ([mk(kind=1, a=(0.02, -0.03, 0.01, 0.04, -0.02, 0.03)), mk(), mk(lr_pose=0.0, lr_aff=0.0)],
                [(-1, 0, 0, 1.0), (0, 1, 0, 0.5), (2, 1, 0, 1.0), (1, 0, 0, 1.0), (-1, 1, 0, 2.0)], (0, 1))
    if shape == "C":
        return ([mk(lr_pose=0.0, lr_aff=0.0), mk(flags=1), mk(kind=1, a=(0.01, 0.02, -0.03, 0.02, 0.01, -0.02)), mk(lr_aff=0.0)],
                [(0, 1, 0, 1.0), (0, 2, 0, 1.0), (0, 3, 0, 1.0), (1, 3, 0, 0.5), (3, 1, 0, 0.5), (-1, 2, 0, 1.0)], (1, 3))
    raise KeyError(shape)


class Win:
    """One hand-made window: nodes (+ a sentinel node), edges, pose / aff slots (+ a sentinel row), one SpPair array per level it has (all
    naming the same slots, as the package's levels do), a 16-float state full of junk and a pinned state_host."""

    def __init__(self, rec, name, rng, shape, levels):
        _lib, _ = lib_of()
        nodes, self.edges, self.targets = window_shape(rng, shape)
        self.n_nodes, self.n_edges, self.levels, self.name = len(nodes), len(self.edges), tuple(levels), name
        sent = np.zeros(1, wg.NODE)
        sent.view(f32)[:] = SENT
        rec.add(name + ".nodes", T(np.concatenate([np.array(nodes, wg.NODE), sent]).view(f32)))
        rec.add(name + ".pose", T(np.full((self.n_edges + 1) * 16, SENT, f32)))
        rec.add(name + ".aff", T(np.full((self.n_edges + 1) * 4, SENT, f32)))
        rec.add(name + ".state", tailed(np.arange(16) + 40.0))
        rec.add(name + ".state_host", torch.from_numpy(np.full(16 + TAIL, SENT, f32)).pin_memory())
        earr = (_lib.SpWindowEdge * self.n_edges)()
        for e, edge in enumerate(self.edges):
            earr[e].src_node, earr[e].trg_node, earr[e].block, earr[e].weight = int(edge[0]), int(edge[1]), int(edge[2]), float(edge[3])
        rec.add(name + ".edges", T(np.frombuffer(bytes(earr), np.uint8).copy()), pointers=False)
        for l in self.levels:
            rec.add(f"{name}.pairs{l}", self.pair_array(rec[name + ".pose"], rec[name + ".aff"]), pointers=True)
        self.rec = rec

    def pair_array(self, pose, aff):
        """SpPair records that name nothing but their slots (the glue must not touch anything else of a pair)."""
        _lib, _ = lib_of()
        parr = (_lib.SpPair * self.n_edges)()
        for e in range(self.n_edges):
            parr[e].pose, parr[e].aff = pose.data_ptr() + 64 * e, aff.data_ptr() + 16 * e
        return T(np.frombuffer(bytes(parr), np.uint8).copy())

    def fill(self, cw, phases):
        r, n = self.rec, self.name
        for l in range(LEVELS):
            g = cw.gn[l]
            g.pairs = r[f"{n}.pairs{l}"].data_ptr() if l in self.levels else None
            if l in self.levels:
                g.edges, g.nodes, g.state = r[n + ".edges"].data_ptr(), r[n + ".nodes"].data_ptr(), r[n + ".state"].data_ptr()
                g.n_edges, g.n_nodes = self.n_edges, self.n_nodes
        for p, (level, iters, eps, tol) in enumerate(phases):
            cw.phase[p].level, cw.phase[p].max_iters, cw.phase[p].irls_eps, cw.phase[p].conv_tol = level, iters, eps, tol
        cw.n_phases, cw.check_every, cw.check_first, cw.flags = len(phases), 4, 1, 2
        cw.lam0, cw.lm_up, cw.lm_down, cw.lm_min = (LM[k] for k in ("lam0", "lm_up", "lm_down", "lm_min"))
        cw.state_host = r[n + ".state_host"].data_ptr()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one record
# ---------------------------------------------------------------------------------------------------------------------------------------------
_tables = {}


def device_table(name):
    """The scene's point table on the device (its set-up is pinned by test_gpu_point_table.py), shared and never written."""
    if name not in _tables:
        from super_primitive_amd.segment_table import SegmentTable
        sc = cr.scene(name)
        _tables[name] = SegmentTable(T(sc["masks"]), T(sc["L"]), T(sc["keypoints"]))
        assert (_tables[name].N, _tables[name].P) == (sc["table"].N, sc["table"].P)
    return _tables[name]


def spec(**kw):
    s = dict(H=18, W=22, n_levels=3, stages=TRACK | SUPP | CRITERION, scene=None, t_levels=(0, 1, 2), s_levels=(0, 1), t_shape="A", s_shape="C",
             aff=True, supp_images=3, kld_n=7, seed=1, alias=False, phases=())
    s.update(kw)
    return s


class Record:
    """Every buffer one SpChainStep names, by name; ``snapshot`` reads them all back."""

    def __init__(self, sp):
        _lib, lib = lib_of()
        self.sp, self.bufs, self.pointers = sp, {}, set()
        rng = np.random.default_rng([sp["seed"], sp["H"], sp["W"]])
        H, W, nl, stages = sp["H"], sp["W"], sp["n_levels"], sp["stages"]
        self.sizes = cr.level_sizes(H, W, LEVELS)
        st = self.st = _lib.SpChainStep()
        st.stages, st.H, st.W, st.n_levels = stages, H, W, nl
        st.track_iters, st.supp_iters = -7, -7
        sc = self.scene = cr.scene(sp["scene"]) if sp["scene"] else None
        assert sc is None or (sc["H"], sc["W"]) == (H, W)
        pose_in = sc["pose"] if sc is not None else wg.random_pose(rng)
        # the frame and its planar levels ([0] is "unused": a live sentinel buffer, so a read of it shows and a write too)
        self.add("image", tailed(rng.uniform(0.05, 1.0, 3 * H * W)))
        st.image = self["image"].data_ptr()
        for l in range(LEVELS):
            if l < max(nl, 1):
                h, w = (H, W) if l == 0 else self.sizes[l]
                self.add(f"level{l}", tailed(np.full(3 * h * w, SENT)))
                st.level[l] = self[f"level{l}"].data_ptr()
        # the tracker's window and target
        self.track = Win(self, "track", rng, sp["t_shape"], sp["t_levels"])
        self.track.fill(st.track, sp["phases"])
        tg = st.track_target
        tg.node = self.track.targets[0]
        for l in sp["t_levels"]:
            h, w = self.sizes[l]
            self.add(f"track.packed{l}", tailed(rng.uniform(2.0, 3.0, 3 * h * w)))
            tg.packed[l] = self[f"track.packed{l}"].data_ptr()
        self.add("track.pose_in", tailed(pose_in))
        tg.pose = self["track.pose_in"].data_ptr()
        if sp["aff"]:
            self.add("track.aff_in", tailed([0.125, -0.25]))
            tg.aff = self["track.aff_in"].data_ptr()
        self.add("out_aff", tailed([SENT, SENT]))          # (named by the record only with an affine pair, as the package does; held either way)
        if sp["aff"]:
            st.out_aff = self["out_aff"].data_ptr()
        self.add("out_pose", tailed(np.full(16, SENT) if stages & TRACK else pose_in))
        st.out_pose = self["out_pose"].data_ptr()
        # the supplementary mapper's window, its two targets, the depth copy
        self.supp = Win(self, "supp", rng, sp["s_shape"], sp["s_levels"])
        self.supp.fill(st.supp, sp["phases"])
        for j in range(2):
            tg = st.supp_target[j]
            tg.node = self.supp.targets[j]
            for l in sp["s_levels"]:
                h, w = self.sizes[l]
                self.add(f"supp{j}.packed{l}", tailed(rng.uniform(4.0 + 2 * j, 5.0 + 2 * j, 3 * h * w)))
                tg.packed[l] = self[f"supp{j}.packed{l}"].data_ptr()
            if sp["alias"] and j == 1:
                tg.pose = self["out_pose"].data_ptr()
            else:
                self.add(f"supp{j}.pose_in", tailed(wg.random_pose(rng)))
                tg.pose = self[f"supp{j}.pose_in"].data_ptr()
            if sp["aff"]:
                self.add(f"supp{j}.aff_in", tailed([0.5 + j, -0.75 - j]))
                tg.aff = self[f"supp{j}.aff_in"].data_ptr()
        st.supp_images, st.kld_n = sp["supp_images"], sp["kld_n"]
        self.add("kld_src", tailed(rng.uniform(-1.0, 1.0, sp["kld_n"])))
        self.add("kld_dst", tailed(np.full(sp["kld_n"], SENT)))
        st.kld_src, st.kld_dst = self["kld_src"].data_ptr(), self["kld_dst"].data_ptr()
        # the keyframe the criterion renders
        st.valid_thresh = 1e-6
        if sc is not None:
            tab = self.table = device_table(sp["scene"])
            st.pix, st.baseL, st.seg_off, st.kp_L = tab.pix.data_ptr(), tab.baseL.data_ptr(), tab.seg_off.data_ptr(), tab.kp_L.data_ptr()
            st.N, st.P = tab.N, tab.P
            self.add("kld", tailed(sc["kld"]))
            self.add("K", tailed(sc["K"]))
            self.add("kf_pose", tailed(sc["kf_pose"]))
            self.add("keys", T(np.full(H * W + TAIL, DIRTY_KEY, np.int64)))
            self.add("depth", tailed(np.full(H * W, SENT)))
            self.add("rel_pose", tailed(np.full(16, SENT)))
            self.add("crit", tailed(np.full(4, SENT)))
            self.n_ws = lib.sp_kf_criterion_ws_words()
            self.add("crit_ws", T(np.full(self.n_ws + TAIL, DIRTY_WS, np.int32)))
            self.add("crit_host", torch.from_numpy(np.full(4 + TAIL, SENT, f32)).pin_memory())
            st.kld, st.K, st.kf_pose = self["kld"].data_ptr(), self["K"].data_ptr(), self["kf_pose"].data_ptr()
            st.keys, st.depth_out, st.rel_pose = self["keys"].data_ptr(), self["depth"].data_ptr(), self["rel_pose"].data_ptr()
            st.crit, st.crit_ws, st.crit_host = self["crit"].data_ptr(), self["crit_ws"].data_ptr(), self["crit_host"].data_ptr()

    def add(self, name, t, pointers=False):
        assert name not in self.bufs
        self.bufs[name] = t
        if pointers:
            self.pointers.add(name)

    def __getitem__(self, name):
        return self.bufs[name]

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: npy(v).copy() for k, v in self.bufs.items()}


def call(records):
    """One sp_chain_step_multi over the records; args_dev, states_dev and states_host carry tails.  Returns (per record: before, after,
    track_iters, supp_iters), states_host."""
    _lib, lib = lib_of()
    S = len(records)
    before = [r.snapshot() for r in records]
    nbytes = lib.sp_chain_multi_bytes()
    args = T(np.full(S * nbytes + 64, 0xA5, np.uint8))
    states_dev = T(np.full(36 * S + TAIL, SENT, f32))
    states_host = torch.from_numpy(np.full(36 * S + TAIL, SENT, f32)).pin_memory()
    arr = (_lib.SpChainStep * S)()
    for k, r in enumerate(records):
        arr[k] = r.st
    rc = lib.sp_chain_step_multi(arr, S, _lib.ptr(args), _lib.ptr(states_dev), states_host.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "sp_chain_step_multi")
    torch.cuda.synchronize()
    assert (npy(args)[S * nbytes:] == 0xA5).all(), "args_dev written behind n * sp_chain_multi_bytes()"
    sd_, sh = npy(states_dev), states_host.numpy().copy()
    assert (sd_[36 * S:] == SENT).all() and (sh[36 * S:] == SENT).all(), "states written behind 36 * n"
    assert same(sd_, sh)
    out = [(b, r.snapshot(), arr[k].track_iters, arr[k].supp_iters) for k, (r, b) in enumerate(zip(records, before))]
    stages = records[0].sp["stages"]
    for k, (r, (_, after, _, _)) in enumerate(zip(records, out)):             # the layout of states_host: [16 n] track, [16 n] supp, [4 n] criteria
        if stages & TRACK:
            assert same(sh[16 * k:16 * k + 16], after["track.state"][:16])
        if stages & SUPP:
            assert same(sh[16 * (S + k):16 * (S + k) + 16], after["supp.state"][:16])
        if stages & CRITERION:
            assert same(sh[32 * S + 4 * k:32 * S + 4 * k + 4], after["crit"][:4])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the judgement of one record, stage by stage
# ---------------------------------------------------------------------------------------------------------------------------------------------
def nodes_of(buf):
    return buf.view(wg.NODE)


def standalone_pyramid_step(src, C, h, w):
    _lib, lib = lib_of()
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x, planar, packed = T(src), T(np.full(C * ho * wo, SENT, f32)), T(np.full(C * ho * wo, SENT, f32))
    _lib.check(lib.sp_blur_decimate(_lib.ptr(x), C, h, w, _lib.ptr(planar), _lib.stream_ptr()), "sp_blur_decimate")
    _lib.check(lib.sp_pack_rgb(_lib.ptr(planar), 1, ho, wo, _lib.ptr(packed), _lib.stream_ptr()), "sp_pack_rgb")
    torch.cuda.synchronize()
    return npy(planar), npy(packed)


def judge_pyramid(r, before, after, exp, tag):
    H, W, nl = r.sp["H"], r.sp["W"], r.sp["n_levels"]
    image = before["image"][:3 * H * W]
    if 0 in r.sp["t_levels"]:
        exp["track.packed0"][:3 * H * W] = cr.pack(image.reshape(3, H, W)).ravel()
    src, (h, w) = image, (H, W)
    for l in range(1, nl):
        ho, wo = r.sizes[l]
        n = 3 * ho * wo
        got = after[f"level{l}"][:n]
        want, mag = cr.blur_decimate(src.reshape(3, h, w))
        d = (np.abs(got.reshape(3, ho, wo) - want) / np.spacing(np.maximum(mag, 1e-30).astype(f32))).max()
        note("pyramid level", d)
        assert d <= cr.BLUR_ULPS, f"{tag}: level {l} off by {d:.3g} ulp at the window's largest magnitude"
        planar, packed = standalone_pyramid_step(src, 3, h, w)
        assert same(got, planar), f"{tag}: level {l} is not sp_blur_decimate's"
        exp[f"level{l}"][:n] = got
        if l in r.sp["t_levels"]:
            exp[f"track.packed{l}"][:n] = cr.pack(got.reshape(3, ho, wo)).ravel()
            assert same(after[f"track.packed{l}"][:n], packed), f"{tag}: packed level {l} is not sp_pack_rgb's"
        src, (h, w) = got, (ho, wo)


def judge_window(r, win, after, exp, targets, tag):
    """Node overwrites (``targets``: (node, pose16, aff or None)), the recomposed slots, the fresh state."""
    _lib, lib = lib_of()
    name = win.name
    want = nodes_of(exp[name + ".nodes"])
    for node, pose, aff in targets:
        cr.set_node(want, node, pose, aff)
    got_nodes = nodes_of(after[name + ".nodes"])
    for i in range(win.n_nodes + 1):
        assert got_nodes[i].tobytes() == want[i].tobytes(), f"{tag}: {name} node {i}"
    pose, aff = after[name + ".pose"].reshape(-1, 16), after[name + ".aff"].reshape(-1, 4)
    for e, edge in enumerate(win.edges):
        P, af = wg.compose_edge(edge, got_nodes)
        assert np.array_equal(aff[e], af), f"{tag}: {name} aff slot {e}"
        nt = got_nodes[edge[1]]
        kind1 = nt["kind"] == 1 and nt["a"].any()
        d = max(pose_ulps(pose[e], P))
        note("pose slot, kind 1 with a tangent" if kind1 else "pose slot", d)
        assert d <= (KIND1_ULPS - 1 if kind1 else 1), f"{tag}: {name} pose slot {e} off by {d:.3g} ulp"
    # bitwise sp_window_compose on a copy of the device's nodes
    nodes2, pose2, aff2 = T(after[name + ".nodes"]), T(np.full_like(after[name + ".pose"], SENT)), T(np.full_like(after[name + ".aff"], SENT))
    pairs2 = win.pair_array(pose2, aff2)
    _lib.check(lib.sp_window_compose(_lib.ptr(pairs2), _lib.ptr(r[name + ".edges"]), win.n_edges, _lib.ptr(nodes2), win.n_nodes, _lib.stream_ptr()),
               "sp_window_compose")
    torch.cuda.synchronize()
    assert same(npy(pose2), after[name + ".pose"]) and same(npy(aff2), after[name + ".aff"]), f"{tag}: {name} slots are not sp_window_compose's"
    assert same(npy(nodes2), after[name + ".nodes"])
    exp[name + ".pose"], exp[name + ".aff"] = after[name + ".pose"].copy(), after[name + ".aff"].copy()
    exp[name + ".state"][:16] = cr.fresh_state(LM["lam0"])
    exp[name + ".state_host"][:16] = cr.fresh_state(LM["lam0"])


def judge_track(r, before, after, exp, tag):
    sp = r.sp
    judge_pyramid(r, before, after, exp, tag)
    node = r.track.targets[0]
    judge_window(r, r.track, after, exp, [(node, before["track.pose_in"][:16], before["track.aff_in"][:2] if sp["aff"] else None)], tag)
    nd = nodes_of(after["track.nodes"])[node]
    got = after["out_pose"][:16]
    want = wg.renormalise_rotation(nd["T"])
    rot, tr = pose_ulps(got, want)
    note("out_pose rotation", rot)
    assert rot <= wg.RENORM_OPS + 1, f"{tag}: out_pose rotation off by {rot:.3g} ulp"
    assert same(got.reshape(4, 4)[:, 3], nd["T"].reshape(4, 4)[:, 3]) and same(got[12:], nd["T"][12:]), f"{tag}: out_pose translation / last row"
    exp["out_pose"][:16] = got
    if sp["aff"]:
        exp["out_aff"][:2] = nd["aff"]


def judge_supp(r, before, after, exp, tag):
    sp = r.sp
    for l in sp["s_levels"]:
        h, w = r.sizes[l]
        n = 3 * h * w
        frame = after[f"track.packed{l}"][:n] if l in sp["t_levels"] else None
        assert frame is not None or not sp["supp_images"] & 2
        a, b = cr.slot_moves(before[f"supp0.packed{l}"][:n], before[f"supp1.packed{l}"][:n], frame, sp["supp_images"])
        exp[f"supp0.packed{l}"][:n], exp[f"supp1.packed{l}"][:n] = a, b
    targets = []
    for j in range(2):
        pose = after["out_pose"][:16] if (sp["alias"] and j == 1) else before[f"supp{j}.pose_in"][:16]
        targets.append((r.supp.targets[j], pose, before[f"supp{j}.aff_in"][:2] if sp["aff"] else None))
    judge_window(r, r.supp, after, exp, targets, tag)
    exp["kld_dst"][:sp["kld_n"]] = before["kld_src"][:sp["kld_n"]]


def close_crit(name, got, want, bound, tag):
    if np.isnan(want):
        assert np.isnan(got), f"{tag}: {name} {got} instead of NaN"
        return
    d = abs(float(got) - want) / np.spacing(f32(abs(want))) if got != want else 0.0
    note(name, d)
    assert d <= bound, f"{tag}: {name} {got!r} against {want!r}: {d:.3g} ulp"


def judge_criterion_values(got4, depth, thresh, A, B, tag):
    ratio, scale, diff, angle, cnt = cr.criterion(depth, thresh, A, B)
    assert got4[0] == ratio, f"{tag}: ratio {got4[0]!r} against {ratio!r} ({cnt} valid)"
    assert same(got4[1:2], np.array([scale], f32)) or (np.isnan(scale) and np.isnan(got4[1])), f"{tag}: scale {got4[1]!r} against {scale!r}"
    close_crit("crit translation", got4[2], diff, cr.CRIT_DIFF_ULPS, tag)
    close_crit("crit angle", got4[3], angle, cr.CRIT_ANGLE_ULPS, tag)
    return cnt


def judge_render(got, rr, tag):
    """test_gpu_segment_depth.py's rule: touched set, value and winner on every untainted pixel."""
    ok, hit = ~rr.taint, rr.count > 0
    assert np.array_equal((got != 0)[ok], hit[ok]), f"{tag}: touched set differs on {((got != 0) != hit)[ok].sum()} untainted pixels"
    sel = ok & hit
    gap = (np.abs(got - rr.image)[sel] / rr.image[sel]).max(initial=0.0)
    note("render value (relative, RTOL 2e-6)", gap)
    assert gap <= sd.RTOL, f"{tag}: render off by {gap:.3g}"
    kept = np.nonzero(rr.pix >= 0)[0]
    match = np.abs(rr.qz[kept] - got.reshape(-1)[rr.pix[kept]]) <= sd.RTOL * rr.qz[kept]
    decoded = np.full(got.size, -1, np.int64)
    np.maximum.at(decoded, rr.pix[kept][match], kept[match])
    assert np.array_equal(decoded.reshape(got.shape)[ok], rr.winner[ok]), f"{tag}: another point won a pixel"


def judge_criterion(r, before, after, exp, tag):
    _lib, lib = lib_of()
    sp, sc, tab = r.sp, r.scene, r.table
    H, W = sp["H"], sp["W"]
    A, B = after["out_pose"][:16], before["kf_pose"][:16]
    rel = after["rel_pose"][:16].reshape(4, 4)
    want, bound = cr.inv_rigid_times(A, B), cr.rel_pose_bound(A, B)
    assert same(rel[3], np.array([0, 0, 0, 1], f32)), f"{tag}: last row of rel_pose {rel[3]}"
    d = (np.abs(rel - want)[:3] / bound[:3]).max()
    note("rel_pose (share of its bound)", d)
    assert d <= 1.0, f"{tag}: rel_pose at {d:.3g} of its derived bound"
    exp["rel_pose"][:16] = rel.ravel()
    depth = after["depth"][:H * W]
    if sc["kind"] != "same":
        rr = cr.render(sc, rel)
        assert rr.taint.mean() <= 0.02
        judge_render(depth.reshape(H, W), rr, tag)
        if not rr.taint.any() and sc["parity"] is not None:
            assert int((depth > 1e-6).sum()) % 2 == sc["parity"]
    keys2, depth2 = T(np.full(H * W, DIRTY_KEY, np.int64)), T(np.full(H * W, SENT, f32))
    _lib.check(lib.sp_depth_splat(_lib.ptr(tab.pix), _lib.ptr(tab.baseL), _lib.ptr(tab.seg_off), _lib.ptr(tab.kp_L), _lib.ptr(r["kld"]), tab.N, tab.P,
                                  H, W, _lib.ptr(r["K"]), _lib.ptr(r["rel_pose"]), _lib.ptr(keys2), _lib.ptr(depth2), _lib.stream_ptr()), "sp_depth_splat")
    ws2, crit2 = T(np.full(r.n_ws, DIRTY_WS, np.int32)), T(np.full(4, SENT, f32))
    _lib.check(lib.sp_kf_criterion_ws(_lib.ptr(r["depth"]), H * W, 1e-6, _lib.ptr(r["out_pose"]), _lib.ptr(r["kf_pose"]), _lib.ptr(ws2), _lib.ptr(crit2),
                                      _lib.stream_ptr()), "sp_kf_criterion_ws")
    torch.cuda.synchronize()
    assert same(npy(depth2), depth), f"{tag}: depth_out is not sp_depth_splat's on {(npy(depth2) != depth).sum()} pixels"
    exp["depth"][:H * W] = depth
    got4 = after["crit"][:4]
    cnt = judge_criterion_values(got4, depth, 1e-6, A, B, tag)
    assert same(npy(crit2), got4), f"{tag}: crit {got4} is not sp_kf_criterion_ws's {npy(crit2)}"
    exp["crit"][:4] = got4
    exp["crit_host"][:4] = got4
    exp["keys"][:H * W] = after["keys"][:H * W]                  # scratch: only their tails are held
    exp["crit_ws"][:r.n_ws] = after["crit_ws"][:r.n_ws]
    return cnt


def judge(r, result, tag):
    """Everything one record's buffers hold after the call.  Returns the count of valid pixels (or None)."""
    before, after, t_iters, s_iters = result
    stages = r.sp["stages"]
    exp = {k: v.copy() for k, v in before.items()}
    cnt = None
    if stages & TRACK:
        judge_track(r, before, after, exp, tag)
    if stages & SUPP:
        judge_supp(r, before, after, exp, tag)
    if stages & CRITERION:
        cnt = judge_criterion(r, before, after, exp, tag)
    assert t_iters == (0 if stages & TRACK else -7) and s_iters == (0 if stages & SUPP else -7), f"{tag}: iterations {t_iters}, {s_iters}"
    for k in exp:
        assert same(after[k], exp[k]), f"{tag}: buffer {k} differs from its expectation at {np.nonzero(bits(after[k]) != bits(exp[k]))[0][:8]} (bytes)"
    return cnt


def run_one(sp, tag):
    r = Record(sp)
    res = call([r])[0]
    return r, res, judge(r, res, tag)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# A. glue-only calls
# ---------------------------------------------------------------------------------------------------------------------------------------------
SKIPPED = ((1, 0, 1e-3, 2e-3), (0, -1, 1e-3, 2e-3), (1, 0, 1e-5, 1e-4))          # phases the header lets a stage skip

FRAMES = {
    "18x22, three levels": spec(scene="odd18x22", alias=True, seed=11),
    "16x24, kind-1 target at node 0": spec(H=16, W=24, scene="even16x24", stages=TRACK | CRITERION, t_shape="B", seed=12),
    "2x2, a 1x1 level": spec(H=2, W=2, n_levels=2, stages=TRACK | SUPP, t_levels=(0, 1), s_levels=(0, 1), seed=13),
    "one level": spec(n_levels=1, stages=TRACK | SUPP, t_levels=(0,), s_levels=(0,), t_shape="C", s_shape="B", seed=14),
    "tracker without level 0": spec(stages=TRACK | SUPP, t_levels=(1, 2), s_levels=(1,), seed=15),
    "every phase skipped": spec(scene="even18x22", phases=SKIPPED, seed=16, aff=False),
}


@pytest.mark.parametrize("name", list(FRAMES))
def test_glue_frames(name):
    run_one(FRAMES[name], name)


@pytest.mark.parametrize("stages", [TRACK, SUPP, CRITERION, TRACK | CRITERION, TRACK | SUPP | CRITERION])
def test_glue_stage_masks(stages):
    r, (before, after, _, _), _ = run_one(spec(stages=stages, scene="odd18x22", alias=bool(stages & TRACK), seed=20 + stages), f"stages {stages}")
    if stages == CRITERION:
        assert same(after["out_pose"], before["out_pose"]) and same(before["out_pose"][:16], r.scene["pose"].ravel())
    if not stages & TRACK:                     # the windows and buffers of an absent stage: the final sweep held them to their bytes; say so
        assert same(after["track.state"], before["track.state"]) and same(after["level1"], before["level1"])


@pytest.mark.parametrize("supp_images", [0, 1, 2, 3])
def test_slot_moves(supp_images):
    r, (before, after, _, _), _ = run_one(spec(stages=SUPP, supp_images=supp_images, seed=30 + supp_images), f"supp_images {supp_images}")
    n = 3 * 18 * 22
    if supp_images == 3:                       # slot 0 ends with the OLD slot 1, slot 1 with the frame
        assert same(after["supp0.packed0"][:n], before["supp1.packed0"][:n]) and same(after["supp1.packed0"][:n], before["track.packed0"][:n])
        assert not same(before["supp1.packed0"][:n], before["track.packed0"][:n])
    assert same(after["track.packed2"], before["track.packed2"])                     # a level the supp window lacks


@pytest.mark.parametrize("scene,count", [("behind18x22", 0), ("same18x22", None), ("flip18x22", None), ("even18x22", 0), ("odd18x22", 1)])
def test_criterion_scenes(scene, count):
    r, (before, after, _, _), cnt = run_one(spec(stages=CRITERION, scene=scene, seed=40), scene)
    c = after["crit"][:4]
    if scene == "behind18x22":
        assert cnt == 0 and c[0] == 0 and np.isnan(c[1]) and np.isnan(c[2]) and 0 < c[3] < 20
        assert not after["depth"][:18 * 22].any()
    elif scene == "same18x22":
        assert cnt > 50 and c[2] == 0 and c[3] == 0 and c[1] > 0.5
    elif scene == "flip18x22":
        assert abs(float(c[3]) - 180.0) < 1e-3
    else:
        assert cnt % 2 == count and cnt > 50


THREE = [spec(scene="odd18x22", alias=True, seed=51, kld_n=7, supp_images=3, aff=True, t_shape="A", s_shape="C"),
         spec(scene="flip18x22", seed=52, kld_n=0, supp_images=1, aff=False, t_shape="B", s_shape="B", t_levels=(1, 2)),
         spec(scene="same18x22", seed=53, kld_n=300, supp_images=2, aff=True, t_shape="C", s_shape="C", s_levels=(1,))]


@pytest.mark.parametrize("stages", [TRACK | SUPP | CRITERION, CRITERION, SUPP])
def test_three_records(stages):
    specs = [dict(s, stages=stages, alias=s["alias"] and bool(stages & TRACK)) for s in THREE]
    together = [Record(s) for s in specs]
    results = call(together)
    for k, (r, res) in enumerate(zip(together, results)):
        judge(r, res, f"S = 3, record {k}")
    for k, s in enumerate(specs):
        alone = Record(s)
        res = call([alone])[0]
        for name in res[1]:
            if name in alone.pointers or name in ("keys", "crit_ws"):
                continue
            assert same(res[1][name], results[k][1][name]), f"record {k}: {name} differs between S = 3 and S = 1"
        assert res[2:] == results[k][2:]


@pytest.mark.parametrize("name", ["zero130x128", "granule66x64"])
def test_stride_loops_of_the_criterion(name):
    sc = cr.scene(name)
    r, _, cnt = run_one(spec(H=sc["H"], W=sc["W"], stages=CRITERION, scene=name, seed=60), name)
    assert cnt > 100


def test_stride_loops_of_the_slot_moves_and_the_depth_copy():
    assert 3 * 150 * 148 > 256 * 256 and 16385 + 3 > 64 * 256
    run_one(spec(H=150, W=148, n_levels=1, stages=SUPP, t_levels=(0,), s_levels=(0,), kld_n=16385 + 3, seed=61), "150x148, kld_n 16388")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# C. sp_kf_criterion_ws at its own granule
# ---------------------------------------------------------------------------------------------------------------------------------------------
def criterion_contents(n, rng):
    """{name: (depth float32 (n,), thresh)}: contents that steer the radix passes."""
    out = {}
    out["all equal"] = (np.full(n, 1.5, f32), 1e-6)
    out["lowest byte"] = ((np.uint32(0x3FC00000) + rng.integers(0, 256, n).astype(np.uint32)).view(f32), 1e-6)
    out["top byte"] = (rng.choice(np.array([1e-5, 0.5, 2.0, 3e4], f32), n), 1e-6)
    plateau = np.sort(rng.uniform(0.2, 9.0, n).astype(f32))
    plateau[n // 3:max(2 * n // 3, n // 3 + 1)] = 1.25 if n > 2 else plateau[n // 3]
    out["plateau across the median"] = (rng.permutation(np.sort(plateau)), 1e-6)
    for parity in (0, 1):
        d = rng.uniform(0.2, 9.0, n).astype(f32)
        holes = rng.permutation(n)[:(n // 3 // 2) * 2 + ((n - parity) % 2)]          # an even number of holes, one more where the parity asks
        d[holes] = 0.0
        assert (d > 1e-6).sum() % 2 == parity
        out[f"{'odd' if parity else 'even'} count"] = (d, 1e-6)
    out["a value equal to thresh"] = (rng.choice(np.array([0.75, 0.5, 1.0, 2.0], f32), n), 0.75)
    out["a denormal above thresh = 0"] = (rng.choice(np.array([0.0, 1e-42, 1e-40, 3.0], f32), n), 0.0)
    out["NaN and negative"] = (rng.choice(np.array([np.nan, -1.0, -0.0, 0.7, 1.3], f32), n), 1e-6)
    out["+inf among the valid"] = (rng.choice(np.array([np.inf, np.inf, 1.0, 0.0], f32), n), 1e-6)
    return out


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8193])
def test_criterion_at_its_granule(n):
    _lib, lib = lib_of()
    rng = np.random.default_rng(9000 + n)
    A, B = wg.random_pose(rng), wg.random_pose(rng)
    A[3] = B[3] = (0, 0, 0, 1)
    a, b = T(A), T(B)
    words = lib.sp_kf_criterion_ws_words()
    ws = T(np.full(words + TAIL, DIRTY_WS, np.int32))
    for name, (depth, thresh) in criterion_contents(n, rng).items():
        assert depth.shape == (n,) and depth.dtype == f32
        d, out = tailed(depth, fill=7.0), tailed(np.full(4, SENT))
        runs = []
        for _ in range(2):                     # the second call finds the workspace the first one left
            _lib.check(lib.sp_kf_criterion_ws(_lib.ptr(d), n, float(thresh), _lib.ptr(a), _lib.ptr(b), _lib.ptr(ws), _lib.ptr(out), _lib.stream_ptr()),
                       "sp_kf_criterion_ws")
            torch.cuda.synchronize()
            runs.append(npy(out).copy())
        tag = f"n = {n}, {name}"
        assert same(runs[0], runs[1]), f"{tag}: a dirty workspace changes the result"
        assert (runs[0][4:] == SENT).all() and same(npy(d)[:n], depth) and (npy(ws)[words:] == DIRTY_WS).all(), tag
        judge_criterion_values(runs[0][:4], depth, f32(thresh), A, B, tag)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# B. the phases: the call against the same schedule stepped on a twin window
# ---------------------------------------------------------------------------------------------------------------------------------------------
_sequence = []


def sequence():
    if not _sequence:
        from test_gpu_sequence import make_sequence_inputs
        _sequence.append(make_sequence_inputs(n=6, H=48, W=64, N=6))
    return _sequence[0]


def t32(a):
    return T(np.asarray(a, f32))


def window_result(win):
    torch.cuda.synchronize()
    gn = win._gn_state()
    return dict(nodes=npy(win.nodes).copy(), kld=npy(win.kld).copy(), nodes_backup=npy(gn["nodes_backup"]).copy(), kld_backup=npy(gn["kld_backup"]).copy(),
                state=npy(gn["state"]).copy(), losses=npy(gn["losses"]).copy())


class Bound:
    """A keyframe-0 tracker (and, for SUPP, the supplementary mapper of frames i - 1 and i) of the 48x64 sequence, bound to a ChainStep."""

    def __init__(self, i, supp=False, kld=None, phases=None):
        from super_primitive_amd.odometery.chain import ChainStep
        from super_primitive_amd.odometery.loops import GnSuppMapper, GnTracker
        seq, frames, to_kf = sequence()
        self.i, self.frames = i, frames
        kf, pose0, aff0 = to_kf(0), t32(seq[0].T_wc), torch.zeros(2, device="cuda:0")
        kld = t32(seq[0].kld_gt) if kld is None else kld
        self.tracker = GnTracker(kf, kld, pose0, frames[i], (0, 3), kf_aff=aff0)
        self.mapper = None
        if supp:
            rows = [[(frames[j], t32(seq[j].T_wc), aff0.clone()) for j in (i - 1, i)]]
            self.mapper = GnSuppMapper([kf], [pose0], [kld], [aff0], rows, 10)
        for obj in (self.tracker, self.mapper):
            if obj is not None and phases is not None:
                obj.phases = list(phases)
        self.chain = ChainStep(6, 48, 64, 3, torch.device("cuda:0"))
        self.chain.bind_tracker(self.tracker, kf, True)
        if supp:
            self.chain.bind_mapper(self.mapper)
            for j in (i - 1, i):               # the tracked poses the supplementary mapping starts from: a little off the truth
                self.chain.hist_pose[j].copy_(t32(seq[j].T_wc))
                self.chain.hist_pose[j][:3, 3] += 0.002 * (j + 1)
                self.chain.hist_aff[j].copy_(t32([0.01 * j, -0.02]))
        self.win = (self.mapper if supp else self.tracker).win
        self.pose0 = pose0

    def job(self, start=None):
        if self.mapper is not None:
            return dict(stages=SUPP, i=self.i, prev=self.i - 1, supp_images=0)
        pose, aff = (self.pose0, t32([0.01, -0.01])) if start is None else start
        return dict(stages=TRACK, i=self.i, image=self.frames[self.i].image, start_pose=pose, start_aff=aff)

    def result(self, iters):
        out = window_result(self.win)
        out["iters"] = iters
        out["state_host"] = self.win._gn_state()["state_host"].numpy().copy()
        if self.mapper is None:
            out["out_pose"], out["out_aff"] = npy(self.chain.hist_pose[self.i]).copy(), npy(self.chain.hist_aff[self.i]).copy()
        else:
            out["tracker_kld"] = npy(self.tracker.win.kld).copy()
        return out

    def stepped(self, start=None):
        """The stages' work before the phases through the package's own (pinned) entry points, then ``chain_step_ref.run_stepped``."""
        from super_primitive_amd.lie.lie_algebra import renormalise_se3
        from super_primitive_amd.optim import window as W
        _lib, lib = lib_of()
        win, job = self.win, self.job(start)
        if self.mapper is None:
            win.set_nodes({1: dict(T=job["start_pose"], aff=job["start_aff"])})
        else:
            win.set_nodes({self.mapper.slots[k]: dict(T=self.chain.hist_pose[j], aff=self.chain.hist_aff[j]) for k, j in enumerate((self.i - 1, self.i))})
        flags = W.gn_flags(False, W.GN_PREDICTED_EXIT, win.depths_fixed)
        gn = win._gn_state()

        class Ops:
            def read_state(_):
                return npy(gn["state"]).copy()

            def write_state(_, st):
                gn["state"].copy_(t32(st))

            def cost(_, level, eps):
                r = win.gn_record(level)
                _lib.check(lib.sp_pairs_cost(r.pairs, r.chunks, r.spans, r.n_spans, 2, float(eps), r.span_partials, r.seg_partials, _lib.stream_ptr()),
                           "sp_pairs_cost")

            def step(_, level, tol):
                r = win.gn_record(level)
                _lib.check(lib.sp_window_gn_step(r.pairs, r.edges, r.n_edges, r.nodes, r.n_nodes, r.blocks, r.n_blocks, r.sum_N, r.max_N, r.n_unknowns,
                                                 r.span_partials, r.seg_partials, r.scratch, r.nodes_backup, r.kld_backup, flags, W.GN_LM["lm_up"],
                                                 W.GN_LM["lm_down"], W.GN_LM["lm_min"], float(tol), r.state, r.losses, r.max_losses, _lib.stream_ptr()),
                           "sp_window_gn_step")

        phases = (self.mapper or self.tracker).phases
        rounds = cr.run_stepped(Ops(), phases, W.GN_LM["lam0"])
        out = window_result(win)
        out["iters"] = int(out["state"][5])
        out["state_host"] = out["state"].copy()
        if self.mapper is None:
            out["out_pose"] = npy(renormalise_se3(win.node_poses()[1].contiguous())).copy()
            out["out_aff"] = npy(win.node_affines()[1]).copy()
        else:
            out["tracker_kld"] = out["kld"][:len(npy(self.tracker.win.kld))].copy()
        return out, rounds


def run_bound(bounds, starts=None, **sched):
    """One call over the bound chains (one: ChainStep.run's own path).  ``sched``: check_first / check_every overrides."""
    from super_primitive_amd.odometery.chain import ChainStepBatch
    starts = starts or [None] * len(bounds)
    for b in bounds:
        cw = b.chain.st.supp if b.mapper is not None else b.chain.st.track
        for k, v in sched.items():
            setattr(cw, k, v)
    res = ChainStepBatch(torch.device("cuda:0")).run([(b.chain, b.job(s)) for b, s in zip(bounds, starts)])
    return [b.result(r[1] if b.mapper is not None else r[0]) for b, r in zip(bounds, res)]


def assert_same_result(got, want, tag):
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert same(g, w), f"{tag}: {k} differs" + (f": {g} against {w}" if g.size <= 16 else f" in {(bits(g) != bits(w)).sum()} bytes")


def optimum_of(i, supp):
    """What one call on frame i converges to: the mapped log-depths, or the tracked pose and affine pair of a long first phase alone (the optimum of
    THAT level: a later call from it freezes in its first phase)."""
    first = Bound(i).tracker.phases[0]
    b = Bound(i, supp, phases=None if supp else [(first[0], 40, first[2], 1e-6)])
    res = run_bound([b])[0]
    return t32(res["kld"]) if supp else (t32(res["out_pose"]), t32(res["out_aff"]))


# the poll cadence must not show in any result: a window that froze sits through the rounds nobody looked before, inert
CADENCES = (dict(check_first=1, check_every=4), dict(check_first=0, check_every=1), dict(check_first=0, check_every=4))


@pytest.mark.parametrize("supp", [False, True], ids=["TRACK", "SUPP"])
def test_phases_are_the_stepped_calls(supp):
    i = 3
    want, rounds = Bound(i, supp).stepped()
    got = run_bound([Bound(i, supp)])[0]
    print(f"\n{'SUPP' if supp else 'TRACK'} of frame {i}: rounds per phase {rounds}, {want['iters']} iterations, final lambda {want['state'][0]:.3g}")
    assert sum(rounds) >= 2 and want["iters"] == sum(rounds)
    assert_same_result(got, want, "S = 1")
    if supp:
        assert same(got["tracker_kld"], got["kld"][:len(got["tracker_kld"])])
    for sched in CADENCES:
        assert_same_result(run_bound([Bound(i, supp)], **sched)[0], want, str(sched))


@pytest.mark.parametrize("supp", [False, True], ids=["TRACK", "SUPP"])
def test_phases_of_three_records(supp):
    best = optimum_of(2, supp)
    make = lambda: [Bound(2, supp, kld=best if supp else None), Bound(3, supp), Bound(4 if supp else 1, supp)]
    starts = [None if supp else best, None, None]
    wants = [b.stepped(s) for b, s in zip(make(), starts)]
    print(f"\n{'SUPP' if supp else 'TRACK'}, three records: rounds per phase {[r for _, r in wants]}")
    first = wants[0][1]
    limit = Bound(2, supp)
    assert first[0] < (limit.mapper or limit.tracker).phases[0][1], "the record at its optimum does not freeze in its first phase"
    assert sum(wants[1][1]) > sum(first) or sum(wants[2][1]) > sum(first)
    together = run_bound(make(), starts)
    for k, b in enumerate(make()):
        assert_same_result(together[k], wants[k][0], f"record {k} of S = 3 against its stepped reference")
        assert_same_result(run_bound([b], [starts[k]])[0], together[k], f"record {k}: S = 1 against S = 3")
    for sched in CADENCES:                     # the record that freezes after one round of a longer phase, alone, under every cadence
        assert_same_result(run_bound(make()[:1], starts[:1], **sched)[0], wants[0][0], f"the frozen record under {sched}")


def test_phase_with_no_iterations_in_the_middle_is_skipped():
    base = Bound(3).tracker.phases
    phases = [base[0], (base[0][0], 0, 5e-2, 0.5), (base[1][0], -1, 5e-2, 0.5)] + list(base[1:])
    assert len(phases) <= 6
    want, rounds = Bound(3, phases=base).stepped()
    got = run_bound([Bound(3, phases=phases)])[0]
    assert len(rounds) == len(base)
    assert_same_result(got, want, "a max_iters = 0 phase in the middle")
    assert_same_result(Bound(3, phases=phases).stepped()[0], want, "the stepped driver on the same list")
