"""-m gpu: ONE call of the fused SE(3)-Adam window optimiser (sp_window_step: k_window_reduce and both instantiations of k_window_update in
csrc/sp_window.hip) against the float64 yardstick of tests/window_adam_step_ref.py, on the hand-made windows of tests/window_adam_cases.py.

The call reads only the mode-0 partial records, a few SpPair fields and the node / edge / block arrays, so everything is hand-made (no
image, no table, no cost pass; pix, src4, kp_L and trg3 stay NULL).  Rig: guard records valued 1e6 in front of and behind every edge's span
and segment records (tile0, rec0 > 0); sentinel tails behind every kld block, every block's m / v, losses, the 12-float state, the scratch
(sp_window_scratch_doubles) and the pose / aff slots; one sentinel node behind n_nodes; the slots initialised by sp_window_compose and
checked against compose_edge.  After every call EVERY buffer the call may write is compared -- whole nodes, every block's kld / m / v,
every slot, state, losses, all sentinels and guards -- and the reference continues from the DEVICE's values, so each call is judged from
identical inputs.

Bounds (derived, not tuned).
  parameters, moments   adam_bound of the yardstick (its docstring counts the roundings); the host file proves it is at most 2e-6 lr + 1 ulp
                        of the parameter on every input used here, and that torch.optim.Adam on the CPU lies inside it
  kind-0 T, folded      a float64 product rounded once: 1 ulp at max(|entry|, 1) / max(|t|, 1), plus what the tangent's own adam_bound is
                        worth in T Exp(-a): 2.02 sum_k bound_k (window_adam_step_ref; 0.2 ulp at lr_pose = 1e-3)
  ... renormalised      RENORM_OPS + 1 ulp on the rotation (window_gn_step_ref), the tangent's share doubled
  pose slots            judged from the device's OWN new nodes: 1 ulp for kind 0 and for a kind-1 target with a zero tangent; KIND1_ULPS - 1
                        = 20 ulp (test_gpu_window_gn_step.py) for a kind-1 target with a tangent; aff slots bitwise
  state                 [0, 1, 3] exact; [5, 10, 11] untouched; loss = [4], [2] and losses[] bitwise on dyadic records (every float64 sum is
                        exact in any order and every weight a power of two), else 1 ulp; [6..9] as doubles to 1e-13 relative
  no update             a frozen call: bitwise everywhere; iteration 0 under skip_first: bitwise but for state[1, 4] (and [2] with rel_tol) and
                        losses[0]
Pinned as it is, and questionable:
  - a kind-0 node with a non-zero tangent is folded in even when no edge names it and lr_pose = 0 (graph shapes, node 6);
  - under abs_loss an edge with r == 0 still decays the moments of everything it touches and so moves those parameters (abs_loss, edge 2);
  - a kind-1 node named as a SOURCE gets the kind-0 source gradient added to its persistent tangent; the header says such a node is only
    ever a target, and no case here makes it a source.

Case -> branch
  test_reduction        n_tiles in {1, 15, 16, 17, 127, 128, 129, 257} (the 16 column groups and the 8 x 16 trip of reduce_columns<16>), 0, 1,
                        7, 8, 9, 17 records per segment (the 8-record trip of the segment loop), N in {1, 255, 256, 257} (thread stride), NaN
                        in column 13
  test_graph_shapes     src_node = -1, a source-and-target node, parallel edges, fixed nodes with and without renormalisation, lr_aff = 0,
                        nodes without an edge, a frozen block between free ones, a block no edge names, weights != 1, one NULL SpPair.aff
  test_kind1            a persistent tangent of norm 0, 1e-3, 0.7 at node 0, 31 (Dual<1> through LDS), 32 (Dual<6>) of 34 and at node 40 of 66
                        (unstaged)
  test_kind1_around_the_series_threshold   a tangent whose rotational theta^2 is 0.5 (1 -+ 2^-20) (se3_exp_times' series | closed forms) and 2, at
                        node 0 and node 32 of 34
  test_fold_in_branches fixed kind-0 nodes with preset tangents of theta^2 = 1e-10, 1e-4 (1 -+ 1e-3) (se3_exp_d's series | closed form), 0.3, 9,
                        from the identity (each entry at 1 ulp of its own magnitude against tests/se3_ref.py) and from general poses
  test_staging_limits   (edges, nodes) = (96, 64) staged | (97, 64), (96, 65) not | (1024, 3); 64 and 66 blocks with their own lr and N in {1,
                        64, 65, 130} (SP_WIN_LDS_BLOCKS, the 4-wave and the 64-lane loops), staged and not; 96x64 and 96x65 agree bitwise
  test_abs_loss_signs   r > 0, < 0, == 0 with and without abs_loss
  test_skip_first_and_counts, test_rel_tol_freeze, test_max_losses   the state machine, records swapped between calls
  test_compose_only     sp_window_compose on the (96, 64) and (97, 64) graphs: nodes untouched, the slots the step leaves
Measured on an MI355X: the 45 tests of this file take 1.5 s (the slowest case 0.4 s, the first launch), 3.4 s with start-up;
the worst distances are printed at the end of the file.
"""
import time

import numpy as np
import pytest
import torch

import window_adam_cases as cases
import window_adam_step_ref as ref
from window_adam_step_ref import f32
from window_gn_step_ref import RENORM_OPS
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

GUARD = 1.0e6
SENTINEL = -5.0
TAIL = 3
KIND1_ULPS = 21          # as in test_gpu_window_gn_step.py
WORST = {}
T0 = time.perf_counter()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"\nworst distance from the reference over the file ({time.perf_counter() - T0:.1f} s): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def note(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def pose_ulps(got16, exp16):
    g, e = np.asarray(got16, f32).reshape(4, 4), np.asarray(exp16, f32).reshape(4, 4)
    assert np.array_equal(g[3], e[3])
    d = np.abs(g[:3].astype(np.float64) - e[:3].astype(np.float64))
    scale = np.maximum(np.abs(e[:3]), 1)
    scale[:, 3] = max(np.abs(e[:3, 3]).max(), 1)
    return d, np.spacing(scale.astype(f32)).astype(np.float64)


class Rig:
    """One window case on the device and its reference state."""

    def __init__(self, case):
        from super_primitive_amd import _lib
        self._lib, self.lib, self.case = _lib, _lib.load(), case
        nodes, edges, blocks = case.nodes, case.edges, case.blocks
        self.n_nodes, self.n_edges, self.n_blocks = len(nodes), len(edges), len(blocks)
        self.Ns = [int(N) for N, _ in blocks]
        self.max_N = max(self.Ns) + 2
        self.args = case.args
        span, seg, self.win = case.window(0)
        self.span_host, self.seg_host = span, seg
        self.span, self.seg = T(span), T(seg)
        sent = np.zeros(1, ref.NODE)
        sent.view(f32)[:] = SENTINEL
        self.sentinel_node = sent
        self.nodes_in = np.array(nodes, ref.NODE)
        self.nodes = T(np.concatenate([self.nodes_in, sent]).view(np.uint8))
        koff = np.cumsum([0] + [N + TAIL for N in self.Ns])
        self.koff = koff
        bufs = []
        for vals in (case.klds, case.bm, case.bv):
            a = np.full(int(koff[-1]), SENTINEL, f32)
            for k, N in enumerate(self.Ns):
                a[koff[k]:koff[k] + N] = vals[k]
            bufs.append(T(a))
        self.kld, self.bm, self.bv = bufs
        self.pose = T(np.full((self.n_edges + 1, 16), SENTINEL, f32))
        self.aff = T(np.full((self.n_edges + 1, 4), SENTINEL, f32))
        self.max_losses = int(self.args.max_losses)
        self.losses = T(np.full(self.max_losses + TAIL, SENTINEL, f32))
        pairs = self.win["pairs"]
        self.sto = T(np.concatenate([p["seg_tile_off"] for p in pairs]).astype(np.int32))
        sto_off = np.cumsum([0] + [p["N"] + 1 for p in pairs])
        parr = (_lib.SpPair * self.n_edges)()
        earr = (_lib.SpWindowEdge * self.n_edges)()
        for e, (edge, q) in enumerate(zip(edges, pairs)):          # pix, src4, kp_L, trg3 stay NULL: the optimiser must not touch them
            d = parr[e]
            d.kld = self.kld.data_ptr() + 4 * int(koff[edge[2]])
            d.pose = self.pose[e].data_ptr()
            d.aff = None if e in case.no_aff else self.aff[e].data_ptr()
            d.seg_tile_off = self.sto.data_ptr() + 4 * int(sto_off[e])
            d.N, d.P, d.tile0, d.n_tiles, d.rec0 = q["N"], q["P"], q["tile0"], q["n_tiles"], q["rec0"]
            earr[e].src_node, earr[e].trg_node, earr[e].block, earr[e].weight = int(edge[0]), int(edge[1]), int(edge[2]), float(edge[3])
        barr = (_lib.SpWindowBlock * self.n_blocks)()
        for k, (N, lr) in enumerate(blocks):
            barr[k].kld, barr[k].m, barr[k].v = (t.data_ptr() + 4 * int(koff[k]) for t in (self.kld, self.bm, self.bv))
            barr[k].N, barr[k].lr = int(N), float(lr)
        self.pairs, self.edges, self.blocks = (T(np.frombuffer(bytes(a), np.uint8).copy()) for a in (parr, earr, barr))
        n = self.lib.sp_window_scratch_doubles(self.n_edges, self.max_N)
        assert n == self.n_edges * (28 + self.max_N)
        self.n_scratch = n
        scratch = np.zeros(n + TAIL)
        scratch[n:] = SENTINEL
        self.scratch = T(scratch)
        self.ref = case.state()
        self.ref["losses"] = np.full(self.max_losses + TAIL, SENTINEL, f32)
        st = np.full(ref.STATE + TAIL, SENTINEL, f32)
        st[:ref.STATE] = self.ref["state"]
        self.state = T(st)
        self.compose()
        got = self.read()
        assert bits(got["nodes"]) == bits(self.nodes_in), "sp_window_compose wrote a node"
        self.check_sentinels(got, "compose")
        assert (got["losses"] == SENTINEL).all() and bits(got["state"][:ref.STATE]) == bits(self.ref["state"])
        self.check_slots(got, "sp_window_compose")
        self.ref["pose"], self.ref["aff"] = got["pose"][:-1].copy(), got["aff"][:-1].copy()

    def compose(self):
        p, L = self._lib.ptr, self._lib
        L.check(self.lib.sp_window_compose(p(self.pairs), p(self.edges), self.n_edges, p(self.nodes), self.n_nodes, L.stream_ptr()), "compose")
        torch.cuda.synchronize()

    def load(self, call):
        span, seg, win = self.case.window(call)
        assert span.shape == self.span_host.shape and seg.shape == self.seg_host.shape
        self.span_host, self.seg_host = span, seg
        self.span.copy_(T(span))
        self.seg.copy_(T(seg))

    def poke(self, k, val):
        self.state[k] = float(val)
        self.ref["state"][k] = val

    def read(self):
        nodes = npy(self.nodes).view(ref.NODE)
        kld, bm, bv = npy(self.kld), npy(self.bm), npy(self.bv)
        cut = lambda a: [a[self.koff[k]:self.koff[k] + N].copy() for k, N in enumerate(self.Ns)]
        return dict(nodes=nodes[:-1].copy(), node_tail=nodes[-1:].copy(), all=(kld, bm, bv), klds=cut(kld), bm=cut(bm), bv=cut(bv),
                    pose=npy(self.pose), aff=npy(self.aff), state=npy(self.state), losses=npy(self.losses),
                    scratch_tail=npy(self.scratch[self.n_scratch:]), span=npy(self.span), seg=npy(self.seg))

    def launch(self):
        p, a, L = self._lib.ptr, self.args, self._lib
        rc = self.lib.sp_window_step(p(self.pairs), p(self.edges), self.n_edges, p(self.nodes), self.n_nodes, p(self.blocks), self.n_blocks,
                                     self.max_N, p(self.span), p(self.seg), p(self.scratch), int(a.abs_loss), int(a.skip_first), float(a.rel_tol),
                                     p(self.state), p(self.losses), self.max_losses, L.stream_ptr())
        L.check(rc, "sp_window_step")
        torch.cuda.synchronize()

    def run(self):
        """Every call of the case; returns the decisions."""
        out = []
        for call in range(len(self.case.calls)):
            if call:
                self.load(call)
            for k, val in self.case.pokes.get(call, {}).items():
                self.poke(k, val)
            out.append(self.step(f"{self.case.name} call {call}")["decision"])
        return out

    def step(self, what=""):
        """Launch once, compare everything with the reference, let the reference continue from the device's values.  Returns ``info``."""
        info, before = {}, self.ref
        want = ref.window_adam_step_ref(self.span_host, self.seg_host, self.win, before, self.args, info)
        self.launch()
        got = self.read()
        tag = f"{what} ({info['decision']})"
        self.check_sentinels(got, tag)
        self.check_state(got, want, before, info, tag)
        if info["decision"] == "step":
            self.check_blocks(got, before, info, tag)
            self.check_nodes(got, want, before, info, tag)
            self.check_slots(got, tag)
        else:
            for k in ("nodes", "pose", "aff"):
                assert bits(got[k][:len(before[k])]) == bits(before[k]), f"{tag}: {k} moved"
            for k in ("klds", "bm", "bv"):
                assert all(bits(a) == bits(b) for a, b in zip(got[k], before[k])), f"{tag}: {k} moved"
        self.ref = dict(nodes=got["nodes"], klds=got["klds"], bm=got["bm"], bv=got["bv"], pose=got["pose"][:-1].copy(), aff=got["aff"][:-1].copy(),
                        state=got["state"][:ref.STATE].copy(), losses=got["losses"].copy())
        return info

    def check_sentinels(self, got, tag):
        assert bits(got["span"]) == bits(self.span_host) and bits(got["seg"]) == bits(self.seg_host), f"{tag}: records written"
        assert bits(got["node_tail"]) == bits(self.sentinel_node), f"{tag}: the node behind n_nodes"
        for a in got["all"]:
            for k, N in enumerate(self.Ns):
                assert (a[self.koff[k] + N:self.koff[k + 1]] == SENTINEL).all(), f"{tag}: tail of block {k}"
        assert (got["pose"][-1] == SENTINEL).all() and (got["aff"][-1] == SENTINEL).all(), f"{tag}: slot tails"
        for e in self.case.no_aff:
            assert (got["aff"][e] == SENTINEL).all(), f"{tag}: the aff slot of edge {e}, whose SpPair.aff is NULL"
        assert (got["losses"][self.max_losses:] == SENTINEL).all() and (got["state"][ref.STATE:] == SENTINEL).all(), f"{tag}: losses / state tail"
        assert (got["scratch_tail"] == SENTINEL).all(), f"{tag}: scratch tail"

    def check_state(self, got, want, before, info, tag):
        s, ws, bs = got["state"][:ref.STATE], want["state"], before["state"]
        if info["decision"] == "frozen":
            assert bits(s) == bits(bs) and bits(got["losses"]) == bits(before["losses"]), f"{tag}: a frozen call wrote state or losses"
            return
        for k in (0, 1, 3):
            assert s[k] == ws[k], f"{tag}: state[{k}] {s[k]} != {ws[k]}"
        assert bits(s[[5, 10, 11]]) == bits(bs[[5, 10, 11]]), f"{tag}: state[5, 10, 11] written"
        if not float(self.args.rel_tol) > 0:
            assert bits(s[2:3]) == bits(bs[2:3]), f"{tag}: state[2] written without rel_tol"
        pairs = [(f"state[{k}]", s[k], ws[k]) for k in (2, 4)] + [(f"losses[{i}]", a, b) for i, (a, b) in enumerate(zip(got["losses"], want["losses"]))]
        for name, a, b in pairs:
            d = abs(float(a) - float(b)) / np.spacing(abs(b))
            note("loss (ulp)", d)
            assert d <= (0 if self.case.exact else 1), f"{tag}: {name} {a!r} != {b!r} ({d:.3g} ulp)"
        gp, wp = ref.running_products(s), ref.running_products(ws)
        d = np.abs(gp - wp) / wp
        note("beta^t (relative)", d.max())
        assert (d <= 1e-13).all(), f"{tag}: running products {gp} != {wp}"
        if info["decision"] == "skipped":
            assert bits(np.delete(s, [1, 2, 4])) == bits(np.delete(bs, [1, 2, 4])) and bits(got["losses"][1:]) == bits(before["losses"][1:]), tag

    def adam(self, name, tag, ent, p, m, v):
        """One Adam application against its entry of ``info``: parameter (None = folded away), m, v within adam_bound."""
        for what, a, b, bound in (("parameter", p, ent["p"], ent["b_p"]), ("m", m, ent["m"], ent["b_m"]), ("v", v, ent["v"], ent["b_v"])):
            if a is None:
                continue
            d = np.abs(np.asarray(a, np.float64) - b)
            note(f"{name} {what} / adam_bound", (d / np.where(bound > 0, bound, 1)).max())
            if what == "parameter":
                note(f"{name} parameter / lr", d.max() / ent["lr"])
            assert (d <= bound).all(), f"{tag}: {name} {what} off by {d.max():.3g}, bound {np.ravel(bound)[d.argmax()]:.3g}"

    def check_blocks(self, got, before, info, tag):
        for b in range(self.n_blocks):
            if ("kld", b) in info:
                self.adam("kld", f"{tag} block {b}", info[("kld", b)], got["klds"][b], got["bm"][b], got["bv"][b])
            else:
                for k in ("klds", "bm", "bv"):
                    assert bits(got[k][b]) == bits(before[k][b]), f"{tag}: {k} of block {b}, which takes no step"

    def check_nodes(self, got, want, before, info, tag):
        for i in range(self.n_nodes):
            g, w, b = got["nodes"][i], want["nodes"][i], before["nodes"][i]
            nt = f"{tag} node {i}"
            for field in ("lr_pose", "lr_aff", "kind", "flags"):
                assert g[field] == b[field], f"{nt}: {field}"
            if ("a", i) in info:
                self.adam("tangent" if b["kind"] == 1 else "kind-0 tangent", nt, info[("a", i)], g["a"] if b["kind"] == 1 else None, g["m"], g["v"])
            else:
                assert bits(g["m"]) == bits(b["m"]) and bits(g["v"]) == bits(b["v"]), f"{nt}: pose moments of a node that takes no step"
                if b["kind"] == 1:
                    assert bits(g["a"]) == bits(b["a"]), f"{nt}: tangent"
            if ("aff", i) in info:
                self.adam("aff", nt, info[("aff", i)], g["aff"], g["aff_m"], g["aff_v"])
            else:
                assert all(bits(g[f]) == bits(b[f]) for f in ("aff", "aff_m", "aff_v")), f"{nt}: affine part of a node that takes no step"
            if b["kind"] == 1:
                assert bits(g["T"]) == bits(b["T"]), f"{nt}: the group element of a kind-1 node"
                continue
            assert not g["a"].any(), f"{nt}: tangent not reset"
            renorm = bool(b["flags"] & 1)
            if not renorm and ("a", i) not in info and not b["a"].any():
                assert bits(g["T"]) == bits(b["T"]), f"{nt}: pose of a node that neither folds nor renormalises"
                continue
            d, sp = pose_ulps(g["T"], w["T"])
            allowed = sp.copy()
            allowed[:, :3] *= (RENORM_OPS + 1) if renorm else 1
            allowed = allowed + info.get(("T", i), 0.0) * (2 if renorm else 1)
            name = "T renormalised" if renorm else "T"
            note(name + " (ulp)", (d / sp).max())
            assert (d <= allowed).all(), f"{nt}: {name} off by {(d / sp).max():.3g} ulp (allowed {(allowed / sp).max():.3g})"

    def check_slots(self, got, tag):
        """Every edge's pose and aff slot, judged from the device's own nodes."""
        for e, edge in enumerate(self.win["edges"]):
            P, af = ref.compose_edge(edge, got["nodes"])
            if e not in self.case.no_aff:
                assert bits(got["aff"][e]) == bits(af), f"{tag}: aff slot {e}"
            nt = got["nodes"][edge[1]]
            kind1 = nt["kind"] == 1 and nt["a"].any()
            d, sp = pose_ulps(got["pose"][e], P)
            note("pose slot, kind 1 (ulp)" if kind1 else "pose slot (ulp)", (d / sp).max())
            assert (d <= sp * (KIND1_ULPS - 1 if kind1 else 1)).all(), f"{tag}: pose slot {e} off by {(d / sp).max():.3g} ulp"


def shared(rig, n_nodes):
    r = rig.ref
    return [bits(r["nodes"][:n_nodes])] + [bits(x) for k in ("klds", "bm", "bv") for x in r[k]] + [bits(r[k]) for k in ("pose", "aff", "state", "losses")]


@pytest.mark.parametrize("n_tiles", cases.REDUCTION_TILES)
def test_reduction(n_tiles):
    assert Rig(cases.reduction_case(n_tiles)).run() == ["step"]


def test_graph_shapes():
    rig = Rig(cases.graph_shapes_case())
    start = rig.ref
    assert rig.run() == ["step"] * 3
    end = rig.ref
    assert bits(end["klds"][1]) == bits(start["klds"][1]) and bits(end["klds"][3]) == bits(start["klds"][3])
    assert bits(end["nodes"][6]["T"]) != bits(start["nodes"][6]["T"]), "the idle fixed node's tangent was not folded in"
    assert bits(end["nodes"][4]) == bits(start["nodes"][4]) and bits(end["nodes"][5]["aff"]) == bits(start["nodes"][5]["aff"])


@pytest.mark.parametrize("norm,idx,n_nodes", cases.KIND1)
def test_kind1(norm, idx, n_nodes):
    rig = Rig(cases.kind1_case(norm, idx, n_nodes))
    a0 = rig.ref["nodes"][idx]["a"].copy()
    assert rig.run() == ["step"] * 2
    assert (rig.ref["nodes"][idx]["a"] != a0).all(), "the persistent tangent did not move"


@pytest.mark.parametrize("theta2,idx,n_nodes", cases.KIND1_THETA2)
def test_kind1_around_the_series_threshold(theta2, idx, n_nodes):
    """se3_exp_times on either side of theta^2 = 0.5 and at 2, on Dual<1> (the slots) and Dual<6> (the gradient), with test_kind1's bounds."""
    rig = Rig(cases.kind1_case(0.3, idx, n_nodes, theta2))
    a0 = rig.ref["nodes"][idx]["a"].copy()
    assert ((a0[3:] * a0[3:]).sum(dtype=f32) < 0.5) == (theta2 == "0.5-")
    assert rig.run() == ["step"] * 2
    assert (rig.ref["nodes"][idx]["a"] != a0).all(), "the persistent tangent did not move"


@pytest.mark.parametrize("identity", [1, 0], ids=["identity", "general"])
def test_fold_in_branches(identity):
    """se3_exp_d in its series and in its closed form.  The rig holds every new T to 1 ulp at max(|entry|, 1) of the yardstick; from the
    identity the new T is Exp(-a) itself and every entry is held to FOLD_ULPS = 1 ulp of its OWN magnitude against se3_ref.exp_se3 (scipy's
    expm, no branch on theta): a wrong series coefficient is not hidden under a unit-size entry."""
    import se3_ref
    rig = Rig(cases.fold_in_case(identity))
    start = rig.ref["nodes"].copy()
    assert rig.run() == ["step"]
    twists = se3_ref.fold_in_twists()
    assert {bool((a[3:] ** 2).sum() < 1e-4) for _, a in twists} == {True, False}
    for k, (name, a) in enumerate(twists):
        nd, nd0 = rig.ref["nodes"][2 + k], start[2 + k]
        assert bits(nd0["a"]) == bits(a.astype(f32)) and not nd["a"].any() and nd["lr_pose"] == 0
        want = nd0["T"].astype(np.float64).reshape(4, 4) @ se3_ref.exp_se3(-nd0["a"].astype(np.float64))
        got = nd["T"].reshape(4, 4)
        assert bits(got[3]) == bits(nd0["T"][12:])
        if identity:
            d = se3_ref.own_ulps(got[:3], want[:3]).max()
            note("fold-in from the identity (ulp of the entry)", d)
            assert d <= se3_ref.FOLD_ULPS, f"{name}: {d:.3g} ulp of the entry's own magnitude from Exp(-a)"
        else:
            d, sp = pose_ulps(got, want.astype(f32))
            assert (d <= sp).all(), name


@pytest.mark.parametrize("which", cases.STAGING)
def test_staging_limits(which):
    rig = Rig(cases.staging_case(which))
    assert rig.run() == ["step"]
    if which == "96x65":          # the same graph staged in LDS: bit for bit
        staged = Rig(cases.staging_case("96x64"))
        staged.run()
        assert shared(staged, 64) == shared(rig, 64), "the staged and the unstaged instantiation differ on the same window"


@pytest.mark.parametrize("abs_loss", [1, 0])
def test_abs_loss_signs(abs_loss):
    rig = Rig(cases.abs_loss_case(abs_loss))
    start = rig.ref
    info = rig.step(f"abs_loss={abs_loss} call 0")
    r = info["grads"]["r"]
    assert r[0] > 0 and r[1] < 0 and r[2] == 0 and info["grads"]["c"].tolist() == ([1.0, -2.0, 0.0] if abs_loss else [1.0, 2.0, 1.0])
    if abs_loss:          # the edge with r == 0 gives no gradient, and yet its nodes and block decay their moments
        assert not info[("a", 3)]["g"].any() and not info[("kld", 2)]["g"].any()
        assert (np.abs(rig.ref["nodes"][3]["m"]) < np.abs(start["nodes"][3]["m"])).all() and (rig.ref["bv"][2] < start["bv"][2]).all()
    rig.step(f"abs_loss={abs_loss} call 1")


def test_skip_first_and_counts():
    rig = Rig(cases.skip_first_case())
    assert rig.run() == ["skipped", "step", "step", "step"]
    s = rig.ref["state"]
    assert (s[0], s[1]) == (1, 4) and np.array_equal(ref.running_products(s), [0.9, 0.999]) and rig.ref["nodes"]["m"].any()
    assert rig.ref["losses"][0] == rig.ref["losses"][1]


@pytest.mark.parametrize("rel_tol", [1e-2, 0.0])
def test_rel_tol_freeze(rel_tol):
    rig = Rig(cases.rel_tol_case(rel_tol))
    if rel_tol:
        assert rig.run() == ["step", "step", "step", "frozen", "frozen"]
        assert rig.ref["state"][3] == 1 and rig.ref["state"][1] == 3 and rig.ref["state"][0] == 40
    else:
        assert rig.run() == ["step"] * 3 and rig.ref["state"][2] == 123.0 and rig.ref["state"][3] == 0


@pytest.mark.parametrize("max_losses", [0, 2])
def test_max_losses(max_losses):
    rig = Rig(cases.max_losses_case(max_losses))
    assert rig.run() == ["step"] * 4
    assert rig.ref["state"][1] == 4 and (rig.ref["losses"][max_losses:] == SENTINEL).all() and (rig.ref["losses"][:max_losses] != SENTINEL).all()


@pytest.mark.parametrize("which", ["96x64", "97x64"])
def test_compose_only(which):
    rig = Rig(cases.staging_case(which))          # (the constructor composes, checks every slot and that no node moved)
    rig.run()
    left = rig.read()
    rig.pose.fill_(SENTINEL)
    rig.aff.fill_(SENTINEL)
    rig.compose()
    got = rig.read()
    assert bits(got["nodes"]) == bits(left["nodes"]) and bits(got["pose"]) == bits(left["pose"]) and bits(got["aff"]) == bits(left["aff"])
    assert bits(got["state"]) == bits(left["state"]) and all(bits(a) == bits(b) for a, b in zip(got["all"], left["all"]))
    rig.check_sentinels(got, "compose after a step")
