"""-m gpu: ONE call of the window Gauss-Newton / LM solver (sp_window_gn_step: k_window_gn_reduce, k_window_gn_schur and the four
instantiations of k_window_gn_update in csrc/sp_window_gn.hip) against the float64 dense solve of tests/window_gn_step_ref.py.

The call reads only the partial records, a few SpPair fields and the node / edge / block arrays, so everything is hand-made (no image, no
table, no cost pass).  Rig: guard records valued 1e6 in front of and behind every edge's span and segment records (tile0, rec0 > 0); kld
slots, kld_backup, losses, the pose / aff slots and the scratch with sentinel tails; one sentinel node behind n_nodes in nodes and
nodes_backup; the pose slots initialised by sp_window_compose.  After every call EVERY buffer the call may write is compared -- nodes
(whole struct), every block's kld, both backups, every edge's pose and aff slot, state[0..15], losses, all sentinels and guards -- and the
reference continues from the DEVICE's values, so each call is judged from identical inputs.

Bounds (derived, not tuned).  The device solves in float64 and rounds once to float32; every stepped system's dense damped matrix is
asserted to have a condition number <= 1e6, so both float64 solves are good to ~1e-9 relative, far below a float32 ulp.  Hence
  kld, aff      2 ulp: one for the cast of the step, one for the add -- taken at the larger of |step| and |result| (the cast rounds at the
                step's scale, the add at the result's);
  T, kind 0     no renormalisation: a float64 product rounded once = 1 ulp at max(|entry|, 1) for the rotation, max(|t|, 1) for the
                translation.  With renormalisation (flags bit 0 of the node): the restated float32 routine has 19 operations on its longest
                path (3 adds + sqrt; q * q or a difference; the division by den; s = 4 products, 3 adds, 1 division; an entry = 2 products,
                an add, a product, a subtraction), one ulp each at scale 1, + 1 for its input: 20 ulp at 1 on the rotation;
  T, kind 1     X <- Exp(d) Exp(a) X where the device forms Exp(a) X in FLOAT32 (se3_exp_times, the routine the cost pass's pose comes
                from): per entry of E = I + A W + B W^2, 2 casts + 5 roundings of W^2 + 2 products + 2 adds = 11 half-ulps at scale <= 1,
                three such entries times |X| <= scale and 5 roundings of the 3-term product sum (7 with the translation's 4 terms + V t):
                (3 * 11 + 7) / 2 = 20 ulp at max(|X|, 1), + 1 for the final cast: 21 ulp.  The same 20 for the pose slot of a kind-1 target
                whose tangent is not zero.  With a ZERO tangent (every call after the first step, which clears it) Exp(0) X is exact in
                float32 (W = 0, E = I, 1 * x + 0 + 0) and the kind-0 bound applies: 1 ulp;
  pose slots    judged from the device's OWN new nodes (so the node bound does not compound): a float64 product rounded once, 1 ulp at
                max(|entry|, 1) / max(|t|, 1); aff slots bitwise;
  state         [0, 2, 3, 4, 5, 6, 8, 9] exact, [10..15] untouched; losses and state[1, 7] bitwise where the records are dyadic (every
                float64 sum exact in any order), otherwise 1 ulp;
  no step       (frozen, converged, too many unknowns) bitwise everywhere; a reject restores nodes and log-depths bitwise from the backups
                and re-composes the slots (the slot bound); a failed factorisation moves state[0, 1, 4, 5, 7, 8], losses and the backups.
Pinned as it is, and questionable: a failed factorisation leaves state[1] = this call's loss and the backups = this point although no step
was accepted (harmless: the next call may neither reject nor converge), and it moves NO log-depth, unlike the per-pair solver, whose
depths take their own Newton step when the pose block fails.

Case -> branch
  test_camera_sizes          n_y = 0 (the 'supp' diagonal solve), 2, 6, 8, 62, 64 | 66, 78 (last block of two pivots), 126, 128 | 130, 190,
                             192 | 194, 254, 512 (64 nodes; one block's list exactly 64 edges; nc = 512 with N = 33: C chunks of 8192 / 512 = 16 rows,
                             three of them -- 16 x 512 fills the staging buffer exactly -- the last of one row)
  test_oversized_n_unknowns  n_y = 40 under n_unknowns = 40, 128, 192, 256: identity padding, all four bitwise equal in nodes and kld
  test_graph_shapes          src_node = -1, kind-1 target with a tangent, source-and-target node, parallel edges, a fixed node in the middle,
                             a frozen block between free ones, a block that meets fixed nodes only (nc = 0), renormalisation
  test_schur_rows            block N in {1, 255, 256, 257, 511, 512, 513} (thread stride, SP_WGN_SCHUR_ROWS)
  test_schur_two_chunks      nc = 56, N = 147: two C chunks of 8192 / 56 = 146 rows, 1596 pairs = 4 tiles
  test_frozen_rows           a segment without records, one with D (1 + lambda) = 5e-13, clamps at +0.5 and -0.5
  test_block_edge_list       64 edges of one block (the list exactly full), 65 (the walk over all edges)
  test_back_substitution     N across NTHR / 4 rows per trip of every instantiation
  test_reduction             n_tiles in {1, 4, 5, 6, 11} (the five column groups of reduce_columns<48>), 0..9 records per segment
  test_inline_reduce         flags bit 2 with 4 edges (reduced inside the update kernel) and 5 (separate launch)
  test_pose_only_flag        flags bit 0 with free blocks: the depths stay and the cameras step.  kld_backup is NOT left untouched: every step
                             call copies the (unmoved) log-depths into it, whatever the flags -- pinned as the device does it
  test_predicted_exit        flags bit 1 at lambda = 1e-4 (freezes), at 0.1 (does not), after a failed factorisation (does not)
  test_accept_reject_accept  the LM machine, record contents swapped between calls
  test_converged_ignores     a converged window ignores three further calls
  test_failed_factorisation  a negative lambda; which of state[2, 3, 4, 8] move
  test_too_many_unknowns     n_unknowns smaller than the window's own: state[9], state[6], nothing else
  test_max_losses            losses[] stops at max_losses, state[5] goes on
"""
import ctypes

import numpy as np
import pytest
import torch

import window_gn_step_ref as ref
from window_gn_step_ref import WinArgs, f32
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

GUARD = 1.0e6
SENTINEL = -5.0
TAIL = 3
KIND1_ULPS = 21
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst distance from the reference over the file (ulp): " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))


def ulps(got, exp, scale):
    return np.abs(np.asarray(got, np.float64) - np.asarray(exp, np.float64)) / np.spacing(np.asarray(scale, f32)).astype(np.float64)


def pose_ulps(got16, exp16):
    """Distance of two 4x4 poses in ulp at max(|entry|, 1) (rotation) / max(|t|, 1) (translation); the last row must be equal."""
    g, e = np.asarray(got16, f32).reshape(4, 4), np.asarray(exp16, f32).reshape(4, 4)
    assert np.array_equal(g[3], e[3])
    rot = ulps(g[:3, :3], e[:3, :3], np.maximum(np.abs(e[:3, :3]), 1)).max()
    tr = ulps(g[:3, 3], e[:3, 3], np.full(3, max(np.abs(e[:3, 3]).max(), 1))).max()
    return float(rot), float(tr)


class Rig:
    """One window on the device and its reference state.  nodes: list of ref.make_node; edges: (src_node, trg_node, block, weight);
    blocks: (N, lr); recs: one ref.make_window_records per edge.  ``load`` swaps the record CONTENTS."""

    def __init__(self, nodes, edges, blocks, recs, klds, lam0=2.0, n_unknowns=None, max_losses=6, **args):
        from super_primitive_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.n_nodes, self.n_edges, self.n_blocks = len(nodes), len(edges), len(blocks)
        self.Ns = [int(N) for N, _ in blocks]
        self.sum_N, self.max_N = sum(self.Ns), max(self.Ns) + 2
        ny = ref.number_unknowns(nodes)[2]
        self.args = WinArgs(n_unknowns=ny if n_unknowns is None else n_unknowns, max_losses=max_losses, **args)
        for e, r in zip(edges, recs):
            assert r["pair"]["N"] == self.Ns[e[2]]
        span, seg, pairs = ref.lay_out(recs, GUARD)
        self.win = dict(edges=list(edges), blocks=list(blocks), pairs=pairs)
        self.span_host, self.seg_host = span, seg
        self.span, self.seg = T(span), T(seg)
        sent = np.zeros((), ref.NODE)
        sent.reshape(1).view(f32)[:] = SENTINEL
        self.sentinel_node = sent
        self.nodes = T(np.concatenate([np.array(nodes, ref.NODE), sent.reshape(1)]).view(np.uint8))
        self.nodes_backup = T(np.full((self.n_nodes + 1) * 44, SENTINEL, f32))
        koff = np.cumsum([0] + [N + TAIL for N in self.Ns])
        kld = np.full(int(koff[-1]), SENTINEL, f32)
        for k, N in enumerate(self.Ns):
            kld[koff[k]:koff[k] + N] = klds[k]
        self.koff, self.kld = koff, T(kld)
        self.kld_backup = T(np.full(self.sum_N + TAIL, SENTINEL, f32))
        self.pose = T(np.full((self.n_edges + 1, 16), SENTINEL, f32))
        self.aff = T(np.full((self.n_edges + 1, 4), SENTINEL, f32))
        self.losses = T(np.full(max_losses + TAIL, SENTINEL, f32))
        st = np.zeros(ref.STATE + TAIL, f32)
        st[0], st[1], st[ref.STATE:] = lam0, -1.0, SENTINEL
        self.state = T(st)
        self.sto = T(np.concatenate([p["seg_tile_off"] for p in pairs]).astype(np.int32))
        sto_off = np.cumsum([0] + [p["N"] + 1 for p in pairs])
        parr = (_lib.SpPair * self.n_edges)()
        earr = (_lib.SpWindowEdge * self.n_edges)()
        for e, (edge, q) in enumerate(zip(edges, pairs)):          # pix, src4, kp_L, trg3 stay NULL: the solver must not touch them
            d = parr[e]
            d.kld = self.kld.data_ptr() + 4 * int(koff[edge[2]])
            d.pose, d.aff = self.pose[e].data_ptr(), self.aff[e].data_ptr()
            d.seg_tile_off = self.sto.data_ptr() + 4 * int(sto_off[e])
            d.N, d.P, d.tile0, d.n_tiles, d.rec0 = q["N"], q["P"], q["tile0"], q["n_tiles"], q["rec0"]
            earr[e].src_node, earr[e].trg_node, earr[e].block, earr[e].weight = int(edge[0]), int(edge[1]), int(edge[2]), float(edge[3])
        barr = (_lib.SpWindowBlock * self.n_blocks)()
        for k, (N, lr) in enumerate(blocks):                      # m, v (Adam moments) stay NULL
            barr[k].kld, barr[k].N, barr[k].lr = self.kld.data_ptr() + 4 * int(koff[k]), int(N), float(lr)
        self.pairs, self.edges, self.blocks = (T(np.frombuffer(bytes(a), np.uint8).copy()) for a in (parr, earr, barr))
        n = self.lib.sp_window_gn_scratch_doubles(self.n_edges, self.n_blocks, self.sum_N, self.max_N, int(self.args.n_unknowns))
        assert n > 0
        self.n_scratch = n
        scratch = np.zeros(n + TAIL)
        scratch[n:] = SENTINEL
        self.scratch = T(scratch)
        p = _lib.ptr
        _lib.check(self.lib.sp_window_compose(p(self.pairs), p(self.edges), self.n_edges, p(self.nodes), self.n_nodes, _lib.stream_ptr()), "compose")
        torch.cuda.synchronize()
        self.ref = ref.new_state(nodes, klds, npy(self.pose)[:-1], npy(self.aff)[:-1], lam0=lam0, losses_len=max_losses + TAIL, sentinel=SENTINEL)
        for e, edge in enumerate(edges):                          # the slots sp_window_compose left, against the reference's compose
            P, af = ref.compose_edge(edge, self.ref["nodes"])
            assert np.array_equal(self.ref["aff"][e], af)
            nt = nodes[edge[1]]
            bound = KIND1_ULPS - 1 if nt["kind"] == 1 and nt["a"].any() else 1
            assert max(pose_ulps(self.ref["pose"][e], P)) <= bound, f"sp_window_compose, edge {e}"

    def load(self, recs):
        span, seg, pairs = ref.lay_out(recs, GUARD)
        assert span.shape == self.span_host.shape and seg.shape == self.seg_host.shape
        self.span_host, self.seg_host = span, seg
        self.span.copy_(T(span))
        self.seg.copy_(T(seg))

    def read(self):
        nodes = npy(self.nodes).view(ref.NODE)
        kld = npy(self.kld)
        return dict(nodes=nodes[:-1].copy(), node_tail=nodes[-1:].copy(), nodes_backup=npy(self.nodes_backup).view(ref.NODE)[:-1].copy(),
                    backup_tail=npy(self.nodes_backup)[-44:].copy(), kld_all=kld,
                    klds=[kld[self.koff[k]:self.koff[k] + N].copy() for k, N in enumerate(self.Ns)], kld_backup=npy(self.kld_backup),
                    pose=npy(self.pose), aff=npy(self.aff), state=npy(self.state), losses=npy(self.losses),
                    scratch_tail=npy(self.scratch[self.n_scratch:]), span=npy(self.span), seg=npy(self.seg))

    def launch(self):
        p, a = self._lib.ptr, self.args
        rc = self.lib.sp_window_gn_step(p(self.pairs), p(self.edges), self.n_edges, p(self.nodes), self.n_nodes, p(self.blocks), self.n_blocks,
                                        self.sum_N, self.max_N, int(a.n_unknowns), p(self.span), p(self.seg), p(self.scratch), p(self.nodes_backup),
                                        p(self.kld_backup), int(a.flags), float(a.lm_up), float(a.lm_down), float(a.lm_min), float(a.conv_tol),
                                        p(self.state), p(self.losses), int(a.max_losses), self._lib.stream_ptr())
        self._lib.check(rc, "sp_window_gn_step")
        torch.cuda.synchronize()

    def step(self, exact=True, what=""):
        """Launch once, compare everything with the reference, let the reference continue from the device's values.  Returns ``info``."""
        info = {}
        before = self.ref
        want = ref.window_gn_step_ref(self.span_host, self.seg_host, self.win, before, self.args, info)
        self.launch()
        got = self.read()
        c = Compared(tag=f"{what} ({info['decision']})", dec=info["decision"], info=info, before=before, want=want, got=got, exact=exact, worst={})
        self.check_sentinels(c)
        self.check_state(c)
        self.check_backups(c)
        self.check_klds(c)
        self.check_nodes(c)
        self.check_slots(c)
        print(f"{c.tag}: n_y {info['n_y']}" + (f", cond {info['cond']:.3g}, lambda {info['lam']:.3g}" if "cond" in info else "") +
              "; worst (ulp) " + ", ".join(f"{k} {v:.3g}" for k, v in c.worst.items()))
        # the reference goes on from what the device holds
        self.ref = dict(nodes=got["nodes"], klds=got["klds"], nodes_backup=got["nodes_backup"], kld_backup=got["kld_backup"][:self.sum_N].copy(),
                        pose=got["pose"][:-1].copy(), aff=got["aff"][:-1].copy(), state=got["state"][:ref.STATE].copy(), losses=got["losses"].copy())
        return info

    def check_sentinels(self, c):
        """Guard records, the sentinel node, every tail: untouched, whatever the call decided."""
        got, tag = c.got, c.tag
        assert np.array_equal(got["span"].view(np.uint32), self.span_host.view(np.uint32)), f"{tag}: span records written"
        assert np.array_equal(got["seg"].view(np.uint32), self.seg_host.view(np.uint32)), f"{tag}: segment records written"
        assert np.array_equal(got["node_tail"], self.sentinel_node.reshape(1)) and (got["backup_tail"] == SENTINEL).all(), f"{tag}: node sentinels"
        for k, N in enumerate(self.Ns):
            assert (got["kld_all"][self.koff[k] + N:self.koff[k + 1]] == SENTINEL).all(), f"{tag}: kld tail of block {k}"
        assert (got["kld_backup"][self.sum_N:] == SENTINEL).all() and (got["pose"][-1] == SENTINEL).all() and (got["aff"][-1] == SENTINEL).all(), tag
        assert (got["losses"][int(self.args.max_losses):] == SENTINEL).all() and (got["state"][ref.STATE:] == SENTINEL).all(), tag
        assert (got["scratch_tail"] == SENTINEL).all(), f"{tag}: scratch tail"

    def check_state(self, c):
        """cond <= 1e6 of a stepped system; counters, flags and lambda exact; losses and state[1, 7] bitwise on dyadic records, else 1 ulp."""
        tag = c.tag
        if c.dec == "step":
            assert c.info["cond"] <= 1e6, f"{tag}: condition number {c.info['cond']:.3g}"
        s, ws = c.got["state"], c.want["state"]
        for k in (0, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15):
            assert s[k] == ws[k], f"{tag}: state[{k}] {s[k]} != {ws[k]}"
        pairs = [(f"state[{k}]", s[k], ws[k]) for k in (1, 7)]
        pairs += [(f"losses[{i}]", a, b) for i, (a, b) in enumerate(zip(c.got["losses"], c.want["losses"]))]
        for name, a, b in pairs:
            d = abs(float(a) - float(b)) / np.spacing(abs(b))
            c.note("loss", d)
            assert d <= (0 if c.exact else 1), f"{tag}: {name} {a!r} != {b!r} ({d:.3g} ulp)"

    def check_backups(self, c):
        """Bitwise: the point left by a call that backs up, untouched otherwise."""
        assert np.array_equal(c.got["nodes_backup"].view(np.uint32), c.want["nodes_backup"].view(np.uint32)), f"{c.tag}: nodes_backup"
        assert np.array_equal(c.got["kld_backup"][:self.sum_N].view(np.uint32), c.want["kld_backup"].view(np.uint32)), f"{c.tag}: kld_backup"

    def check_klds(self, c):
        """A step: 2 ulp at the larger of |step| and |result| on active rows, bitwise on the others; any other call: bitwise."""
        got, want, info, tag = c.got, c.want, c.info, c.tag
        off = 0
        for k, N in enumerate(self.Ns):
            if c.dec == "step" and N:
                active = info["active"][off:off + N]
                scale = np.maximum(np.maximum(np.abs(want["klds"][k]), np.abs(info["dd"][off:off + N]).astype(f32)), f32(1e-30))
                d = ulps(got["klds"][k], want["klds"][k], scale)
                d[~active] = np.where(got["klds"][k] == c.before["klds"][k], 0, np.inf)[~active]
                c.note("kld", d.max())
                assert d.max() <= 2, f"{tag}: kld of block {k} off by {d.max():.3g} ulp at {d.argmax()}"
            else:
                assert np.array_equal(got["klds"][k].view(np.uint32), want["klds"][k].view(np.uint32)), f"{tag}: kld of block {k}"
            off += N

    def check_nodes(self, c):
        """A step: aff 2 ulp, T by kind (see the bounds above), every other field of the struct bitwise; any other call: the whole struct bitwise."""
        info, tag = c.info, c.tag
        pose_off, aff_off, _ = ref.number_unknowns(c.before["nodes"])
        for i in range(self.n_nodes):
            g, w, b = c.got["nodes"][i], c.want["nodes"][i], c.before["nodes"][i]
            if c.dec != "step":
                assert g.tobytes() == w.tobytes(), f"{tag}: node {i}"
                continue
            for field in ("m", "v", "aff_m", "aff_v", "lr_pose", "lr_aff", "kind", "flags"):
                assert np.array_equal(g[field], b[field]), f"{tag}: node {i} field {field}"
            assert np.array_equal(g["a"], w["a"]), f"{tag}: node {i} tangent"
            if aff_off[i] >= 0:
                dy = info["dy"][aff_off[i]:aff_off[i] + 2]
                d = ulps(g["aff"], w["aff"], np.maximum(np.maximum(np.abs(w["aff"]), np.abs(dy).astype(f32)), f32(1e-30))).max()
                c.note("aff", d)
                assert d <= 2, f"{tag}: node {i} aff off by {d:.3g} ulp"
            else:
                assert np.array_equal(g["aff"], b["aff"]), f"{tag}: node {i} aff (fixed)"
            if pose_off[i] < 0:
                assert np.array_equal(g["T"], b["T"]), f"{tag}: node {i} pose (fixed)"
                continue
            rot, tr = pose_ulps(g["T"], w["T"])
            if b["kind"] == 1 and b["a"].any():
                name, bound_r, bound_t = "T kind 1", KIND1_ULPS, KIND1_ULPS
            elif b["kind"] == 1:                       # Exp(0) X is exact in float32
                name, bound_r, bound_t = "T kind 1, zero tangent", 1, 1
            elif b["flags"] & 1:
                name, bound_r, bound_t = "T renormalised", ref.RENORM_OPS + 1, 1
            else:
                name, bound_r, bound_t = "T", 1, 1
            c.note(name + " rot", rot)
            c.note(name + " t", tr)
            assert rot <= bound_r and tr <= bound_t, f"{tag}: node {i} ({name}) off by {rot:.3g} / {tr:.3g} ulp"

    def check_slots(self, c):
        """Every edge's pose and aff slot: bitwise after a call that does not compose, else judged from the device's own new nodes."""
        got, tag = c.got, c.tag
        for e, edge in enumerate(self.win["edges"]):
            if c.dec in ("frozen", "converged", "too_many"):
                assert np.array_equal(got["pose"][e].view(np.uint32), c.before["pose"][e].view(np.uint32)), f"{tag}: pose slot {e}"
                assert np.array_equal(got["aff"][e].view(np.uint32), c.before["aff"][e].view(np.uint32)), f"{tag}: aff slot {e}"
                continue
            P, af = ref.compose_edge(edge, got["nodes"])
            assert np.array_equal(got["aff"][e], af), f"{tag}: aff slot {e}"
            nt = got["nodes"][edge[1]]
            d = max(pose_ulps(got["pose"][e], P))
            c.note("pose slot", d)
            assert d <= (KIND1_ULPS - 1 if nt["kind"] == 1 and nt["a"].any() else 1), f"{tag}: pose slot {e} off by {d:.3g} ulp"


class Compared:
    """One compared call: the decision, the states before / wanted / got, and the worst distances seen (``note`` also feeds the file's)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def note(self, name, v):
        self.worst[name] = max(self.worst.get(name, 0.0), float(v))
        WORST[name] = max(WORST.get(name, 0.0), float(v))


# ---------------------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------------------
def node_of(rng, code, **kw):
    """'F' fixed, 'PA' pose + affine (8 unknowns), 'P' pose only (6), 'A' affine only (2)."""
    aff = rng.integers(-4, 5, 2) / 64.0
    return ref.make_node(T=ref.random_pose(rng), aff=aff, lr_pose=1.0 if "P" in code else 0.0, lr_aff=0.5 if "A" in code else 0.0, **kw)


def draw_klds(rng, blocks):
    return [(rng.integers(-8, 9, N) / 64.0).astype(f32) for N, _ in blocks]


def chain_window(rng, codes, N_star=5, N_chain=4, exact=True, rps=2, n_tiles=3, **kw):
    """Nodes ``codes``; every node from 1 on is the target of an anchor edge of block 0 (from node 0 when that is fixed, from the identity
    otherwise) and, from 2 on, of an edge from its predecessor in block 1: both blocks meet every free node (nc = n_y)."""
    nodes = [node_of(rng, c) for c in codes]
    anchor = 0 if codes[0] == "F" else -1
    edges = [(anchor, i, 0, 1.0) for i in range(0 if anchor < 0 else 1, len(codes))]
    edges += [(i - 1, i, 1, 0.5) for i in range(2, len(codes))]
    blocks = [(N_star, 1.0), (N_chain, 1.0)] if len(codes) > 2 else [(N_star, 1.0)]
    recs = [ref.make_window_records(rng, blocks[e[2]][0], rps, n_tiles, exact=exact) for e in edges]
    return Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks), **kw)


def codes_for(ny):
    """A fixed first node, then 8-unknown nodes with one 6- or 2-unknown node in the middle where n_y asks for it."""
    if ny == 512:
        return ["PA"] * 64
    if ny == 0:
        return ["F", "F"]
    rest = {0: [], 2: ["A"], 6: ["P"]}[ny % 8]
    full = ["PA"] * (ny // 8)
    return ["F"] + full[:len(full) // 2] + rest + full[len(full) // 2:]


@pytest.mark.parametrize("ny", [0, 2, 6, 8, 62, 64, 66, 78, 126, 128, 130, 190, 192, 194, 254, 512])
def test_camera_sizes(ny):
    rng = np.random.default_rng(5000 + ny)
    rig = chain_window(rng, codes_for(ny), N_star=33 if ny == 512 else 5)          # (nc = 512: chunks of 16 rows -- 16, 16 and 1)
    for call in range(2):
        info = rig.step(what=f"n_y={ny} call {call}")
        assert info["decision"] == "step" and info["n_y"] == ny and info["active"].all()


def test_oversized_n_unknowns():
    results = []
    for n_unknowns in (40, 128, 192, 256):
        rig = chain_window(np.random.default_rng(40), ["F"] + ["PA"] * 5, n_unknowns=n_unknowns)
        for call in range(2):
            assert rig.step(what=f"n_y=40 in n_unknowns={n_unknowns} call {call}")["decision"] == "step"
        results.append((rig.ref["nodes"].tobytes(), np.concatenate(rig.ref["klds"]).tobytes()))
    for r in results[1:]:
        assert r == results[0], "the instantiations differ on the same window"


def test_graph_shapes():
    rng = np.random.default_rng(77)
    nodes = [node_of(rng, "PA", flags=1), node_of(rng, "F"), node_of(rng, "PA"),
             node_of(rng, "P", kind=1, a=(0.02, -0.03, 0.01, 0.04, -0.02, 0.03)), node_of(rng, "F"), node_of(rng, "A")]
    blocks = [(5, 1.0), (4, 0.0), (6, 1.0), (3, 1.0)]
    edges = [(-1, 0, 0, 1.0), (0, 2, 0, 1.0), (0, 2, 0, 0.5), (2, 0, 2, 1.0), (1, 2, 1, 1.0), (-1, 3, 2, 1.0), (1, 4, 3, 1.0), (2, 5, 2, 2.0),
             (1, 0, 2, 1.0)]
    recs = [ref.make_window_records(rng, blocks[e[2]][0], 2, 4) for e in edges]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    frozen_kld = rig.ref["klds"][1].copy()
    for call in range(3):
        info = rig.step(what=f"graph shapes call {call}")
        assert info["decision"] == "step" and info["n_y"] == 24
        assert info["active"].tolist() == [True] * 5 + [False] * 4 + [True] * 9
        assert np.array_equal(rig.ref["klds"][1], frozen_kld)
    assert not rig.ref["nodes"][3]["a"].any()


@pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 512, 513])
def test_schur_rows(N):
    rng = np.random.default_rng(6000 + N)
    nodes = [node_of(rng, "F"), node_of(rng, "PA")]
    blocks = [(3, 0.0), (N, 1.0)]                      # the ballast block keeps the camera system definite at N = 1 and makes row0 = 3
    edges = [(0, 1, 0, 1.0), (0, 1, 1, 1.0)]
    recs = [ref.make_window_records(rng, 3, 3, 2), ref.make_window_records(rng, N, 1, 3, rows_per_record=2, exact=False)]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    for call in range(2):
        info = rig.step(exact=False, what=f"block N={N} call {call}")
        assert info["decision"] == "step" and info["active"].sum() == N


def test_schur_two_chunks():
    rng = np.random.default_rng(56)
    nodes = [node_of(rng, "F")] + [node_of(rng, "PA") for _ in range(7)]
    blocks = [(147, 1.0)]
    edges = [(0, i, 0, 1.0) for i in range(1, 8)] + [(1, 2, 0, 1.0)]
    recs = [ref.make_window_records(rng, 147, 1, 5, rows_per_record=1, exact=False) for e in edges]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    for call in range(2):
        info = rig.step(exact=False, what=f"nc=56 N=147 call {call}")
        assert info["decision"] == "step" and info["n_y"] == 56 and info["active"].all()


def test_frozen_rows():
    rng = np.random.default_rng(91)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(6, 1.0), (4, 1.0)]
    edges = [(0, 1, 0, 1.0), (0, 2, 1, 1.0), (1, 2, 1, 1.0)]
    recs = [ref.make_window_records(rng, 6, [2, 1, 0, 3, 1, 2], 3), ref.make_window_records(rng, 4, 2, 3), ref.make_window_records(rng, 4, 2, 3)]
    scale = 1.0 / (3.0 * recs[0]["pair"]["P"])
    ref.set_segment(recs[0], 0, c=np.zeros(8), D=4.0, bd=-24.0)          # its own Newton step at lambda = 1: 24 / 8 = +3 -> +0.5
    ref.set_segment(recs[0], 3, c=np.zeros(8), D=2.0, bd=16.0)           # -4 -> -0.5
    ref.set_segment(recs[0], 4, D=2.5e-13 / scale)                      # D (1 + lambda) = 5e-13 <= 1e-12: no unknown
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    info = rig.step(exact=False, what="frozen rows")
    assert info["decision"] == "step" and info["active"].tolist() == [True, True, False, True, False, True] + [True] * 4
    assert info["dd"][0] == 0.5 and info["dd"][3] == -0.5 and abs(info["unclamped"][0] - 3) < 1e-9 and abs(info["unclamped"][3] + 4) < 1e-9
    D4 = info["H"][16 + 4, 16 + 4] * 2
    assert 4e-13 < D4 < 6e-13
    rig.step(exact=False, what="frozen rows, second call")


@pytest.mark.parametrize("n_edges", [64, 65])
def test_block_edge_list(n_edges):
    rng = np.random.default_rng(6400 + n_edges)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(2, 0.0), (3, 1.0)]
    shapes = [(0, 1), (0, 2), (1, 2), (2, 1)]
    edges = [(0, 1, 0, 1.0)] + [shapes[k % 4] + (1, 0.25) for k in range(n_edges)]        # (a foreign edge first: the list is a compaction)
    recs = [ref.make_window_records(rng, blocks[e[2]][0], 1, 2, rows_per_record=2) for e in edges]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    for call in range(2):
        assert rig.step(what=f"{n_edges} edges of one block call {call}")["decision"] == "step"


@pytest.mark.parametrize("n_unknowns,N", [(128, 127), (128, 128), (128, 129), (192, 63), (192, 64), (192, 65), (256, 255), (256, 256), (256, 257)])
def test_back_substitution(n_unknowns, N):
    rng = np.random.default_rng(7000 + n_unknowns + N)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "P")]
    blocks = [(N, 1.0)]
    edges = [(0, 1, 0, 1.0), (1, 2, 0, 1.0), (0, 2, 0, 1.0)]
    recs = [ref.make_window_records(rng, N, 1, 3, rows_per_record=1, exact=False) for e in edges]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks), n_unknowns=n_unknowns)
    info = rig.step(exact=False, what=f"back-substitution n_unknowns={n_unknowns} N={N}")
    assert info["decision"] == "step" and info["active"].all()


@pytest.mark.parametrize("n_tiles", [1, 4, 5, 6, 11])
def test_reduction(n_tiles):
    rng = np.random.default_rng(8000 + n_tiles)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(10, 1.0)]
    edges = [(0, 1, 0, 1.0), (1, 2, 0, 1.0), (0, 2, 0, 1.0)]
    recs = [ref.make_window_records(rng, 10, np.roll(np.arange(10), e), n_tiles) for e in range(3)]
    rig = Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks))
    info = rig.step(exact=True, what=f"n_tiles={n_tiles}")
    assert info["decision"] == "step" and info["active"].all()


def inline_rig(n_edges):
    rng = np.random.default_rng(8800)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(4, 0.0)]
    edges = [(0, 1, 0, 1.0), (1, 2, 0, 1.0), (0, 2, 0, 1.0), (2, 1, 0, 0.5), (0, 1, 0, 0.5)][:n_edges]
    recs = [ref.make_window_records(rng, 4, 2, 5) for e in edges]
    return Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks), flags=4)


@pytest.mark.parametrize("n_edges", [4, 5])
def test_inline_reduce(n_edges, monkeypatch):
    rig = inline_rig(n_edges)
    for call in range(2):
        info = rig.step(what=f"flags bit 2, {n_edges} edges, call {call}")
        assert info["decision"] == "step" and not info["active"].any()
    if n_edges == 4:          # the same window with the reduction in a launch of its own: bit for bit
        monkeypatch.setenv("SP_WGN_NO_INLINE", "1")
        other = inline_rig(n_edges)
        for call in range(2):
            other.step(what=f"flags bit 2, {n_edges} edges, separate reduce launch, call {call}")
        assert other.ref["nodes"].tobytes() == rig.ref["nodes"].tobytes() and np.array_equal(other.ref["pose"], rig.ref["pose"])
        assert np.array_equal(other.ref["state"], rig.ref["state"]) and np.array_equal(other.ref["losses"], rig.ref["losses"])


def small_rig(seed=123, exact=True, **kw):
    rng = np.random.default_rng(seed)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA", flags=1), node_of(rng, "P")]
    blocks = [(3, 1.0), (4, 0.0), (4, 1.0)]
    edges = [(0, 1, 0, 1.0), (0, 2, 0, 0.5), (1, 2, 2, 1.0), (2, 1, 2, 2.0), (-1, 3, 2, 1.0), (1, 3, 1, 1.0)]
    recs = [ref.make_window_records(rng, blocks[e[2]][0], 2, 3, exact=exact) for e in edges]
    return Rig(nodes, edges, blocks, recs, draw_klds(rng, blocks), **kw), recs


def with_loss(recs, factor):
    out = []
    for r in recs:
        r = dict(r, span=r["span"].copy())
        ref.scale_cost(r, factor)
        out.append(r)
    return out


def test_pose_only_flag():
    rig, _ = small_rig(flags=1)
    klds = [k.copy() for k in rig.ref["klds"]]
    for call in range(2):
        info = rig.step(what=f"flags bit 0 call {call}")
        assert info["decision"] == "step" and not info["active"].any() and np.abs(info["dy"]).min() > 0
        assert all(np.array_equal(a, b) for a, b in zip(rig.ref["klds"], klds))
        assert np.array_equal(rig.ref["kld_backup"], np.concatenate(klds))


def test_predicted_exit():
    rig, _ = small_rig(flags=2, lam0=2e-4, conv_tol=10.0)
    info = rig.step(what="predicted exit at lambda = 1e-4")
    assert info["decision"] == "step" and info["lam"] == float(f32(2e-4) * f32(0.5)) and info["predicted"] and 0 < info["gain"]
    assert rig.ref["state"][6] == 1 and rig.step(what="after the predicted exit")["decision"] == "frozen"
    rig, _ = small_rig(flags=2, lam0=0.2, conv_tol=10.0)
    info = rig.step(what="predicted exit at lambda = 0.1")
    assert info["decision"] == "step" and not info["predicted"] and rig.ref["state"][6] == 0
    rig, _ = small_rig(flags=2, lam0=2e-4, conv_tol=1e-9)
    info = rig.step(what="predicted exit, a gain above the tolerance")
    assert info["decision"] == "step" and not info["predicted"] and info["gain"] > 1e-9 * info["loss"] and rig.ref["state"][6] == 0
    rig, _ = small_rig(flags=2, lam0=-3.0, conv_tol=10.0, lm_up=-1e-4, lm_down=1.0, lm_min=-10.0)
    info = rig.step(what="predicted exit after a failed factorisation")
    assert info["decision"] == "failed" and rig.ref["state"][6] == 0


def test_accept_reject_accept():
    rig, recs = small_rig(lam0=0.25)
    decisions = []
    for call, factor in enumerate((1.0, 0.5, 0.75, 0.5, 0.25)):
        rig.load(with_loss(recs, factor))
        decisions.append(rig.step(what=f"LM call {call}")["decision"])
    assert decisions == ["step", "step", "reject", "step", "step"]
    s = rig.ref["state"]
    assert (s[0], s[2], s[3], s[4], s[5]) == (0.25, 4, 1, 0, 5)          # 0.25 / 2 / 2, x 8 on the reject, kept by the step after it, / 2


def test_converged_ignores_further_calls():
    rig, recs = small_rig(lam0=0.25, conv_tol=1e-2)
    for call, (factor, dec) in enumerate(((1.0, "step"), (0.5, "step"), (0.5 * (1 - 2.0 ** -10), "converged"), (0.25, "frozen"), (4.0, "frozen"),
                                          (0.25, "frozen"))):
        rig.load(with_loss(recs, factor))
        assert rig.step(what=f"convergence call {call}")["decision"] == dec
    assert rig.ref["state"][5] == 3 and rig.ref["state"][6] == 1


def test_failed_factorisation():
    rig, _ = small_rig(lam0=-3.0, conv_tol=1e-2, lm_up=-1e-4, lm_down=1.0, lm_min=-10.0)
    start = ref.copy_state(rig.ref)
    info = rig.step(what="1 + lambda < 0")
    s = rig.ref["state"]
    assert info["decision"] == "failed" and s[:10].tolist() == [float(f32(-3.0) * f32(-1e-4)), s[7], 0, 0, 1, 1, 0, s[7], 1, 0]
    assert np.array_equal(rig.ref["nodes"], start["nodes"]) and all(np.array_equal(a, b) for a, b in zip(rig.ref["klds"], start["klds"]))
    info = rig.step(what="the same point, lambda = 3e-4")            # no convergence test (the loss equals the stored one), lambda not lowered
    s = rig.ref["state"]
    assert info["decision"] == "step" and s[0] == f32(-3.0) * f32(-1e-4) and (s[2], s[3], s[4], s[6], s[8]) == (1, 0, 0, 0, 1)


def test_too_many_unknowns():
    rig, _ = small_rig(n_unknowns=16)                                 # the window has 22
    start = ref.copy_state(rig.ref)
    for call in range(2):
        assert rig.step(what=f"too many unknowns call {call}")["decision"] == "too_many"
    s = rig.ref["state"]
    assert s[9] == 1 and s[6] == 1 and s[5] == 0 and np.array_equal(np.delete(s, [6, 9]), np.delete(start["state"], [6, 9]))


def test_max_losses():
    rig, recs = small_rig(lam0=0.25, max_losses=2, exact=False)
    for call, factor in enumerate((1.0, 0.5, 0.25, 0.125)):
        rig.load(with_loss(recs, factor))
        assert rig.step(exact=False, what=f"max_losses call {call}")["decision"] == "step"
    assert rig.ref["state"][5] == 4 and (rig.ref["losses"][2:] == SENTINEL).all() and (rig.ref["losses"][:2] > 0).all()
