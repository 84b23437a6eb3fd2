"""The hand-made windows and pairs that tests/test_gpu_window_adam_step.py and tests/test_gpu_pairs_adam_step.py run on the device --
numpy only, so that tests/test_window_adam_step_ref_host.py can prove on a CPU what the GPU files take for granted about their own inputs
(exact sums, the cap on adam_bound, the kind-1 cancellation cap).

Moments.  A 'warm' case starts at Adam step t0 with moments drawn from the case's own first gradient, |m0| <= |g| and 0.25 g^2 <= v0 <=
2 g^2 (so that no step exceeds 2 lr) (m0 = g, v0 = 16 g^2 for a kind-1 tangent: the float32 error of its gradient is divided by sqrt(v)); a 'fresh' case starts from
zero moments at t = 0.  Both keep adam_bound below 2e-6 lr + 1 ulp (asserted by the host file)."""
import numpy as np

import window_adam_step_ref as ref
from window_adam_step_ref import AdamArgs, f32

LR_POSE, LR_AFF, LR_KLD = 1e-3, 1e-5, 1e-2


class Case:
    """nodes, edges (src, trg, block, weight), blocks (N, lr), klds / bm / bv per block, calls = the records of every call, args, t0,
    pokes = {call: {state index: value}} written before that call, no_aff = edges without an aff slot, exact = dyadic records."""

    def __init__(self, name, nodes, edges, blocks, calls, rng, warm=True, t0=37, exact=True, pokes=None, no_aff=(), **args):
        self.name, self.nodes, self.edges, self.blocks, self.calls = name, [n.copy() for n in nodes], list(edges), list(blocks), calls
        self.args, self.exact, self.pokes, self.no_aff = AdamArgs(**args), exact, pokes or {}, frozenset(no_aff)
        self.t0 = t0 if warm else 0
        for e, r in zip(edges, calls[0]):
            assert r["pair"]["N"] == blocks[e[2]][0]
        self.klds = [(rng.integers(-8, 9, N) / 64.0).astype(f32) for N, _ in blocks]
        self.bm = [np.zeros(N, f32) for N, _ in blocks]
        self.bv = [np.zeros(N, f32) for N, _ in blocks]
        for nd in self.nodes:
            ref.set_moments(nd, 0, 0, 0, 0)
        if warm:
            self.seed_moments(rng)

    def window(self, call=0):
        span, seg, pairs = ref.lay_out(self.calls[call])
        return span, seg, dict(edges=self.edges, blocks=self.blocks, pairs=pairs, no_aff=self.no_aff)

    def slots(self):
        nodes = np.array(self.nodes, ref.NODE)
        return [ref.compose_edge(e, nodes) for e in self.edges]

    def gradients(self, call=0):
        span, seg, win = self.window(call)
        return ref.window_gradients(span, seg, win, np.array(self.nodes, ref.NODE), [s[0] for s in self.slots()], int(self.args.abs_loss))

    def seed_moments(self, rng):
        gr = self.gradients()

        def draw(g, kind1=False):
            g = np.asarray(g, np.float64)
            m = np.where(g != 0, g * (1.0 if kind1 else rng.uniform(-1, 1, g.shape)), 1e-3 * rng.uniform(-1, 1, g.shape))
            v = np.where(g != 0, g * g * (16.0 if kind1 else rng.uniform(0.25, 2.0, g.shape)), 1e-6 * rng.uniform(0.5, 2.0, g.shape))
            return m.astype(f32), v.astype(f32)
        for b in range(len(self.blocks)):
            self.bm[b], self.bv[b] = draw(gr["gk"][b])
        for i, nd in enumerate(self.nodes):          # (in node order, after the blocks: an idle node appended to a window changes no other draw)
            nd["m"], nd["v"] = draw(gr["g6"][i], nd["kind"] == 1)
            nd["aff_m"], nd["aff_v"] = draw(gr["gaff"][i])

    def state(self):
        sl = self.slots()
        st = ref.new_state(self.nodes, self.klds, self.bm, self.bv, [s[0] for s in sl], [s[1] for s in sl], t=self.t0)
        for e in self.no_aff:
            st["aff"][e] = -5.0
        return st

    def run_host(self):
        """The yardstick alone over every call (continuing from its own values): yields (call, info, before, after)."""
        st = self.state()
        for call in range(len(self.calls)):
            span, seg, win = self.window(call)
            for k, val in self.pokes.get(call, {}).items():
                st["state"][k] = val
            info = {}
            new = ref.window_adam_step_ref(span, seg, win, st, self.args, info)
            yield call, info, st, new
            st = new


def node_of(rng, code, **kw):
    """'F' fixed, 'PA' pose + affine, 'P' pose only, 'A' affine only."""
    aff = rng.integers(-4, 5, 2) / 64.0
    return ref.make_node(T=ref.random_pose(rng), aff=aff, lr_pose=LR_POSE if "P" in code else 0.0, lr_aff=LR_AFF if "A" in code else 0.0, **kw)


def records(rng, edges, blocks, n_tiles=2, rps=1, **kw):
    return [ref.make_adam_records(rng, blocks[e[2]][0], rps, n_tiles, **kw) for e in edges]


# ---------------------------------------------------------------------------------------------------------------------------------
REDUCTION_TILES = [1, 15, 16, 17, 127, 128, 129, 257]


def reduction_case(n_tiles):
    """Three edges of n_tiles spans each; block 0 has 6 segments of 0, 1, 7, 8, 9 and 17 records, block 1 has N in {1, 255, 256, 257} by
    turns with the same record counts cycled; column 13 holds NaN."""
    k = REDUCTION_TILES.index(n_tiles)
    rng = np.random.default_rng(1000 + n_tiles)
    N1 = [1, 255, 256, 257][k % 4]
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(6, LR_KLD), (N1, LR_KLD)]
    edges = [(0, 1, 0, 1.0), (1, 2, 1, 0.5), (0, 2, 1, 2.0)]
    rps = {0: [0, 1, 7, 8, 9, 17], 1: np.roll(np.resize([0, 1, 7, 8, 9, 17], N1), k)}
    recs = [ref.make_adam_records(rng, blocks[e[2]][0], rps[e[2]], n_tiles, poison=np.nan) for e in edges]
    return Case(f"n_tiles={n_tiles}", nodes, edges, blocks, [recs], rng, warm=bool(k % 2), abs_loss=k % 2)


def graph_shapes_case():
    rng = np.random.default_rng(77)
    nodes = [node_of(rng, "F", flags=1), node_of(rng, "PA"), node_of(rng, "PA", flags=1), node_of(rng, "A"), node_of(rng, "F"), node_of(rng, "P"),
             node_of(rng, "F", a=(1e-3, -2e-3, 5e-4, 2e-3, -1e-3, 1.5e-3)), node_of(rng, "PA", flags=1), node_of(rng, "A", flags=1)]
    # node 3: fixed pose in the middle, affine free, no renormalisation; node 4: all fixed; node 5: lr_aff = 0; node 6: no edge, lr_pose = 0
    # and a tangent (folded in all the same); node 7: no edge, renormalised; node 8: pose fixed, renormalised
    blocks = [(5, LR_KLD), (4, 0.0), (6, 2 * LR_KLD), (3, LR_KLD)]          # 1 frozen between free ones, 3 named by no edge
    edges = [(-1, 1, 0, 1.0), (1, 2, 0, 0.5), (1, 2, 0, 2.0), (2, 1, 2, 1.0), (0, 2, 1, 1.0), (4, 5, 2, 0.25), (2, 3, 2, 1.0), (3, 5, 1, 4.0),
             (1, 8, 0, 1.0)]
    calls = [records(rng, edges, blocks, n_tiles=3, rps=2) for _ in range(3)]
    return Case("graph shapes", nodes, edges, blocks, calls, rng, no_aff=(3,))


KIND1 = [(norm, idx, n) for norm in (0.0, 1e-3, 0.7) for idx, n in ((0, 34), (31, 34), (32, 34), (40, 66))]


# theta^2 of the tangent's rotational part on either side of 0.5, where se3_exp_times leaves its series for the closed forms, and at 2; node
# 0 (Dual<1> through LDS) and node 32 of 34 (Dual<6>)
KIND1_THETA2 = [(name, idx, 34) for name in ("0.5-", "0.5+", "2") for idx in (0, 32)]
THETA2 = {"0.5-": 0.5 * (1 - 2.0 ** -20), "0.5+": 0.5 * (1 + 2.0 ** -20), "2": 2.0}


def kind1_case(norm, idx, n_nodes, theta2=None):
    """A kind-1 node with a persistent tangent of the given norm at index idx of n_nodes, the target of two identity-source edges (the SfM
    shape); the two last nodes are kind 0 and joined by an edge; every other node is idle.  The records are the first draw whose kind-1
    sums cancel by less than 8 (the cap the host file asserts).  theta2 (a key of THETA2): the rotational part has that theta^2 as the
    kernel sums it in float32 (on the named side of 0.5), the translational part the norm."""
    for seed in range(200):
        rng = np.random.default_rng([seed, idx, n_nodes, int(norm * 1e4)] + ([int(THETA2[theta2] * 1e4)] if theta2 else []))
        nodes = [node_of(rng, "PA") for _ in range(n_nodes)]
        d = rng.standard_normal(6)
        a = (norm * d / np.linalg.norm(d)).astype(f32)
        if theta2:
            a = np.concatenate([norm * d[:3] / np.linalg.norm(d[:3]), np.sqrt(THETA2[theta2]) * d[3:] / np.linalg.norm(d[3:])]).astype(f32)
            t = a[3] * a[3] + a[4] * a[4] + a[5] * a[5]
            assert abs(float(t) - THETA2[theta2]) <= 4 * np.spacing(f32(t)) and (t < 0.5) == (THETA2[theta2] < 0.5)
        nodes[idx] = node_of(rng, "PA", kind=1, a=a)
        blocks = [(3, LR_KLD), (2, LR_KLD)]
        edges = [(-1, idx, 0, 1.0), (-1, idx, 1, 0.5), (n_nodes - 2, n_nodes - 1, 1, 1.0)]
        recs = records(rng, edges, blocks, n_tiles=2, rps=1, exact=False)
        case = Case(f"kind 1, |a|={norm:g}{', theta2=' + theta2 if theta2 else ''}, node {idx} of {n_nodes}", nodes, edges, blocks, [recs, recs], rng, t0=300, exact=False, abs_loss=1)
        gr = case.gradients()
        if (gr["k1_terms"][idx] <= 4 * np.abs(gr["g6"][idx])).all():
            return case
    raise AssertionError("no draw without cancellation")


def fold_in_case(identity):
    """Fixed kind-0 nodes (lr_pose = 0) with a preset tangent each, folded in exactly as given: T <- T Exp(-a) through se3_exp_d, with
    theta^2 = 1e-10, either side of 1e-4 (its series against its closed form), 0.3 and 9 (se3_ref.fold_in_twists).  identity: every such T
    is the identity, so that the new T IS Exp(-a) and every entry can be judged at its own magnitude.  Nodes 0 and 1 carry the one edge."""
    import se3_ref
    rng = np.random.default_rng(616 + identity)
    nodes = [node_of(rng, "F"), node_of(rng, "PA")]
    for _, a in se3_ref.fold_in_twists():
        nd = node_of(rng, "F", a=a.astype(f32))
        if identity:
            nd["T"] = np.eye(4, dtype=f32).ravel()
        nodes.append(nd)
    blocks = [(3, LR_KLD)]
    edges = [(0, 1, 0, 1.0)]
    return Case(f"fold-in from {'the identity' if identity else 'general poses'}", nodes, edges, blocks, [records(rng, edges, blocks)], rng)


STAGING = ["96x64", "97x64", "96x65", "1024x3", "blocks64", "blocks66", "blocks66x65"]


def staging_case(which):
    rng = np.random.default_rng(4242)          # (one seed: 96x64 and 96x65 are the same graph but for the idle node)
    if which.startswith("blocks"):
        n_blocks = int(which[6:8])
        n_nodes = 65 if which.endswith("x65") else 10
        nodes = [node_of(rng, "F")] + [node_of(rng, "PA", flags=i & 1) for i in range(1, n_nodes)]
        blocks = [([1, 64, 65, 130][b % 4], 0.0 if b == 5 else LR_KLD * (1 + b / 64.0)) for b in range(n_blocks)]
        edges = []
        for b in range(n_blocks):
            s, t = b % 9, 1 + (b * 4 + 3) % 9
            edges.append((s, 9 if t == s else t, b, [0.5, 1.0, 2.0][b % 3]))
        return Case(which, nodes, edges, blocks, [records(rng, edges, blocks, n_tiles=1, rps=1)], rng)
    n_edges, n_nodes = (int(x) for x in which.split("x"))
    live = min(n_nodes, 64)
    nodes = [node_of(rng, "F")] + [node_of(rng, "PA", flags=i & 1) for i in range(1, live)]
    blocks = [(3, LR_KLD), (4, 2 * LR_KLD), (5, LR_KLD)]
    edges = []
    for e in range(n_edges):
        s, t = e % live, (e * 7 + 1) % live
        edges.append((s, t if t != s else (t + 1) % live, e % 3, [0.5, 1.0, 2.0][e % 3]))
    recs = records(rng, edges, blocks, n_tiles=2, rps=1)
    nodes += [node_of(np.random.default_rng(5), "PA") for _ in range(n_nodes - live)]          # idle
    return Case(which, nodes, edges, blocks, [recs], rng)


def abs_loss_case(abs_loss):
    """Residuals > 0, < 0 and exactly 0; the edge with r = 0 alone touches nodes 3, 4 and block 2."""
    rng = np.random.default_rng(909)
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA"), node_of(rng, "PA"), node_of(rng, "PA")]
    blocks = [(3, LR_KLD), (4, LR_KLD), (2, LR_KLD)]
    edges = [(0, 1, 0, 1.0), (1, 2, 1, 2.0), (3, 4, 2, 1.0)]
    recs = [ref.make_adam_records(rng, blocks[e[2]][0], 2, 3, residual=res) for e, res in zip(edges, (1.75, -2.5, 0.0))]
    return Case(f"abs_loss={abs_loss}", nodes, edges, blocks, [recs, recs], rng, abs_loss=abs_loss)


def small_window(rng):
    nodes = [node_of(rng, "F"), node_of(rng, "PA"), node_of(rng, "PA", flags=1), node_of(rng, "P")]
    blocks = [(3, LR_KLD), (4, 0.0), (4, LR_KLD)]
    edges = [(0, 1, 0, 1.0), (0, 2, 0, 0.5), (1, 2, 2, 1.0), (2, 1, 2, 2.0), (-1, 3, 2, 1.0), (1, 3, 1, 1.0)]
    return nodes, edges, blocks


def skip_first_case():
    """skip_first: call 0 records its loss and updates nothing; three more calls on swapped records; state[0] = 0 before the last one."""
    rng = np.random.default_rng(31)
    nodes, edges, blocks = small_window(rng)
    sets = [records(rng, edges, blocks, n_tiles=3, rps=2) for _ in range(3)]
    return Case("skip_first", nodes, edges, blocks, [sets[0], sets[0], sets[1], sets[2]], rng, warm=False, abs_loss=1, skip_first=1,
                pokes={3: {0: 0.0}})


def rel_tol_case(rel_tol):
    """Positive residuals scaled by 1, 1/2, 1/2 (1 - 2^-10), 1/4, 4: with rel_tol = 1e-2 the third call meets it (and still updates), the
    last two are ignored.  state[2] starts at 123 so that rel_tol = 0 is seen not to write it ..."""
    rng = np.random.default_rng(57)
    nodes, edges, blocks = small_window(rng)
    base = records(rng, edges, blocks, n_tiles=3, rps=2)
    calls = [[ref.scale_residual(r, f) for r in base] for f in (1.0, 0.5, 0.5 * (1 - 2.0 ** -10), 0.25, 4.0)]
    case = Case(f"rel_tol={rel_tol:g}", nodes, edges, blocks, calls if rel_tol else calls[:3], rng, rel_tol=rel_tol, pokes={0: {2: 123.0}})
    if rel_tol:          # ... and, with rel_tol, at the first loss itself: iteration 0 has no previous loss to compare with, whatever state[2] holds
        case.pokes = {0: {2: f32(case.gradients()["loss"])}}
    return case


def max_losses_case(max_losses):
    rng = np.random.default_rng(58)
    nodes, edges, blocks = small_window(rng)
    calls = [records(rng, edges, blocks, n_tiles=3, rps=2, exact=False) for _ in range(2)]
    return Case(f"max_losses={max_losses}", nodes, edges, blocks, [calls[0], calls[1], calls[0], calls[1]], rng, exact=False, max_losses=max_losses)


def all_cases():
    """Every window case of the GPU file, as (id, builder)."""
    out = [(f"reduction-{n}", lambda n=n: reduction_case(n)) for n in REDUCTION_TILES]
    out.append(("graph_shapes", graph_shapes_case))
    out += [(f"kind1-{norm:g}-{idx}of{n}", lambda a=(norm, idx, n): kind1_case(*a)) for norm, idx, n in KIND1]
    out += [(f"kind1-theta2={t}-{idx}of{n}", lambda a=(0.3, idx, n, t): kind1_case(*a)) for t, idx, n in KIND1_THETA2]
    out += [(f"fold_in-{i}", lambda i=i: fold_in_case(i)) for i in (1, 0)]
    out += [(f"staging-{w}", lambda w=w: staging_case(w)) for w in STAGING]
    out += [(f"abs_loss-{a}", lambda a=a: abs_loss_case(a)) for a in (1, 0)]
    out.append(("skip_first", skip_first_case))
    out += [(f"rel_tol-{r:g}", lambda r=r: rel_tol_case(r)) for r in (1e-2, 0.0)]
    out += [(f"max_losses-{m}", lambda m=m: max_losses_case(m)) for m in (0, 2)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# sp_pairs_adam_step: three pairs, the middle one under test
# ---------------------------------------------------------------------------------------------------------------------------------
PAIR_LRS = (1e-2, 1e-3, 1e-5)          # kld, pose, aff (two_frame_sfm.py's rates)
PAIR_CASES = [dict(N=1, n_tiles=1, aff=True, residual=None, step=0), dict(N=256, n_tiles=17, aff=False, residual=-2.5, step=0),
              dict(N=257, n_tiles=129, aff=True, residual=0.0, step=0), dict(N=257, n_tiles=17, aff=True, residual=-1.25, step=300),
              dict(N=9, n_tiles=1, aff=False, residual=None, step=300)]


def pair_case(k):
    """dict(pairs = [dict(rec sets per call, pose, kld, aff, step, moments)] x 3, calls = 3): the neighbours are small and fixed."""
    spec = PAIR_CASES[k]
    rng = np.random.default_rng(7100 + k)

    def one(N, n_tiles, aff, residual, step):
        rps = np.resize([0, 1, 7, 8, 9, 17], N)
        sets = [ref.make_adam_records(rng, N, rps, n_tiles, residual=residual) for _ in range(3)]
        if step:          # a warm pair sees the records its moments were drawn from in every call (the cap on adam_bound wants |g| ~ sqrt(v))
            sets = [sets[0]] * 3
        return dict(sets=sets, pose=ref.random_pose(rng), kld=(rng.integers(-8, 9, N) / 64.0).astype(f32),
                    aff=(rng.integers(-4, 5, 4) / 64.0).astype(f32) if aff else None, step=step, N=N)
    pairs = [one(5, 3, True, None, 0), one(**spec), one(4, 70, False, None, 0)]
    max_N = max(p["N"] for p in pairs) + 3
    for p in pairs:
        st = ref.pair_state(p["pose"], p["kld"], p["aff"], max_N, step=p["step"])
        if p["step"]:          # warm: moments from the pair's own first gradient, as for the windows
            info = {}
            ref.pair_adam_step_ref(p["sets"][0]["span"], p["sets"][0]["seg"], p["sets"][0]["pair"], st, PAIR_LRS, max_N, info)
            o = info["offsets"]
            for name, mo, vo in (("kld", o["mk"], o["vk"]), ("xi", o["mx"], o["vx"])) + ((("aff", o["ma"], o["va"]),) if p["aff"] is not None else ()):
                g = info[name]["g"].astype(np.float64)
                st["st"][mo:mo + len(g)] = np.where(g != 0, g * rng.uniform(-1, 1, len(g)), 1e-3 * rng.uniform(-1, 1, len(g)))
                st["st"][vo:vo + len(g)] = np.where(g != 0, g * g * rng.uniform(0.25, 2.0, len(g)), 1e-6 * rng.uniform(0.5, 2.0, len(g)))
        p["state"] = st
    return dict(pairs=pairs, max_N=max_N, calls=3)


def run_pair_host(case):
    """The yardstick over the case's calls, pair by pair: yields (call, pair index, info, before, after)."""
    states = [p["state"] for p in case["pairs"]]
    for call in range(case["calls"]):
        for i, p in enumerate(case["pairs"]):
            r = p["sets"][call]
            info = {}
            new = ref.pair_adam_step_ref(r["span"], r["seg"], r["pair"], states[i], PAIR_LRS, case["max_N"], info)
            yield call, i, info, states[i], new
            states[i] = new
