"""The float64 yardstick of one sp_window_step / sp_pairs_adam_step call (tests/window_adam_step_ref.py) checked without a GPU against
independent statements of the same things, and the conditions the two GPU files rely on proved on their own inputs
(tests/window_adam_cases.py):
  - the gradient chain against float64 autograd through torch.linalg.matrix_exp on the statements of the eager loop
    (odometery/loops.py::_map_window_eager: P = D_trg inv(T_trg) T_src inv(D_src) for kind 0, Exp(a) X for kind 1), evaluated on the
    record-linear cost r_e(P, aff, kld) = r0_e + <dr/dP_e, P - P0_e> + ...: 1e-9 relative;
  - its Adam step against torch.optim.Adam (CPU, float32, state preloaded) and against a plain np.float32 restatement of adam_torch, on
    the inputs of every GPU case: both within adam_bound, and adam_bound <= 2e-6 lr + 1 ulp of the parameter everywhere;
  - the running products 0.9^t, 0.999^t against pow;
  - every dyadic record set sums exactly; the kind-1 sums cancel by less than 8."""
import numpy as np
import pytest
import torch

import window_adam_cases as cases
import window_adam_step_ref as ref
from window_adam_step_ref import f32

CASES = cases.all_cases()


def hat(xi):
    z = torch.zeros((), dtype=torch.float64)
    return torch.stack([torch.stack([z, -xi[5], xi[4], xi[0]]), torch.stack([xi[5], z, -xi[3], xi[1]]), torch.stack([-xi[4], xi[3], z, xi[2]]),
                        torch.stack([z, z, z, z])])


def eager_gradients(nodes, T64, edges, blocks, reduced, abs_loss):
    """The eager loop's statements in float64 torch on the record-linear cost; returns (g6 (n x 6), gaff (n x 2), [gk per block], slots)."""
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    T = [t64(x) for x in T64]
    tang = [(t64(nd["a"]) if nd["kind"] == 1 else torch.zeros(6, dtype=torch.float64)).requires_grad_(True) for nd in nodes]
    aff = [t64(nd["aff"]).requires_grad_(True) for nd in nodes]
    kld = [torch.zeros(int(N), dtype=torch.float64, requires_grad=True) for N, _ in blocks]
    eye = torch.eye(4, dtype=torch.float64)
    loss, slots = 0.0, []
    for (src, trg, blk, w), (r0, g_t, g_R, da, db, dk) in zip(edges, reduced):
        if nodes[trg]["kind"] == 1:
            P = torch.linalg.matrix_exp(hat(tang[trg])) @ T[trg]
        else:
            D_trg = torch.linalg.matrix_exp(hat(tang[trg]))
            T_src, D_src = (T[src], torch.linalg.matrix_exp(hat(tang[src]))) if src >= 0 else (eye, eye)
            P = D_trg @ torch.linalg.inv(T[trg]) @ T_src @ torch.linalg.inv(D_src)
        P0 = P.detach()
        slots.append(P0.numpy().copy())
        drdP = t64(np.concatenate([g_R, g_t[:, None]], 1))
        gain = aff[trg] - (aff[src] if src >= 0 else torch.zeros(2, dtype=torch.float64))
        r = r0 + (drdP * (P - P0)[:3]).sum() + da * (gain[0] - gain[0].detach()) + db * (gain[1] - gain[1].detach()) + (t64(dk) * kld[blk]).sum()
        loss = loss + float(f32(w)) * (r.abs() if abs_loss else r)
    loss.backward()
    g = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy()
    return np.stack([g(x) for x in tang]), np.stack([g(x) for x in aff]), [g(x) for x in kld], slots


def chain_window(shape, rng):
    node = lambda code, **kw: cases.node_of(rng, code, **kw)
    if shape == "mapping":          # 3 keyframes (the first fixed), two supporting frames; every keyframe is matched against the others
        nodes = [node("F"), node("PA"), node("PA"), node("PA"), node("PA")]
        blocks = [(3, 1e-2), (4, 1e-2), (2, 1e-2)]
        edges = [(0, 1, 0, 1.0), (0, 2, 0, 1.0), (1, 0, 1, 1.0), (1, 2, 1, 0.5), (2, 0, 2, 1.0), (2, 1, 2, 2.0), (0, 3, 0, 1.0), (2, 4, 2, 1.0),
                 (2, 4, 2, 0.5)]
        return nodes, edges, blocks, 0
    if shape == "sfm":              # identity source, kind-1 targets with a tangent, loss = sum |r|
        nodes = [node("PA", kind=1, a=rng.uniform(-0.3, 0.3, 6).astype(f32)), node("PA", kind=1, a=rng.uniform(-0.05, 0.05, 6).astype(f32))]
        return nodes, [(-1, 0, 0, 1.0), (-1, 1, 0, 1.0)], [(5, 1e-2)], 1
    nodes = [node("F"), node("PA"), node("PA")]          # tracking: one keyframe, two tracked frames, depths frozen
    return nodes, [(0, 1, 0, 1.0), (0, 2, 0, 1.0)], [(4, 0.0)], 0


@pytest.mark.parametrize("shape", ["mapping", "sfm", "tracking"])
def test_gradient_chain_against_autograd_through_matrix_exp(shape):
    rng = np.random.default_rng({"mapping": 1, "sfm": 2, "tracking": 3}[shape])
    nodes, edges, blocks, abs_loss = chain_window(shape, rng)
    recs = [ref.make_adam_records(rng, blocks[e[2]][0], 2, 3, exact=False, residual=-0.7 if (abs_loss and k == 1) else None) for k, e in enumerate(edges)]
    span, seg, pairs = ref.lay_out(recs)
    nodes = np.array(nodes, ref.NODE)
    from gn_step_ref import se3_exp
    T64 = [se3_exp(np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.4, 0.4, 3)])) for _ in nodes]      # float64 rigid motions: the slot IS
    reduced = [ref.reduce_edge(span, seg, p) for p in pairs]                                                      # the composed pose
    g6, gaff, gk, slots = eager_gradients(nodes, T64, edges, blocks, reduced, abs_loss)
    got = ref.window_gradients(span, seg, dict(edges=edges, blocks=blocks, pairs=pairs), nodes, slots, abs_loss, T64=T64)
    for name, a, b in [("tangents", got["g6"], g6), ("affine", got["gaff"], gaff)] + [(f"kld {k}", got["gk"][k], gk[k]) for k in range(len(gk))]:
        assert np.abs(b).max() > 0, name
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), f"{shape}: {name} off by {np.abs(a - b).max() / np.abs(b).max():.3g}"
    if abs_loss:
        assert (got["r"] < 0).any() and (got["r"] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
def adam_entries():
    """(tag, entry, t, b1t, b2t) of every Adam application of every call of every GPU case."""
    for cid, build in CASES:
        for call, info, _, _ in build().run_host():
            for key, ent in info.items():
                if isinstance(ent, dict) and "b_p" in ent:
                    yield f"{cid} call {call} {key}", ent, info["t"], info["b1t"], info["b2t"]
    for k in range(len(cases.PAIR_CASES)):
        for call, i, info, _, _ in cases.run_pair_host(cases.pair_case(k)):
            for key in ("kld", "xi", "aff"):
                if key in info:
                    yield f"pair case {k} call {call} pair {i} {key}", info[key], info["t"], info["b1t"], info["b2t"]


def torch_adam(ent, t):
    p = torch.nn.Parameter(torch.tensor(ent["p0"].copy()))
    opt = torch.optim.Adam([p], lr=ent["lr"], betas=(0.9, 0.999), eps=1e-8, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.tensor(ent["m0"].copy()), exp_avg_sq=torch.tensor(ent["v0"].copy()))
    p.grad = torch.tensor(ent["g"].copy())
    opt.step()
    return p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()


def test_adam_step_within_bound_of_torch_and_of_float32_and_bound_under_cap():
    worst = dict(torch=0.0, float32=0.0, cap=0.0, steps=0)
    n = 0
    for tag, ent, t, b1t, b2t in adam_entries():
        n += ent["g"].size
        p0 = ent["p0"]
        cap = 2e-6 * ent["lr"] + np.spacing(np.abs(ent["p"]).astype(f32)).astype(np.float64)
        assert (ent["b_p"] <= cap).all(), f"{tag}: adam_bound {ent['b_p'].max():.3g} above the cap {cap[ent['b_p'].argmax()]:.3g}"
        worst["cap"] = max(worst["cap"], float((ent["b_p"] / cap).max()))
        worst["steps"] = max(worst["steps"], t)
        assert abs(b1t - 0.9 ** t) <= 1e-13 and abs(b2t - 0.999 ** t) <= 1e-13, tag
        for name, (p, m, v) in (("torch", torch_adam(ent, t)), ("float32", ref.adam_float32(ent["g"], ent["m0"], ent["v0"], p0, ent["lr"], b1t, b2t))):
            for what, a, b, bound in (("p", p, ent["p"], ent["b_p"]), ("m", m, ent["m"], ent["b_m"]), ("v", v, ent["v"], ent["b_v"])):
                d = np.abs(a.astype(np.float64) - b)
                assert (d <= bound).all(), f"{tag}: {name} {what} off by {d.max():.3g}, bound {bound[d.argmax()]:.3g}"
            worst[name] = max(worst[name], float((np.abs(p.astype(np.float64) - ent["p"]) / ent["b_p"]).max()))
    assert n > 5000
    print(f"\n{n} Adam parameters; worst |float32 - float64| / adam_bound: torch {worst['torch']:.3g}, np.float32 {worst['float32']:.3g}; "
          f"worst adam_bound / cap {worst['cap']:.3g}; longest step count {worst['steps']}")


def test_running_products_stay_within_1e_13_of_pow():
    longest = max(t for _, _, t, _, _ in adam_entries())
    b1, b2 = 1.0, 1.0
    for t in range(1, max(longest, 400) + 1):
        b1, b2 = b1 * 0.9, b2 * 0.999
        assert abs(b1 - 0.9 ** t) <= 1e-13 and abs(b2 - 0.999 ** t) <= 1e-13, t
    assert longest >= 300


def test_exact_record_sets_sum_exactly_and_kind1_sums_do_not_cancel():
    kind1 = 0
    for cid, build in CASES:
        case = build()
        for recs in case.calls:
            for r in recs:
                assert r["exact"] == case.exact
                if case.exact:
                    assert ref.sums_exact(r), cid
        if case.exact:
            assert all(float(f32(e[3])) in (0.25, 0.5, 1.0, 2.0, 4.0) for e in case.edges), cid          # w |r| is exact: the loss is bitwise
        for call, info, before, _ in case.run_host():
            if info["decision"] != "step":
                continue
            gr = info["grads"]
            for i, nd in enumerate(before["nodes"]):
                if nd["kind"] == 1 and gr["touched"][i]:
                    kind1 += 1
                    assert (gr["k1_terms"][i] <= 8 * np.abs(gr["g6"][i])).all(), f"{cid} call {call}: kind-1 node {i} cancels"
    assert kind1 >= 2 * len(cases.KIND1)
    for k in range(len(cases.PAIR_CASES)):
        for p in cases.pair_case(k)["pairs"]:
            assert all(ref.sums_exact(r) for r in p["sets"])


def test_state_machine_by_hand():
    """skip_first, the restart of the bias correction, the rel_tol freeze and max_losses, on the yardstick alone."""
    runs = {cid: list(build().run_host()) for cid, build in CASES if cid.split("-")[0] in ("skip_first", "rel_tol", "max_losses")}
    sk = runs["skip_first"]
    assert [i["decision"] for _, i, _, _ in sk] == ["skipped", "step", "step", "step"] and [i["t"] for _, i, _, _ in sk] == [0, 1, 2, 1]
    first = sk[0]
    assert first[3]["nodes"].tobytes() == first[2]["nodes"].tobytes() and first[3]["losses"][0] == first[3]["state"][4] and first[3]["state"][1] == 1
    assert np.array_equal(ref.running_products(sk[3][3]["state"]), [0.9, 0.999]) and sk[3][3]["nodes"]["m"].any()
    rt = runs["rel_tol-0.01"]
    assert [i["decision"] for _, i, _, _ in rt] == ["step", "step", "step", "frozen", "frozen"] and [i.get("done") for _, i, _, _ in rt[:3]] == [False, False, True]
    assert rt[2][3]["nodes"].tobytes() != rt[2][2]["nodes"].tobytes() and rt[4][3]["state"].tobytes() == rt[2][3]["state"].tobytes()
    r0 = runs["rel_tol-0"]
    assert all(new["state"][2] == 123.0 and new["state"][3] == 0 for _, _, _, new in r0)
    for m in (0, 2):
        last = runs[f"max_losses-{m}"][-1][3]
        assert last["state"][1] == 4 and (last["losses"][m:] == -5.0).all() and (last["losses"][:m] != -5.0).all()
