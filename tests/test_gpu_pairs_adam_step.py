"""-m gpu: ONE sp_pairs_adam_step call (solve_adam in csrc/sp_solve_device.h, what bench.py --mode adam times) on three pairs against the
float64 yardstick ``pair_adam_step_ref`` of tests/window_adam_step_ref.py.  The middle pair is the one under test (its strides into every
array are non-zero); the neighbours are small and always the same.

Everything is hand-made (tests/window_adam_cases.py): guard records valued 1e6 around every pair's span and segment records, pix / src4 /
kp_L / trg3 NULL, kld rows and the m_kld / v_kld parts of the state with sentinel tails behind N, losses with a tail.  After every call
every buffer is compared and the reference continues from the device's values.

Bounds (derived): kld, the target affine pair and all moments within adam_bound (<= 2e-6 lr + 1 ulp, proved by the host file); the pose
is Exp(step) pose in float64 rounded once: 1 ulp at max(|entry|, 1) / max(|t|, 1) plus what the step's own adam_bound is worth (2.02 sum_k
bound_k); the last row is exactly 0 0 0 1; aff[0, 1] (the source's pair) and st[1] untouched; st[0] exact; losses bitwise (dyadic records).

Cases: N in {1, 256, 257, 9}, n_tiles in {1, 17, 129}, aff NULL and set, residual > 0, < 0 and exactly 0 (sign 0: every gradient is zero and
the moments still decay), steps 1, 2, 3 from zero moments and 301..303 from preloaded ones (the pow-based bias correction), three
consecutive calls each."""
import time

import numpy as np
import pytest
import torch

import window_adam_cases as cases
import window_adam_step_ref as ref
from window_adam_step_ref import f32
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

GUARD = 1.0e6
SENTINEL = -5.0
TAIL = 3
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


class Rig:
    def __init__(self, case):
        from super_primitive_amd import _lib
        self._lib, self.lib, self.case = _lib, _lib.load(), case
        pairs = case["pairs"]
        self.n, self.max_N, self.Ns = len(pairs), case["max_N"], [p["N"] for p in pairs]
        self.ref = [p["state"] for p in pairs]
        kld = np.full((self.n, self.max_N), SENTINEL, f32)
        for i, p in enumerate(pairs):
            kld[i, :p["N"]] = p["kld"]
        self.kld = T(kld)
        self.pose = T(np.stack([p["pose"] for p in pairs]).reshape(self.n, 16).astype(f32))
        self.aff = T(np.stack([p["aff"] if p["aff"] is not None else np.full(4, SENTINEL, f32) for p in pairs]))
        self.state = T(np.stack([st["st"] for st in self.ref]))
        self.losses = T(np.full(self.n + TAIL, SENTINEL, f32))
        self.tile0 = np.cumsum([1] + [p["sets"][0]["pair"]["n_tiles"] + 1 for p in pairs])
        self.rec0 = np.cumsum([1] + [len(p["sets"][0]["seg"]) + 1 for p in pairs])
        self.sto = T(np.concatenate([p["sets"][0]["pair"]["seg_tile_off"] for p in pairs]).astype(np.int32))
        sto_off = np.cumsum([0] + [N + 1 for N in self.Ns])
        arr = (_lib.SpPair * self.n)()
        self.views = []
        for i, p in enumerate(pairs):                     # pix, src4, kp_L, trg3 stay NULL
            d, q = arr[i], p["sets"][0]["pair"]
            d.kld, d.pose = self.kld[i].data_ptr(), self.pose[i].data_ptr()
            d.aff = None if p["aff"] is None else self.aff[i].data_ptr()
            d.seg_tile_off = self.sto.data_ptr() + 4 * int(sto_off[i])
            d.N, d.P, d.tile0, d.n_tiles, d.rec0 = q["N"], q["P"], int(self.tile0[i]), q["n_tiles"], int(self.rec0[i])
            self.views.append(dict(q, tile0=int(self.tile0[i]), rec0=int(self.rec0[i])))
        self.pairs = T(np.frombuffer(bytes(arr), np.uint8).copy())
        self.span_host = np.full((int(self.tile0[-1]), ref.NVP), GUARD, f32)
        self.seg_host = np.full((int(self.rec0[-1]), ref.NVS), GUARD, f32)

    def load(self, call):
        for i, p in enumerate(self.case["pairs"]):
            r = p["sets"][call]
            self.span_host[self.tile0[i]:self.tile0[i] + len(r["span"])] = r["span"]
            self.seg_host[self.rec0[i]:self.rec0[i] + len(r["seg"])] = r["seg"]
        self.span, self.seg = T(self.span_host), T(self.seg_host)

    def step(self, call):
        self.load(call)
        infos = [{} for _ in range(self.n)]
        want = [ref.pair_adam_step_ref(self.span_host, self.seg_host, self.views[i], self.ref[i], cases.PAIR_LRS, self.max_N, infos[i])
                for i in range(self.n)]
        L, p = self._lib, self._lib.ptr
        lr = [float(x) for x in cases.PAIR_LRS]
        L.check(self.lib.sp_pairs_adam_step(p(self.pairs), self.n, self.max_N, p(self.span), p(self.seg), lr[0], lr[1], lr[2], p(self.state),
                                            p(self.losses), L.stream_ptr()), "sp_pairs_adam_step")
        torch.cuda.synchronize()
        kld, pose, aff, state, losses = npy(self.kld), npy(self.pose), npy(self.aff), npy(self.state), npy(self.losses)
        assert bits(npy(self.span)) == bits(self.span_host) and bits(npy(self.seg)) == bits(self.seg_host), "records written"
        assert (losses[self.n:] == SENTINEL).all()
        M = self.max_N
        for i, (w, info, before) in enumerate(zip(want, infos, self.ref)):
            tag, N, o, st = f"call {call} pair {i}", self.Ns[i], info["offsets"], state[i]
            assert (kld[i, N:] == SENTINEL).all() and (st[2 + N:2 + M] == SENTINEL).all() and (st[2 + M + N:2 + 2 * M] == SENTINEL).all(), f"{tag}: tails"
            assert st[0] == w["st"][0] and st[1] == 0, f"{tag}: step count {st[0]}"
            assert bits(losses[i:i + 1]) == bits(np.array([w["loss"]], f32)), f"{tag}: loss {losses[i]!r} != {w['loss']!r}"
            parts = [("kld", kld[i, :N], o["mk"], o["vk"], N), ("xi", None, o["mx"], o["vx"], 6)]
            if w["aff"] is not None:
                parts.append(("aff", aff[i, 2:], o["ma"], o["va"], 2))
                assert bits(aff[i, :2]) == bits(before["aff"][:2]), f"{tag}: the source's affine pair moved"
            else:
                assert (aff[i] == SENTINEL).all() and not st[o["ma"]:].any(), f"{tag}: affine part of a pair without one"
            for name, pgot, mo, vo, n in parts:
                ent = info[name]
                for what, a, b, bound in (("parameter", pgot, ent["p"], ent["b_p"]), ("m", st[mo:mo + n], ent["m"], ent["b_m"]),
                                          ("v", st[vo:vo + n], ent["v"], ent["b_v"])):
                    if a is None:
                        continue
                    d = np.abs(a.astype(np.float64) - b)
                    note(f"{name} {what} / adam_bound", (d / np.where(bound > 0, bound, 1)).max())
                    if what == "parameter":
                        note(f"{name} parameter / lr", d.max() / ent["lr"])
                    assert (d <= bound).all(), f"{tag}: {name} {what} off by {d.max():.3g}, bound {bound[d.argmax()]:.3g}"
            g, e = pose[i].reshape(4, 4), w["pose"]
            assert g[3].tolist() == [0, 0, 0, 1], f"{tag}: last row of the pose"
            scale = np.maximum(np.abs(e[:3]), 1)
            scale[:, 3] = max(np.abs(e[:3, 3]).max(), 1)
            sp = np.spacing(scale.astype(f32)).astype(np.float64)
            d = np.abs(g[:3].astype(np.float64) - e[:3])
            note("pose (ulp)", (d / sp).max())
            assert (d <= sp + info["T"]).all(), f"{tag}: pose off by {(d / sp).max():.3g} ulp"
            # the reference goes on from what the device holds
            w["kld"], w["pose"], w["st"] = kld[i, :N].copy(), g.copy(), st.copy()
            if w["aff"] is not None:
                w["aff"] = aff[i].copy()
        self.ref = want
        return infos


@pytest.mark.parametrize("k", range(len(cases.PAIR_CASES)))
def test_one_call_on_the_middle_pair(k):
    spec = cases.PAIR_CASES[k]
    rig = Rig(cases.pair_case(k))
    for call in range(3):
        info = rig.step(call)[1]
        assert info["t"] == spec["step"] + call + 1
        if spec["residual"] is not None:
            assert info["residual"] * 3 * rig.views[1]["P"] == pytest.approx(spec["residual"], abs=1e-12) and np.sign(info["residual"]) == np.sign(spec["residual"])
        if spec["residual"] == 0.0:
            assert not info["kld"]["g"].any() and not info["xi"]["g"].any()
