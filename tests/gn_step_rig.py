"""The rig of the -m gpu solver tests (test_gpu_gn_step.py, test_gpu_schedule_verdict.py): a few pairs on the device, driven from
hand-made partial records (no image, no table), and their reference states (gn_step_ref.py, schedule_verdict_ref.py).

Every case launches THREE pairs; the middle one is the pair under test, so its tile0, rec0, backup / lm_state / adam_state strides and
its pose0 / kld0 offsets are non-zero and max_N > N; the neighbours are compared with the reference as well, and so is every buffer a call
may write -- with a verdict also status, diag, attempts and evals, each with a sentinel entry in front of and behind the pairs' own.
After each compared call the reference continues from the DEVICE's values, so every call is judged from identical inputs."""
import ctypes

import numpy as np
import torch

import gn_step_ref as ref
import schedule_verdict_ref as sv
from gn_step_ref import GnArgs, f32
from gpu_util import T, npy

GUARD = 1.0e6          # records in front of and behind the pairs' own: reading one moves every sum far
SENTINEL = -5.0
STATUS_SENTINEL = -77  # status of a pair without a filed verdict, and of the entries around the pairs' own
DIAG_SENTINEL = -9.0   # diag of the same (a pair's own diag[5] is zeroed, as the header asks)
COUNT_SENTINEL = 7     # attempts / evals around the pairs' own
TAIL0 = 9.0            # kld0 behind a pair's N entries: a restart that copies one too many shows in the pair's kld tail


def make_pair(rng, N, rps, n_spans, exact=True, lam0=2.0, phase=0, residual_scale=0.25):
    rec = ref.make_records(rng, N, rps, n_spans, exact=exact, residual_scale=residual_scale)
    return dict(rec=rec, pose=ref.random_pose(rng), kld=(1.0 + 0.5 * rng.random(N)).astype(f32), lam0=lam0, phase=phase)


def neighbours(rng, exact=True):
    return (make_pair(rng, 5, [1, 0, 3, 2, 9], 3, exact=exact, lam0=0.5), make_pair(rng, 9, 2, 70, exact=exact, lam0=8.0))


def swap_cost(rec, base, factor):
    """``rec`` with the sum |r| column of ``base`` times ``factor``: a scripted cost on another system."""
    out = dict(rec, span=rec["span"].copy())
    out["span"][:, 0] = base["span"][:, 0]
    ref.scale_cost(out, factor)
    return out


def set_cost(rec, cost):
    """``rec`` with the pair's cost sum |r| / (3 P) exactly ``cost`` (a dyadic value): the whole sum sits in the first span."""
    out = dict(rec, span=rec["span"].copy())
    s = 3.0 * rec["pair"]["P"] * cost
    assert float(f32(s)) == s
    out["span"][:, 0] = 0
    out["span"][0, 0] = s
    return out


def set_segment_cost(rec, n, a, c):
    """Columns [8] (sum |r|) and [9] (valid points) of segment n (it must own a record): halves, quarters, ... over its records, the rest in
    the last one, so that the sum over the records is exact for dyadic a and c in any order."""
    sto = rec["pair"]["seg_tile_off"]
    k = int(sto[n + 1] - sto[n])
    assert k > 0, "the segment has no record to hold the values"
    w = np.array([0.5 ** (i + 1) for i in range(k - 1)] + [0.5 ** (k - 1)])
    for col, val in ((8, a), (9, c)):
        parts = (val * w).astype(f32)
        assert parts.astype(np.float64).sum() == val, (val, k)
        rec["seg"][sto[n]:sto[n + 1], col] = parts


def same(got, exp, ulps):
    """Distance of two float32 in ulp of the expected one; non-finite values must agree in kind (NaN with NaN, an infinity with itself)."""
    got, exp = np.atleast_1d(np.asarray(got, f32)), np.atleast_1d(np.asarray(exp, f32))
    fin, inf = np.isfinite(exp), np.isinf(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], exp[inf]), (got, exp)
    d = np.zeros(exp.shape)
    d[fin] = np.abs(got[fin].astype(np.float64) - exp[fin].astype(np.float64)) / np.spacing(np.maximum(np.abs(exp[fin]), f32(1e-30)))
    return d


class Rig:
    """A few pairs on the device and their reference states.  entry: 'gn' | 'conv' | 'sched'; phases: list of dict(max_iters, conv_tol,
    flags, next) for 'sched'.  The layout (N, record counts) of every pair is fixed; ``load`` swaps the record CONTENTS.

    Scheduled launches only, all optional: verdict (schedule_verdict_ref.Verdict; ``attempts`` / ``evals`` False = those arrays NULL),
    sched_entry / retry_entry / retry2_entry, per_phase (every phase reads record arrays of its own: ``load(recs, phase=p)``)."""

    def __init__(self, pairs, entry="gn", conv_tol=0.0, phases=None, lm=(8.0, 0.5, 1e-7), adam_lr=(1e-2, 1e-3), verdict=None, attempts=True,
                 evals=False, sched_entry=0, retry_entry=-1, retry2_entry=-1, per_phase=False):
        from super_primitive_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.entry, self.conv_tol, self.phases, self.lm, self.adam_lr = entry, conv_tol, phases, lm, adam_lr
        self.v, self.sched_entry, self.retry_entry, self.retry2_entry = verdict, sched_entry, retry_entry, retry2_entry
        self.n = len(pairs)
        self.max_N = max(p["rec"]["pair"]["N"] for p in pairs) + 3
        self.Ns = [p["rec"]["pair"]["N"] for p in pairs]
        self.tile0 = np.cumsum([1] + [p["rec"]["pair"]["n_tiles"] for p in pairs])
        self.rec0 = np.cumsum([1] + [len(p["rec"]["seg"]) for p in pairs])
        self.ref = []
        kld = np.full((self.n, self.max_N), SENTINEL, f32)
        for i, p in enumerate(pairs):
            st = ref.new_state(p["pose"], p["kld"], self.max_N, lam0=p["lam0"], scheduled=entry == "sched")
            if entry == "gn":
                st["done"] = None
            if entry == "sched":
                st["phase"] = p["phase"]
            st["backup"][:] = SENTINEL
            st["cost"] = f32(SENTINEL)
            if verdict is not None or evals:
                st = sv.with_verdict_state(st, attempts=attempts and verdict is not None, evals=evals, status=STATUS_SENTINEL, diag_fill=DIAG_SENTINEL)
            self.ref.append(st)
            kld[i, :self.Ns[i]] = p["kld"]
        self.kld = T(kld)
        self.pose = T(np.stack([st["pose"] for st in self.ref]).reshape(self.n, 16))
        self.lm_state = T(np.stack([st["lm_state"] for st in self.ref]))
        self.backup = T(np.full((self.n, 16 + self.max_N), SENTINEL, f32))
        self.costs = T(np.full(self.n, SENTINEL, f32))
        self.done = T(np.zeros(self.n, np.int32))
        self.phase = T(np.array([p["phase"] for p in pairs], np.int32))
        self.iters = T(np.zeros(self.n, np.int32))
        self.adam_state = T(np.zeros((self.n, 2 + 2 * (self.max_N + 8)), f32))
        self.adam_prev = npy(self.adam_state).copy()
        # the verdict's arrays: one sentinel entry in front of and behind the pairs' own; pose0 / kld0 laid out like pose / kld
        self.status = T(np.full(self.n + 2, STATUS_SENTINEL, np.int32))
        diag = np.full((self.n + 2, sv.DIAG_FLOATS), DIAG_SENTINEL, f32)
        diag[1:-1, 5] = 0
        self.diag = T(diag)
        cnt = np.full(self.n + 2, COUNT_SENTINEL, np.int32)
        cnt[1:-1] = 0
        self.attempts = T(cnt) if attempts else None
        ev = np.full((self.n + 2, sv.MAX_PHASES), COUNT_SENTINEL, np.int32)
        ev[1:-1] = 0
        self.evals = T(ev) if evals else None
        kld0 = kld.copy()
        for i, N in enumerate(self.Ns):
            kld0[i, N:] = TAIL0
        self.kld0, self.pose0 = T(kld0), self.pose.clone()
        self.sto = T(np.concatenate([p["rec"]["pair"]["seg_tile_off"] for p in pairs]).astype(np.int32))
        sto_off = np.cumsum([0] + [N + 1 for N in self.Ns])
        arr = (_lib.SpPair * self.n)()
        for i, p in enumerate(pairs):                     # pix, src4, kp_L, trg3, aff stay NULL: the solver must not touch them
            d, q = arr[i], p["rec"]["pair"]
            d.kld, d.pose = self.kld[i].data_ptr(), self.pose[i].data_ptr()
            d.seg_tile_off = self.sto.data_ptr() + 4 * int(sto_off[i])
            d.N, d.P, d.tile0, d.n_tiles, d.rec0 = q["N"], q["P"], int(self.tile0[i]), q["n_tiles"], int(self.rec0[i])
        self.pairs = T(np.frombuffer(bytes(arr), np.uint8).copy())
        n_arrays = len(phases) if per_phase else 1
        self.spans = [T(np.full((int(self.tile0[-1]) + 1, ref.NVP), GUARD, f32)) for _ in range(n_arrays)]
        self.segs = [T(np.full((int(self.rec0[-1]) + 1, ref.NVS), GUARD, f32)) for _ in range(n_arrays)]
        self.span, self.seg = self.spans[0], self.segs[0]
        self.phase_recs = [None] * n_arrays
        self.load([p["rec"] for p in pairs])

    # -- records ---------------------------------------------------------------------------------------------------------------------
    def load(self, recs, phase=None):
        """The record contents of every pair: into every record array, or into phase ``phase``'s own (per_phase)."""
        for k in (range(len(self.spans)) if phase is None else [phase]):
            self.phase_recs[k] = list(recs)
            for i, r in enumerate(recs):
                assert r["span"].shape == (self.tile0[i + 1] - self.tile0[i], ref.NVP) and len(r["seg"]) == self.rec0[i + 1] - self.rec0[i]
                self.spans[k][int(self.tile0[i]):int(self.tile0[i + 1])] = T(r["span"])
                if len(r["seg"]):
                    self.segs[k][int(self.rec0[i]):int(self.rec0[i + 1])] = T(r["seg"])
        self.recs = self.phase_recs[0]

    def recs_of(self, i):
        """phase -> the records pair i reads in that phase."""
        return lambda p: self.phase_recs[p if len(self.phase_recs) > 1 else 0][i]

    def poke(self, i, kld=None, pose=None, kld0=None, pose0=None):
        """Overwrite entries of pair i on the device and in the reference: dicts index -> value."""
        for name, dev_t, vals in (("kld", self.kld, kld), ("pose", self.pose, pose), ("kld0", self.kld0, kld0), ("pose0", self.pose0, pose0)):
            for k, x in (vals or {}).items():
                dev_t[i, k] = float(x)
                if name == "kld":
                    self.ref[i]["kld"][k] = x
                if name == "pose":
                    self.ref[i]["pose"].reshape(16)[k] = x
        torch.cuda.synchronize()

    # -- the reference ---------------------------------------------------------------------------------------------------------------
    def args(self, i):
        a = dict(lm_up=self.lm[0], lm_down=self.lm[1], lm_min=self.lm[2], adam_lr_pose=self.adam_lr[0], adam_lr_kld=self.adam_lr[1])
        if self.entry == "conv":
            a["conv_tol"] = self.conv_tol
        if self.entry == "sched":
            p = self.ref[i]["phase"]
            ph = self.phases[p]
            fl = ph.get("flags", 0)
            a.update(conv_tol=ph.get("conv_tol", 0.0), max_iters=ph["max_iters"], next_phase=ph.get("next", 0) or p + 1,
                     pose_only=bool(fl & self._lib.SP_PHASE_POSE_ONLY), depth_damp=0.125 * ((fl >> self._lib.SP_PHASE_DEPTH_DAMP_SHIFT) & 0xff),
                     predicted_exit=bool(fl & self._lib.SP_PHASE_PREDICTED_EXIT), adam=bool(fl & self._lib.SP_PHASE_ADAM))
        return GnArgs(**a)

    def sched_info(self):
        return sv.sched_info(self.phases, self.sched_entry, self.retry_entry, self.retry2_entry)

    def expect(self, i, info=None):
        """The reference's new state of pair i for the loaded records."""
        st = self.ref[i]
        if self.entry == "sched" and "status" in st:
            k0, p0 = npy(self.kld0)[i], npy(self.pose0)[i]
            return sv.schedule_step_ref(self.recs_of(i), st, self.sched_info(), self.v, k0, p0, self.lm, self.adam_lr, info=info)
        if self.entry == "sched" and st["phase"] >= len(self.phases):
            if info is not None:
                info["decision"] = "finished"
            return ref.copy_state(st)
        r = self.recs_of(i)(st["phase"] if self.entry == "sched" else 0)
        a = self.args(i)
        if a.get("adam"):
            if info is not None:
                info["decision"] = "adam"
            return ref.adam_sched_ref(r["span"], r["seg"], r["pair"], st, a)
        return ref.gn_step_ref(r["span"], r["seg"], r["pair"], st, a, info)

    # -- launches --------------------------------------------------------------------------------------------------------------------
    def schedule(self, pairs_ptr=None, launched_spans=True):
        """The SpSchedule of ``phases``.  launched_spans False: every phase has n_spans = 0, a run launches no cost pass."""
        sched = self._lib.SpSchedule()
        for k, spec in enumerate(self.phases):
            ph, a = sched.phase[k], k if len(self.spans) > 1 else 0
            ph.pairs, ph.span_partials, ph.seg_partials = pairs_ptr or self.pairs.data_ptr(), self.spans[a].data_ptr(), self.segs[a].data_ptr()
            ph.n_spans, ph.max_iters, ph.conv_tol = int(self.tile0[-1]) if launched_spans else 0, spec["max_iters"], spec.get("conv_tol", 0.0)
            ph.flags, ph.next = spec.get("flags", 0), spec.get("next", 0)
        sched.n_phases, sched.entry, sched.retry_entry, sched.retry2_entry = len(self.phases), self.sched_entry, self.retry_entry, self.retry2_entry
        sched.adam_lr_pose, sched.adam_lr_kld, sched.adam_state = self.adam_lr[0], self.adam_lr[1], self.adam_state.data_ptr()
        return sched

    def verdict_struct(self):
        """The SpVerdict of ``v`` over this rig's arrays (None without a verdict and without evals)."""
        if self.v is None and self.evals is None:
            return None
        v = self._lib.SpVerdict()
        if self.v is not None:
            v.status, v.diag = self.status[1:].data_ptr(), self.diag[1:].data_ptr()
            v.attempts = self.attempts[1:].data_ptr() if self.attempts is not None else None
            v.pose0, v.kld0, v.pose_base, v.kld_base = self.pose0.data_ptr(), self.kld0.data_ptr(), self.pose.data_ptr(), self.kld.data_ptr()
            for k, x in self.v.items():
                setattr(v, k, x)
        if self.evals is not None:
            v.evals = self.evals[1:].data_ptr()
        return v

    def call_sched_step(self, sched, v):
        """sp_pairs_schedule_gn_step's return code."""
        L, p = self._lib, self._lib.ptr
        up, down, lmin = (float(x) for x in self.lm)
        return self.lib.sp_pairs_schedule_gn_step(ctypes.addressof(sched), self.n, self.max_N, up, down, lmin, p(self.lm_state), p(self.backup),
                                                  p(self.costs), p(self.phase), p(self.iters), ctypes.addressof(v) if v is not None else None,
                                                  L.stream_ptr())

    def launch(self):
        L, p = self._lib, self._lib.ptr
        up, down, lmin = (float(x) for x in self.lm)
        if self.entry == "gn":
            rc = self.lib.sp_pairs_gn_step(p(self.pairs), self.n, self.max_N, p(self.span), p(self.seg), up, down, lmin, p(self.lm_state),
                                           p(self.backup), p(self.costs), L.stream_ptr())
        elif self.entry == "conv":
            rc = self.lib.sp_pairs_gn_step_conv(p(self.pairs), self.n, self.max_N, p(self.span), p(self.seg), up, down, lmin, p(self.lm_state),
                                                p(self.backup), p(self.costs), float(self.conv_tol), p(self.done), L.stream_ptr())
        else:
            rc = self.call_sched_step(self.schedule(), self.verdict_struct())
        L.check(rc, self.entry)
        torch.cuda.synchronize()

    def run(self, check_every, max_rounds):
        """sp_pairs_schedule_run over the rig's pairs, no cost pass (n_spans = 0): (rounds, flag_host[0..7])."""
        L, p = self._lib, self._lib.ptr
        up, down, lmin = (float(x) for x in self.lm)
        sched, v = self.schedule(launched_spans=False), self.verdict_struct()
        flag_dev, flag_host = torch.full((8,), -1, dtype=torch.int32, device="cuda"), torch.full((8,), -1, dtype=torch.int32).pin_memory()
        rc = self.lib.sp_pairs_schedule_run(ctypes.addressof(sched), self.n, self.max_N, up, down, lmin, p(self.lm_state), p(self.backup), p(self.costs),
                                            p(self.phase), p(self.iters), int(check_every), int(max_rounds), p(flag_dev), flag_host.data_ptr(),
                                            ctypes.addressof(v) if v is not None else None, L.stream_ptr())
        torch.cuda.synchronize()
        return L.check_run(rc, "sp_pairs_schedule_run"), flag_host.numpy().copy()

    def run_queue(self, n_slots, check_every, max_rounds, lam0):
        """sp_pairs_schedule_run_queue: the rig's pairs wait in the queue, n_slots of them are worked on at a time (max_spans = 0: no cost
        pass).  Per-pair results land in the rig's pose / kld / status / diag / attempts / evals and in the returned q_lm / q_costs.
        Returns dict(rounds, head, slot_pair, q_lm, q_costs)."""
        L, p = self._lib, self._lib.ptr
        up, down, lmin = (float(x) for x in self.lm)
        rec = ctypes.sizeof(L.SpPair)
        slot_desc = self.pairs[:n_slots * rec].clone()
        sched, v = self.schedule(pairs_ptr=slot_desc.data_ptr(), launched_spans=False), self.verdict_struct()
        lm = np.zeros((n_slots, ref.LM), f32)
        lm[:, 0], lm[:, 1] = lam0, -1.0
        lm_state, backup, costs = T(lm), T(np.full((n_slots, 16 + self.max_N), SENTINEL, f32)), T(np.full(n_slots, SENTINEL, f32))
        phase, iters = T(np.full(n_slots, self.sched_entry, np.int32)), T(np.zeros(n_slots, np.int32))
        adam = T(np.zeros((n_slots, 2 + 2 * (self.max_N + 8)), f32))
        sched.adam_state = adam.data_ptr()
        head, slot_pair, active = T(np.array([n_slots], np.int32)), T(np.arange(n_slots, dtype=np.int32)), T(np.full(n_slots, -1, np.int32))
        q_costs, q_lm = T(np.full(self.n, SENTINEL, f32)), T(np.full((self.n, ref.LM), SENTINEL, f32))
        q = L.SpQueue()
        for k in range(len(self.phases)):
            q.qpairs[k], q.slot_pairs[k], q.max_spans[k] = self.pairs.data_ptr(), slot_desc.data_ptr(), 0
        q.n_queue, q.head, q.slot_pair, q.q_costs, q.q_lm, q.lam0, q.active = self.n, head.data_ptr(), slot_pair.data_ptr(), q_costs.data_ptr(), q_lm.data_ptr(), lam0, active.data_ptr()
        flag_dev, flag_host = torch.full((8,), -1, dtype=torch.int32, device="cuda"), torch.full((8,), -1, dtype=torch.int32).pin_memory()
        rc = self.lib.sp_pairs_schedule_run_queue(ctypes.addressof(sched), ctypes.addressof(q), n_slots, self.max_N, up, down, lmin, p(lm_state), p(backup),
                                                  p(costs), p(phase), p(iters), int(check_every), int(max_rounds), p(flag_dev), flag_host.data_ptr(),
                                                  ctypes.addressof(v) if v is not None else None, L.stream_ptr())
        torch.cuda.synchronize()
        return dict(rounds=L.check_run(rc, "sp_pairs_schedule_run_queue"), head=int(npy(head)[0]), slot_pair=npy(slot_pair).tolist(), q_lm=npy(q_lm), q_costs=npy(q_costs), phase=npy(phase).tolist(),
                    flag=flag_host.numpy().copy())

    def snapshot(self):
        """Every per-pair buffer a scheduled launch may write, as numpy arrays."""
        out = dict(pose=npy(self.pose), kld=npy(self.kld), lm_state=npy(self.lm_state), costs=npy(self.costs), phase=npy(self.phase), iters=npy(self.iters),
                   status=npy(self.status), diag=npy(self.diag), adam=npy(self.adam_state), backup=npy(self.backup))
        if self.attempts is not None:
            out["attempts"] = npy(self.attempts)
        if self.evals is not None:
            out["evals"] = npy(self.evals)
        return {k: v.copy() for k, v in out.items()}

    # -- one compared call -----------------------------------------------------------------------------------------------------------
    def step(self, exact=True, what=""):
        """Launch once, compare every pair with the reference, let the reference continue from the device's values.  Returns the
        reference's ``info`` of every pair."""
        infos = [{} for _ in range(self.n)]
        want = [self.expect(i, infos[i]) for i in range(self.n)]
        self.launch()
        kld, pose, lm, backup, costs = npy(self.kld), npy(self.pose), npy(self.lm_state), npy(self.backup), npy(self.costs)
        done, phase, iters, adam = npy(self.done), npy(self.phase), npy(self.iters), npy(self.adam_state)
        for span, seg in zip(self.spans, self.segs):
            assert np.array_equal(npy(span[0]), np.full(ref.NVP, GUARD, f32)) and np.array_equal(npy(seg[-1]), np.full(ref.NVS, GUARD, f32))
        worst = {}
        for i, (w, info) in enumerate(zip(want, infos)):
            tag, N, dec = f"{what} pair {i} ({info['decision']})", self.Ns[i], info["decision"]
            again = bool(info.get("verdict", {}).get("again"))             # restarted in this very launch: bitwise the initial values
            if dec in ("step", "adam"):
                assert info.get("cond", 1.0) <= 1e6, f"{tag}: condition number {info['cond']:.3g}"
            wk = np.full(self.max_N, SENTINEL, f32)
            wk[:N] = w["kld"]
            if dec == "adam" and not again:
                lr_p, lr_k = self.adam_lr
                dk, dp = np.abs(kld[i].astype(np.float64) - wk), np.abs(pose[i].astype(np.float64) - w["pose"].ravel())
                assert (dk <= 1e-6 * lr_k + np.spacing(np.abs(wk))).all(), f"{tag}: kld off by {dk.max():.3g}"
                assert (dp <= 1e-6 * lr_p + np.spacing(np.abs(w["pose"].ravel()))).all(), f"{tag}: pose off by {dp.max():.3g}"
                wa = ref.adam_moments(w, self.max_N)
                assert adam[i, 0] == wa[0] and adam[i, 1] == 0
                M = self.max_N               # each moment vector to 1e-6 of its own scale: a handful of float32 roundings per iteration
                for lo, hi in ((2, 2 + M), (2 + M, 2 + 2 * M), (2 + 2 * M, 8 + 2 * M), (8 + 2 * M, 14 + 2 * M), (14 + 2 * M, len(wa))):
                    np.testing.assert_allclose(adam[i, lo:hi], wa[lo:hi], rtol=1e-6, atol=1e-6 * np.abs(wa[lo:hi]).max(), err_msg=tag)
                for name, v in (("adam kld / lr", dk.max() / lr_k), ("adam pose / lr", dp.max() / lr_p)):
                    worst[name] = max(worst.get(name, 0.0), v)
            else:
                ulps = 2 if dec == "step" and not again else 0
                for name, got, exp in (("kld", kld[i], wk), ("pose", pose[i], w["pose"].ravel())):
                    d = same(got, exp, ulps)
                    worst[name] = max(worst.get(name, 0.0), float(d.max()))
                    assert d.max() <= ulps, f"{tag}: {name} off by {d.max():.3g} ulp at {d.argmax()}"
                # no Adam iteration: the moments are what they were (all zero until a pair's first one), or zero again after a restart
                assert np.array_equal(adam[i], np.zeros_like(adam[i]) if again else self.adam_prev[i]), f"{tag}: Adam moments"
            assert np.array_equal(backup[i], w["backup"]), f"{tag}: backup"
            for k in (0, 2, 3, 4, 7):
                assert lm[i, k] == w["lm_state"][k], f"{tag}: lm_state[{k}] {lm[i, k]} != {w['lm_state'][k]}"
            for name, got, exp in [(f"lm_state[{k}]", lm[i, k], w["lm_state"][k]) for k in (1, 5, 6)] + [("costs", costs[i], w["cost"])]:
                d = float(same(got, exp, 1).max())
                worst["cost"] = max(worst.get("cost", 0.0), d)
                assert d <= (0 if exact else 1), f"{tag}: {name} {got!r} != {exp!r} ({d:.3g} ulp)"
            if self.entry == "conv":
                assert done[i] == w["done"], f"{tag}: done"
            if self.entry == "sched":
                assert (phase[i], iters[i]) == (w["phase"], w["iters"]), f"{tag}: phase / iters {phase[i], iters[i]} != {w['phase'], w['iters']}"
            # the reference goes on from what the device holds
            w["kld"], w["pose"] = kld[i, :N].copy(), pose[i].reshape(4, 4).copy()
            w["lm_state"], w["cost"] = lm[i].copy(), costs[i]
        if self.entry == "sched" and "status" in want[0]:
            self.compare_verdict(want, infos, exact, what)
        self.adam_prev = adam.copy()
        print(f"{what}: worst distance from the reference (ulp) " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
        self.ref = want
        return infos

    def compare_verdict(self, want, infos, exact, what):
        """status, diag, attempts, evals of every pair and the sentinels around them: decisions, integers, diag[1, 3, 4, 6, 7] bitwise;
        diag[0, 2, 5] (copies of a cost / a valid fraction) by the cost rule."""
        status, diag = npy(self.status), npy(self.diag)
        assert status[0] == status[-1] == STATUS_SENTINEL and (diag[[0, -1]] == DIAG_SENTINEL).all(), f"{what}: a write outside the pairs' status / diag"
        for name, t in (("attempts", self.attempts), ("evals", self.evals)):
            if t is not None:
                assert (npy(t)[[0, -1]] == COUNT_SENTINEL).all(), f"{what}: a write outside the pairs' {name}"
        for i, (w, info) in enumerate(zip(want, infos)):
            tag = f"{what} pair {i} ({info['decision']}, verdict {info.get('verdict', {}).get('bits')})"
            if self.v is not None:
                assert status[i + 1] == w["status"], f"{tag}: status {status[i + 1]:#x} != {w['status']:#x}"
                for k in (1, 3, 4, 6, 7):
                    assert same(diag[i + 1, k], w["diag"][k], 0) == 0, f"{tag}: diag[{k}] {diag[i + 1, k]!r} != {w['diag'][k]!r}"
                for k in (0, 2, 5):
                    assert same(diag[i + 1, k], w["diag"][k], 1) <= (0 if exact else 1), f"{tag}: diag[{k}] {diag[i + 1, k]!r} != {w['diag'][k]!r}"
                if w["attempts"] is not None:
                    assert npy(self.attempts)[i + 1] == w["attempts"], f"{tag}: attempts"
                w["diag"] = diag[i + 1].copy()
            if w["evals"] is not None:
                assert np.array_equal(npy(self.evals)[i + 1], w["evals"]), f"{tag}: evals {npy(self.evals)[i + 1]} != {w['evals']}"
