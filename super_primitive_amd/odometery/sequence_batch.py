"""S odometry sequences in LOCKSTEP: the throughput form of config 3 (the MonoVO chain, ``sequence.py``).

One sequence leaves the GPU nearly idle -- its frame is a chain of small dependent launches.  ``run_sequences``
walks the frame indices of S sequences together and, at every index, hands the per-frame stages of all sequences that can take them to
ONE ``sp_chain_step_multi`` call per stage mask (``chain.ChainStepBatch``), and the scheduled mappings that fall on that index to
``PoseWindowBatch`` (one Gauss-Newton phase loop over all their windows).  Everything else -- sequences before their first mapping,
window builds, keyframe creation -- runs per sequence exactly as ``MonoVO.step`` does (whose native step is the same call on the sequence's
one record).  Per sequence the results are bitwise those of ``run_sequence`` on it alone (tests/test_gpu_sequence_batch.py)."""
from __future__ import annotations

import time

import torch

from ..optim.window import PoseWindowBatch
from .loops import map_window_gn_begin, map_window_gn_end, map_window_gn_phases, run_gn_phases
from .sequence import DEFAULTS, MonoVO

_LDS_Y = 192          # PoseWindowBatch: windows of at most this many camera unknowns, or all above, ride together


def _sync():
    torch.cuda.current_stream().synchronize()


def _check(sequences, engine, cfg):
    if engine != "gn":
        raise ValueError(f"run_sequences: engine {engine!r}: only the Gauss-Newton engine ('gn') runs in lockstep")
    c = dict(DEFAULTS, **cfg)
    if not c['native_step']:
        raise ValueError("run_sequences: native_step=False: the lockstep path is the native step's")
    if c['motion_prior']:
        raise ValueError("run_sequences: motion_prior is not supported in lockstep")
    if not sequences:
        raise ValueError("run_sequences: no sequences")
    sizes = {tuple(s['frames'][0].image.shape[-2:]) for s in sequences}
    if len(sizes) != 1:
        raise ValueError(f"run_sequences: frames of different sizes {sorted(sizes)}")


def _run_mappings(due, counters):
    """The scheduled mappings of the sequences in ``due`` (MonoVO objects), their Gauss-Newton phases side by side where
    ``PoseWindowBatch`` takes them (windows that need the depths-fixed flag, or that are alone in their size class, run alone)."""
    parts = []
    for mvo in due:
        ctx, (args, kw) = mvo._map_begin_scheduled()
        parts.append((mvo, ctx, map_window_gn_begin(*args, **kw)))
    groups = {}
    for mvo, ctx, m in parts:
        win = m['win']
        if win is None:
            continue
        key = (None, id(m)) if win.depths_fixed else (win.gn_unknowns > _LDS_Y, tuple(map_window_gn_phases(m)))
        groups.setdefault(key, []).append(m)
    for key, ms in groups.items():
        phases = map_window_gn_phases(ms[0])
        if len(ms) >= 2:
            batch = PoseWindowBatch([m['win'] for m in ms])
            for level, n, eps, tol in phases:
                batch.run_gn(level, n, irls_eps=eps, conv_tol=tol)
            counters['mapping_batches'] += 1
            counters['windows_per_batch'].append(len(ms))
        else:
            run_gn_phases(ms[0]['win'], phases)
            counters['mappings_alone'] += 1
        for m in ms:
            m['n'] = m['win'].gn_iterations()        # (the pinned copy the run's last poll left: no read-back)
    for mvo, ctx, m in parts:
        mvo._mapping_end(ctx, map_window_gn_end(m))
        mvo._mapping_done()


def _run_chain(batch, jobs, counters):
    """jobs: {sequence index: ChainStep.run keywords}; one multi call per stage mask.  Returns {sequence index: criterion | None}."""
    by_mask = {}
    for k, kw in jobs.items():
        by_mask.setdefault(int(kw['stages']), []).append(k)
    out = {}
    for ks in by_mask.values():
        res = batch.run([(jobs[k]['_chain'], {a: b for a, b in jobs[k].items() if a != '_chain'}) for k in ks])
        counters['multi_calls'] += 1
        counters['sequences_per_call'].append(len(ks))
        for k, (_, _, crit) in zip(ks, res):
            out[k] = crit
    return out


def run_sequences(sequences, engine="gn", stats=None, **cfg):
    """sequences: [dict(frames, to_keyframe, pose0, kld0, depth_of=None, log=None)] -- ``run_sequence``'s arguments per sequence; ``cfg``
    (``DEFAULTS`` overrides) is shared by all.  Returns one result dict per sequence with ``run_sequence``'s keys; ``seconds`` is the
    SHARED wall time split per stage (native calls, per-sequence steps, mappings, keyframe work), the same dict for every sequence.
    ``stats``: an optional dict that receives the counters (multi calls, sequences per call, mapping batches, windows per batch)."""
    _check(sequences, engine, cfg)
    from .chain import ChainStepBatch
    mvos = [MonoVO(s['frames'], s['to_keyframe'], s['pose0'], s['kld0'], engine="gn", log=s.get('log'), depth_of=s.get('depth_of'), **cfg)
            for s in sequences]
    if not all(m.native for m in mvos):
        raise ValueError("run_sequences: the sequences must live on a GPU (the native step)")
    batch = ChainStepBatch(mvos[0].dev)
    counters = dict(multi_calls=0, sequences_per_call=[], mapping_batches=0, windows_per_batch=[], mappings_alone=0, steps_alone=0)
    secs = dict(native_begin=0.0, native_call=0.0, native_end=0.0, alone=0.0, mapping=0.0, criterion_call=0.0, keyframe=0.0)
    n_max = max(len(m.frames) for m in mvos)
    _sync()
    for i in range(1, n_max):
        active = [k for k, m in enumerate(mvos) if i < len(m.frames)]
        lock = [k for k in active if mvos[k].initialised]
        # (2) sequences the native step does not cover yet: alone, as MonoVO.step
        t0 = time.perf_counter()
        for k in active:
            if k not in lock:
                mvos[k].step(i)
                counters['steps_alone'] += 1
        _sync(); t1 = time.perf_counter(); secs['alone'] += t1 - t0
        if not lock:
            continue
        # (1) the per-frame stages: one multi call per stage mask
        jobs = {}
        for k in lock:
            kw = mvos[k]._native_begin(i)
            kw['_chain'] = mvos[k].chain
            jobs[k] = kw
        t2 = time.perf_counter(); secs['native_begin'] += t2 - t1
        crit = _run_chain(batch, jobs, counters)
        t3 = time.perf_counter(); secs['native_call'] += t3 - t2
        for k in lock:
            mvos[k]._native_end(i)
        t4 = time.perf_counter(); secs['native_end'] += t4 - t3
        # (3) the scheduled mappings due at this index, side by side
        due = [mvos[k] for k in lock if mvos[k]._mapping_due()]
        if due:
            _run_mappings(due, counters)
        _sync(); t5 = time.perf_counter(); secs['mapping'] += t5 - t4
        # (4) the criterion-only call of the sequences whose first call had none
        late = {}
        for k in lock:
            if crit[k] is None:
                kw = mvos[k]._native_criterion_job()
                kw['_chain'] = mvos[k].chain
                late[k] = kw
        if late:
            crit.update(_run_chain(batch, late, counters))
        t6 = time.perf_counter(); secs['criterion_call'] += t6 - t5
        # (5) keyframe decisions and new keyframes, per sequence
        for k in lock:
            assert mvos[k].current_ts == i
            mvos[k]._native_keyframe(i, crit[k])
        _sync(); secs['keyframe'] += time.perf_counter() - t6
    if stats is not None:
        stats.update(counters)
    out = []
    for m in mvos:
        r = m.result()
        r['seconds'] = secs
        out.append(r)
    return out
