"""-m gpu: S odometry sequences in lockstep (``odometery.sequence_batch.run_sequences``, ``chain.ChainStepBatch`` /
``sp_chain_step_multi``): every sequence's result is bitwise what ``run_sequence`` gives on it alone."""
import pytest
import torch

from gpu_util import T
from test_gpu_sequence import make_sequence_inputs

pytestmark = pytest.mark.gpu

CFG = dict(window_size=3, translation_thresh=0.1)


def _inputs(seed, n=30, cut=None):
    seq, frames, to_kf = make_sequence_inputs(n=n, seed=seed)
    if cut is not None:
        frames = frames[:cut]
    return dict(frames=frames, to_keyframe=to_kf, pose0=T(seq[0].T_wc), kld0=T(seq[0].kld_gt), depth_of=lambda i, s=seq: T(s[i].kld_gt))


def _assert_same(a, b, what):
    assert torch.equal(a['track_poses'], b['track_poses']), what
    assert torch.equal(a['kf_poses'], b['kf_poses']), what
    for key in ('kf_ids', 'all_kf_ids', 'supp_ids', 'n_mappings', 'n_supp_mappings', 'n_init_mappings'):
        assert a[key] == b[key], (what, key, a[key], b[key])
    for key in ('kf_klds', 'kf_affs'):
        assert len(a[key]) == len(b[key]), (what, key)
        for x, y in zip(a[key], b[key]):
            assert torch.equal(x, y), (what, key)


def _alone(s):
    from super_primitive_amd.odometery.sequence import run_sequence
    return run_sequence(s['frames'], s['to_keyframe'], s['pose0'], s['kld0'], engine="gn", depth_of=s['depth_of'], **CFG)


def test_lockstep_equals_alone_bitwise():
    from super_primitive_amd.odometery.sequence_batch import run_sequences
    a, b, c = _inputs(31), _inputs(32), _inputs(33)
    dup = dict(a)                                            # the same inputs twice: their mappings fall on the same frame indices
    ragged = _inputs(34, cut=18)                             # ~60 % of the length: drops out while the others go on
    seqs = [a, b, c, dup, ragged]
    stats = {}
    outs = run_sequences(seqs, engine="gn", stats=stats, **CFG)
    alone = [_alone(s) for s in seqs]
    for k, (x, y) in enumerate(zip(outs, alone)):
        _assert_same(x, y, f"sequence {k}")
    assert all(len(o['track_poses']) == len(s['frames']) for o, s in zip(outs, seqs))
    assert len(alone[0]['all_kf_ids']) >= 3 and alone[0]['n_mappings'] >= 2, alone[0]['all_kf_ids']
    assert max(stats['sequences_per_call']) >= 4, stats
    assert stats['mapping_batches'] >= 1 and max(stats['windows_per_batch']) >= 2, stats
    print(f"\nlockstep: {stats['multi_calls']} multi calls (sequences per call: max {max(stats['sequences_per_call'])}), "
          f"{stats['mapping_batches']} mapping batches (windows: {stats['windows_per_batch']}), {stats['mappings_alone']} mappings alone")


def _advanced(seeds, upto):
    """MonoVO objects of the given sequences, stepped through frames 1 .. upto - 1."""
    from super_primitive_amd.odometery.sequence import MonoVO
    mvos = []
    for seed in seeds:
        s = _inputs(seed)
        m = MonoVO(s['frames'], s['to_keyframe'], s['pose0'], s['kld0'], engine="gn", depth_of=s['depth_of'], **CFG)
        for i in range(1, upto):
            m.step(i)
        mvos.append(m)
    return mvos


@pytest.mark.parametrize("upto", [3, 8])
def test_one_frame_per_record(upto):
    from super_primitive_amd.odometery.chain import ChainStepBatch
    seeds = [31, 32, 33, 31]
    ref, lock = _advanced(seeds, upto), _advanced(seeds, upto)
    i = upto
    res_ref = []
    for m in ref:
        job = m._native_begin(i)
        res_ref.append((job['stages'], m.chain.run(**job)))
    # (one call per stage mask, as run_sequences groups them; _native_begin once per sequence -- it moves the running frames' slots)
    groups = {}
    for k, m in enumerate(lock):
        job = m._native_begin(i)
        groups.setdefault(int(job['stages']), []).append((k, job))
    res_lock = {}
    batch = ChainStepBatch(lock[0].dev)
    for stages, kjobs in groups.items():
        for (k, _), r in zip(kjobs, batch.run([(lock[k].chain, job) for k, job in kjobs])):
            res_lock[k] = (stages, r)
    for k, (m_ref, m_lock) in enumerate(zip(ref, lock)):
        (s_ref, (ti_r, si_r, c_r)), (s_lock, (ti_l, si_l, c_l)) = res_ref[k], res_lock[k]
        assert s_ref == s_lock
        assert torch.equal(m_ref.chain.hist_pose[i], m_lock.chain.hist_pose[i]), k
        assert torch.equal(m_ref.chain.hist_aff[i], m_lock.chain.hist_aff[i]), k
        assert (ti_r, si_r) == (ti_l, si_l), k
        assert c_r == c_l, k
        if m_ref.chain.mapper is not None:
            assert torch.equal(m_ref.chain.mapper.win.kld, m_lock.chain.mapper.win.kld), k
            assert torch.equal(m_ref.chain.tracker.win.kld, m_lock.chain.tracker.win.kld), k
            assert torch.equal(m_ref.chain.mapper.win.nodes, m_lock.chain.mapper.win.nodes), k
    assert batch.sizes and max(batch.sizes) >= 2


def test_single_sequence_through_lockstep():
    from super_primitive_amd.odometery.sequence_batch import run_sequences
    s = _inputs(35)
    (out,) = run_sequences([s], engine="gn", **CFG)
    _assert_same(out, _alone(s), "S = 1")
