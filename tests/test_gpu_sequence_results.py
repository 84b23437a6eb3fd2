"""-m gpu: what a sequence reports (``odometery/sequence.py`` ``result()['kf_trajectory']`` / ``['kf_archive']``,
``odometery/results.py`` ``sequence_map``) on the 30-frame 224x288x40 sequence of tests/test_gpu_sequence.py with a window of TWO
keyframes, so that keyframes retire: the keyframe trajectory against the mapping log, the archive against the values a keyframe held when
it left the window, the three drivers (native step, step by step, lockstep) against each other, and the aligned world map."""
import numpy as np
import pytest
import torch

import traj_align_ref as ref
from gpu_util import T, npy
from test_gpu_sequence import make_sequence_inputs

pytestmark = pytest.mark.gpu

CFG = dict(window_size=2, translation_thresh=0.1)


def _recording_vo():
    from super_primitive_amd.odometery.sequence import MonoVO

    class Recording(MonoVO):
        """Copies of what the oldest keyframe holds, taken just before it leaves the window."""

        def pop_kf(self, i):
            self.__dict__.setdefault("popped", {})[self.kf_ids[i]] = (self.kf_poses[i].clone(), self.kf_klds[i].clone(), self.kf_affs[i].clone(), self.kfs[i])
            super().pop_kf(i)

    return Recording


@pytest.fixture(scope="module")
def runs():
    """The runs every test below looks at, made once: 'native' (30 frames, keep_keyframes, log, pops recorded), 'short' (20 frames of
    another sequence), 'steps' (the 30 frames step by step, default storage), 'lockstep' (both sequences through run_sequences)."""
    from super_primitive_amd.odometery.sequence import run_sequence
    from super_primitive_amd.odometery.sequence_batch import run_sequences
    seq, frames, to_kf = make_sequence_inputs()
    seq2, frames2, to_kf2 = make_sequence_inputs(n=20, seed=32)
    pose0, kld0 = T(seq[0].T_wc), T(seq[0].kld_gt)
    log = []
    vo = _recording_vo()(frames, to_kf, pose0, kld0, engine="gn", log=log, keep_keyframes=True, **CFG)
    native = vo.run()
    short = run_sequence(frames2, to_kf2, T(seq2[0].T_wc), T(seq2[0].kld_gt), engine="gn", keep_keyframes=True, **CFG)
    steps = run_sequence(frames, to_kf, pose0, kld0, engine="gn", native_step=False, **CFG)
    lockstep = run_sequences([dict(frames=frames, to_keyframe=to_kf, pose0=pose0, kld0=kld0),
                              dict(frames=frames2, to_keyframe=to_kf2, pose0=T(seq2[0].T_wc), kld0=T(seq2[0].kld_gt))], engine="gn", keep_keyframes=True, **CFG)
    torch.cuda.synchronize()
    return dict(seq=seq, pose0=pose0, log=log, popped=vo.popped, native=native, short=short, steps=steps, lockstep=lockstep)


def test_keyframe_trajectory_follows_the_mapping_log(runs):
    out, log = runs['native'], runs['log']
    last = {}
    for _, ev, d in log:
        if ev == 'mapping':
            for i, p in zip(d['kf_ids'], d['kf_poses']):
                last[i] = p
    assert len(out['all_kf_ids']) >= 4 and len(runs['popped']) >= 2, out['all_kf_ids']            # keyframes retired
    traj = out['kf_trajectory']
    assert set(traj) == set(last) | {0}
    for i, pose in traj.items():
        assert pose.shape == (4, 4) and pose.is_cuda
        assert torch.equal(pose, last[i] if i in last else runs['pose0']), i
    # a keyframe no scheduled mapping saw is absent; every other one is there
    assert set(out['all_kf_ids']) - set(traj) <= {out['all_kf_ids'][-1]}
    # existing keys untouched
    assert out['kf_ids'] == out['all_kf_ids'][-2:] and out['kf_poses'].shape == (2, 4, 4)


def test_archive_holds_what_a_keyframe_held_when_it_retired(runs):
    out, popped = runs['native'], runs['popped']
    arch = out['kf_archive']
    assert list(arch) == out['all_kf_ids'] and set(popped) == set(out['all_kf_ids'][:-2])
    for i, (pose, kld, aff, kf) in popped.items():
        e = arch[i]
        assert set(e) == {'pose', 'kld', 'aff', 'kf'}
        assert torch.equal(e['pose'], pose) and torch.equal(e['kld'], kld) and torch.equal(e['aff'], aff), i
        assert e['kf'] is kf
    for k, i in enumerate(out['kf_ids']):                       # window keyframes: the current values
        e = arch[i]
        assert torch.equal(e['pose'], out['kf_poses'][k]) and e['kld'] is out['kf_klds'][k] and e['aff'] is out['kf_affs'][k]


def test_step_by_step_path_gives_the_same_results(runs):
    a, b = runs['steps'], runs['native']
    assert sorted(a['kf_trajectory']) == sorted(b['kf_trajectory']) and list(a['kf_archive']) == list(b['kf_archive'])
    dp = max(float((a['kf_trajectory'][i] - b['kf_trajectory'][i]).abs().max()) for i in a['kf_trajectory'])
    da = max(float((a['kf_archive'][i]['pose'] - b['kf_archive'][i]['pose']).abs().max()) for i in a['kf_archive'])
    assert dp <= 5e-6 and da <= 5e-6, (dp, da)


def test_lockstep_gives_the_single_runs_bitwise(runs):
    for alone, lock in zip((runs['native'], runs['short']), runs['lockstep']):
        assert sorted(alone['kf_trajectory']) == sorted(lock['kf_trajectory']) and list(alone['kf_archive']) == list(lock['kf_archive'])
        assert len(alone['kf_archive']) >= 3
        for i in alone['kf_trajectory']:
            assert torch.equal(alone['kf_trajectory'][i], lock['kf_trajectory'][i]), i
        for i, e in alone['kf_archive'].items():
            for key in ('pose', 'kld', 'aff'):
                assert torch.equal(e[key], lock['kf_archive'][i][key]), (i, key)
            assert lock['kf_archive'][i]['kf'] is not None


def test_keyframes_are_stored_on_request_only(runs):
    from super_primitive_amd.image.keyframe import KeyFrame
    from super_primitive_amd.odometery.results import sequence_map
    assert all(e['kf'] is None for e in runs['steps']['kf_archive'].values())
    arch = runs['native']['kf_archive']
    assert all(isinstance(arch[i]['kf'], KeyFrame) for i in runs['popped'])
    with pytest.raises(ValueError, match="keep_keyframes"):
        sequence_map(runs['steps'], 4)


def test_sequence_map_aligned_against_the_ground_truth(runs):
    from super_primitive_amd.core.dense_optim import unproject_kf
    from super_primitive_amd.odometery.results import sequence_map
    out, seq = runs['native'], runs['seq']
    G = np.stack([f.T_wc for f in seq]).astype(np.float32)
    m = sequence_map(out, stride=4, gt_poses=T(G))
    torch.cuda.synchronize()
    arch = out['kf_archive']
    ids = sorted(arch)
    assert m['ids'] == ids
    Q = [-(-int(arch[i]['kf'].keypoint_regions.sum()) // 4) for i in ids]
    assert m['points'].shape == (sum(Q), 3) and m['offsets'].tolist() == np.concatenate(([0], np.cumsum(Q))).tolist()
    # both absolute trajectory errors against the restatement on the same trajectories, at the alignment tolerance
    traj_ids = sorted(out['kf_trajectory'])
    assert m['traj_ids'] == traj_ids and len(traj_ids) >= 3
    pred = np.stack([npy(out['kf_trajectory'][i]) for i in traj_ids])
    want, spread = ref.permutation_spread(pred, G[traj_ids], anchor_rotation=True)
    tol = ref.tolerance(spread)
    got = {f: npy(m['align'][f][0]) for f in ('rot', 'trans_scaled', 's', 'rot_reanchor')}
    print(f"\nsequence map: {sum(Q)} points of {len(ids)} keyframes; trajectory of {len(traj_ids)} keyframes, condition {ref.condition(pred, G[traj_ids]):.3f}; "
          f"ATE with scale {float(m['ate_scaled']):.3e} (restatement {want['ate_scaled']:.3e}), without {float(m['ate']):.3e} ({want['ate']:.3e}); scale {float(got['s']):.5f}")
    assert abs(float(m['ate_scaled']) - want['ate_scaled']) <= tol['ate_scaled'] and abs(float(m['ate']) - want['ate']) <= tol['ate']
    # the aligned points against the float64 formula on the bitwise-known camera points
    rec = {f: got[f] for f in got}
    for k, i in enumerate(ids):
        a, b = int(m['offsets'][k]), int(m['offsets'][k + 1])
        p = npy(unproject_kf(arch[i]['kf'], arch[i]['kld'])['src_pts'][::4])
        world, bound = ref.world_points(p, npy(arch[i]['pose']), rec)
        err = np.abs(npy(m['points'][a:b]).astype(np.float64) - world).max(1)
        assert np.all(err <= bound), (i, float((err / bound).max()))
        assert bool((m['kf_index'][a:b] == k).all())
    # without ground truth: the map in the sequence's own frame, no alignment keys
    plain = sequence_map(out, stride=4)
    assert 'align' not in plain and plain['points'].shape == m['points'].shape and torch.equal(plain['colours'], m['colours'])
