# S copies of one resident sequence through run_sequences, for a kernel trace of the lockstep path (the dispatches per frame index at S = 1
# and S = 16):  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/lockstep_trace.py S n_frames
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
from test_gpu_sequence import make_sequence_inputs, T
from super_primitive_amd.image.keyframe import KeyFrame
from super_primitive_amd.odometery.sequence_batch import run_sequences
S, n = int(sys.argv[1]), int(sys.argv[2])
seq, frames, _ = make_sequence_inputs(n, rot_scale=0.3, seed=100)
res = [(T(f.image), T(f.K), T(f.logdepth_perseg), T(f.keypoints), T(f.keypoint_regions)) for f in seq]
seqs = [dict(frames=frames, to_keyframe=lambda i: KeyFrame(*res[i]), pose0=T(seq[0].T_wc), kld0=T(seq[0].kld_gt), depth_of=lambda i: T(seq[i].kld_gt))
        for _ in range(S)]
st = {}
run_sequences(seqs, stats=st, translation_thresh=0.095, window_size=5)
torch.cuda.synchronize()
print("STATS", S, n, st['multi_calls'], st['mapping_batches'], st['windows_per_batch'])
