"""Reference builders of the many-pairs work list and the padded table layout, in plain Python / numpy: what the library's host helpers
``sp_host_work_list`` and ``sp_host_layout`` (through ``optim.batch_prepare.flat_work_list`` / ``host_layout``) are tested against."""
import numpy as np

from super_primitive_amd.optim.pair_batch import GRANULE


def build_work_list(pads, span_points, tile_points):
    """Chunks {pair, seg, start, count}, spans {first chunk, n chunks, points, pair} and the per-pair record offsets of
    the many-pairs cost kernels (include/sp_hip.h, "Work list") for pairs whose padded layouts are ``pads``.
    Returns dict(chunks (C,4) int32, spans (S,4) int32, seg_rec_offs [per pair (N+1,) int32], c_off, s_off)."""
    chunk_max = max(GRANULE, tile_points // GRANULE * GRANULE)
    chunks, spans, seg_rec_offs, c_off, spans_per_pair = [], [], [], [0], []
    for m, pd in enumerate(pads):
        first = len(chunks)
        sto = [0]
        for n, (pc, off) in enumerate(zip(pd['pc'], pd['pseg_off'][:-1])):
            k = int(-(-pc // chunk_max))                       # pieces of (nearly) equal, granule-aligned length
            if k:
                per = int(-(-(pc // GRANULE) // k)) * GRANULE
                done = 0
                while done < pc:
                    cnt = int(min(per, pc - done))
                    chunks.append((m, n, int(off + done), cnt))
                    done += cnt
            sto.append(4 * (len(chunks) - first))              # records: 4 per chunk (one per wave)
        seg_rec_offs.append(np.asarray(sto, dtype=np.int32))
        c_off.append(len(chunks))
        # spans: greedy runs of consecutive chunks
        ns, q = 0, first
        while q < len(chunks):
            q1, pts = q, 0
            while q1 < len(chunks) and (q1 == q or pts + chunks[q1][3] <= span_points):
                pts += chunks[q1][3]
                q1 += 1
            spans.append((q, q1 - q, pts, m))
            ns += 1
            q = q1
        spans_per_pair.append(ns)
    return dict(chunks=np.asarray(chunks, dtype=np.int32).reshape(-1, 4), spans=np.asarray(spans, dtype=np.int32).reshape(-1, 4),
                seg_rec_offs=seg_rec_offs, c_off=c_off, s_off=np.concatenate(([0], np.cumsum(spans_per_pair))))


def flat_layout(counts, n_off, granule=GRANULE, table=None):
    """Padded layout of many tables at once.  counts: real points of every segment, all tables concatenated; n_off[t]:
    first segment of table t.  Returns (pc, seg_pos, p_off): padded run length of every segment, its position relative to
    its own table, and the tables' offsets into one flat array.  ``granule``: 256, or 64 for wave-span work lists."""
    counts = np.asarray(counts, dtype=np.int64)
    pc = (counts + granule - 1) // granule * granule
    cum = np.concatenate(([0], np.cumsum(pc)))
    p_off = cum[n_off]
    if table is None:
        table = np.repeat(np.arange(len(n_off) - 1), np.diff(n_off))
    return pc, cum[:-1] - p_off[table], p_off


def flat_work_list_numpy(pc, seg_pos, n_off, span_points, tile_points):
    """The same work list in vectorised numpy (the independent statement the host helper ``sp_host_work_list`` is tested against)."""
    pc = np.asarray(pc, dtype=np.int64)
    n_off = np.asarray(n_off, dtype=np.int64)
    M, S = len(n_off) - 1, len(pc)
    Ns = np.diff(n_off)
    pair_of_seg = np.repeat(np.arange(M), Ns)
    seg_in_pair = np.arange(S) - n_off[pair_of_seg]
    chunk_max = max(GRANULE, tile_points // GRANULE * GRANULE)
    k = -(-pc // chunk_max)                                                     # pieces per segment (0 for an empty one)
    per = -(-(pc // GRANULE) // np.maximum(k, 1)) * GRANULE                    # (nearly) equal, granule-aligned lengths
    cumk = np.concatenate(([0], np.cumsum(k)))
    C = int(cumk[-1])
    seg_idx = np.repeat(np.arange(S), k)
    j = np.arange(C) - cumk[:-1][seg_idx]
    start = seg_pos[seg_idx] + j * per[seg_idx]
    cnt = np.minimum(per[seg_idx], pc[seg_idx] - j * per[seg_idx])
    chunks = np.stack((pair_of_seg[seg_idx], seg_in_pair[seg_idx], start, cnt), axis=1).astype(np.int32)
    c_off = cumk[n_off]
    # per-pair CSR of the segment records: 4 records per chunk (one per wave)
    ext_pair = np.repeat(np.arange(M), Ns + 1)
    sto_off = n_off + np.arange(M + 1)
    ext_local = np.arange(S + M) - sto_off[:-1][ext_pair]
    seg_tile_off = (4 * (cumk[n_off[ext_pair] + ext_local] - cumk[n_off[ext_pair]])).astype(np.int32)
    # spans: greedy runs of consecutive chunks of one pair, all pairs advanced together
    cum = np.concatenate(([0], np.cumsum(cnt)))
    cur, end = c_off[:-1].copy(), c_off[1:]
    parts = []
    act = np.nonzero(cur < end)[0]
    while act.size:
        q0 = cur[act]
        q1 = np.searchsorted(cum, cum[q0] + span_points, side='right') - 1
        q1 = np.minimum(np.maximum(q1, q0 + 1), end[act])
        parts.append(np.stack((q0, q1 - q0, cum[q1] - cum[q0], act), axis=1))
        cur[act] = q1
        act = act[q1 < end[act]]
    spans = np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.int64)
    spans = spans[np.lexsort((spans[:, 0], spans[:, 3]))].astype(np.int32)
    s_off = np.concatenate(([0], np.cumsum(np.bincount(spans[:, 3], minlength=M))))
    return dict(chunks=chunks, spans=spans, seg_tile_off=seg_tile_off, sto_off=sto_off, c_off=c_off, s_off=s_off)
