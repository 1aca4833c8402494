"""NumPy / float64 restatement of chunked inference and its stitching (``inference.chunk_plan``, ``pe_stitch_chunks``),
written frame by frame from the rule and not from the plan's runs.

Chunk k of a row of ``n_frames`` frames starts at ``s_k = k * max(chunk_size - overlap, 1)`` (while ``s_k < n_frames``)
and is valid over ``[s_k, e_k)``, ``e_k = min(s_k + chunk_size, n_frames)``.  A stitch is described per OUTPUT frame by
``(a, fa, b, fb, w)``: the output is frame ``fa`` of chunk ``a``; where ``b >= 0`` it is blended with frame ``fb`` of
chunk ``b`` as ``A + w (B - A)``, ``w`` a float32."""
import numpy as np


def chunk_spans(n_frames, chunk_size, overlap):
    step = max(chunk_size - overlap, 1)
    return [(s, min(s + chunk_size, n_frames)) for s in range(0, n_frames, step)]


def owners(n_frames, chunk_size, overlap):
    """Owner chunk of every frame in "center" mode: the covering chunk with the smallest
    ``|2 (t - s_k) - (chunk_size - 1)|``, the smaller k on a tie (``argmin`` returns the first minimum)."""
    spans = chunk_spans(n_frames, chunk_size, overlap)
    t = np.arange(n_frames)
    cost = np.full((len(spans), n_frames), np.inf)
    for k, (s, e) in enumerate(spans):
        cost[k, s:e] = np.abs(2 * (t[s:e] - s) - (chunk_size - 1))
    return np.argmin(cost, axis=0)


def crossfade_weight(j, n_ov):
    """float32 ``(j + 1) / (n_ov + 1)``."""
    return np.float32(j + 1) / np.float32(n_ov + 1)


def frame_map(n_frames, chunk_size, overlap, mode):
    """int64 ``(n_out, 4)`` rows ``(a, fa, b, fb)`` and float32 ``(n_out,)`` weights (0 where ``b == -1``)."""
    spans = chunk_spans(n_frames, chunk_size, overlap)
    rows, w = [], []
    if mode == "concat":
        for k, (s, e) in enumerate(spans):
            rows += [(k, f, -1, 0) for f in range(e - s)]
        return np.array(rows, np.int64).reshape(-1, 4), np.zeros(len(rows), np.float32)
    if mode == "center":
        own = owners(n_frames, chunk_size, overlap)
        rows = [(int(k), t - spans[k][0], -1, 0) for t, k in enumerate(own)]
        return np.array(rows, np.int64).reshape(-1, 4), np.zeros(len(rows), np.float32)
    assert mode == "crossfade" and 2 * overlap <= chunk_size
    for t in range(n_frames):
        cover = [k for k, (s, e) in enumerate(spans) if s <= t < e]
        assert 1 <= len(cover) <= 2
        if len(cover) == 1:
            rows.append((cover[0], t - spans[cover[0]][0], -1, 0))
            w.append(np.float32(0))
        else:
            k, k1 = cover
            assert k1 == k + 1
            n_ov, j = spans[k][1] - spans[k1][0], t - spans[k1][0]
            rows.append((k, t - spans[k][0], k1, j))
            w.append(crossfade_weight(j, n_ov))
    return np.array(rows, np.int64).reshape(-1, 4), np.array(w, np.float32)


def stitch(chunks, n_frames, chunk_size, overlap, mode):
    """``chunks`` (K, chunk_size[, C]) of one row, K the rule's chunk count -> ``(out, scale)``: the stitched row --
    copies keep the dtype and the bits, "crossfade" is evaluated in float64 -- and ``|A| + |B|`` on blended elements
    (0 on copied ones), which scales the float32 rounding bound ``4 * 2^-24 * (|A| + |B|)`` of ``A + w (B - A)``."""
    chunks = np.asarray(chunks)
    fm, w = frame_map(n_frames, chunk_size, overlap, mode)
    A = chunks[fm[:, 0], fm[:, 1]]
    if mode != "crossfade":
        return A.copy(), np.zeros(A.shape)
    seam = fm[:, 2] >= 0
    B = chunks[np.maximum(fm[:, 2], 0), fm[:, 3]].astype(np.float64)
    A = A.astype(np.float64)
    ww = w.astype(np.float64).reshape((-1,) + (1,) * (A.ndim - 1))
    sm = seam.reshape(ww.shape)
    return np.where(sm, A + ww * (B - A), A), np.where(sm, np.abs(A) + np.abs(B), 0.0)


def plan_frame_map(plan, r):
    """The same description read off row ``r`` of an ``inference.chunk_plan``: its runs expanded frame by frame, chunk
    numbers mapped back to the rule's through the row's ``kept``.  Also checks that the runs tile the row's output:
    every output frame exactly once."""
    row = plan["rows"][r]
    kept = np.asarray(row["kept"], np.int64)
    base = row["chunks"][0]
    runs = plan["runs"][row["runs"][0]:row["runs"][1]]
    rows, w = [], []
    at = row["out_offset"]
    for a, fa, dst, n, n_ov, j0, b, fb in runs.tolist():
        assert dst == at and n >= 1, "runs leave a gap or overlap"
        at += n
        for i in range(n):
            if n_ov:
                rows.append((kept[a - base], fa + i, kept[b - base], fb + i))
                w.append(crossfade_weight(j0 + i, n_ov))
            else:
                rows.append((kept[a - base], fa + i, -1, 0))
                w.append(np.float32(0))
    assert at == row["out_offset"] + row["out_len"]
    return np.array(rows, np.int64).reshape(-1, 4), np.array(w, np.float32)
