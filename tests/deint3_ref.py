"""A numpy restatement of the motion-adaptive deinterlacer D3, written from INTEGRATION.md "Deinterlaced output" (not from the kernel): shared by
test_deint3_host.py and test_deint3_gpu.py."""
import numpy as np

from deint_ref import join_frame, split_frame


def deint3_plane(P, Q, p, T=10, stats=None):
    """D3 on one plane P (H x W, uint8) against the same plane Q of the previous display frame: rows of parity p are kept; a missing sample is the
    average of the kept rows above and below where any of the nine |P - Q| around it exceeds T, and P's own sample elsewhere.
    stats: a list that gets (missing-row samples, moving ones) per missing row."""
    P = np.asarray(P, dtype=np.uint8)
    Q = np.asarray(Q, dtype=np.uint8)
    assert P.shape == Q.shape
    H, W = P.shape
    assert H >= 2
    D = P.copy()
    Pi = P.astype(np.int64)
    m = np.abs(Pi - Q.astype(np.int64)) > T
    xs = np.arange(W)
    for y in range(H):
        if (y & 1) == p:
            continue
        up = y - 1 if y - 1 >= 0 else y + 1
        dn = y + 1 if y + 1 < H else y - 1
        i = (Pi[up] + Pi[dn] + 1) >> 1
        moving = np.zeros(W, bool)
        for r in (up, y, dn):
            for k in (-1, 0, 1):
                moving |= m[r][np.clip(xs + k, 0, W - 1)]
        if stats is not None:
            stats.append((W, int(moving.sum())))
        D[y] = np.where(moving, i, Pi[y])
    return D


def deint3_frame(buf, prev, w, h, fmt, p, T=10, stats=None):
    """D3 on a tight frame against the previous tight frame: every plane on its own, the same kept parity.
    stats: {"luma": [...], "chroma": [...]} as deint3_plane's."""
    Y, U, V = split_frame(buf, w, h, fmt)
    Yq, Uq, Vq = split_frame(prev, w, h, fmt)
    sl = stats["luma"] if stats is not None else None
    sc = stats["chroma"] if stats is not None else None
    return join_frame(deint3_plane(Y, Yq, p, T, sl), deint3_plane(U, Uq, p, T, sc), deint3_plane(V, Vq, p, T, sc), fmt)


def moving_share(st):
    n = sum(a for a, _ in st)
    return sum(b for _, b in st) / n if n else 0.0
