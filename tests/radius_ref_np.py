"""Brute-force numpy restatement of the radius-search rule (include/slamfusion.h, sf_map_radius_search / sf_map_radius_graph), what
tests/test_gpu_radius_search.py compares against and tests/test_radius_rule.py pins to scipy: row i holds every indexed point the
window accepts with float32 d2 = ((dx*dx)+dy*dy)+dz*dz < float32(radius^2) (strict), the arithmetic of knn_ref in
tests/test_gpu_knn.py, over mp.index()["pts4"]; a non-finite query has an empty row.  "index" order: ascending position in the
index; "distance": ascending (bits of d2, position), the order of sf_map_knn.  Not a test module."""
import numpy as np


class HostIndex:
    """What radius_ref / knn_ref need of a Map, without a device: the finite points in their given order, ids bit-cast in column 3."""

    def __init__(self, points):
        x = np.asarray(points, np.float32).reshape(-1, 3)
        keep = np.flatnonzero(np.isfinite(x).all(1))
        self.pts4 = np.empty((len(keep), 4), np.float32)
        self.pts4[:, :3] = x[keep]
        self.pts4[:, 3] = keep.astype(np.uint32).view(np.float32)

    def index(self):
        return dict(pts4=self.pts4)


def radius_ref(mp, q, radius, order="index", accept=None, chunk=256):
    """-> offsets int64 [n + 1], idx int32 [total] (original ids), d2 float32 [total]; `accept` takes the points in index order."""
    pts4 = mp.index()["pts4"]
    P = np.ascontiguousarray(pts4[:, :3])
    ids = pts4[:, 3].view(np.uint32).astype(np.int64)
    q = np.asarray(q, np.float32).reshape(-1, 3)
    n, m = len(q), len(P)
    r2 = np.float32(float(radius) * float(radius))
    counts = np.zeros(n, np.int64)
    out_i, out_d = [], []
    if m > 0 and n > 0:
        ok_pt = np.ones(m, bool) if accept is None else accept(P)
        with np.errstate(invalid="ignore", over="ignore"):
            for s in range(0, n, chunk):
                c = q[s:s + chunk]
                dx, dy, dz = (c[:, None, d] - P[None, :, d] for d in range(3))
                d = ((dx * dx) + dy * dy) + dz * dz
                assert d.dtype == np.float32
                ok = (d < r2) & ok_pt[None, :] & np.isfinite(c).all(1)[:, None]
                rows, cols = np.nonzero(ok)                                   # row-major: ascending position inside a row
                dd = d[rows, cols]
                if order == "distance":
                    o = np.lexsort((cols, dd.view(np.uint32), rows))
                    rows, cols, dd = rows[o], cols[o], dd[o]
                else:
                    assert order == "index", order
                counts[s:s + chunk] = ok.sum(1)
                out_i.append(ids[cols].astype(np.int32))
                out_d.append(dd)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    idx = np.concatenate(out_i) if out_i else np.empty(0, np.int32)
    d2 = np.concatenate(out_d) if out_d else np.empty(0, np.float32)
    return offsets, idx.astype(np.int32), d2.astype(np.float32)


def rows_cut(offsets, idx, d2, k):
    """The first k entries of every row as sf_map_knn lays them out: idx [n, k] (-1 tails), d2 [n, k] (inf tails), count [n]."""
    n = len(offsets) - 1
    cnt = np.minimum(np.diff(offsets), k).astype(np.int32)
    oi = np.full((n, k), -1, np.int32)
    od = np.full((n, k), np.inf, np.float32)
    col = np.arange(k)[None, :]
    take = col < cnt[:, None]
    src = (offsets[:-1, None] + col)[take]
    oi[take] = idx[src]
    od[take] = d2[src]
    return oi, od, cnt
