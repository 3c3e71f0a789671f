"""numpy reference of the per-Gaussian importance scores (gsr_forward_scores), no GPU.

From an `oracle.forward(...)` state -- its sorted list, tile ranges and preprocess outputs -- every
tile's list is replayed over the tile's 256 pixels in float32 in the oracle's operation order
(oracle/gsr_oracle.c blend_tile): power, exp, min(0.99, .), the power > 0 and alpha < 1/255
rejections, the T (1 - alpha) < 1e-4 termination.  The tiles of a block advance one list entry per
step, so a block costs as many steps of array operations as its longest list has entries.

Besides the three scores, every Gaussian gets the smallest relative distance of any of its examined
(pixel, Gaussian) pairs to a decision threshold, |alpha - 1/255| / (1/255) and
|T (1 - alpha) - 1e-4| / 1e-4: a pair nearer than the arithmetic difference between this replay
(exp) and the kernels (exp2 of a pre-scaled exponent) can fall on either side, and the GPU tests
exclude such Gaussians from the value comparison (and bound how many there may be).
"""
from __future__ import annotations

import numpy as np

TILE = 16
NEAR = 1e-3  # a pair within this relative distance of a threshold counts as "near"


def scores(state) -> dict:
    """state: oracle.forward(...).state.  Returns
      max_w (P,) float32, sum_w (P,) float64 (float32 terms accumulated in float64), hits (P,) int64,
      dist (P,) float64: the Gaussian's smallest threshold distance (inf: no examined pair),
      near_pairs: examined pairs within NEAR of a threshold, examined_pairs: all examined pairs,
      pix_sum_w (H, W) and pix_hits (H, W): per pixel, the float32 sum of w and the contributing pairs."""
    cam = state.cam
    H, W = cam.height, cam.width
    gx, gy = cam.grid
    P = state.P
    _, _, gid = state.sorted()
    rng = state.ranges().astype(np.int64)
    pre = state.preprocess()
    xy, co = pre["xy"].astype(np.float32), pre["conic_o"].astype(np.float32)
    f32 = np.float32
    max_w = np.zeros(P, f32)
    sum_w = np.zeros(P, np.float64)
    hits = np.zeros(P, np.int64)
    dist = np.full(P, np.inf)
    pix_sum = np.zeros((H, W), np.float64)
    pix_hits = np.zeros((H, W), np.int64)
    near_pairs = examined = 0
    busy = np.nonzero(rng[:, 1] > rng[:, 0])[0]
    third, cut, one, inf = f32(1.0) / f32(255.0), f32(0.0001), f32(1.0), f32(np.inf)
    # blocks of BLOCK tiles, each walked to its end: a block's arrays (BLOCK x 256 floats) stay in cache
    for b0 in range(0, len(busy), BLOCK):
        n, e = _walk(busy[b0:b0 + BLOCK], gx, W, H, gid, rng, xy, co, third, cut, one, inf,
                     max_w, sum_w, hits, dist, pix_sum, pix_hits)
        near_pairs += n
        examined += e
    return dict(max_w=max_w, sum_w=sum_w, hits=hits, dist=dist, near_pairs=near_pairs, examined_pairs=examined,
                pix_sum_w=pix_sum, pix_hits=pix_hits)


BLOCK = 128


def _walk(tiles, gx, W, H, gid, rng, xy, co, third, cut, one, inf, max_w, sum_w, hits, dist, pix_sum, pix_hits):
    """The lists of `tiles`, all advancing one entry per step; accumulates into the output arrays and
    returns (near pairs, examined pairs)."""
    f32 = np.float32
    near_pairs = examined = 0
    lx, ly = np.meshgrid(np.arange(TILE), np.arange(TILE))
    px = (tiles % gx)[:, None] * TILE + lx.ravel()[None, :]   # (tiles, 256)
    py = (tiles // gx)[:, None] * TILE + ly.ravel()[None, :]
    inside = (px < W) & (py < H)
    live = inside.copy()                                      # pixels still walking their list
    pfx, pfy = px.astype(f32), py.astype(f32)
    T = np.ones(px.shape, f32)
    S = np.zeros(px.shape, f32)
    N = np.zeros(px.shape, np.int32)
    start, length = rng[tiles, 0], rng[tiles, 1] - rng[tiles, 0]

    def retire(sel):  # the finished tiles' per-pixel results
        m = inside[sel]
        pix_sum[py[sel][m], px[sel][m]] = S[sel][m]
        pix_hits[py[sel][m], px[sel][m]] = N[sel][m]

    i = 0
    while True:
        # the state arrays hold the unfinished tiles only: they are compacted when a tile finishes
        keep = (length > i) & live.any(1)
        if not keep.all():
            retire(~keep)
            px, py, inside, live, pfx, pfy, T, S, N, start, length = (
                a[keep] for a in (px, py, inside, live, pfx, pfy, T, S, N, start, length))
        if len(start) == 0:
            break
        g = gid[start + i].astype(np.int64)
        examined += int(live.sum())
        c = co[g]
        dx = xy[g, 0][:, None] - pfx
        dy = xy[g, 1][:, None] - pfy
        power = f32(-0.5) * (c[:, 0:1] * dx * dx + c[:, 2:3] * dy * dy) - c[:, 1:2] * dx * dy
        with np.errstate(over="ignore"):
            alpha = np.minimum(f32(0.99), c[:, 3:4] * np.exp(power))
        cand = live & ~(power > 0)               # reaches the alpha test
        passed = cand & ~(alpha < third)         # reaches the termination test
        test_T = T * (one - alpha)
        stop = passed & (test_T < cut)
        use = passed & ~stop
        w = np.where(use, alpha * T, f32(0.0))
        # threshold distances of the examined pairs (float32 is ample for a 1e-3 .. 1e-6 window)
        d = np.where(cand, np.abs(alpha - third) / third, inf)
        d = np.where(passed, np.minimum(d, np.abs(test_T - cut) / cut), d)
        near_pairs += int(np.count_nonzero(d < f32(NEAR)))
        np.minimum.at(dist, g, d.min(1))
        np.maximum.at(max_w, g, w.max(1))
        np.add.at(sum_w, g, w.sum(1, dtype=np.float64))
        np.add.at(hits, g, np.count_nonzero(use, axis=1))
        np.copyto(T, test_T, where=use)
        S += w
        N += use
        live &= ~stop
        i += 1
    return near_pairs, examined
