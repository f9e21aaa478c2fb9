"""TEST INFRASTRUCTURE ONLY (the product never imports it).  Restatement of the Inpainting plugin's method "telea_fronts"
(elevation_mapping_cupy_amd/csrc/emap_inpaint_fronts.hip, contract in include/emap_hip.h and DESIGN.md §8): Telea's estimator with the
float32 arithmetic of telea() in emap_inpaint_host.hip (radius 1), scheduled by fronts of the L1 distance to the known pixels instead of
by a serial priority queue.

* ``inpaint_fronts``: vectorised over the pixels of one front (a 1024^2 map runs in seconds); the device must equal it bit for bit.
* ``inpaint_fronts_loops``: the same contract as plain per-pixel loops with a BFS distance (small images only), a second statement that
  the vectorised one is checked against.
* ``inpaint_front_rule``: the existing method "front" (k_inpaint_sweep: distance-weighted mean of the known 8-neighbours, one sweep per
  front) for comparisons of agreement with the host Telea."""
from collections import deque

import numpy as np

F32 = np.float32
BIG = F32(1.0e6)
INF = 1 << 29


def distance(mask):
    """L1 distance to the nearest pixel with mask == 0 (INF if there is none): column pass, then row pass (min-plus over |dj|)."""
    m = np.asarray(mask) != 0
    rows, cols = m.shape
    g = np.empty((rows, cols), np.int64)
    h = np.full(cols, INF, np.int64)
    for i in range(rows):
        h = np.where(m[i], np.minimum(h + 1, INF), 0); g[i] = h
    h = np.full(cols, INF, np.int64)
    for i in range(rows - 1, -1, -1):
        h = np.where(m[i], np.minimum(h + 1, INF), 0); g[i] = np.minimum(g[i], h)
    j = np.arange(cols, dtype=np.int64)
    fwd = np.minimum.accumulate(g - j, axis=1) + j
    bwd = np.minimum.accumulate((g + j)[:, ::-1], axis=1)[:, ::-1] - j
    return np.minimum(np.minimum(fwd, bwd), INF)


def _check(image, mask, radius):
    image = np.asarray(image, np.uint8); mask = np.asarray(mask)
    if radius != 1 or image.ndim != 2 or image.shape[0] < 2 or image.shape[1] < 2 or mask.shape != image.shape:
        raise ValueError("telea_fronts: radius 1 and images of at least 2 x 2 pixels only")
    return image, mask


def inpaint_fronts(image, mask, radius=1):
    image, mask = _check(image, mask, radius)
    rows, cols = image.shape
    d = distance(mask)
    dmax = int(d.max())
    if dmax == 0 or dmax >= INF:
        return image.copy()
    out = image.astype(F32)                                      # values: computed for earlier fronts, the input otherwise
    dp = np.full((rows + 2, cols + 2), -1, np.int64); dp[1:-1, 1:-1] = d          # framed; the frame (-1) is always known
    T = np.full((rows + 2, cols + 2), BIG, F32)
    hole = np.zeros((rows + 2, cols + 2), bool); hole[1:-1, 1:-1] = mask != 0
    band = ~hole & (np.roll(hole, 1, 0) | np.roll(hole, -1, 0) | np.roll(hole, 1, 1) | np.roll(hole, -1, 1))
    band[0, :] = band[-1, :] = band[:, 0] = band[:, -1] = False
    T[band] = F32(-0.0)
    flat = d.ravel()
    order = np.argsort(flat, kind="stable")
    bounds = np.searchsorted(flat[order], np.arange(1, dmax + 2))
    for k in range(1, dmax + 1):
        idx = order[bounds[k - 1]:bounds[k]]
        i, j = idx // cols, idx % cols                           # image coordinates; framed = + 1
        fi, fj = i + 1, j + 1

        def kn(a, b):
            return dp[fi + a, fj + b] < k

        def tv(a, b):
            return T[fi + a, fj + b]

        def ov(x, y):
            return out[x, y]

        def solve(a1, b1, a2, b2):
            a11, a22 = tv(a1, b1), tv(a2, b2)
            m12 = np.where(a11 < a22, a11, a22)
            k1, k2 = kn(a1, b1), kn(a2, b2)
            df = a11 - a22
            with np.errstate(invalid="ignore"):
                both = np.where(np.abs(df) >= F32(1.0), F32(1.0) + m12, (a11 + a22 + np.sqrt(F32(2.0) - df * df)) * F32(0.5))
            return np.where(k1, np.where(k2, both, F32(1.0) + a11), np.where(k2, F32(1.0) + a22, F32(1.0) + m12)).astype(F32)

        s1, s2, s3, s4 = solve(-1, 0, 0, -1), solve(1, 0, 0, -1), solve(-1, 0, 0, 1), solve(1, 0, 0, 1)
        a = np.where(s1 < s2, s1, s2); c = np.where(s3 < s4, s3, s4)
        dist = np.where(a < c, a, c).astype(F32)
        zero = np.zeros_like(dist)
        gx = np.where(kn(0, 1), np.where(kn(0, -1), (tv(0, 1) - tv(0, -1)) * F32(0.5), tv(0, 1) - dist),
                      np.where(kn(0, -1), dist - tv(0, -1), zero))
        gy = np.where(kn(1, 0), np.where(kn(-1, 0), (tv(1, 0) - tv(-1, 0)) * F32(0.5), tv(1, 0) - dist),
                      np.where(kn(-1, 0), dist - tv(-1, 0), zero))
        Ia, Jx, Jy, s = zero.copy(), zero.copy(), zero.copy(), np.full_like(dist, F32(1.0e-20))
        for a_, b_ in ((-1, 0), (0, -1), (0, 1), (1, 0)):          # the radius-1 window in the host's row-major order
            kk, ll = i + a_, j + b_
            ok = (kk >= 0) & (ll >= 0) & (kk < rows) & (ll < cols) & kn(a_, b_)
            kc, lc = np.clip(kk, 0, rows - 1), np.clip(ll, 0, cols - 1)
            km, kp = kc + (kc == 0), kc - (kc == rows - 1)
            lm, lp = lc + (lc == 0), lc - (lc == cols - 1)
            ry, rx = F32(-a_), F32(-b_)
            len2 = rx * rx + ry * ry
            dst = F32(1.0) / (len2 * np.sqrt(len2))
            lev = F32(1.0) / (F32(1.0) + np.abs(tv(a_, b_) - dist))
            dr = rx * gx + ry * gy
            dr = np.where(np.abs(dr) <= F32(0.01), F32(0.000001), dr).astype(F32)
            w = np.abs(dst * lev * dr)
            kx1, kx0 = dp[fi + a_, np.clip(fj + b_ + 1, 0, cols + 1)] < k, dp[fi + a_, np.clip(fj + b_ - 1, 0, cols + 1)] < k
            ky1, ky0 = dp[np.clip(fi + a_ + 1, 0, rows + 1), fj + b_] < k, dp[np.clip(fi + a_ - 1, 0, rows + 1), fj + b_] < k
            lmm, lpp = np.clip(lm - 1, 0, cols - 1), np.clip(lp + 1, 0, cols - 1)
            kmm, kpp = np.clip(km - 1, 0, rows - 1), np.clip(kp + 1, 0, rows - 1)
            gIx = np.where(kx1, np.where(kx0, (ov(km, lpp) - ov(km, lmm)) * F32(2.0), ov(km, lpp) - ov(km, lm)),
                           np.where(kx0, ov(km, lp) - ov(km, lmm), zero))
            gIy = np.where(ky1, np.where(ky0, (ov(kpp, lm) - ov(kmm, lm)) * F32(2.0), ov(kpp, lm) - ov(km, lm)),
                           np.where(ky0, ov(kp, lm) - ov(kmm, lm), zero))
            Ia = np.where(ok, Ia + w * ov(km, lm), Ia)
            Jx = np.where(ok, Jx - w * gIx * rx, Jx)
            Jy = np.where(ok, Jy - w * gIy * ry, Jy)
            s = np.where(ok, s + w, s)
        sat = Ia / s + (Jx + Jy) / (np.sqrt(Jx * Jx + Jy * Jy) + F32(1.0e-20))
        T[fi, fj] = dist
        out[i, j] = np.clip(np.rint(sat.astype(F32)), 0, 255)
    return out.astype(np.uint8)


def inpaint_fronts_loops(image, mask, radius=1):
    """The same contract, pixel by pixel, with the distance from a breadth-first search (small images only)."""
    image, mask = _check(image, mask, radius)
    rows, cols = image.shape
    d = np.full((rows, cols), -1, np.int64)
    q = deque()
    for i in range(rows):
        for j in range(cols):
            if not mask[i, j]:
                d[i, j] = 0; q.append((i, j))
    while q:
        i, j = q.popleft()
        for a, b in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            x, y = i + a, j + b
            if 0 <= x < rows and 0 <= y < cols and d[x, y] < 0:
                d[x, y] = d[i, j] + 1; q.append((x, y))
    if not (d == 0).any() or d.max() == 0:
        return image.copy()
    out = image.astype(F32)
    T = np.full((rows + 2, cols + 2), BIG, F32)
    for i in range(rows):
        for j in range(cols):
            if d[i, j] == 0 and any(0 <= i + a < rows and 0 <= j + b < cols and d[i + a, j + b] > 0 for a, b in ((-1, 0), (1, 0), (0, -1), (0, 1))):
                T[i + 1, j + 1] = F32(-0.0)
    one = F32(1.0)
    for k in range(1, int(d.max()) + 1):
        new = []
        for i in range(rows):
            for j in range(cols):
                if d[i, j] != k:
                    continue
                kn = lambda x, y: x < 0 or y < 0 or x >= rows or y >= cols or d[x, y] < k          # noqa: E731
                t = lambda x, y: T[x + 1, y + 1]                                                # noqa: E731
                o = lambda x, y: out[x, y]                                                      # noqa: E731

                def solve(x1, y1, x2, y2):
                    a11, a22 = t(x1, y1), t(x2, y2)
                    m12 = a11 if a11 < a22 else a22
                    if kn(x1, y1):
                        if kn(x2, y2):
                            return one + m12 if abs(a11 - a22) >= one else (a11 + a22 + np.sqrt(F32(2.0) - (a11 - a22) * (a11 - a22))) * F32(0.5)
                        return one + a11
                    return one + a22 if kn(x2, y2) else one + m12

                v = [solve(i - 1, j, i, j - 1), solve(i + 1, j, i, j - 1), solve(i - 1, j, i, j + 1), solve(i + 1, j, i, j + 1)]
                a = v[0] if v[0] < v[1] else v[1]; c = v[2] if v[2] < v[3] else v[3]
                dist = a if a < c else c
                if kn(i, j + 1):
                    gx = (t(i, j + 1) - t(i, j - 1)) * F32(0.5) if kn(i, j - 1) else t(i, j + 1) - dist
                else:
                    gx = dist - t(i, j - 1) if kn(i, j - 1) else F32(0.0)
                if kn(i + 1, j):
                    gy = (t(i + 1, j) - t(i - 1, j)) * F32(0.5) if kn(i - 1, j) else t(i + 1, j) - dist
                else:
                    gy = dist - t(i - 1, j) if kn(i - 1, j) else F32(0.0)
                Ia, Jx, Jy, s = F32(0), F32(0), F32(0), F32(1.0e-20)
                for kk in range(i - 1, i + 2):
                    km, kp = kk + (kk == 0), kk - (kk == rows - 1)
                    for ll in range(j - 1, j + 2):
                        lm, lp = ll + (ll == 0), ll - (ll == cols - 1)
                        if kk < 0 or ll < 0 or kk >= rows or ll >= cols or not kn(kk, ll) or (ll - j) ** 2 + (kk - i) ** 2 > 1:
                            continue
                        ry, rx = F32(i - kk), F32(j - ll)
                        len2 = rx * rx + ry * ry
                        dst = one / (len2 * np.sqrt(len2))
                        lev = one / (one + abs(t(kk, ll) - dist))
                        dr = rx * gx + ry * gy
                        if abs(dr) <= F32(0.01):
                            dr = F32(0.000001)
                        w = abs(dst * lev * dr)
                        if kn(kk, ll + 1):
                            gIx = (o(km, lp + 1) - o(km, lm - 1)) * F32(2.0) if kn(kk, ll - 1) else o(km, lp + 1) - o(km, lm)
                        else:
                            gIx = o(km, lp) - o(km, lm - 1) if kn(kk, ll - 1) else F32(0.0)
                        if kn(kk + 1, ll):
                            gIy = (o(kp + 1, lm) - o(km - 1, lm)) * F32(2.0) if kn(kk - 1, ll) else o(kp + 1, lm) - o(km, lm)
                        else:
                            gIy = o(kp, lm) - o(km - 1, lm) if kn(kk - 1, ll) else F32(0.0)
                        Ia = Ia + w * o(km, lm)
                        Jx = Jx - w * gIx * rx
                        Jy = Jy - w * gIy * ry
                        s = s + w
                sat = Ia / s + (Jx + Jy) / (np.sqrt(Jx * Jx + Jy * Jy) + F32(1.0e-20))
                new.append((i, j, dist, F32(min(max(np.rint(F32(sat)), 0), 255))))
        for i, j, dist, val in new:                              # every pixel of the front at once
            T[i + 1, j + 1] = dist; out[i, j] = val
    return out.astype(np.uint8)


def inpaint_front_rule(image, mask):
    """Method "front" (k_inpaint_sweep): per sweep, every unknown pixel with a known 8-neighbour becomes rint(sum w v / sum w) over
    them (w = 1 along an axis, 0.70710678 on a diagonal); sweeps until nothing is left to fill."""
    v = np.asarray(image, F32).copy(); m = (np.asarray(mask) == 0)
    rows, cols = v.shape
    if m.all() or not m.any():
        return np.asarray(image, np.uint8).copy()
    while not m.all():
        vp = np.zeros((rows + 2, cols + 2), F32); vp[1:-1, 1:-1] = v
        mp = np.zeros((rows + 2, cols + 2), bool); mp[1:-1, 1:-1] = m
        s = np.zeros_like(v); w = np.zeros_like(v)
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if not dr and not dc:
                    continue
                wt = F32(0.70710678) if dr and dc else F32(1.0)
                kn = mp[1 + dr:rows + 1 + dr, 1 + dc:cols + 1 + dc]
                s = np.where(kn, s + wt * vp[1 + dr:rows + 1 + dr, 1 + dc:cols + 1 + dc], s)
                w = np.where(kn, w + wt, w)
        fill = ~m & (w > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(fill, np.clip(np.rint(s / w), 0, 255), v).astype(F32)
        m = m | fill
    return v.astype(np.uint8)
