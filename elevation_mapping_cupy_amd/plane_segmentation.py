"""Host model of the plane segmentation on the device (``emap_plane_segmentation``, csrc/emap_planeseg.hip): NumPy
in IEEE double with the device's operation order, stage by stage.  It is the A/B route of ``ElevationMap.get_plane_segmentation``
(``EMAP_PLANES_RESIDENT=0``: the whole map is downloaded and segmented here) and what the tests compare the device against, bit for
bit.  The stages restate convex_plane_decomposition's SlidingWindowPlaneExtractor.cpp (:19-41, :79-144, :147-150, :165-220, :277-300),
grid_map's SlidingWindowIterator (edge handling EMPTY) and the numbering of OpenCV's connectedComponents; neither library is pinned
by a compiled reference.  Every plane is ``(M, M)`` in published index space, cell ``(i, j)`` at ``idx = i * M + j``."""
from __future__ import annotations

import types

import numpy as np

SWEEPS = 4            # EM_PLANE_SWEEPS: Jacobi sweeps, fixed
TILE = 32             # the label pass's tile
Q_BITS = 13           # EM_PLANE_Q_BITS
Q_RANGE = 32.0        # EM_PLANE_Q_RANGE
PLANE_DTYPE = np.dtype([("label", np.int32), ("n_points", np.int32), ("needs_refinement", np.int32), ("n_left_out", np.int32),
                        ("support", np.float64, (3,)), ("normal", np.float64, (3,))])


def _sel(i, a0, a1, a2):
    return np.where(i == 0, a0, np.where(i == 1, a1, a2))


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """one Jacobi rotation of the pair (p, q), r the third index; vp / vq: columns p, q of the vectors (three rows each); a pair with
    apq == 0 is skipped"""
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = [app - t * apq, aqq + t * apq, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq]
        nvp = [c * vp[k] - s * vq[k] for k in range(3)]
        nvq = [s * vp[k] + c * vq[k] for k in range(3)]
    app, aqq, apq, arp, arq = (np.where(on, n, o) for n, o in zip(new, (app, aqq, apq, arp, arq)))
    return app, aqq, apq, arp, arq, [np.where(on, n, o) for n, o in zip(nvp, vp)], [np.where(on, n, o) for n, o in zip(nvq, vq)]


def jacobi3(a00, a01, a02, a11, a12, a22, sweeps=SWEEPS):
    """cyclic Jacobi on symmetric 3 x 3 matrices (arrays of any one shape), pairs (0,1), (0,2), (1,2), ``sweeps`` sweeps: ``(w, v)`` with
    the eigenvalues ``w[k]`` ascending (ties to the lower index) and ``v[k][row]`` their vectors"""
    a00, a01, a02, a11, a12, a22 = (np.array(a, np.float64) for a in (a00, a01, a02, a11, a12, a22))
    one, zero = np.ones_like(a00), np.zeros_like(a00)
    c0, c1, c2 = [one, zero, zero], [zero, one, zero], [zero, zero, one]      # columns of v
    for _ in range(sweeps):
        a00, a11, a01, a02, a12, c0, c1 = _rotate(a00, a11, a01, a02, a12, c0, c1)
        a00, a22, a02, a01, a12, c0, c2 = _rotate(a00, a22, a02, a01, a12, c0, c2)
        a11, a22, a12, a01, a02, c1, c2 = _rotate(a11, a22, a12, a01, a02, c1, c2)
    i0, i1, i2 = (np.full(a00.shape, k, np.int8) for k in range(3))

    def swap_if_less(ia, ib):
        less = _sel(ib, a00, a11, a22) < _sel(ia, a00, a11, a22)
        return np.where(less, ib, ia), np.where(less, ia, ib)

    i0, i1 = swap_if_less(i0, i1)
    i1, i2 = swap_if_less(i1, i2)
    i0, i1 = swap_if_less(i0, i1)
    w = [_sel(i, a00, a11, a22) for i in (i0, i1, i2)]
    v = [[_sel(i, c0[row], c1[row], c2[row]) for row in range(3)] for i in (i0, i1, i2)]
    return w, v


def plane_normal(n, s, q, sweeps=SWEEPS):
    """normalAndErrorFromCovariance (:19-41): ``n`` points, sums ``s`` (3), upper triangle ``q`` (xx xy xz yy yz zz) of the sum of squares;
    ``(normal (3), error, eigenvalues (3), covariance (6))``"""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        m = [s[k] / n for k in range(3)]
        cov = [q[0] / n - m[0] * m[0], q[1] / n - m[0] * m[1], q[2] / n - m[0] * m[2], q[3] / n - m[1] * m[1], q[4] / n - m[1] * m[2], q[5] / n - m[2] * m[2]]
    w, v = jacobi3(*cov, sweeps=sweeps)
    ok = w[1] > 1e-8
    flip = v[0][2] < 0.0
    unit = (0.0, 0.0, 1.0)
    normal = [np.where(ok, np.where(flip, -v[0][k], v[0][k]), unit[k]) for k in range(3)]
    err = np.where(ok, np.where(w[0] > 0.0, w[0], 0.0), 1e30)
    return normal, err, w, cov


def window_pass(h, kernel_size, resolution, thr2, cos_local, sweeps=SWEEPS):
    """runSlidingWindowDetector (:115-136) without the opening.  Points ``(-kr res, -kc res, h)``, kr / kc counted from the UNCLIPPED
    window's corner, cells outside the map absent; summed column outer, row inner.  Returns a namespace: ``planar`` bool, ``normals``
    float32 ``(3, M, M)`` (zero where the centre is not finite), and in double ``normal``, ``err``, ``n``, ``w``, ``cov`` for the tests"""
    h = np.ascontiguousarray(h, np.float32)
    M, K, H = h.shape[0], int(kernel_size), int(kernel_size) // 2
    res = float(resolution)
    hp = np.full((M + 2 * H, M + 2 * H), np.nan, np.float32)
    hp[H:H + M, H:H + M] = h
    n = np.zeros((M, M))
    s = [np.zeros((M, M)) for _ in range(3)]
    q = [np.zeros((M, M)) for _ in range(6)]
    for kc in range(K):
        py = float(-kc) * res
        for kr in range(K):
            px = float(-kr) * res
            hh = hp[kr:kr + M, kc:kc + M]
            fin = np.isfinite(hh)
            pz = np.where(fin, hh, np.float32(0.0)).astype(np.float64)
            add = lambda acc, val: acc + np.where(fin, val, 0.0)      # noqa: E731  (a sum never is -0.0: adding +0.0 changes nothing)
            n = n + fin
            s = [add(s[0], px), add(s[1], py), add(s[2], pz)]
            q = [add(q[0], px * px), add(q[1], px * py), add(q[2], px * pz), add(q[3], py * py), add(q[4], py * pz), add(q[5], pz * pz)]
    normal, err, w, cov = plane_normal(np.where(n >= 3, n, 1.0), s, q, sweeps)
    few = n < 3
    centre = np.isfinite(h)
    unit = (0.0, 0.0, 1.0)
    normal = [np.where(few, unit[k], normal[k]) for k in range(3)]
    err = np.where(few, 1e30, err)
    planar = centre & (err < thr2) & (normal[2] > cos_local)
    normals = np.stack([np.where(centre, normal[k], 0.0).astype(np.float32) for k in range(3)])
    return types.SimpleNamespace(planar=planar, normals=normals, normal=normal, err=err, n=n, w=w, cov=cov, centre=centre)


def _cross(img, r, dilate):
    """erosion / dilation with a cross of radius r, indices clamped (BORDER_REPLICATE)"""
    M = img.shape[0]
    p = np.pad(img, r, mode="edge")
    out = img.copy()
    for d in range(1, r + 1):
        for a in (p[r - d:r - d + M, r:r + M], p[r + d:r + d + M, r:r + M], p[r:r + M, r - d:r - d + M], p[r:r + M, r + d:r + d + M]):
            out = (out | a) if dilate else (out & a)
    return out


def opening(planar, radius, dilate=True):
    """MORPH_OPEN with MORPH_CROSS (:137-143); ``dilate=False`` leaves the second half out (a test's lost piece)"""
    if radius <= 0:
        return planar
    e = _cross(planar, radius, False)
    return _cross(e, radius, True) if dilate else e


# ---- labels: union-find in which a link only ever points to a smaller idx ----------------------------------------------------------------
def jump(parent):
    """every cell's root (the parents of cells that are not planar are -1 and stay)"""
    p = parent.copy()
    on = p >= 0
    while True:
        pp = p.copy()
        pp[on] = p[p[on]]
        if (pp == p).all():
            return p
        p = pp


def _edges(planar, conn):
    """(a, b, crossing): the linked pairs idx a > idx b of planar neighbours, and whether the pair crosses a tile border"""
    M = planar.shape[0]
    i, j = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    idx = i * M + j
    out = []
    steps = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if conn == 8 else [])
    for di, dj in steps:
        ok = planar & (i + di >= 0) & (j + dj >= 0) & (j + dj < M)
        ii, jj = np.clip(i + di, 0, M - 1), np.clip(j + dj, 0, M - 1)
        ok = ok & planar[ii, jj]
        cross = (i // TILE != ii // TILE) | (j // TILE != jj // TILE)
        out.append((idx[ok], (ii * M + jj)[ok], cross[ok]))
    return tuple(np.concatenate(c) for c in zip(*out))


def hook(parent, a, b, last_wins=False, rounds=None):
    """the unions of the pairs (a, b) on ``parent`` (flat, -1: not planar): only ROOTS get new links, each to a smaller root; the other
    cells keep their links (``jump`` gives everyone's root).  ``last_wins`` / ``rounds``: a lost piece of the tests -- one plain store
    per root instead of a minimum that is tried again"""
    parent = parent.copy()
    k = 0
    while rounds is None or k < rounds:
        k += 1
        flat = jump(parent)
        ra, rb = flat[a], flat[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        sel = lo != hi
        if not sel.any():
            break
        if last_wins:
            parent[hi[sel]] = lo[sel]
        else:
            np.minimum.at(parent, hi[sel], lo[sel])
    return parent


def components(planar, conn, merge=True, flatten=True, lost_arm=False):
    """every cell's root (-1: not planar) as the device finds it: a tile-local pass, the links across tile borders, a flatten.  The root
    is the component's smallest idx.  ``merge`` / ``flatten`` / ``lost_arm``: the tests' lost pieces"""
    M = planar.shape[0]
    a, b, cross = _edges(planar, conn)
    parent = np.where(planar.ravel(), np.arange(M * M), -1)
    parent = jump(hook(parent, a[~cross], b[~cross]))        # k_ps_local writes local ROOTS
    if merge:
        parent = hook(parent, a[cross], b[cross], last_wins=lost_arm, rounds=1 if lost_arm else None)
    return (jump(parent) if flatten else parent).reshape(M, M)


def numbering(root, column_major=False):
    """label = 1 + the rank of the cell's root among the roots in ascending idx (the first cell a raster scan meets); 0: not planar"""
    M = root.shape[0]
    flat = root.ravel()
    idx = np.arange(M * M)
    bits = flat == idx
    if column_major:
        order = (idx % M) * M + idx // M
        rank = np.empty(M * M, np.int64)
        rank[np.argsort(order, kind="stable")] = np.cumsum(bits[np.argsort(order, kind="stable")]) - bits[np.argsort(order, kind="stable")]
    else:
        rank = np.cumsum(bits) - bits
    labels = np.where(flat >= 0, 1 + rank[np.maximum(flat, 0)], 0).astype(np.int32)
    return labels.reshape(M, M), int(bits.sum())


def label_planes(h, normals, root, labels, resolution, origin_xy, min_points, cos_plane, dist_thr, cos_angle, reject=True, sweeps=SWEEPS):
    """computePlaneParametersForLabel without RANSAC (:165-220) on exact fixed-point moments about each label's anchor, and the verdict
    of isGloballyPlanar (:277-300).  Returns ``(labels with the rejected ones at 0, planes, details)``"""
    h = np.ascontiguousarray(h, np.float32)
    M = h.shape[0]
    res, (ox, oy) = float(resolution), (float(origin_xy[0]), float(origin_xy[1]))
    flat, hf = root.ravel(), h.ravel()
    idx = np.arange(M * M)
    member = (flat >= 0) & np.isfinite(hf)
    cnt = np.bincount(flat[member], minlength=M * M)
    amin = np.full(M * M, np.iinfo(np.int64).max)
    np.minimum.at(amin, flat[member], idx[member])
    owners = np.nonzero((flat == idx) & (cnt >= max(int(min_points), 3)))[0]      # ascending idx: ascending labels
    S = owners.size
    slot_of = np.full(M * M, -1)
    slot_of[owners] = np.arange(S)
    out = labels.copy()
    planes = np.zeros(0, PLANE_DTYPE)
    details = types.SimpleNamespace(normal_z=np.zeros(0), max_dist=np.zeros(0), min_dot=np.zeros(0), slots=S)
    if S == 0:
        return out, planes, details
    sl = np.where(flat >= 0, slot_of[np.maximum(flat, 0)], -1)
    inn = member & (sl >= 0)
    ha = hf[amin[owners]].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(inn, hf, np.float32(0.0)).astype(np.float64) - np.where(inn, ha[np.maximum(sl, 0)], 0.0)
    left = inn & (np.abs(d) > Q_RANGE)
    use = inn & ~left
    left_out = np.bincount(sl[left], minlength=S)
    k = sl[use]
    di = (idx[use] // M - owners[k] // M).astype(np.int64)
    dj = (idx[use] % M - owners[k] % M).astype(np.int64)
    qq = np.rint(d[use] * float(1 << Q_BITS)).astype(np.int64)
    sums = np.zeros((10, S), np.int64)
    for r, c in enumerate((np.ones_like(di), di, dj, qq, di * di, dj * dj, di * dj, di * qq, dj * qq, qq * qq)):
        np.add.at(sums[r], k, c)
    f = sums.astype(np.float64)
    n, rr, u = f[0], res * res, 1.0 / float(1 << Q_BITS)
    uu = u * u
    s = [-(f[1] * res), -(f[2] * res), f[3] * u]
    q = [f[4] * rr, f[6] * rr, -(f[7] * res) * u, f[5] * rr, -(f[8] * res) * u, f[9] * uu]
    normal, _, w, _ = plane_normal(n, s, q, sweeps)
    ia, ja = (owners // M).astype(np.float64), (owners % M).astype(np.float64)
    support = [(ox - ia * res) + s[0] / n, (oy - ja * res) + s[1] / n, ha + s[2] / n]
    accept = normal[2] > cos_plane
    if reject:
        gone = (sl >= 0) & ~accept[np.maximum(sl, 0)]
        out = np.where(gone.reshape(M, M), 0, out).astype(np.int32)
    # isGloballyPlanar, folded per label: the largest distance, the smallest dot product with the float window normals
    fold = member & (sl >= 0) & accept[np.maximum(sl, 0)]
    kf = sl[fold]
    px, py, pz = ox - (idx[fold] // M).astype(np.float64) * res, oy - (idx[fold] % M).astype(np.float64) * res, hf[fold].astype(np.float64)
    nx, ny, nz = normal[0][kf], normal[1][kf], normal[2][kf]
    dist = np.abs(((nx * px + ny * py) + nz * pz) - ((nx * support[0][kf] + ny * support[1][kf]) + nz * support[2][kf]))
    wn = [normals[a].ravel()[fold].astype(np.float64) for a in range(3)]
    dot = (nx * wn[0] + ny * wn[1]) + nz * wn[2]
    max_dist, min_dot = np.zeros(S), np.full(S, np.inf)
    np.maximum.at(max_dist, kf, dist)
    np.minimum.at(min_dot, kf, dot)
    planes = np.zeros(int(accept.sum()), PLANE_DTYPE)
    a = np.nonzero(accept)[0]
    planes["label"] = labels.ravel()[owners[a]]
    planes["n_points"] = sums[0][a]
    planes["n_left_out"] = left_out[a]
    planes["needs_refinement"] = (max_dist[a] > dist_thr) | (min_dot[a] < cos_angle)
    planes["support"] = np.stack([support[c][a] for c in range(3)], axis=1)
    planes["normal"] = np.stack([normal[c][a] for c in range(3)], axis=1)
    details = types.SimpleNamespace(normal_z=normal[2], accept=accept, max_dist=max_dist[a], min_dot=min_dot[a], slots=S, w=w, owners=owners)
    return out, planes, details


def cosines(plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees, global_plane_fit_angle_error_threshold_degrees):
    """the three angles as the cosines the device gets, in double"""
    return tuple(float(np.cos(np.float64(a) * np.pi / 180.0)) for a in
                 (plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees, global_plane_fit_angle_error_threshold_degrees))


def segment(h, resolution, origin_xy, *, kernel_size=3, planarity_opening_filter=0, plane_inclination_threshold_degrees=30.0,
            local_plane_inclination_threshold_degrees=35.0, plane_patch_error_threshold=0.02, min_number_points_per_label=4, connectivity=4,
            global_plane_fit_distance_error_threshold=0.025, global_plane_fit_angle_error_threshold_degrees=25.0):
    """the whole model on one published height plane: a namespace with ``labels``, ``n_labels``, ``planes``, ``normals``, ``planar``"""
    cos_plane, cos_local, cos_angle = cosines(plane_inclination_threshold_degrees, local_plane_inclination_threshold_degrees,
                                              global_plane_fit_angle_error_threshold_degrees)
    thr = float(plane_patch_error_threshold)
    win = window_pass(h, kernel_size, resolution, thr * thr, cos_local)
    planar = opening(win.planar, int(planarity_opening_filter))
    root = components(planar, int(connectivity))
    labels, n_labels = numbering(root)
    labels, planes, details = label_planes(h, win.normals, root, labels, resolution, origin_xy, min_number_points_per_label, cos_plane,
                                           float(global_plane_fit_distance_error_threshold), cos_angle)
    return types.SimpleNamespace(labels=labels, n_labels=n_labels, planes=planes, normals=win.normals, planar=planar, window=win, details=details)
