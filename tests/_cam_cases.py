"""The camera path's case table: every branch of k_image_corr (projection, the four image borders, the occlusion walk inside and
outside the map, the two different is_valid tests, the tolerance) on injected maps of 34 / 66 / 98 cells and images of at most
48 x 64.  tests/test_cam_cases.py proves on the CPU (oracle + NumPy) that the table reaches every branch and that every walk ends;
tests/test_hip_camera.py runs the same cases on the GPU against the oracle.

A case is a dict: C, H, W, f (focal length in pixels), dist (radtan on / off), pos (camera position relative to the map centre, in
CELLS for x and y and metres for z), look ("down" | "level"), shift (the move_to before the map is injected, in cells; None = origin 0),
tol (tolerance_z_collision; None = the library's default 0.10), mode."""
import numpy as np

RES = 0.04
CLASSES = ("unknown", "behind", "off-left", "off-right", "off-top", "off-bottom", "occluded", "visible", "own-cell", "walk-leaves-map")
DIST = np.array([0.05, -0.01, 0.002, -0.001, 0.0005], np.float32)
WALL_H, PILLAR_H, KERB_H, HALF = 0.6, 2.0, 0.08, 0.5


def camera_map(C):
    """(7, C, C) map with known content: gentle relief, two unknown bands that hold garbage ABOVE every line of sight (a walk that
    forgot the is_valid test would be stopped by them), a wall of known height across the +x half whose middle third is stored with
    is_valid = 0.5 (the projection skips such a cell, `!= 1`; the walk lets it occlude, `!= 0`), a kerb of 8 cm in front of it (below the
    default tolerance of 10 cm) and a pillar taller than any camera."""
    xx, yy = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    m = np.zeros((7, C, C), np.float32)
    m[0] = (0.03 * np.sin(xx * 0.37) + 0.02 * np.cos(yy * 0.23)).astype(np.float32)
    m[1] = 0.01
    m[2] = 1.0
    for band in (slice(3, 5), slice(C - 6, C - 4)):
        m[2, band, :] = 0.0; m[0, band, :] = 5.0                   # unknown rows
    m[2, :, 2] = 0.0; m[0, :, 2] = 5.0                              # an unknown column
    wx = C // 2 + C // 5                                           # the wall: one row of cells on the +x side of the centre
    lo, hi = C // 4, C - C // 4
    m[0, wx, lo:hi] = WALL_H
    m[2, wx, lo:hi] = 1.0
    third = (hi - lo) // 3
    m[2, wx, lo + third:lo + 2 * third] = HALF
    m[0, C // 2 + C // 10, lo:hi] = KERB_H                        # a kerb lower than the default tolerance: occludes only under a smaller one
    m[0, C // 2 + C // 8:C // 2 + C // 8 + 2, 3 * C // 4:3 * C // 4 + 4] = PILLAR_H     # 2 x 4 cells, off the wall's shadow
    return m


def _rot_down(yaw):
    """world -> camera, optical axis -z (camera x = world x turned by yaw, camera y = -world y)"""
    c, s = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return (np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]]) @ Rz.T).astype(np.float32)


R_LEVEL = np.array([[0, -1.0, 0], [0, 0, -1.0], [1.0, 0, 0]], np.float32)      # optical axis +x, image up = world z


def _case(name, C, pos, look="down", H=48, W=64, f=40.0, dist=False, shift=None, tol=None, mode="reference_fp16", yaw=0.0):
    return dict(name=name, C=C, pos=pos, look=look, H=H, W=W, f=f, dist=dist, shift=shift, tol=tol, mode=mode, yaw=yaw)


def cases():
    out = []
    for dist in (False, True):
        d = "_radtan" if dist else ""
        # the down-looking camera, origin 0 and with the circular origin's seam through the camera cell in both axes
        out.append(_case("down" + d, 66, (3.3, -2.6, 1.6), dist=dist, yaw=0.3))
        out.append(_case("down_seam" + d, 66, (0.4, 0.3, 1.6), dist=dist, shift=(33, -33, 0.05)))
        # 0.4 m above the terrain, horizontal axis: half the map behind it, the wall and the pillar in front of it
        out.append(_case("low_wall" + d, 98, (-10.5, 0.4, 0.4), look="level", dist=dist))
        # narrow image: all four borders cut the map
        out.append(_case("narrow" + d, 34, (0.5, 0.5, 1.6), H=16, W=16, f=40.0, dist=dist, yaw=0.2))
    out.append(_case("low_wall_seam", 98, (-10.5, 0.4, 0.4), look="level", shift=(-39, 49, -0.02)))
    out.append(_case("own_cell", 34, (0.0, 0.0, 1.2)))                       # exactly over the (known) centre cell
    # camera cell outside the map: high side (as before the fix), low side (negative index; the uint32 cast of the reference wraps it)
    for name, px, py in (("beyond_x", 27.3, 2.2), ("beyond_y", -1.2, 25.6), ("beyond_xy", 24.3, 23.4),
                         ("negative_x", -27.3, 2.2), ("negative_y", 1.2, -25.6), ("negative_xy", -24.3, -23.4)):
        out.append(_case(name, 34, (px, py, 1.6)))
    out.append(_case("negative_x_level", 66, (-45.5, 0.4, 0.4), look="level"))       # the low camera from outside the map
    out.append(_case("low_wall_tol0", 98, (-10.5, 0.4, 0.4), look="level", tol=0.0))
    out.append(_case("low_wall_tol05", 98, (-10.5, 0.4, 0.4), look="level", tol=0.5))
    out.append(_case("low_wall_fp32", 98, (-10.5, 0.4, 0.4), look="level", mode="fp32"))
    out.append(_case("down_seam_fp32", 66, (0.4, 0.3, 1.6), shift=(33, -33, 0.05), mode="fp32", dist=True))
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def center_of(c):
    """the map centre after the case's move_to (ElevationMap.move_to from the origin: whole cells in x and y)"""
    s = c["shift"] or (0, 0, 0.0)
    return np.array([s[0] * RES, s[1] * RES, s[2]], np.float32)


def camera_of(c):
    """K, D, R (world -> camera), t, H, W of a case"""
    H, W = c["H"], c["W"]
    K = np.array([[c["f"], 0, W / 2], [0, c["f"], H / 2], [0, 0, 1]], np.float32)
    D = DIST.copy() if c["dist"] else np.zeros(5, np.float32)
    R = R_LEVEL if c["look"] == "level" else _rot_down(c["yaw"])
    cam = center_of(c).astype(np.float64) + np.array([c["pos"][0] * RES, c["pos"][1] * RES, c["pos"][2]])
    t = (-R.astype(np.float64) @ cam).astype(np.float32)
    return K, D, R, t, H, W


def oracle_run(eo, P, c, emap=None, tol="case"):
    """the oracle's (uv, valid) of a case, and the inputs it was given: (uv, valid, (Pm, x1, y1, z1, K, D, center))"""
    from elevation_mapping_cupy_amd.elevation_mapping import camera_cell
    K, D, R, t, H, W = camera_of(c)
    center = center_of(c)
    x1, y1, z1 = camera_cell(center, c["C"], RES, R, t)
    Pm = (K @ np.concatenate([R, t[:, None]], 1)).astype(np.float32)
    tol = (0.10 if c["tol"] is None else c["tol"]) if tol == "case" else tol
    m = camera_map(c["C"]) if emap is None else emap
    uv, va = eo.image_correspondence(P, m, x1, y1, z1, Pm.ravel(), K.ravel(), D, H, W, center, tol)
    return uv, va, (Pm, x1, y1, z1, K, D, center)


def classify(c, emap, uv, valid, inputs):
    """One class per cell, (C, C) array of indices into CLASSES, from a NumPy restatement of the projection (float32, the kernel's
    order of operations) and the oracle's `valid`.  A cell off more than one border goes to the first border the kernel tests
    (left, top, right, bottom) and is NOT counted for the others: the counts are of cells that ONE border test alone removes."""
    Pm, x1, y1, z1, K, D, center = inputs
    C, f32 = c["C"], np.float32
    x0, y0 = np.meshgrid(np.arange(C), np.arange(C), indexing="ij")
    p1 = ((x0 - C // 2).astype(np.float64) * RES + np.float64(center[0])).astype(f32)
    p2 = ((y0 - C // 2).astype(np.float64) * RES + np.float64(center[1])).astype(f32)
    p3 = emap[0] + center[2]
    Pm = Pm.ravel()
    row = lambda k: p1 * Pm[4 * k] + p2 * Pm[4 * k + 1] + p3 * Pm[4 * k + 2] + Pm[4 * k + 3]  # noqa: E731
    with np.errstate(all="ignore"):
        u, v, d = row(0), row(1), row(2)
        u, v = u / d, v / d
        if np.any(D != 0):
            k1, k2, q1, q2, k3 = D
            fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
            x, y = (u - cx) / fx, (v - cy) / fy
            r2 = x * x + y * y
            radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
            uc = x * radial + 2 * q1 * x * y + q2 * (r2 + 2 * x * x)
            vc = y * radial + 2 * q2 * x * y + q1 * (r2 + 2 * y * y)
            u, v = fx * uc + cx, fy * vc + cy
    assert u.dtype == f32 and d.dtype == f32
    off = np.stack([u < 0, v < 0, u >= f32(c["W"]), v >= f32(c["H"])])           # left, top, right, bottom: the kernel's order
    n_off = off.sum(0)
    cls = np.full((C, C), -1, np.int32)
    idx = {n: i for i, n in enumerate(CLASSES)}
    todo = np.ones((C, C), bool)

    def take(mask, name):
        nonlocal todo
        cls[todo & mask] = idx[name]; todo = todo & ~mask
    take(emap[2] != 1, "unknown")
    take(d <= 0, "behind")
    corner = n_off > 1
    for k, name in enumerate(("off-left", "off-top", "off-right", "off-bottom")):
        take(off[k] & ~corner, name)
    for k, name in enumerate(("off-left", "off-top", "off-right", "off-bottom")):
        take(off[k], name)
    exclusive = {name: int((cls == idx[name])[~corner].sum()) for name in ("off-left", "off-top", "off-right", "off-bottom")}
    cam_inside = 0 <= x1 < C and 0 <= y1 < C
    take((x0 == int(x1)) & (y0 == int(y1)), "own-cell")
    take(valid == 0, "occluded")
    take(np.full((C, C), not cam_inside), "walk-leaves-map")
    take(np.ones((C, C), bool), "visible")
    # the restatement and the oracle agree on who was projected into the image at all, and on what the classes mean
    in_image = cls >= idx["occluded"]
    assert np.array_equal(in_image, (uv[0] != 0) | (uv[1] != 0) | (valid != 0)), c["name"]
    assert np.array_equal(uv[0][in_image], u[in_image]) and np.array_equal(uv[1][in_image], v[in_image]), c["name"]
    assert valid[cls >= idx["visible"]].all() and not valid[~in_image].any(), c["name"]
    counts = {n: int((cls == i).sum()) for i, n in enumerate(CLASSES)}
    counts.update(exclusive)
    return cls, counts
