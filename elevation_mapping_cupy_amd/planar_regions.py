"""Host model of the planar regions on the device (``emap_planar_regions``, csrc/emap_regions.hip): NumPy, integer
exact, stage by stage as the device computes it.  It is the A/B route of ``ElevationMap.get_planar_regions``
(``EMAP_REGIONS_RESIDENT=0``) and the yardstick the GPU tests compare bit for bit; tests/test_planar_region_cases.py checks it on the
CPU against independent restatements (scipy.ndimage, literal loops).

What is restated: the middle stage of convex_plane_decomposition's ``PlaneDecompositionPipeline::update`` --
``ContourExtraction::extractPlanarRegions`` (ContourExtraction.cpp:28-128), the x 3 upsampling (Upsampling.cpp:12-68) and the frame
of a region (PlanarRegion.cpp:5-50).  OpenCV's ``erode`` / ``findContours`` and CGAL's ``isInside`` are restated, not pinned.

A label image ``X`` (0: background) is traced as CRACKS: crack (pixel p, side s) has the index ``4 idx(p) + s``; side 0 is the top
edge travelled west, 1 the left edge travelled south, 2 the bottom edge travelled east, 3 the right edge travelled north -- the
foreground on the left hand.  The successor map is a permutation of the cracks, its cycles are the borders (rings)."""
from __future__ import annotations

import types

import numpy as np

from . import plane_segmentation as ps

MARGIN_MAX = 14                     # margin_size 0 .. 14: an ellipse of at most 31 pixels (EMAP_TERRAIN_KERNEL_MAX)
SIDE_MAX = 7724                     # 4 U U < 2^31 with U = 3 M - 2 (crack indices are int32)
RAW_SIDE_MAX = 23170                # ... with U = M
RING_DTYPE = np.dtype([(n, np.int32) for n in ("first_vertex", "n_vertices", "image", "is_hole", "label", "root", "crack", "boundary")])      # the bytes of emap_region_ring
TRAVEL = ((0, -1), (1, 0), (0, 1), (-1, 0))      # side s: the direction of travel (row, column)
ACROSS = ((-1, 0), (0, -1), (1, 0), (0, 1))      # side s: the pixel on the other side of the edge
CROSS = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))


# ---- 1. the upsampled image ------------------------------------------------------------------------------------------------------------------
def upsample_index(M, edge3=False):
    """the cell that pixel u of the U = 3 M - 2 image reads (Upsampling.cpp:12-58): the first and the last cell give 2 pixels, the others 3.
    ``edge3``: a lost piece of the tests -- every cell gives 3"""
    if edge3:
        return np.arange(3 * M) // 3
    U = 3 * M - 2
    u = np.arange(U)
    return np.where(u < 2, 0, np.where(u >= U - 2, M - 1, 1 + (u - 2) // 3))


def upsample(labels, edge3=False):
    s = upsample_index(labels.shape[0], edge3)
    return np.ascontiguousarray(labels[np.ix_(s, s)])


# ---- 2. erosions, all labels in one pass ----------------------------------------------------------------------------------------------------
def ellipse_offsets(k):
    """getStructuringElement(MORPH_ELLIPSE, (k, k)) as (row, column) offsets from the anchor (emap_api_terrain.hip: ellipse_spans)"""
    r = k // 2
    out = []
    for a in range(k):
        dy = a - r
        dx = int(np.rint(r * np.sqrt((r * r - dy * dy) / float(r * r)))) if r else 0
        out += [(dy, b - r) for b in range(max(r - dx, 0), min(r + dx + 1, k))]
    return tuple(out)


def erode(X, offsets):
    """a pixel keeps its label iff every pixel under the element has it; indices clamped at the edge (BORDER_REPLICATE)"""
    U = X.shape[0]
    h = max(max(abs(a), abs(b)) for a, b in offsets)
    P = np.pad(X, h, mode="edge")
    keep = X != 0
    for a, b in offsets:
        keep &= P[h + a:h + a + U, h + b:h + b + U] == X
    return np.where(keep, X, 0).astype(np.int32)


def zero_frame(X):
    X = X.copy()
    X[0, :] = X[-1, :] = X[:, 0] = X[:, -1] = 0
    return X


def inset(X, frame=True):
    """the cross erosion of extractBoundaryAndInset (:72-78), the image's outer rows and columns zeroed"""
    E = erode(X, CROSS)
    return zero_frame(E) if frame else E


# ---- 3. the fallback per label, stated locally ---------------------------------------------------------------------------------------------
def fallback_flags(Bm, n_labels):
    """flag[L]: some pixel of Bm with label L has an 8-neighbour in Bm with label L -- the label keeps the margin"""
    U = Bm.shape[0]
    P = np.pad(Bm, 1)
    hit = np.zeros((U, U), bool)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            if a or b:
                hit |= P[1 + a:1 + a + U, 1 + b:1 + b + U] == Bm
    flag = np.zeros(n_labels + 1, bool)
    flag[np.unique(Bm[hit & (Bm != 0)])] = True
    flag[0] = False
    return flag


def images(labels, n_labels, margin_size=1, mode=0, frame=True, fallback=True, edge3=False):
    """(A, B): the boundary image and the inset image.  mode 1: ``labels`` is a 0 / 1 mask, traced as it is"""
    labels = np.ascontiguousarray(labels, np.int32)
    if mode == 1:
        return labels.copy(), inset(labels, frame)
    up = upsample(labels, edge3)
    Am, Ac = erode(up, ellipse_offsets(2 * (1 + margin_size) + 1)), erode(up, CROSS)
    flag = fallback_flags(inset(Am, frame), n_labels) if fallback else np.ones(n_labels + 1, bool)
    A = np.where(flag[up], Am, Ac).astype(np.int32)
    return A, inset(A, frame)


# ---- 4. components ---------------------------------------------------------------------------------------------------------------------------
def components8(X, merge=True):
    """the root (smallest idx) of every pixel's 8-connected component of X != 0; -1 outside.  After a cross erosion two different labels
    are never 8-adjacent, so the components of the binary image are label-pure"""
    return ps.components(X != 0, 8, merge=merge).astype(np.int32)


# ---- 5. borders as crack cycles ------------------------------------------------------------------------------------------------------------
def _shift(P, a, b, U):
    return P[1 + a:1 + a + U, 1 + b:1 + b + U]


def crack_bits(X):
    """(U, U, 4) bool: crack (p, s) exists iff X[p] != 0 and the pixel across s is outside the image or has another value"""
    U = X.shape[0]
    P = np.pad(X, 1)
    return np.stack([(X != 0) & (_shift(P, *ACROSS[s], U) != X) for s in range(4)], axis=2)


def successors(X, conn8=True):
    """(raw, succ): the cracks of X in ascending index (raw = 4 idx + s) and every crack's successor as a COMPACT index.  ``conn8`` False:
    a lost piece of the tests, the turn to the diagonal neighbour dropped"""
    U = X.shape[0]
    P = np.pad(X, 1)
    bits = crack_bits(X)
    idx = np.arange(U * U).reshape(U, U)
    nxt = np.zeros((U, U, 4), np.int64)
    for s in range(4):
        d, b = TRAVEL[s], ACROSS[s]
        al = _shift(P, d[0], d[1], U) == X
        ar = _shift(P, b[0] + d[0], b[1] + d[1], U) == X
        right = ar if conn8 else (ar & al)
        o_ar = 4 * (idx + (b[0] + d[0]) * U + (b[1] + d[1])) + (s - 1) % 4
        o_al = 4 * (idx + d[0] * U + d[1]) + s
        o_p = 4 * idx + (s + 1) % 4
        nxt[:, :, s] = np.where(right, o_ar, np.where(al, o_al, o_p))
    flat = bits.ravel()
    raw = np.flatnonzero(flat)
    rank = np.cumsum(flat) - flat
    return raw.astype(np.int64), rank[nxt.ravel()[raw]].astype(np.int64)


def cycle_roots(succ):
    """every crack's ring: the smallest compact index of its cycle"""
    m, nx = np.arange(len(succ)), succ.copy()
    span = 1
    while span < max(len(succ), 1):
        m = np.minimum(m, m[nx])
        nx = nx[nx]
        span *= 2
    return m


def doubling_rounds(n):
    """ceil(log2 n) for n >= 2, else 1: 2^rounds steps reach every crack of the longest possible ring"""
    return max(int(n - 1).bit_length(), 1) if n >= 2 else 1


def vertex_flags(raw, succ, U):
    """v[k]: crack k is the LAST crack of its owner's run and the chain pixel's incoming step differs from its outgoing step
    (CHAIN_APPROX_SIMPLE); the single crack (p, 0) of an isolated pixel"""
    n = len(raw)
    own = raw >> 2
    pred = np.empty(n, np.int64)
    pred[succ] = np.arange(n)
    last = own[succ] != own
    f = np.arange(n)
    for _ in range(3):                                         # a run has at most 4 cracks
        back = pred[f]
        f = np.where(own[back] == own[f], back, f)
    r, c = own // U, own % U
    pin, nout = pred[f], succ
    v = last & ((r[f] - r[pin] != r[nout] - r) | (c[f] - c[pin] != c[nout] - c))
    s1 = succ
    s2 = succ[s1]
    s3 = succ[s2]
    alone = ((raw & 3) == 0) & (own[s1] == own) & (succ[s3] == np.arange(n))      # the ring IS the pixel's four sides (a pixel that hangs on a diagonal has the same run inside a longer ring)
    return (v | alone).astype(np.int64)


def rank_vertices(succ, cyc, v, rounds):
    """V[k]: the vertices from crack k (inclusive) to the end of its ring, by pointer doubling with the ring's root as terminal"""
    n = len(succ)
    k = np.arange(n)
    isroot = cyc == k
    nx = np.where(isroot, k, succ)
    V = np.where(isroot, 0, v)
    for _ in range(rounds):
        V = V + V[nx]
        nx = nx[nx]
    return V


def trace(X, roots, image, boundary_roots, conn8=True, rounds=None):
    """the rings of one image in ascending smallest crack, and their vertices (x = column, y = row) in ring order then chain order;
    ``rounds``: the doubling rounds (None: enough for this image on its own)"""
    U = X.shape[0]
    raw, succ = successors(X, conn8)
    n = len(raw)
    if n == 0:
        return np.zeros(0, RING_DTYPE), np.zeros((0, 2), np.int32)
    cyc = cycle_roots(succ)
    v = vertex_flags(raw, succ, U)
    V = rank_vertices(succ, cyc, v, doubling_rounds(n) if rounds is None else rounds)
    heads = np.flatnonzero(cyc == np.arange(n))
    rings = np.zeros(len(heads), RING_DTYPE)
    pix = raw[heads] >> 2
    nv = v[heads] + V[succ[heads]]
    rings["n_vertices"] = nv
    rings["first_vertex"] = np.cumsum(nv) - nv
    rings["image"] = image
    rings["label"] = X.ravel()[pix]
    rings["root"] = roots.ravel()[pix]
    rings["crack"] = raw[heads]
    rings["is_hole"] = ~((pix == rings["root"]) & ((raw[heads] & 3) == 0))
    rings["boundary"] = boundary_roots.ravel()[np.maximum(rings["root"], 0)]
    ring_of = np.cumsum(cyc == np.arange(n)) - 1                # compact index of a head -> ring
    ks = np.flatnonzero(v)
    head = cyc[ks]
    at = np.where(ks == head, 0, v[head] + V[succ[head]] - V[ks])
    pos = rings["first_vertex"][ring_of[head]] + at
    total = int(nv.sum())
    vertices = np.full((total, 2), -1, np.int32)
    keep = (at >= 0) & (at < nv[ring_of[head]])                # (a lost doubling round leaves positions that are not any)
    own = raw[ks] >> 2
    vertices[pos[keep], 0] = (own % U)[keep]
    vertices[pos[keep], 1] = (own // U)[keep]
    return rings, vertices


def trace_images(A, B, conn8=True, merge=True, short=0):
    """rings and vertices of both images, A's before B's -- the device's answer"""
    ra, rb = components8(A, merge), components8(B, merge)
    na, nb = int(crack_bits(A).sum()), int(crack_bits(B).sum())
    rounds = doubling_rounds(na + nb) - short
    rings_a, va = trace(A, ra, 0, ra, conn8, rounds)
    rings_b, vb = trace(B, rb, 1, ra, conn8, rounds)
    rings_b["first_vertex"] += len(va)
    return np.concatenate([rings_a, rings_b]), np.concatenate([va, vb]), ra, rb


def check_labels(labels, n_labels, margin_size, mode):
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[0] != labels.shape[1] or labels.shape[0] < 2:
        raise ValueError("labels must be a square plane of at least 2 x 2 cells")
    if mode not in (0, 1):
        raise ValueError("mode is 0 (regions) or 1 (raw mask)")
    if labels.shape[0] > (SIDE_MAX if mode == 0 else RAW_SIDE_MAX):
        raise ValueError("the plane is too large: crack indices are 32-bit")
    if mode == 0 and not 0 <= int(margin_size) <= MARGIN_MAX:
        raise ValueError("margin_size must lie in 0 .. %d" % MARGIN_MAX)
    if mode == 1 and ((labels != 0) & (labels != 1)).any():
        raise ValueError("a raw mask holds only 0 and 1")
    if mode == 0 and (int(n_labels) < 0 or (labels < 0).any() or (labels > int(n_labels)).any()):
        raise ValueError("labels must lie in 0 .. n_labels")


def trace_labels(labels, n_labels, margin_size=1, mode=0, *, conn8=True, merge=True, frame=True, fallback=True, edge3=False, short=0):
    """the contour stage on a label plane: a namespace of ``rings`` (RING_DTYPE), ``vertices`` int32 (n, 2), and the images ``A``, ``B``.
    The keywords behind ``mode`` are the tests' lost pieces"""
    check_labels(labels, n_labels, margin_size, mode)
    A, B = images(labels, n_labels, margin_size, mode, frame, fallback, edge3)
    rings, vertices, ra, rb = trace_images(A, B, conn8, merge, short)
    return types.SimpleNamespace(rings=rings, vertices=vertices, A=A, B=B, roots_a=ra, roots_b=rb)


# ---- 6. regions -----------------------------------------------------------------------------------------------------------------------------
def assemble(rings, vertices):
    """regions in ascending (label, boundary root): per region the boundary's outer ring, then its holes in ring order, then the insets
    in ascending root, each with its holes.  A list of dicts ``label``, ``root``, ``boundary`` and ``insets`` (a polygon: a dict of
    ``outer`` and ``holes``, int32 (n, 2) pixel arrays x = column, y = row).  An inset component of one pixel is no inset, a boundary
    component without inset is no region (ContourExtraction.cpp:85-99, :114)"""
    def poly(image, root):
        sel = np.flatnonzero((rings["image"] == image) & (rings["root"] == root))
        cut = [vertices[rings["first_vertex"][k]:rings["first_vertex"][k] + rings["n_vertices"][k]] for k in sel]
        outer = [c for k, c in zip(sel, cut) if not rings["is_hole"][k]]
        return dict(outer=outer[0], holes=[c for k, c in zip(sel, cut) if rings["is_hole"][k]])
    outs = rings[rings["is_hole"] == 0]
    bnd, ins = outs[outs["image"] == 0], outs[(outs["image"] == 1) & (outs["n_vertices"] > 1)]
    regions = []
    for b in np.sort(bnd, order=["label", "root"]):
        mine = np.sort(ins[ins["boundary"] == b["root"]], order="root")
        if len(mine):
            regions.append(dict(label=int(b["label"]), root=int(b["root"]), boundary=poly(0, b["root"]), insets=[poly(1, r) for r in mine["root"]]))
    return regions


def transform_plane_to_world(normal, support):
    """getTransformLocalToGlobal (PlanarRegion.cpp:5-29): a 4 x 4 double, the plane's frame in the map frame"""
    n = np.asarray(normal, np.float64)
    z = n / np.sqrt((n * n).sum())
    y = np.cross(z, np.array([1.0, 0.0, 0.0]))
    y2 = float((y * y).sum())
    if y2 > 1e-3:                                              # crossTolerance
        y = y / np.sqrt(y2)
    else:                                                      # the normal is almost unitX
        y = np.cross(z, np.cross(np.array([0.0, 1.0, 0.0]), z))
        y = y / np.sqrt((y * y).sum())
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = np.cross(y, z), y, z, np.asarray(support, np.float64)
    return T


def to_plane(pixels, T, resolution, origin_xy):
    """pixelToWorldFrame (ContourExtraction.cpp:139-142: x and y transposed) then projectToPlaneAlongGravity (PlanarRegion.cpp:31-50)"""
    px = np.asarray(pixels, np.float64).reshape(-1, 2)
    wx, wy = origin_xy[0] - resolution * px[:, 1], origin_xy[1] - resolution * px[:, 0]
    dx, dy = wx - T[0, 3], wy - T[1, 3]
    dz = (-dx * T[0, 2] - dy * T[1, 2]) / T[2, 2]
    d = np.stack([dx, dy, dz], axis=1)
    return np.stack([d @ T[:3, 0], d @ T[:3, 1]], axis=1)


def build_regions(rings, vertices, planes, resolution, origin_xy, scale=3.0):
    """the PlanarRegions of an answer: ``assemble`` plus, per region, the plane record of its label, ``transform_plane_to_world``, every
    ring also in plane coordinates (``*_plane`` keys) and ``bbox2d`` (xmin, ymin, xmax, ymax of the boundary's outer ring, plane
    coordinates).  A label without a plane record gets no region (the reference walks labelPlaneParameters)"""
    rec = {int(p["label"]): p for p in planes}
    out = []
    for g in assemble(rings, vertices):
        if g["label"] not in rec:
            continue
        p = rec[g["label"]]
        T = transform_plane_to_world(p["normal"], p["support"])
        conv = lambda q: dict(q, outer_plane=to_plane(q["outer"], T, resolution / scale, origin_xy),      # noqa: E731
                              holes_plane=[to_plane(h, T, resolution / scale, origin_xy) for h in q["holes"]])
        b = conv(g["boundary"])
        lo, hi = b["outer_plane"].min(axis=0), b["outer_plane"].max(axis=0)
        out.append(types.SimpleNamespace(label=g["label"], root=g["root"], plane=p, transform_plane_to_world=T, boundary=b,
                                         insets=[conv(q) for q in g["insets"]], bbox2d=(float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1]))))
    return out


def regions(labels, n_labels, planes, resolution, origin_xy, margin_size=1):
    """the host route of ``ElevationMap.get_planar_regions`` behind the terrain chain: ``rings``, ``vertices`` and ``regions``"""
    t = trace_labels(labels, n_labels, margin_size, 0)
    return types.SimpleNamespace(rings=t.rings, vertices=t.vertices, regions=build_regions(t.rings, t.vertices, planes, resolution, origin_xy))
