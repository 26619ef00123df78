"""CPU restatement of the map draw (include/dmslam_render.h; GlobalModel::renderPointCloud, GlobalModel.cpp:419-505) in numpy.

It follows DESIGN.md §4 R2, R3 and R6-R10 literally, in the same fp32 operation order as csrc/render.hip, but the way OpenGL
executes: per draw, per surfel (primitive), per triangle of its strip, with a depth-tested framebuffer — here a per-pixel minimum
over keys, which is the sequential GL_LESS result.  Test infrastructure, like oracle/.

Surfels are the structured records of fusion.SURFEL_DTYPE (pos4 col4 nrm4 times[8]).  Images are window rows (row 0 at the bottom).
"""
import numpy as np

F = np.float32
SUB = 256        # R6: 1/256 px snap
GUARD = F(255.0)  # R8: guard band
CLEARED = np.uint64(0xFFFFFFFFFFFFFFFF)
TU = np.array([-1, 1, -1, 1], F)
TV = np.array([-1, -1, 1, 1], F)
STRIP = ((0, 1, 2), (2, 1, 3))


def clip_of(M, x, y, z):
    """M (x, y, z, 1): rows accumulated left to right (arrays of any shape)."""
    M = np.asarray(M, F).reshape(16)
    return tuple((((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3]).astype(F) for r in range(4))


def mvp_from_pose(P, T):
    """dms_render_mvp_from_pose: P * diag(1, -1, -1, 1) * [R^T | -R^T t] in fp32."""
    P = np.asarray(P, F).reshape(16)
    T = np.asarray(T, F).reshape(16)
    V = np.zeros(16, F)
    for r in range(3):
        sg = F(1) if r == 0 else F(-1)
        V[4 * r + 0] = sg * T[0 + r]
        V[4 * r + 1] = sg * T[4 + r]
        V[4 * r + 2] = sg * T[8 + r]
        V[4 * r + 3] = sg * -((T[0 + r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11])
    V[15] = F(1)
    out = np.zeros(16, F)
    for r in range(4):
        for c in range(4):
            out[4 * r + c] = ((P[4 * r] * V[c] + P[4 * r + 1] * V[4 + c]) + P[4 * r + 2] * V[8 + c]) + P[4 * r + 3] * V[12 + c]
    return out.reshape(4, 4)


def depth24(zw):
    """R3: round(zw (2^24 - 1)) in fp64; 0xFFFFFFFF outside [0, 1] (and NaN)."""
    zw = np.asarray(zw, F)
    ok = (zw >= 0) & (zw <= 1)
    d = np.rint(np.where(ok, zw, F(0)).astype(np.float64) * 16777215.0).astype(np.int64)
    return np.where(ok, d, 0xFFFFFFFF).astype(np.int64)


def disc_corners(M, pos, nrm):
    """draw_global_surface.geom:185-212: clip-space corners (4 tuples of x, y, z, w arrays) of P + x, P + y, P - y, P - x."""
    nx, ny, nz, r = (nrm[:, k].astype(F) for k in range(4))
    vx, vy, vz = (ny - nz).astype(F), (-nx).astype(F), nx
    rn = (F(1) / np.sqrt(((vx * vx + vy * vy) + vz * vz).astype(F))).astype(F)
    xx, xy, xz = ((vx * rn) * r) * F(1.41421356), ((vy * rn) * r) * F(1.41421356), ((vz * rn) * r) * F(1.41421356)
    yx, yy, yz = ny * xz - nz * xy, nz * xx - nx * xz, nx * xy - ny * xx
    px, py, pz = pos[:, 0].astype(F), pos[:, 1].astype(F), pos[:, 2].astype(F)
    return [clip_of(M, px + xx, py + xy, pz + xz), clip_of(M, px + yx, py + yy, pz + yz),
            clip_of(M, px - yx, py - yy, pz - yz), clip_of(M, px - xx, py - xy, pz - xz)]


def plane_dist(c, k):
    x, y, z, w = c
    gw = GUARD * w
    return (z + w, gw - x, gw + x, gw - y, gw + y)[k]


def to_window(c, W, H):
    x, y, z, w = c
    hw, hh = F(W * 0.5), F(H * 0.5)
    xn, yn, zn = x / w, y / w, z / w
    X = np.rint(((xn + F(1)) * hw) * F(SUB)).astype(np.int64)
    Y = np.rint(((yn + F(1)) * hh) * F(SUB)).astype(np.int64)
    return X, Y, (zn * F(0.5) + F(0.5)).astype(F), (F(1) / w).astype(F)


def first_px(lo):
    return -((SUB // 2 - lo) >> 8)


def last_px(hi):
    return (hi - SUB // 2) >> 8


def raster_triangles(tri, W, H, key_lo, shift, zbuf):
    """R6 / R7 / R10 for a batch of triangles: tri = dict of v{0,1,2}_{X,Y,z,iw,u,v} arrays; key_lo, shift per triangle.  Keys go
    into zbuf (flat H*W uint64) by minimum."""
    g = {k: np.asarray(v) for k, v in tri.items()}
    n = len(g["v0_X"])
    if n == 0:
        return
    X0, Y0, X1, Y1, X2, Y2 = (g["v0_X"], g["v0_Y"], g["v1_X"], g["v1_Y"], g["v2_X"], g["v2_Y"])
    area = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0)
    sw = area < 0
    def pick(a, b):  # v1 / v2 swapped where the area is negative
        return np.where(sw, b, a), np.where(sw, a, b)
    V = {"0": {k: g["v0_" + k] for k in ("X", "Y", "z", "iw", "u", "v")}, "1": {}, "2": {}}
    for k in ("X", "Y", "z", "iw", "u", "v"):
        V["1"][k], V["2"][k] = pick(g["v1_" + k], g["v2_" + k])
    area = np.abs(area)
    keep = area != 0
    # triangle bounding box of pixel centres, clamped to the viewport
    Xs = np.stack([V[i]["X"] for i in "012"])
    Ys = np.stack([V[i]["Y"] for i in "012"])
    x0 = np.maximum(first_px(Xs.min(0)), 0)
    x1 = np.minimum(last_px(Xs.max(0)), W - 1)
    y0 = np.maximum(first_px(Ys.min(0)), 0)
    y1 = np.minimum(last_px(Ys.max(0)), H - 1)
    keep &= (x1 >= x0) & (y1 >= y0)
    idx = np.nonzero(keep)[0]
    if len(idx) == 0:
        return
    bw = (x1 - x0 + 1)[idx]
    bh = (y1 - y0 + 1)[idx]
    cnt = bw * bh
    # chunks of at most ~4 M (triangle, pixel) pairs
    starts = np.concatenate([[0], np.cumsum(cnt)])
    lim = 1 << 22
    lo = 0
    while lo < len(idx):
        hi = lo + 1
        while hi < len(idx) and starts[hi + 1] - starts[lo] <= lim:
            hi += 1
        sel = idx[lo:hi]
        c = cnt[lo:hi]
        t = np.repeat(np.arange(len(sel)), c)
        off = np.arange(int(c.sum())) - np.repeat(starts[lo:hi] - starts[lo], c)
        tb = sel[t]
        px = x0[tb] + off % bw[lo:hi][t]
        py = y0[tb] + off // bw[lo:hi][t]
        Px = px.astype(np.int64) * SUB + SUB // 2
        Py = py.astype(np.int64) * SUB + SUB // 2
        e, inside = [], np.ones(len(tb), bool)
        for a, b in (("1", "2"), ("2", "0"), ("0", "1")):
            ax, ay = V[a]["X"][tb], V[a]["Y"][tb]
            dx, dy = V[b]["X"][tb] - ax, V[b]["Y"][tb] - ay
            ek = dx * (Py - ay) - dy * (Px - ax)
            tl = (dy < 0) | ((dy == 0) & (dx < 0))
            inside &= (ek > 0) | ((ek == 0) & tl)
            e.append(ek)
        inv = (F(1) / area[tb].astype(np.float64).astype(F)).astype(F)
        b = [(ek.astype(np.float64).astype(F) * inv).astype(F) for ek in e]
        v0, v1, v2 = (V[i] for i in "012")
        z = ((b[0] * v0["z"][tb] + b[1] * v1["z"][tb]) + b[2] * v2["z"][tb]).astype(F)
        with np.errstate(all="ignore"):
            inside &= (z >= 0) & (z <= 1)
            q0, q1, q2 = b[0] * v0["iw"][tb], b[1] * v1["iw"][tb], b[2] * v2["iw"][tb]
            den = (q0 + q1) + q2
            u = ((q0 * v0["u"][tb] + q1 * v1["u"][tb]) + q2 * v2["u"][tb]) / den
            v = ((q0 * v0["v"][tb] + q1 * v1["v"][tb]) + q2 * v2["v"][tb]) / den
            inside &= ~((u * u + v * v).astype(F) > 1)
            zf = np.fmin(np.fmax((z + shift[tb]).astype(F), F(0)), F(1))
        d = depth24(zf)
        inside &= d < 0xFFFFFF
        key = (d[inside].astype(np.uint64) << np.uint64(40)) | key_lo[tb][inside]
        np.minimum.at(zbuf, (py[inside] * W + px[inside]).astype(np.int64), key)
        lo = hi


def clip_polygon(poly):
    """R8: Sutherland-Hodgman against near, then the four guard planes; new vertices from the inside end.  poly: list of
    (x, y, z, w, u, v) float32 tuples."""
    for k in range(5):
        out = []
        n = len(poly)
        for i in range(n):
            A, B = poly[i], poly[(i + 1) % n]
            da, db = plane_dist(A[:4], k), plane_dist(B[:4], k)
            ia, ib = da >= 0, db >= 0
            if ia:
                out.append(A)
            if ia != ib:
                I, O = (A, B) if ia else (B, A)
                di, do = (da, db) if ia else (db, da)
                t = F(di / (di - do))
                out.append(tuple(F(I[j] + t * (O[j] - I[j])) for j in range(6)))
        poly = out
        if not poly:
            break
    return poly


def disc_keys(surf, M, W, H, threshold, unstable, seq, zbuf):
    """Pass 1 of the disc program for one draw: keys of every fragment into zbuf."""
    n = len(surf)
    if n == 0:
        return
    pos, nrm = surf["pos"].astype(F), surf["nrm"].astype(F)
    ids = np.arange(n, dtype=np.uint64)
    drawn = (pos[:, 3] > F(threshold)) | bool(unstable)
    cv = disc_corners(M, pos, nrm)
    oc = [np.zeros(n, np.int64) for _ in range(4)]
    for k in range(4):
        for p in range(5):
            oc[k] |= (~(plane_dist(cv[k], p) >= 0)).astype(np.int64) << p
    clipped = (oc[0] | oc[1] | oc[2] | oc[3]) != 0
    rejected = (oc[0] & oc[1] & oc[2] & oc[3]) != 0
    shift = np.where(pos[:, 3] <= F(threshold), nrm[:, 3], F(0)).astype(F)
    key_lo = (np.uint64(seq) << np.uint64(32)) | ids
    simple = np.nonzero(drawn & ~clipped)[0]
    wv = [to_window(tuple(a[simple] for a in cv[k]), W, H) for k in range(4)]
    for tri in STRIP:
        t = {}
        for slot, k in enumerate(tri):
            X, Y, z, iw = wv[k]
            t["v%d_X" % slot], t["v%d_Y" % slot], t["v%d_z" % slot], t["v%d_iw" % slot] = X, Y, z, iw
            t["v%d_u" % slot] = np.full(len(simple), TU[k], F)
            t["v%d_v" % slot] = np.full(len(simple), TV[k], F)
        raster_triangles(t, W, H, key_lo[simple], shift[simple], zbuf)
    for i in np.nonzero(drawn & clipped & ~rejected)[0]:
        corners = [tuple(F(cv[k][j][i]) for j in range(4)) + (TU[k], TV[k]) for k in range(4)]
        for tri in STRIP:
            poly = clip_polygon([corners[k] for k in tri])
            if len(poly) < 3 or not all(v[3] > 0 for v in poly):
                continue
            wvs = [to_window(tuple(np.array([v[j]], F) for j in range(4)), W, H) + (np.array([v[4]], F), np.array([v[5]], F))
                   for v in poly]
            for k in range(2, len(poly)):
                t = {}
                for slot, w in enumerate((wvs[0], wvs[k - 1], wvs[k])):
                    for name, val in zip(("X", "Y", "z", "iw", "u", "v"), w):
                        t["v%d_%s" % (slot, name)] = val
                raster_triangles(t, W, H, key_lo[i:i + 1], shift[i:i + 1], zbuf)


def point_keys(surf, M, W, H, threshold, seq, zbuf):
    """Pass 1 of the point program (R2)."""
    n = len(surf)
    if n == 0:
        return
    pos = surf["pos"].astype(F)
    x, y, z, w = clip_of(M, pos[:, 0], pos[:, 1], pos[:, 2])
    with np.errstate(all="ignore"):
        xn, yn, zn = x / w, y / w, z / w
        ok = (pos[:, 3] > F(threshold)) & (w > 0)
        ok &= (xn >= -1) & (xn <= 1) & (yn >= -1) & (yn <= 1) & (zn >= -1) & (zn <= 1)
        pxf = np.floor((xn + F(1)) * F(W * 0.5))
        pyf = np.floor((yn + F(1)) * F(H * 0.5))
    px = np.where(ok, pxf, -1).astype(np.int64)
    py = np.where(ok, pyf, -1).astype(np.int64)
    ok &= (px >= 0) & (py >= 0) & (px < W) & (py < H)
    d = depth24((zn * F(0.5) + F(0.5)).astype(F))
    ok &= d < 0xFFFFFF
    i = np.nonzero(ok)[0]
    key = (d[i].astype(np.uint64) << np.uint64(40)) | (np.uint64(seq) << np.uint64(32)) | i.astype(np.uint64)
    np.minimum.at(zbuf, py[i] * W + px[i], key)


def surfel_colour(s, p):
    """draw_global_surface.geom:123-182 (discs) / draw_feedback.vert:297-314 (points) for the surfels `s` (records) under draw
    parameters p; float32 (n, 3)."""
    n = len(s)
    nrm, col, times = s["nrm"].astype(F), s["col"].astype(F), s["times"].astype(F)
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    sabs = np.abs((nx + ny) + nz).astype(F)
    points = p.get("draw_points", False)
    ct = p.get("color_type", 0)
    with np.errstate(all="ignore"):
        if p.get("cluster_color") is not None:
            c = np.tile(np.asarray(p["cluster_color"], F), (n, 1))
        elif ct == 1:
            c = nrm[:, :3].copy()
        elif ct == 2:
            ci = col[:, 0].astype(np.int64)
            c = np.stack([((ci >> 16) & 0xFF).astype(F) / F(255), ((ci >> 8) & 0xFF).astype(F) / F(255), (ci & 0xFF).astype(F) / F(255)], 1)
        elif not points and ct == 3:
            ratio = (F(2) * (col[:, 2] - F(1))) / (F(p["time"]) - F(1))
            x = np.fmax(F(0), F(1) - ratio)
            y = np.fmax(F(0), ratio - F(1))
            z = (F(1) - x) - y
            sc = sabs + F(0.1)
            c = np.stack([x * sc, y * sc, z * sc], 1)
        elif not points and ct == 4:
            s0, s1, s2 = times[:, 0] != F(-3), times[:, 1] != F(-3), times[:, 2] != F(-3)
            z0 = F(0)
            g = (np.where(s0, z0, z0) + np.where(s1, F(0.8), z0)) + np.where(s2, z0, z0)
            r = (np.where(s0, z0, z0) + np.where(s1, F(0.1), z0)) + np.where(s2, F(0.8), z0)
            b = (np.where(s0, F(0.8), z0) + np.where(s1, F(0.2), z0)) + np.where(s2, z0, z0)
            total = (s0.astype(np.int32) + s1.astype(np.int32) + s2.astype(np.int32)).astype(F)
            c = np.stack([(r / total) * sabs + F(0.1), (g / total) * sabs + F(0.1), (b / total) * sabs + F(0.1)], 1)
        else:
            gr = F(0.5) * sabs + F(0.1)
            c = np.stack([gr, gr, gr], 1)
        c = c.astype(F)
        if not points and p.get("draw_window", False):
            dt = (F(p["time"]) - times[:, p.get("time_idx", 0)]).astype(F)
            td = F(p.get("time_delta", 0))
            c = np.where((dt > td)[:, None], c * F(0.25), c)
            c = np.where((dt < td)[:, None], c * np.array([0, 1, 0], F), c)
    return c.astype(F)


def rgba8(c):
    """R9: floor(clamp(c, 0, 1) 255 + 0.5), alpha 255; a channel that is not finite (NaN, +-inf) writes 0."""
    with np.errstate(invalid="ignore"):
        b = np.where(np.isfinite(c), np.floor(np.fmin(np.fmax(c, F(0)), F(1)) * F(255) + F(0.5)), F(0)).astype(np.uint8)
    return np.concatenate([b, np.full((len(b), 1), 255, np.uint8)], 1)


class Target:
    """The render target of dmslam_render.h: colour (H, W, 4) u8, depth24 (H, W) u32, key (H, W) u64."""

    def __init__(self, W, H, clear_rgba=(0, 0, 0, 0)):
        self.W, self.H = W, H
        self.clear(clear_rgba)

    def clear(self, rgba=(0, 0, 0, 0)):
        c = np.floor(np.fmin(np.fmax(np.asarray(rgba, F), F(0)), F(1)) * F(255) + F(0.5)).astype(np.uint8)
        self.color = np.tile(c, (self.H, self.W, 1))
        self.depth = np.full((self.H, self.W), 0xFFFFFF, np.uint32)
        self.key = np.full(self.H * self.W, CLEARED, np.uint64)
        self.seq = 0

    def draw(self, surf, mvp, pose=None, **p):
        """One draw: p = threshold, draw_unstable, draw_points, draw_window, color_type, time, time_idx, time_delta, cluster_color.
        With pose, mvp is the projection (dms_render_mvp_from_pose)."""
        M = np.asarray(mvp, F) if pose is None else mvp_from_pose(mvp, pose)
        kb = np.full(self.H * self.W, CLEARED, np.uint64)
        if p.get("draw_points", False):
            point_keys(surf, M, self.W, self.H, p.get("threshold", 0.0), self.seq, kb)
        else:
            disc_keys(surf, M, self.W, self.H, p.get("threshold", 0.0), p.get("draw_unstable", False), self.seq, kb)
        won = kb < self.key
        self.key = np.minimum(self.key, kb)
        pix = np.nonzero(won)[0]
        ids = (self.key[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if len(pix):
            col = rgba8(surfel_colour(surf[ids], p))
            self.color.reshape(-1, 4)[pix] = col
            self.depth.reshape(-1)[pix] = (self.key[pix] >> np.uint64(40)).astype(np.uint32)
        self.seq += 1

    def images(self, image_order=False):
        out = (self.color.copy(), self.depth.copy(), self.key.reshape(self.H, self.W).copy())
        return tuple(a[::-1].copy() for a in out) if image_order else out


# ---- tests/golden/ref_render.npz: the reference's draw programs on Mesa llvmpipe -------------------------------------------------
def fixture_map(z):
    """the fixture's surfels as records of fusion.SURFEL_DTYPE's layout (pos4 col4 nrm4 times[8], sensors 3..7 never seen)"""
    dt = np.dtype([("pos", "<f4", (4,)), ("col", "<f4", (4,)), ("nrm", "<f4", (4,)), ("times", "<f4", (8,))])
    s = np.zeros(len(z["pos"]), dt)
    s["pos"], s["col"], s["nrm"] = z["pos"], z["col"], z["nrm"]
    s["times"][:] = -3
    s["times"][:, :3] = z["times"]
    return s


def fixture_draws(z, name):
    import json

    draws = json.loads(str(z[name + "__draws"]))
    for p in draws:
        if p.get("cluster_color") is not None:
            p["cluster_color"] = tuple(p["cluster_color"])
    return draws


def fixture_stats(z, name, rgba, depth):
    """Counted mismatches of (rgba, depth) against the llvmpipe images of case `name`, as fractions of llvmpipe's covered pixels:
    coverage (covered on one side only), depth (both covered, 24-bit depths more than 1 apart), colour (both covered, depths within 1,
    a channel more than 1 apart)."""
    c, d = z[name + "__rgba"], z[name + "__depth"]
    cg, cr = d < 0xFFFFFF, depth < 0xFFFFFF
    n = max(1, int(cg.sum()))
    both = cg & cr
    dd = np.abs(d.astype(np.int64) - depth.astype(np.int64))
    near = both & (dd <= 1)
    bd = np.abs(c.astype(np.int64) - rgba.astype(np.int64)).max(-1)
    return {"covered": int(cg.sum()), "coverage": (cg != cr).sum() / n, "depth": (both & (dd > 1)).sum() / n,
            "colour": (near & (bd > 1)).sum() / n}


# bounds the counted mismatches stay inside: measured on the committed fixture, restatement and HIP alike
FIXTURE_BOUNDS = {"coverage": 0.0075, "colour": 0.005, "depth_discs": 0.25, "depth_points": 0.0}
