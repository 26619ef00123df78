"""CPU restatement of the live-frame cloud draw (include/dmslam_render_cloud.h; FeedbackBuffer::compute + ::render,
Core/src/Shaders/FeedbackBuffer.cpp:84-187) in numpy, on top of tests/render_ref.py.

The way the reference executes it: first the per-buffer vertex stage (vertex_feedback.vert + .geom with geometry.glsl / surfels.glsl /
color.glsl) makes the compacted vertex list of ONE metric depth image in column-major pixel order, then the point program
(draw_feedback.{vert,frag}) draws that list with MVP * pose.  DESIGN.md §4 R1-R3, R9 and R19-R21, in the fp32 operation order of
csrc/render.hip.  Test infrastructure, like oracle/.
"""
import numpy as np

import render_ref as R

F = np.float32
RAW, FILTERED = 0, 1


def uv_coord(i, n):
    """the uv buffer's entry (FeedbackBuffer.cpp:38-46): ((float)i / (float)n) + 1.0 / (2 * (float)n) in double, stored as float"""
    i = np.asarray(i)
    return ((i.astype(F) / F(n)).astype(np.float64) + 1.0 / np.float64(F(2) * F(n))).astype(F)


def texel(u, n):
    """R1: NEAREST texel floor(u n) in fp32, CLAMP_TO_EDGE"""
    return np.clip(np.floor((u * F(n)).astype(F)), 0, n - 1).astype(np.int64)


def vertex(depth, sx, sy, x, y, cam):
    """geometry.glsl getVertex: ((x - cx) z) / fx with cam = (cx, cy, 1/fx, 1/fy)"""
    cx, cy, ifx, ify = cam
    z = depth[sy, sx].astype(F)
    return (((x - cx) * z) * ifx).astype(F), (((y - cy) * z) * ify).astype(F), z


def clip_of4(M, x, y, z, w):
    """M (x, y, z, w): rows accumulated left to right"""
    M = np.asarray(M, F).reshape(16)
    return tuple((((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] * w).astype(F) for r in range(4))


def cloud_clip(mvp_eff, model_pose, x, y, z):
    """R19: MVP * (pose * (p, 1)) in fp32, two matrix-vector products (dms_render_cloud_clip)"""
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    return clip_of4(mvp_eff, *clip_of4(model_pose, x, y, z, np.ones_like(x)))


def product_first_clip(mvp_eff, model_pose, x, y, z):
    """the OTHER grouping, (MVP * pose) * (p, 1) with a 4 x 4 product first - not the rule; for the test of R19"""
    A, B = np.asarray(mvp_eff, F).reshape(4, 4), np.asarray(model_pose, F).reshape(4, 4)
    M = np.zeros((4, 4), F)
    for r in range(4):
        for c in range(4):
            M[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return R.clip_of(M, np.asarray(x, F), np.asarray(y, F), np.asarray(z, F))


def feedback_vertices(rgba, depth, K, max_depth):
    """FeedbackBuffer::compute over one metric depth image: the emitted vertices in buffer order (column-major), as a dict of
    e (source pixel x * rows + y), pos (n, 3), conf (bool: confidence(x, y, 1) > 0), nrm (n, 3), rgb (n, 3) bytes."""
    depth = np.asarray(depth, F)
    rows, cols = depth.shape
    fx, fy, cx, cy = (F(v) for v in K)
    cam = (cx, cy, F(1) / fx, F(1) / fy)
    with np.errstate(all="ignore"):
        keep = (depth > 0) & ~(depth > F(max_depth))  # vertex_feedback.vert:55-62, .geom:38
        px, py = np.nonzero(keep.T)                   # column-major: x outer, y inner
        tx, ty = uv_coord(px, cols), uv_coord(py, rows)
        x, y = (tx * F(cols)).astype(F), (ty * F(rows)).astype(F)
        vx, vy, vz = vertex(depth, px, py, x, y, cam)
        # surfels.glsl confidence(x, y, 1) > 0: the library's exp flushes arguments below -87 to 0 (detmath.hpp)
        dx, dy = x - cx, y - cy
        rd = (np.sqrt((dx * dx + dy * dy).astype(F)).astype(F) / F(400)).astype(F)
        arg = (-(rd * rd).astype(F) / F(0.72)).astype(F)
        conf = ~(arg < F(-87)) & ~np.isnan(arg)
        # geometry.glsl getNormal: central differences over the SAME depth image, taps by R1 (R20)
        sx, sy = texel(tx, cols), texel(ty, rows)
        icol, irow = F(1) / F(cols), F(1) / F(rows)
        xf = vertex(depth, texel(tx + icol, cols), sy, x + F(1), y, cam)
        xb = vertex(depth, texel(tx - icol, cols), sy, x - F(1), y, cam)
        yf = vertex(depth, sx, texel(ty + irow, rows), x, y + F(1), cam)
        yb = vertex(depth, sx, texel(ty - irow, rows), x, y - F(1), cam)
        v = (vx, vy, vz)
        del_x = [(((xb[k] + v[k]) / F(2)) - ((xf[k] + v[k]) / F(2))).astype(F) for k in range(3)]
        del_y = [(((yb[k] + v[k]) / F(2)) - ((yf[k] + v[k]) / F(2))).astype(F) for k in range(3)]
        c = [del_x[1] * del_y[2] - del_x[2] * del_y[1], del_x[2] * del_y[0] - del_x[0] * del_y[2], del_x[0] * del_y[1] - del_x[1] * del_y[0]]
        rn = (F(1) / np.sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]).astype(F)).astype(F)).astype(F)
        nrm = np.stack([c[0] * rn, c[1] * rn, c[2] * rn], 1).astype(F)
    rgb = np.asarray(rgba, np.uint8)[py, px, :3]
    return {"e": (px * rows + py).astype(np.uint64), "pos": np.stack([vx, vy, vz], 1).astype(F), "conf": conf, "nrm": nrm, "rgb": rgb}


def cloud_colour(v, color_type):
    """draw_feedback.vert:39-54 (no cluster colour): float32 (n, 3)"""
    with np.errstate(all="ignore"):
        if color_type == 1:
            return v["nrm"].copy()
        if color_type == 2:  # decodeColor(encodeColor(c)): the bytes over 255
            return (v["rgb"].astype(F) / F(255)).astype(F)
        n = v["nrm"]
        g = (F(0.5) * np.abs((n[:, 0] + n[:, 1]) + n[:, 2]).astype(F) + F(0.1)).astype(F)
        return np.stack([g, g, g], 1)


def draw_cloud(target, rgba, depth, K, max_depth, mvp, model_pose=None, color_type=0, pose=None, product_first=False):
    """One cloud draw into a render_ref.Target.  With pose, mvp is the projection (view pose in HBM: dms_render_mvp_from_pose).
    product_first=True groups the matrices the OTHER way, (MVP * pose) * v - not the rule; for the test of R19."""
    t = target
    V = np.asarray(mvp, F).reshape(4, 4) if pose is None else R.mvp_from_pose(mvp, pose)
    P = np.eye(4, dtype=F) if model_pose is None else np.asarray(model_pose, F).reshape(4, 4)
    v = feedback_vertices(rgba, depth, K, max_depth)
    pos = v["pos"]
    x, y, z, w = (product_first_clip if product_first else cloud_clip)(V, P, pos[:, 0], pos[:, 1], pos[:, 2])
    kb = np.full(t.H * t.W, R.CLEARED, np.uint64)
    with np.errstate(all="ignore"):  # R2 / R3, as render_ref.point_keys
        xn, yn, zn = x / w, y / w, z / w
        ok = v["conf"] & (w > 0)
        ok &= (xn >= -1) & (xn <= 1) & (yn >= -1) & (yn <= 1) & (zn >= -1) & (zn <= 1)
        pxf = np.floor((xn + F(1)) * F(t.W * 0.5))
        pyf = np.floor((yn + F(1)) * F(t.H * 0.5))
    px = np.where(ok, pxf, -1).astype(np.int64)
    py = np.where(ok, pyf, -1).astype(np.int64)
    ok &= (px >= 0) & (py >= 0) & (px < t.W) & (py < t.H)
    d = R.depth24((zn * F(0.5) + F(0.5)).astype(F))
    ok &= d < 0xFFFFFF
    i = np.nonzero(ok)[0]
    key = (d[i].astype(np.uint64) << np.uint64(40)) | (np.uint64(t.seq) << np.uint64(32)) | v["e"][i]  # R21
    np.minimum.at(kb, py[i] * t.W + px[i], key)
    won = kb < t.key
    t.key = np.minimum(t.key, kb)
    pix = np.nonzero(won)[0]
    if len(pix):
        idx = np.searchsorted(v["e"], t.key[pix] & np.uint64(0xFFFFFFFF))
        sel = {k: a[idx] for k, a in v.items()}
        t.color.reshape(-1, 4)[pix] = R.rgba8(cloud_colour(sel, color_type))
        t.depth.reshape(-1)[pix] = (t.key[pix] >> np.uint64(40)).astype(np.uint32)
    t.seq += 1


# ---- tests/golden/ref_render_cloud.npz: vertex_feedback.* + draw_feedback.* on Mesa llvmpipe --------------------------------------
# The counted mismatches (render_ref.fixture_stats) stay inside render_ref.FIXTURE_BOUNDS' coverage / colour / depth_points (= 0),
# the bounds of the map's point draw, with ONE exception measured on the restatement against llvmpipe:
# the RAW buffer's 24-bit depths.  The context's raw metric depth texture is LINEAR-filtered (Context.h:171-177) where R1 / R20 take
# the NEAREST texel: the fp32 texel coordinate u * cols - 0.5 of the uv buffer is not an integer at 16 % of the columns and 12 % of
# the rows, so llvmpipe's z mixes in a neighbour (3 % of the pixels read the previous texel at weight 0.99999905) and the depth moves
# by a few units of 2^-24.  Measured pixels with depths more than 1 apart: tracked 200 of 18629, oblique 111 of 9842 (0 and 43 when the
# restatement samples z LINEAR as well); the FILTERED buffer (a NEAREST texture): 0.  The bounds are those counts plus one pixel.
FIXTURE_DEPTH_RAW_PIXELS = {"tracked": 201, "oblique": 112}


def fixture_case(z, name):
    """(buffer, color_type, view name) of a fixture case"""
    import json

    return json.loads(str(z[name + "__case"]))


def fixture_run(z, name):
    """the restatement's (rgba, depth24, key) of a fixture case"""
    c = fixture_case(z, name)
    h, w = z[name + "__depth"].shape
    t = R.Target(w, h, tuple(z["clear"]))
    draw_cloud(t, z["rgba"], z["depth_raw"] if c["buffer"] == "RAW" else z["depth_filtered"], tuple(float(v) for v in z["K"]),
               float(z["max_depth"]), z[c["view"] + "__mvp"], z["pose"], c["color_type"])
    return t.images()


def check_fixture_stats(z, name, st):
    """the bounds above on the counted mismatches `st` (render_ref.fixture_stats) of a case"""
    c, b = fixture_case(z, name), R.FIXTURE_BOUNDS
    assert st["covered"] > 0
    assert st["coverage"] <= b["coverage"] and st["colour"] <= b["colour"], (name, st)
    if c["buffer"] == "RAW":
        assert round(st["depth"] * st["covered"]) <= FIXTURE_DEPTH_RAW_PIXELS[c["view"]], (name, st)
    else:
        assert st["depth"] <= b["depth_points"], (name, st)
