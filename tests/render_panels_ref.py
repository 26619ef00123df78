"""CPU restatement of the view's image panels (include/dmslam_render_panels.h; GUI/src/MainController.cpp:649-664) in numpy, on top of
tests/render_ref.py for the target model and the byte conversion R9: the two shader passes (depth_norm.frag through
ComputePack::compute, visualise_textures.frag through IndexMap::renderDepth) and GUI::displayImg's flipped, stretched, textured quad.
DESIGN.md §4 R9 and R22-R26, in the fp32 operation order of csrc/render.hip.  Test infrastructure, like oracle/.

Source images are in image order (row 0 = top), the target's rows are window rows (row 0 = bottom).
"""
import numpy as np

import render_ref as R

F = np.float32
RGBA8, L8 = 0, 1
NEAREST, LINEAR = 0, 1
DEPTH_NORM, MODEL, RGB, MODEL_IMAGE = 0, 1, 2, 3
FILTERS = {DEPTH_NORM: LINEAR, MODEL: NEAREST, RGB: LINEAR, MODEL_IMAGE: NEAREST}


def unorm8(v):
    """R9 of one channel (R.rgba8 without the alpha it appends)"""
    v = np.asarray(v, F)
    return R.rgba8(v.reshape(-1, 1))[:, 0].reshape(v.shape)


def to_uint(x):
    """GLSL's uint(float) as the library fixes it: clamped to [0, 2^32 - 1], 0 for NaN"""
    x = F(x)
    return 0 if not x > 0 else 0xFFFFFFFF if x >= F(4294967296.0) else int(x)


def depth_norm(depth_u16, min_val, max_val):
    """depth_norm.frag stored by R26: (H, W) u8"""
    v = np.asarray(depth_u16, np.uint16).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = (F(1.0) - v.astype(F) / F(max_val)).astype(F)
    return np.where((v > to_uint(min_val)) & (v < to_uint(max_val)), unorm8(val), 0).astype(np.uint8)


def model_depth_image(vertex, max_depth):
    """visualise_textures.frag into the cleared drawTexture: (H, W, 4) u8"""
    z = np.asarray(vertex, F)[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        b = unorm8((F(1.0) - (z / F(max_depth)).astype(F)).astype(F))
        keep = ~((z > F(max_depth)) | (z <= F(0)))
    return np.where(keep[..., None], np.repeat(b[..., None], 4, -1), 0).astype(np.uint8)


def texels(image, fmt):
    """R25: the image as floats (H, W, 4): byte / 255, luminance as (L, L, L, 1)"""
    image = np.asarray(image, np.uint8)
    if fmt == L8:
        l = (image.astype(F) / F(255)).astype(F)
        return np.stack([l, l, l, np.ones_like(l)], -1)
    return (image.astype(F) / F(255)).astype(F)


def blit_block(image, fmt, filt, vw, vh, color=(1, 1, 1)):
    """The vh x vw block of colour bytes a blit writes, in WINDOW rows (row 0 = the viewport's bottom row): R22-R25"""
    tex = texels(image, fmt)
    SH, SW = tex.shape[:2]
    i, j = np.arange(vw), np.arange(vh)
    u = (((i.astype(F) + F(0.5)) / F(vw)).astype(F) * F(SW)).astype(F)
    v = ((((vh - 1 - j).astype(F) + F(0.5)) / F(vh)).astype(F) * F(SH)).astype(F)
    if filt == NEAREST:
        ix = np.minimum(np.floor(u).astype(np.int64), SW - 1)
        iy = np.minimum(np.floor(v).astype(np.int64), SH - 1)
        c = tex[iy[:, None], ix[None, :]]
    else:
        x, y = (u - F(0.5)).astype(F), (v - F(0.5)).astype(F)
        fx, fy = np.floor(x), np.floor(y)
        ax, ay = (x - fx).astype(F)[None, :, None], (y - fy).astype(F)[:, None, None]
        i0, i1 = np.clip(fx.astype(np.int64), 0, SW - 1), np.clip(fx.astype(np.int64) + 1, 0, SW - 1)
        j0, j1 = np.clip(fy.astype(np.int64), 0, SH - 1), np.clip(fy.astype(np.int64) + 1, 0, SH - 1)
        t00, t10 = tex[j0[:, None], i0[None, :]], tex[j0[:, None], i1[None, :]]
        t01, t11 = tex[j1[:, None], i0[None, :]], tex[j1[:, None], i1[None, :]]
        one = F(1)
        w00, w10 = ((one - ax) * (one - ay)).astype(F), (ax * (one - ay)).astype(F)
        w01, w11 = ((one - ax) * ay).astype(F), (ax * ay).astype(F)
        c = (((w00 * t00 + w10 * t10).astype(F) + w01 * t01).astype(F) + w11 * t11).astype(F)
    m = np.array([color[0], color[1], color[2], 1.0], F)
    return unorm8((c * m).astype(F))


def blit(target, image, fmt, filt, vp, color=(1, 1, 1)):
    """dms_render_blit into an R.Target: colour only; depth, key and seq stay"""
    x, y, w, h = vp
    assert w > 0 and h > 0 and x >= 0 and y >= 0 and x + w <= target.W and y + h <= target.H
    target.color[y:y + h, x:x + w] = blit_block(image, fmt, filt, w, h, color)


def draw_panels(target, rgba, depth_u16, model_rgba, vertex, viewports, depth_cutoff, mask=15):
    """dms_fusion_draw_panels as the separate calls in the reference's order; returns (DEPTH_NORM, Model image)"""
    norm = depth_norm(depth_u16, F(0.3) * F(1000), F(depth_cutoff) * F(1000))
    model = model_depth_image(vertex, depth_cutoff)
    src = {DEPTH_NORM: (norm, L8), MODEL: (model, RGBA8), RGB: (rgba, RGBA8), MODEL_IMAGE: (model_rgba, RGBA8)}
    for k in range(4):
        if (mask >> k) & 1:
            blit(target, src[k][0], src[k][1], FILTERS[k], viewports[k])
    return norm, model


# ---- tests/golden/ref_render_panels.npz: the reference's shader programs and a textured quad on Mesa llvmpipe ---------------------
# DESIGN §5.  (mismatching bytes, largest byte difference) of the restatement against the fixture, measured when the fixture was made;
# the tests bound each count at the recorded value plus one and each difference at the recorded value.  Both shader passes and the
# minifying NEAREST blits agree exactly.  The magnifying NEAREST blits differ only on viewport column 105 and row 78, where the sample
# position is exactly a texel edge (u = 80, v = 60): llvmpipe's interpolated texcoord falls just below it and picks the texel before.
# LINEAR differs by one (once by two) byte steps: llvmpipe filters with fixed-point weights, R24 with fp32 weights.
FIXTURE_RECORDED = {
    "depth_norm": (0, 0),
    "model": (0, 0),
    "depth_norm_mag": (4887, 1),
    "depth_norm_min": (1269, 1),
    "model_mag": (324, 166),
    "model_min": (0, 0),
    "rgb_mag": (11326, 1),
    "rgb_min": (2733, 1),
    "model_image_mag": (445, 255),
    "model_image_min": (0, 0),
    "rgb_nearest_min": (0, 0),
    "model_image_linear_mag": (10747, 2),
    "rgb_tinted_min": (4131, 1),
}
SOURCES = {0: ("depth_norm", L8), 1: ("model", RGBA8), 2: ("rgba", RGBA8), 3: ("model_rgba", RGBA8)}


def fixture_case(z, name):
    import json

    return json.loads(str(z[name + "__case"]))


def fixture_blit(z, name):
    """the restatement's colour image of a fixture case; the two intermediates come from the FIXTURE, so that each
    stage is compared on its own"""
    c = fixture_case(z, name)
    key, fmt = SOURCES[c["source"]]
    t = R.Target(c["target"][0], c["target"][1], tuple(z["clear"]))
    blit(t, z[key], fmt, c["linear"], c["viewport"], c["color"])
    return t.color


def check_fixture(name, exp, got):
    n, d = fixture_stats(exp, got)
    rn, rd = FIXTURE_RECORDED[name]
    assert n <= rn + 1 and d <= rd, (name, (n, d), "recorded", (rn, rd))
    return n, d


def fixture_stats(exp, got):
    """(mismatching bytes, largest byte difference)"""
    d = np.abs(np.asarray(exp, np.int64) - np.asarray(got, np.int64))
    return int((d != 0).sum()), int(d.max()) if d.size else 0
