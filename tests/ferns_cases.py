"""Crafted key-frame thumbnails for the fern database tests (host only, fixed seeds).

A thumbnail is the triple (RGBA8 image, RGBA32F vertex map, RGBA32F normal map) of W/8 x H/8 pixels that dms_fusion_thumbnails packs into
one block.  Everything here is built from a fern table - an oracle object (oracle/orc_ferns.Ferns: pos, rgbd, num, width, height) - so that
the descriptor of a thumbnail has an EXACT number of valid ferns and differs from another one's in an EXACT number of ferns; every such
count is asserted against the oracle's _encode before the thumbnail is handed out (a count that cannot be placed is an assertion failure).

Whole pixels are flipped, as tests/helpers.py:fern_boundary_thumbnails does: black <-> white changes the three colour bits of every fern on
the pixel unless a threshold is 255; 0.3 m <-> 3.5 m changes the depth bit for every threshold in [400, maxDepth] (300 > d never, 3500 > d
always), so a flipped pixel changes the code of EVERY fern that sits on it; depth 0 invalidates every fern on the pixel.
"""
import numpy as np

BAD = 255
NEAR, FAR = np.float32(0.3), np.float32(3.5)
W, H = 320, 240  # thumbnails 40 x 30
K = (264.0, 264.0, 160.0, 120.0)  # fx, fy, cx, cy


def pixel_ferns(o):
    """{(y, x): number of ferns of the table that sit on the pixel}"""
    cnt = {}
    for i in range(o.num):
        p = (int(o.pos[i, 1]), int(o.pos[i, 0]))
        cnt[p] = cnt.get(p, 0) + 1
    return cnt


def _set_depth(o, verts, y, x, z):
    """a vertex of depth z on the ray of thumbnail pixel (x, y) (the verification tracker gets a plane, not a degenerate point)"""
    fx, fy, cx, cy = [np.float32(v) / np.float32(8) for v in (o.fx, o.fy, o.cx, o.cy)]
    z = np.float32(z)
    verts[y, x] = ((np.float32(x) - cx) * z / fx, (np.float32(y) - cy) * z / fy, z, 1.0) if z > 0 else (0, 0, 0, 0)


def base(o):
    """every fern valid: black image, a plane at 0.3 m (depth bit 0 everywhere), normals towards the camera"""
    th, tw = o.height, o.width
    img = np.zeros((th, tw, 4), np.uint8)
    img[..., 3] = 255
    verts = np.zeros((th, tw, 4), np.float32)
    for y in range(th):
        for x in range(tw):
            _set_depth(o, verts, y, x, NEAR)
    norms = np.zeros((th, tw, 4), np.float32)
    norms[..., 2] = -1.0
    codes, good, _ = o._encode(img, verts)
    assert good == o.num and (codes != BAD).all()
    return img, verts, norms


def _pick(cnt, pixels, want, rng, small_first=False):
    """a subset of `pixels` whose fern counts add up to exactly `want` (greedy over a shuffled order; single-fern pixels fill the rest)"""
    order = list(pixels)
    rng.shuffle(order)
    if small_first:
        order.sort(key=lambda p: cnt[p])
    got, left = [], want
    for p in order:
        if left == 0:
            break
        if cnt[p] <= left:
            got.append(p)
            left -= cnt[p]
    assert left == 0, "could not place %d ferns on whole pixels (%d left over)" % (want, left)
    return got


def variant(o, thumb, differ=0, valid=None, seed=0, avoid=()):
    """A thumbnail whose descriptor is valid in exactly `valid` ferns (default: as many as `thumb`'s) and differs from `thumb`'s in exactly
    `differ` of the ferns valid in both.  `avoid`: pixels that must stay as they are.  Returns (thumbnail, flipped pixels, invalidated pixels)."""
    rng = np.random.RandomState(seed)
    cnt = pixel_ferns(o)
    img, verts, norms = [a.copy() for a in thumb]
    c0, g0, _ = o._encode(img, verts)
    valid = g0 if valid is None else valid
    assert 0 <= valid <= g0 and 0 <= differ <= valid
    avoid = set(avoid)
    live = sorted(p for p in cnt if verts[p[0], p[1], 2] > 0 and p not in avoid)
    kept = sum(cnt[p] for p in avoid if p in cnt and verts[p[0], p[1], 2] > 0)
    if valid - kept < (g0 - kept) // 2:  # few survivors: choose the pixels that STAY valid, single-fern pixels first (any `differ` fits on them)
        keep = set(_pick(cnt, live, valid - kept, rng, small_first=True))
        dead = [p for p in live if p not in keep]
    else:
        dead = _pick(cnt, live, g0 - valid, rng)
        keep = set(live) - set(dead)
    for (y, x) in dead:
        _set_depth(o, verts, y, x, 0)
    flip = _pick(cnt, sorted(keep), differ, rng, small_first=valid < 16)
    for (y, x) in flip:
        img[y, x, :3] = 255 - img[y, x, :3]
        _set_depth(o, verts, y, x, FAR if verts[y, x, 2] == NEAR else NEAR)
    c1, g1, _ = o._encode(img, verts)
    both = (c0 != BAD) & (c1 != BAD)
    assert g1 == valid, (g1, valid)
    assert int(both.sum()) == valid and int((c0 != c1)[both].sum()) == differ, (int(both.sum()), int((c0 != c1)[both].sum()), differ)
    return (img, verts, norms), flip, dead


def depth_at_threshold(o, thumb, fern=0):
    """Two copies of `thumb` whose pixel under fern `fern` has the LARGEST float32 depth z with int(float32(z) * float32(1000)) == d (the
    fern's depth threshold: bit 0, d > d is false) and the next float32 above it (the product truncates to d + 1: bit 1): pins both the
    truncation and the strict comparison of f2i_rz(v.z * 1000.0f) > d."""
    d = int(o.rgbd[fern, 3])
    mm = lambda z: int(np.float32(z) * np.float32(1000.0))
    z = np.float32((d + 1) / 1000.0)
    while mm(z) > d:
        z = np.nextafter(z, np.float32(0))
    hi = np.nextafter(z, np.float32(10))
    assert mm(z) == d and mm(hi) == d + 1, (d, z, hi)
    y, x = int(o.pos[fern, 1]), int(o.pos[fern, 0])
    out = []
    for zz, bit in ((z, 0), (hi, 1)):
        img, verts, norms = [a.copy() for a in thumb]
        _set_depth(o, verts, y, x, zz)
        assert verts[y, x, 2] == zz
        codes, _, _ = o._encode(img, verts)
        assert codes[fern] != BAD and (codes[fern] & 1) == bit
        out.append((img, verts, norms))
    return out


def pose(seed):
    """a rigid pose with no exactly representable entries (its bits must survive the database and the re-posing of a merge)"""
    r = np.random.RandomState(1000 + seed)
    q = r.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = r.uniform(-3, 3, 3)
    return T.astype(np.float32)


def upsample(thumb):
    """full-resolution textures whose NEAREST thumbnails (ratio 8: texel 8 j + 4) are `thumb`"""
    return tuple(np.ascontiguousarray(np.repeat(np.repeat(t, 8, axis=0), 8, axis=1)) for t in thumb)


def pack(thumb):
    """the block of dms_fusion_thumbnails: RGBA8 image (padded to 16 bytes) | RGBA32F vertex | RGBA32F normal"""
    img, verts, norms = thumb
    ib = img.reshape(-1).view(np.uint8)
    pad = (-ib.size) % 16
    return np.concatenate([ib, np.zeros(pad, np.uint8), verts.reshape(-1).view(np.uint8), norms.reshape(-1).view(np.uint8)])


# ---- the scenarios: each returns plain data (thumbnails, poses, times); tests/test_ferns_cases_cpu.py asserts on the CPU what
# tests/test_ferns_database_gpu.py relies on, both from these same constructors ---------------------------------------------------------

TIE_ZERO_IDS = (10, 205, 516)  # one thumbnail stored three times: blocks 2 / 51 / 129, waves 2 / 1 / 0, fused rounds 1 / 25 / (beyond 512)
TIE_PAIR_IDS = (13, 330)       # two different frames at the same non-zero dissimilarity: blocks 3 / 82, waves 1 / 2, fused rounds 1 / 41
TIE_PAIR_K = 10
BIG_STOPS = (1, 3, 4, 5, 8, 9, 511, 512, 513, 519)  # 519 = 4 * 129 + 3
BIG_TARGETS = (0, 3, 4, 7, 8, 255, 256, 507, 508, 511, 512)


def big_sequence(o):
    """The large database: BIG_STOPS[-1] thumbnails, all stored (threshold -1).  Returns dict(frames=[(thumb, pose, time)], tie_zero=thumb,
    tie_pair_query=thumb, queries={stop: [(thumb, target id or None)]})."""
    n = BIG_STOPS[-1]
    b = base(o)
    tie_zero = variant(o, b, differ=240, seed=9001)[0]
    tq, _, _ = variant(o, b, differ=235, seed=9002)
    t1, flip1, _ = variant(o, tq, differ=TIE_PAIR_K, seed=9003)
    t2, flip2, _ = variant(o, tq, differ=TIE_PAIR_K, seed=9004, avoid=flip1)
    assert not set(flip1) & set(flip2)
    frames = []
    for j in range(n):
        if j in TIE_ZERO_IDS:
            t = tie_zero
        elif j in TIE_PAIR_IDS:
            t = t1 if j == TIE_PAIR_IDS[0] else t2
        else:  # (every 7th frame with fewer valid ferns: the good counts of the database differ)
            t = variant(o, b, differ=150 + (j * 37) % 90, valid=(300 + j % 50) if j % 7 == 3 else None, seed=j)[0]
        frames.append((t, pose(j), 10 + j))
    queries, near = {}, {}
    for stop in BIG_STOPS:
        ids = sorted(set(t for t in BIG_TARGETS + tuple(range(stop - 8, stop)) if 0 <= t < stop) - set(TIE_ZERO_IDS) - set(TIE_PAIR_IDS))
        if stop >= 8:
            assert set(t % 8 for t in ids) == set(range(8))
        for t in ids:
            if t not in near:
                near[t] = variant(o, frames[t][0], differ=3, seed=20000 + t)[0]
        qs = [(near[t], t) for t in ids]
        qs += [(tie_zero, None), (tq, None)]
        queries[stop] = qs
    return dict(frames=frames, tie_zero=tie_zero, tie_pair_query=tq, queries=queries)


def age_gate_case(o):
    """query + three stored frames at dissimilarity 2 / 4 / 6 of 500 whose ages at time 1000 are 299, 300 and 301, and two far frames"""
    b = base(o)
    q = variant(o, b, differ=200, seed=31)[0]
    frames = [(variant(o, b, differ=230, seed=32)[0], pose(40), 990),
              (variant(o, q, differ=2, seed=33)[0], pose(41), 701),
              (variant(o, q, differ=4, seed=34)[0], pose(42), 700),
              (variant(o, b, differ=220, seed=35)[0], pose(43), 995),
              (variant(o, q, differ=6, seed=36)[0], pose(44), 699)]
    return dict(query=q, frames=frames, time=1000, time_none=900)


def valid_count_cases(o):
    """[(name, stored thumbnail, [query thumbnails], (g, gj))] with one stored frame each, and the query without a valid fern"""
    b = base(o)
    s7 = variant(o, b, differ=0, valid=7, seed=51)[0]
    s3 = variant(o, b, differ=0, valid=3, seed=52)[0]
    cases = [("500 against 7", s7, [b, variant(o, b, differ=120, seed=53)[0]], (500, 7)),
             ("7 against 500", b, [s7, variant(o, s7, differ=3, seed=54)[0]], (7, 500)),
             ("1 against 500", b, [variant(o, b, differ=0, valid=1, seed=55)[0], variant(o, b, differ=1, valid=1, seed=56)[0]], (1, 500)),
             ("3 against 3", s3, [variant(o, s3, differ=2, seed=57)[0], variant(o, s3, differ=1, seed=58)[0]], (3, 3))]
    empty = variant(o, b, differ=0, valid=0, seed=59)[0]
    return cases, empty


def threshold_cases(o):
    """[(threshold, stored, frame exactly AT the threshold, frame one fern above it)]: 250 / 500 = 0.5 and 150 / 500 = float32(0.3)"""
    b = base(o)
    out = []
    for k, thr, s in ((250, np.float32(0.5), 61), (150, np.float32(0.3), 63)):
        out.append((thr, b, variant(o, b, differ=k, seed=s)[0], variant(o, b, differ=k + 1, seed=s + 1)[0]))
    return out


def other_table_thumbs(o):
    """five crafted thumbnails for a table of any size"""
    b = base(o)
    return [b, variant(o, b, differ=min(o.num, 3), seed=1)[0], variant(o, b, differ=0, valid=o.num // 2, seed=2)[0]] + depth_at_threshold(o, b, fern=o.num - 1)


def full_case(o, n=8):
    b = base(o)
    return [(variant(o, b, differ=200 + j, seed=70 + j)[0], pose(70 + j), 5 + j) for j in range(n)]


def merge_case(o_src, o_dst, n_src=130, n_dst=20):
    """destination frames, source frames (a third near a destination frame, a third near the source frame before them, the rest new), the
    transform and the threshold of a merge that rejects some"""
    b = base(o_dst)
    dst = [(variant(o_dst, b, differ=150 + 3 * j, seed=300 + j)[0], pose(300 + j), 100 + j) for j in range(n_dst)]
    src = []
    for j in range(n_src):
        if j % 3 == 0:
            t = variant(o_dst, dst[j % n_dst][0], differ=20 + j % 60, seed=400 + j)[0]  # 0.04 .. 0.16 from a destination frame
        elif j % 3 == 1 and j > 1:
            t = variant(o_dst, src[j - 2][0], differ=35 + j % 30, valid=480 if j % 2 else None, seed=400 + j)[0]
        else:
            t = variant(o_dst, b, differ=160 + j, seed=400 + j)[0]
        src.append((t, pose(400 + j), 1000 + j))
    T = pose(999)
    return dict(dst=dst, src=src, T=T, threshold=np.float32(0.1))


def mixed_sequence(o):
    """about 60 (thumbnail, pose, time, threshold) offers that contain every kind of case: duplicates, ties, few / one / no valid ferns,
    thresholds met exactly, old and young frames"""
    b = base(o)
    seq = []
    add = lambda t, thr: seq.append((t, pose(len(seq)), 37 * len(seq) % 1000, np.float32(thr)))
    add(b, 0.1)
    for j in range(1, 12):
        add(variant(o, b, differ=150 + 7 * j, seed=500 + j)[0], 0.1)
    add(seq[3][0], 0.1)  # a duplicate: rejected at +0
    add(seq[3][0], -1.0)  # stored all the same: a tie at +0
    cases, empty = valid_count_cases(o)
    for _, s, qs, _ in cases:
        add(s, -1.0)
        for q in qs:
            add(q, 0.2)
    add(empty, -1.0)
    add(variant(o, b, differ=0, valid=1, seed=155)[0], -1.0)  # a stored frame with one valid fern
    tq = variant(o, b, differ=235, seed=9002)[0]
    t1, f1, _ = variant(o, tq, differ=TIE_PAIR_K, seed=9003)
    add(t1, -1.0)
    add(variant(o, tq, differ=TIE_PAIR_K, seed=9004, avoid=f1)[0], -1.0)
    add(tq, 0.02)  # exactly at 10 / 500 = 0.02f against both: rejected
    add(tq, 0.0199)
    for thr, _, at, above in threshold_cases(o):
        add(at, float(thr))
        add(above, float(thr))
    ag = age_gate_case(o)
    for t, _, _ in ag["frames"]:
        add(t, 0.05)
    add(ag["query"], 0.003)
    while len(seq) < 60:
        j = len(seq)
        add(variant(o, seq[j % 12][0], differ=(11 * j) % 70, valid=500 - (j % 5) * 60, seed=600 + j)[0], 0.07)
    return seq
