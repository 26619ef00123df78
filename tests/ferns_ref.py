"""Vectorised restatement of the reference's fern database (Ferns.cpp addFrame / findFrame / blockHDAware / consume) for databases of
hundreds of frames, where the inverted-list walk of oracle/orc_ferns.py is too slow.  tests/test_ferns_cases_cpu.py holds it to
orc_ferns.Ferns decision for decision and bit for bit; the GPU tests compare the library with it.  Host only."""
import numpy as np

from oracle.orc_ferns import _mul44

BAD = 255
FLT_MAX = np.float32(3.402823466e+38)


class RefDB:
    def __init__(self, o, capacity=None):
        """o: the table (an orc_ferns.Ferns, or anything with num, pos[num][2] = (x, y), rgbd[num][4])"""
        self.num = int(o.num)
        self.px, self.py = np.asarray(o.pos[:, 0], np.int64), np.asarray(o.pos[:, 1], np.int64)
        self.rgbd = np.asarray(o.rgbd, np.int32)
        self.capacity = capacity
        self.codes = np.zeros((0, self.num), np.uint8)
        self.good, self.time, self.pose, self.thumbs = [], [], [], []
        self.dropped = 0

    def __len__(self):
        return len(self.good)

    def encode(self, thumb):
        """(codes[num], good count) - Ferns.cpp:208-233"""
        img, verts = thumb[0], thumb[1]
        z = verts[self.py, self.px, 2].astype(np.float32)
        pix = img[self.py, self.px].astype(np.int32)
        mm = (z * np.float32(1000.0)).astype(np.float32).astype(np.int64)  # (int)(z * 1000.0f): truncation
        code = ((pix[:, 0] > self.rgbd[:, 0]) << 3) | ((pix[:, 1] > self.rgbd[:, 1]) << 2) | ((pix[:, 2] > self.rgbd[:, 2]) << 1) | (mm > self.rgbd[:, 3])
        ok = z > 0
        return np.where(ok, code, BAD).astype(np.uint8), int(ok.sum())

    def dissimilarities(self, q, g):
        """float32 dissimilarity of descriptor (q, g) against every stored frame; NaN where min(g, gj) == 0"""
        co = ((self.codes == q[None, :]) & (q[None, :] != BAD)).sum(1)
        maxCo = np.minimum(g, np.asarray(self.good, np.int64)).astype(np.float32)
        with np.errstate(all="ignore"):
            return ((maxCo - co.astype(np.float32)).astype(np.float32) / maxCo).astype(np.float32)

    def search(self, q, g, time, interMap):
        """(id or -1, float32 dissimilarity): skip NaN, the first strictly smaller, frames older than 300 unless interMap (Ferns.cpp:327-339)"""
        if len(self) == 0:
            return -1, FLT_MAX
        d = self.dissimilarities(q, g)
        ok = ~np.isnan(d)
        if not interMap:
            ok &= (time - np.asarray(self.time, np.int64)) > 300
        if not ok.any():
            return -1, FLT_MAX
        i = int(np.argmin(np.where(ok, d, np.float32(np.inf))))  # argmin: the FIRST of equal minima
        return i, np.float32(d[i])

    def hd(self, q, i):
        """blockHDAware's operands against stored frame i: (codes valid in both, of those equal)"""
        c = self.codes[i]
        both = (q != BAD) & (c != BAD)
        return int(both.sum()), int((q == c)[both].sum())

    def row(self, q, g, time, interMap):
        """the hit row of dms_ferns_search_blocks_hd: {id, dissimilarity bits, valid in both, equal} or {-1, 0, 0, 0}"""
        i, d = self.search(q, g, time, interMap)
        if i < 0:
            return [-1, 0, 0, 0]
        return [i, int(np.array([d], np.float32).view(np.int32)[0])] + list(self.hd(q, i))

    def hit(self, q, g, time, interMap):
        i, _ = self.search(q, g, time, interMap)
        if i < 0:
            return False
        c, e = self.hd(q, i)
        with np.errstate(all="ignore"):
            return bool(float(np.float32(e) / np.float32(c)) > 0.3)

    def add(self, thumb, pose, time, threshold):
        """addFrame's decision (Ferns.cpp:235-275): slot, -1 (rejected) or -2 (wanted, but the database is at its capacity)"""
        q, g = self.encode(thumb)
        minimum = FLT_MAX
        if g > 0 and len(self):
            d = self.dissimilarities(q, g)
            d = d[~np.isnan(d)]
            if d.size and d.min() < minimum:
                minimum = np.float32(d.min())
        self.last_minimum = minimum
        if not ((minimum > np.float32(threshold) or len(self) == 0) and g > 0):
            return -1
        if self.capacity is not None and len(self) >= self.capacity:
            self.dropped += 1
            return -2
        self.codes = np.concatenate([self.codes, q[None, :]])
        self.good.append(g)
        self.time.append(int(time))
        self.pose.append(np.array(pose, np.float32).reshape(4, 4))
        self.thumbs.append(thumb)
        return len(self) - 1

    def consume(self, other, T, threshold, count=None):
        """Ferns.cpp:160-168: every frame of `other`, re-posed, through add (re-encoded with this table)"""
        added = 0
        for j in range(len(other) if count is None else count):
            added += int(self.add(other.thumbs[j], _mul44(T, other.pose[j]), other.time[j], threshold) >= 0)
        return added
