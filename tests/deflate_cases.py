"""Inputs for the block deflate encoder (csrc/deflate_core.hpp), from fixed seeds, shared by tests/test_deflate_cpu.py and
tests/test_deflate_gpu.py.  Small on purpose; B is the encoder's block size as the library exports it."""
import functools

import numpy as np

VGA = "bench_depth_640x480"


def block_size():
    from densemonoslam_amd import ingest

    return ingest.deflate_blocks_block_size()


def _rows_like_the_row_above(rng, rows, width):
    """rows of `width` bytes that each repeat the row above with a few changed pixels"""
    out = [rng.integers(0, 256, width, dtype=np.uint8)]
    for _ in range(rows - 1):
        r = out[-1].copy()
        r[rng.integers(0, width, 5)] = rng.integers(0, 256, 5, dtype=np.uint8)
        out.append(r)
    return np.concatenate(out).tobytes()


def _distinct_within_32k(n):
    """bytes whose every 3-byte string is new within any 32 KB: a counter in base 251 interleaved with a byte that no digit takes, so
    nothing can be matched and a block has literals only"""
    k = np.arange((n + 2) // 3, dtype=np.uint32)
    trip = np.stack([k % 251, (k // 251) % 251, np.full(k.size, 255)], 1).astype(np.uint8)
    return trip.reshape(-1)[:n].tobytes()


def _skewed(rng, n):
    """21 byte values with Fibonacci-like frequencies, shuffled: code lengths far from uniform"""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    pool = np.concatenate([np.full(f, 40 + 3 * i, np.uint8) for i, f in enumerate(fib)])
    reps = (n + pool.size - 1) // pool.size
    x = np.tile(pool, reps)[:n]
    rng.shuffle(x)
    return x.tobytes()


def _synth_depth(width, height, K):
    from densemonoslam_amd import synth

    return np.ascontiguousarray(synth.frame(3, width=width, height=height, K=K, noise=True)[0], np.uint16).tobytes()


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, bytes)] in a fixed order"""
    from densemonoslam_amd import synth

    B = block_size()
    rng = np.random.default_rng(20260)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = []
    for n in (1, 2, 3, 4):
        out.append(("len_%d" % n, rnd(n)))
    for name, n in (("random_B-1", B - 1), ("random_B", B), ("random_B+1", B + 1), ("random_3B+17", 3 * B + 17)):
        out.append((name, rnd(n)))
    for n in (257, 258, 259, 260, 2 * B + 5):
        out.append(("run_%d" % n, bytes([0x5a]) * n))
    out.append(("zeros_70001", bytes(70001)))
    out.append(("long_run_u16", np.full(50000, 1234, np.uint16).tobytes() + b"\x07"))
    out.append(("all_distinct", _distinct_within_32k(40000)))
    one = bytearray(_distinct_within_32k(3000))
    one[2000:2012] = one[500:512]  # the only repeat: one match, one distance symbol
    out.append(("one_match", bytes(one)))
    head = rnd(40000 - 32768)
    filler = _distinct_within_32k(32768 - len(head))
    out.append(("repeat_at_32768", head + filler + head))  # 40 000 bytes; the second part repeats the first at distance 32 768
    out.append(("repeat_at_32769", head + filler + b"\xfe" + head[:-1]))  # ... at 32 769, which no match may use
    out.append(("rows_1280", _rows_like_the_row_above(rng, 20, 1280)))
    out.append(("depth_160x120", _synth_depth(160, 120, tuple(v / 4.0 for v in synth.K_640))))
    blocky = rng.integers(400, 4000, (6, 8)).astype(np.uint16).repeat(8, 0).repeat(8, 1)
    out.append(("blocky_64x48", np.ascontiguousarray(blocky).tobytes()))
    out.append(("skewed_21_values", _skewed(rng, 3 * B + 100)))
    out.append((VGA, _synth_depth(640, 480, synth.K_640)))
    return out


def by_name(name):
    return dict(cases())[name]
